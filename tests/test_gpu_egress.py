"""GPU tests of the egress stage (nfcs_egress_plan_device, nfcs_egress_enqueue_device) through the C ABI:
against the reference's results on the fixture burst (tests/golden/egress_ref.npz), against the CPU forms
of the same tables (Egress.plan_host, Egress.enqueue_host) at the sizes where the kernels change path, the
optional arguments, the upload rules, and the whole pipeline in one stream."""
import numpy as np
import pytest

import netflow_amd as nf
import oracle
from acl_common import eval_host, rule
from egress_common import Q, assert_same, egress_fixture, fixture_egress, fixture_want, plan_host
from l2_common import decide_host as l2_decide_host
from l2_common import entries_of
from route_common import FWD_DSTS, decide_host as route_decide_host
from route_common import fixture_fib, route_fixture

pytestmark = pytest.mark.gpu

T = nf.EGRESS_TILE_PKTS
FILL = 0xEE


@pytest.fixture(scope="module")
def fx():
    z, frames = egress_fixture()
    return z, frames, fixture_want(z)


def pack_at(frames, starts):
    """Frames at the given byte offsets (multiples of 16, ascending, not overlapping)."""
    desc = np.zeros(len(frames), dtype=nf.DESC_DTYPE)
    end = 0
    for i, (f, o) in enumerate(zip(frames, starts)):
        assert o % 16 == 0 and o >= end
        desc[i] = (o // 16, len(f))
        end = o + (len(f) + 15) // 16 * 16
    arena = np.zeros(max(end, 16), dtype=np.uint8)
    for f, o in zip(frames, starts):
        arena[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    return arena, desc


def filled(engine, nbytes):
    return engine.alloc(nbytes + 16).upload(np.full(nbytes + 16, FILL, np.uint8))


def up(engine, a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return engine.alloc(max(a.nbytes, 16)).upload(a)


def run_plan(engine, eg, arena, desc, l3=None, st=None, l2=None, upload=True):
    """(port, ops, queue) from the device. Every output has one element more than n, which must stay as
    it was; the frames must stay as they were."""
    n = len(desc)
    if upload:
        eg.upload(engine)
    d_arena, d_desc = up(engine, arena, np.uint8), up(engine, desc, nf.DESC_DTYPE)
    d_port, d_ops, d_queue = filled(engine, 4 * (n + 1)), filled(engine, 4 * (n + 1)), filled(engine, n + 1)
    engine.egress_plan_device(eg, d_arena, arena.nbytes, d_desc, n, d_port, d_ops, d_queue,
                              l3_port=None if l3 is None else up(engine, l3, np.uint32),
                              fwd_status=None if st is None else up(engine, st, np.uint8),
                              l2_port=None if l2 is None else up(engine, l2, np.uint32))
    engine.sync()
    assert np.array_equal(d_arena.download(np.uint8, arena.nbytes), arena), "the plan wrote into the frames"
    port, ops, queue = d_port.download(np.uint32, n + 1), d_ops.download(np.uint32, n + 1), d_queue.download(np.uint8, n + 1)
    assert port[n] == 0xEEEEEEEE and ops[n] == 0xEEEEEEEE and queue[n] == FILL, "a store past element n"
    return port[:n].copy(), ops[:n].copy(), queue[:n].copy()


def run_enqueue(engine, eg, port, queue, depth, want=("result", "key_dropped"), upload=True, d_depth=None):
    """The device's enqueue as the dict Egress.enqueue_host returns (optional outputs not in `want` are
    passed as NULL and come back as None), plus "order_buf": all n entries of d_order, and "d_depth"."""
    n, keys = len(port), eg.keys()[1]
    if upload:
        eg.upload(engine)
    d_port, d_queue = up(engine, port, np.uint32), up(engine, queue, np.uint8)
    if d_depth is None:
        d_depth = engine.alloc(4 * keys + 32).upload(np.concatenate([np.asarray(depth, np.uint32),
                                                                      np.full(4, 0xEEEEEEEE, np.uint32)]))
    d_order, d_ks = filled(engine, 4 * (n + 1)), filled(engine, 4 * (keys + 2))
    d_res = filled(engine, n + 1) if "result" in want else None
    d_drop = filled(engine, 4 * (keys + 1)) if "key_dropped" in want else None
    engine.egress_enqueue_device(eg, d_port, d_queue, n, d_depth, d_order, d_ks, result=d_res, key_dropped=d_drop)
    engine.sync()
    ks = d_ks.download(np.uint32, keys + 2)
    order = d_order.download(np.uint32, n + 1)
    dep = d_depth.download(np.uint32, keys + 1)
    assert ks[keys + 1] == 0xEEEEEEEE and order[n] == 0xEEEEEEEE and dep[keys] == 0xEEEEEEEE, "a store past the end"
    total = int(ks[keys])
    assert total <= n and (order[total:n] == 0xEEEEEEEE).all(), "entries past the total must stay as they were"
    out = {"key_start": ks[:keys + 1].copy(), "order": order[:total].copy(), "depth": dep[:keys].copy(),
           "order_buf": order[:n].copy(), "d_depth": d_depth, "result": None, "key_dropped": None}
    if d_res is not None:
        r = d_res.download(np.uint8, n + 1)
        assert r[n] == FILL
        out["result"] = r[:n].copy()
    if d_drop is not None:
        d = d_drop.download(np.uint32, keys + 1)
        assert d[keys] == 0xEEEEEEEE
        out["key_dropped"] = d[:keys].copy()
    return out


# ---- the plan kernel --------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["align16", "align128", "late112"])
@pytest.mark.parametrize("source", ["l2", "l3"])
def test_plan_fixture_matches_reference(engine, fx, layout, source):
    """16-byte and 128-byte frame starts, and frames starting 112 bytes into a 128-byte line, so that
    bytes 12..19 straddle two lines."""
    z, frames, want = fx
    if layout == "late112":
        arena, desc = pack_at(frames, [256 * i + 112 for i in range(len(frames))])
    else:
        arena, desc = oracle.pack_frames(frames, align=16 if layout == "align16" else 128)
    with fixture_egress(z) as eg:
        port, ops, queue = run_plan(engine, eg, arena, desc, **{source: z["port"]})
    assert np.array_equal(port, z["port"]) and np.array_equal(ops, want["ops"]) and np.array_equal(queue, want["queue"])


def test_plan_port_selection_and_the_status_gate(engine, fx):
    """l3 wins where it is not IF_NONE, and with fwd_status only where ST_FLAG_FWD is set; else l2; else none.
    Each optional input NULL in turn."""
    z, frames, _ = fx
    n = len(frames)
    arena, desc = oracle.pack_frames(frames)
    rng = np.random.default_rng(11)
    l3 = rng.integers(0, 12, n).astype(np.uint32)
    l3[rng.random(n) < 0.4] = nf.IF_NONE
    l2 = rng.integers(0, 12, n).astype(np.uint32)
    l2[rng.random(n) < 0.4] = nf.IF_NONE
    st = rng.integers(0, 128, n).astype(np.uint8)
    st[rng.random(n) < 0.5] |= nf.ST_FLAG_FWD
    fwd = (st & nf.ST_FLAG_FWD) != 0
    none = np.full(n, nf.IF_NONE, np.uint32)
    cases = {
        "l3 only": (dict(l3=l3), l3),
        "l2 only": (dict(l2=l2), l2),
        "l3 + l2": (dict(l3=l3, l2=l2), np.where(l3 != nf.IF_NONE, l3, l2)),
        "l3 + status": (dict(l3=l3, st=st), np.where(fwd, l3, none)),
        "all three": (dict(l3=l3, st=st, l2=l2), np.where(fwd & (l3 != nf.IF_NONE), l3, l2)),
    }
    with fixture_egress(z) as eg:
        for name, (args, want_port) in cases.items():
            port, ops, queue = run_plan(engine, eg, arena, desc, **args)
            assert np.array_equal(port, want_port), name
            h_ops, h_queue = plan_host(eg, want_port, frames)
            assert np.array_equal(ops, h_ops) and np.array_equal(queue, h_queue), name
            gone = want_port == nf.IF_NONE
            assert gone.sum() > 50 and (ops[gone] == nf.VLAN_NOP).all() and (queue[gone] == nf.QUEUE_NONE).all(), name


def test_plan_argument_errors(engine, fx):
    z, _, _ = fx
    buf = engine.alloc(256)
    L = nf.lib()
    with fixture_egress(z) as eg:
        call = lambda l3, st, l2, port=buf.ptr, ops=buf.ptr, queue=buf.ptr, n=1, e=eg: L.nfcs_egress_plan_device(  # noqa: E731
            engine.ctx, e.ptr, buf.ptr, 256, buf.ptr, n, l3, st, l2, port, ops, queue, None)
        assert call(buf.ptr, None, None) == -1          # not uploaded
        eg.upload(engine)
        assert call(None, None, None) == -1             # no port array at all
        assert call(None, buf.ptr, buf.ptr) == -1       # a status without the L3 ports
        assert call(buf.ptr, None, None, port=None) == -1
        assert call(buf.ptr, None, None, ops=None) == -1
        assert call(buf.ptr, None, None, queue=None) == -1
        assert call(buf.ptr + 2, None, None) == -1      # misaligned ports
        assert call(None, None, buf.ptr, n=0, port=None, ops=None, queue=None) == 0  # n == 0: nothing is looked at
        engine.sync()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_plan_sizes_and_bad_descriptors(engine, fx, n):
    """Wave and workgroup edges on slices of the fixture, with the first and the last descriptor (and one in
    the middle) reaching outside the arena: no port, no edit, no queue for those, their neighbours as before."""
    z, frames, want = fx
    sel = [(7 * i) % len(frames) for i in range(n)]
    arena, desc = oracle.pack_frames([frames[i] for i in sel])
    bad = desc.copy()
    bad[0]["off16"] = arena.nbytes // 16  # starts at the arena's end
    bad[0]["len"] = max(int(bad[0]["len"]), 1)
    bad[n - 1]["len"] = arena.nbytes - int(bad[n - 1]["off16"]) * 16 + 1  # one byte past it
    bad[n // 2]["off16"] = 0xFFFFFFFF
    w_port, w_ops, w_queue = z["port"][sel].copy(), want["ops"][sel].copy(), want["queue"][sel].copy()
    with fixture_egress(z) as eg:
        port, ops, queue = run_plan(engine, eg, arena, desc, l2=z["port"][sel])
        assert np.array_equal(port, w_port) and np.array_equal(ops, w_ops) and np.array_equal(queue, w_queue)
        port, ops, queue = run_plan(engine, eg, arena, bad, l2=z["port"][sel], upload=False)
    for i in {0, n - 1, n // 2}:
        w_port[i], w_ops[i], w_queue[i] = nf.IF_NONE, nf.VLAN_NOP, nf.QUEUE_NONE
    assert np.array_equal(port, w_port) and np.array_equal(ops, w_ops) and np.array_equal(queue, w_queue)


# ---- plan -> VLAN -> enqueue on the fixture -----------------------------------------------------------

def test_fixture_plan_vlan_enqueue_match_reference(engine, fx):
    """The three calls in one stream with no host step: the frame bytes and lengths after the edit, d_order
    per key, d_key_start, d_key_dropped, d_result and d_depth all equal the reference's."""
    z, frames, want = fx
    n, keys = len(frames), want["keys"]
    arena, desc = oracle.pack_frames(frames, align=128)
    with fixture_egress(z) as eg:
        eg.upload(engine)
        d_arena, d_desc = up(engine, arena, np.uint8), up(engine, desc, nf.DESC_DTYPE)
        d_l2 = up(engine, z["port"], np.uint32)
        d_port, d_ops, d_queue = engine.alloc(4 * n), engine.alloc(4 * n), engine.alloc(n)
        d_depth = up(engine, want["depth0"], np.uint32)
        d_order, d_ks, d_res, d_drop = filled(engine, 4 * n), engine.alloc(4 * (keys + 1)), engine.alloc(n), engine.alloc(4 * keys)
        engine.egress_plan_device(eg, d_arena, arena.nbytes, d_desc, n, d_port, d_ops, d_queue, l2_port=d_l2)
        engine.vlan_device(d_arena, arena.nbytes, d_desc, n, d_ops, 0, None, 128)
        engine.egress_enqueue_device(eg, d_port, d_queue, n, d_depth, d_order, d_ks, result=d_res, key_dropped=d_drop)
        engine.sync()
        out, desc_out = d_arena.download(np.uint8, arena.nbytes), d_desc.download(nf.DESC_DTYPE, n)
        ks = d_ks.download(np.uint32, keys + 1)
        got = {"key_start": ks, "order": d_order.download(np.uint32, n)[:int(ks[keys])], "depth": d_depth.download(np.uint32, keys),
               "result": d_res.download(np.uint8, n), "key_dropped": d_drop.download(np.uint32, keys)}
    assert np.array_equal(desc_out["len"], z["lens_out"]) and np.array_equal(desc_out["off16"], desc["off16"])
    for i in range(n):
        o, ln = int(desc["off16"][i]) * 16, int(z["lens_out"][i])
        assert np.array_equal(out[o:o + ln], z["frames_out"][i, :ln]), f"frame {i} differs from the reference's"
    assert_same(got, want)


# ---- the enqueue kernels against enqueue_host ---------------------------------------------------------

@pytest.fixture(scope="module")
def big_table():
    """1,024 ports x 8 queues, with depths that drop some of a cycling burst."""
    eg = nf.Egress()
    for p in range(1024):
        eg.set_port(p, num_queues=8, max_queue_depth=1 + p % 3)
    yield eg.commit()
    eg.close()


@pytest.fixture(scope="module")
def small_table():
    """Ports 0..11: port 5 never set, port 7 without QoS, queue counts 1..8, small and large depths."""
    eg = nf.Egress()
    for p in range(12):
        if p != 5:
            eg.set_port(p, has_qos=p != 7, num_queues=1 + p % 8, max_queue_depth=(3, 40, 1000, 100000)[p % 4])
    yield eg.commit()
    eg.close()


SIZES = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 3 * T + 65]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", ["one_key", "cycle_all", "two_keys", "random"])
def test_enqueue_matches_host(engine, big_table, small_table, n, pattern):
    rng = np.random.default_rng(n)
    i = np.arange(n)
    if pattern == "one_key":
        eg, port, queue = small_table, np.full(n, 3), np.full(n, 2)          # depth 100000: everything fits
    elif pattern == "cycle_all":
        eg, port, queue = big_table, (i // 8) % 1024, i % 8                   # every (port, queue) in turn
    elif pattern == "two_keys":
        eg, port, queue = small_table, np.where(i % 2 == 0, 1, 9), np.where(i % 2 == 0, 0, 1)  # depths 40
    else:
        eg = small_table
        port = rng.integers(0, 14, n).astype(np.uint32)                       # 12, 13: past the table
        port[rng.random(n) < 0.1] = nf.IF_NONE
        queue = rng.integers(0, 10, n)                                        # bad queues among them
    keys = eg.keys()[1]
    depth = rng.integers(0, 3, keys).astype(np.uint32)
    want = eg.enqueue_host(port, queue, depth)
    got = run_enqueue(engine, eg, port, queue, depth)
    assert_same(got, want, f"{pattern} n={n}: ")
    if pattern == "random" and n >= T:
        assert set(want["result"].tolist()) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("case", ["room_0", "room_exact", "room_in_second_tile", "room_on_tile_edge", "depth_above_cap"])
def test_enqueue_room_cases(engine, case):
    """All packets of 3T + 65 on one key (port 2, queue 1) but every seventh on another (port 0, queue 0,
    always room), so the key's count per tile is not the tile size."""
    n = 3 * T + 65
    i = np.arange(n)
    port, queue = np.where(i % 7 == 2, 0, 2).astype(np.uint32), np.where(i % 7 == 2, 0, 1).astype(np.uint8)
    mine = np.flatnonzero(port == 2)
    count = len(mine)
    cap, start = {
        "room_0": (50, 50),
        "room_exact": (count + 9, 9),
        "room_in_second_tile": (int((mine < T).sum()) + 100, 0),   # the 100th packet of the key in tile 1 is the last in
        "room_on_tile_edge": (int((mine < 2 * T).sum()), 0),       # packet 2T - 1, tile 1's last, is the last in
        "depth_above_cap": (50, 0xFFFFFFF0),                       # must not underflow
    }[case]
    room = max(0, cap - start)
    with nf.Egress().set_port(0, num_queues=1, max_queue_depth=n).set_port(2, num_queues=2, max_queue_depth=cap).commit() as eg:
        keys = eg.keys()[1]
        depth = np.zeros(keys, np.uint32)
        depth[2 * Q + 1] = start
        want = eg.enqueue_host(port, queue, depth)
        got = run_enqueue(engine, eg, port, queue, depth)
    assert_same(got, want, case + ": ")
    k = 2 * Q + 1
    assert got["key_start"][k + 1] - got["key_start"][k] == min(room, count) and got["key_dropped"][k] == count - min(room, count)
    assert np.array_equal(got["order"][got["key_start"][k]:got["key_start"][k + 1]], mine[:min(room, count)])
    if case == "room_on_tile_edge":
        assert got["result"][mine[room - 1]] == nf.EQ_ENQUEUED and mine[room - 1] == 2 * T - 1
        assert got["result"][mine[room]] == nf.EQ_DROP_FULL and mine[room] == 2 * T


def test_enqueue_second_call_chains_on_the_first_calls_depth(engine, small_table):
    rng = np.random.default_rng(77)
    n = 2 * T + 1
    eg = small_table
    keys = eg.keys()[1]
    port, queue = rng.integers(0, 12, n).astype(np.uint32), rng.integers(0, 4, n).astype(np.uint8)
    depth = np.zeros(keys, np.uint32)
    want1 = eg.enqueue_host(port, queue, depth)
    want2 = eg.enqueue_host(port[::-1], queue[::-1], want1["depth"])
    got1 = run_enqueue(engine, eg, port, queue, depth)
    got2 = run_enqueue(engine, eg, port[::-1], queue[::-1], None, upload=False, d_depth=got1["d_depth"])
    assert_same(got1, want1, "first: ")
    assert_same(got2, want2, "second: ")
    assert want2["key_dropped"].sum() > want1["key_dropped"].sum() > 0


@pytest.mark.parametrize("left_out", ["result", "key_dropped", "both"])
def test_enqueue_optional_outputs_left_out(engine, small_table, left_out):
    rng = np.random.default_rng(5)
    n = T + 65
    port, queue = rng.integers(0, 13, n).astype(np.uint32), rng.integers(0, 9, n).astype(np.uint8)
    depth = np.zeros(small_table.keys()[1], np.uint32)
    want = small_table.enqueue_host(port, queue, depth)
    keep = tuple(k for k in ("result", "key_dropped") if k != left_out and left_out != "both")
    got = run_enqueue(engine, small_table, port, queue, depth, want=keep)
    assert [got[k] is not None for k in ("result", "key_dropped")] == [k in keep for k in ("result", "key_dropped")]
    assert_same(got, want)


def test_enqueue_is_deterministic(engine, big_table):
    rng = np.random.default_rng(9)
    n = 3 * T + 65
    port, queue = rng.integers(0, 64, n).astype(np.uint32), rng.integers(0, 8, n).astype(np.uint8)
    depth = np.zeros(big_table.keys()[1], np.uint32)
    a = run_enqueue(engine, big_table, port, queue, depth)
    b = run_enqueue(engine, big_table, port, queue, depth, upload=False)
    assert np.array_equal(a["order_buf"], b["order_buf"]) and np.array_equal(a["result"], b["result"])
    assert (a["result"] == nf.EQ_DROP_FULL).sum() > n // 2  # depths 1..3 over 512 keys


def test_enqueue_upload_rules_arguments_and_no_packets(engine):
    L = nf.lib()
    buf = engine.alloc(4096)
    with nf.Egress().set_port(1, num_queues=2, max_queue_depth=1).commit() as eg:
        call = lambda port=buf.ptr, queue=buf.ptr, n=1, depth=buf.ptr, order=buf.ptr, ks=buf.ptr: \
            L.nfcs_egress_enqueue_device(engine.ctx, eg.ptr, port, queue, n, depth, None, order, ks, None, None)  # noqa: E731
        assert call() == -1  # not uploaded
        eg.upload(engine)
        for missing in ("port", "queue", "depth", "order", "ks"):
            assert call(**{missing: None}) == -1, missing
        assert call(depth=buf.ptr + 2) == -1
        assert call(n=0, port=None, queue=None, depth=None, order=None, ks=None) == 0  # n == 0: nothing is written
        port, queue, depth = [1, 1, 1, 0], [1, 1, 0, 0], np.zeros(16, np.uint32)
        old = eg.enqueue_host(port, queue, depth)
        assert old["result"].tolist() == [nf.EQ_ENQUEUED, nf.EQ_DROP_FULL, nf.EQ_ENQUEUED, nf.EQ_DROP_NO_CONFIG]
        assert_same(run_enqueue(engine, eg, port, queue, depth, upload=False), old)
        eg.set_port(1, num_queues=2, max_queue_depth=2)  # invalidates the commit, not the upload
        with pytest.raises(nf.NfcsError):
            eg.keys()
        eg.commit()
        assert_same(run_enqueue(engine, eg, port, queue, depth, upload=False), old)  # committed, not yet uploaded
        new = eg.enqueue_host(port, queue, depth)
        assert new["result"].tolist() == [nf.EQ_ENQUEUED, nf.EQ_ENQUEUED, nf.EQ_ENQUEUED, nf.EQ_DROP_NO_CONFIG]
        assert_same(run_enqueue(engine, eg, port, queue, depth), new)
    with nf.Egress().commit() as none:  # no port set: zero keys
        got = run_enqueue(engine, none, [3, nf.IF_NONE, 0], [0, 0, 0], np.zeros(0, np.uint32))
        assert got["result"].tolist() == [nf.EQ_DROP_NO_CONFIG, nf.EQ_SKIP, nf.EQ_DROP_NO_CONFIG]
        assert got["key_start"].tolist() == [0]


# ---- the whole pipeline -------------------------------------------------------------------------------

def host_order(a: str) -> int:
    return int.from_bytes(bytes(int(x) for x in a.split(".")), "big")


def test_whole_pipeline_in_one_stream(engine):
    """route lookup -> ACL -> forward -> L2 lookup -> plan -> VLAN -> enqueue: seven calls on one stream with
    no host step between them, on a slice of the route fixture's frames, against the oracle and the host
    functions chained on the CPU."""
    z, frames = route_fixture()
    frames = frames[:600]
    arena, desc = oracle.pack_frames(frames, align=128)
    n = len(desc)
    rules = np.concatenate([rule(nf.ACL_DENY, dst_ip=host_order(FWD_DSTS[0])), rule(nf.ACL_PERMIT)])
    with fixture_fib(z, "a") as fib, nf.Acl().set_rules(rules).commit() as acl, nf.Fdb() as fdb, nf.Egress() as eg:
        want_rt, want_nh, want_if = route_decide_host(fib, frames)
        l2_frames = [f for f, v in zip(frames, want_rt) if v == nf.RT_NOT_IPV4 and len(f) >= 14]
        macs = np.unique(np.array([np.frombuffer(f[:6], np.uint8) for f in l2_frames[::2]]), axis=0)
        fdb.set_entries(entries_of(macs, np.ones(len(macs)), 1 + np.arange(len(macs)) % 3))
        for p in range(4):
            fdb.set_port(p, native_vlan=1)
        fdb.commit()
        ifs = sorted({int(x) for x in want_if if x != nf.IF_NONE} | {1, 2, 3})
        for k, p in enumerate(ifs):  # the egress ports: those the routes and the FDB name, shallow queues
            eg.set_port(p, type=(nf.L2_ACCESS, nf.L2_TRUNK)[k % 2], native_vlan=1, num_queues=(4, 8, 3)[k % 3],
                        max_queue_depth=(6, 25, 1000)[k % 3])
        eg.commit()
        keys = eg.keys()[1]
        # the CPU chain
        want_action, _, _ = eval_host(acl, frames)
        masked = np.where(want_action == nf.ACL_PERMIT, want_nh, nf.NH_NONE).astype(np.uint32)
        nht = fib.nexthops_host()
        ref, rdesc = arena.copy(), desc.copy()
        rst = oracle.l3_forward_batch(ref, rdesc, masked, nht.view(np.uint8).reshape(-1, 12))
        l2 = l2_decide_host(fdb, 0, frames)
        l2_port = np.where(want_rt == nf.RT_NOT_IPV4, l2[1], nf.IF_NONE).astype(np.uint32)
        fwd = (rst & nf.ST_FLAG_FWD) != 0
        want_port = np.where(fwd & (want_if != nf.IF_NONE), want_if, l2_port).astype(np.uint32)
        after_fwd = oracle.unpack_frames(ref, rdesc)
        want_ops, want_queue = plan_host(eg, want_port, after_fwd)
        want_queue[want_port == nf.IF_NONE] = nf.QUEUE_NONE
        oracle.vlan_batch(ref, rdesc, want_ops, None, cap_all=128)
        want = eg.enqueue_host(want_port, want_queue, np.zeros(keys, np.uint32))
        assert fwd.sum() > n // 5 and (l2_port != nf.IF_NONE).sum() >= 10 and (want_port == nf.IF_NONE).sum() > 20
        assert ((want_action != nf.ACL_PERMIT) & (want_nh != nf.NH_NONE)).sum() >= 5  # the ACL takes packets away
        assert (want["result"] == nf.EQ_DROP_FULL).sum() > 10 and (want["result"] == nf.EQ_ENQUEUED).sum() > 50
        # the device chain
        for obj in (fib, acl, fdb, eg):
            obj.upload(engine)
        d_tab, tab_n = fib.nexthops()
        d_arena, d_desc = up(engine, arena, np.uint8), up(engine, desc, nf.DESC_DTYPE)
        d_nh, d_if, d_rt, d_act, d_st = (engine.alloc(4 * n), engine.alloc(4 * n), engine.alloc(n), engine.alloc(n),
                                         engine.alloc(n))
        d_l2, d_port, d_ops, d_queue = engine.alloc(4 * n), engine.alloc(4 * n), engine.alloc(4 * n), engine.alloc(n)
        d_depth = up(engine, np.zeros(keys, np.uint32), np.uint32)
        d_order, d_ks, d_res, d_drop = engine.alloc(4 * n), engine.alloc(4 * (keys + 1)), engine.alloc(n), engine.alloc(4 * keys)
        engine.route_lookup_device(fib, d_arena, arena.nbytes, d_desc, n, d_nh, egress_if=d_if, verdict=d_rt)
        engine.acl_eval_device(acl, d_arena, arena.nbytes, d_desc, n, d_act, nh=d_nh)
        engine.l3_forward_device(d_arena, arena.nbytes, d_desc, d_nh, n, d_tab, tab_n, d_st)
        engine.l2_lookup_device(fdb, 0, d_arena, arena.nbytes, d_desc, n, d_l2, rt_verdict=d_rt)
        engine.egress_plan_device(eg, d_arena, arena.nbytes, d_desc, n, d_port, d_ops, d_queue, l3_port=d_if,
                                  fwd_status=d_st, l2_port=d_l2)
        engine.vlan_device(d_arena, arena.nbytes, d_desc, n, d_ops, 0, None, 128)
        engine.egress_enqueue_device(eg, d_port, d_queue, n, d_depth, d_order, d_ks, result=d_res, key_dropped=d_drop)
        engine.sync()
        ks = d_ks.download(np.uint32, keys + 1)
        got = {"key_start": ks, "order": d_order.download(np.uint32, n)[:int(ks[keys])], "depth": d_depth.download(np.uint32, keys),
               "result": d_res.download(np.uint8, n), "key_dropped": d_drop.download(np.uint32, keys)}
        port, ops, queue = d_port.download(np.uint32, n), d_ops.download(np.uint32, n), d_queue.download(np.uint8, n)
        out, desc_out = d_arena.download(np.uint8, arena.nbytes), d_desc.download(nf.DESC_DTYPE, n)
    assert np.array_equal(port, want_port) and np.array_equal(ops, want_ops) and np.array_equal(queue, want_queue)
    assert np.array_equal(desc_out, rdesc) and np.array_equal(out, ref)
    assert_same(got, want)
