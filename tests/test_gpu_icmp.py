"""GPU tests of the ICMP responder (nfcs_icmp_respond_device) through the C ABI. Every test compares the device's
message arrays, statuses and totals with Icmp.respond_host (arrays equal) and the arena byte for byte with the
arena the host walk leaves, bytes outside the emitted messages included; the message arrays carry guard entries
past cap that must stay as they were. The fixture (tests/golden/icmp_ref.npz) is also compared with what the
reference sent, and runs through lookup -> respond -> plan -> enqueue -> update in one stream."""
import numpy as np
import pytest

import netflow_amd as nf
from icmp_common import (FAR, FILL, HOST, ME, assert_layout, assert_same_respond, device_respond, fixture_fib, fixture_icmp,
                         icmp_fixture, ipv4, messages_of, pack_with_region, region_for, round_up, run_of, small_tables)

pytestmark = pytest.mark.gpu

T = nf.ICMP_TILE_PKTS


@pytest.fixture(scope="module")
def fx(engine):
    z, frames = icmp_fixture()
    with fixture_fib(z) as fib, fixture_icmp(z) as icmp:
        fib.upload(engine)
        icmp.upload(engine)
        yield z, frames, fib, icmp


def check(engine, icmp, fib, ingress, arena, msg_base, msg_align, desc, verdict, cap, ip_id=None, what=""):
    """Device against host: the arrays, the statuses, the totals, the whole arena. Returns the host's output and
    the arena it left."""
    host_arena = arena.copy()
    want = icmp.respond_host(fib, ingress, host_arena, msg_base, msg_align, desc, verdict, cap, ip_id=ip_id)
    got = device_respond(engine, icmp, fib, ingress, arena, msg_base, msg_align, desc, verdict, cap, ip_id=ip_id)
    assert_same_respond(got, want, what)
    bad = np.flatnonzero(got["arena"] != host_arena)
    assert len(bad) == 0, f"{what}the arena differs from the host walk's at {bad[:8].tolist()} (msg_base {msg_base})"
    return want, host_arena


def tiled(run, idx):
    return ([run["frames"][i] for i in idx], run["verdict"][idx], run["ip_id"][idx])


# ---- the fixture ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("msg_align", [16, 64, 128])
@pytest.mark.parametrize("r", [0, 1])
def test_fixture_device_equals_host_equals_reference(engine, fx, r, msg_align):
    z, frames, fib, icmp = fx
    run = run_of(z, frames, r)
    arena, desc, msg_base = pack_with_region(run["frames"], 16, region_for(run["sent"], msg_align) + 256, msg_align)
    cap = len(run["sent"]) + 5
    want, after = check(engine, icmp, fib, run["ingress"], arena, msg_base, msg_align, desc, run["verdict"], cap, run["ip_id"])
    assert messages_of(after, want) == run["sent"]
    assert np.array_equal(want["status"], run["status"])
    assert_layout(want, after, msg_base, msg_align, cap, arena)


# ---- sizes around the machinery --------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, T - 1, T, T + 1, 3 * T + 7])
def test_sizes_around_the_tile(engine, fx, n):
    """The fixture tiled: messages crossing tile boundaries; at 3 tiles and more a tile without any message and a
    tile of nothing but messages come first."""
    z, frames, fib, icmp = fx
    run = run_of(z, frames, 0)
    nf0 = len(run["frames"])
    is_msg = np.zeros(nf0, bool)
    is_msg[[i for i, _, _ in run["sent"]]] = True
    if n >= 3 * T:
        none, only = np.flatnonzero(~is_msg), np.flatnonzero(is_msg & (np.array([len(f) for f in run["frames"]]) < 300))
        idx = np.concatenate([none[np.arange(T) % len(none)], only[np.arange(T) % len(only)], (np.arange(n - 2 * T) * 7 + 3) % nf0])
    else:
        idx = (np.arange(n) * 7 + 1) % nf0 if n > 1 else np.array([run["sent"][0][0]])
    fr, verdict, ip_id = tiled(run, idx)
    region = sum(round_up(len(m), 16) for i, _, m in run["sent"]) * (n // nf0 + 2) + T * 400
    arena, desc, msg_base = pack_with_region(fr, 16, region, 16)
    want, after = check(engine, icmp, fib, 0, arena, msg_base, 16, desc, verdict, n, ip_id)
    t = want["totals"]
    assert int(t["messages"]) == int(t["messages_needed"]) == int(is_msg[idx].sum()) >= 1
    by_src = {i: (p, m) for i, p, m in run["sent"]}
    assert messages_of(after, want) == [(k,) + by_src[int(i)] for k, i in enumerate(idx) if is_msg[i]]
    if n >= 3 * T:
        src = want["msg_src"][:int(t["messages"])]
        assert not (src < T).any() and (np.bincount(src // T)[1] == T)


def test_every_cut_of_a_burst(engine, fx):
    """cap and the region cut at every position of a 40-message burst: the prefix is emitted, the totals say what
    was needed, the bytes before msg_base, the bytes of the region behind the prefix and the entries past cap stay
    as they were."""
    z, frames, fib, icmp = fx
    run = run_of(z, frames, 0)
    take = [i for i, _, m in run["sent"] if len(m) < 400][:40]
    sub, verdict, ip_id = tiled(run, np.array(take))
    by_src = {i: (p, m) for i, p, m in run["sent"]}
    full = [(k,) + by_src[i] for k, i in enumerate(take)]
    slots = np.cumsum([round_up(len(m), 64) for _, _, m in full])
    for cut in range(41):
        for by_cap in (True, False):
            region = int(slots[-1]) if by_cap else (int(slots[cut - 1]) if cut else 0) + (48 if cut < 40 else 0)
            cap = cut if by_cap else 40
            arena, desc, msg_base = pack_with_region(sub, 16, region, 64)
            want, after = check(engine, icmp, fib, 0, arena, msg_base, 64, desc, verdict, cap, ip_id, f"cut {cut} {by_cap}: ")
            assert messages_of(after, want) == full[:cut], (cut, by_cap)
            assert int(want["totals"]["messages_needed"]) == 40 and int(want["totals"]["msg_bytes_needed"]) == int(slots[-1])
            assert (want["status"][cut:] == nf.ICMP_ST_OVERFLOW).all()
            assert_layout(want, after, msg_base, 64, cap, arena)


@pytest.mark.parametrize("k", range(8))
def test_source_frames_at_each_line_offset(engine, fx, k):
    """Every source frame starts 16 k bytes into a 128-byte line: the shifted 16-byte loads start at every dword of
    a line, and those of a frame's last chunks end at the line's end."""
    z, frames, fib, icmp = fx
    run = run_of(z, frames, 0)
    idx = np.arange(k % 3, len(run["frames"]), 3)
    fr, verdict, ip_id = tiled(run, idx)
    arena, desc, msg_base = pack_with_region(fr, 128, 1 << 17, 16, lead=16 * k)
    assert (desc["off16"] % 8 == k).all()
    want, after = check(engine, icmp, fib, 0, arena, msg_base, 16, desc, verdict, len(fr), ip_id)
    assert int(want["totals"]["messages"]) == int(want["totals"]["messages_needed"]) >= 60


def test_last_source_frame_ends_at_the_end_of_the_arena(engine, fx):
    """An empty region (msg_base == arena_bytes) right behind the last frame's last chunk: nothing is emitted and
    the statuses say OVERFLOW; then the same burst with a region of exactly the bytes needed."""
    z, frames, fib, icmp = fx
    run = run_of(z, frames, 0)
    picked = run["sent"][-6:] + run["sent"][:30:5]  # errors, then echo requests: the last frame is a request with a payload
    idx = np.array([i for i, _, _ in picked])
    fr, verdict, ip_id = tiled(run, idx)
    assert run["status"][idx[-1]] == nf.ICMP_ST_ECHO_REPLY and len(fr[-1]) > 100
    need = sum(round_up(len(by), 16) for i, _, by in picked)
    for region in (0, need):
        arena, desc, msg_base = pack_with_region(fr, 16, region, 16)
        want, _ = check(engine, icmp, fib, 0, arena, msg_base, 16, desc, verdict, 12, ip_id)
        assert int(want["totals"]["messages"]) == (12 if region else 0) and int(want["totals"]["messages_needed"]) == 12


def test_requests_with_long_payloads(engine):
    """Replies of several row passes (1,536 message bytes each), the longest reply there is (65,549 bytes), odd
    and even lengths, and the two statuses of frames the reference would mishandle."""
    import struct
    rng = np.random.default_rng(11)
    fr = []
    for p in (1494, 1495, 1536 - 42, 1536 - 41, 3 * 1536 - 42, 3 * 1536 - 41, 3 * 1536 - 43, 9000, 9001, 65506, 65507):
        fr.append(ipv4(HOST, ME, 1, struct.pack(">BBHHH", 8, 0, 0, p, 2) + rng.integers(0, 256, p, dtype=np.uint8).tobytes()))
    fr.append(ipv4(HOST, ME, 1, bytes(65515), ihl=1, tl=65535, ident=0x0800))
    fr.append(ipv4(HOST, FAR, 17, bytes(30), ttl=1, ihl=15)[:14 + 40])
    verdict = np.array([nf.RT_LOCAL] * 12 + [nf.RT_TTL_EXPIRED], np.uint8)
    fib, icmp = small_tables()
    with fib, icmp:
        fib.upload(engine)
        icmp.upload(engine)
        arena, desc, msg_base = pack_with_region(fr, 16, 1 << 18, 16)
        want, after = check(engine, icmp, fib, 1, arena, msg_base, 16, desc, verdict, 16)
    assert want["status"].tolist() == [nf.ICMP_ST_ECHO_REPLY] * 11 + [nf.ICMP_ST_TOO_LONG, nf.ICMP_ST_OOB]
    import oracle
    for _, _, m in messages_of(after, want):
        assert oracle.update_frame(m)[0] == m


def test_message_region_past_32_gib(engine, fx):
    """One arena with msg_base past 32 GiB: the message descriptors carry off16 >= 2^31 and every slot offset needs
    36 bits. Sources at the arena's start and past 32 GiB in turn. Compared with the host walk over the same burst in
    a small arena, the descriptors moved by the distance between the two regions."""
    z, frames, fib, icmp = fx
    run = run_of(z, frames, 0)
    base = (32 << 30) + 8192
    try:
        big = engine.alloc(base + (8 << 20))
    except nf.NfcsError:
        pytest.skip("the device lacks the memory for an arena past 32 GiB")
    try:
        n = 2 * T + 77
        idx = (np.arange(n) * 5 + 2) % len(run["frames"])
        fr, verdict, ip_id = tiled(run, idx)
        lo_arena, lo_desc, lo_end = pack_with_region(fr[0::2], 16, 0, 128)
        hi_arena, hi_desc, hi_end = pack_with_region(fr[1::2], 16, 0, 128)
        assert lo_end < (2 << 20) and hi_end < (2 << 20)
        # the device's arena: low frames at 0, high frames at base, the region behind them
        desc = np.zeros(n, nf.DESC_DTYPE)
        desc[0::2], desc[1::2] = lo_desc, hi_desc
        desc["off16"][1::2] += base // 16
        msg_base = base + (2 << 20)
        region = 4 << 20
        big.upload(lo_arena, 0)
        big.upload(hi_arena, base)
        big.upload(np.full(region + 4096, FILL, np.uint8), msg_base - 2048)
        # the host's arena: low frames at 0, high frames at 2 MiB, the region at 4 MiB
        small = np.full((4 << 20) + region, FILL, np.uint8)
        small[:lo_end], small[2 << 20:(2 << 20) + hi_end] = lo_arena, hi_arena
        sdesc = desc.copy()
        sdesc["off16"][1::2] = hi_desc["off16"] + (2 << 20) // 16
        want = icmp.respond_host(fib, 0, small, 4 << 20, 128, sdesc, verdict, n, ip_id=ip_id)
        m = int(want["totals"]["messages"])
        assert m == int(want["totals"]["messages_needed"]) > 500
        up = lambda a, dt: engine.alloc(max(np.asarray(a).nbytes, 16)).upload(np.ascontiguousarray(a, dt))  # noqa: E731
        d_desc, d_v, d_id = up(desc, nf.DESC_DTYPE), up(verdict, np.uint8), up(ip_id, np.uint16)
        d_md, d_mp, d_ms, d_st, d_tot = engine.alloc(8 * n), engine.alloc(4 * n), engine.alloc(4 * n), engine.alloc(n), engine.alloc(32)
        arena_bytes = msg_base + region
        engine.icmp_respond_device(icmp, fib, 0, big, arena_bytes, msg_base, 128, d_desc, n, d_v, n, d_md, d_mp, d_ms, d_tot,
                                   ip_id=d_id, status=d_st)
        engine.sync()
        md = d_md.download(nf.DESC_DTYPE, n)
        shift = (msg_base - (4 << 20)) // 16
        assert (md["off16"][:m] >= 1 << 31).all()
        assert np.array_equal(md["off16"][:m].astype(np.int64) - shift, want["msg_desc"]["off16"][:m].astype(np.int64))
        assert np.array_equal(md["len"], want["msg_desc"]["len"]) and (md["off16"][m:] == 0).all()
        assert np.array_equal(d_mp.download(np.uint32, n), want["msg_port"])
        assert np.array_equal(d_ms.download(np.uint32, n), want["msg_src"])
        assert np.array_equal(d_st.download(np.uint8, n), want["status"])
        tot = d_tot.download(nf.ICMP_TOTALS_DTYPE, 1)[0]
        assert all(int(tot[k]) == int(want["totals"][k]) for k in nf.ICMP_TOTALS_DTYPE.names)
        got = big.download(np.uint8, region + 4096, msg_base - 2048)
        assert (got[:2048] == FILL).all() and (got[2048 + region:] == FILL).all(), "a store outside the region"
        assert np.array_equal(got[2048:2048 + region], small[4 << 20:]), "the region differs from the host walk's"
        assert np.array_equal(big.download(np.uint8, lo_end, 0), lo_arena) and np.array_equal(big.download(np.uint8, hi_end, base), hi_arena)
        for b in (d_desc, d_v, d_id, d_md, d_mp, d_ms, d_st, d_tot):
            b.free()
    finally:
        big.free()


# ---- the chain -------------------------------------------------------------------------------------------

def test_chain_lookup_respond_plan_enqueue_update(engine, fx):
    """nfcs_route_lookup_device -> respond -> plan -> enqueue on one stream with no host step, over all cap entries
    (the padding is inert), then nfcs_update_device over the message list: the plan edits no message
    (NFCS_VLAN_NOP), every emitted message is enqueued on its port, and update_checksums() over the messages
    changes no byte, so the checksums the stage wrote are the reference's."""
    z, frames, fib, icmp = fx
    run = run_of(z, frames, 0)
    n, cap = len(run["frames"]), 256
    arena, desc, msg_base = pack_with_region(run["frames"], 16, 1 << 17, 16)
    with nf.Egress() as eg:
        for p in range(int(z["num_ports"])):
            eg.set_port(p, type=nf.L2_TRUNK if p & 1 else nf.L2_ACCESS, tag_native=bool(p & 2), native_vlan=1 + p,
                        num_queues=1 + p % 8, max_queue_depth=1000)
        eg.commit().upload(engine)
        keys = eg.keys()[1]
        up = lambda a, dt: engine.alloc(max(np.asarray(a).nbytes, 16)).upload(np.ascontiguousarray(a, dt))  # noqa: E731
        d_arena, d_desc, d_id = up(arena, np.uint8), up(desc, nf.DESC_DTYPE), up(run["ip_id"], np.uint16)
        d_nh, d_v = engine.alloc(4 * n), engine.alloc(n)
        d_md, d_mp, d_ms, d_tot = engine.alloc(8 * cap), engine.alloc(4 * cap), engine.alloc(4 * cap), engine.alloc(32)
        d_port, d_ops, d_queue = engine.alloc(4 * cap), engine.alloc(4 * cap), engine.alloc(cap)
        d_depth = up(np.zeros(keys, np.uint32), np.uint32)
        d_order, d_ks, d_res = engine.alloc(4 * cap), engine.alloc(4 * (keys + 1)), engine.alloc(cap)
        d_ust = engine.alloc(cap)
        engine.route_lookup_device(fib, d_arena, msg_base, d_desc, n, d_nh, verdict=d_v)
        engine.icmp_respond_device(icmp, fib, 0, d_arena, arena.nbytes, msg_base, 16, d_desc, n, d_v, cap, d_md, d_mp, d_ms,
                                   d_tot, ip_id=d_id)
        engine.egress_plan_device(eg, d_arena, arena.nbytes, d_md, cap, d_port, d_ops, d_queue, l2_port=d_mp)
        engine.egress_enqueue_device(eg, d_port, d_queue, cap, d_depth, d_order, d_ks, result=d_res)
        engine.sync()
        built = d_arena.download(np.uint8, arena.nbytes)
        engine.update_device(d_arena, arena.nbytes, d_md, cap, d_ust)
        engine.sync()
        v = d_v.download(np.uint8, n)
        ours = np.isin(run["verdict"], (nf.RT_LOCAL, nf.RT_TTL_EXPIRED, nf.RT_NO_ROUTE))
        assert np.array_equal(v[ours], run["verdict"][ours]) and not np.isin(v[~ours], (3, 4, 5)).any()
        out = {"msg_desc": d_md.download(nf.DESC_DTYPE, cap), "msg_port": d_mp.download(np.uint32, cap),
               "msg_src": d_ms.download(np.uint32, cap), "totals": d_tot.download(nf.ICMP_TOTALS_DTYPE, 1)[0]}
        m = int(out["totals"]["messages"])
        assert messages_of(built, out) == run["sent"] and m == len(run["sent"]) < cap
        assert (d_ops.download(np.uint32, cap) == nf.VLAN_NOP).all()
        assert np.array_equal(d_port.download(np.uint32, cap), out["msg_port"])
        res = d_res.download(np.uint8, cap)
        assert (res[:m] == nf.EQ_ENQUEUED).all() and (res[m:] == nf.EQ_SKIP).all()
        order, ks = d_order.download(np.uint32, cap), d_ks.download(np.uint32, keys + 1)
        assert int(ks[keys]) == m
        for key in range(keys):  # within one (port, queue) the messages keep the reference's order
            seq = order[int(ks[key]):int(ks[key + 1])]
            assert (np.diff(seq.astype(np.int64)) > 0).all() and (out["msg_port"][seq] == key // nf.QOS_MAX_QUEUES).all()
        assert (d_ust.download(np.uint8, cap)[:m] == nf.ST_V4_ICMP).all()
        assert np.array_equal(d_arena.download(np.uint8, arena.nbytes), built), "update_checksums() changed a message"


def test_not_uploaded_and_n_zero(engine, fx):
    z, frames, fib, icmp = fx
    L = nf.lib()
    buf = engine.alloc(4096).upload(np.zeros(4096, np.uint8))  # one packet of length 0, verdict FORWARD
    b = buf.ptr

    def args(base=2048, n=1):
        if n == 0:
            return (b, 4096, base, 16, None, 0, None, None, 0, None, None, None, None, None, None)
        return (b, 4096, base, 16, b, n, b + 64, None, 1, b + 128, b + 256, b + 320, None, b + 384, None)

    with fixture_icmp(z) as raw:  # committed, never uploaded
        assert L.nfcs_icmp_respond_device(engine.ctx, raw.ptr, fib.ptr, 0, *args()) == -1
        with nf.Icmp() as fresh:
            assert L.nfcs_icmp_upload(engine.ctx, fresh.ptr) == -1  # before commit
        raw.upload(engine)
        assert L.nfcs_icmp_respond_device(engine.ctx, raw.ptr, fib.ptr, 0, *args()) == 0
        raw.set_ports_up([], 8)  # invalidates the commit, not the upload
        assert L.nfcs_icmp_respond_device(engine.ctx, raw.ptr, fib.ptr, 0, *args()) == 0
        assert L.nfcs_icmp_upload(engine.ctx, raw.ptr) == -1
        with nf.Fib() as nofib:
            assert L.nfcs_icmp_respond_device(engine.ctx, raw.ptr, nofib.ptr, 0, *args()) == -1
        engine.sync()
    assert L.nfcs_icmp_respond_device(engine.ctx, icmp.ptr, fib.ptr, 0, *args(n=0)) == 0
    assert L.nfcs_icmp_respond_device(engine.ctx, icmp.ptr, fib.ptr, 0, *args(base=2040)) == -1
    assert L.nfcs_icmp_respond_device(engine.ctx, icmp.ptr, fib.ptr, 0, *args(base=4112)) == -1
    engine.sync()
    got = buf.download(np.uint8, 4096)
    assert (got[128:136] == 0).all() and (got[256:260] == 0xFF).all() and (got[320:324] == 0xFF).all()  # one inert entry
    assert not got[384:416].any() and not got[416:].any()
    buf.free()
