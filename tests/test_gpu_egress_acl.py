"""GPU tests of the egress ACLs (nfcs_egress_acl_device) through the C ABI. Every run compares the device's
d_port, d_action, d_rule, d_redirect and counters with AclSet.egress_acl_host (arrays equal), checks canary
entries behind every output array, and asserts that the arena is byte for byte what was uploaded; the tests
then hold the host's answer against what their inputs were built to give. The fixture
(tests/golden/egress_acl_ref.npz) is checked against the reference directly, and runs through plan -> VLAN ->
egress ACL -> enqueue -> TX-queue append -> dequeue in one stream against the reference's dequeue record."""
import itertools

import numpy as np
import pytest

import netflow_amd as nf
from acl_common import rule
from egress_acl_common import (FILL, NONE, Fixture, crc64, marked_lists, model_per_list, pack, src_of, udp_frame,
                               want_marked)

pytestmark = pytest.mark.gpu

EE4, EE8 = 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE
GUARD = 256  # canary bytes behind arena_bytes
EINVAL = -1
A3 = (nf.ACL_DENY, nf.ACL_REDIRECT, nf.ACL_PERMIT)


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def up(engine, a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return engine.alloc(max(a.nbytes, 16)).upload(a)


def filled(engine, nbytes):
    return engine.alloc(nbytes + 16).upload(np.full(nbytes + 16, FILL, np.uint8))


def run(engine, s, arena, desc, port, counters=None, rule_out=True, redirect_out=True, upload=True, arena_bytes=None):
    """One call on the device with canaries everywhere; returns the dict AclSet.egress_acl_host returns, plus
    the counters after the call. counters: (denied_pkts, denied_bytes) to start from, or None."""
    n = len(desc)
    arena_bytes = arena.nbytes if arena_bytes is None else arena_bytes
    if upload:
        s.upload(engine)
    d_arena = up(engine, np.concatenate([arena, np.full(GUARD, FILL, np.uint8)]), np.uint8)
    d_desc = up(engine, desc, nf.DESC_DTYPE)
    d_port = up(engine, np.concatenate([np.asarray(port, np.uint32), np.full(4, EE4, np.uint32)]), np.uint32)
    d_action = filled(engine, n)
    d_rule = filled(engine, 4 * n) if rule_out else None
    d_redirect = filled(engine, 4 * n) if redirect_out else None
    d_pk = d_by = None
    if counters is not None:
        ports = len(counters[0])
        d_pk = up(engine, np.concatenate([counters[0], np.full(4, EE4, np.uint32)]), np.uint32)
        d_by = up(engine, np.concatenate([counters[1], np.full(4, EE8, np.uint64)]), np.uint64)
    engine.egress_acl_device(s, d_arena, arena_bytes, d_desc, n, d_port, d_action, d_rule, d_redirect, d_pk, d_by)
    engine.sync()
    out = {}
    back = d_arena.download(np.uint8, arena.nbytes + GUARD)
    assert np.array_equal(back[:arena.nbytes], arena), "the call wrote into the arena"
    assert (back[arena.nbytes:] == FILL).all()
    assert np.array_equal(d_desc.download(nf.DESC_DTYPE, n), desc), "the call wrote a descriptor"
    p = d_port.download(np.uint32, n + 4)
    assert (p[n:] == EE4).all(), "a store past d_port"
    a = d_action.download(np.uint8, n + 16)
    assert (a[n:] == FILL).all(), "a store past d_action"
    out["port"], out["action"] = p[:n].copy(), a[:n].copy()
    for name, buf in (("rule", d_rule), ("redirect", d_redirect)):
        if buf is not None:
            v = buf.download(np.uint32, n + 4)
            assert (v[n:] == EE4).all(), f"a store past d_{name}"
            out[name] = v[:n].copy()
    if counters is not None:
        pk, by = d_pk.download(np.uint32, ports + 4), d_by.download(np.uint64, ports + 4)
        assert (pk[ports:] == EE4).all() and (by[ports:] == EE8).all(), "a store past the counters"
        out["denied_pkts"], out["denied_bytes"] = pk[:ports].copy(), by[:ports].copy()
    return out


def check(engine, s, arena, desc, port, counters=None, what="", **kw):
    """Device against host. Returns the host's output (with its counters when counters are given)."""
    hc = None if counters is None else (counters[0].copy(), counters[1].copy())
    want = s.egress_acl_host(arena[:kw.get("arena_bytes", arena.nbytes)], desc, port, *(hc or ()))
    if hc is not None:
        want["denied_pkts"], want["denied_bytes"] = hc
    got = run(engine, s, arena, desc, port, counters=counters, **kw)
    for k, v in got.items():
        assert np.array_equal(v, want[k]), f"{what}{k} differs from the host's"
    return want


def build_set(lists, ids=None, ports=None):
    """List k gets id ids[k] (default k) and is bound to port ports[k] (default k)."""
    s = nf.AclSet()
    for k, r in enumerate(lists):
        s.set_list(k if ids is None else ids[k], r)
        s.bind_port(k if ports is None else ports[k], k if ids is None else ids[k])
    return s.commit()


# ---- the fixture ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("align", [16, 128])
def test_fixture_matches_the_reference(engine, fx, align):
    arena, desc = pack(fx.frames, align)  # after the fixture's pops, applied on the host
    with fx.aclset() as s:
        ports = s.info()[0]
        want = check(engine, s, arena, desc, fx.port, counters=(np.zeros(ports, np.uint32), np.zeros(ports, np.uint64)))
    z = fx.z
    assert np.array_equal(want["action"], z["action"]) and np.array_equal(want["rule"], z["rule"])
    assert np.array_equal(want["redirect"], z["redirect"])
    assert np.array_equal(want["port"], np.where(z["action"] == nf.ACL_DENY, NONE, fx.port))
    drops, nbytes = fx.denied_counters()
    assert np.array_equal(want["denied_pkts"], drops[:ports]) and np.array_equal(want["denied_bytes"], nbytes[:ports])


# ---- sizes, bad descriptors, packets without a port ---------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_sizes_and_bad_descriptors(engine, n):
    lengths = [1, 3, 4, 5, 9]
    frames = [udp_frame(i % 5) for i in range(n)]
    arena, desc = pack(frames)
    desc = desc.copy()
    port = (np.arange(n) % 5).astype(np.uint32)  # every wave holds every list
    first_bad = desc[0].copy()
    desc[0]["off16"] = arena.nbytes // 16        # the first starts at the arena's end
    if n > 1:
        desc[n - 1]["len"] = 4096                # the last reaches past it
    if n > 2:
        port[1] = NONE
        desc[1] = (0x0FFFFFFF, 0xFFFFFFFF)       # garbage that is not looked at
    with build_set(marked_lists(lengths)) as s:
        want = check(engine, s, arena, desc, port, counters=(np.zeros(5, np.uint32), np.zeros(5, np.uint64)))
    for i in range(n):
        if i == 0 or (i == n - 1 and n > 1):
            exp = (nf.ACL_BAD_DESC, NONE, NONE, NONE)
        elif i == 1 and n > 2:
            exp = (nf.ACL_NO_PORT, NONE, NONE, NONE)
        else:
            a, r, d = want_marked(i % 5, lengths[i % 5])
            exp = (a, r, d, NONE if a == nf.ACL_DENY else i % 5)
        assert (want["action"][i], want["rule"][i], want["redirect"][i], want["port"][i]) == exp, i
    assert first_bad["len"] > 0


# ---- the lists of a wave -----------------------------------------------------------------------------------

@pytest.mark.parametrize("per_wave", [False, True])
@pytest.mark.parametrize("L", [1, 2, 3, 63, 64])
def test_lists_per_wave(engine, L, per_wave):
    """per_wave False: packet i -> port i % L, every wave sees every list (up to 64 scans in a wave);
    True: packet i -> port (i // 64) % L, each wave sees one list."""
    lengths = [(1, 3, 4, 5, 9)[k % 5] for k in range(L)]
    n = 64 * L + 65 if per_wave else max(2 * L + 1, 257)
    idx = np.arange(n)
    port = ((idx // 64) % L if per_wave else idx % L).astype(np.uint32)
    frames = [udp_frame(int(p)) for p in port]
    arena, desc = pack(frames)
    with build_set(marked_lists(lengths)) as s:
        want = check(engine, s, arena, desc, port, counters=(np.zeros(L, np.uint32), np.zeros(L, np.uint64)))
    exp = [want_marked(int(p), lengths[int(p)]) for p in port]
    assert np.array_equal(want["action"], np.array([e[0] for e in exp], np.uint8))
    assert np.array_equal(want["rule"], np.array([e[1] for e in exp], np.uint32))
    assert np.array_equal(want["redirect"], np.array([e[2] for e in exp], np.uint32))
    denied = want["action"] == nf.ACL_DENY
    assert np.array_equal(want["denied_pkts"], np.bincount(port[denied], minlength=L).astype(np.uint32))


def test_exactly_512_rules_with_the_tested_list_last(engine):
    never = rule(action=nf.ACL_DENY, src_ip=0x7F000001)
    filler = np.concatenate([never] * 495 + [rule(action=nf.ACL_DENY, src_ip=src_of(7))])  # would deny frame 7
    last = np.concatenate([never] * 12 + [rule(action=nf.ACL_REDIRECT, redirect_port=33, src_ip=src_of(7))])  # 13 -> 16
    n = 130
    port = (np.arange(n) % 2).astype(np.uint32)
    frames = [udp_frame(7)] * n
    arena, desc = pack(frames)
    with build_set([filler, last], ids=[0, 127]) as s:
        assert s.info() == (2, 2, 512)
        want = check(engine, s, arena, desc, port)
    assert (want["action"][0::2] == nf.ACL_DENY).all() and (want["rule"][0::2] == 495).all()
    assert (want["action"][1::2] == nf.ACL_REDIRECT).all() and (want["rule"][1::2] == 12).all()
    assert (want["redirect"][1::2] == 33).all()


# ---- lanes without a scan ------------------------------------------------------------------------------------

def test_lanes_without_a_scan_among_lanes_with_one(engine):
    deny = rule(action=nf.ACL_DENY, src_ip=src_of(1))
    with nf.AclSet() as s:
        # port 0: a list; 1: empty list; 2: removed list; 3: a list id never set; 4: unbound; 5: a list; 6, 7...: past `ports`
        s.set_list(0, deny).set_list(1, np.zeros(0, nf.ACL_RULE_DTYPE)).set_list(2, deny)
        s.bind_port(0, 0).bind_port(1, 1).bind_port(2, 2).bind_port(3, 99).bind_port(5, 0).remove_list(2).commit()
        assert s.info() == (6, 1, 4)
        kinds = np.array([0, 1, 2, 3, 4, 5, 6, 1023, 70000, NONE], np.uint32)
        n = 257
        port = kinds[np.arange(n) % len(kinds)]
        frames = [udp_frame(1)] * n
        arena, desc = pack(frames)
        want = check(engine, s, arena, desc, port, counters=(np.zeros(6, np.uint32), np.zeros(6, np.uint64)))
        scanned = (port == 0) | (port == 5)
        assert (want["action"][scanned] == nf.ACL_DENY).all() and (want["port"][scanned] == NONE).all()
        assert (want["action"][port == NONE] == nf.ACL_NO_PORT).all()
        rest = ~scanned & (port != NONE)
        assert (want["action"][rest] == nf.ACL_PERMIT).all() and np.array_equal(want["port"][rest], port[rest])
        assert (want["rule"][~scanned] == NONE).all()
        # a whole burst without any scan: garbage descriptors where there is no port, frames never read
        port2 = np.array([1, 2, 3, 4, 6, 1023, 70000, NONE], np.uint32)[np.arange(n) % 8]
        desc2 = desc.copy()
        desc2[port2 == NONE] = (0x0FFFFFFF, 0xFFFFFFFF)
        want = check(engine, s, arena, desc2, port2, counters=(np.zeros(6, np.uint32), np.zeros(6, np.uint64)), upload=False)
        assert ((want["action"] == nf.ACL_PERMIT) | (want["action"] == nf.ACL_NO_PORT)).all()
        assert np.array_equal(want["port"], port2) and not want["denied_pkts"].any()


# ---- late chunks -----------------------------------------------------------------------------------------------

def test_late_chunks_in_a_mixed_wave(engine):
    """IHL 15 puts the UDP ports at bytes 74..77: only the lists that name a port need them, and only some
    packets of a wave carry options."""
    L = 6
    lengths = [3, 4, 5, 9, 1, 3]
    lists = marked_lists(lengths, by_port=True)
    n = 300
    port = (np.arange(n) % L).astype(np.uint32)
    rng = np.random.default_rng(5)
    long_hdr = rng.random(n) < 0.5
    hit = rng.random(n) < 0.7
    frames = [udp_frame(int(p), ihl=15 if lo else 5, dport=7000 + int(p) if h else 9) for p, lo, h in zip(port, long_hdr, hit)]
    frames[5] = frames[5][:76]  # IHL 15 cut inside the ports: udp() absent
    arena, desc = pack(frames)
    with build_set(lists) as s:
        want = check(engine, s, arena, desc, port)
    a, r, d = model_per_list(port, frames, lambda p: lists[p])
    assert np.array_equal(want["action"], a) and np.array_equal(want["rule"], r) and np.array_equal(want["redirect"], d)
    full = hit & (np.arange(n) != 5)
    assert np.array_equal(want["rule"][full], np.array(lengths, np.uint32)[port[full]] - 1)
    assert (want["rule"][~hit] == NONE).all() and long_hdr[full].any() and not long_hdr[full].all()


# ---- d_port in and out ---------------------------------------------------------------------------------------

def test_port_array_in_and_out(engine):
    rng = np.random.default_rng(11)
    L, n = 9, 1000
    lengths = [(1, 3, 4, 5, 9)[k % 5] for k in range(L)]
    port = rng.integers(0, L + 3, n).astype(np.uint32)
    port[rng.random(n) < 0.1] = NONE
    tag = np.where(rng.random(n) < 0.6, np.minimum(port, L - 1), rng.integers(0, L, n))
    frames = [udp_frame(int(t)) for t in tag]
    arena, desc = pack(frames)
    desc = desc.copy()
    bad = rng.random(n) < 0.05
    desc["len"][bad] = 1 << 20
    with build_set(marked_lists(lengths)) as s:
        want = check(engine, s, arena, desc, port)
    gone = (want["action"] == nf.ACL_DENY) | (want["action"] == nf.ACL_BAD_DESC)
    assert gone.any() and (want["action"] == nf.ACL_REDIRECT).any() and (want["action"] == nf.ACL_PERMIT).any()
    assert (want["port"][gone] == NONE).all() and np.array_equal(want["port"][~gone], port[~gone])
    assert np.array_equal(want["action"] == nf.ACL_BAD_DESC, bad & (port != NONE))


# ---- the counters ----------------------------------------------------------------------------------------------

def test_counters_accumulate_over_two_calls(engine):
    rng = np.random.default_rng(12)
    L, n = 7, 700
    lengths = [(1, 3, 4, 5, 9)[k % 5] for k in range(L)]
    with build_set(marked_lists(lengths)) as s:
        pk, by = np.zeros(L, np.uint32), np.zeros(L, np.uint64)
        total_pk, total_by = np.zeros(L, np.int64), np.zeros(L, np.int64)
        for call in range(2):
            port = rng.integers(0, L, n).astype(np.uint32)
            frames = [udp_frame(int(p), length=60 + int(rng.integers(0, 40))) for p in port]
            frames = [f + bytes(int(rng.integers(0, 900))) for f in frames]
            arena, desc = pack(frames)
            want = check(engine, s, arena, desc, port, counters=(pk, by), upload=call == 0)
            denied = want["action"] == nf.ACL_DENY
            total_pk += np.bincount(port[denied], minlength=L)
            total_by += np.bincount(port[denied], weights=desc["len"][denied], minlength=L).astype(np.int64)
            pk, by = want["denied_pkts"], want["denied_bytes"]
            assert np.array_equal(pk, total_pk.astype(np.uint32)) and np.array_equal(by, total_by.astype(np.uint64))
        assert (pk[0::3] > 0).all() and not pk[1::3].any() and not pk[2::3].any()  # lists 0, 3, 6 deny


def test_257_denied_on_one_port_and_sums_past_32_bits(engine):
    n = 257
    frames = [udp_frame(0) + bytes(i) for i in range(n)]
    arena, desc = pack(frames)
    port = np.full(n, 3, np.uint32)
    with nf.AclSet() as s:
        s.set_list(0, rule(action=nf.ACL_DENY)).bind_port(3, 0).commit()
        start = (np.array([0, 0, 0, 0xFFFFFF00], np.uint32), np.array([5, 0, 0, 0xFFFFFFF0], np.uint64))
        want = check(engine, s, arena, desc, port, counters=start)
    assert (want["action"] == nf.ACL_DENY).all() and (want["port"] == NONE).all()
    assert list(want["denied_pkts"]) == [0, 0, 0, (0xFFFFFF00 + n) & 0xFFFFFFFF]
    assert list(want["denied_bytes"]) == [5, 0, 0, 0xFFFFFFF0 + int(desc["len"].sum())]
    assert int(want["denied_bytes"][3]) > 1 << 32


# ---- optional outputs and argument errors ------------------------------------------------------------------------

@pytest.mark.parametrize("rule_out,redirect_out,counters", list(itertools.product([False, True], repeat=3)))
def test_optional_outputs(engine, rule_out, redirect_out, counters):
    lengths = [1, 3, 4, 5, 9]
    n = 200
    port = (np.arange(n) % 5).astype(np.uint32)
    frames = [udp_frame(int(p)) for p in port]
    arena, desc = pack(frames)
    with build_set(marked_lists(lengths)) as s:
        want = check(engine, s, arena, desc, port, rule_out=rule_out, redirect_out=redirect_out,
                     counters=(np.zeros(5, np.uint32), np.zeros(5, np.uint64)) if counters else None)
    assert (want["action"] == np.array(A3, np.uint8)[port % 3]).all()


def test_argument_errors_and_upload_rules(engine):
    L = nf.lib()
    c = engine.ctx
    arena, desc = pack([udp_frame(0)] * 4)
    port = np.zeros(4, np.uint32)
    d_arena, d_desc, d_port = up(engine, arena, np.uint8), up(engine, desc, nf.DESC_DTYPE), up(engine, port, np.uint32)
    d_action, d_pk, d_by = filled(engine, 4), up(engine, np.zeros(4, np.uint32), np.uint32), up(engine, np.zeros(4, np.uint64), np.uint64)

    def call(s, n=4, action=d_action.ptr, pk=None, by=None, port_ptr=d_port.ptr):
        return L.nfcs_egress_acl_device(c, s.ptr, d_arena.ptr, arena.nbytes, d_desc.ptr, n, port_ptr, action, None, None,
                                        pk, by, None)

    with nf.AclSet() as s:
        s.set_list(0, rule(action=nf.ACL_DENY, src_ip=src_of(0))).bind_port(0, 0).commit()
        assert call(s) == EINVAL                                   # committed, not uploaded
        s.upload(engine)
        assert call(s, pk=d_pk.ptr) == EINVAL and call(s, by=d_by.ptr) == EINVAL  # exactly one counter array
        assert call(s, action=None) == EINVAL and call(s, port_ptr=None) == EINVAL
        assert call(s, port_ptr=d_port.ptr + 2) == EINVAL
        assert L.nfcs_egress_acl_device(c, None, d_arena.ptr, arena.nbytes, d_desc.ptr, 4, d_port.ptr, d_action.ptr, None,
                                        None, None, None, None) == EINVAL
        assert L.nfcs_egress_acl_device(c, s.ptr, None, 0, None, 0, None, None, None, None, None, None, None) == 0  # n == 0
        engine.sync()
        assert (d_action.download(np.uint8, 4) == FILL).all()      # nothing ran so far
        # a setter invalidates the commit, not the upload: the device keeps serving the uploaded lists
        s.set_list(0, rule(action=nf.ACL_PERMIT))
        with pytest.raises(nf.NfcsError):
            s.eval_host(0, udp_frame(0))
        with pytest.raises(nf.NfcsError):
            s.upload(engine)                                        # not committed
        got = run(engine, s, arena, desc, port, upload=False)
        assert (got["action"] == nf.ACL_DENY).all() and (got["port"] == NONE).all()
        s.commit().upload(engine)
        got = run(engine, s, arena, desc, port, upload=False)
        assert (got["action"] == nf.ACL_PERMIT).all() and (got["rule"] == 0).all() and (got["port"] == 0).all()


# ---- the whole egress stage ----------------------------------------------------------------------------------------

def test_fixture_whole_stage_in_one_stream(engine, fx):
    """plan -> VLAN -> egress ACL -> enqueue -> TX-queue append -> dequeue of everything on one stream with no
    host step, from the frames as they were before process_egress: per (port, queue) the same packets in the
    same order, with the same lengths and bytes, as the reference dequeued, the same tail drops, the same deny
    counters."""
    z = fx.z
    n = len(fx.frames_in)
    arena, desc = pack(fx.frames_in)
    with fx.aclset() as s, fx.egress() as eg:
        s.upload(engine)
        eg.upload(engine)
        ports, keys = eg.keys()
        aports = s.info()[0]
        with nf.TxQueues(eg, engine) as txq:
            d_arena, d_desc = up(engine, arena, np.uint8), up(engine, desc, nf.DESC_DTYPE)
            d_l2 = up(engine, fx.port, np.uint32)
            d_port, d_ops, d_queue = engine.alloc(4 * n), engine.alloc(4 * n), engine.alloc(n)
            d_action, d_rule = engine.alloc(n), engine.alloc(4 * n)
            d_pk, d_by = up(engine, np.zeros(aports, np.uint32), np.uint32), up(engine, np.zeros(aports, np.uint64), np.uint64)
            d_depth = up(engine, np.zeros(keys, np.uint32), np.uint32)
            d_order, d_ks, d_drop = engine.alloc(4 * n), engine.alloc(4 * (keys + 1)), engine.alloc(4 * keys)
            d_result = engine.alloc(n)
            d_handle = up(engine, np.arange(n, dtype=np.uint64), np.uint64)
            d_tx, d_txq, d_start = engine.alloc(8 * n), engine.alloc(n), engine.alloc(4 * (ports + 1))
            engine.egress_plan_device(eg, d_arena, arena.nbytes, d_desc, n, d_port, d_ops, d_queue, l2_port=d_l2)
            engine.vlan_device(d_arena, arena.nbytes, d_desc, n, d_ops, 0, None, 64)
            engine.egress_acl_device(s, d_arena, arena.nbytes, d_desc, n, d_port, d_action, d_rule, None, d_pk, d_by)
            engine.egress_enqueue_device(eg, d_port, d_queue, n, d_depth, d_order, d_ks, result=d_result, key_dropped=d_drop)
            engine.txq_append_device(txq, d_order, d_ks, d_depth, n, handle=d_handle)
            engine.txq_dequeue_device(txq, d_depth, d_tx, n, d_start, budget_all=1 << 30, tx_queue=d_txq)
            engine.sync()
            action, first = d_action.download(np.uint8, n), d_rule.download(np.uint32, n)
            out, odesc = d_arena.download(np.uint8, arena.nbytes), d_desc.download(nf.DESC_DTYPE, n)
            result, dropped = d_result.download(np.uint8, n), d_drop.download(np.uint32, keys)
            tx, tx_queue, start = d_tx.download(np.uint64, n), d_txq.download(np.uint8, n), d_start.download(np.uint32, ports + 1)
            pk, by, depth = d_pk.download(np.uint32, aports), d_by.download(np.uint64, aports), d_depth.download(np.uint32, keys)
    assert np.array_equal(action, z["action"]) and np.array_equal(first, z["rule"])
    assert np.array_equal(odesc["len"], z["len_out"])
    assert np.array_equal(result == nf.EQ_SKIP, z["action"] == nf.ACL_DENY)
    drops, nbytes = fx.denied_counters()
    assert np.array_equal(pk, drops[:aports]) and np.array_equal(by, nbytes[:aports])
    assert not depth.any()
    queues = {}
    for p in range(ports):
        for j in range(int(start[p]), int(start[p + 1])):
            i = int(tx[j])
            o = int(odesc[i]["off16"]) * 16
            queues.setdefault(p * nf.QOS_MAX_QUEUES + int(tx_queue[j]), []).append(
                (i, int(odesc[i]["len"]), crc64(out[o:o + min(int(odesc[i]["len"]), 64)].tobytes())))
    want_q, want_drops = fx.reference_queues()
    assert queues == want_q
    for k, d in want_drops.items():
        assert int(dropped[k]) == d, k
