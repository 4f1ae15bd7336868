"""GPU tests of the stage counters' stripes and fold: the ingress dispatch's RX counters, the
egress ACL's deny counters and the frame digest, each summed per workgroup into one of S stripes of the context's
counter scratch and folded into the caller's array by a kernel behind the stage's. Every count is compared with the
host definition (Fdb.ingress_dispatch_host, AclSet.egress_acl_host / egress_acl_items_host, oracle.digest) at sizes
around a wave, a workgroup and one full round of stripes (256 * S packets), over chained launches (the stripes are
zero again after each fold), from two streams into one array, and after refused calls. 64 guard bytes lie behind every
device array, the counters included."""
import ctypes

import numpy as np
import pytest

import netflow_amd as nf
import dispatch_common as dc
import oracle
from acl_common import rule
from egress_acl_common import FILL, NONE, pack, udp_frame

pytestmark = pytest.mark.gpu
RX = nf.RX_STATS_DTYPE
S, S_ACL = 64, 16  # nfcs_internal.h kCtStripes, kCtAclStripes
WG = 256           # packets per workgroup of both kernels
NRX = dc.EDGE_PORTS + 2  # the chained test's array: a record for the port the table does not have


@pytest.fixture(scope="module")
def efdb(engine):
    with dc.edge_fdb() as fdb:
        yield fdb.upload(engine)


def edge_burst(n):
    """n frames of dispatch_common's edge list in turn: live, DENY, REDIRECT to a down port and out of range, bad
    descriptors, frames from 0 to 1500 bytes. The stage inputs are the list's own."""
    e = dc.Edges()
    idx = np.arange(n) % e.n
    return e.arena, e.desc[idx], {k: v[idx] for k, v in e.s.items()}, e


def dispatch_launch(engine, g, fdb, ingress, arena, desc, s, d_rx, stream=None):
    n = len(desc)
    engine.ingress_dispatch_device(fdb, ingress, dc.EDGE_PORTS, g.up(arena, np.uint8), len(arena), g.up(desc, nf.DESC_DTYPE), n,
                                   g.up(s["rt"], np.uint8), g.up(s["nh"], np.uint32), g.up(s["l2p"], np.uint32), g.up(s["l2v"], np.uint8),
                                   action=g.up(s["action"], np.uint8), redirect=g.up(s["redirect"], np.uint32), rx_stats=d_rx,
                                   stream=stream)


def dispatch_host(fdb, ingress, arena, desc, s, rx):
    return fdb.ingress_dispatch_host(ingress, dc.EDGE_PORTS, arena, len(arena), desc, s["rt"], s["nh"], s["l2p"], s["l2v"],
                                     action=s["action"], redirect=s["redirect"], rx_stats=rx)


# ---- the dispatch's counters -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, WG * S - 1, WG * S, WG * S + 1])
def test_dispatch_counters_at_workgroup_and_stripe_edges(engine, efdb, n):
    arena, desc, s, e = edge_burst(n)
    rx = np.zeros(dc.EDGE_PORTS, RX)
    g = dc.Guarded(engine)
    d_rx = g.up(rx, RX)
    got = dc.device_dispatch(engine, efdb, dc.EDGE_INGRESS, dc.EDGE_PORTS, arena, len(arena), desc, s, d_rx=d_rx, g=g)
    want = dispatch_host(efdb, dc.EDGE_INGRESS, arena, desc, s, rx)
    dc.assert_dispatch(got, want, want["cls"], what=f"n = {n}: ")
    drx = d_rx.download(RX, dc.EDGE_PORTS)
    assert np.array_equal(drx, rx), f"n = {n}: counters {drx} != {rx}"
    drops = int(np.isin(want["cls"], dc.DROPS).sum())
    lens = desc["len"].astype(np.uint64)
    assert tuple(int(rx[dc.EDGE_INGRESS][k]) for k in RX.names) == (
        n + drops, int(lens.sum() + lens[np.isin(want["cls"], dc.DROPS)].sum()), drops)
    if n >= e.n:
        assert drops > 0 and (want["cls"] == nf.SW_BAD_DESC).any() and (want["cls"] == nf.SW_L3_FWD).any()
    g.free()


def test_dispatch_counters_chain_and_a_down_link_adds_nothing(engine, efdb):
    """Three launches on one stream into one array with one download: each fold leaves the stripes clean for the next.
    A fourth launch on the port whose link is down, and a fifth on a port the table does not have, add nothing."""
    g = dc.Guarded(engine)
    rx = np.zeros(NRX, RX)
    d_rx = g.up(rx, RX)
    for n in (WG * S + 1, 65, 3 * WG):
        arena, desc, s, _ = edge_burst(n)
        dispatch_launch(engine, g, efdb, dc.EDGE_INGRESS, arena, desc, s, d_rx)
        dispatch_host(efdb, dc.EDGE_INGRESS, arena, desc, s, rx)
    engine.sync()
    after3 = d_rx.download(RX, NRX)
    assert np.array_equal(after3, rx), f"{after3} != {rx}"
    assert int(rx[dc.EDGE_INGRESS]["rx_drops"]) > 3 * S
    arena, desc, s, _ = edge_burst(WG * S + 1)
    for ingress in (dc.EDGE_DOWN, dc.EDGE_PORTS + 1):
        dispatch_launch(engine, g, efdb, ingress, arena, desc, s, d_rx)
        dispatch_host(efdb, ingress, arena, desc, s, rx)
    engine.sync()
    assert np.array_equal(d_rx.download(RX, NRX), after3) and np.array_equal(rx, after3)
    # and the stripes are still clean
    arena, desc, s, _ = edge_burst(257)
    dispatch_launch(engine, g, efdb, dc.EDGE_INGRESS, arena, desc, s, d_rx)
    dispatch_host(efdb, dc.EDGE_INGRESS, arena, desc, s, rx)
    engine.sync()
    assert np.array_equal(d_rx.download(RX, NRX), rx)
    g.check()
    g.free()


def test_dispatch_counters_from_two_streams_into_one_array(engine, efdb):
    """One launch on a caller's stream and one on the context's own, into the same array, no sync between."""
    hip = ctypes.CDLL("libamdhip64.so.7")
    st = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(st)) == 0
    g = dc.Guarded(engine)
    try:
        rx = np.zeros(dc.EDGE_PORTS, RX)
        d_rx = g.up(rx, RX)
        bursts = [edge_burst(WG * S + 1), edge_burst(5 * WG + 3)]
        engine.sync()
        for (arena, desc, s, _), stream in zip(bursts, (st.value, None)):
            dispatch_launch(engine, g, efdb, dc.EDGE_INGRESS, arena, desc, s, d_rx, stream=stream)
            dispatch_host(efdb, dc.EDGE_INGRESS, arena, desc, s, rx)
        assert hip.hipStreamSynchronize(st) == 0
        engine.sync()
        got = d_rx.download(RX, dc.EDGE_PORTS)
        assert np.array_equal(got, rx), f"{got} != {rx}"
        g.check()
    finally:
        g.free()
        hip.hipStreamDestroy(st)


def test_a_refused_dispatch_leaves_counters_and_outputs(engine):
    arena, desc, s, _ = edge_burst(300)
    g = dc.Guarded(engine)
    d_rx, d_cls = g.up(np.full(dc.EDGE_PORTS * 3, 7, np.uint64), np.uint64), g.out(300)
    d_nh = g.up(s["nh"], np.uint32)
    with dc.edge_fdb() as never_uploaded, pytest.raises(nf.NfcsError):
        engine.ingress_dispatch_device(never_uploaded, dc.EDGE_INGRESS, dc.EDGE_PORTS, g.up(arena, np.uint8), len(arena),
                                       g.up(desc, nf.DESC_DTYPE), 300, g.up(s["rt"], np.uint8), d_nh, g.up(s["l2p"], np.uint32),
                                       g.up(s["l2v"], np.uint8), cls=d_cls, rx_stats=d_rx)
    engine.sync()
    assert (d_rx.download(np.uint64, dc.EDGE_PORTS * 3) == 7).all() and (d_cls.download(np.uint8, 300) == FILL).all()
    assert np.array_equal(d_nh.download(np.uint32, 300), s["nh"])
    g.check()
    g.free()


# ---- the egress ACL's counters -------------------------------------------------------------------------------------

ACL_PORTS = 37  # 74 slots per stripe: five lines, the last one partly used


@pytest.fixture(scope="module")
def deny_set(engine):
    """Every port 0..36 bound to one list that denies source 10.9.0.0 (udp_frame(0)) and permits the rest."""
    with nf.AclSet() as s:
        s.set_list(0, rule(action=nf.ACL_DENY, src_ip=(10 << 24) | (9 << 16)))
        for p in range(ACL_PORTS):
            s.bind_port(p, 0)
        yield s.commit().upload(engine)


def acl_both(engine, s, arena, desc, port, entry, start=None):
    """(device, host) of one call: dicts of port, action, pk, by. entry: plain, items or bypass."""
    n = len(desc)
    item_src = bypass = None
    if entry == "bypass":
        rng = np.random.default_rng(n)
        item_src = rng.integers(0, n // 2 + 5, n).astype(np.uint32)
        bypass = (rng.random(n // 2 + 1) < 0.3).astype(np.uint8)
    pk0, by0 = start or (np.zeros(ACL_PORTS, np.uint32), np.zeros(ACL_PORTS, np.uint64))
    pk, by = pk0.copy(), by0.copy()
    if entry == "plain":
        want = s.egress_acl_host(arena, desc, port, pk, by)
    else:
        want = s.egress_acl_items_host(arena, desc, port, item_src, bypass, pk, by)
    g = dc.Guarded(engine)
    d_arena, d_desc, d_port, d_a = g.up(arena, np.uint8), g.up(desc, nf.DESC_DTYPE), g.up(port, np.uint32), g.out(n)
    d_pk, d_by = g.up(pk0, np.uint32), g.up(by0, np.uint64)
    if entry == "plain":
        engine.egress_acl_device(s, d_arena, len(arena), d_desc, n, d_port, d_a, None, None, d_pk, d_by)
    else:
        engine.egress_acl_items_device(s, d_arena, len(arena), d_desc, n, d_port, d_a,
                                       item_src=None if item_src is None else g.up(item_src, np.uint32),
                                       bypass=None if bypass is None else g.up(bypass, np.uint8),
                                       n_src=0 if bypass is None else len(bypass), denied_pkts=d_pk, denied_bytes=d_by)
    engine.sync()
    got = dict(port=d_port.download(np.uint32, n), action=d_a.download(np.uint8, n), pk=d_pk.download(np.uint32, ACL_PORTS),
               by=d_by.download(np.uint64, ACL_PORTS))
    assert np.array_equal(d_arena.download(np.uint8, len(arena)), arena)
    g.check()
    g.free()
    return got, dict(port=want["port"], action=want["action"], pk=pk, by=by)


@pytest.mark.parametrize("entry", ["plain", "items", "bypass"])
@pytest.mark.parametrize("traffic", ["one port", "every port", "none denied"])
@pytest.mark.parametrize("n", [1, 64, 257, WG * S_ACL + 1])
def test_egress_acl_counters(engine, deny_set, n, traffic, entry):
    i = np.arange(n)
    port = np.full(n, 5, np.uint32) if traffic == "one port" else ((i * 7) % ACL_PORTS).astype(np.uint32)
    frames = [udp_frame(1 if traffic == "none denied" else 0, length=60 + int(k) % 90) for k in i]
    arena, desc = pack(frames)
    got, want = acl_both(engine, deny_set, arena, desc, port, entry)
    for k in want:
        assert np.array_equal(got[k], want[k]), f"{k}: {got[k]} != {want[k]}"
    denied = want["action"] == nf.ACL_DENY
    assert np.array_equal(want["pk"], np.bincount(port[denied], minlength=ACL_PORTS).astype(np.uint32))
    if traffic == "none denied":
        assert not denied.any()
    elif entry != "bypass":
        assert denied.all() and int(want["pk"].sum()) == n
    else:
        assert n < 64 or (denied.any() and not denied.all())
    if traffic == "every port" and n >= 257 and entry != "bypass":
        assert (want["pk"] > 0).all()


def test_egress_acl_bytes_are_summed_in_64_bits(engine, deny_set):
    """65,536 descriptors of 65,535 bytes on one frame (the length is counted, the bytes behind the headers are never
    read): a workgroup's sum passes 2^24, a stripe's 2^28, and the port's counter, started near 2^32, passes it."""
    n = 65536
    arena = np.full(65536, FILL, np.uint8)
    f = udp_frame(0)
    arena[:len(f)] = np.frombuffer(f, np.uint8)
    desc = np.zeros(n, nf.DESC_DTYPE)
    desc["len"] = 65535
    port = np.where(np.arange(n) % 4 == 0, 9, 11).astype(np.uint32)
    start = (np.zeros(ACL_PORTS, np.uint32), np.zeros(ACL_PORTS, np.uint64))
    start[0][9], start[1][9], start[1][11] = 0xFFFFFF00, 0xFFFFFFF0, 1 << 32
    got, want = acl_both(engine, deny_set, arena, desc, port, "plain", start=start)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert int(want["by"][9]) == 0xFFFFFFF0 + 16384 * 65535 and int(want["by"][11]) == (1 << 32) + 49152 * 65535
    assert int(want["pk"][9]) == (0xFFFFFF00 + 16384) & 0xFFFFFFFF and int(want["pk"][11]) == 49152
    assert int(want["by"][11]) - (1 << 32) > 1 << 31


def test_egress_acl_counters_chain_on_one_stream(engine, deny_set):
    """Three launches into one pair of arrays with one download: the fold leaves the stripes clean."""
    g = dc.Guarded(engine)
    pk, by = np.zeros(ACL_PORTS, np.uint32), np.zeros(ACL_PORTS, np.uint64)
    d_pk, d_by = g.up(pk, np.uint32), g.up(by, np.uint64)
    for n in (WG * S_ACL + 1, 64, 700):
        port = ((np.arange(n) * 5) % ACL_PORTS).astype(np.uint32)
        arena, desc = pack([udp_frame(int(k) % 2, length=60 + int(k) % 50) for k in range(n)])
        deny_set.egress_acl_host(arena, desc, port, pk, by)
        engine.egress_acl_device(deny_set, g.up(arena, np.uint8), len(arena), g.up(desc, nf.DESC_DTYPE), n, g.up(port, np.uint32),
                                 g.out(n), None, None, d_pk, d_by)
    engine.sync()
    assert np.array_equal(d_pk.download(np.uint32, ACL_PORTS), pk) and np.array_equal(d_by.download(np.uint64, ACL_PORTS), by)
    assert int(pk.sum()) > 2000
    g.check()
    g.free()


def test_a_refused_egress_acl_leaves_counters_and_outputs(engine):
    n = 300
    arena, desc = pack([udp_frame(0)] * n)
    g = dc.Guarded(engine)
    d_port, d_a = g.up(np.zeros(n, np.uint32), np.uint32), g.out(n)
    d_pk, d_by = g.up(np.full(4, 7, np.uint32), np.uint32), g.up(np.full(4, 7, np.uint64), np.uint64)
    with nf.AclSet() as s:
        s.set_list(0, rule(action=nf.ACL_DENY)).bind_port(0, 0).commit()  # never uploaded
        with pytest.raises(nf.NfcsError):
            engine.egress_acl_device(s, g.up(arena, np.uint8), len(arena), g.up(desc, nf.DESC_DTYPE), n, d_port, d_a, None, None,
                                     d_pk, d_by)
        with pytest.raises(nf.NfcsError):
            engine.egress_acl_items_device(s, g.up(arena, np.uint8), len(arena), g.up(desc, nf.DESC_DTYPE), n, d_port, d_a,
                                           denied_pkts=d_pk, denied_bytes=d_by)
    engine.sync()
    assert (d_pk.download(np.uint32, 4) == 7).all() and (d_by.download(np.uint64, 4) == 7).all()
    assert (d_a.download(np.uint8, n) == FILL).all() and not d_port.download(np.uint32, n).any()
    g.check()
    g.free()


# ---- the digest ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, WG * S + 1])
def test_digest_equals_the_oracle_twice(engine, oracle_lib, n):
    rng = np.random.default_rng(n)
    pool = [rng.integers(0, 256, int(ln), dtype=np.uint8).tobytes() for ln in (1, 15, 16, 17, 60, 64, 333, 1500)]
    arena, desc = pack([pool[k % len(pool)] for k in range(n)])
    g = dc.Guarded(engine)
    d_arena, d_desc = g.up(arena, np.uint8), g.up(desc, nf.DESC_DTYPE)
    want = oracle_lib.digest(arena, desc, 5)
    first = engine.digest_device(d_arena, len(arena), d_desc, n, 5)
    again = engine.digest_device(d_arena, len(arena), d_desc, n, 5)
    assert first == want and again == want, f"{first:#x}, {again:#x} != {want:#x}"
    g.check()
    g.free()
