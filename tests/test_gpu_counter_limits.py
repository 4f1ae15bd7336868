"""GPU tests of the egress ACL's deny counters at the limits of egress_acl_kernel's LDS table and of the port range
(the cases and what each reaches are in counter_limits_common.py, their claims are proven on the CPU by
test_counter_limits.py): colliding ports, probe chains, probes that wrap past entry 255, a table with all 256 entries
taken, folds of more than one workgroup, the counter scratch's last slot, and the scratch's three regions used one
after the other on one stream. Every count is compared per port, exactly, with the numpy model and with the library's
host walk; 64 guard bytes lie behind every device array, the counters included, and every arena is compared after the
call."""
import numpy as np
import pytest

import netflow_amd as nf
import counter_limits_common as cl
import dispatch_common as dc
from egress_acl_common import pack

pytestmark = pytest.mark.gpu
RX = nf.RX_STATS_DTYPE


@pytest.fixture(scope="module")
def sets(engine):
    s = {P: cl.deny_set(P).upload(engine) for P in cl.SETS}
    yield s
    for x in s.values():
        x.close()


def launch(engine, g, s, c, entry, d_pk, d_by):
    """One call of the case's entry on uploaded copies; returns what to download and compare."""
    arena, desc, port, item_src, bypass = cl.inputs(c, entry)
    n = c["n"]
    d_arena, d_desc, d_port, d_a = g.up(arena, np.uint8), g.up(desc, nf.DESC_DTYPE), g.up(port, np.uint32), g.out(n)
    if entry == "plain":
        engine.egress_acl_device(s, d_arena, len(arena), d_desc, n, d_port, d_a, None, None, d_pk, d_by)
    else:
        engine.egress_acl_items_device(s, d_arena, len(arena), d_desc, n, d_port, d_a, item_src=g.up(item_src, np.uint32),
                                       bypass=g.up(bypass, np.uint8), n_src=len(bypass), denied_pkts=d_pk, denied_bytes=d_by)
    return arena, desc, d_arena, d_desc, d_port, d_a


def compare(c, got, m, h, what=""):
    for k in ("action", "port"):
        assert np.array_equal(got[k], m[k]), f"{what}{k} differs from the model"
        assert np.array_equal(got[k], h[k]), f"{what}{k} differs from the host walk"
    for k in ("pk", "by"):
        bad = np.flatnonzero(got[k] != m[k])
        assert len(bad) == 0, (f"{what}{k}: {len(bad)} ports differ from the model, the first port {bad[0]} (bucket "
                               f"{cl.bucket(bad[0])}): {got[k][bad[0]]} != {m[k][bad[0]]}")
        assert np.array_equal(got[k], h[k]), f"{what}{k} differs from the host walk"


@pytest.mark.parametrize("entry", cl.ENTRIES)
@pytest.mark.parametrize("name", list(cl.CASES))
def test_deny_counters(engine, sets, name, entry):
    c = cl.CASES[name]
    P, n, s = c["P"], c["n"], sets[c["P"]]
    m, h = cl.model(c, entry), cl.host(s, c, entry)
    g = dc.Guarded(engine)
    d_pk, d_by = g.up(c["pk0"], np.uint32), g.up(c["by0"], np.uint64)
    arena, desc, d_arena, d_desc, d_port, d_a = launch(engine, g, s, c, entry, d_pk, d_by)
    engine.sync()
    got = dict(action=d_a.download(np.uint8, n), port=d_port.download(np.uint32, n), pk=d_pk.download(np.uint32, P),
               by=d_by.download(np.uint64, P))
    assert np.array_equal(d_arena.download(np.uint8, len(arena)), arena), "the call wrote into the arena"
    assert np.array_equal(d_desc.download(nf.DESC_DTYPE, n), desc)
    g.check()
    g.free()
    compare(c, got, m, h)


def test_the_scratchs_regions_stay_apart(engine, sets, oracle_lib):
    """One stream, nothing downloaded before the end: the 1,024-port call, a counted dispatch, the digest, a call on a
    37-port set (another stride), the 1,024-port call again, a counted dispatch. A stripe left dirty or a region that
    reaches into its neighbour shows in a later call's counters. (nfcs_digest_device hands its one word to the host
    itself; no array is downloaded before the last launch.)"""
    g = dc.Guarded(engine)
    big, entry = cl.CASES["fold-1024"], "items"
    s1024 = sets[1024]
    want_big = cl.model(big, entry)
    again = dict(big, pk0=want_big["pk"], by0=want_big["by"])  # the second call goes on counting
    want_again, host_again = cl.model(again, entry), cl.host(s1024, again, entry)
    d_pk, d_by = g.up(big["pk0"], np.uint32), g.up(big["by0"], np.uint64)
    # the dispatch: dispatch_common's edge burst, 64 * 256 + 1 frames, so every one of its stripes is used
    e = dc.Edges()
    idx = np.arange(64 * 256 + 1) % e.n
    e_desc, e_s = e.desc[idx], {k: v[idx] for k, v in e.s.items()}
    rx = np.zeros(dc.EDGE_PORTS, RX)
    d_rx = g.up(rx, RX)
    # the digest: frames of many lengths
    rng = np.random.default_rng(3)
    pool = [rng.integers(0, 256, int(ln), dtype=np.uint8).tobytes() for ln in (1, 15, 16, 17, 60, 64, 333, 1500)]
    dg_arena, dg_desc = pack([pool[k % len(pool)] for k in range(64 * 256 + 1)])
    # the 37-port set of the older counting tests: a stride of 80 slots
    i = np.arange(256 * 16 + 1)
    small = cl.make(37, (i * 7) % 37, tag=i % 4 == 0, start=True)
    want_small = cl.model(small, "plain")

    def dispatch(fdb):
        engine.ingress_dispatch_device(fdb, dc.EDGE_INGRESS, dc.EDGE_PORTS, g.up(e.arena, np.uint8), len(e.arena),
                                       g.up(e_desc, nf.DESC_DTYPE), len(idx), g.up(e_s["rt"], np.uint8), g.up(e_s["nh"], np.uint32),
                                       g.up(e_s["l2p"], np.uint32), g.up(e_s["l2v"], np.uint8), action=g.up(e_s["action"], np.uint8),
                                       redirect=g.up(e_s["redirect"], np.uint32), rx_stats=d_rx)
        fdb.ingress_dispatch_host(dc.EDGE_INGRESS, dc.EDGE_PORTS, e.arena, len(e.arena), e_desc, e_s["rt"], e_s["nh"].copy(),
                                  e_s["l2p"].copy(), e_s["l2v"].copy(), action=e_s["action"], redirect=e_s["redirect"], rx_stats=rx)

    with dc.edge_fdb() as fdb, cl.deny_set(37) as s37:
        fdb.upload(engine), s37.upload(engine)
        host_small = cl.host(s37, small, "plain")
        d_spk, d_sby = g.up(small["pk0"], np.uint32), g.up(small["by0"], np.uint64)
        first = launch(engine, g, s1024, big, entry, d_pk, d_by)
        dispatch(fdb)
        d_dg_arena, d_dg_desc = g.up(dg_arena, np.uint8), g.up(dg_desc, nf.DESC_DTYPE)
        digest = engine.digest_device(d_dg_arena, len(dg_arena), d_dg_desc, len(dg_desc), 5)
        third = launch(engine, g, s37, small, "plain", d_spk, d_sby)
        second = launch(engine, g, s1024, again, entry, d_pk, d_by)
        dispatch(fdb)
        engine.sync()
    assert digest == oracle_lib.digest(dg_arena, dg_desc, 5)
    assert np.array_equal(d_rx.download(RX, dc.EDGE_PORTS), rx) and int(rx[dc.EDGE_INGRESS]["rx_drops"]) > 2 * 64
    for (c, m, h, (_, _, _, _, d_port, d_a), pk, by, what) in (
            (again, want_again, host_again, second, d_pk, d_by, "the 1,024-port set after both calls: "),
            (small, want_small, host_small, third, d_spk, d_sby, "the 37-port set: ")):
        got = dict(action=d_a.download(np.uint8, c["n"]), port=d_port.download(np.uint32, c["n"]), pk=pk.download(np.uint32, c["P"]),
                   by=by.download(np.uint64, c["P"]))
        compare(c, got, m, h, what)
    assert np.array_equal(first[5].download(np.uint8, big["n"]), want_big["action"])
    g.check()
    g.free()
