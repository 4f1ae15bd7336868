"""GPU tests of the ingress dispatch kernel and of the egress ACL over items with bypass: the device stage equals
the host stage (tests/test_dispatch.py holds that one to the reference's Switch) on the fixture's bursts at 16- and
128-byte frame starts, on the hand-built edges, at burst sizes around a wave, a workgroup and three tiles, with
descriptors that reach past the arena, and with frames past 32 GiB. 64 guard bytes of 0xEE lie behind every device
array, the counters included. Nothing reaches outside allocated memory: a descriptor "outside the arena" is outside
arena_bytes, inside the allocation."""
import numpy as np
import pytest

import netflow_amd as nf
import dispatch_common as dc
import oracle
import switch_common as sw
from egress_acl_common import Fixture as EgressAclFixture
from egress_acl_common import pack
from flood_common import pack_with_tail, round_up

pytestmark = pytest.mark.gpu
RX = nf.RX_STATS_DTYPE


@pytest.fixture(scope="module")
def fx():
    return sw.Fixture()


@pytest.fixture(scope="module")
def t(fx, engine):
    t = sw.tables(fx.z)
    t["fdb"].upload(engine)
    yield t
    sw.close_tables(t)


@pytest.fixture(scope="module")
def inputs(fx, t):
    """Per burst: (ingress, frames, stage inputs), computed once."""
    return [(ingress, frames, dc.stage_inputs(t, ingress, frames)) for ingress, _, frames, _ in fx.bursts]


@pytest.fixture(scope="module")
def efdb(engine):
    with dc.edge_fdb() as fdb:
        yield fdb.upload(engine)


def rx_tuple(rx, port):
    return tuple(int(rx[port][k]) for k in RX.names)


def both(engine, fdb, ingress, num_ports, arena, arena_bytes, desc, s, g=None, **kw):
    """(device result, host result, device counters, host counters) of one call from zeroed counters."""
    rx = np.zeros(num_ports, RX)
    g_own = g or dc.Guarded(engine)
    d_rx = g_own.up(rx, RX)
    got = dc.device_dispatch(engine, fdb, ingress, num_ports, arena, arena_bytes, desc, s, d_rx=d_rx, g=g_own, **kw)
    want = fdb.ingress_dispatch_host(ingress, num_ports, arena, arena_bytes, desc, s["rt"], s["nh"], s["l2p"], s["l2v"],
                                     action=s["action"], redirect=s["redirect"], rx_stats=rx)
    drx = d_rx.download(RX, num_ports)
    if g is None:
        g_own.free()
    return got, want, drx, rx


@pytest.mark.parametrize("align", [16, 128])
def test_device_equals_host_on_the_fixture(engine, fx, t, inputs, align):
    for b, (ingress, frames, s) in enumerate(inputs):
        arena, desc, copy_base = pack_with_tail(frames, align, 0)
        got, want, drx, rx = both(engine, t["fdb"], ingress, t["num_ports"], arena, copy_base, desc, s)
        dc.assert_dispatch(got, want, want["cls"], what=f"burst {b}, align {align}: ")
        assert np.array_equal(drx, rx) and rx_tuple(rx, ingress)[0] >= len(frames), f"burst {b}: counters {drx} != {rx}"
        assert (rx_tuple(rx, ingress)[2] > 50) == (ingress in t["ingress_acl"])  # a port without a list drops nothing
        first = fx.bursts[b][1]
        assert np.array_equal(dc.to_code(got["cls"]), fx.z["code"][first:first + len(frames)])


def test_counters_chain_over_three_calls_without_a_download(engine, fx, t, inputs):
    """Three bursts on two ingress ports into one counter array, launched back to back; then one download."""
    g = dc.Guarded(engine)
    d_rx = g.up(np.zeros(t["num_ports"], RX), RX)
    rx = np.zeros(t["num_ports"], RX)
    for ingress, frames, s in inputs:
        arena, desc, copy_base = pack_with_tail(frames, 16, 0)
        d = [g.up(arena, np.uint8), g.up(desc, nf.DESC_DTYPE), g.up(s["rt"], np.uint8), g.up(s["nh"], np.uint32), g.up(s["l2p"], np.uint32),
             g.up(s["l2v"], np.uint8)]
        opt = lambda a, dt: None if a is None else g.up(a, dt)  # noqa: E731
        engine.ingress_dispatch_device(t["fdb"], ingress, t["num_ports"], d[0], copy_base, d[1], len(frames), d[2], d[3], d[4], d[5],
                                       action=opt(s["action"], np.uint8), redirect=opt(s["redirect"], np.uint32), rx_stats=d_rx)
        dc.dispatch_host(t, ingress, arena, copy_base, desc, s, rx_stats=rx)
    engine.sync()
    got = d_rx.download(RX, t["num_ports"])
    assert np.array_equal(got, rx), f"{got} != {rx}"
    ps = fx.z["port_stats_2"]
    for k, name in enumerate(RX.names):
        assert np.array_equal(got[name], ps[:, k].astype(np.uint64)), name
    g.check()
    g.free()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 3 * 1024 + 7])
def test_burst_sizes(engine, t, inputs, n):
    """Burst 0 repeated or cut: one lane, a wave less one, a wave, a wave and one, a workgroup and one, three tiles and
    seven: partial waves and workgroups reduce their counters like whole ones."""
    ingress, frames, s = inputs[0]
    idx = np.arange(n) % len(frames)
    fr = [frames[i] for i in idx]
    sn = {k: (None if v is None else np.asarray(v)[idx]) for k, v in s.items()}
    arena, desc, copy_base = pack_with_tail(fr, 16, 0)
    got, want, drx, rx = both(engine, t["fdb"], ingress, t["num_ports"], arena, copy_base, desc, sn)
    dc.assert_dispatch(got, want, want["cls"], what=f"n = {n}: ")
    assert np.array_equal(drx, rx), f"n = {n}: counters {drx} != {rx}"
    assert rx_tuple(rx, ingress)[0] >= n


@pytest.mark.parametrize("case", ["acl", "no list", "link down", "no such port", "no class", "no bypass", "no counters", "no outputs"])
def test_edges(engine, efdb, case):
    e = dc.Edges(repeat=3)  # 99 frames: a wave and a partial one
    s = dict(e.s)
    ingress, want_out = dc.EDGE_INGRESS, ("cls", "bypass")
    cls = e.cls
    if case == "no list":
        s["action"] = s["redirect"] = None
        cls = e.cls_no_acl
    elif case == "link down":
        ingress, cls = dc.EDGE_DOWN, np.full(e.n, nf.SW_RX_DOWN, np.uint8)
    elif case == "no such port":
        ingress, cls = dc.EDGE_PORTS + 1, np.full(e.n, nf.SW_RX_DOWN, np.uint8)
    elif case == "no class":
        want_out = ("bypass",)
    elif case == "no bypass":
        want_out = ("cls",)
    elif case == "no outputs":
        want_out = ()
    rx = np.zeros(dc.EDGE_PORTS + 2, RX)
    g = dc.Guarded(engine)
    d_rx = None if case in ("no counters", "no outputs") else g.up(rx, RX)
    got = dc.device_dispatch(engine, efdb, ingress, dc.EDGE_PORTS, e.arena, len(e.arena), e.desc, s, d_rx=d_rx, want=want_out, g=g)
    host = efdb.ingress_dispatch_host(ingress, dc.EDGE_PORTS, e.arena, len(e.arena), e.desc, s["rt"], s["nh"], s["l2p"], s["l2v"],
                                      action=s["action"], redirect=s["redirect"], rx_stats=rx)
    dc.assert_dispatch(got, host, host["cls"], what=case + ", against the host: ")
    dc.assert_dispatch(got, e.want(cls, with_acl=case != "no list"), cls, what=case + ", against switch.hpp: ")
    if d_rx is not None:
        assert np.array_equal(d_rx.download(RX, len(rx)), rx)
        assert rx_tuple(rx, dc.EDGE_INGRESS) == (e.want(cls)["rx"] if ingress == dc.EDGE_INGRESS else (0, 0, 0))
    g.free()


def test_an_empty_burst_launches_nothing(engine, efdb):
    engine.ingress_dispatch_device(efdb, 0, dc.EDGE_PORTS, None, 0, None, 0, None, None, None, None)
    with nf.Fdb() as other, pytest.raises(nf.NfcsError):  # never uploaded
        engine.ingress_dispatch_device(other.commit(), 0, 6, None, 0, None, 0, None, None, None, None)


def test_descriptors_past_the_arena(engine, fx, t, inputs):
    """arena_bytes cut in the middle of burst 0 (the allocation holds the whole of it and the guard): the frames behind
    the cut come in as BAD_DESC verdicts, every third of them with the verdicts of a live frame instead, which the
    stage's own test of the descriptor catches. All of them read BAD_DESC, are masked and counted, none is a drop."""
    ingress, frames, s = inputs[0]
    arena, desc, copy_base = pack_with_tail(frames, 16, 0)
    cut = (int(desc[len(frames) // 2]["off16"]) * 16 + 8) & ~7
    dead = desc["off16"].astype(np.int64) * 16 + (desc["len"].astype(np.int64) + 15) // 16 * 16 > cut
    s = {k: (None if v is None else v.copy()) for k, v in s.items()}
    if s["action"] is None:
        s["action"], s["redirect"] = np.zeros(len(frames), np.uint8), np.full(len(frames), dc.NONE, np.uint32)
    told = dead & (np.arange(len(frames)) % 3 != 0)
    s["action"][told], s["rt"][told], s["l2v"][told] = nf.ACL_BAD_DESC, nf.RT_BAD_DESC, nf.L2_BAD_DESC
    got, want, drx, rx = both(engine, t["fdb"], ingress, t["num_ports"], arena, cut, desc, s)
    dc.assert_dispatch(got, want, want["cls"])
    assert dead.sum() > 300 and (got["cls"][dead] == nf.SW_BAD_DESC).all() and (got["cls"][~dead] != nf.SW_BAD_DESC).all()
    assert (got["nh"][dead] == nf.NH_NONE).all() and (got["l2_port"][dead] == nf.IF_NONE).all()
    assert np.array_equal(drx, rx) and rx_tuple(rx, ingress)[0] == len(frames) + int(np.isin(got["cls"], dc.DROPS).sum())


# ---- frames past 32 GiB ------------------------------------------------------------------------------------------

BASE = (32 << 30) + 4096  # byte offset of the high region: off16 = 2^31 + 256
LO = 4096
N = 20001                 # 312 waves and a partial one


def test_high_offsets_split(engine, t, inputs):
    """Even packets at the arena's start, odd ones past 32 GiB, so every wave spans both: a frame's byte offset needs
    36 bits. Only the two regions are uploaded."""
    ingress, frames, s = inputs[0]
    idx = np.arange(N) % len(frames)
    fr = [frames[i] for i in idx]
    sn = {k: (None if v is None else np.asarray(v)[idx]) for k, v in s.items()}
    desc, cdesc = np.zeros(N, nf.DESC_DTYPE), np.zeros(N, nf.DESC_DTYPE)
    parts, cbase = [], 0
    for dbase, which in ((LO, slice(0, None, 2)), (BASE, slice(1, None, 2))):
        arena, d = oracle.pack_frames(fr[which], align=16)
        for dst, base in ((desc, dbase), (cdesc, cbase)):
            dst["off16"][which] = d["off16"].astype(np.uint64) + base // 16
            dst["len"][which] = d["len"]
        parts.append((dbase, cbase, arena))
        cbase += round_up(arena.nbytes, 128)
    end = BASE + parts[1][2].nbytes
    assert int(desc["off16"].max()) >= 1 << 31 and LO + parts[0][2].nbytes < BASE
    compact = np.zeros(cbase, np.uint8)
    big = engine.alloc(end + dc.GUARD)
    try:
        for dbase, cb, a in parts:
            big.upload(a, dbase)
            compact[cb:cb + a.nbytes] = a
        big.upload(np.full(dc.GUARD, dc.FILL, np.uint8), end)
        rx = np.zeros(t["num_ports"], RX)
        want = t["fdb"].ingress_dispatch_host(ingress, t["num_ports"], compact, cbase, cdesc, sn["rt"], sn["nh"], sn["l2p"], sn["l2v"],
                                              action=sn["action"], redirect=sn["redirect"], rx_stats=rx)
        g = dc.Guarded(engine)
        d_rx, d_desc = g.up(np.zeros(t["num_ports"], RX), RX), g.up(desc, nf.DESC_DTYPE)
        d_nh, d_l2p, d_l2v = g.up(sn["nh"], np.uint32), g.up(sn["l2p"], np.uint32), g.up(sn["l2v"], np.uint8)
        d_cls, d_byp = g.out(N), g.out(N)
        opt = lambda a, dt: None if a is None else g.up(a, dt)  # noqa: E731
        engine.ingress_dispatch_device(t["fdb"], ingress, t["num_ports"], big, end, d_desc, N, g.up(sn["rt"], np.uint8), d_nh, d_l2p,
                                       d_l2v, action=opt(sn["action"], np.uint8), redirect=opt(sn["redirect"], np.uint32), cls=d_cls,
                                       bypass=d_byp, rx_stats=d_rx)
        engine.sync()
        got = dict(nh=d_nh.download(np.uint32, N), l2_port=d_l2p.download(np.uint32, N), l2_verdict=d_l2v.download(np.uint8, N),
                   cls=d_cls.download(np.uint8, N), bypass=d_byp.download(np.uint8, N))
        dc.assert_dispatch(got, want, want["cls"])
        assert np.array_equal(d_rx.download(RX, t["num_ports"]), rx)
        assert len(set(got["cls"][0::2])) > 12 and len(set(got["cls"][1::2])) > 12
        for dbase, _, a in parts:
            assert np.array_equal(big.download(np.uint8, a.nbytes, dbase), a), "the call wrote into the frames"
        assert (big.download(np.uint8, dc.GUARD, end) == dc.FILL).all()
        g.check()
        g.free()
    finally:
        big.free()


# ---- the egress ACL over items -----------------------------------------------------------------------------------

def device_items(engine, s, arena, desc, port, item_src, bypass, nports):
    g = dc.Guarded(engine)
    n = len(desc)
    d_arena, d_desc, d_port = g.up(arena, np.uint8), g.up(desc, nf.DESC_DTYPE), g.up(port, np.uint32)
    d_a, d_r, d_p = g.out(n), g.out(4 * n), g.out(4 * n)
    d_pk, d_by = g.up(np.zeros(nports, np.uint32), np.uint32), g.up(np.zeros(nports, np.uint64), np.uint64)
    d_src = None if item_src is None else g.up(item_src, np.uint32)
    d_byp = None if bypass is None else g.up(bypass, np.uint8)
    engine.egress_acl_items_device(s, d_arena, len(arena), d_desc, n, d_port, d_a, item_src=d_src, bypass=d_byp,
                                   n_src=0 if bypass is None else len(bypass), rule=d_r, redirect=d_p, denied_pkts=d_pk, denied_bytes=d_by)
    engine.sync()
    out = dict(port=d_port.download(np.uint32, n), action=d_a.download(np.uint8, n), rule=d_r.download(np.uint32, n),
               redirect=d_p.download(np.uint32, n), pk=d_pk.download(np.uint32, nports), by=d_by.download(np.uint64, nports))
    assert np.array_equal(d_arena.download(np.uint8, len(arena)), arena)
    g.check()
    g.free()
    return out


@pytest.mark.parametrize("bypassing", [False, True])
def test_items_kernel_equals_its_host_twin(engine, bypassing):
    """Without item_src and bypass: the egress ACL itself, byte for byte (and the existing entry point gives the same).
    With them: the host twin, which tests/test_dispatch.py holds to mask, call, restore."""
    fx = EgressAclFixture()
    reps = 5  # 5 x the fixture: several workgroups
    frames, port = fx.frames * reps, np.tile(fx.port, reps)
    arena, desc = pack(frames)
    n = len(desc)
    rng = np.random.default_rng(26)
    item_src = bypass = None
    if bypassing:
        n_src = n // 2
        item_src = rng.integers(0, n_src + 5, n).astype(np.uint32)
        item_src[rng.random(n) < 0.1] = nf.ITEM_NONE
        bypass = (rng.random(n_src) < 0.4).astype(np.uint8)
    with fx.aclset() as s:
        nports = s.info()[0]
        pk, by = np.zeros(nports, np.uint32), np.zeros(nports, np.uint64)
        want = s.egress_acl_items_host(arena, desc, port, item_src, bypass, pk, by)
        s.upload(engine)
        got = device_items(engine, s, arena, desc, port, item_src, bypass, nports)
        if not bypassing:
            g = dc.Guarded(engine)
            d_port, d_a = g.up(port, np.uint32), g.out(n)
            engine.egress_acl_device(s, g.up(arena, np.uint8), len(arena), g.up(desc, nf.DESC_DTYPE), n, d_port, d_a)
            engine.sync()
            assert np.array_equal(d_port.download(np.uint32, n), got["port"]) and np.array_equal(d_a.download(np.uint8, n), got["action"])
            g.check()
            g.free()
    for k in ("port", "action", "rule", "redirect"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["pk"], pk) and np.array_equal(got["by"], by) and pk.sum() > 50
    assert ((want["action"] == nf.ACL_BYPASS).sum() > 100) == bypassing
