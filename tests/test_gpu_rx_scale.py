"""GPU tests of nfcs_switch_rx_device past one enqueue tile per scan segment: bursts of 17 and 129
enqueue tiles through the composite and the dequeue, against dispatch_common.host_switch_rx on the same inputs, on every
array the call hands out, the arenas, classes, RX and deny counters, depths, tail drops and the dequeued TX lists; with
the expand cut by `cap` and by the copy region, an odd `cap`, one workspace reused by three calls, optional outputs
NULL, and the scratch the stages share growing between the composite's expand and its enqueue. The inputs and what
they reach are built in rx_scale_common.py and proven on the CPU by test_rx_scale.py. Guard bytes lie behind every
device array and behind the workspace."""
import ctypes

import numpy as np
import pytest

import netflow_amd as nf
import dispatch_common as dc
import rx_scale_common as rs
import switch_common as sw

pytestmark = pytest.mark.gpu
Q = nf.QOS_MAX_QUEUES


@pytest.fixture(scope="module")
def sc():
    s = rs.Scale()
    yield s
    s.close()


def same(got, want, what=""):
    sw.assert_same(got, want, what, arenas=True)
    dc.assert_same_rx(got, want, what)


@pytest.mark.parametrize("kind,tiles,align", [("fits", *c) for c in rs.FITS] + [("tight", *c) for c in rs.TIGHT])
def test_everything_fits(engine, sc, kind, tiles, align):
    """fits: the issue's sizes, cap = 4 n. tight: cap and region exactly what the burst needs, so the last enqueue tile
    holds items. Both: device equals the host chain, and the conservation identities hold on the device's own output."""
    t, bursts, kw = sc.case(kind, tiles, align)
    got = dc.device_switch_rx(engine, t, bursts, **kw)
    same(got, sc.host(kind, tiles, align))
    rs.identities(got, len(bursts[0][2]), Q, sc.skip_ports)


@pytest.mark.parametrize("tiles,align", rs.CUTS)
@pytest.mark.parametrize("kind", ["cap_cut", "region_cut"])
def test_the_expand_is_cut(engine, sc, kind, tiles, align):
    """The entries [items, cap) are inert for the plan, the VLAN edit, the egress ACL, the enqueue and the append."""
    t, bursts, kw = sc.case(kind, tiles, align)
    got, want = dc.device_switch_rx(engine, t, bursts, **kw), sc.host(kind, tiles, align)
    same(got, want)
    tot = got["totals"][0]
    assert int(tot["items"]) < int(tot["items_needed"])
    items = int(tot["items"])
    assert (got["iport"][0][items:] == nf.IF_NONE).all() and (got["isrc"][0][items:] == nf.ITEM_NONE).all()
    assert not np.isin(got["order"][0][:int(got["key_start"][0][-1])], np.arange(items, len(got["iport"][0]))).any()
    assert (got["tx_raw"][0][0] & 0xFFFFFFFF < items).all()


def test_odd_cap_and_odd_n_and_the_exact_workspace(engine, sc):
    """cap = 4 n + 3 with n odd: every sub-array of the workspace starts after rounding. One byte less is refused."""
    tiles, align = 17, 16
    t, bursts, kw = sc.case("fits", tiles, align)
    n = len(bursts[0][2])
    cap = sw.FANOUT * n + 3
    assert n % 2 == 1 and cap % 2 == 1
    need = nf.switch_rx_workspace_bytes(n, cap)
    assert need % 16 == 0 and need > nf.switch_rx_workspace_bytes(n, cap - 3) - 16
    with pytest.raises(nf.NfcsError):
        dc.device_switch_rx(engine, t, bursts, cap=cap, ws_bytes=need - 1, **kw)
    engine.sync()
    got = dc.device_switch_rx(engine, t, bursts, cap=cap, ws_bytes=need, **kw)
    want = dc.host_switch_rx(t, bursts, cap=cap, **kw)
    same(got, want)
    assert int(got["totals"][0]["items"]) == int(got["totals"][0]["items_needed"])


def test_one_workspace_for_three_calls(engine, sc):
    """One workspace sized for the largest call and filled once; 129 tiles, 17 tiles, 129 tiles of another port's
    frames on one stream with nothing downloaded between them, depths, counters and rings chained. A stage that reads
    a workspace entry this call did not write sees the call before."""
    align = 128
    n_big, n_small = rs.SIZES[129], rs.SIZES[17]
    t = sc.t(rs.depth_for(n_big))
    bursts = [rs.burst(sc.fx, rs.INGRESS, n_big), rs.burst(sc.fx, rs.INGRESS, n_small, first=n_big),
              rs.burst(sc.fx, rs.OTHER, n_big, first=n_big + n_small)]
    size = max(nf.switch_rx_workspace_bytes(len(b[2]), sw.FANOUT * len(b[2])) for b in bursts)
    ws = engine.alloc(size + dc.GUARD).upload(np.full(size + dc.GUARD, dc.FILL, np.uint8))
    got = dc.device_switch_rx(engine, t, bursts, align=align, copy_align=align, workspace=(ws, size))
    assert (ws.download(np.uint8, dc.GUARD, offset=size) == dc.FILL).all(), "the guard behind the workspace changed"
    ws.free()
    want = dc.host_switch_rx(t, bursts, align=align, copy_align=align)
    same(got, want)
    for b in range(3):
        assert int(want["key_start"][b][-1]) > 0 and int(want["key_dropped"][b].sum()) > 0 and len(want["tx_raw"][b][0]) > 0
        rs.identities(got, len(bursts[b][2]), Q, sc.skip_ports, b=b)


def test_optional_outputs_null(engine, sc):
    """No ingress list, aclset NULL, txq NULL, rx_stats, cls and key_dropped NULL, at 17 tiles."""
    t, bursts, kw = sc.case("fits", 17, 16)
    null = ("ingress_acl", "txq", "rx_stats", "cls", "key_dropped")
    got = dc.device_switch_rx(engine, t, bursts, egress_acl=False, null=null, **kw)
    want = dc.host_switch_rx(t, bursts, egress_acl=False, null=null, **kw)
    same(got, want)
    assert not got["rx_stats"][0]["rx_packets"].any() and not got["denied_pkts"][0].any() and len(got["tx_raw"][0][0]) == 0
    assert int(got["key_start"][0][-1]) > 0 and got["depth"][0].any()


@pytest.mark.parametrize("caller_stream", [False, True])
def test_the_scratch_grows_inside_the_call(sc, caller_stream):
    """A context of its own: the expand's acquire allocates the scratch's first 2^18 words, the enqueue of the same call
    needs 35 x 8,192 and grows it; a second call follows on the grown scratch. With caller_stream the first burst (its
    call, dequeue and state copies) runs on a caller's stream and the second follows on the context's own with no host
    synchronisation between them. This pins the path's results, not the race (§24)."""
    t = rs.growth_tables(sc.fx, rs.depth_for(rs.GROW_N))
    hip, st = ctypes.CDLL("libamdhip64.so.7"), ctypes.c_void_p()
    try:
        assert t["eg"].keys() == (rs.GROW_PORT + 1, (rs.GROW_PORT + 1) * Q) and rs.growth_words(rs.GROW_N) > 1 << 18
        bursts = [rs.growth_burst(sc.fx), rs.growth_burst(sc.fx)]
        want = dc.host_switch_rx(t, bursts, align=16, copy_align=16)
        with nf.Engine() as own:
            if caller_stream:
                assert hip.hipStreamCreate(ctypes.byref(st)) == 0
            got = dc.device_switch_rx(own, t, bursts, align=16, copy_align=16, stream=st.value)
            same(got, want)
            for b in range(2):
                rs.identities(got, rs.GROW_N, Q, sc.skip_ports, b=b)
            for obj in [t["fib"], t["fdb"], t["eg"], t["aclset"], *t["ingress_acl"].values()]:
                obj.close()
            if st.value:
                assert hip.hipStreamDestroy(st) == 0
    finally:
        sw.close_tables(t)
