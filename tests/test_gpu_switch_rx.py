"""GPU test of the one-call RX pipeline: the three bursts of tests/golden/switch_ref.npz through
Engine.switch_rx_device and txq_dequeue_device (dispatch_common.device_switch_rx: every burst launched before anything
is downloaded, depths, deny counters, RX counters and TX rings chained on the device), held to what the reference's
netflow::Switch left, and to dispatch_common.host_switch_rx for what the reference does not record: the arenas, the
classes and a switch without egress lists. Guard bytes lie behind every array and behind the workspace."""
import numpy as np
import pytest

import netflow_amd as nf
import dispatch_common as dc
import switch_common as sw
from flood_common import pack_with_tail

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return sw.Fixture()


@pytest.fixture(scope="module")
def t(fx):
    t = sw.tables(fx.z)
    yield t
    sw.close_tables(t)


@pytest.fixture(scope="module")
def host(fx, t):
    return dc.host_switch_rx(t, fx.bursts)


def check_classes_and_counters(fx, got):
    for b, (ingress, first, frames, _) in enumerate(fx.bursts):
        assert np.array_equal(dc.to_code(got["cls"][b]), fx.z["code"][first:first + len(frames)]), f"burst {b}: classes"
        ps = fx.z[f"port_stats_{b}"]
        for k, name in enumerate(nf.RX_STATS_DTYPE.names):
            assert np.array_equal(got["rx_stats"][b][name], ps[:, k].astype(np.uint64)), f"burst {b}: {name}"


def test_the_fixture_through_the_composite(engine, fx, t, host):
    got = dc.device_switch_rx(engine, t, fx.bursts)
    sw.assert_same(got, fx.want(), "against the reference: ")
    sw.assert_same(got, host, "against the CPU chain: ", arenas=True)
    check_classes_and_counters(fx, got)
    for b in range(len(fx.bursts)):
        assert np.array_equal(got["cls"][b], host["cls"][b]) and np.array_equal(got["rx_stats"][b], host["rx_stats"][b])


def test_16_byte_frame_starts_and_copy_slots(engine, fx, t):
    got = dc.device_switch_rx(engine, t, fx.bursts, align=16, copy_align=16)
    sw.assert_same(got, fx.want(), "against the reference: ")
    sw.assert_same(got, dc.host_switch_rx(t, fx.bursts, align=16, copy_align=16), "against the CPU chain: ", arenas=True)
    check_classes_and_counters(fx, got)


def test_a_port_with_no_ingress_list_and_no_egress_lists(engine, fx, t):
    """The fixture's burst on port 2, which has no ingress list, with aclset NULL: the host chain built the same way."""
    bursts = [b for b in fx.bursts if b[0] == 2]
    assert len(bursts) == 1 and 2 not in t["ingress_acl"]
    bursts = [(2, 0, bursts[0][2], bursts[0][3])]
    got = dc.device_switch_rx(engine, t, bursts, egress_acl=False)
    want = dc.host_switch_rx(t, bursts, egress_acl=False)
    sw.assert_same(got, want, arenas=True)
    assert np.array_equal(got["cls"][0], want["cls"][0]) and np.array_equal(got["rx_stats"][0], want["rx_stats"][0])
    assert not got["denied_pkts"][0].any() and sum(len(p) for p in got["tx"][0].values()) > 300
    assert not np.isin(got["cls"][0], [nf.SW_IN_DENY, nf.SW_RED_OK, nf.SW_RED_DOWN, nf.SW_RED_RANGE]).any()


def test_workspace_one_byte_short_and_tables_not_uploaded(engine, fx, t):
    """NFCS_EINVAL before anything is launched: every output and the workspace keep their fill."""
    for obj in [t["fib"], t["fdb"], t["eg"], t["aclset"], *t["ingress_acl"].values()]:
        obj.upload(engine)
    ingress, _, frames, _ = fx.bursts[0]
    frames = frames[:100]
    n, cap = len(frames), 4 * len(frames)
    ports, keys = t["eg"].keys()
    arena, desc, copy_base = pack_with_tail(frames, 16, sw.region_bytes(frames, 16))
    need = nf.switch_rx_workspace_bytes(n, cap)
    assert need % 16 == 0 and need >= 19 * n + 10 * cap and nf.switch_rx_workspace_bytes(0, 0) == 0
    assert nf.switch_rx_workspace_bytes(n + 1, cap) > need and nf.switch_rx_workspace_bytes(n, cap + 16) > need
    g = dc.Guarded(engine)
    d_arena, d_desc, d_depth = g.up(arena, np.uint8), g.up(desc, nf.DESC_DTYPE), g.up(np.zeros(keys, np.uint32), np.uint32)
    outs = [g.out(8 * cap), g.out(4 * cap), g.out(4 * cap), g.out(32), g.out(4 * cap), g.out(4 * (keys + 1))]
    d_ws = g.out(need)
    d_rx = g.up(np.zeros(t["num_ports"], nf.RX_STATS_DTYPE), nf.RX_STATS_DTYPE)

    def call(ws_bytes, fib=t["fib"], ws=d_ws):
        engine.switch_rx_device(fib, t["fdb"], t["eg"], ingress, t["num_ports"], d_arena, arena.nbytes, copy_base, 16, d_desc, n, cap,
                                d_depth, *outs, ws, ws_bytes, ingress_acl=t["ingress_acl"].get(ingress), aclset=t["aclset"], rx_stats=d_rx)

    with pytest.raises(nf.NfcsError):
        call(need - 1)
    with pytest.raises(nf.NfcsError):
        call(need, ws=d_ws.ptr + 8)  # not on a 16-byte boundary
    with nf.Fib() as other, pytest.raises(nf.NfcsError):
        call(need, fib=other.commit())  # committed, never uploaded
    engine.sync()
    for buf, nbytes in g.bufs[3:10]:
        assert (buf.download(np.uint8, nbytes) == dc.FILL).all(), "a refused call wrote something"
    assert not d_rx.download(np.uint8, 24 * t["num_ports"]).any() and not d_depth.download(np.uint32, keys).any()
    assert np.array_equal(d_arena.download(np.uint8, arena.nbytes), arena)
    call(need)  # and with the exact size it runs
    engine.sync()
    tot = outs[3].download(nf.FLOOD_TOTALS_DTYPE, 1)[0]
    assert 0 < int(tot["items"]) == int(tot["items_needed"]) <= cap and int(d_rx.download(nf.RX_STATS_DTYPE, t["num_ports"])[ingress]["rx_packets"]) >= n
    g.check()
    g.free()
