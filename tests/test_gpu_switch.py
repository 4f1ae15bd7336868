"""GPU test of the whole device pipeline against the reference's Switch: switch_common.device_switch (route lookup
-> ACL -> L2 lookup -> forward -> flood expand -> plan -> VLAN -> egress ACL -> enqueue -> append -> dequeue, with
switch_common.glue() between the calls) over the three bursts of tests/golden/switch_ref.npz, held directly to
what the reference's netflow::Switch left, and to switch_common.host_switch for what the reference does not
record: the arenas, other frame geometries and a burst beyond three tiles. Reads only the fixture."""
import pytest

import netflow_amd as nf
from switch_common import Fixture, assert_same, close_tables, device_switch, host_switch, tables

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return Fixture()


@pytest.fixture(scope="module")
def t(fx):
    t = tables(fx.z)
    yield t
    close_tables(t)


@pytest.fixture(scope="module")
def host(fx, t):
    """The CPU chain at the default geometry, which tests/test_switch.py holds to the reference."""
    return host_switch(t, fx.bursts)


def test_device_chain_equals_the_reference_switch(engine, fx, t, host):
    """TX bytes and order per port, depths after every burst, tail drops and the deny counters against the fixture;
    then the whole arena of every burst, copy region included, against the CPU chain's. device_switch checks the
    guard bytes behind the arenas and behind every output array."""
    got = device_switch(engine, t, fx.bursts)
    assert_same(got, fx.want(), "against the reference: ")
    assert_same(got, host, "against the CPU chain: ", arenas=True)
    assert max(a.nbytes for a in got["arena"]) < 8 << 20


@pytest.mark.parametrize("align,copy_align", [(16, 16), (16, 128), (128, 16)])
def test_other_geometries_give_the_same_answers(engine, fx, t, align, copy_align):
    """Frames packed at 16-byte starts or at 128-byte line starts, copies in 16-byte or 128-byte slots: what is
    sent, queued, dropped and counted is the reference's, and the arenas are the CPU chain's at that geometry."""
    got = device_switch(engine, t, fx.bursts, align=align, copy_align=copy_align)
    assert_same(got, fx.want(), f"align {align}, copy_align {copy_align}, against the reference: ")
    assert_same(got, host_switch(t, fx.bursts, align=align, copy_align=copy_align), "against the CPU chain: ", arenas=True)


def test_a_burst_beyond_three_tiles(engine, fx, t):
    """Burst 0 appended to itself up to 3 x 1,024 + 7 frames, then the other two bursts, against the CPU chain."""
    ingress, first, frames, budget = fx.bursts[0]
    n = 3 * nf.EGRESS_TILE_PKTS + 7
    long = (frames * 3)[:n]
    assert len(long) == n
    bursts = [(ingress, 0, long, budget)] + [(i, n + f, fr, b) for i, f, fr, b in fx.bursts[1:]]
    got = device_switch(engine, t, bursts, align=16)
    want = host_switch(t, bursts, align=16)
    assert sum(len(p) for p in want["tx"][2].values()) > 1000 and want["dropped"][2].sum() > 500
    assert_same(got, want, arenas=True)
