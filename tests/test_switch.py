"""The whole pipeline on the CPU against the reference's Switch (tests/golden/switch_ref.npz, made by
tests/golden/make_switch_golden.py from a real netflow::Switch): switch_common.host_switch, the library's *_host
functions and the oracle chained in INTEGRATION.md's order with switch_common.glue() between them, over the
fixture's three bursts. The first test holds everything the reference left; the per-class tests name the frames
of one class and say what became of them, so that a failure names the rule that broke."""
import os
import sys

import numpy as np
import pytest

import netflow_amd as nf
from switch_common import (C_IN_DENY, C_L3_FWD, C_RED_DOWN, C_RED_RANGE, EV_EDENY, EV_ENQ, EV_FULL, Fixture, assert_same, close_tables,
                           host_switch, outcome, tables)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_switch_golden import check_classes, class_masks  # noqa: E402

# classes for which the reference sends nothing at all
QUIET = ("ingress deny l3", "ingress deny l2", "ingress redirect to a down port", "ingress redirect past num_ports", "local",
         "ttl", "no route", "arp miss", "no interface mac", "drop same port", "drop link down", "drop stp", "drop vlan", "arp",
         "lldp", "zero mac", "runt", "l3 egress deny", "l2 egress deny", "tail drop of a forwarded packet",
         "unicast to a port without a QoS config")
# one packet on the port the reference named; True: four bytes shorter than the frame
ONE = {"l3 forwarded": None, "l3 forwarded tcp untagged": False, "l3 forwarded tcp tagged": None,
       "l3 forwarded udp untagged": False, "l3 forwarded udp tagged": None, "l3 forwarded icmp untagged": False,
       "l3 forwarded icmp tagged": None, "l3 forwarded with options": None, "l3 forwarded, tag popped": True,
       "l3 egress redirect permitted": None, "ingress redirect": None, "ingress redirect, tag popped": True,
       "ingress redirect past a denying egress list": None, "l2 forward": None}
BY_EVENTS = ("flood fan-out >= 2", "flood fan-out < 2", "flood, one copy denied and one popped", "tail drop of a flood copy", "ipv6",
             "long tagged frame popped")


@pytest.fixture(scope="module")
def fx():
    return Fixture()


@pytest.fixture(scope="module")
def host(fx):
    t = tables(fx.z)
    try:
        return host_switch(t, fx.bursts)
    finally:
        close_tables(t)


@pytest.fixture(scope="module")
def classes(fx):
    return class_masks(fx.z)


def events_of(z, i):
    ev = z["ev"][int(z["ev_start"][i]):int(z["ev_start"][i + 1])]
    return [(int(e) >> 16, (int(e) >> 8) & 0xFF, int(e) & 0xFF) for e in ev]


def test_host_chain_equals_the_reference_switch(fx, host):
    """TX bytes and order per port, depths after every burst, tail drops and the deny counters."""
    want = fx.want()
    assert sum(len(p) for tx in want["tx"] for p in tx.values()) > 1500
    assert want["depth"][0].sum() > 100 and want["depth"][1].sum() > 100 and want["depth"][2].sum() == 0
    assert want["dropped"][2].sum() > 100 and want["denied_pkts"][2].sum() > 100 and min(want["rx_drops"][:2]) > 50
    assert_same(host, want)


def test_fixture_holds_every_class(fx):
    check_classes(fx.z)
    assert 700 <= min(len(b[2]) for b in fx.bursts) and max(len(b[2]) for b in fx.bursts) <= 1200
    assert max(len(b[2]) for b in fx.bursts) > nf.EGRESS_TILE_PKTS
    long = [f for f in fx.frames if len(f) >= 1400]
    assert len(long) >= 20 and all(f[12:14] == b"\x81\x00" and len(f) <= 1518 for f in long)


def test_every_frame_is_in_a_class(fx, classes):
    """No frame of the fixture escapes the per-class tests, and every class has a test."""
    covered = np.zeros(len(fx.frames), bool)
    for m in classes.values():
        covered |= m
    assert covered.all(), np.flatnonzero(~covered)[:20]
    assert set(classes) == set(QUIET) | set(ONE) | set(BY_EVENTS)


@pytest.mark.parametrize("name", QUIET)
def test_class_sends_nothing(fx, host, classes, name):
    got = outcome(host, len(fx.frames))
    idx = np.flatnonzero(classes[name])
    assert len(idx) >= 10
    bad = [int(i) for i in idx if got[i]]
    assert not bad, f"{name}: frames {bad[:10]} were sent: {[got[i] for i in bad[:10]]}"


@pytest.mark.parametrize("name", sorted(ONE))
def test_class_sends_one_packet_on_the_reference_port(fx, host, classes, name):
    got = outcome(host, len(fx.frames))
    idx = np.flatnonzero(classes[name])
    assert len(idx) >= 10
    for i in idx:
        i = int(i)
        assert len(got[i]) == 1 and got[i][0][0] == int(fx.z["port"][i]), f"{name}: frame {i} -> {got[i]}"
        if ONE[name] is not None:
            assert got[i][0][1] == len(fx.frames[i]) - (4 if ONE[name] else 0), f"{name}: frame {i} -> {got[i]}"


@pytest.mark.parametrize("name", BY_EVENTS)
def test_class_sends_what_the_reference_enqueued(fx, host, classes, name):
    """One packet per enqueue the reference's counters saw for the frame, on those ports; none for a tail drop or
    an egress deny."""
    got = outcome(host, len(fx.frames))
    idx = np.flatnonzero(classes[name])
    assert len(idx) >= 3
    for i in idx:
        i = int(i)
        ev = events_of(fx.z, i)
        assert [p for p, _ in got[i]] == sorted(p for k, p, _ in ev if k == EV_ENQ), f"{name}: frame {i} -> {got[i]}, events {ev}"
        if name == "flood, one copy denied and one popped":
            assert any(k == EV_EDENY for k, _, _ in ev) and any(ln == len(fx.frames[i]) - 4 for _, ln in got[i])
        if name == "tail drop of a flood copy":
            assert any(k == EV_FULL for k, _, _ in ev)
        if name == "long tagged frame popped":
            assert any(ln == len(fx.frames[i]) - 4 for _, ln in got[i])


def test_l3_forward_rewrites_ttl_macs_and_checksums(fx, host):
    """The bytes of a forwarded packet: TTL one less, the next hop's and the interface's MACs, and an IPv4 header
    that sums to 0xFFFF (the frames arrive with zero checksums)."""
    z = fx.z
    mac_of = {int(i): bytes(m) for i, m in zip(z["if_id"], z["if_mac"])}
    arp = {bytes(m) for m in z["arp_mac"]}
    seen = 0
    for tx in host["tx"]:
        for p, pkts in tx.items():
            for s, data in pkts:
                if z["code"][s] != C_L3_FWD:
                    continue
                f = fx.frames[s]
                l2_in, l2 = (18 if f[12:14] == b"\x81\x00" else 14), (18 if data[12:14] == b"\x81\x00" else 14)
                assert data[l2 + 8] == f[l2_in + 8] - 1 and data[6:12] == mac_of[p] and data[0:6] in arp, s
                hdr = data[l2:l2 + 4 * (data[l2] & 15)]
                total = sum(int.from_bytes(hdr[k:k + 2], "big") for k in range(0, len(hdr), 2))
                assert (total & 0xFFFF) + (total >> 16) == 0xFFFF, s
                seen += 1
    assert seen > 300


def test_ingress_deny_counts(fx, host):
    """rx_drops grows by the denied frames and the redirects to a bad port, nothing else."""
    z = fx.z
    for b, (ingress, lo, frames, _) in enumerate(fx.bursts):
        code = z["code"][lo:lo + len(frames)]
        assert host["rx_drops"][b] == int(np.isin(code, [C_IN_DENY, C_RED_DOWN, C_RED_RANGE]).sum())
