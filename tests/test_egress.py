"""CPU tests of the egress stage's host side (nfcs_egress: set_port, commit, plan_host, enqueue_host)
through the C ABI: against the reference's results on the fixture (tests/golden/egress_ref.npz), against
a plain-Python restatement on random tables, the argument errors, the commit rules, and the host code as a
stand-alone program under the host sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import netflow_amd as nf
from egress_common import (Q, assert_same, egress_fixture, fixture_egress, fixture_ports, fixture_want, model_enqueue,
                           model_plan, plan_host, random_table)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return egress_fixture()


def test_plan_host_matches_reference(fx):
    z, frames = fx
    want = fixture_want(z)
    with fixture_egress(z) as eg:
        ops, queue = plan_host(eg, z["port"], frames)
        assert eg.keys() == (want["keys"] // Q, want["keys"])
    assert np.array_equal(ops, want["ops"])
    assert np.array_equal(queue, want["queue"])


def test_enqueue_host_matches_reference(fx):
    z, _ = fx
    want = fixture_want(z)
    with fixture_egress(z) as eg:
        got = eg.enqueue_host(z["port"], want["queue"], want["depth0"])
    assert_same(got, want)
    assert (got["result"] == nf.EQ_DROP_FULL).sum() == want["key_dropped"].sum() > 0


def test_argument_errors():
    L = nf.lib()
    assert L.nfcs_egress_create(None) == -1
    for fn in (L.nfcs_egress_destroy, L.nfcs_egress_clear_ports, L.nfcs_egress_commit):
        assert fn(None) == -1
    eg = nf.Egress()
    rec = np.zeros(1, nf.EGRESS_PORT_DTYPE)
    assert L.nfcs_egress_set_port(None, rec.ctypes.data) == -1
    assert L.nfcs_egress_set_port(eg.ptr, None) == -1
    for field, bad, good in (("port_id", 1024, 1023), ("port_id", 0xFFFFFFFF, 0), ("type", 3, 2),
                             ("native_vlan", 4096, 4095), ("num_queues", 9, 8)):
        rec = np.zeros(1, nf.EGRESS_PORT_DTYPE)
        rec[field] = bad
        assert L.nfcs_egress_set_port(eg.ptr, rec.ctypes.data) == -1, (field, bad)
        rec[field] = good
        assert L.nfcs_egress_set_port(eg.ptr, rec.ctypes.data) == 0, (field, good)
    u = ctypes.c_uint32()
    # before the commit
    assert L.nfcs_egress_keys(eg.ptr, ctypes.byref(u), ctypes.byref(u)) == -1
    assert L.nfcs_egress_plan_host(eg.ptr, 0, None, 0, ctypes.byref(u), ctypes.byref(u)) == -1
    eg.commit()
    assert L.nfcs_egress_keys(None, None, None) == -1
    assert L.nfcs_egress_keys(eg.ptr, None, None) == 0
    assert L.nfcs_egress_plan_host(None, 0, None, 0, None, None) == -1
    assert L.nfcs_egress_plan_host(eg.ptr, 0, None, 14, None, None) == -1  # len > 0 without a frame
    assert L.nfcs_egress_plan_host(eg.ptr, 0, None, 0, None, None) == 0
    keys = eg.keys()[1]
    port, queue = np.zeros(4, np.uint32), np.zeros(4, np.uint8)
    depth, order, ks = np.zeros(keys, np.uint32), np.zeros(4, np.uint32), np.zeros(keys + 1, np.uint32)
    p = lambda a: a.ctypes.data
    assert L.nfcs_egress_enqueue_host(eg.ptr, p(port), p(queue), 4, p(depth), None, p(order), p(ks), None) == 0
    assert L.nfcs_egress_enqueue_host(None, p(port), p(queue), 4, p(depth), None, p(order), p(ks), None) == -1
    assert L.nfcs_egress_enqueue_host(eg.ptr, None, p(queue), 4, p(depth), None, p(order), p(ks), None) == -1
    assert L.nfcs_egress_enqueue_host(eg.ptr, p(port), None, 4, p(depth), None, p(order), p(ks), None) == -1
    assert L.nfcs_egress_enqueue_host(eg.ptr, p(port), p(queue), 4, None, None, p(order), p(ks), None) == -1
    assert L.nfcs_egress_enqueue_host(eg.ptr, p(port), p(queue), 4, p(depth), None, None, p(ks), None) == -1
    assert L.nfcs_egress_enqueue_host(eg.ptr, p(port), p(queue), 4, p(depth), None, p(order), None, None) == -1
    assert L.nfcs_egress_enqueue_host(eg.ptr, None, None, 0, p(depth), None, None, p(ks), None) == 0  # n == 0
    # the device entry points without a context
    assert L.nfcs_egress_upload(None, eg.ptr) == -1
    assert L.nfcs_egress_plan_device(None, eg.ptr, None, 0, None, 0, None, None, None, None, None, None, None) == -1
    assert L.nfcs_egress_enqueue_device(None, eg.ptr, None, None, 0, None, None, None, None, None, None) == -1
    eg.close()
    with pytest.raises(nf.NfcsError):
        nf.Egress().set_port(1024)
    with pytest.raises(nf.NfcsError):
        nf.Egress().set_port(0, num_queues=256)  # does not fit the record's byte


def test_zero_queues_and_zero_depth_are_read_as_one():
    """QosConfig::validate_and_prepare: num_queues 0 becomes 1, max_queue_depth 0 becomes 1."""
    tagged = bytes(12) + b"\x81\x00\xe0\x05\x88\xb5" + bytes(46)
    with nf.Egress().set_port(2, has_vlan_config=False, num_queues=0, max_queue_depth=0).commit() as eg:
        assert eg.plan_host(2, tagged) == (nf.VLAN_NOP, 0) and eg.plan_host(2, bytes(64)) == (nf.VLAN_NOP, 0)
        got = eg.enqueue_host([2, 2, 2], [0, 1, 0], np.zeros(24, np.uint32))
    assert got["result"].tolist() == [nf.EQ_ENQUEUED, nf.EQ_BAD_QUEUE, nf.EQ_DROP_FULL]
    assert got["depth"][16] == 1 and got["key_dropped"][16] == 1 and got["order"].tolist() == [0]


@pytest.mark.parametrize("setter", ["set_port", "clear_ports"])
def test_each_setter_invalidates_the_commit(setter):
    with nf.Egress().set_port(1).commit() as eg:
        assert eg.keys() == (2, 16)
        if setter == "set_port":
            eg.set_port(4)
        else:
            eg.clear_ports()
        with pytest.raises(nf.NfcsError):
            eg.keys()
        with pytest.raises(nf.NfcsError):
            eg.plan_host(1, bytes(64))
        with pytest.raises(nf.NfcsError):
            eg.enqueue_host([], [], [])
        eg.commit()
        assert eg.keys() == ((5, 40) if setter == "set_port" else (0, 0))


def test_port_never_set_and_replacement():
    native = bytes(12) + b"\x81\x00\x60\x0a\x88\xb5" + bytes(46)  # PCP 3, VLAN 10
    with nf.Egress().set_port(5, type=nf.L2_ACCESS, native_vlan=10, num_queues=8).commit() as eg:
        assert eg.keys() == (6, 48)
        assert eg.plan_host(5, native) == (nf.VLAN_POP, 7)   # popped: no PCP left, the last queue
        for unset in (0, 4, 6, 1023, 5000):                  # below, next to, above the table, above every id
            assert eg.plan_host(unset, native) == (nf.VLAN_NOP, 0)
        assert eg.plan_host(nf.IF_NONE, native) == (nf.VLAN_NOP, nf.QUEUE_NONE)
        got = eg.enqueue_host([0, 6, 5000, nf.IF_NONE, 5], [0, 0, 0, nf.QUEUE_NONE, 7], np.zeros(48, np.uint32))
        assert got["result"].tolist() == [nf.EQ_DROP_NO_CONFIG] * 3 + [nf.EQ_SKIP, nf.EQ_ENQUEUED]
        assert got["key_start"][47] == 0 and got["key_start"][48] == 1 and got["order"].tolist() == [4]
        eg.set_port(5, type=nf.L2_TRUNK, tag_native=True, native_vlan=10, num_queues=8).commit()  # replaces
        assert eg.plan_host(5, native) == (nf.VLAN_NOP, 4)   # (7 - 3) * 8 / 8
        eg.clear_ports().commit()
        assert eg.keys() == (0, 0) and eg.plan_host(5, native) == (nf.VLAN_NOP, 0)
        got = eg.enqueue_host([5, nf.IF_NONE], [0, 0], [])
        assert got["result"].tolist() == [nf.EQ_DROP_NO_CONFIG, nf.EQ_SKIP] and got["key_start"].tolist() == [0]


def test_depth_above_the_cap_leaves_no_room():
    with nf.Egress().set_port(0, num_queues=2, max_queue_depth=5).commit() as eg:
        depth = np.zeros(8, np.uint32)
        depth[0], depth[1] = 9, 3
        got = eg.enqueue_host([0] * 6, [0, 1, 1, 1, 0, 1], depth)
    assert got["result"].tolist() == [nf.EQ_DROP_FULL, 0, 0, nf.EQ_DROP_FULL, nf.EQ_DROP_FULL, nf.EQ_DROP_FULL]
    assert got["depth"][:2].tolist() == [9, 5] and got["key_dropped"][:2].tolist() == [2, 2]
    assert got["order"].tolist() == [1, 2] and got["key_start"][:3].tolist() == [0, 0, 2]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_matches_plain_python_restatement(fx, seed):
    z, frames = fx
    rng = np.random.default_rng(700 + seed)
    nports = (12, 40, 3)[seed - 1]
    eg, cfg = random_table(rng, nports)
    n = 3000
    sel = rng.integers(0, len(frames), n)
    port = rng.integers(0, nports + 2, n).astype(np.uint32)
    port[rng.random(n) < 0.05] = nf.IF_NONE
    with eg:
        ports, keys = eg.keys()
        assert keys == ports * Q and ports == (max(cfg) + 1 if cfg else 0)
        ops, queue = plan_host(eg, port, [frames[i] for i in sel])
        want = [model_plan(cfg, int(p), frames[i]) for p, i in zip(port, sel)]
        assert ops.tolist() == [w[0] for w in want]
        assert queue.tolist() == [w[1] for w in want]
        bad = rng.random(n) < 0.05
        queue[bad] = rng.integers(0, 12, int(bad.sum()))
        depth = rng.integers(0, 9, keys).astype(np.uint32)
        got = eg.enqueue_host(port, queue, depth)
        assert_same(got, model_enqueue(cfg, keys, port, queue, depth))
        again = eg.enqueue_host(port, queue, got["depth"])  # a second burst chained on the first one's depths
        assert_same(again, model_enqueue(cfg, keys, port, queue, got["depth"]))
    assert set(got["result"].tolist()) == {0, 1, 2, 3, 4}


def test_fixture_ports_cover_the_cases(fx):
    z, _ = fx
    p = fixture_ports(z)
    assert {0, 1, 2} == set(p["type"].tolist()) and {0, 1, 3, 4, 8} <= set(p["num_queues"].tolist())
    assert (p["has_vlan_config"] == 0).any() and (p["has_qos"] == 0).any() and (p["max_queue_depth"] == 0).any()
    assert 8 not in p["port_id"].tolist() and (z["port"] == 8).sum() > 20  # frames leave through a port never set


def test_egress_compile_standalone_under_host_sanitizers(tmp_path):
    """The compile step, the plan and the enqueue as a stand-alone host program (its own main, no HIP,
    nothing loaded into Python) under AddressSanitizer + UBSan, frames in heap blocks of their exact length."""
    exe = str(tmp_path / "egress_compile_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "netflow_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "egress_compile_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "egress compile OK" in r.stdout


def test_python_constants_match_the_header():
    import re
    hdr = open(os.path.join(ROOT, "include", "nfcs.h")).read()
    for name, value in (("NFCS_QOS_MAX_QUEUES", nf.QOS_MAX_QUEUES), ("NFCS_QUEUE_NONE", nf.QUEUE_NONE),
                        ("NFCS_EGRESS_TILE_PKTS", nf.EGRESS_TILE_PKTS)):
        m = re.search(r"#define\s+" + name + r"\s+(0x[0-9A-Fa-f]+|\d+)u", hdr)
        assert m and int(m.group(1), 0) == value, name
    for k, name in enumerate(("ENQUEUED", "SKIP", "DROP_NO_CONFIG", "DROP_FULL", "BAD_QUEUE")):
        assert re.search(r"NFCS_EQ_" + name + r"\s*=\s*" + str(k) + r"\b", hdr) and getattr(nf, "EQ_" + name) == k
