"""CPU tests of the forwarding table (nfcs_fib_*): the compile step and the one-address decision
against what the reference decides on the fixture frames (tests/golden/route_ref.npz, made by
tests/golden/make_route_golden.py from RoutingManager and the Packet accessors), and the argument
errors. No GPU: the table is host code until nfcs_fib_upload."""
import ctypes

import numpy as np
import pytest

import netflow_amd as nf
from route_common import TABLES, decide_host, fixture_fib, make_fib, route_fixture

EINVAL = -1


@pytest.fixture(scope="module")
def fx():
    return route_fixture()


def test_fixture_covers_every_verdict(fx):
    z, frames = fx
    seen = set()
    for t in TABLES:
        v = z["verdict_" + t]
        seen |= set(int(x) for x in v)
        assert (v == nf.RT_FORWARD).mean() >= 0.25, t
    # BAD_DESC is about arenas, not frames: the GPU tests make those
    assert seen == {nf.RT_FORWARD, nf.RT_NOT_IPV4, nf.RT_LOCAL, nf.RT_TTL_EXPIRED, nf.RT_NO_ROUTE,
                    nf.RT_ARP_MISS, nf.RT_NO_IF_MAC}
    lens = set(int(x) for x in z["lens"])
    assert {13, 14, 17, 33, 34, 37, 38} <= lens and max(lens) <= 64


@pytest.mark.parametrize("table", TABLES)
def test_lookup_host_matches_reference(fx, table):
    z, frames = fx
    with fixture_fib(z, table) as fib:
        v, nh, eif = decide_host(fib, frames)
        nht = fib.nexthops_host()
    assert np.array_equal(v, z["verdict_" + table])
    assert np.array_equal(eif, z["egress_" + table])
    fwd = v == nf.RT_FORWARD
    assert (nh[~fwd] == nf.NH_NONE).all() and (nh[fwd] < len(nht)).all()
    got = np.concatenate([nht["dst_mac"][nh[fwd]], nht["src_mac"][nh[fwd]]], axis=1)
    assert np.array_equal(got, z["macs_" + table][fwd])


def test_next_hop_table_shape(fx):
    z, _ = fx
    with fixture_fib(z, "a") as fib:
        nht = fib.nexthops_host()
    # one entry per distinct ARP address, then one per gateway route whose gateway and interface resolve
    arps = len(set(int(x) for x in z["arp_ip"]))
    assert arps < len(nht) <= arps + int((z["routes_a"][:, 2] != 0).sum())


def test_argument_errors():
    L = nf.lib()
    fib = nf.Fib()
    v = ctypes.c_uint32()
    # lookup and table before commit
    assert L.nfcs_fib_lookup_host(fib.ptr, 1, 64, ctypes.byref(v), None, None) == EINVAL
    assert L.nfcs_fib_nexthops_host(fib.ptr, None, 0, ctypes.byref(v)) == EINVAL
    # null with n > 0
    for fn in (L.nfcs_fib_set_routes, L.nfcs_fib_set_arp, L.nfcs_fib_set_if_macs, L.nfcs_fib_set_local_ips):
        assert fn(fib.ptr, None, 1) == EINVAL
        assert fn(None, None, 0) == EINVAL
        assert fn(fib.ptr, None, 0) == 0
    # too many routes
    r = np.zeros(nf.FIB_MAX_ROUTES + 1, dtype=nf.FIB_ROUTE_DTYPE)
    assert L.nfcs_fib_set_routes(fib.ptr, r.ctypes.data, len(r)) == EINVAL
    assert L.nfcs_fib_set_routes(fib.ptr, r.ctypes.data, nf.FIB_MAX_ROUTES) == 0
    assert L.nfcs_fib_commit(fib.ptr) == 0
    assert L.nfcs_fib_lookup_host(fib.ptr, 1, 64, ctypes.byref(v), None, None) == 0
    # a setter invalidates the commit
    assert L.nfcs_fib_set_local_ips(fib.ptr, None, 0) == 0
    assert L.nfcs_fib_lookup_host(fib.ptr, 1, 64, ctypes.byref(v), None, None) == EINVAL
    # the device side needs a context and an upload
    assert L.nfcs_fib_upload(None, fib.ptr) == EINVAL
    assert L.nfcs_fib_nexthops(fib.ptr, ctypes.byref(ctypes.c_void_p()), ctypes.byref(v)) == EINVAL
    assert L.nfcs_route_lookup_device(None, fib.ptr, None, 0, None, 0, None, None, None, None) == EINVAL
    assert L.nfcs_fib_create(None) == EINVAL and L.nfcs_fib_destroy(None) == EINVAL and L.nfcs_fib_commit(None) == EINVAL
    fib.close()


def test_empty_tables():
    with make_fib(np.zeros((0, 4), np.uint32), [], np.zeros((0, 6), np.uint8), [], np.zeros((0, 6), np.uint8), []) as fib:
        assert len(fib.nexthops_host()) == 0
        assert fib.lookup_host(nf.ip4("10.0.0.1"), 64) == (nf.RT_NO_ROUTE, nf.NH_NONE, nf.IF_NONE)
        assert fib.lookup_host(nf.ip4("10.0.0.1"), 1) == (nf.RT_TTL_EXPIRED, nf.NH_NONE, nf.IF_NONE)
        assert fib.lookup_host(0, 0)[0] == nf.RT_TTL_EXPIRED


def test_duplicate_arp_entries_last_wins():
    ip = nf.ip4
    routes = [[ip("10.0.0.0"), ip("255.0.0.0"), 0, 1], [0, 0, ip("10.0.0.9"), 2]]
    arp_ip = [ip("10.0.0.9"), ip("10.0.0.7"), ip("10.0.0.9"), ip("10.0.0.7"), ip("10.0.0.9")]
    arp_mac = np.array([[k] * 6 for k in (1, 2, 3, 4, 5)], np.uint8)
    with make_fib(routes, arp_ip, arp_mac, [1, 2, 1], np.array([[0xA1] * 6, [0xA2] * 6, [0xB1] * 6], np.uint8), []) as fib:
        nht = fib.nexthops_host()
        assert len(nht) == 3  # two distinct addresses and the gateway route
        for dst, dmac, smac, eif in ((ip("10.0.0.7"), 4, 0xB1, 1), (ip("10.0.0.9"), 5, 0xB1, 1), (ip("8.8.8.8"), 5, 0xA2, 2)):
            v, nh, e = fib.lookup_host(dst, 9)
            assert (v, e) == (nf.RT_FORWARD, eif)
            assert bytes(nht["dst_mac"][nh]) == bytes([dmac] * 6) and bytes(nht["src_mac"][nh]) == bytes([smac] * 6)
        assert fib.lookup_host(ip("10.0.0.8"), 9) == (nf.RT_ARP_MISS, nf.NH_NONE, nf.IF_NONE)


def test_first_match_wins_in_given_order():
    ip = nf.ip4
    # the order is the caller's: a /8 in front of a /24 shadows it (the reference's sort is not redone)
    routes = [[ip("10.0.0.0"), ip("255.0.0.0"), 0, 1], [ip("10.1.2.0"), ip("255.255.255.0"), 0, 2]]
    macs = np.array([[7] * 6], np.uint8)
    ifm = np.array([[1] * 6, [2] * 6], np.uint8)
    with make_fib(routes, [ip("10.1.2.3")], macs, [1, 2], ifm, []) as fib:
        assert fib.lookup_host(ip("10.1.2.3"), 5)[2] == 1
    with make_fib(routes[::-1], [ip("10.1.2.3")], macs, [1, 2], ifm, []) as fib:
        assert fib.lookup_host(ip("10.1.2.3"), 5)[2] == 2


def test_fib_compile_standalone_under_host_sanitizers(tmp_path):
    """The compile step and the decision as a stand-alone host program (its own main, no HIP, nothing
    loaded into Python) under AddressSanitizer + UBSan, checked against a direct walk of the inputs."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "fib_compile_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "netflow_amd", "csrc"),
                    os.path.join(root, "tests", "cpp", "fib_compile_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fib compile OK" in r.stdout


def test_cpp_make_fib_host_only(tmp_path):
    """netflow_amd::make_fib_from (packet.hpp; what netflow_adapter.hpp's make_fib forwards to) over a
    stand-in routing table: compiled with g++ against the C ABI and run on the host, no GPU."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(nf.LIB_PATH):
        nf.build()
    exe, libdir = str(tmp_path / "make_fib_test"), os.path.dirname(nf.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "make_fib_test.cpp"), "-o", exe, "-L" + libdir,
                    "-l:" + os.path.basename(nf.LIB_PATH), "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "make_fib OK" in r.stdout
