"""CPU tests of the egress ACLs (nfcs_aclset_*, nfcs_egress_acl_host): the per-port decision and the deny
counters against what the reference's egress pipeline did with the fixture's (frame, egress port) pairs
(tests/golden/egress_acl_ref.npz, made by tests/golden/make_egress_acl_golden.py from AclManager,
InterfaceManager, VlanManager and QosManager), against acl_common.model_eval applied per list, the commit's
layout and limits, and the argument errors. No GPU: the set is host code until nfcs_aclset_upload."""
import os
import subprocess

import numpy as np
import pytest

import netflow_amd as nf
from acl_common import rule
from egress_acl_common import (NONE, Fixture, host_decision, marked_lists, model_per_list, pack, udp_frame,
                               want_marked)

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def test_abi_version_unchanged_and_symbols_present():
    L = nf.lib()
    assert L.nfcs_abi_version() == 2
    for name in ("nfcs_aclset_create", "nfcs_aclset_destroy", "nfcs_aclset_set_list", "nfcs_aclset_remove_list",
                 "nfcs_aclset_bind_port", "nfcs_aclset_clear", "nfcs_aclset_commit", "nfcs_aclset_upload",
                 "nfcs_aclset_info", "nfcs_aclset_eval_host", "nfcs_egress_acl_device", "nfcs_egress_acl_host"):
        assert hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "nfcs.h")).read()
    assert "#define NFCS_ABI_VERSION 2" in hdr
    assert "#define NFCS_ACLSET_MAX_LISTS 128u" in hdr and nf.ACLSET_MAX_LISTS == 128
    assert "#define NFCS_ACL_LIST_NONE 0xFFFFFFFFu" in hdr and nf.ACL_LIST_NONE == 0xFFFFFFFF
    assert "#define NFCS_ACL_NO_PORT 4u" in hdr and nf.ACL_NO_PORT == 4
    assert "#define NFCS_L2_MAX_PORTS 1024u" in hdr


def test_fixture_covers_what_it_should(fx):
    """What the generator asserted, seen from here: every kind of port, pops that matter, tail drops."""
    z = fx.z
    assert 3000 <= len(fx.port) <= 6000
    assert (z["action"] == nf.ACL_REDIRECT).sum() >= 20 and (z["enqueued"][z["action"] == nf.ACL_REDIRECT] == 1).all()
    assert (z["action_unpopped"] != z["action"]).sum() >= 20
    for port in (4, 5, 6):
        assert fx.list_of(port) is None and (fx.port == port).sum() >= 20
    assert fx.bound[0] == fx.bound[2]
    assert (z["stats"][:, :, 1][z["stats"][:, :, 0] != NONE] > 0).any()


def test_eval_host_matches_reference(fx):
    with fx.aclset() as s:
        action, first, port = host_decision(s, fx.port, fx.frames)
    assert np.array_equal(action, fx.z["action"])
    assert np.array_equal(first, fx.z["rule"])
    assert np.array_equal(port, fx.z["redirect"])


def test_egress_acl_host_matches_reference_with_counters(fx):
    arena, desc = pack(fx.frames)
    with fx.aclset() as s:
        ports, lists, padded = s.info()
        assert ports == 8 and lists == 4 and padded == 24 + 28 + 8 + 4
        pk, by = np.zeros(ports, np.uint32), np.zeros(ports, np.uint64)
        out = s.egress_acl_host(arena, desc, fx.port, pk, by)
    assert np.array_equal(out["action"], fx.z["action"])
    assert np.array_equal(out["rule"], fx.z["rule"])
    assert np.array_equal(out["redirect"], fx.z["redirect"])
    assert np.array_equal(out["port"], np.where(fx.z["action"] == nf.ACL_DENY, NONE, fx.port))
    drops, nbytes = fx.denied_counters()  # tx_drops (= tx_packets) and tx_bytes of get_port_stats
    assert np.array_equal(pk, drops[:ports]) and np.array_equal(by, nbytes[:ports])
    assert not drops[ports:].any()


def test_unpopped_frames_give_the_unpopped_answer(fx):
    """The call must see the frame as the VLAN stage left it: on the frames before the pop the library gives
    what the reference gives on its un-popped copy, which differs."""
    with fx.aclset() as s:
        action, _, _ = host_decision(s, fx.port, fx.frames_in)
    assert np.array_equal(action, fx.z["action_unpopped"])


def test_per_list_numpy_model_matches_reference_and_library(fx):
    action, first, port = model_per_list(fx.port, fx.frames, fx.list_of)
    assert np.array_equal(action, fx.z["action"])
    assert np.array_equal(first, fx.z["rule"])
    assert np.array_equal(port, fx.z["redirect"])


def test_ports_without_a_list_permit():
    deny_all = rule(action=nf.ACL_DENY)
    f = udp_frame(1)
    with nf.AclSet() as s:
        s.set_list(0, deny_all).set_list(1, np.zeros(0, nf.ACL_RULE_DTYPE)).set_list(2, deny_all)
        s.bind_port(0, 0).bind_port(1, 1).bind_port(2, 2).bind_port(3, 77).bind_port(6, 0).remove_list(2).commit()
        assert s.info() == (7, 1, 4)  # the shared list lies once
        assert s.eval_host(0, f) == (nf.ACL_DENY, 0, NONE) and s.eval_host(6, f) == (nf.ACL_DENY, 0, NONE)
        for port in (1, 2, 3, 4, 5, 7, 1023, 5000):  # empty, removed, never set, unbound x2, past `ports`
            assert s.eval_host(port, f) == (nf.ACL_PERMIT, nf.ACL_NO_MATCH, NONE), port
        s.bind_port(6, nf.ACL_LIST_NONE).commit()
        assert s.info() == (4, 1, 4) and s.eval_host(6, f) == (nf.ACL_PERMIT, nf.ACL_NO_MATCH, NONE)
        s.set_list(2, deny_all).commit()  # the binding stayed: the list is back
        assert s.eval_host(2, f) == (nf.ACL_DENY, 0, NONE) and s.info() == (4, 2, 8)
        s.clear().commit()
        assert s.info() == (0, 0, 0) and s.eval_host(0, f) == (nf.ACL_PERMIT, nf.ACL_NO_MATCH, NONE)


def test_rule_index_counts_inside_the_ports_list():
    lengths = [1, 3, 4, 5, 9]
    lists = marked_lists(lengths)
    with nf.AclSet() as s:
        for k, r in enumerate(lists):
            s.set_list(10 + k, r).bind_port(k, 10 + k)
        s.commit()
        assert s.info() == (5, 5, 4 + 4 + 4 + 8 + 12)
        for k, ln in enumerate(lengths):
            assert s.eval_host(k, udp_frame(k)) == want_marked(k, ln), k


def test_commit_limits():
    never = rule(action=nf.ACL_DENY, src_ip=0x7F000001)
    with nf.AclSet() as s:
        s.set_list(0, np.concatenate([never] * 509)).set_list(5, never).bind_port(0, 0).bind_port(1, 5)
        with pytest.raises(nf.NfcsError):  # 512 + 4 padded
            s.commit()
        L = nf.lib()
        assert L.nfcs_aclset_commit(s.ptr) == EINVAL
        s.set_list(0, np.concatenate([never] * 505))  # 508 + 4: exactly 512 padded
        last = rule(action=nf.ACL_REDIRECT, redirect_port=9)
        s.set_list(5, last).commit()
        assert s.info() == (2, 2, 512)
        assert s.eval_host(1, udp_frame(3)) == (nf.ACL_REDIRECT, 0, 9)
        assert s.eval_host(0, udp_frame(3)) == (nf.ACL_PERMIT, nf.ACL_NO_MATCH, NONE)
        s.set_list(0, np.concatenate([never] * 505 + [never] * 4))  # 509 rules pad to 512: 516 again
        assert L.nfcs_aclset_commit(s.ptr) == EINVAL


def test_argument_errors():
    L = nf.lib()
    r = rule(action=nf.ACL_DENY)
    with nf.AclSet() as s:
        assert L.nfcs_aclset_set_list(s.ptr, 128, r.ctypes.data, 1) == EINVAL
        assert L.nfcs_aclset_set_list(s.ptr, 127, r.ctypes.data, 1) == 0
        assert L.nfcs_aclset_remove_list(s.ptr, 128) == EINVAL
        assert L.nfcs_aclset_bind_port(s.ptr, 1024, 0) == EINVAL
        assert L.nfcs_aclset_bind_port(s.ptr, 1023, 127) == 0
        assert L.nfcs_aclset_bind_port(s.ptr, 0, 128) == EINVAL
        assert L.nfcs_aclset_set_list(s.ptr, 0, None, 1) == EINVAL
        many = np.concatenate([r] * 513)
        assert L.nfcs_aclset_set_list(s.ptr, 0, many.ctypes.data, 513) == EINVAL
        bad = r.copy()
        bad["fields"] = 0x200
        assert L.nfcs_aclset_set_list(s.ptr, 0, bad.ctypes.data, 1) == EINVAL
        bad = r.copy()
        bad["action"] = 3
        assert L.nfcs_aclset_set_list(s.ptr, 0, bad.ctypes.data, 1) == EINVAL
        # before the first commit the host calls refuse
        a = nf._u32()
        assert L.nfcs_aclset_eval_host(s.ptr, 0, None, 0, a, None, None) == EINVAL
        assert L.nfcs_aclset_info(s.ptr, None, None, None) == EINVAL
        s.commit()
        assert s.info() == (1024, 1, 4) and s.eval_host(1023, udp_frame(0))[0] == nf.ACL_DENY
        # every setter invalidates the commit
        for setter in (lambda: s.set_list(3, r), lambda: s.remove_list(3), lambda: s.bind_port(2, 3), lambda: s.clear()):
            s.commit()
            setter()
            assert L.nfcs_aclset_eval_host(s.ptr, 0, None, 0, a, None, None) == EINVAL
            arena, desc = pack([udp_frame(0)])
            with pytest.raises(nf.NfcsError):
                s.egress_acl_host(arena, desc, np.zeros(1, np.uint32))
        s.commit()
        arena, desc = pack([udp_frame(0)])
        with pytest.raises(nf.NfcsError):  # one counter array without the other
            s.egress_acl_host(arena, desc, np.zeros(1, np.uint32), np.zeros(4, np.uint32), None)
        assert L.nfcs_egress_acl_host(s.ptr, None, 0, None, 0, None, None, None, None, None, None) == 0  # n == 0
    assert L.nfcs_aclset_create(None) == EINVAL and L.nfcs_aclset_destroy(None) == EINVAL


def test_host_burst_no_port_and_bad_descriptors():
    frames = [udp_frame(0)] * 6
    arena, desc = pack(frames)
    desc = desc.copy()
    desc[0]["off16"] = len(arena) // 16  # starts at the arena's end
    desc[5]["len"] = 200                 # reaches past it
    desc[2] = (0x0FFFFFFF, 0xFFFFFFF0)   # garbage, but no port: not looked at
    port = np.array([0, 0, NONE, 1, 9, 0], np.uint32)
    with nf.AclSet() as s:
        s.set_list(0, rule(action=nf.ACL_DENY)).bind_port(0, 0).commit()
        pk, by = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
        out = s.egress_acl_host(arena, desc, port, pk, by)
    assert list(out["action"]) == [nf.ACL_BAD_DESC, nf.ACL_DENY, nf.ACL_NO_PORT, nf.ACL_PERMIT, nf.ACL_PERMIT,
                                   nf.ACL_BAD_DESC]
    assert list(out["port"]) == [NONE, NONE, NONE, 1, 9, NONE]
    assert list(out["rule"]) == [NONE, 0, NONE, NONE, NONE, NONE] and (out["redirect"] == NONE).all()
    assert pk[0] == 1 and by[0] == len(frames[1])


def test_aclset_compile_standalone_under_host_sanitizers(tmp_path):
    """Commit and decision as a stand-alone host program (its own main, no HIP, nothing loaded into Python)
    under AddressSanitizer + UBSan, checked against a direct walk of each port's list."""
    exe = str(tmp_path / "aclset_compile_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "netflow_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "aclset_compile_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "aclset compile OK" in r.stdout


def test_cpp_make_acl_set_host_only(tmp_path):
    """netflow_amd::make_acl_set_from (packet.hpp; what netflow_adapter.hpp's make_acl_set forwards to) over
    stand-in structs: compiled with g++ against the C ABI and run on the host, no GPU."""
    if not os.path.exists(nf.LIB_PATH):
        nf.build()
    exe, libdir = str(tmp_path / "make_aclset_test"), os.path.dirname(nf.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "make_aclset_test.cpp"), "-o", exe, "-L" + libdir,
                    "-l:" + os.path.basename(nf.LIB_PATH), "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "make_acl_set OK" in r.stdout
