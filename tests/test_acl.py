"""CPU tests of the ACL rule list (nfcs_acl_*): the compile step and the one-frame decision against what
the reference decides on the fixture frames (tests/golden/acl_ref.npz, made by
tests/golden/make_acl_golden.py from AclManager and the Packet accessors), against a numpy restatement
of check_match (also with address masks, which the reference does not have), and the argument errors.
No GPU: the list is host code until nfcs_acl_upload."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import netflow_amd as nf
from acl_common import LISTS, acl_fixture, eval_host, fixture_rules, make_acl, model_eval, rule

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return acl_fixture()


def test_abi_version_unchanged_and_symbols_present():
    L = nf.lib()
    assert L.nfcs_abi_version() == 2
    for name in ("nfcs_acl_create", "nfcs_acl_destroy", "nfcs_acl_set_rules", "nfcs_acl_commit", "nfcs_acl_upload",
                 "nfcs_acl_eval_host", "nfcs_acl_eval_device"):
        assert hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "nfcs.h")).read()
    assert "#define NFCS_ABI_VERSION 2" in hdr
    assert f"sizeof(nfcs_acl_rule) == {nf.ACL_RULE_DTYPE.itemsize}" in hdr
    for name, value in (("NFCS_ACL_PERMIT", 0), ("NFCS_ACL_DENY", 1), ("NFCS_ACL_REDIRECT", 2), ("NFCS_ACL_BAD_DESC", 3),
                        ("NFCS_ACL_MAX_RULES", nf.ACL_MAX_RULES)):
        assert f"#define {name} {value}u" in hdr, name
    assert nf.ACL_GROUP == int(open(os.path.join(ROOT, "netflow_amd", "csrc", "nfcs_acl.h")).read()
                               .split("constexpr uint32_t kAclGroup = ")[1].split(";")[0])


def test_fixture_covers_what_it_should(fx):
    z, frames = fx
    assert 1000 <= len(frames) <= 1500 and max(len(f) for f in frames) <= 128
    lens = set(len(f) for f in frames)
    assert {13, 14, 17, 18, 33, 34, 37, 38, 41, 42, 52, 53} <= lens  # l2+19/20, l4+7/8, l4+18/19 at IHL 5
    for name in LISTS:
        rules = fixture_rules(z, name)
        action, first = z["action_" + name], z["rule_" + name]
        hit = first != nf.ACL_NO_MATCH
        assert set(first[hit].tolist()) == set(range(len(rules))), name  # every rule decides somewhere
        assert max((action == a).mean() for a in (0, 1, 2)) <= 0.60
        assert set(action.tolist()) == {nf.ACL_PERMIT, nf.ACL_DENY, nf.ACL_REDIRECT}
        # a REDIRECT rule without a port decided DENY somewhere
        noport = (rules["action"] == nf.ACL_REDIRECT) & (rules["redirect_port"] == nf.IF_NONE)
        assert noport.any() and (action[hit][noport[first[hit]]] == nf.ACL_DENY).all() and noport[first[hit]].any()
    assert 0.10 <= (z["rule_a"] == nf.ACL_NO_MATCH).mean() <= 0.50
    assert not (z["rule_b"] == nf.ACL_NO_MATCH).any()  # its last rule has no match fields
    # c is a's rules in another order, and the order changes decisions
    ids_a, ids_c = fixture_rules(z, "a")["rule_id"], fixture_rules(z, "c")["rule_id"]
    assert sorted(ids_a) == sorted(ids_c) and list(ids_a) != list(ids_c)
    assert (ids_a[z["rule_a"][z["rule_a"] != nf.ACL_NO_MATCH]] != ids_c[z["rule_c"][z["rule_c"] != nf.ACL_NO_MATCH]]).any()


@pytest.mark.parametrize("name", LISTS)
def test_eval_host_matches_reference(fx, name):
    z, frames = fx
    with make_acl(fixture_rules(z, name)) as acl:
        action, first, port = eval_host(acl, frames)
    assert np.array_equal(action, z["action_" + name])
    assert np.array_equal(first, z["rule_" + name])
    assert np.array_equal(port, z["redirect_" + name])


@pytest.mark.parametrize("name", LISTS)
def test_numpy_model_matches_reference(fx, name):
    z, frames = fx
    action, first, port = model_eval(fixture_rules(z, name), frames)
    assert np.array_equal(action, z["action_" + name])
    assert np.array_equal(first, z["rule_" + name])
    assert np.array_equal(port, z["redirect_" + name])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_address_masks_match_numpy_model(fx, seed):
    """The extension the reference cannot pin: (ntohl(address) & mask) == (rule address & mask), with
    random masks on every address rule of list a. Pinned against the numpy model, on the fixture frames."""
    z, frames = fx
    rng = np.random.default_rng(seed)
    rules = fixture_rules(z, "a")
    masks = np.array([0xFFFFFFFF, 0xFFFFFF00, 0xFFFF0000, 0xFF000000, 0x00000000, 0xFFFF00FF, 0x0000FFFF], np.uint32)
    rules["src_ip_mask"] = np.where(rng.random(len(rules)) < 0.2, rng.integers(0, 1 << 32, len(rules), dtype=np.uint64),
                                    masks[rng.integers(0, len(masks), len(rules))])
    rules["dst_ip_mask"] = masks[rng.integers(0, len(masks), len(rules))]
    want = model_eval(rules, frames)
    with make_acl(rules) as acl:
        got = eval_host(acl, frames)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert not np.array_equal(want[1], z["rule_a"])  # the masks changed decisions


def test_address_mask_semantics():
    ip = lambda a: int.from_bytes(bytes(int(x) for x in a.split(".")), "big")  # noqa: E731  host order

    def udp(src, dst, length=60):
        b = bytearray(60)
        b[12:14] = b"\x08\x00"
        b[14], b[23] = 0x45, 17
        b[26:30], b[30:34] = ip(src).to_bytes(4, "big"), ip(dst).to_bytes(4, "big")
        return bytes(b[:length])

    rules = np.concatenate([rule(nf.ACL_DENY, src_ip=ip("10.1.2.99"), src_ip_mask=0xFFFFFF00),   # 10.1.2.0/24
                            rule(nf.ACL_REDIRECT, 5, dst_ip=ip("1.2.3.4"), dst_ip_mask=0)])       # any IPv4 header
    with make_acl(rules) as acl:
        assert acl.eval_host(udp("10.1.2.3", "9.9.9.9")) == (nf.ACL_DENY, 0, nf.IF_NONE)
        assert acl.eval_host(udp("10.1.3.3", "9.9.9.9")) == (nf.ACL_REDIRECT, 1, 5)
        assert acl.eval_host(udp("10.1.3.3", "9.9.9.9", 33)) == (nf.ACL_PERMIT, nf.ACL_NO_MATCH, nf.IF_NONE)  # no ipv4()
        arp = bytearray(udp("10.1.3.3", "9.9.9.9"))
        arp[12:14] = b"\x08\x06"
        assert acl.eval_host(bytes(arp))[0] == nf.ACL_PERMIT  # mask 0 still needs EtherType 0x0800


def test_rule_without_fields_matches_every_frame():
    """Checked against the compiled reference when the fixture was designed: a rule with no fields
    matches a 10-byte frame and a tagged 16-byte frame; one that names the EtherType matches neither."""
    tagged16 = bytes(12) + b"\x81\x00\x00\x0a"
    with make_acl(rule(nf.ACL_DENY)) as acl:
        for f in (b"", bytes(10), tagged16, bytes(64)):
            assert acl.eval_host(f) == (nf.ACL_DENY, 0, nf.IF_NONE)
    with make_acl(rule(nf.ACL_DENY, ethertype=0)) as acl:
        assert acl.eval_host(bytes(10))[0] == nf.ACL_PERMIT
        assert acl.eval_host(tagged16)[0] == nf.ACL_PERMIT  # tagged without a VLAN header: no EtherType
        assert acl.eval_host(bytes(14))[0] == nf.ACL_DENY   # EtherType 0 is a value like any other


def test_redirect_without_port_stops_the_scan():
    rules = np.concatenate([rule(nf.ACL_REDIRECT), rule(nf.ACL_PERMIT), rule(nf.ACL_REDIRECT, 9)])
    with make_acl(rules) as acl:
        assert acl.eval_host(bytes(64)) == (nf.ACL_DENY, 0, nf.IF_NONE)
    with make_acl(rules[::-1]) as acl:
        assert acl.eval_host(bytes(64)) == (nf.ACL_REDIRECT, 0, 9)


def test_first_match_wins_in_given_order():
    a, b = rule(nf.ACL_DENY, protocol=17, rule_id=1), rule(nf.ACL_PERMIT, ethertype=0x0800, rule_id=2)
    f = bytearray(60)
    f[12:14], f[14], f[23] = b"\x08\x00", 0x45, 17
    with make_acl(np.concatenate([a, b])) as acl:
        assert acl.eval_host(bytes(f))[:2] == (nf.ACL_DENY, 0)
    with make_acl(np.concatenate([b, a])) as acl:  # the order is the caller's, whatever the ids or a sort would say
        assert acl.eval_host(bytes(f))[:2] == (nf.ACL_PERMIT, 0)


def test_argument_errors():
    L = nf.lib()
    acl = nf.Acl()
    v = ctypes.c_uint32()
    frame = bytes(64)
    # eval before commit
    assert L.nfcs_acl_eval_host(acl.ptr, frame, 64, ctypes.byref(v), None, None) == EINVAL
    # null with n > 0, null objects
    assert L.nfcs_acl_set_rules(acl.ptr, None, 1) == EINVAL
    assert L.nfcs_acl_set_rules(None, None, 0) == EINVAL
    assert L.nfcs_acl_set_rules(acl.ptr, None, 0) == 0
    # too many rules
    r = np.zeros(nf.ACL_MAX_RULES + 1, dtype=nf.ACL_RULE_DTYPE)
    assert L.nfcs_acl_set_rules(acl.ptr, r.ctypes.data, len(r)) == EINVAL
    assert L.nfcs_acl_set_rules(acl.ptr, r.ctypes.data, nf.ACL_MAX_RULES) == 0
    # an action or a field bit the header does not define
    bad = np.zeros(2, dtype=nf.ACL_RULE_DTYPE)
    bad[1]["action"] = 3
    assert L.nfcs_acl_set_rules(acl.ptr, bad.ctypes.data, 2) == EINVAL
    bad[1]["action"], bad[1]["fields"] = 0, 0x200
    assert L.nfcs_acl_set_rules(acl.ptr, bad.ctypes.data, 2) == EINVAL
    assert L.nfcs_acl_commit(acl.ptr) == 0
    assert L.nfcs_acl_eval_host(acl.ptr, frame, 64, ctypes.byref(v), None, None) == 0
    assert L.nfcs_acl_eval_host(acl.ptr, frame, 64, None, None, None) == 0  # every out pointer may be NULL
    assert L.nfcs_acl_eval_host(acl.ptr, None, 0, ctypes.byref(v), None, None) == 0
    assert L.nfcs_acl_eval_host(acl.ptr, None, 1, ctypes.byref(v), None, None) == EINVAL
    # a setter invalidates the commit
    assert L.nfcs_acl_set_rules(acl.ptr, None, 0) == 0
    assert L.nfcs_acl_eval_host(acl.ptr, frame, 64, ctypes.byref(v), None, None) == EINVAL
    # the device side needs a context and an upload
    assert L.nfcs_acl_commit(acl.ptr) == 0
    assert L.nfcs_acl_upload(None, acl.ptr) == EINVAL
    assert L.nfcs_acl_eval_device(None, acl.ptr, None, 0, None, 0, None, None, None, None, None) == EINVAL
    assert L.nfcs_acl_create(None) == EINVAL and L.nfcs_acl_destroy(None) == EINVAL and L.nfcs_acl_commit(None) == EINVAL
    with pytest.raises(nf.NfcsError):
        nf.Acl().set_rules(r)
    acl.close()


def test_empty_list_permits_everything(fx):
    _, frames = fx
    with make_acl(np.zeros(0, dtype=nf.ACL_RULE_DTYPE)) as acl:
        action, first, port = eval_host(acl, frames[:200])
    assert (action == nf.ACL_PERMIT).all() and (first == nf.ACL_NO_MATCH).all() and (port == nf.IF_NONE).all()


def test_acl_compile_standalone_under_host_sanitizers(tmp_path):
    """The compile step and the decision as a stand-alone host program (its own main, no HIP, nothing
    loaded into Python) under AddressSanitizer + UBSan, checked against a direct walk of the rules."""
    exe = str(tmp_path / "acl_compile_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "netflow_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "acl_compile_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "acl compile OK" in r.stdout


def test_cpp_make_acl_host_only(tmp_path):
    """netflow_amd::make_acl_from (packet.hpp; what netflow_adapter.hpp's make_acl forwards to) over a
    stand-in rule struct with std::optional fields: compiled with g++ against the C ABI and run on the
    host, no GPU."""
    if not os.path.exists(nf.LIB_PATH):
        nf.build()
    exe, libdir = str(tmp_path / "make_acl_test"), os.path.dirname(nf.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "make_acl_test.cpp"), "-o", exe, "-L" + libdir,
                    "-l:" + os.path.basename(nf.LIB_PATH), "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "make_acl OK" in r.stdout
