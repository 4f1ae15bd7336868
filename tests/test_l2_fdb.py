"""CPU tests of the L2 forwarding database (nfcs_fdb): Fdb.lookup_host and Fdb.flood_ports_host against
the reference's decisions (tests/golden/l2_ref.npz), against a dict restatement on random tables, the
argument errors and commit rules of the header, duplicate keys, and the hash table's properties."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import netflow_amd as nf
from l2_common import (RUNS, WRAP_SEED_LIMIT, decide_host, entries_of, fixture_fdb, fixture_ports, frame_of,
                       l2_fixture, model_decide, random_macs, set_ports, wrapping_table)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def fx():
    return l2_fixture()


@pytest.mark.parametrize("run", RUNS)
def test_lookup_host_matches_reference(fx, run):
    z, frames = fx
    with fixture_fdb(z) as fdb:
        v, e, vl, le = decide_host(fdb, int(z["ingress"][run]), frames)
    assert np.array_equal(v, z[f"verdict_{run}"])
    assert np.array_equal(e, z[f"egress_{run}"])
    assert np.array_equal(vl, z[f"vlan_{run}"])
    assert np.array_equal(le, z[f"learn_{run}"])


@pytest.mark.parametrize("run", RUNS)
def test_flood_ports_match_reference(fx, run):
    z, _ = fx
    num_ports = int(z["num_ports"])
    with fixture_fdb(z) as fdb:
        for k, vlan in enumerate(z["flood_vlans"]):
            want = z["flood_ports"][run, k, :int(z["flood_n"][run, k])]
            got = fdb.flood_ports_host(int(z["ingress"][run]), int(vlan), num_ports)
            assert np.array_equal(got, want), (run, int(vlan))
            # fewer ports asked for: a prefix of the list; more than are configured: nothing new
            assert np.array_equal(fdb.flood_ports_host(int(z["ingress"][run]), int(vlan), 6), want[want < 6])
            assert np.array_equal(fdb.flood_ports_host(int(z["ingress"][run]), int(vlan), 4000), want)


def test_flood_ports_cap_counts_all_and_writes_cap(fx):
    z, _ = fx
    L = nf.lib()
    with fixture_fdb(z) as fdb:
        full = fdb.flood_ports_host(0, 10, int(z["num_ports"]))
        assert len(full) >= 4
        out, n = np.full(8, 0xABCDABCD, np.uint32), ctypes.c_uint32()
        assert L.nfcs_fdb_flood_ports_host(fdb.ptr, 0, 10, int(z["num_ports"]), out.ctypes.data, 2, ctypes.byref(n)) == 0
        assert n.value == len(full) and np.array_equal(out[:2], full[:2]) and (out[2:] == 0xABCDABCD).all()
        assert L.nfcs_fdb_flood_ports_host(fdb.ptr, 0, 10, int(z["num_ports"]), None, 0, ctypes.byref(n)) == 0
        assert n.value == len(full)


def random_case(seed, entries_n, frames_n=600):
    """Random entries over a few VLANs and ports (some beyond the configured ones), the fixture's ports,
    and frames whose MACs are mostly the entries'."""
    rng = np.random.default_rng(seed)
    macs = random_macs(rng, entries_n + 20)
    vl_pool = np.array([0, 1, 10, 20, 30, 99, 4095])
    entries = entries_of(macs[:entries_n], rng.choice(vl_pool, entries_n), rng.integers(0, 14, entries_n),
                         rng.integers(0, 2, entries_n))
    frames = []
    for _ in range(frames_n):
        d, s = macs[int(rng.integers(0, len(macs)))], macs[int(rng.integers(0, len(macs)))]
        vlan = int(rng.choice(vl_pool)) if rng.random() < 0.6 else None
        frames.append(frame_of(d, s, vlan, int(rng.choice([0, 13, 14, 17, 18, 60]))))
    return entries, frames


@pytest.mark.parametrize("seed,entries_n", [(1, 0), (2, 7), (3, 300), (4, 3000)])
def test_lookup_host_matches_dict_model(fx, seed, entries_n):
    z, _ = fx
    ports = fixture_ports(z)
    entries, frames = random_case(seed, entries_n)
    with set_ports(nf.Fdb().set_entries(entries), ports).commit() as fdb:
        for ingress in (0, 3, 5, 6, 11, 2000):
            got = decide_host(fdb, ingress, frames)
            want = model_decide(entries, ports, ingress, frames)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), ingress


def test_argument_errors():
    L = nf.lib()
    fdb = nf.Fdb()
    v, frame = ctypes.c_uint32(), bytes(64)
    port = np.zeros(1, dtype=nf.L2_PORT_DTYPE)
    p = port.ctypes.data
    vl = np.array([10, 4095], np.uint16)
    # before commit
    assert L.nfcs_fdb_lookup_host(fdb.ptr, 0, frame, 64, ctypes.byref(v), None, None, None) == EINVAL
    assert L.nfcs_fdb_stats(fdb.ptr, None, None, None, None) == EINVAL
    assert L.nfcs_fdb_flood_ports_host(fdb.ptr, 0, 1, 4, None, 0, ctypes.byref(v)) == EINVAL
    # null with n > 0, null objects, too many entries
    assert L.nfcs_fdb_set_entries(fdb.ptr, None, 1) == EINVAL
    assert L.nfcs_fdb_set_entries(None, None, 0) == EINVAL
    assert L.nfcs_fdb_set_entries(fdb.ptr, None, 0) == 0
    big = np.zeros(nf.FDB_MAX_ENTRIES + 1, dtype=nf.FDB_ENTRY_DTYPE)
    assert L.nfcs_fdb_set_entries(fdb.ptr, big.ctypes.data, len(big)) == EINVAL
    # ports: the id, the native VLAN, an allowed VLAN, the type
    assert L.nfcs_fdb_set_port(fdb.ptr, None, None, 0) == EINVAL
    assert L.nfcs_fdb_set_port(None, p, None, 0) == EINVAL
    assert L.nfcs_fdb_set_port(fdb.ptr, p, None, 1) == EINVAL
    port[0]["port_id"] = nf.L2_MAX_PORTS
    assert L.nfcs_fdb_set_port(fdb.ptr, p, None, 0) == EINVAL
    port[0]["port_id"], port[0]["native_vlan"] = nf.L2_MAX_PORTS - 1, 4096
    assert L.nfcs_fdb_set_port(fdb.ptr, p, None, 0) == EINVAL
    port[0]["native_vlan"], port[0]["type"] = 4095, 3
    assert L.nfcs_fdb_set_port(fdb.ptr, p, None, 0) == EINVAL
    port[0]["type"] = nf.L2_TRUNK
    assert L.nfcs_fdb_set_port(fdb.ptr, p, vl.ctypes.data, 2) == 0
    vl[1] = 4096
    assert L.nfcs_fdb_set_port(fdb.ptr, p, vl.ctypes.data, 2) == EINVAL
    assert L.nfcs_fdb_commit(fdb.ptr) == 0
    assert L.nfcs_fdb_lookup_host(fdb.ptr, 0, frame, 64, None, None, None, None) == 0  # every out pointer may be NULL
    assert L.nfcs_fdb_lookup_host(fdb.ptr, 0, None, 0, ctypes.byref(v), None, None, None) == 0
    assert v.value == nf.L2_NO_ETH
    assert L.nfcs_fdb_lookup_host(fdb.ptr, 0, None, 1, ctypes.byref(v), None, None, None) == EINVAL
    assert L.nfcs_fdb_flood_ports_host(fdb.ptr, 0, 1, 4, None, 0, None) == EINVAL
    assert L.nfcs_fdb_flood_ports_host(fdb.ptr, 0, 1, 4, None, 1, ctypes.byref(v)) == EINVAL
    # the device side needs a context and an upload
    assert L.nfcs_fdb_upload(None, fdb.ptr) == EINVAL
    assert L.nfcs_l2_lookup_device(None, fdb.ptr, 0, None, 0, None, 0, None, None, None, None, None, None) == EINVAL
    assert L.nfcs_fdb_create(None) == EINVAL and L.nfcs_fdb_destroy(None) == EINVAL
    assert L.nfcs_fdb_commit(None) == EINVAL and L.nfcs_fdb_clear_ports(None) == EINVAL
    with pytest.raises(nf.NfcsError):
        nf.Fdb().set_entries(big)
    fdb.close()


@pytest.mark.parametrize("setter", ["set_entries", "set_port", "clear_ports"])
def test_each_setter_invalidates_the_commit(setter):
    with nf.Fdb().commit() as fdb:
        assert fdb.lookup_host(0, bytes(64))[0] == nf.L2_FLOOD
        {"set_entries": lambda: fdb.set_entries(np.zeros(0, nf.FDB_ENTRY_DTYPE)),
         "set_port": lambda: fdb.set_port(3), "clear_ports": fdb.clear_ports}[setter]()
        with pytest.raises(nf.NfcsError):
            fdb.lookup_host(0, bytes(64))
        with pytest.raises(nf.NfcsError):
            fdb.stats()
        with pytest.raises(nf.NfcsError):
            fdb.flood_ports_host(0, 1, 4)
        assert fdb.commit().lookup_host(0, bytes(64))[0] == nf.L2_FLOOD


def test_port_defaults_memory_and_replacement():
    m = np.array([[2, 0, 0, 0, 0, 1]], np.uint8)
    with nf.Fdb().set_entries(entries_of(m, [1], [700])) as fdb:
        # the entry's port was never set: link down, whatever its id; so is an ingress port never set
        fdb.set_port(0, native_vlan=1).commit()
        assert fdb.lookup_host(0, frame_of(m[0], bytes(6)))[:3] == (nf.L2_DROP_LINK_DOWN, nf.IF_NONE, 1)
        fdb.set_port(700, stp_forwarding=False, native_vlan=1).commit()
        assert fdb.lookup_host(0, frame_of(m[0], bytes(6)))[0] == nf.L2_DROP_STP
        fdb.set_port(700, type=nf.L2_TRUNK, native_vlan=5, allowed_vlans=[7]).commit()  # the same id again replaces it
        assert fdb.lookup_host(0, frame_of(m[0], bytes(6)))[0] == nf.L2_DROP_VLAN
        fdb.set_port(700, type=nf.L2_HYBRID, native_vlan=5, allowed_vlans=[7, 1]).commit()
        assert fdb.lookup_host(0, frame_of(m[0], bytes(6)))[:2] == (nf.L2_FORWARD, 700)
        assert fdb.lookup_host(5000, frame_of(m[0], bytes(6)))[:3] == (nf.L2_DROP_VLAN, nf.IF_NONE, 1)
        assert list(fdb.flood_ports_host(0, 1, 1024)) == [700] and list(fdb.flood_ports_host(700, 1, 1024)) == [0]
        fdb.clear_ports().commit()
        assert fdb.lookup_host(0, frame_of(m[0], bytes(6)))[0] == nf.L2_DROP_LINK_DOWN
        assert len(fdb.flood_ports_host(0, 1, 1024)) == 0


def test_access_port_ignores_its_allowed_set_and_short_tagged_frames_use_the_native_vlan():
    m = np.array([[2, 0, 0, 0, 0, 1], [2, 0, 0, 0, 0, 2]], np.uint8)
    with nf.Fdb().set_entries(entries_of(m, [10, 20], [1, 1])) as fdb:
        fdb.set_port(0, native_vlan=10, allowed_vlans=[20]).set_port(1, type=nf.L2_TRUNK, allowed_vlans=[10, 20]).commit()
        assert fdb.lookup_host(0, frame_of(m[0], m[1]))[:3] == (nf.L2_FORWARD, 1, 10)
        assert fdb.lookup_host(0, frame_of(m[1], m[0], vlan=20))[:3] == (nf.L2_DROP_VLAN, nf.IF_NONE, 20)
        for length in (14, 17):  # tagged with VLAN 20 but without a whole VLAN header: the native VLAN
            assert fdb.lookup_host(0, frame_of(m[0], m[1], vlan=20, length=length))[:3] == (nf.L2_FORWARD, 1, 10)
        assert fdb.lookup_host(0, frame_of(m[0], m[1], vlan=20, length=13)) == (nf.L2_NO_ETH, nf.IF_NONE, 0, nf.L2_LEARN_NONE)


def test_duplicate_keys_first_wins():
    m = np.array([[2, 0, 0, 0, 0, 1]] * 3 + [[0] * 6] * 2, np.uint8)
    e = entries_of(m, [10, 10, 11, 0, 0], [1, 2, 3, 4, 5], [0, 1, 0, 1, 0])
    with nf.Fdb().set_entries(e).set_port(0, native_vlan=10).commit() as fdb:
        for p in (1, 2, 3, 4, 5):
            fdb.set_port(p, type=nf.L2_TRUNK, allowed_vlans=[10, 11, 0])
        fdb.set_port(0, type=nf.L2_TRUNK, native_vlan=10, allowed_vlans=[10, 11, 0]).commit()
        assert fdb.stats()["entries"] == 3
        assert fdb.lookup_host(0, frame_of(m[0], m[0]))[:2] == (nf.L2_FORWARD, 1)
        assert fdb.lookup_host(0, frame_of(m[0], m[0]))[3] == nf.L2_LEARN_MOVED  # the first is dynamic, on port 1
        assert fdb.lookup_host(0, frame_of(m[0], m[0], vlan=11))[:2] == (nf.L2_FORWARD, 3)
        # the all-zero MAC on VLAN 0 is a key like any other; the first of its two entries is static
        assert fdb.lookup_host(0, frame_of(bytes(6), bytes(6), vlan=0)) == (nf.L2_FORWARD, 4, 0, nf.L2_LEARN_NONE)
    with nf.Fdb().set_port(0).commit() as fdb:  # and in an empty table it misses, though every slot is zero
        assert fdb.lookup_host(0, frame_of(bytes(6), bytes(6), vlan=0)) == (nf.L2_FLOOD, nf.IF_NONE, 0, nf.L2_LEARN_NEW)


def found_and_missed(fdb, macs, vlans, ports, absent):
    """Every entry is found as a destination (no port is configured, so a hit reads DROP_LINK_DOWN and a
    miss FLOOD) and as a source (a dynamic entry on another port: MOVED; on the ingress port: REFRESH);
    the absent keys miss both ways."""
    for m, v, p in zip(macs, vlans, ports):
        assert fdb.lookup_host(4000, frame_of(m, m, int(v))) == (nf.L2_DROP_LINK_DOWN, nf.IF_NONE, int(v), nf.L2_LEARN_MOVED)
        assert fdb.lookup_host(int(p), frame_of(m, m, int(v)))[::3] == (nf.L2_DROP_SAME_PORT, nf.L2_LEARN_REFRESH)
    for m in absent:
        assert fdb.lookup_host(4000, frame_of(m, m, 7))[::3] == (nf.L2_FLOOD, nf.L2_LEARN_NEW)


def absent_keys(rng, macs, n=1000):
    have = {bytes(m) for m in macs}
    out = [m for m in rng.integers(0, 256, size=(n + 50, 6), dtype=np.uint8) if bytes(m) not in have]
    return out[:n]


@pytest.mark.parametrize("entries_n", [1, 2, 3, 4, 5, 1000])
def test_every_entry_found_and_absent_keys_miss(entries_n):
    rng = np.random.default_rng(100 + entries_n)
    macs = random_macs(rng, entries_n)
    vlans, ports = rng.integers(0, 4096, entries_n), rng.integers(0, 8, entries_n)
    with nf.Fdb().set_entries(entries_of(macs, vlans, ports)).commit() as fdb:
        st = fdb.stats()
        slots = 16
        while slots < 2 * entries_n:
            slots *= 2
        assert st["entries"] == entries_n and st["slots"] == slots and 1 <= st["max_probe"] <= entries_n
        found_and_missed(fdb, macs, vlans, ports, absent_keys(rng, macs))


def test_empty_table_stats():
    with nf.Fdb().commit() as fdb:
        assert fdb.stats() == dict(entries=0, slots=16, max_probe=0, wrapped=0)


def test_wrapped_probe_sequences():
    seed, macs, vlans, ports = wrapping_table()
    assert seed < WRAP_SEED_LIMIT
    with nf.Fdb().set_entries(entries_of(macs, vlans, ports)).commit() as fdb:
        st = fdb.stats()
        assert st["wrapped"] > 0 and st["max_probe"] >= 3 and st["slots"] == 64
        found_and_missed(fdb, macs, vlans, ports, absent_keys(np.random.default_rng(seed), macs))


def test_fdb_compile_standalone_under_host_sanitizers(tmp_path):
    """The compile step and the decision as a stand-alone host program (its own main, no HIP, nothing
    loaded into Python) under AddressSanitizer + UBSan, checked against a direct walk of its inputs."""
    exe = str(tmp_path / "fdb_compile_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "netflow_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "fdb_compile_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fdb compile OK" in r.stdout


def test_cpp_make_fdb_host_only(tmp_path):
    """netflow_amd::make_fdb_from (packet.hpp; what netflow_adapter.hpp's make_fdb forwards to) over
    mirror types with the reference's member names: compiled with g++ against the C ABI and run on the
    host, no GPU."""
    if not os.path.exists(nf.LIB_PATH):
        nf.build()
    exe, libdir = str(tmp_path / "make_fdb_test"), os.path.dirname(nf.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "make_fdb_test.cpp"), "-o", exe, "-L" + libdir,
                    "-l:" + os.path.basename(nf.LIB_PATH), "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "make_fdb OK" in r.stdout
