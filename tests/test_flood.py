"""CPU tests of flood replication's host side (nfcs_flood_expand_host, the per-VLAN port bitmap of
nfcs_fdb_commit): the bitmap's mask against nfcs_fdb_flood_ports_host, the expand against the reference's
dequeue record (tests/golden/flood_ref.npz) through the egress stage's host functions, against a dict/loop
restatement on random inputs, the overflow rule, the argument errors, commit invalidation, and the host code
as a stand-alone program under the sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import netflow_amd as nf
from egress_common import Q
from flood_common import (CUTS, FULL_PORTS, FULL_SRC, NONE, assert_same_expand, fixture_egress, fixture_fdb, flood_fixture,
                          model_expand, packed, reference_queues, round_up, small_burst)
from l2_common import set_ports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return flood_fixture()


def mask_ports(fdb, ingress, num_ports, vlans):
    """The flood ports per VLAN as the expand lists them: one flooded 14-byte packet per VLAN."""
    n = len(vlans)
    fan = min(num_ports, 1024)
    desc, used = packed([14] * n)
    out = fdb.flood_expand_host(ingress, num_ports, used + 16 * n * fan, used, 16, desc, n * fan,
                                l2_port=np.full(n, NONE, np.uint32), l2_verdict=np.full(n, nf.L2_FLOOD, np.uint8),
                                l2_vlan=np.asarray(vlans, np.uint16))
    m = int(out["totals"]["items"])
    assert m == int(out["totals"]["items_needed"]) == int(out["totals"]["copies"])
    src, port = out["item_src"][:m], out["item_port"][:m]
    return [port[src == i].tolist() for i in range(n)]


def test_bitmap_mask_equals_flood_ports_host_on_the_fixture(fx):
    z, _ = fx
    vlans = list(range(4096))
    with fixture_fdb(z) as fdb:
        for ingress in range(14):  # 11: never set; 12, 13: past the table
            for num_ports in (12, 5):
                got = mask_ports(fdb, ingress, num_ports, vlans)
                for v in (0, 1, 10, 20, 30, 40, 99, 4095):
                    assert got[v] == fdb.flood_ports_host(ingress, v, num_ports).tolist(), (ingress, num_ports, v)
                assert sum(len(g) for g in got) == sum(len(fdb.flood_ports_host(ingress, v, num_ports)) for v in
                                                       (1, 10, 20, 30, 40, 99))  # no other VLAN floods anywhere


@pytest.mark.parametrize("seed", range(4))
def test_bitmap_mask_equals_flood_ports_host_on_random_tables(seed):
    """Port ids around the mask's word boundaries; num_ports below, at and above the highest port set; an
    ingress port never set."""
    rng = np.random.default_rng(100 + seed)
    ids = sorted({0, 1, 2, 30, 31, 32, 33, 62, 63, 64, 65, 66} | set(int(x) for x in rng.integers(0, 70, 12)))
    ids = [p for p in ids if p != 40]  # 40: never set
    vlans = [1, 7, 31, 32, 33, 4095]
    with nf.Fdb() as fdb:
        for p in ids:
            typ = int(rng.integers(0, 3))
            fdb.set_port(p, link_up=rng.random() < 0.85, stp_forwarding=rng.random() < 0.85,
                         has_vlan_config=rng.random() < 0.9, type=typ, native_vlan=int(rng.choice(vlans)),
                         allowed_vlans=[v for v in vlans if rng.random() < 0.6])
        fdb.commit()
        top = max(ids)
        seen = 0
        for ingress in (0, 31, 32, 33, 64, 65, 40, top, top + 5):
            for num_ports in (1, 31, 32, 33, 64, top, top + 1, top + 2, 1024, 5000):
                got = mask_ports(fdb, ingress, num_ports, vlans + [0, 4094])
                for k, v in enumerate(vlans + [0, 4094]):
                    want = fdb.flood_ports_host(ingress, v, num_ports).tolist()
                    assert got[k] == want, (ingress, num_ports, v)
                    seen += len(want)
        assert seen > 200


def host_chain(fdb, eg, ingress, num_ports, frames, verdict, egress, vlan, copy_align=16):
    """expand -> plan -> pop (numpy) -> enqueue on the CPU: ({key: [(src, port, len, bytes)]}, key_dropped,
    the expand's output)."""
    desc, used = packed([len(f) for f in frames])
    out = fdb.flood_expand_host(ingress, num_ports, used + (1 << 22), round_up(used, 128), copy_align, desc, 16384,
                                l2_port=egress, l2_verdict=verdict, l2_vlan=vlan)
    m = int(out["totals"]["items"])
    assert m == int(out["totals"]["items_needed"])
    port, src = out["item_port"][:m], out["item_src"][:m]
    queue, edited = np.zeros(m, np.uint8), []
    for k in range(m):
        f = frames[int(src[k])]
        assert int(out["item_desc"][k]["len"]) == len(f)
        op, queue[k] = eg.plan_host(int(port[k]), f)
        edited.append(f[:12] + f[16:] if op == nf.VLAN_POP else f)
    keys = eg.keys()[1]
    res = eg.enqueue_host(port, queue, np.zeros(keys, np.uint32))
    queues = {}
    for key in range(keys):
        seq = res["order"][int(res["key_start"][key]):int(res["key_start"][key + 1])]
        if len(seq):
            queues[key] = [(int(src[k]), int(port[k]), len(edited[k]), edited[k][:64]) for k in seq]
    return queues, res["key_dropped"], out


@pytest.mark.parametrize("r", [0, 1, 2])
def test_expand_plan_enqueue_match_the_reference(fx, r):
    """Per queue the same packets in the same order with the same bytes, and the same tail drops."""
    z, frames = fx
    ingress, num_ports = int(z["ingress"][r]), int(z["num_ports"])
    with fixture_fdb(z) as fdb, fixture_egress(z) as eg:
        queues, dropped, out = host_chain(fdb, eg, ingress, num_ports, frames, z[f"verdict_{r}"], z[f"egress_{r}"],
                                          z[f"vlan_{r}"])
    want_q, want_drops = reference_queues(z, r)
    assert queues == want_q
    for k, d in want_drops.items():
        assert int(dropped[k]) == d, k
    # the item list itself: per flooded frame the reference's ports in its order
    m = int(out["totals"]["items"])
    fs = z[f"flood_start_{r}"]
    for i in np.flatnonzero(z[f"verdict_{r}"] == nf.L2_FLOOD):
        assert out["item_port"][:m][out["item_src"][:m] == i].tolist() == z[f"flood_port_{r}"][int(fs[i]):int(fs[i + 1])].tolist()
    assert int(out["totals"]["flooded"]) == int((z[f"verdict_{r}"] == nf.L2_FLOOD).sum())
    if r == 2:
        assert int(out["totals"]["copies"]) == 0 and int(out["totals"]["flooded"]) > 20


def random_inputs(rng, n, nports=40):
    """An Fdb over random ports, its port list, and one burst's arrays."""
    fdb, ports = nf.Fdb(), []
    vlans = [1, 10, 20, 4095]
    for p in range(nports):
        if rng.random() < 0.15:
            continue
        rec = np.zeros(1, nf.L2_PORT_DTYPE)[0]
        rec["port_id"], rec["link_up"], rec["stp_forwarding"] = p, rng.random() < 0.9, rng.random() < 0.9
        rec["has_vlan_config"], rec["type"], rec["native_vlan"] = rng.random() < 0.9, int(rng.integers(0, 3)), int(rng.choice(vlans))
        ports.append((rec, [v for v in vlans if rng.random() < 0.7]))
    set_ports(fdb, ports).commit()
    lens = rng.choice([0, 13, 14, 16, 17, 64, 200, 1514], n)
    desc, used = packed(lens)
    l3 = rng.integers(0, nports, n).astype(np.uint32)
    l3[rng.random(n) < 0.7] = NONE
    l2 = rng.integers(0, nports, n).astype(np.uint32)
    l2[rng.random(n) < 0.6] = NONE
    st = np.where(rng.random(n) < 0.5, nf.ST_FLAG_FWD | 2, 2).astype(np.uint8)
    verdict = rng.choice([nf.L2_FLOOD, nf.L2_FORWARD, nf.L2_DROP_VLAN, nf.L2_SKIP], n, p=[0.6, 0.2, 0.1, 0.1]).astype(np.uint8)
    vlan = rng.choice(vlans + [0, 4096, 0xFFFF], n).astype(np.uint16)
    return fdb, ports, desc, used, dict(l3_port=l3, fwd_status=st, l2_port=l2, l2_verdict=verdict, l2_vlan=vlan)


@pytest.mark.parametrize("seed", range(6))
def test_expand_matches_the_restatement_on_random_inputs(seed):
    rng = np.random.default_rng(500 + seed)
    n = 300
    fdb, ports, desc, used, arrays = random_inputs(rng, n)
    desc[5]["off16"] = 0xFFFFFFFF                       # dead: past the arena
    copy_base = round_up(used, 128) - (128 if seed % 2 else 0)  # odd seeds: the last frames reach into the copy region
    given = [("l3_port", "fwd_status", "l2_port", "l2_verdict", "l2_vlan"), ("l2_port", "l2_verdict", "l2_vlan"),
             ("l3_port", "l2_verdict", "l2_vlan"), ("l2_port",), ("l3_port", "fwd_status", "l2_port"),
             ("l3_port", "l2_port", "l2_vlan")][seed]
    args = {k: arrays[k] for k in given}
    with fdb:
        for ingress, num_ports, align in ((0, 40, 16), (3, 17, 128), (39, 64, 64), (50, 40, 16)):
            full = model_expand(ports, ingress, num_ports, 1 << 40, copy_base, align, desc, 20000, **args)
            need_items, need_bytes = int(full["totals"]["items_needed"]), int(full["totals"]["copy_bytes_needed"])
            for cap, room in ((20000, 1 << 30), (need_items // 2, 1 << 30), (20000, need_bytes // 3), (need_items, need_bytes)):
                want = model_expand(ports, ingress, num_ports, copy_base + room, copy_base, align, desc, cap, **args)
                got = fdb.flood_expand_host(ingress, num_ports, copy_base + room, copy_base, align, desc, cap, **args)
                assert_same_expand(got, want, f"ingress {ingress} cap {cap} room {room}: ")
    if "l2_verdict" in given:
        assert int(full["totals"]["flooded"]) > 20


@pytest.mark.parametrize("cap,room", sorted(CUTS))
def test_overflow_emits_a_prefix_and_pads(cap, room):
    """cap and the region each cut at 0, between two copies of one source, and at the exact fit. The raw call
    gets arrays four entries longer than cap: nothing is written past cap."""
    fdb, desc, copy_base, args = small_burst()
    with fdb:
        want = fdb.flood_expand_host(0, 4, copy_base + 1000, copy_base, 16, desc, 16, **args)
        assert want["item_port"][:9].tolist() == FULL_PORTS and want["item_src"][:9].tolist() == FULL_SRC
        assert int(want["totals"]["items"]) == 9 and int(want["totals"]["copy_bytes"]) == 192
        item_desc = np.full(cap + 4, 0xEE, np.uint8).repeat(8).view(nf.DESC_DTYPE)
        item_port, item_src = np.full(cap + 4, 0xEEEEEEEE, np.uint32), np.full(cap + 4, 0xEEEEEEEE, np.uint32)
        totals = np.zeros(1, nf.FLOOD_TOTALS_DTYPE)
        rc = nf.lib().nfcs_flood_expand_host(fdb.ptr, 0, 4, copy_base + room, copy_base, 16, desc.ctypes.data, 5, None, None,
                                             args["l2_port"].ctypes.data, args["l2_verdict"].ctypes.data,
                                             args["l2_vlan"].ctypes.data, cap, item_desc.ctypes.data, item_port.ctypes.data,
                                             item_src.ctypes.data, totals.ctypes.data)
    assert rc == 0
    m, t = CUTS[(cap, room)], totals[0]
    assert (int(t["items"]), int(t["items_needed"]), int(t["flooded"]), int(t["copy_bytes_needed"])) == (m, 9, 2, 192)
    copies = sum(1 for k in range(m) if FULL_SRC[k] in (1, 3))
    assert int(t["copies"]) == copies and int(t["copy_bytes"]) == 32 * copies
    assert np.array_equal(item_desc[:m], want["item_desc"][:m]) and item_port[:m].tolist() == FULL_PORTS[:m]
    assert item_src[:m].tolist() == FULL_SRC[:m]
    assert (item_desc[m:cap]["off16"] == 0).all() and (item_desc[m:cap]["len"] == 0).all()
    assert (item_port[m:cap] == nf.IF_NONE).all() and (item_src[m:cap] == nf.ITEM_NONE).all()
    assert (item_port[cap:] == 0xEEEEEEEE).all() and (item_src[cap:] == 0xEEEEEEEE).all()
    assert (item_desc[cap:]["off16"] == 0xEEEEEEEE).all() and (item_desc[cap:]["len"] == 0xEEEEEEEE).all()
    for k in range(m):  # a copy exactly when it lies in the region, inside it, in item order
        o = int(item_desc[k]["off16"]) * 16
        assert (o >= copy_base) == (FULL_SRC[k] in (1, 3))
        assert o < copy_base or o + 32 <= copy_base + room


def test_argument_errors_and_no_packets():
    fdb, desc, copy_base, args = small_burst()
    L = nf.lib()
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data

    def call(n=5, l3=None, st=None, l2=p, verdict=p, vlan=p, arena_bytes=copy_base + 512, base=copy_base, align=16,
             num_ports=4, cap=4, items=p, totals=p, d=desc.ctypes.data):
        return L.nfcs_flood_expand_host(fdb.ptr, 0, num_ports, arena_bytes, base, align, d, n, l3, st, l2, verdict, vlan, cap,
                                        items, items, items, totals)

    with fdb:
        assert call() == 0
        assert call(l2=None, verdict=None, vlan=None) == -1      # both port arrays NULL
        assert call(st=p) == -1                                   # a status without the L3 ports
        assert call(vlan=None) == -1                              # a verdict without the VLANs
        assert call(verdict=None, vlan=None) == 0                 # the compaction alone
        assert call(verdict=None) == 0
        for align in (0, 8, 24, 48):
            assert call(align=align) == -1, align                 # not a power of two >= 16
        assert call(base=copy_base + 16, align=32) == -1          # copy_base not a multiple of copy_align
        assert call(base=copy_base + 1024) == -1                  # copy_base past the arena
        assert call(base=copy_base + 512) == 0                    # an empty region is legal
        assert call(n=1 << 23, num_ports=1024) == -1              # the item count would not fit 32 bits
        assert call(totals=None) == -1 and call(d=None) == -1 and call(items=None) == -1
        assert call(cap=0, items=None) == 0
        assert call(n=0, d=None, items=None, totals=None) == 0    # n == 0: nothing is looked at or written
        assert call(n=0, l2=None, verdict=None, vlan=None) == -1  # the argument rules come first, as in the plan
        assert L.nfcs_flood_expand_host(None, 0, 4, 1024, 512, 16, p, 1, None, None, p, None, None, 1, p, p, p, p) == -1


def test_commit_invalidation():
    fdb, desc, copy_base, args = small_burst()
    with fdb:
        a = fdb.flood_expand_host(0, 4, copy_base + 512, copy_base, 16, desc, 16, **args)
        fdb.set_port(2, link_up=False, native_vlan=1)  # invalidates the commit
        with pytest.raises(nf.NfcsError):
            fdb.flood_expand_host(0, 4, copy_base + 512, copy_base, 16, desc, 16, **args)
        b = fdb.commit().flood_expand_host(0, 4, copy_base + 512, copy_base, 16, desc, 16, **args)
    assert int(a["totals"]["copies"]) == 6 and int(b["totals"]["copies"]) == 4
    assert b["item_port"][:7].tolist() == [2, 1, 3, 3, 1, 3, 1]  # the unicast packet to port 2 keeps its item


def test_flood_compile_main_under_sanitizers(tmp_path):
    """The bitmap's compile step, the mask and the host walk as a stand-alone host program (its own main, no
    HIP, nothing loaded into Python) under AddressSanitizer + UBSan, arrays in heap blocks of their exact size."""
    exe = str(tmp_path / "flood_compile_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "netflow_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "flood_compile_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "flood compile OK" in r.stdout


def test_python_constants_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "nfcs.h")).read()
    for name, value in (("NFCS_FLOOD_TILE_PKTS", nf.FLOOD_TILE_PKTS), ("NFCS_ITEM_NONE", nf.ITEM_NONE)):
        m = re.search(r"#define\s+" + name + r"\s+(0x[0-9A-Fa-f]+|\d+)u", hdr)
        assert m and int(m.group(1), 0) == value, name
    assert nf.FLOOD_TOTALS_DTYPE.names == ("items", "items_needed", "copies", "flooded", "copy_bytes", "copy_bytes_needed")
    assert Q == 8
