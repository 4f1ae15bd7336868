"""GPU tests of the route / ARP lookup kernel (nfcs_route_lookup_device) through the C ABI: against
the reference's decisions on the fixture frames (tests/golden/route_ref.npz), against the CPU decision
of the same tables (Fib.lookup_host) at the sizes where the kernel changes path, and end to end in
front of the fused forward against the oracle."""
import numpy as np
import pytest

import netflow_amd as nf
import oracle
from l3_common import random_l3_case
from route_common import (TABLES, decide_host, dst_pool, fixture_fib, make_fib, rewrite_dsts, route_fixture)

pytestmark = pytest.mark.gpu

ip = nf.ip4
MAC_A, MAC_B = np.array([[0x02, 1, 2, 3, 4, 5]], np.uint8), np.array([[0x02, 9, 8, 7, 6, 5]], np.uint8)


@pytest.fixture(scope="module")
def fx():
    return route_fixture()


def run_lookup(engine, fib, arena, desc, arena_bytes=None, outputs=True):
    """(nh, egress_if, verdict) from the device; outputs=False passes NULL for the optional two."""
    n = len(desc)
    fib.upload(engine)
    d_arena = engine.alloc(arena.nbytes).upload(arena)
    d_desc = engine.alloc(max(desc.nbytes, 16)).upload(desc)
    d_nh = engine.alloc(max(4 * n, 16)).upload(np.full(n, 0xDEADBEEF, np.uint32))
    d_if = engine.alloc(max(4 * n, 16)) if outputs else None
    d_v = engine.alloc(max(n, 16)) if outputs else None
    engine.route_lookup_device(fib, d_arena, arena.nbytes if arena_bytes is None else arena_bytes, d_desc, n,
                               d_nh, d_if, d_v)
    engine.sync()
    assert np.array_equal(d_arena.download(np.uint8, arena.nbytes), arena), "the lookup wrote into the frames"
    nh = d_nh.download(np.uint32, n)
    return (nh, d_if.download(np.uint32, n), d_v.download(np.uint8, n)) if outputs else (nh, None, None)


def ipv4_frame(dst: int, ttl: int = 64, tagged: bool = False, length: int = 60) -> bytes:
    b = bytearray(length if length >= 38 else 38)
    b[12:14] = b"\x81\x00" if tagged else b"\x08\x00"
    l2 = 18 if tagged else 14
    if tagged:
        b[16:18] = b"\x08\x00"
    b[l2] = 0x45
    b[l2 + 8] = ttl
    b[l2 + 16:l2 + 20] = int(dst).to_bytes(4, "little")
    return bytes(b[:length])


@pytest.mark.parametrize("align", [16, 128])
@pytest.mark.parametrize("table", TABLES)
def test_fixture_matches_reference(engine, fx, table, align):
    z, frames = fx
    arena, desc = oracle.pack_frames(frames, align=align)
    with fixture_fib(z, table) as fib:
        nh, eif, v = run_lookup(engine, fib, arena, desc)
        nht = fib.nexthops_host()
        assert fib.nexthops()[1] == len(nht)
    assert np.array_equal(v, z["verdict_" + table])
    assert np.array_equal(eif, z["egress_" + table])
    fwd = v == nf.RT_FORWARD
    assert (nh[~fwd] == nf.NH_NONE).all() and (nh[fwd] < len(nht)).all()
    got = np.concatenate([nht["dst_mac"][nh[fwd]], nht["src_mac"][nh[fwd]]], axis=1)
    assert np.array_equal(got, z["macs_" + table][fwd])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 1000])
def test_sizes_and_bad_descriptors(engine, fx, n):
    """Wave and workgroup edges (64 packets per wave, 256 per workgroup), the first and the last
    descriptor reaching outside the arena, and the optional outputs left out."""
    z, frames = fx
    frames = [frames[(7 * i) % len(frames)] for i in range(n)]
    arena, desc = oracle.pack_frames(frames, align=16)
    with fixture_fib(z, "b") as fib:
        want_v, want_nh, want_if = decide_host(fib, frames)
        nh, eif, v = run_lookup(engine, fib, arena, desc)
        assert np.array_equal(v, want_v) and np.array_equal(nh, want_nh) and np.array_equal(eif, want_if)
        nh_only, _, _ = run_lookup(engine, fib, arena, desc, outputs=False)
        assert np.array_equal(nh_only, want_nh)
        bad = desc.copy()
        bad[0]["off16"] = arena.nbytes // 16  # starts at the arena's end
        bad[n - 1]["len"] = arena.nbytes - int(bad[n - 1]["off16"]) * 16 + 1  # one byte past it
        nh, eif, v = run_lookup(engine, fib, arena, bad)
    for i in {0, n - 1}:
        want_v[i], want_nh[i], want_if[i] = nf.RT_BAD_DESC, nf.NH_NONE, nf.IF_NONE
    assert np.array_equal(v, want_v) and np.array_equal(nh, want_nh) and np.array_equal(eif, want_if)


@pytest.mark.parametrize("routes_n", [0, 1, 8, 9, 65, nf.FIB_MAX_ROUTES])
def test_route_counts_match_at_last_entry(engine, routes_n):
    """Host routes 10.(i>>8).(i&255).1/32 on interface i + 1; only the address of the LAST one (index
    routes_n - 1) has an ARP entry, so a FORWARD with that route's interface proves the scan reached the
    last entry: the last pair of a full group of 8 (8, 4096) and the only real pair of a padded group
    (1, 9, 65). That the scan stops at the first match shows at the front: entry 0's route is given
    again at index 1 with another interface, which must never be the answer."""
    addr = [ip(f"10.{i >> 8}.{i & 255}.1") for i in range(max(routes_n, 1))]
    routes = [[addr[i], 0xFFFFFFFF, 0, i + 1] for i in range(routes_n)]
    last = routes_n - 1
    if routes_n > 2:
        routes[1] = [addr[0], 0xFFFFFFFF, 0, 7777]  # shadowed by entry 0
    dsts = [addr[0], addr[last] if routes_n else ip("10.9.9.9"), addr[len(addr) // 2], ip("10.250.0.1")]
    frames = [ipv4_frame(d, tagged=bool(k & 1)) for k, d in enumerate(dsts * 40)]
    arena, desc = oracle.pack_frames(frames)
    if_ids = list(range(1, routes_n + 2)) + [7777]
    if_mac = np.repeat(MAC_B, len(if_ids), axis=0)
    # ARP entries for the last route's address and for entry 0's: both forward, each on its own route
    arp_ip = [addr[last], addr[0]] if routes_n else []
    with make_fib(np.array(routes, np.uint32).reshape(-1, 4), arp_ip, np.repeat(MAC_A, len(arp_ip), axis=0), if_ids,
                  if_mac, []) as fib:
        want_v, want_nh, want_if = decide_host(fib, frames)
        nh, eif, v = run_lookup(engine, fib, arena, desc)
    assert np.array_equal(v, want_v) and np.array_equal(nh, want_nh) and np.array_equal(eif, want_if)
    if routes_n == 0:
        assert (v == nf.RT_NO_ROUTE).all()
    else:
        assert v[1] == nf.RT_FORWARD and eif[1] == routes_n  # the last entry's interface
        assert v[0] == nf.RT_FORWARD and eif[0] == 1  # entry 0, not its copy at index 1
        assert v[3] == nf.RT_NO_ROUTE
        if routes_n > 2:
            assert v[2] == nf.RT_ARP_MISS  # a route in the middle, connected, no ARP entry


@pytest.mark.parametrize("arps_n", [0, 1, 2, 1000])
def test_arp_counts_and_search_edges(engine, arps_n):
    """One connected default route; ARP addresses 10.1.x.y every third value: hits on the first and
    the last address, misses below, between and above."""
    base = int.from_bytes(bytes([10, 1, 0, 10]), "big")
    host = [base + 3 * i for i in range(arps_n)]
    as_u32 = lambda h: int.from_bytes(h.to_bytes(4, "big"), "little")
    arp_ip = [as_u32(h) for h in host]
    arp_mac = np.array([[2, 0, 0, i >> 8, i & 255, 1] for i in range(arps_n)], np.uint8).reshape(-1, 6)
    probe = [base - 1, base + 1, base + 3 * max(arps_n - 1, 0) + 1, base + 3 * arps_n + 50]
    if arps_n:
        probe += [host[0], host[-1], host[arps_n // 2]]
    frames = [ipv4_frame(as_u32(h), ttl=2 + (k & 3)) for k, h in enumerate(probe * 30)]
    arena, desc = oracle.pack_frames(frames)
    with make_fib([[0, 0, 0, 4]], arp_ip, arp_mac, [4], MAC_B, []) as fib:
        want_v, want_nh, want_if = decide_host(fib, frames)
        nh, eif, v = run_lookup(engine, fib, arena, desc)
        nht = fib.nexthops_host()
    assert np.array_equal(v, want_v) and np.array_equal(nh, want_nh) and np.array_equal(eif, want_if)
    assert (v[:4] == nf.RT_ARP_MISS).all()
    if arps_n:
        assert (v[4:7] == nf.RT_FORWARD).all() and (eif[4:7] == 4).all()
        for k, i in ((4, 0), (5, arps_n - 1), (6, arps_n // 2)):
            assert bytes(nht["dst_mac"][nh[k]]) == bytes(arp_mac[i])


@pytest.mark.parametrize("table", TABLES)
def test_fresh_frames_match_host_decision(engine, fx, table):
    z, _ = fx
    rng = np.random.default_rng(77)
    frames = rewrite_dsts(oracle.fuzz_frames(77, 0, 4096), dst_pool(3), rng, 0.5)
    arena, desc = oracle.pack_frames(frames)
    with fixture_fib(z, table) as fib:
        want_v, want_nh, want_if = decide_host(fib, frames)
        nh, eif, v = run_lookup(engine, fib, arena, desc)
    assert (want_v == nf.RT_FORWARD).mean() >= 0.25
    assert np.array_equal(v, want_v) and np.array_equal(nh, want_nh) and np.array_equal(eif, want_if)


@pytest.mark.parametrize("table", TABLES)
def test_lookup_then_forward_matches_oracle(engine, fx, table):
    """Lookup and fused forward on one stream, no host step between them: byte-equal to the oracle's
    forward given the next hops the CPU decision yields; frames not forwarded are untouched."""
    z, _ = fx
    rng = np.random.default_rng(31)
    frames = rewrite_dsts(random_l3_case(31, 4096)[0], dst_pool(3), rng, 0.5)
    arena, desc = oracle.pack_frames(frames)
    n = len(desc)
    with fixture_fib(z, table) as fib:
        want_v, want_nh, _ = decide_host(fib, frames)
        nht = fib.nexthops_host()
        fib.upload(engine)
        d_tab, tab_n = fib.nexthops()
        d_arena = engine.alloc(arena.nbytes).upload(arena)
        d_desc = engine.alloc(desc.nbytes).upload(desc)
        d_nh, d_v, d_st = engine.alloc(4 * n), engine.alloc(n), engine.alloc(n)
        engine.route_lookup_device(fib, d_arena, arena.nbytes, d_desc, n, d_nh, None, d_v)
        engine.l3_forward_device(d_arena, arena.nbytes, d_desc, d_nh, n, d_tab, tab_n, d_st)
        engine.sync()
        out, st, v = d_arena.download(np.uint8, arena.nbytes), d_st.download(np.uint8, n), d_v.download(np.uint8, n)
    assert (want_v == nf.RT_FORWARD).mean() >= 0.25
    ref = arena.copy()
    rst = oracle.l3_forward_batch(ref, desc, want_nh, nht.view(np.uint8).reshape(-1, 12))
    assert np.array_equal(v, want_v)
    assert np.array_equal(st, rst)
    assert np.array_equal(out, ref)
    assert ((st & nf.ST_FLAG_FWD) != 0).sum() > n // 8
    for i in np.nonzero(v != nf.RT_FORWARD)[0]:
        o, ln = int(desc[i]["off16"]) * 16, int(desc[i]["len"])
        assert np.array_equal(out[o:o + ln], arena[o:o + ln]), i
