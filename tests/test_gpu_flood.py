"""GPU tests of flood replication (nfcs_flood_expand_device) through the C ABI. Every test compares the
device's item arrays and totals with Fdb.flood_expand_host (arrays equal) and the arena byte for byte with the
numpy copy model of flood_common.copy_model, bytes outside the emitted slots included; the item arrays and the
arena carry canary entries past cap and past arena_bytes that must stay as they were. The fixture
(tests/golden/flood_ref.npz) also runs through L2 lookup -> expand -> plan -> VLAN -> enqueue in one stream,
against the reference's dequeue record."""
import numpy as np
import pytest

import netflow_amd as nf
from flood_common import (CUTS, FILL, NONE, assert_same_expand, copy_model, fixture_egress, fixture_fdb, flood_fixture,
                          pack_with_tail, reference_queues, round_up, small_burst)

pytestmark = pytest.mark.gpu

T = nf.FLOOD_TILE_PKTS
SCAN = 256  # tile sums per trip of the scan kernel's loop (nfcs_kernels.hip kFloodScanThreads)
GUARD = 256  # canary bytes behind arena_bytes
EE = 0xEEEEEEEE


@pytest.fixture(scope="module")
def fx():
    return flood_fixture()


def up(engine, a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return engine.alloc(max(a.nbytes, 16)).upload(a)


def filled(engine, nbytes):
    return engine.alloc(nbytes + 16).upload(np.full(nbytes + 16, FILL, np.uint8))


class Run:
    """One expand on the device: the buffers stay available for calls that follow on the same stream."""

    def __init__(self, engine, fdb, ingress, num_ports, arena, desc, copy_base, align, cap, arrays, upload=True, sync=True):
        self.engine, self.n, self.cap, self.arena_bytes = engine, len(desc), cap, arena.nbytes
        if upload:
            fdb.upload(engine)
        self.d_arena = up(engine, np.concatenate([arena, np.full(GUARD, FILL, np.uint8)]), np.uint8)
        self.d_desc = up(engine, desc, nf.DESC_DTYPE)
        dt = {"l3_port": np.uint32, "fwd_status": np.uint8, "l2_port": np.uint32, "l2_verdict": np.uint8, "l2_vlan": np.uint16}
        self.d_in = {k: up(engine, v, dt[k]) for k, v in arrays.items()}
        self.d_item_desc, self.d_item_port = filled(engine, 8 * (cap + 4)), filled(engine, 4 * (cap + 4))
        self.d_item_src, self.d_totals = filled(engine, 4 * (cap + 4)), filled(engine, 64)
        engine.flood_expand_device(fdb, ingress, num_ports, self.d_arena, arena.nbytes, copy_base, align, self.d_desc, self.n,
                                   cap, self.d_item_desc, self.d_item_port, self.d_item_src, self.d_totals, **self.d_in)
        if sync:
            engine.sync()

    def result(self):
        cap = self.cap
        item_desc = self.d_item_desc.download(nf.DESC_DTYPE, cap + 4)
        item_port, item_src = self.d_item_port.download(np.uint32, cap + 4), self.d_item_src.download(np.uint32, cap + 4)
        tot = self.d_totals.download(np.uint8, 64)
        assert (tot[32:] == FILL).all(), "a store behind d_totals"
        assert (item_port[cap:] == EE).all() and (item_src[cap:] == EE).all(), "a store past cap"
        assert (item_desc[cap:]["off16"] == EE).all() and (item_desc[cap:]["len"] == EE).all(), "a store past cap"
        arena = self.d_arena.download(np.uint8, self.arena_bytes + GUARD)
        assert (arena[self.arena_bytes:] == FILL).all(), "a store past arena_bytes"
        return {"item_desc": item_desc[:cap].copy(), "item_port": item_port[:cap].copy(), "item_src": item_src[:cap].copy(),
                "totals": tot[:32].copy().view(nf.FLOOD_TOTALS_DTYPE)[0], "arena": arena[:self.arena_bytes].copy()}


def check(engine, fdb, ingress, num_ports, arena, desc, copy_base, align, cap, arrays, what="", upload=True):
    """Device against host: the arrays, the totals, the arena. Returns the host's output."""
    want = fdb.flood_expand_host(ingress, num_ports, arena.nbytes, copy_base, align, desc, cap, **arrays)
    got = Run(engine, fdb, ingress, num_ports, arena, desc, copy_base, align, cap, arrays, upload=upload).result()
    assert_same_expand(got, want, what)
    assert np.array_equal(got["arena"], copy_model(arena, desc, want, copy_base)), what + "the arena differs from the copy model"
    return want


def access_table(ports, vlan=1):
    """Ports 0..ports-1, all ACCESS on one VLAN, link up, forwarding: a flood from p reaches every other port."""
    fdb = nf.Fdb()
    for p in range(ports):
        fdb.set_port(p, native_vlan=vlan)
    return fdb.commit()


def mixed_arrays(rng, n, nports, p_flood=0.3, p_uni=0.4):
    l2 = rng.integers(0, nports, n).astype(np.uint32)
    l2[rng.random(n) >= p_uni] = NONE
    verdict = np.where(rng.random(n) < p_flood, nf.L2_FLOOD, nf.L2_DROP_VLAN).astype(np.uint8)
    return dict(l2_port=l2, l2_verdict=verdict, l2_vlan=np.ones(n, np.uint16))


# ---- the fixture ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("align", [16, 128])
@pytest.mark.parametrize("r", [0, 1, 2])
def test_fixture_expand_matches_host(engine, fx, r, align):
    z, frames = fx
    arena, desc, copy_base = pack_with_tail(frames, 16, 1 << 19)
    arrays = dict(l2_port=z[f"egress_{r}"], l2_verdict=z[f"verdict_{r}"], l2_vlan=z[f"vlan_{r}"])
    with fixture_fdb(z) as fdb:
        want = check(engine, fdb, int(z["ingress"][r]), int(z["num_ports"]), arena, desc, copy_base, align, 8192, arrays)
    assert int(want["totals"]["items"]) == int(want["totals"]["items_needed"])
    assert (int(want["totals"]["copies"]) > 500) == (r != 2)


@pytest.mark.parametrize("r", [0, 1, 2])
def test_fixture_chain_matches_the_reference(engine, fx, r):
    """L2 lookup -> expand -> plan -> VLAN -> enqueue on one stream with no host step; plan, VLAN and enqueue run
    over all cap entries, the padding being inert. Per queue the same packets in the same order with the same
    bytes as the reference dequeued, and the same tail drops."""
    z, frames = fx
    n, cap, ingress = len(frames), 8192, int(z["ingress"][r])
    arena, desc, copy_base = pack_with_tail(frames, 16, 1 << 19)
    with fixture_fdb(z) as fdb, fixture_egress(z) as eg:
        fdb.upload(engine)
        eg.upload(engine)
        keys = eg.keys()[1]
        d_arena, d_desc = up(engine, arena, np.uint8), up(engine, desc, nf.DESC_DTYPE)
        d_l2, d_verdict, d_vlan = engine.alloc(4 * n), engine.alloc(n), engine.alloc(2 * n)
        d_idesc, d_iport, d_isrc, d_tot = engine.alloc(8 * cap), engine.alloc(4 * cap), engine.alloc(4 * cap), engine.alloc(32)
        d_port, d_ops, d_queue = engine.alloc(4 * cap), engine.alloc(4 * cap), engine.alloc(cap)
        d_depth = up(engine, np.zeros(keys, np.uint32), np.uint32)
        d_order, d_ks, d_drop = engine.alloc(4 * cap), engine.alloc(4 * (keys + 1)), engine.alloc(4 * keys)
        engine.l2_lookup_device(fdb, ingress, d_arena, copy_base, d_desc, n, d_l2, verdict=d_verdict, vlan=d_vlan)
        engine.flood_expand_device(fdb, ingress, int(z["num_ports"]), d_arena, arena.nbytes, copy_base, 16, d_desc, n, cap,
                                   d_idesc, d_iport, d_isrc, d_tot, l2_port=d_l2, l2_verdict=d_verdict, l2_vlan=d_vlan)
        engine.egress_plan_device(eg, d_arena, arena.nbytes, d_idesc, cap, d_port, d_ops, d_queue, l2_port=d_iport)
        engine.vlan_device(d_arena, arena.nbytes, d_idesc, cap, d_ops, 0, None, 64)
        engine.egress_enqueue_device(eg, d_port, d_queue, cap, d_depth, d_order, d_ks, key_dropped=d_drop)
        engine.sync()
        assert np.array_equal(d_verdict.download(np.uint8, n), z[f"verdict_{r}"])
        out, idesc = d_arena.download(np.uint8, arena.nbytes), d_idesc.download(nf.DESC_DTYPE, cap)
        iport, isrc = d_iport.download(np.uint32, cap), d_isrc.download(np.uint32, cap)
        ks, order, dropped = d_ks.download(np.uint32, keys + 1), d_order.download(np.uint32, cap), d_drop.download(np.uint32, keys)
    queues = {}
    for key in range(keys):
        seq = order[int(ks[key]):int(ks[key + 1])]
        if len(seq):
            queues[key] = [(int(isrc[k]), int(iport[k]), int(idesc[k]["len"]),
                            bytes(out[int(idesc[k]["off16"]) * 16:int(idesc[k]["off16"]) * 16 + min(int(idesc[k]["len"]), 64)]))
                           for k in seq]
    want_q, want_drops = reference_queues(z, r)
    assert queues == want_q
    for k, d in want_drops.items():
        assert int(dropped[k]) == d, k


# ---- sizes around the machinery --------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7])
def test_sizes_around_the_tile(engine, n):
    rng = np.random.default_rng(n)
    lens = rng.choice([14, 60, 64, 100, 300], n)
    frames = [rng.integers(0, 256, int(ln), dtype=np.uint8).tobytes() for ln in lens]
    with access_table(5) as fdb:
        arrays = mixed_arrays(rng, n, 5)
        arrays["l2_verdict"][n - 1], arrays["l2_port"][n - 1] = nf.L2_FLOOD, NONE  # the last packet floods
        arena, desc, copy_base = pack_with_tail(frames, 16, 4 * 304 * n)
        want = check(engine, fdb, 2, 5, arena, desc, copy_base, 16, 4 * n + 3, arrays)
    assert int(want["totals"]["copies"]) >= 4 and int(want["totals"]["items"]) == int(want["totals"]["items_needed"])


def test_crossing_the_scan_loops_boundary(engine):
    """More tile sums than one trip of the scan kernel's loop takes: 14-byte frames in 16-byte slots, 1% floods
    and 1% unicast packets, spread over every tile; the copy region then cut inside the last trip's tiles."""
    n = SCAN * T + T + 7
    rng = np.random.default_rng(3)
    desc = np.zeros(n, nf.DESC_DTYPE)
    desc["off16"], desc["len"] = np.arange(n), 14
    copy_base = round_up(16 * n, 128)
    arena = np.full(copy_base + (1 << 19), FILL, np.uint8)
    arena[:16 * n] = rng.integers(0, 256, 16 * n, dtype=np.uint8)
    with access_table(4) as fdb:
        arrays = mixed_arrays(rng, n, 4, p_flood=0.01, p_uni=0.01)
        want = check(engine, fdb, 0, 4, arena, desc, copy_base, 16, 1 << 14, arrays)
        t = want["totals"]
        assert int(t["items"]) == int(t["items_needed"]) > 5000 and int(want["item_src"][int(t["items"]) - 1]) > SCAN * T
        short = arena[:copy_base + int(t["copy_bytes_needed"]) - 16 * 10]  # the last 10 copies do not fit
        cut = check(engine, fdb, 0, 4, short, desc, copy_base, 16, 1 << 14, arrays, "cut: ", upload=False)
        assert int(cut["totals"]["copies"]) == int(t["copies"]) - 10
        assert int(cut["item_src"][int(cut["totals"]["items"]) - 1]) > SCAN * T


LENS = [14, 15, 16, 17, 31, 32, 33, 64, 255, 256, 257, 1500, 1514, 1535, 1536, 1537, 1552, 3072, 3073, 9000]


@pytest.mark.parametrize("align", [16, 128])
def test_frame_lengths_and_slot_alignment(engine, align):
    """One row pass of the copy takes 16 lanes x 6 chunks = 1,536 bytes, one instruction of a row 256."""
    rng = np.random.default_rng(align)
    frames = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in LENS]
    n = len(frames)
    arena, desc, copy_base = pack_with_tail(frames, 16, 3 * sum(round_up(ln, 128) for ln in LENS))
    arrays = dict(l2_port=np.full(n, NONE, np.uint32), l2_verdict=np.full(n, nf.L2_FLOOD, np.uint8), l2_vlan=np.ones(n, np.uint16))
    with access_table(4) as fdb:
        want = check(engine, fdb, 1, 4, arena, desc, copy_base, align, 3 * n, arrays)
    assert int(want["totals"]["copies"]) == 3 * n
    assert int(want["totals"]["copy_bytes"]) == 3 * sum(round_up(ln, align) for ln in LENS)


@pytest.mark.parametrize("ports,ingress,num_ports,fan", [(1, 0, 1, 0), (2, 0, 2, 1), (32, 0, 32, 31), (33, 0, 33, 32),
                                                          (34, 33, 34, 33), (34, 5, 32, 31), (1024, 1023, 1024, 1023)])
def test_fan_outs(engine, ports, ingress, num_ports, fan):
    rng = np.random.default_rng(ports)
    frames = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in (64, 14, 200)]
    arena, desc, copy_base = pack_with_tail(frames, 16, 3 * 208 * max(fan, 1))
    arrays = dict(l2_port=np.array([NONE, 0, NONE], np.uint32), l2_verdict=np.full(3, nf.L2_FLOOD, np.uint8),
                  l2_vlan=np.ones(3, np.uint16))
    with access_table(ports) as fdb:
        want = check(engine, fdb, ingress, num_ports, arena, desc, copy_base, 16, 2 * fan + 2, arrays)
    assert int(want["totals"]["items"]) == 2 * fan + 1 and int(want["totals"]["flooded"]) == 2
    assert want["item_port"][:fan].tolist() == [p for p in range(num_ports) if p != ingress]


def test_vlan_out_of_range_and_unknown_ingress_flood_nowhere(engine):
    frames = [bytes(64)] * 4
    arena, desc, copy_base = pack_with_tail(frames, 16, 4096)
    arrays = dict(l2_port=np.full(4, NONE, np.uint32), l2_verdict=np.full(4, nf.L2_FLOOD, np.uint8),
                  l2_vlan=np.array([1, 4096, 0xFFFF, 2], np.uint16))
    with access_table(4) as fdb:
        a = check(engine, fdb, 0, 4, arena, desc, copy_base, 16, 16, arrays)
        b = check(engine, fdb, 9, 4, arena, desc, copy_base, 16, 16, arrays, upload=False)
    assert (int(a["totals"]["copies"]), int(a["totals"]["flooded"])) == (3, 4)
    assert (int(b["totals"]["copies"]), int(b["totals"]["flooded"])) == (0, 4)


# ---- which packets ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("given", [("l2_port",), ("l2_verdict", "l2_vlan", "l3_port"), ("l3_port", "fwd_status", "l2_port"),
                                   ("l3_port", "fwd_status", "l2_port", "l2_verdict", "l2_vlan"),
                                   ("l3_port", "l2_port", "l2_verdict", "l2_vlan")])
def test_mixed_bursts_and_dead_descriptors(engine, given):
    """Unicast only (no verdicts), floods only, the L3 arrays with the status masking some; descriptors past
    arena_bytes, at its end, and reaching into the copy region yield no item and are not read."""
    n = T + 100
    rng = np.random.default_rng(len(given) * 7 + len(given[0]))
    lens = rng.choice([14, 64, 333], n)
    frames = [rng.integers(0, 256, int(ln), dtype=np.uint8).tobytes() for ln in lens]
    arena, desc, copy_base = pack_with_tail(frames, 16, 1 << 20)
    arrays = mixed_arrays(rng, n, 6, p_flood=0.5, p_uni=0.3)
    arrays["l3_port"] = np.where(rng.random(n) < 0.3, rng.integers(0, 6, n), NONE).astype(np.uint32)
    arrays["fwd_status"] = np.where(rng.random(n) < 0.5, nf.ST_FLAG_FWD | 2, 2).astype(np.uint8)
    if "l2_port" not in given:
        arrays["l3_port"][:] = NONE  # floods only
    desc[3]["off16"] = 0xFFFFFFFF
    desc[4]["off16"] = arena.nbytes // 16                      # starts at the arena's end
    desc[5] = (copy_base // 16 - 1, 17)                        # reaches 16 bytes into the copy region
    desc[6] = (copy_base // 16, 64)                            # lies in the copy region
    desc[7] = (copy_base // 16 - 1, 16)                        # ends exactly at copy_base: live
    for i in range(3, 8):
        arrays["l2_verdict"][i], arrays["l2_port"][i], arrays["l3_port"][i] = nf.L2_FLOOD, NONE, NONE
    args = {k: arrays[k] for k in given}
    with access_table(6) as fdb:
        want = check(engine, fdb, 1, 6, arena, desc, copy_base, 16, 6 * n, args)
    m = int(want["totals"]["items"])
    src = want["item_src"][:m]
    assert not np.isin([3, 4, 5, 6], src).any() and m > 200
    if "l2_verdict" in given:
        assert (src == 7).sum() == 5
    else:
        assert int(want["totals"]["copies"]) == 0 and int(want["totals"]["flooded"]) == 0


# ---- overflow --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap,room", sorted(CUTS))
def test_overflow_cuts(engine, cap, room):
    fdb, desc, copy_base, arrays = small_burst()
    rng = np.random.default_rng(1)
    arena = np.full(copy_base + room, FILL, np.uint8)
    arena[:copy_base] = rng.integers(0, 256, copy_base, dtype=np.uint8)
    with fdb:
        want = check(engine, fdb, 0, 4, arena, desc, copy_base, 16, cap, arrays)
    assert int(want["totals"]["items"]) == CUTS[(cap, room)] and int(want["totals"]["items_needed"]) == 9


def test_overflow_in_a_large_burst(engine):
    """cap and the region each cut in the middle of a tile that is not the first, between two copies of one
    source; then the exact fit of both."""
    n = 2 * T + 300
    rng = np.random.default_rng(8)
    frames = [rng.integers(0, 256, 40, dtype=np.uint8).tobytes() for _ in range(n)]
    with access_table(5) as fdb:
        arrays = mixed_arrays(rng, n, 5)
        arena, desc, copy_base = pack_with_tail(frames, 16, 48 * 4 * n)
        full = fdb.flood_expand_host(0, 5, arena.nbytes, copy_base, 16, desc, 4 * n, **arrays)
        items, nbytes = int(full["totals"]["items"]), int(full["totals"]["copy_bytes"])
        k = next(k for k in range(items * 2 // 3, items) if full["item_src"][k] == full["item_src"][k + 1])
        assert int(full["item_src"][k]) > T
        a = check(engine, fdb, 0, 5, arena, desc, copy_base, 16, k + 1, arrays, "cap: ")
        room = int(full["item_desc"][k + 1]["off16"]) * 16 - copy_base + 47  # one byte short of item k + 1's slot
        b = check(engine, fdb, 0, 5, arena[:copy_base + room], desc, copy_base, 16, 4 * n, arrays, "region: ", upload=False)
        c = check(engine, fdb, 0, 5, arena[:copy_base + nbytes], desc, copy_base, 16, items, arrays, "exact: ", upload=False)
    assert int(a["totals"]["items"]) == int(b["totals"]["items"]) == k + 1 < items == int(c["totals"]["items"])


# ---- the context's scratch, the upload rules, the arguments ---------------------------------------------

def test_two_bursts_back_to_back_on_one_stream(engine):
    """The second call reuses the scratch the first one left (grown to the context's minimum on first use), in
    stream order, with no host sync between them."""
    rng = np.random.default_rng(21)
    runs = []
    with access_table(5) as fdb:
        fdb.upload(engine)
        for n in (3 * T + 7, 65):
            frames = [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(n)]
            arena, desc, copy_base = pack_with_tail(frames, 16, 64 * 4 * n)
            arrays = mixed_arrays(rng, n, 5)
            want = fdb.flood_expand_host(3, 5, arena.nbytes, copy_base, 16, desc, 4 * n, **arrays)
            runs.append((Run(engine, fdb, 3, 5, arena, desc, copy_base, 16, 4 * n, arrays, upload=False, sync=False),
                         want, arena, desc, copy_base))
        engine.sync()
        for run, want, arena, desc, copy_base in runs:
            got = run.result()
            assert_same_expand(got, want)
            assert np.array_equal(got["arena"], copy_model(arena, desc, want, copy_base))


def test_upload_rules_arguments_and_no_packets(engine):
    fdb, desc, copy_base, arrays = small_burst()
    L = nf.lib()
    buf = engine.alloc(8192)
    p = buf.ptr

    def call(n=5, l3=None, st=None, l2=p, verdict=p, vlan=p, arena=p, arena_bytes=copy_base + 512, base=copy_base, align=16,
             cap=4, items=p + 4096, totals=p + 2048, d=p):
        return L.nfcs_flood_expand_device(engine.ctx, fdb.ptr, 0, 4, arena, arena_bytes, base, align, d, n, l3, st, l2, verdict,
                                          vlan, cap, items, items, items, totals, None)

    with fdb:
        assert call() == -1                                        # not uploaded
        fdb.upload(engine)
        assert call(l2=None, verdict=None, vlan=None) == -1        # both port arrays NULL
        assert call(st=p) == -1                                    # a status without the L3 ports
        assert call(vlan=None) == -1                               # a verdict without the VLANs
        for align in (0, 8, 24):
            assert call(align=align) == -1
        assert call(base=copy_base + 16, align=32) == -1 and call(base=copy_base + 1024) == -1
        assert call(arena=None) == -1 and call(d=None) == -1 and call(totals=None) == -1 and call(items=None) == -1
        assert call(arena=p + 8) == -1 and call(totals=p + 4) == -1 and call(items=p + 2) == -1 and call(l2=p + 2) == -1
        assert call(n=0, arena=None, d=None, items=None, totals=None) == 0  # n == 0: no launch, nothing written
        engine.sync()
        # the upload serves until the next upload, whatever the host object is told meanwhile
        rng = np.random.default_rng(2)
        arena = np.full(copy_base + 512, FILL, np.uint8)
        arena[:copy_base] = rng.integers(0, 256, copy_base, dtype=np.uint8)
        old = check(engine, fdb, 0, 4, arena, desc, copy_base, 16, 16, arrays, upload=False)
        fdb.set_port(2, link_up=False, native_vlan=1)
        with pytest.raises(nf.NfcsError):
            fdb.flood_expand_host(0, 4, arena.nbytes, copy_base, 16, desc, 16, **arrays)
        fdb.commit()
        got = Run(engine, fdb, 0, 4, arena, desc, copy_base, 16, 16, arrays, upload=False).result()
        assert_same_expand(got, old, "committed, not yet uploaded: ")
        new = check(engine, fdb, 0, 4, arena, desc, copy_base, 16, 16, arrays)
    assert int(old["totals"]["copies"]) == 6 and int(new["totals"]["copies"]) == 4
