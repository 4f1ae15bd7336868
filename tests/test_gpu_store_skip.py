"""Store skipping (netflow_amd/csrc/nfcs_kernels.hip row_process): the plain update's fast
path writes a checksum field only when the frame's two bytes differ from the computed value, inline or
through the engine's deferred records. Memory after a call must be what the oracle leaves for every mix
of right and wrong fields, so every burst here carries, each as at least 5% of its packets (asserted
from the oracle's before and after bytes):

  both fields already right / only IPv4 wrong / only L4 wrong / both wrong / a field wrong in its high
  byte only / one wrong in its low byte only / UDP 0x0000 where the value is 0xFFFF / UDP 0xFFFF already
  right / IPv4 0xFFFF where the value is 0x0000.

The frames are the fuzz generator's (IPv4 and IPv6, TCP, UDP and ICMP, 25% tagged, IP options, IHL < 5,
inconsistent lengths), picked by length; frames with both fields or a valid UDP checksum are all kept,
the others thinned to half, so the classes that need them reach their share. The generator's bytes are
random, so it gives a UDP or IPv4 checksum of exactly zero about once in 65,535 frames: those classes
are made by tuning one 16-bit word the other checksum does not cover (the first UDP payload word, the
IPv4 identification). Every case compares the whole arena and the status bytes with the oracle; a
second call, which finds every field right, must leave the oracle's second-call bytes: the same bytes
for every frame but the IHL < 5 overlaps, whose update is not idempotent in the reference either."""
import functools

import numpy as np
import pytest

import netflow_amd as nf
import oracle

pytestmark = pytest.mark.gpu

CLASSES = ("both_right", "only_ip_wrong", "only_l4_wrong", "both_wrong", "high_byte_only", "low_byte_only",
           "udp_zero_to_ffff", "udp_ffff_right", "ip_ffff_to_zero")
UDP_ST = (nf.ST_V4_UDP, nf.ST_V6_UDP)


def fields(arena, desc, st):
    """Per packet, from the oracle's status and the frame: the arena offsets of the IPv4 and the L4
    checksum field (-1: none), the frame offsets of the two, and whether it is an IHL < 5 overlap."""
    base = desc["off16"].astype(np.int64) * 16
    ln = desc["len"].astype(np.int64)
    safe = np.minimum(base + 13, arena.size - 1)
    tagged = (ln >= 14) & (arena[np.minimum(base + 12, arena.size - 1)] == 0x81) & (arena[safe] == 0x00)
    l2 = np.where(tagged, 18, 14)
    b = (st & 0x3F).astype(np.int64)
    has_ip = (b >= nf.ST_V4) & (b <= nf.ST_V4_L4SKIP)
    ihl = arena[np.minimum(base + l2, arena.size - 1)].astype(np.int64) & 15
    l4 = np.where(has_ip, l2 + 4 * ihl, l2 + 40)
    fo = np.select([(b == nf.ST_V4_TCP) | (b == nf.ST_V6_TCP), (b == nf.ST_V4_UDP) | (b == nf.ST_V6_UDP),
                    b == nf.ST_V4_ICMP], [l4 + 15, l4 + 6, l4 + 2], -1)
    ip_f = np.where(has_ip, l2 + 10, -1)
    return (np.where(has_ip, base + ip_f, -1), np.where(fo >= 0, base + fo, -1), ip_f, fo,
            (st & nf.ST_FLAG_OVERLAP) != 0)


def be16_at(arena, pos):
    return (arena[pos].astype(np.int64) << 8) | arena[pos + 1]


def put16(arena, pos, v):
    arena[pos] = (v >> 8) & 0xFF
    arena[pos + 1] = v & 0xFF


@functools.lru_cache(maxsize=None)
def pool():
    frames = oracle.fuzz_frames(9091, 0, 150000)
    arena, desc = oracle.pack_frames(frames)
    st, _ = oracle.update_batch(arena, desc, nthreads=8)
    ip, l4, _, _, ov = fields(arena, desc, st)
    udp = np.isin(st & 0x3F, UDP_ST)
    keep = (((ip >= 0) & (l4 >= 0)) | udp) & ~ov
    keep |= np.random.default_rng(5).integers(0, 2, len(frames)) == 0
    return [f for f, k in zip(frames, keep) if k]


def spoil(frames, seed):
    """The frames with their checksum fields set per class (the classes are counted afterwards, from
    what the oracle does to the result)."""
    rng = np.random.default_rng(seed)
    arena, desc = oracle.pack_frames(frames)
    good = arena.copy()
    st, _ = oracle.update_batch(good, desc, nthreads=8)
    ip, l4, _, _, ov = fields(good, desc, st)
    base = desc["off16"].astype(np.int64) * 16
    udp = np.isin(st & 0x3F, UDP_ST)
    out = good.copy()  # every field right; the classes below put the wrong ones back
    for i in range(len(frames)):
        if ov[i]:
            out[base[i]:base[i] + len(frames[i])] = np.frombuffer(frames[i], dtype=np.uint8)
            continue
        a, b = int(ip[i]), int(l4[i])
        r = int(rng.integers(0, 100))
        x = int(rng.integers(1, 256))
        if udp[i] and r < 60:
            # the first payload word tuned so that the sum folds to 0xFFFF: the value is 0 -> 0xFFFF
            p = b + 2
            if int(be16_at(good, b - 2)) >= 10 and p + 2 <= base[i] + len(frames[i]):
                s = (~int(be16_at(good, b))) & 0xFFFF
                w = int(be16_at(good, p))
                put16(out, p, (w - s) % 0xFFFF)
                put16(out, b, 0x0000 if r < 30 else 0xFFFF)
            continue
        if a >= 0 and b >= 0:
            k = r % 6
            if k in (1, 3): put16(out, a, int(be16_at(good, a)) ^ (x | (x << 8)))
            if k in (2, 3): put16(out, b, int(be16_at(good, b)) ^ (x | (x << 8)))
            if k == 4: out[a] ^= x
            if k == 5: out[b + 1] ^= x
        elif b >= 0:  # IPv6: one field
            k = r % 4
            if k == 1: put16(out, b, int(be16_at(good, b)) ^ (x | (x << 8)))
            if k == 2: out[b] ^= x
            if k == 3: out[b + 1] ^= x
        elif a >= 0:  # IPv4 without an L4 field: the identification tuned so that the value is 0x0000
            k = r % 4
            if k in (0, 1):
                s = (~int(be16_at(good, a))) & 0xFFFF
                put16(out, a - 6, (int(be16_at(good, a - 6)) - s) % 0xFFFF)
                put16(out, a, 0xFFFF)
            if k == 2: out[a] ^= x
            if k == 3: out[a + 1] ^= x
    return oracle.unpack_frames(out, desc)


def class_shares(before, after, desc, st):
    ip, l4, _, _, _ = fields(after, desc, st)
    hi, hl = ip >= 0, l4 >= 0
    z = np.zeros(len(desc), dtype=np.int64)
    ib, ia = np.where(hi, be16_at(before, np.maximum(ip, 0)), z), np.where(hi, be16_at(after, np.maximum(ip, 0)), z)
    lb, la = np.where(hl, be16_at(before, np.maximum(l4, 0)), z), np.where(hl, be16_at(after, np.maximum(l4, 0)), z)
    ic, lc = hi & (ib != ia), hl & (lb != la)
    udp = np.isin(st & 0x3F, UDP_ST)
    xi, xl = ib ^ ia, lb ^ la
    share = {
        "both_right": hi & hl & ~ic & ~lc,
        "only_ip_wrong": hl & ic & ~lc,
        "only_l4_wrong": hi & lc & ~ic,
        "both_wrong": ic & lc,
        "high_byte_only": (ic & ((xi & 0xFF) == 0)) | (lc & ((xl & 0xFF) == 0)),
        "low_byte_only": (ic & ((xi & 0xFF00) == 0)) | (lc & ((xl & 0xFF00) == 0)),
        "udp_zero_to_ffff": udp & (lb == 0x0000) & (la == 0xFFFF),
        "udp_ffff_right": udp & (lb == 0xFFFF) & (la == 0xFFFF),
        "ip_ffff_to_zero": hi & (ib == 0xFFFF) & (ia == 0x0000),
    }
    return {k: float(v.mean()) for k, v in share.items()}


@functools.lru_cache(maxsize=None)
def burst(kind):
    """(arena, desc, ref, rst, ref2, rst2, before-class shares) of one shape's burst; shared, never modified."""
    lo, hi, n, align, tile = {"long": (1400, 1500, 4096, 16, 1), "long128": (1400, 1500, 4096, 128, 1),
                              "deferred": (1400, 1500, 66000, 16, 16), "mix16": (64, 1500, 4096, 16, 1),
                              "mix128": (64, 1500, 4096, 128, 1), "tiny": (64, 200, 4096, 16, 1)}[kind]
    pick = [f for f in pool() if lo <= len(f) <= hi]
    m = (n + tile - 1) // tile
    assert len(pick) >= m, (kind, len(pick))
    frames = (spoil(pick[:m], 1000 + m) * tile)[:n]
    arena, desc = oracle.pack_frames(frames, align=align)
    ref = arena.copy()
    rst, _ = oracle.update_batch(ref, desc, nthreads=8)
    ref2 = ref.copy()
    rst2, _ = oracle.update_batch(ref2, desc, nthreads=8)
    for a in (arena, desc, ref, rst, ref2, rst2):
        a.setflags(write=False)
    return arena, desc, ref, rst, ref2, rst2, class_shares(arena, ref, desc, rst)


def check_mix(kind):
    arena, desc, ref, rst, ref2, rst2, shares = burst(kind)
    print(kind, {k: round(v, 4) for k, v in shares.items()})
    for k in CLASSES:
        assert shares[k] >= 0.05, (kind, k, shares[k])
    # the second call's expectation: the first call's bytes, except in IHL < 5 overlaps
    ov = fields(ref, desc, rst)[4]
    assert np.array_equal(rst2[~ov], rst[~ov])
    keep = np.ones(arena.size, dtype=bool)
    for i in np.nonzero(ov)[0]:
        o = int(desc[i]["off16"]) * 16
        keep[o:o + int(desc[i]["len"])] = False
    assert np.array_equal(ref2[keep], ref[keep])


def run_case(engine, kind, slot_bytes=0, want_patch=False):
    check_mix(kind)
    arena, desc, ref, rst, ref2, rst2, _ = burst(kind)
    n = len(desc)
    engine.set_slot_bytes(slot_bytes)
    bufs = []
    try:
        d_arena = engine.alloc(arena.nbytes).upload(arena)
        d_desc = engine.alloc(desc.nbytes).upload(desc)
        d_st = engine.alloc(n)
        bufs = [d_arena, d_desc, d_st]
        d_pt = None
        if want_patch:
            d_pt = engine.alloc(8 * n).upload(np.full(8 * n, 0xA5, dtype=np.uint8))
            bufs.append(d_pt)
        for exp, est in ((ref, rst), (ref2, rst2)):
            d_st.upload(np.full(n, 0xEE, dtype=np.uint8))
            engine.update_device(d_arena, arena.nbytes, d_desc, n, d_st, d_pt)
            engine.sync()
            assert np.array_equal(d_st.download(np.uint8, n), est)
            assert np.array_equal(d_arena.download(np.uint8, arena.nbytes), exp)
            if want_patch and exp is ref:
                check_records(d_pt.download(nf.PATCH_DTYPE, n), arena, desc, ref, rst)
    finally:
        engine.set_slot_bytes(0)
        for b in bufs:
            b.free()


def check_records(pt, before, desc, ref, rst):
    """A caller's records hold every field's offset and value, changed or not."""
    ip, l4, ip_f, l4_f, ov = fields(ref, desc, rst)
    assert np.array_equal(pt["ip_off"], np.where(ip_f >= 0, ip_f, nf.PATCH_NONE).astype(np.uint16))
    assert np.array_equal(pt["l4_off"], np.where(l4_f >= 0, l4_f, nf.PATCH_NONE).astype(np.uint16))
    for name, pos in (("ip", ip), ("l4", l4)):
        live = (pos >= 0) & ~ov
        assert np.array_equal(pt[name][live, 0], ref[pos[live]])
        assert np.array_equal(pt[name][live, 1], ref[pos[live] + 1])
    # and applied to the original frames, ip then l4, they reproduce the update (overlaps included)
    re = before.copy()
    base = desc["off16"].astype(np.int64) * 16
    for name in ("ip", "l4"):
        off = pt[name + "_off"].astype(np.int64)
        live = off != nf.PATCH_NONE
        re[base[live] + off[live]] = pt[name][live, 0]
        re[base[live] + off[live] + 1] = pt[name][live, 1]
    assert np.array_equal(re, ref)


def test_deferred_long_shape(engine):
    """66,000 frames of 1400-1500 bytes: above the inline limit, so the long waves defer to the write pass."""
    run_case(engine, "deferred")


def test_deferred_long_shape_caller_records(engine):
    run_case(engine, "deferred", want_patch=True)


@pytest.mark.parametrize("kind", ["long", "long128"])
def test_inline_long_shape(engine, kind):
    """4,096 long frames, packed at 16-byte starts (line-aligned windows off their lines) and on lines."""
    run_case(engine, kind)


@pytest.mark.parametrize("kind", ["mix16", "mix128"])
def test_inline_short_shape(engine, kind):
    """4,096 frames of 64-1500 bytes in the short shape (16-lane rows, 7 waves/SIMD; the hint picks it)."""
    run_case(engine, kind, slot_bytes=1024)


def test_inline_long_shape_mixed_lengths(engine):
    """The same mix through the long shape's line-aligned windows, short frames and all."""
    run_case(engine, "mix16", slot_bytes=4096)


def test_inline_tiny_shape(engine):
    """4,096 frames of 64-200 bytes: 8-lane rows."""
    run_case(engine, "tiny")
