"""Frames at the values where one's-complement arithmetic goes wrong, for tests/test_value_edges.py
(CPU), tests/test_gpu_value_edges.py and tests/golden/make_value_edges_golden.py. Deterministic: fixed seeds only.

Base frames: untagged and 802.1Q-tagged; IPv4 with IHL 5, 6, 7, 15 and (the overlap path) 3 and 4, IPv6; UDP, TCP,
ICMP; even and odd L4 lengths; frame lengths in three bands (64-200, 600-1000, 1400-1500 bytes); TTL 2, 64, 255.

Tuned classes, each made by moving one 16-bit word that only the targeted sum covers (the IPv4 identification, the
first L4 payload word) in a fixed order: ask the oracle for the checksum it computes, move the word by the
difference mod 0xFFFF, ask again and assert:

  udp4_zero_to_ffff, udp6_zero_to_ffff   UDP computes 0, the field becomes 0xFFFF
  tcp_zero, icmp_zero                    the field becomes 0x0000 (and must not get the UDP rule)
  ip_zero                                the IPv4 header checksum 0x0000: one variant tuned for the plain update, one
                                         tuned through oracle.l3_forward_frame (the value after ttl--)
  ip_zero_and_udp_ffff                   both in one frame, again one variant per operation
  icmp_sum_zero                          ICMP type 0 code 0 with a region of zeros: the exact sum is 0, the field 0xFFFF
  second_fold, second_fold_le            the L4 checksum's exact sum gives at least 0x10000 in its first fold step: the
                                         reference's sum over big-endian words, and the sum over little-endian words
                                         that a kernel loading dwords folds. The two are congruent mod 0xFFFF but are
                                         other exact values, and one frame cannot in general need the step in both
                                         (each sum's low byte is fixed by the other's high byte), so each has its frames
  ip_second_fold, ip_second_fold_le      the same for the IPv4 header's sum: made in the second_fold(_le) frames for
                                         the update, and for the forward (ttl-- moves the sum) in the odd_tail_ff
                                         frames (big-endian) and the icmp_sum_zero frames (little-endian)
  odd_tail_ff                            odd L4 length, last byte 0xFF

second_fold has one frame per position (re - 1) mod 16 in 0..15 of the region's last byte in its 16-byte chunk;
odd_tail_ff one per even position: the L4 header starts at an even frame offset, so an odd length ends on one.
The IHL < 5 frames' update is not linear in one word (the pseudo-header covers L4 bytes): there all 65,536 values
of one payload word are tried in a single oracle.update_batch call.

Saturated frames (payload, addresses, ports and the free header words all 0xFF): the maximum frames of
test_gpu_edges.max_frames, and ladders of frame lengths across every row-pass boundary (752..784, 1520..1552,
6128..6160 bytes in 2-byte steps, plus the odd lengths between), also with an all-zero payload."""
import functools
import struct

import numpy as np

import netflow_amd as nf
import oracle

SEED = 20251021
BANDS = {"tiny": (64, 200), "short": (600, 1000), "long": (1400, 1500)}
BURST_N = 4096
DEFERRED_N = 66000
TTLS = (2, 64, 255)
NH_TABLE = np.frombuffer(bytes(range(0x10, 0x10 + 48)), np.uint8).reshape(4, 12).copy()
NH_TABLE.setflags(write=False)
PUSH_OP = oracle.vlan_op("push", 4094, 6)
POP_OP = oracle.vlan_op("pop")
CLASSES = ("udp4_zero_to_ffff", "udp6_zero_to_ffff", "tcp_zero", "icmp_zero", "ip_zero", "ip_zero_and_udp_ffff",
           "icmp_sum_zero", "second_fold", "second_fold_le", "ip_second_fold", "ip_second_fold_le", "odd_tail_ff")
# the slots a burst cycles through: 13 of them, so the next-hop index (i mod 5) meets every slot
SLOTS = ("udp4_zero_to_ffff", "udp6_zero_to_ffff", "tcp_zero", "icmp_zero", "ip_zero", "ip_zero:fwd",
         "ip_zero_and_udp_ffff", "ip_zero_and_udp_ffff:fwd", "icmp_sum_zero", "second_fold", "second_fold_le", "odd_tail_ff",
         "plain")


# ---- the reference's sum in Python integers (unbounded: nothing can overflow) ------------------------------

def py_sum(b) -> int:
    """Packet::calculate_checksum before its fold: big-endian 16-bit words, an odd last byte as the LOW byte."""
    b = bytes(b)
    n = len(b) & ~1
    s = sum(struct.unpack(">%dH" % (n // 2), b[:n]))
    return s + (b[-1] if len(b) & 1 else 0)


def py_finish(s: int) -> int:
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return (~s) & 0xFFFF


def py_checksum(b) -> int:
    return py_finish(py_sum(b))


def be16(v):
    return bytes([(v >> 8) & 0xFF, v & 0xFF])


def get16(f, o):
    return (f[o] << 8) | f[o + 1]


def put16(f, o, v):
    f[o], f[o + 1] = (v >> 8) & 0xFF, v & 0xFF


# ---- geometry of a well-formed frame -------------------------------------------------------------------------

def geom(f):
    """Of a frame the builder made (headers whole, lengths consistent): l2, v4, l4, proto, the IPv4 and L4 checksum
    field offsets (-1: none), the L4 region's length and the offset of the first payload word."""
    l2 = 18 if f[12] == 0x81 and f[13] == 0x00 else 14
    v4 = (f[l2] >> 4) == 4
    if v4:
        ihl4 = (f[l2] & 15) * 4
        l4, proto, L = l2 + ihl4, f[l2 + 9], get16(f, l2 + 2) - ihl4
    else:
        l4, proto, L = l2 + 40, f[l2 + 6], get16(f, l2 + 4)
    if proto == 17:
        L = get16(f, l4 + 4)
    fo, po = {17: (l4 + 6, l4 + 8), 6: (l4 + 15, l4 + 20), 1: (l4 + 2, l4 + 8)}[proto]
    return {"l2": l2, "v4": v4, "l4": l4, "proto": proto, "ip_f": l2 + 10 if v4 else -1, "l4_f": fo, "L": L, "pay": po,
            "re": l4 + L, "overlap": v4 and l4 < l2 + 20}


def l4_exact_sum(f) -> int:
    """The exact sum the reference folds for the frame's L4 checksum (pseudo-header and region, the field as zero);
    for frames without the IHL < 5 overlap."""
    g = geom(f)
    r = bytearray(f[g["l4"]:g["re"]])
    r[g["l4_f"] - g["l4"]] = r[g["l4_f"] - g["l4"] + 1] = 0
    s = py_sum(r)
    if g["proto"] == 1:
        return s
    if g["v4"]:
        return s + py_sum(f[g["l2"] + 12:g["l2"] + 20]) + g["proto"] + g["L"]
    return s + py_sum(f[g["l2"] + 8:g["l2"] + 40]) + (g["L"] >> 16) + (g["L"] & 0xFFFF) + g["proto"]


def ip_exact_sum(f) -> int:
    g = geom(f)
    h = bytearray(f[g["l2"]:g["l4"]])
    h[10] = h[11] = 0
    return py_sum(h)


def first_fold(s: int) -> int:
    return (s & 0xFFFF) + (s >> 16)


def le_sum(b) -> int:
    """The same sum taken over little-endian words, as a kernel that loads dwords takes it: congruent to the byte
    swap of py_sum mod 0xFFFF, but another exact value, so it needs the second fold step on other frames. The odd
    last byte, the low byte of the reference's word, weighs 256 here."""
    b = bytes(b)
    n = len(b) & ~1
    return sum(struct.unpack("<%dH" % (n // 2), b[:n])) + ((b[-1] << 8) if len(b) & 1 else 0)


def swap16(v):
    return ((v & 0xFF) << 8) | (v >> 8)


def l4_exact_sum_le(f) -> int:
    g = geom(f)
    r = bytearray(f[g["l4"]:g["re"]])
    r[g["l4_f"] - g["l4"]] = r[g["l4_f"] - g["l4"] + 1] = 0
    s = le_sum(r)
    if g["proto"] == 1:
        return s
    if g["v4"]:
        return s + le_sum(f[g["l2"] + 12:g["l2"] + 20]) + swap16(g["proto"]) + swap16(g["L"])
    return s + le_sum(f[g["l2"] + 8:g["l2"] + 40]) + swap16(g["L"] >> 16) + swap16(g["L"] & 0xFFFF) + swap16(g["proto"])


def ip_exact_sum_le(f) -> int:
    g = geom(f)
    h = bytearray(f[g["l2"]:g["l4"]])
    h[10] = h[11] = 0
    return le_sum(h)


def fold_word(b, off, exact, le=False, delta=0):
    """The word at `off` of b set so that exact(b) + delta gives at least 0x10000 in its first fold step: its low
    16 bits become 0xFFFF. le: exact sums little-endian words."""
    put16(b, off, 0)
    v = 0xFFFF - ((exact(b) + delta) & 0xFFFF)
    put16(b, off, swap16(v) if le else v)
    assert first_fold(exact(b) + delta) >= 0x10000, (off, le)


# ---- base frames ---------------------------------------------------------------------------------------------

def base_frame(tag, ipv, ihl, proto, n, ttl=64, seed=0, hdr=None, pay=None, icmp_type=8):
    """One frame of n bytes. hdr / pay: None for fixed-seed random bytes, or the fill byte of the header fields
    that are free and of the L4 payload."""
    rng = np.random.default_rng([SEED, seed, n, ihl, proto, tag])

    def fill(k, v):
        return rng.integers(0, 256, k, dtype=np.uint8).tobytes() if v is None else bytes([v]) * k

    eth = bytearray(fill(12, hdr))
    if hdr is None:
        eth[0] &= 0xFE
    if tag:
        eth += b"\x81\x00" + fill(2, hdr)
    l2 = len(eth) + 2
    ip = bytearray(fill(n - l2, hdr))
    if ipv == 4:
        eth += b"\x08\x00"
        l4 = ihl * 4
        ip[0] = 0x40 | ihl
        put16(ip, 2, n - l2)
        if hdr is None:
            put16(ip, 6, 0)
        ip[8], ip[9] = ttl, proto
    else:
        eth += b"\x86\xdd"
        l4 = 40
        ip[0] = 0x60 | (ip[0] & 15)
        put16(ip, 4, n - l2 - 40)
        ip[6], ip[7] = proto, ttl
    L = n - l2 - l4
    po = l4 + {17: 8, 6: 20, 1: 8}[proto]
    assert L >= po - l4 + 2 and n >= l2 + 20, (n, ihl, proto)
    ip[po:] = fill(len(ip) - po, pay)
    if proto == 17:
        put16(ip, l4 + 4, L)
    elif proto == 6:
        ip[l4 + 12] = 0x50 if hdr is None else 0xFF
    else:
        ip[l4], ip[l4 + 1] = (icmp_type, 0) if hdr is None else (hdr, hdr)
    return bytes(eth + ip)


def band_specs(band):
    """The base frames of one band: (tag, ipv, ihl, proto, parity of the L4 length, ttl)."""
    out = []
    for tag in (0, 1):
        for ipv, ihl in ((4, 5), (4, 6), (4, 7), (4, 15), (6, 0), (4, 3), (4, 4)):
            for proto in ((17, 6) if ipv == 6 else (17, 6, 1)):
                for odd in (0, 1):
                    out.append((tag, ipv, ihl, proto, odd, TTLS[len(out) % 3]))
    return out


def spec_len(band, spec, k, pos=None):
    """A frame length in the band with the spec's parity; pos: (re - 1) mod 16 of the frame's last byte."""
    lo, hi = BANDS[band]
    tag, ipv, ihl, proto, odd, _ = spec
    floor = (18 if tag else 14) + max(40 if ipv == 6 else ihl * 4, 20) + {17: 8, 6: 20, 1: 8}[proto] + 2
    lo = max(lo, floor)
    rng = np.random.default_rng([SEED, 7, k, lo, hi])
    n = int(rng.integers(lo, hi + 1))
    if pos is None:
        n -= (n - odd) & 1
        return n if n >= lo else n + 2
    n = lo + ((pos + 1 - lo) % 16) + 16 * int(rng.integers(0, (hi - lo - 15) // 16 + 1))
    assert lo <= n <= hi and (n - 1) % 16 == pos
    return n


# ---- tuning --------------------------------------------------------------------------------------------------

def _after(f, op):
    if op == "fwd":
        out, st = oracle.l3_forward_frame(bytes(f), bytes(NH_TABLE[1]))
        assert st & nf.ST_FLAG_FWD, st
        return out
    return oracle.update_frame(bytes(f))[0]


def tune(f, word_off, field_off, target, op="upd"):
    """Move the word at word_off so that the oracle writes `target` into the field at field_off (as computed: a UDP
    0 reads back as 0xFFFF). The fixed order: ask, move by the difference mod 0xFFFF, ask again and assert."""
    f = bytearray(f)
    c = get16(_after(f, op), field_off)
    if c == 0xFFFF and target == 0 and field_is_udp(f, field_off):
        return bytes(f)  # already computes 0
    s = (~c) & 0xFFFF  # the folded sum now
    want = (~target) & 0xFFFF
    put16(f, word_off, (get16(f, word_off) - s + want) % 0xFFFF)
    got = get16(_after(f, op), field_off)
    assert got == (0xFFFF if target == 0 and field_is_udp(f, field_off) else target), (hex(got), hex(target))
    return bytes(f)


def field_is_udp(f, field_off):
    g = geom(f)
    return g["proto"] == 17 and field_off == g["l4_f"]


def search_overlap(f, target):
    """IHL < 5: every value of the first payload word in one oracle.update_batch call; the first that leaves
    `target` in the L4 field."""
    g = geom(f)
    n = len(f)
    slot = (n + 15) // 16 * 16
    arena = np.zeros((65536, slot), np.uint8)
    arena[:, :n] = np.frombuffer(bytes(f), np.uint8)
    v = np.arange(65536)
    arena[:, g["pay"]], arena[:, g["pay"] + 1] = v >> 8, v & 0xFF
    desc = np.zeros(65536, oracle.DESC_DTYPE)
    desc["off16"], desc["len"] = np.arange(65536) * (slot // 16), n
    flat = arena.reshape(-1)
    oracle.update_batch(flat, desc, nthreads=8, want_result=False)
    after = flat.reshape(65536, slot)
    got = (after[:, g["l4_f"]].astype(np.int64) << 8) | after[:, g["l4_f"] + 1]
    hit = np.flatnonzero(got == target)
    assert len(hit), (hex(target), n)
    out = bytearray(f)
    put16(out, g["pay"], int(hit[0]))
    assert get16(oracle.update_frame(bytes(out))[0], g["l4_f"]) == target
    return bytes(out)


def spoil_field(f, off, v):
    f = bytearray(f)
    put16(f, off, v)
    return bytes(f)


def make(cls, band, spec, k, pos=None):
    """The frame of one slot: the spec's base frame, tuned for the class."""
    cls, _, op = cls.partition(":")
    op = op or "upd"
    tag, ipv, ihl, proto, odd, ttl = spec
    n = spec_len(band, spec, k, pos)
    f = base_frame(tag, ipv, ihl, proto, n, ttl, seed=k, icmp_type=0 if cls == "icmp_sum_zero" else 8)
    g = geom(f)
    if cls == "plain":
        return f
    if cls == "icmp_sum_zero":
        b = bytearray(f)
        b[g["l4"] + 1:] = bytes(len(b) - g["l4"] - 1)
        put16(b, g["l4_f"], 0x1234)  # a stale field: it is taken as zero, the region's exact sum is 0
        fold_word(b, g["l2"] + 4, ip_exact_sum_le, le=True, delta=-1)  # the header's, after the forward's ttl--
        return bytes(b)
    if cls == "odd_tail_ff":
        assert g["L"] & 1
        b = bytearray(f[:-1] + b"\xff")
        if g["v4"]:  # and the IPv4 header's second fold step after the forward's ttl--, in both byte orders
            fold_word(b, g["l2"] + 4, ip_exact_sum, delta=-0x100)
        return bytes(b)
    if cls == "second_fold":
        b = bytearray(f)
        fold_word(b, g["pay"], l4_exact_sum)
        if g["v4"]:
            fold_word(b, g["l2"] + 4, ip_exact_sum)
        return bytes(b)
    if cls == "second_fold_le":
        b = bytearray(f)
        fold_word(b, g["pay"], l4_exact_sum_le, le=True)
        if g["v4"]:
            fold_word(b, g["l2"] + 4, ip_exact_sum_le, le=True)
        return bytes(b)
    if g["overlap"]:
        target = 0xFFFF if proto == 17 else 0x0000
        return search_overlap(f, target)
    if cls in ("udp4_zero_to_ffff", "udp6_zero_to_ffff", "tcp_zero", "icmp_zero", "ip_zero_and_udp_ffff"):
        f = tune(f, g["pay"], g["l4_f"], 0)
        # the stale field: UDP 0x0000 (the value a UDP sender that computes 0 must not send), the others 0xFFFF
        f = spoil_field(f, g["l4_f"], 0x0000 if proto == 17 else 0xFFFF)
    if cls in ("ip_zero", "ip_zero_and_udp_ffff"):
        f = tune(f, g["l2"] + 4, g["ip_f"], 0, op)
        f = spoil_field(f, g["ip_f"], 0xFFFF)
    return f


def compatible(slot, spec):
    tag, ipv, ihl, proto, odd, ttl = spec
    cls = slot.partition(":")[0]
    over = ipv == 4 and ihl < 5
    if cls == "plain":
        return True
    if cls in ("udp4_zero_to_ffff",):
        return ipv == 4 and proto == 17
    if cls == "udp6_zero_to_ffff":
        return ipv == 6 and proto == 17
    if cls == "tcp_zero":
        return proto == 6
    if cls == "icmp_zero":
        return proto == 1
    if cls == "ip_zero":
        return ipv == 4 and not over
    if cls == "ip_zero_and_udp_ffff":
        return ipv == 4 and proto == 17 and not over
    if cls == "icmp_sum_zero":
        return proto == 1 and not over
    if cls in ("second_fold", "second_fold_le"):
        return not over
    if cls == "odd_tail_ff":
        return odd == 1 and not over
    raise KeyError(slot)


@functools.lru_cache(maxsize=None)
def band_frames(band):
    """{name: frame} of the band's distinct frames and, per slot, the list of its names in cycling order."""
    specs = band_specs(band)
    frames, by_slot = {}, {}
    for slot in SLOTS:
        names = []
        mine = [s for s in specs if compatible(slot, s)]
        positions = {"second_fold": range(16), "second_fold_le": range(16), "odd_tail_ff": range(0, 16, 2)}.get(slot, (None,))
        k = 0
        for pos in positions:
            for j, spec in enumerate(mine):
                if pos is not None and (j // 2) % 4 != (pos // 2) % 4:
                    continue  # every position with a quarter of the specs: the set stays small
                p = pos
                if pos is not None and slot.startswith("second_fold") and (pos & 1) != (0 if spec[4] else 1):
                    continue  # an even L4 length ends on an odd position
                name = f"{band}/{slot}/{'t' if spec[0] else 'u'}-v{spec[1]}-ihl{spec[2]}-p{spec[3]}-{'odd' if spec[4] else 'even'}" \
                       f"-ttl{spec[5]}" + ("" if pos is None else f"-pos{pos}")
                frames[name] = make(slot, band, spec, k, p)
                names.append(name)
                k += 1
        assert names, slot
        by_slot[slot] = names
    return frames, by_slot


@functools.lru_cache(maxsize=None)
def burst_names(kind):
    """The names of a burst's frames in order: the slots cycled, each slot cycling over its own frames."""
    if kind == "deferred":
        base = burst_names("long")
        return (base * (DEFERRED_N // len(base) + 1))[:DEFERRED_N]
    if kind == "saturated":
        return list(saturated_frames())
    _, by_slot = band_frames(kind)
    return [by_slot[SLOTS[i % len(SLOTS)]][(i // len(SLOTS)) % len(by_slot[SLOTS[i % len(SLOTS)]])] for i in range(BURST_N)]


def burst_frames(kind):
    src = saturated_frames() if kind == "saturated" else band_frames("long" if kind == "deferred" else kind)[0]
    return [src[nm] for nm in burst_names(kind)]


# ---- saturated frames ------------------------------------------------------------------------------------------

LADDERS = ((752, 784), (1520, 1552), (6128, 6160))


@functools.lru_cache(maxsize=None)
def saturated_frames():
    out = {}
    for tag in (0, 1):
        l2 = 18 if tag else 14
        for proto in (17, 6, 1):
            out[f"sat/max-v4-p{proto}-{'t' if tag else 'u'}"] = base_frame(tag, 4, 5, proto, l2 + 65535, 255, hdr=0xFF, pay=0xFF)
        out[f"sat/max-v6-p17-{'t' if tag else 'u'}"] = base_frame(tag, 6, 0, 17, l2 + 40 + 65535, 255, hdr=0xFF, pay=0xFF)
    for lo, hi in LADDERS:
        for n in range(lo, hi + 1):
            for pay in (0xFF, 0x00):
                if (n & 1) and pay == 0:
                    continue  # the issue's ladder is the even lengths; the odd ones ride along with 0xFF only
                for tag, ipv, proto in ((0, 4, (17, 6, 1)[(n // 2) % 3]), (1, 4, (6, 1, 17)[(n // 2) % 3]), (0, 6, 17), (1, 6, 6)):
                    out[f"sat/ladder-{n}-{pay:02x}-v{ipv}-p{proto}-{'t' if tag else 'u'}"] = \
                        base_frame(tag, ipv, 5 if ipv == 4 else 0, proto, n, 255, hdr=0xFF, pay=pay)
    return out


@functools.lru_cache(maxsize=None)
def named_frames():
    """Every distinct frame, in a fixed order: the three bands, then the saturated ones."""
    out = {}
    for band in BANDS:
        out.update(band_frames(band)[0])
    out.update(saturated_frames())
    return out


# ---- what the fixture records ----------------------------------------------------------------------------------

OPS = ("upd", "fwd", "push", "pop")


def frame_hash(f: bytes) -> int:
    b = np.frombuffer(bytes(f) + bytes(16), dtype=np.uint8).copy()
    return int(oracle.lib().nfo_frame_hash(oracle._ptr(b), len(f)))


def fields_of(f: bytes):
    """The IPv4 and the L4 checksum field of a frame as the reference's parse finds them: (value or -1, value or -1)."""
    if len(f) < 34:
        return -1, -1
    l2 = 18 if f[12:14] == b"\x81\x00" else 14
    et = get16(f, l2 - 2)
    if l2 + 20 <= len(f) and (f[l2] >> 4) == 4:
        ip, proto, l4 = get16(f, l2 + 10), f[l2 + 9], l2 + (f[l2] & 15) * 4
    elif et == 0x86DD and l2 + 40 <= len(f) and (f[l2] >> 4) == 6:
        ip, proto, l4 = -1, f[l2 + 6], l2 + 40
    else:
        return -1, -1
    fo = {17: l4 + 6, 6: l4 + 15}.get(proto, l4 + 2 if proto == 1 and ip >= 0 else -1)
    return ip, (get16(f, fo) if fo >= 0 and fo + 2 <= len(f) else -1)


def record(run):
    """The fixture's arrays: run(op, frame) -> (what the operation returned, its output frame), over named_frames()."""
    frames = named_frames()
    n = len(frames)
    out = {"seed": np.uint64(SEED), "n": np.uint32(n),
           "h_in": np.array([frame_hash(f) for f in frames.values()], np.uint64)}
    for op in OPS:
        ret, ip, l4, ln = (np.zeros(n, np.int32) for _ in range(4))
        h = np.zeros(n, np.uint64)
        for i, f in enumerate(frames.values()):
            ret[i], o = run(op, f)
            ip[i], l4[i] = fields_of(o)
            ln[i], h[i] = len(o), frame_hash(o)
        out.update({f"{op}_ret": ret, f"{op}_ip": ip, f"{op}_l4": l4, f"{op}_len": ln, f"{op}_hash": h})
    return out


# ---- classes, counted from the oracle's before and after bytes ---------------------------------------------------

def classes_of(before, after, st):
    """The tuned classes a frame belongs to, from its bytes before and after an operation (update or forward) and the
    operation's status."""
    b = st & 0x3F
    out = set()
    known = b in (nf.ST_V4_TCP, nf.ST_V4_UDP, nf.ST_V4_ICMP, nf.ST_V6_TCP, nf.ST_V6_UDP)
    if not known or (st & nf.ST_FLAG_OVERLAP):
        if known:
            g = geom(before)
            v = get16(after, g["l4_f"])
            if g["proto"] == 17 and v == 0xFFFF:
                out.add("udp4_zero_to_ffff")
            if g["proto"] == 6 and v == 0:
                out.add("tcp_zero")
            if g["proto"] == 1 and v == 0:
                out.add("icmp_zero")
        return out
    g = geom(after)
    l4v = get16(after, g["l4_f"])
    ipv = get16(after, g["ip_f"]) if g["v4"] else None
    changed_l4 = get16(before, g["l4_f"]) != l4v
    if g["proto"] == 17 and l4v == 0xFFFF and changed_l4:
        out.add("udp4_zero_to_ffff" if g["v4"] else "udp6_zero_to_ffff")
    if g["proto"] == 6 and l4v == 0 and changed_l4:
        out.add("tcp_zero")
    if g["proto"] == 1 and l4v == 0 and changed_l4:
        out.add("icmp_zero")
    if ipv == 0 and get16(before, g["ip_f"]) != 0:
        out.add("ip_zero")
        if g["proto"] == 17 and l4v == 0xFFFF:
            out.add("ip_zero_and_udp_ffff")
    if g["proto"] == 1 and l4v == 0xFFFF and l4_exact_sum(after) == 0:
        out.add("icmp_sum_zero")
    if first_fold(l4_exact_sum(after)) >= 0x10000:
        out.add("second_fold")
    if first_fold(l4_exact_sum_le(after)) >= 0x10000:
        out.add("second_fold_le")
    if g["v4"] and first_fold(ip_exact_sum(after)) >= 0x10000:
        out.add("ip_second_fold")
    if g["v4"] and first_fold(ip_exact_sum_le(after)) >= 0x10000:
        out.add("ip_second_fold_le")
    if (g["L"] & 1) and after[g["re"] - 1] == 0xFF:
        out.add("odd_tail_ff")
    return out


def shares(names, frames_before, frames_after, status, keep=None):
    """Share of each class among the burst's frames (or those where keep is set)."""
    memo, count, total = {}, dict.fromkeys(CLASSES, 0), 0
    for i, nm in enumerate(names):
        if keep is not None and not keep[i]:
            continue
        total += 1
        key = (nm, int(status[i]), frames_after[i])
        if key not in memo:
            memo[key] = classes_of(frames_before[i], frames_after[i], int(status[i]))
        for c in memo[key]:
            count[c] += 1
    return {c: count[c] / max(total, 1) for c in CLASSES}


def nh_index(n):
    return (np.arange(n) % 5).astype(np.uint32)  # 4 = no route


# ---- ICMP: echo requests whose replies carry the values -----------------------------------------------------------

def icmp_request(payload, ident=0x1234, seq=2, ip_ident=7, ttl=64):
    from icmp_common import HOST, ME, ipv4
    return ipv4(HOST, ME, 1, struct.pack(">BBHHH", 8, 0, 0, ident, seq) + bytes(payload), ttl=ttl, ident=ip_ident)


def reply_of(icmp, fib, frame, verdict=None, ip_id=0):
    """The message Icmp.respond_host builds for one frame."""
    from icmp_common import messages_of, pack_with_region
    arena, desc, msg_base = pack_with_region([frame], 16, (len(frame) + 64 + 127) // 128 * 128, 128)
    v = np.array([nf.RT_LOCAL if verdict is None else verdict], np.uint8)
    out = icmp.respond_host(fib, 1, arena, msg_base, 128, desc, v, 1, ip_id=np.array([ip_id], np.uint16))
    msgs = messages_of(arena, out)
    assert len(msgs) == 1, out["status"]
    return msgs[0][2]


def tune_reply(icmp, fib, payload, target, **kw):
    """An echo request whose reply's ICMP checksum is `target`: the first payload word moved, in the fixed order."""
    p = bytearray(payload)
    c = get16(reply_of(icmp, fib, icmp_request(p, **kw)), 36)
    put16(p, 0, (get16(p, 0) - ((~c) & 0xFFFF) + ((~target) & 0xFFFF)) % 0xFFFF)
    f = icmp_request(p, **kw)
    assert get16(reply_of(icmp, fib, f), 36) == target
    return f


def icmp_cases(icmp, fib):
    """[(class, frame, verdict, ip_id)]: echo requests whose replies are icmp_zero, icmp_sum_zero, second_fold (and
    second_fold_le), odd_tail_ff and saturated (all-0xFF payloads of 1..2,000 bytes and of 65,507), and TTL-expired originals that
    are saturated."""
    from icmp_common import FAR, HOST, ipv4
    rng = np.random.default_rng([SEED, 99])
    out = []
    for k, n in enumerate((2, 3, 18, 19, 56, 57, 100, 101, 700, 701, 1472, 1473, 1494, 1495, 3 * 1536 - 42, 3 * 1536 - 41)):
        pay = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        out.append(("icmp_zero", tune_reply(icmp, fib, pay, 0x0000, ident=int(rng.integers(0, 65536)), seq=k), nf.RT_LOCAL, 0))
    for n in (0, 1, 2, 17, 64, 1473, 1536 - 42, 3000):
        out.append(("icmp_sum_zero", icmp_request(bytes(n), ident=0, seq=0), nf.RT_LOCAL, 0))
    for pos in range(16):  # the reply's last byte at every position of its chunk: reply length 42 + n
        n = 64 + 32 * pos + ((pos + 1 - 42 - 64 - 32 * pos) % 16)
        assert (42 + n - 1) % 16 == pos
        pay = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        put16(pay, 0, 0)
        f = icmp_request(pay, ident=0xFFFF, seq=0xFFFF)
        s0 = py_sum(reply_of(icmp, fib, f)[34:36]) + py_sum(reply_of(icmp, fib, f)[38:])
        put16(pay, 0, 0xFFFF - (s0 & 0xFFFF))
        f = icmp_request(pay, ident=0xFFFF, seq=0xFFFF)
        m = reply_of(icmp, fib, f)
        assert first_fold(py_sum(m[34:36]) + py_sum(m[38:])) >= 0x10000
        out.append(("second_fold", f, nf.RT_LOCAL, 0))
        put16(pay, 0, 0)  # and the little-endian sum's, in a frame of its own (a kernel sums the bytes as it loads them)
        m = reply_of(icmp, fib, icmp_request(pay, ident=0xFFFF, seq=0xFFFF))
        put16(pay, 0, swap16(0xFFFF - ((le_sum(m[34:36]) + le_sum(m[38:])) & 0xFFFF)))
        f = icmp_request(pay, ident=0xFFFF, seq=0xFFFF)
        m = reply_of(icmp, fib, f)
        assert first_fold(le_sum(m[34:36]) + le_sum(m[38:])) >= 0x10000
        out.append(("second_fold_le", f, nf.RT_LOCAL, 0))
        if n & 1:
            out.append(("odd_tail_ff", icmp_request(bytes(pay[:-1]) + b"\xff", ident=pos, seq=pos), nf.RT_LOCAL, 0))
    for n in list(range(1, 2001)) + [65507]:
        out.append(("saturated", icmp_request(b"\xff" * n, ident=0xFFFF, seq=0xFFFF, ip_ident=0xFFFF, ttl=255), nf.RT_LOCAL, 0))
    for k, n in enumerate((28, 29, 35, 36, 64, 1500, 6144)):  # TTL expired in transit: originals of 0xFF from HOST to FAR
        for ihl in (5, 15):
            f = bytearray(ipv4(HOST, FAR, 17, b"\xff" * n, ttl=1, ihl=ihl, ident=0xFFFF))
            f[15] = 0xFF
            f[20:22] = b"\xff\xff"
            f[34:14 + 4 * ihl] = b"\xff" * (4 * ihl - 20)
            out.append(("saturated_error", bytes(f), nf.RT_TTL_EXPIRED, 0xFFFF if k & 1 else 0xFF00 + k))
    return out
