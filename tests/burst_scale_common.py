"""Builders and independent models for the burst-scale tests: the enqueue, flood and ICMP stages
at sizes where the code that joins their 1,024-packet tiles does more than the trivial thing.

The models (eq_model, flood_model, flood_arena_model, icmp_model) are numpy and Python integers only and never call
the library: they restate each stage as a stable sort or a cumulative sum over the whole burst, where the library's
host walks (Egress.enqueue_host, Fdb.flood_expand_host, Icmp.respond_host) step through the packets one by one and
the kernels scan tile by tile. The builders tile a handful of templates with numpy into 64-byte slots, stamp every
frame with its packet index (so that a copy or message made from the wrong packet differs in its bytes, not only in
its list entry) and plant the packets that the cut cases cut at."""
import functools
import struct

import numpy as np

import netflow_amd as nf
from icmp_common import FAR, HOST, ME, ipv4

T = nf.EGRESS_TILE_PKTS
assert T == nf.FLOOD_TILE_PKTS == nf.ICMP_TILE_PKTS == 1024
Q = nf.QOS_MAX_QUEUES
NONE = 0xFFFFFFFF
SLOT = 64     # bytes per source frame slot
TAIL = 959    # n = tiles * T - TAIL: the last tile holds 65 packets

# nfcs_kernels.hip, as read for these lists: `constexpr uint32_t kEgSegs = 16`, the `t += 8u` loop of
# egress_scan_tiles_kernel with its `uint32_t v[8]`, and `constexpr uint32_t kFloodScanThreads = 256`.
EG_SEGS, EG_GROUP, SCAN = 16, 8, 256
# egress_scan_tiles_kernel: per = ceil(tiles / kEgSegs) tiles per segment, walked in groups of 8.
#   16: per 1, every segment one tile         17: per 2, segments 9..15 empty (min(seg * per, tiles))
#   33: per 3, segment 10 the last            128: per 8, exactly one full group per segment
#   129: per 9, a second group of one tile; segment 14 has 3 tiles, 15 none
#   137: per 9, segment 15 has 2 tiles        145: per 10, segment 14 ends inside its first group, 15 * 10 > 145
#   257: per 17, three groups (8, 8, 1); segment 15 has 2 tiles
EQ_TILES = [16, 17, 33, 128, 129, 137, 145, 257]
EQ_EXACT = [16, 128, 256]  # also n = tiles * T exactly
# flood_scan_kernel: `for (base = 0; base < tiles; base += kFloodScanThreads)`: one trip up to 256 tiles, the
# second from tile 256, the third from tile 512.
SCAN_TILES = [255, 256, 257, 512, 513]
ICMP_TILES = [256, 257, 513]


def round_up(x, a):
    return (x + a - 1) // a * a


def burst_n(tiles, exact=False):
    return tiles * T - (0 if exact else TAIL)


def eq_segments(tiles):
    """(per, [(t0, t1)] for the 16 segments), as egress_scan_tiles_kernel splits the tiles."""
    per = -(-tiles // EG_SEGS)
    return per, [(min(s * per, tiles), min(min(s * per, tiles) + per, tiles)) for s in range(EG_SEGS)]


def eq_last_segment(tiles):
    """(t0, t1) of the last segment that holds a tile."""
    return [s for s in eq_segments(tiles)[1] if s[1] > s[0]][-1]


def eq_last_full_segment(tiles):
    """(t0, t1) of the last segment of `per` tiles."""
    per, segs = eq_segments(tiles)
    return [s for s in segs if s[1] - s[0] == per][-1]


# ---- the enqueue -------------------------------------------------------------------------------------------

DEPTHS = (3, 40, 1000, 100000)


def eq_table(name):
    """[(port_id, has_qos, num_queues, max_queue_depth)] of the tables the tests use.
    one_key: one port with one queue. keys64: 8 ports x 8 queues, the 64 keys of one workgroup of the tile scan.
    keys65: the same and port 8 with one queue: 65 keys in use, key 64 alone in the second workgroup (the table's
    key count is a multiple of 8: 72). small12: the 12-port table of test_gpu_egress.py. big8192: 1,024 x 8."""
    if name == "one_key":
        return [(0, True, 1, 5000)]
    if name in ("keys64", "keys65"):
        return [(p, True, 8, DEPTHS[p % 4]) for p in range(8)] + ([(8, True, 1, 100000)] if name == "keys65" else [])
    if name == "small12":
        return [(p, p != 7, 1 + p % 8, DEPTHS[p % 4]) for p in range(12) if p != 5]
    if name == "big8192":
        return [(p, True, 8, 1 + p % 3) for p in range(1024)]
    raise KeyError(name)


def eq_port_arrays(rows):
    """(has_qos, num_queues, max_queue_depth) per port id below the highest + 1; a port never set has no QoS."""
    nports = max(r[0] for r in rows) + 1
    has, nq, maxd = np.zeros(nports, bool), np.zeros(nports, np.int64), np.zeros(nports, np.int64)
    for p, h, q, d in rows:
        has[p], nq[p], maxd[p] = h, max(q, 1), max(d, 1)  # validate_and_prepare: 0 reads as 1
    return has, nq, maxd


def make_egress(rows) -> nf.Egress:
    eg = nf.Egress()
    for p, h, q, d in rows:
        eg.set_port(p, has_qos=h, num_queues=q, max_queue_depth=d)
    return eg.commit()


def eq_model(port, queue, depth, has_qos, num_queues, max_depth):
    """enqueue_packet over the burst as a stable sort: classify, stable argsort by key, a packet's arrival index is
    its place among its key's packets, enqueued iff that is below max(0, max_depth - depth)."""
    port, queue = np.asarray(port, np.int64), np.asarray(queue, np.int64)
    n, nports = len(port), len(has_qos)
    keys = nports * Q
    known = port < nports
    pc = np.where(known, port, 0)
    result = np.full(n, nf.EQ_ENQUEUED, np.uint8)
    result[queue >= num_queues[pc]] = nf.EQ_BAD_QUEUE
    result[~known | ~has_qos[pc]] = nf.EQ_DROP_NO_CONFIG
    result[port == NONE] = nf.EQ_SKIP
    idx = np.flatnonzero(result == nf.EQ_ENQUEUED)
    key = port[idx] * Q + queue[idx]
    o = np.argsort(key, kind="stable")
    idx, key = idx[o], key[o]
    count = np.bincount(key, minlength=keys).astype(np.int64)
    first = np.cumsum(count) - count
    arrival = np.arange(len(key)) - first[key]
    depth = np.asarray(depth, np.int64)
    room = np.maximum(0, np.repeat(max_depth, Q) - depth)
    enq = arrival < room[key]
    result[idx[~enq]] = nf.EQ_DROP_FULL
    taken = np.minimum(count, room)
    key_start = np.concatenate([[0], np.cumsum(taken)])
    assert int(key_start[-1]) == int(enq.sum()) <= n
    return {"result": result, "order": idx[enq].astype(np.uint32), "key_start": key_start.astype(np.uint32),
            "depth": (depth + taken).astype(np.uint32), "key_dropped": (count - taken).astype(np.uint32)}


def eq_random(rows, n, seed):
    """(port, queue, depth): a skewed distribution over the table's keys, with IF_NONE, ports past the table and
    bad queues among the packets, 3% each; depths 0..2 before."""
    rng = np.random.default_rng(seed)
    has, nq, _ = eq_port_arrays(rows)
    vp = np.repeat(np.flatnonzero(has), nq[has])
    vq = np.concatenate([np.arange(q) for q in nq[has]])
    w = 1.0 / (1.0 + rng.permutation(len(vp))) ** 1.2
    pick = rng.choice(len(vp), n, p=w / w.sum())
    port, queue = vp[pick].astype(np.uint32), vq[pick].astype(np.uint8)
    u = rng.random(n)
    port[u < 0.03] = NONE
    port[(u >= 0.03) & (u < 0.06)] = len(has) + 1
    queue[(u >= 0.06) & (u < 0.09)] = 8 + rng.integers(0, 100, int(((u >= 0.06) & (u < 0.09)).sum()))
    return port, queue, rng.integers(0, 3, len(has) * Q).astype(np.uint32)


EQ_TABLES = ["one_key", "keys64", "keys65", "small12", "big8192"]
# (table, tiles, exact): every tile count meets `random` on the 12-port table and on 65 keys; one key and 64 keys at
# three sizes; the 8,192-key table at 17 tiles and at 129, whose 129 * 8192 histogram words pass the scratch's 2^18
EQ_RANDOM_CASES = ([(tb, t, False) for t in EQ_TILES for tb in ("small12", "keys65")] +
                   [(tb, t, True) for t in EQ_EXACT for tb in ("small12", "keys65")] +
                   [(tb, t, False) for t in (17, 129, 257) for tb in ("one_key", "keys64")] +
                   [("big8192", 17, False), ("big8192", 129, False)])


def eq_random_case(table, tiles, exact):
    rows = eq_table(table)
    return (rows,) + eq_random(rows, burst_n(tiles, exact), 16 * tiles + 2 * EQ_TABLES.index(table) + exact)


EQ_PATTERNS = ["late_key", "gap_key", "room_cut_group2", "room_cut_seg_last", "room_cut_tail"]
EQ_PATTERN_TILES = [129, 145, 257]
SPECIAL = (3, 2)  # port 3 of small12: 4 queues, depth 100000


def eq_pattern(tiles, pattern, seed=0):
    """(port, queue, depth, meta) on small12: a random background without the key SPECIAL, and SPECIAL's packets
    placed by the pattern.
    late_key: only in the tiles of the last segment that holds a tile.
    gap_key: in no tile of segments 3..9, in every other tile.
    room_cut_*: every third packet of the whole burst; the queue's room ends at meta["cut"], the key's next packet
    meta["next"] is the first one dropped. group2: the cut in tile t0 + 8, the first tile of the second 8-group, of
    the last full segment; seg_last: the last packet of the key in that segment's last tile; tail: in the burst's last
    tile, which lies in the last segment that holds one."""
    rows = eq_table("small12")
    n = burst_n(tiles)
    port, queue, depth = eq_random(rows, n, 1000 * tiles + seed)
    mine = (port == SPECIAL[0]) & (queue == SPECIAL[1])
    queue[mine] = 1
    i = np.arange(n)
    tile = i // T
    _, segs = eq_segments(tiles)
    key = SPECIAL[0] * Q + SPECIAL[1]
    meta = {"key": key}
    if pattern == "late_key":
        t0, t1 = eq_last_segment(tiles)
        put = (tile >= t0) & (i % 5 == 2)
    elif pattern == "gap_key":
        put = ((tile < segs[3][0]) | (tile >= segs[9][1])) & (i % 5 == 2)
        meta["gap"] = (segs[3][0], segs[9][1])
    else:
        put = i % 3 == 1
        t0, t1 = eq_last_full_segment(tiles)
        at = np.flatnonzero(put)
        if pattern == "room_cut_group2":
            in_tile = at[at // T == t0 + EG_GROUP]
            cut = int(in_tile[len(in_tile) // 2])
        elif pattern == "room_cut_seg_last":
            cut = int(at[at // T == t1 - 1][-1])
        else:
            in_tile = at[at // T == tiles - 1]
            cut = int(in_tile[len(in_tile) // 2])
        rank = int(np.searchsorted(at, cut))
        depth[key] = 100000 - (rank + 1)
        meta.update(cut=cut, next=int(at[rank + 1]), room=rank + 1)
    port[put], queue[put] = SPECIAL
    meta["put"] = put
    return port, queue, depth, meta


# ---- flood replication ---------------------------------------------------------------------------------------

FLOOD_PORTS, FLOOD_INGRESS = 8, 0
FLOOD_VLANS = [10, 20, 30, 40]
# (length, class, unicast port or VLAN, weight). Classes: "uni", "flood", "none".
FLOOD_TEMPLATES = [(60, "uni", 3, 12), (64, "uni", 7, 10), (14, "uni", 1, 8),
                   (60, "flood", 10, 3), (64, "flood", 10, 2), (33, "flood", 20, 2), (14, "flood", 20, 1),
                   (47, "flood", 30, 1), (60, "flood", 40, 1),
                   (60, "none", 0, 40), (17, "none", 0, 20)]
FLOOD_PLANT = {20: 3, 24: 0, 40: 5, 44: 1}  # offset in the last tile -> template: the cut cases' packets


def make_fdb() -> nf.Fdb:
    """Ingress 0 a trunk on 10, 20, 30; ports 1..5 access on 10; 6 a trunk on 10, 20; 7 a trunk on 20. VLAN 10
    floods to six ports, 20 to two, 30 to none (no other port has it), 40 to none (the ingress lacks it)."""
    fdb = nf.Fdb()
    fdb.set_port(0, type=nf.L2_TRUNK, allowed_vlans=[10, 20, 30])
    for p in range(1, 6):
        fdb.set_port(p, native_vlan=10)
    fdb.set_port(6, type=nf.L2_TRUNK, allowed_vlans=[10, 20])
    fdb.set_port(7, type=nf.L2_TRUNK, allowed_vlans=[20])
    return fdb.commit()


def flood_lists(fdb):
    """{vlan: its flood ports}: one Fdb.flood_ports_host call per VLAN."""
    return {v: fdb.flood_ports_host(FLOOD_INGRESS, v, FLOOD_PORTS) for v in FLOOD_VLANS}


def stamp(rows, at, index, width):
    """The packet index, little-endian, into bytes [at, at + width) of every row."""
    for b in range(width):
        rows[:, at + b] = (index >> (8 * b)) & 0xFF


@functools.lru_cache(maxsize=2)
def flood_burst(tiles, exact=False):
    """A burst of tiles * T (- 959) frames in 64-byte slots. Returns a dict: frames (n * 64 bytes, read-only), desc,
    tmpl (the template of each packet), uni_port / flood / vlan / lens per packet, arrays (the call's per-packet
    arguments), copy_base, and plant: the packet indexes of FLOOD_PLANT in the last tile."""
    n = burst_n(tiles, exact)
    rng = np.random.default_rng(tiles)
    w = np.array([t[3] for t in FLOOD_TEMPLATES], float)
    tmpl = rng.choice(len(FLOOD_TEMPLATES), n, p=w / w.sum())
    last = (tiles - 1) * T
    plant = {}
    for o, k in FLOOD_PLANT.items():
        tmpl[last + o] = k
        plant[o] = last + o
    body = rng.integers(0, 256, (len(FLOOD_TEMPLATES), SLOT), dtype=np.uint8)
    rows = body[tmpl]
    stamp(rows, 6, np.arange(n), 4)
    lens = np.array([t[0] for t in FLOOD_TEMPLATES], np.uint32)[tmpl]
    cls = np.array([t[1] for t in FLOOD_TEMPLATES])[tmpl]
    arg = np.array([t[2] for t in FLOOD_TEMPLATES], np.uint32)[tmpl]
    desc = np.zeros(n, nf.DESC_DTYPE)
    desc["off16"], desc["len"] = np.arange(n) * (SLOT // 16), lens
    uni, flood = cls == "uni", cls == "flood"
    uni_port = np.where(uni, arg, NONE).astype(np.uint32)
    verdict = np.where(flood, nf.L2_FLOOD, np.where(uni, nf.L2_FORWARD, nf.L2_DROP_VLAN)).astype(np.uint8)
    verdict[(cls == "none") & (lens == 17)] = nf.L2_SKIP
    vlan = np.where(flood, arg, 1).astype(np.uint16)
    frames = rows.reshape(-1)
    out = {"n": n, "tiles": tiles, "frames": frames, "desc": desc, "tmpl": tmpl, "uni_port": uni_port, "flood": flood,
           "vlan": vlan, "lens": lens, "copy_base": round_up(n * SLOT, 128), "plant": plant,
           "arrays": dict(l2_port=uni_port, l2_verdict=verdict, l2_vlan=vlan)}
    for a in (frames, desc, uni_port, verdict, vlan, lens, flood):
        a.setflags(write=False)
    return out


def flood_model(b, lists, copy_align, arena_bytes, cap):
    """The expand as cumulative sums. b: a flood_burst; lists: {vlan: flood ports}. Returns k0 and b0 per packet (the
    exclusive cumulative item count and slot bytes, 64-bit), item_desc / item_port /
    item_src (cap entries, inert past the emitted ones), totals, and item_flood (whether emitted item k is a copy)."""
    n, copy_base = b["n"], b["copy_base"]
    uni, flood = b["uni_port"] != NONE, b["flood"]
    width = max(len(p) for p in lists.values())
    table, cnt_of = np.zeros((4096, max(width, 1)), np.int64), np.zeros(4096, np.int64)
    for v, p in lists.items():
        table[v, :len(p)], cnt_of[v] = p, len(p)
    cnt = np.where(uni, 1, np.where(flood, cnt_of[b["vlan"]], 0)).astype(np.int64)
    slot = np.where(flood, round_up(b["lens"].astype(np.int64), copy_align), 0)
    k0 = np.cumsum(cnt) - cnt
    need = cnt * slot
    b0 = np.cumsum(need) - need
    total_bytes, needed = int(need.sum()), int(cnt.sum())  # 64-bit sums: at most 2^20 packets x 6 x 128 bytes
    src = np.repeat(np.arange(n), cnt)
    j = np.arange(needed) - k0[src]
    end = copy_base + b0[src] + (j + 1) * slot[src]  # the region's end once item k is in
    assert (np.diff(end) >= 0).all()
    emitted = min(int(cap), int(np.searchsorted(end, arena_bytes, side="right")))
    is_copy = flood[src]
    item_port = np.where(is_copy, table[b["vlan"][src], np.minimum(j, width - 1)], b["uni_port"][src])
    off16 = np.where(is_copy, (copy_base + b0[src] + j * slot[src]) // 16, b["desc"]["off16"][src])
    item_desc = np.zeros(cap, nf.DESC_DTYPE)
    item_desc["off16"][:emitted], item_desc["len"][:emitted] = off16[:emitted], b["lens"][src[:emitted]]
    out_port, out_src = np.full(cap, nf.IF_NONE, np.uint32), np.full(cap, nf.ITEM_NONE, np.uint32)
    out_port[:emitted], out_src[:emitted] = item_port[:emitted], src[:emitted]
    totals = np.zeros(1, nf.FLOOD_TOTALS_DTYPE)[0]
    totals["items"], totals["items_needed"], totals["copies"] = emitted, needed, int(is_copy[:emitted].sum())
    totals["flooded"], totals["copy_bytes_needed"] = int(flood.sum()), total_bytes
    totals["copy_bytes"] = int(slot[src[:emitted]].sum())
    return {"k0": k0, "b0": b0, "cnt": cnt, "slot": slot, "item_desc": item_desc, "item_port": out_port,
            "item_src": out_src, "totals": totals, "item_flood": is_copy[:emitted]}


def flood_arena_model(before, b, m):
    """The arena after the expand: every emitted copy holds its source's whole 16-byte chunks, nothing else changes."""
    after = before.copy()
    rows_in, rows_out = before[:len(before) // 16 * 16].reshape(-1, 16), after[:len(after) // 16 * 16].reshape(-1, 16)
    k = np.flatnonzero(m["item_flood"])
    dst, src = m["item_desc"]["off16"][k].astype(np.int64), b["desc"]["off16"][m["item_src"][k]].astype(np.int64)
    chunks = (m["item_desc"]["len"][k].astype(np.int64) + 15) // 16
    for c in range(SLOT // 16):
        sel = chunks > c
        rows_out[dst[sel] + c] = rows_in[src[sel] + c]
    return after


def flood_case(b, lists, copy_align, case):
    """(arena_bytes, cap, the packet the cut lies in or None) of "full", "cap_cut" and "region_cut": cap ends after
    three of the six items of the flooded packet planted at offset 20 of the last tile; the region ends 16 bytes short
    of that packet's third copy."""
    full = flood_model(b, lists, copy_align, 1 << 62, 0)  # k0, b0 and what is needed do not depend on cap
    need_items, need_bytes = int(full["totals"]["items_needed"]), int(full["totals"]["copy_bytes_needed"])
    p = b["plant"][20]
    if case == "full":
        return b["copy_base"] + need_bytes + 256, need_items + 3, None
    if case == "cap_cut":
        return b["copy_base"] + need_bytes, int(full["k0"][p]) + 3, p
    if case == "region_cut":
        return b["copy_base"] + int(full["b0"][p]) + 3 * int(full["slot"][p]) - 16, need_items, p
    raise KeyError(case)


# ---- the ICMP responder ----------------------------------------------------------------------------------------

ICMP_INGRESS = 1


def _echo(payload, type_=8):
    return ipv4(HOST, ME, 1, struct.pack(">BBHHH", type_, 0, 0, 0x1234, 1) + bytes(range(payload)))


# (frame, verdict, message length or 0, class, weight). The lengths are nfcs_icmp.h's rules worked by hand: a reply
# is as long as its request (42 + payload); an error is 42 + the original's IPv4 header + up to 8 bytes behind it.
ICMP_TEMPLATES = [(_echo(2), nf.RT_LOCAL, 44, "echo", 3), (_echo(10), nf.RT_LOCAL, 52, "echo", 4),
                  (_echo(22), nf.RT_LOCAL, 64, "echo", 3),
                  (ipv4(HOST, FAR, 17, bytes(26), ttl=1), nf.RT_TTL_EXPIRED, 70, "ttl", 6),
                  (ipv4(HOST, FAR, 17, bytes(4), ttl=1), nf.RT_TTL_EXPIRED, 66, "ttl", 4),
                  (ipv4(HOST, FAR, 6, bytes(30)), nf.RT_NO_ROUTE, 70, "noroute", 6),
                  (ipv4(HOST, FAR, 6, bytes(16), ihl=6), nf.RT_NO_ROUTE, 74, "noroute", 4),
                  (ipv4(HOST, FAR, 6, bytes(30)), nf.RT_FORWARD, 0, "none", 40),        # transit: ICMP_ST_NONE
                  (ipv4(HOST, ME, 6, bytes(30)), nf.RT_LOCAL, 0, "none", 10),            # TCP to the switch: TO_CPU
                  (_echo(10, type_=0), nf.RT_LOCAL, 0, "none", 10),                      # an echo reply: IGNORED
                  (ipv4(FAR, HOST, 17, bytes(26), ttl=1), nf.RT_TTL_EXPIRED, 0, "none", 10)]  # no route back
ICMP_PLANT = {20: 1, 30: 3, 40: 6, 50: 2}
assert all(len(t[0]) <= SLOT for t in ICMP_TEMPLATES)


@functools.lru_cache(maxsize=2)
def icmp_burst(tiles, exact=False):
    """As flood_burst: frames (n * 64 bytes), desc, tmpl, verdict, ip_id, msg_len and cls per packet, msg_base (128-byte
    aligned), plant."""
    n = burst_n(tiles, exact)
    rng = np.random.default_rng(7 * tiles + 1)
    w = np.array([t[4] for t in ICMP_TEMPLATES], float)
    tmpl = rng.choice(len(ICMP_TEMPLATES), n, p=w / w.sum())
    last = (tiles - 1) * T
    plant = {}
    for o, k in ICMP_PLANT.items():
        tmpl[last + o] = k
        plant[o] = last + o
    body = np.full((len(ICMP_TEMPLATES), SLOT), 0xEE, np.uint8)
    for k, t in enumerate(ICMP_TEMPLATES):
        body[k, :len(t[0])] = np.frombuffer(t[0], np.uint8)
    rows = body[tmpl]
    lens = np.array([len(t[0]) for t in ICMP_TEMPLATES], np.uint32)[tmpl]
    i = np.arange(n)
    stamp(rows, 18, i, 2)  # the IPv4 identification: an error message quotes it
    quoted = rows[:, 38:42].copy()
    stamp(rows, 38, i, 4)  # echo identifier and sequence number / L4 bytes 4..7: replies and errors quote them
    rows[lens < 42, 38:42] = quoted[lens < 42]
    desc = np.zeros(n, nf.DESC_DTYPE)
    desc["off16"], desc["len"] = i * (SLOT // 16), lens
    out = {"n": n, "tiles": tiles, "frames": rows.reshape(-1), "desc": desc, "tmpl": tmpl, "plant": plant,
           "verdict": np.array([t[1] for t in ICMP_TEMPLATES], np.uint8)[tmpl],
           "msg_len": np.array([t[2] for t in ICMP_TEMPLATES], np.uint32)[tmpl],
           "cls": np.array([t[3] for t in ICMP_TEMPLATES])[tmpl], "ip_id": ((i * 7 + 3) & 0xFFFF).astype(np.uint16),
           "msg_base": round_up(n * SLOT, 128)}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def icmp_model(b, msg_align, arena_bytes, cap):
    """The message list as cumulative sums over the per-packet message lengths: index and off (the exclusive
    cumulative message count and slot bytes per packet), overflow (the packets whose message is not emitted), msg_desc /
    msg_src (cap entries, inert past the emitted ones), totals."""
    ln = b["msg_len"].astype(np.int64)
    has = ln > 0
    slot = np.where(has, round_up(ln, msg_align), 0)
    index = np.cumsum(has) - has
    off = np.cumsum(slot) - slot
    who = np.flatnonzero(has)
    end = b["msg_base"] + off[who] + slot[who]
    emitted = min(int(cap), int(np.searchsorted(end, arena_bytes, side="right")))
    msg_desc = np.zeros(cap, nf.DESC_DTYPE)
    msg_desc["off16"][:emitted], msg_desc["len"][:emitted] = (b["msg_base"] + off[who[:emitted]]) // 16, ln[who[:emitted]]
    msg_src = np.full(cap, nf.ITEM_NONE, np.uint32)
    msg_src[:emitted] = who[:emitted]
    totals = np.zeros(1, nf.ICMP_TOTALS_DTYPE)[0]
    totals["messages"], totals["messages_needed"] = emitted, len(who)
    totals["echo_replies"] = int((b["cls"][who[:emitted]] == "echo").sum())
    totals["errors"] = emitted - int(totals["echo_replies"])
    totals["msg_bytes"], totals["msg_bytes_needed"] = int(slot[who[:emitted]].sum()), int(slot.sum())
    overflow = np.zeros(b["n"], bool)
    overflow[who[emitted:]] = True
    return {"index": index, "off": off, "slot": slot, "msg_desc": msg_desc, "msg_src": msg_src, "totals": totals,
            "overflow": overflow}


def icmp_case(b, msg_align, case):
    """(arena_bytes, cap, the first packet whose message is cut or None): cap ends before the message of the packet
    planted at offset 30 of the last tile; the region ends 16 bytes short of that message's slot."""
    full = icmp_model(b, msg_align, 1 << 62, 0)
    need, need_bytes = int(full["totals"]["messages_needed"]), int(full["totals"]["msg_bytes_needed"])
    p = b["plant"][30]
    if case == "full":
        return b["msg_base"] + need_bytes + 256, need + 3, None
    if case == "cap_cut":
        return b["msg_base"] + need_bytes, int(full["index"][p]), p
    if case == "region_cut":
        return b["msg_base"] + int(full["off"][p]) + int(full["slot"][p]) - 16, need, p
    raise KeyError(case)


def with_region(frames, base, arena_bytes, fill=0xEE):
    """The frames, the padding up to `base` and the region up to arena_bytes, filled."""
    arena = np.full(arena_bytes, fill, np.uint8)
    arena[:len(frames)] = frames
    return arena
