"""Shared by tests/test_counter_limits.py and tests/test_gpu_counter_limits.py: the egress ACL's deny
counters where egress_acl_kernel's LDS table and counter_fold_kernel stop doing the trivial thing. The table has 256
entries, hashed by (port * 0x9E3779B1) >> 24 with linear probing; ports 0..63, all the older counting tests use, fall
into 64 different entries, so no probe ever stepped on. The cases here are built from the hash: the first colliding
pair, the fullest bucket, probes that wrap past entry 255, tables with all 256 entries taken, sets of 128, 129, 1,023
and 1,024 ports (a fold of one workgroup exactly, of two, of eight, and the counter scratch's last slot).

The constants below are the kernel's as this file read them; test_counter_limits.py parses them out of the sources
again and recomputes every claim a case makes, so a changed hash fails there and says so.

The model is numpy only and never calls the library: the action of every packet from how the case built it, the
packets per port as a bincount of the denied ones, the bytes per port by integer accumulation in 64 bits."""
import numpy as np

import netflow_amd as nf
from acl_common import rule
from egress_acl_common import FILL, NONE, udp_frame

HASH_MUL, HASH_SHIFT = 0x9E3779B1, 24  # nfcs_kernels.hip, egress_acl_kernel
TABLE = 256                            # kBlock entries, and packets per workgroup
STRIPES, LINE_SLOTS = 16, 16           # nfcs_internal.h kCtAclStripes, kCtLineSlots
MAX_PORTS = 1024                       # nfcs.h NFCS_L2_MAX_PORTS
SETS = (128, 129, 1023, 1024)          # ports bound: 256 slots, 258, a stride rounded up from 2,046, the full scratch
SLOT = 320                             # arena bytes per frame: frames of 60 to 315 bytes
PK1023 = 0xFFFFFF00                    # where port 1023's packet counter starts in the fold cases


def bucket(port, mul=HASH_MUL, shift=HASH_SHIFT):
    return ((int(port) * mul) & 0xFFFFFFFF) >> shift


def table_sim(ports, mul=HASH_MUL, shift=HASH_SHIFT, size=TABLE):
    """The table after the distinct `ports` were entered one after the other: (entry -> port, probes that found
    another port's entry and stepped on, probes that stepped from the last entry to entry 0). Which entries end up
    taken does not depend on the order with linear probing; the counts can."""
    table, stepped, wrapped = {}, 0, 0
    for p in dict.fromkeys(int(x) for x in ports):
        h = bucket(p, mul, shift)
        while h in table:
            stepped += 1
            wrapped += h == size - 1
            h = (h + 1) % size
        table[h] = p
    return table, stepped, wrapped


def buckets_of(ports=range(MAX_PORTS)):
    out = {}
    for p in ports:
        out.setdefault(bucket(p), []).append(p)
    return out


def first_colliding_pair():
    """The pair (a, b), a < b, with the smallest b that share a bucket."""
    seen = {}
    for p in range(MAX_PORTS):
        h = bucket(p)
        if h in seen:
            return seen[h], p
        seen[h] = p
    raise AssertionError("no two ports collide")


def fullest_bucket():
    b = buckets_of()
    h = max(b, key=lambda k: (len(b[k]), -k))
    return h, b[h]


def wrapping_ports(lo=250):
    return [p for p in range(MAX_PORTS) if bucket(p) >= lo]


def acl_stride(ports):
    return (2 * ports + LINE_SLOTS - 1) // LINE_SLOTS * LINE_SLOTS


# ---- the cases ----------------------------------------------------------------------------------------------------

def make(P, port, tag=None, bad=None, byp=None, start=False, spread=90):
    """One case on the set of P ports. port: per packet; tag: 0 = the denied source, anything else is permitted;
    bad: packets whose descriptor lies past the arena; byp: packets whose source frame is marked in the `items`
    entry's bypass array (ignored by the `plain` entry); start: the counters start non-zero. spread 90: the frame lengths are
    60 + (i + i // 24) % 90; spread 256: 60 + i % 256, which gives every packet of a workgroup its own length (the
    full-table cases, where a port has one packet per workgroup and only the bytes can tell two ports apart)."""
    port = np.asarray(port, np.int64).astype(np.uint32)
    n = len(port)
    z = lambda a: np.zeros(n, bool) if a is None else np.asarray(a, bool)
    c = dict(P=P, n=n, port=port, tag=np.zeros(n, np.uint8) if tag is None else np.asarray(tag, np.uint8), bad=z(bad), byp=z(byp),
             length=(60 + (np.arange(n) + (np.arange(n) // 24 if spread == 90 else 0)) % spread).astype(np.uint32))
    rng = np.random.default_rng(P + n)
    c["pk0"], c["by0"] = np.zeros(P, np.uint32), np.zeros(P, np.uint64)
    if start:
        c["pk0"] = rng.integers(1, 1 << 20, P).astype(np.uint32)
        c["by0"] = rng.integers(1, 1 << 40, P).astype(np.uint64)
        c["pk0"][P - 1] = PK1023
    return c


def build_cases():
    i256 = np.arange(256)
    a, b = first_colliding_pair()
    _, six = fullest_bucket()
    wrap = wrapping_ports()
    cases = {}
    for P in (1023, 1024):
        if b < P:
            cases[f"pair in one wave-{P}"] = make(P, np.where(np.arange(64) % 2 == 0, a, b), tag=np.arange(64) % 16 == 1)  # 32 and 28 packets
            for name, (x, y) in (("pair in two waves", (a, b)), ("pair in two waves, the later port first", (b, a))):
                # every eighth packet of the second wave is permitted: 64 and 56 packets, so a swap shows in both counters
                cases[f"{name}-{P}"] = make(P, np.where(i256 < 64, x, np.where(i256 < 128, y, i256 % 64)),
                                            tag=(i256 >= 128) | ((i256 >= 64) & (i256 % 8 == 0)), byp=(i256 >= 128) & (i256 % 3 == 0))
    P = 1024
    # waves 0 and 1 hold two of the six, waves 2 and 3 one each; 42, 22, 48, 16, 64, 56 packets
    w = i256 // 64
    second = ((w == 0) & (i256 % 3 == 0)) | ((w == 1) & (i256 % 4 == 0))
    cases["fullest bucket, spread over the waves"] = make(P, np.array(six)[np.where(second, (w + 4) % len(six), w)],
                                                          tag=(w == 3) & (i256 % 8 == 0))
    # all six in every wave, port k of the six in k + 1 of 21 lanes
    deal = np.repeat(np.arange(6), np.arange(1, 7))
    cases["fullest bucket, all in every wave"] = make(P, np.array(six)[deal[i256 % len(deal)]])
    for n in (256, 513):
        cases[f"wrapping probes-{n}"] = make(P, np.array(wrap)[np.arange(n) % len(wrap)])
    for n in (256, 257, 1025):
        i = np.arange(n)
        for Q in (1023, 1024):
            cases[f"full table low-{n}-{Q}"] = make(Q, i % 256, spread=256)
        cases[f"full table high-{n}"] = make(P, 768 + i % 256, spread=256)
    # a workgroup of 256 distinct denied ports between two that mix every kind of lane in every wave
    i = np.arange(768)
    kind = np.where((i >= 256) & (i < 512), 0, 1 + i % 8)
    port = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5, kind == 6, kind == 7, kind == 8],
                     [300 + i % 256, a, b, 900 + i % 100, NONE, MAX_PORTS, 70000, six[0], six[-1]])
    cases["full table with the rest"] = make(P, port, tag=kind == 3, bad=kind == 7, byp=kind == 8, spread=256)
    port1023 = np.where(port == MAX_PORTS, 1023, np.where(port == 1023, 1022, port))  # 1023 is the port without a list there
    cases["full table with the rest-1023"] = make(1023, port1023, tag=kind == 3, bad=kind == 7, byp=kind == 8, spread=256)
    # the fold: every stripe used twice, one lane in a 33rd workgroup
    n = TABLE * STRIPES * 2 + 1
    i = np.arange(n)
    rng = np.random.default_rng(27)
    named = np.array([0, 127, 128, 511, 1022, 1023])
    others = rng.permutation(np.setdiff1d(np.arange(1024), named))[:200]
    cases["fold-1024"] = make(1024, np.where(i % 2 == 0, named[(i // 2) % 6], others[(i // 2) % 200]), tag=i % 11 == 0,
                              byp=i % 13 == 0, start=True)
    cases["fold-129"] = make(129, np.where(i % 2 == 0, 127 + (i // 2) % 2, (i // 2) % 127), tag=i % 11 == 0, byp=i % 13 == 0, start=True)
    for Q in SETS:  # every port of every set: slots 2 Q - 2 and 2 Q - 1 are the last the fold reads
        i = np.arange(TABLE * STRIPES + 1)
        cases[f"every port-{Q}"] = make(Q, (i * 7) % Q, tag=i % 5 == 0, byp=i % 9 == 0, start=Q in (129, 1023))
    return cases


CASES = build_cases()
ENTRIES = ("plain", "items")


def deny_set(P):
    """Ports 0..P-1 bound to one list that denies source 10.9.0.0 (udp_frame(0)) and permits the rest; committed."""
    s = nf.AclSet()
    s.set_list(0, rule(action=nf.ACL_DENY, src_ip=(10 << 24) | (9 << 16)))
    for p in range(P):
        s.bind_port(p, 0)
    return s.commit()


def inputs(c, entry):
    """arena, desc, port, item_src, bypass of a case: SLOT bytes per frame, the frame udp_frame(tag) continued with
    zeros to its length (udp_frame's own `length` only cuts), FILL behind it."""
    n = c["n"]
    body = np.zeros((2, SLOT), np.uint8)
    for t in (0, 1):
        body[t, :60] = np.frombuffer(udp_frame(t), np.uint8)
    rows = body[(c["tag"] != 0).astype(np.intp)]
    arena = np.where(np.arange(SLOT)[None, :] < c["length"][:, None], rows, FILL).astype(np.uint8).reshape(-1)
    desc = np.zeros(n, nf.DESC_DTYPE)
    desc["off16"], desc["len"] = np.arange(n) * (SLOT // 16), c["length"]
    desc["off16"][c["bad"]] = arena.nbytes // 16  # starts where the arena ends
    item_src = bypass = None
    if entry == "items":  # item k comes from frame k, every 17th from no frame; two frames more than items
        item_src = np.where(np.arange(n) % 17 == 16, nf.ITEM_NONE, np.arange(n)).astype(np.uint32)
        bypass = np.concatenate([c["byp"], [True, True]]).astype(np.uint8)
    return arena, desc, c["port"].copy(), item_src, bypass


def model(c, entry):
    """dict of action, port (after the call), denied (the mask), pk, by: from the case alone."""
    n, P, port = c["n"], c["P"], c["port"]
    has_port = port != NONE
    byp = np.zeros(n, bool)
    if entry == "items":
        byp = c["byp"] & (np.arange(n) % 17 != 16) & has_port
    live = has_port & ~byp & ~c["bad"]
    denied = live & (port < P) & (c["tag"] == 0)
    action = np.where(~has_port, nf.ACL_NO_PORT, np.where(byp, nf.ACL_BYPASS, np.where(~live, nf.ACL_BAD_DESC,
                      np.where(denied, nf.ACL_DENY, nf.ACL_PERMIT)))).astype(np.uint8)
    pk = (c["pk0"].astype(np.uint64) + np.bincount(port[denied], minlength=P).astype(np.uint64)).astype(np.uint32)  # wraps
    by = c["by0"].copy()
    np.add.at(by, port[denied], c["length"][denied].astype(np.uint64))
    return dict(action=action, port=np.where(denied | (action == nf.ACL_BAD_DESC), NONE, port).astype(np.uint32), denied=denied, pk=pk, by=by)


def host(s, c, entry):
    """The library's sequential walk over the same inputs: dict of action, port, pk, by."""
    arena, desc, port, item_src, bypass = inputs(c, entry)
    pk, by = c["pk0"].copy(), c["by0"].copy()
    if entry == "plain":
        out = s.egress_acl_host(arena, desc, port, pk, by)
    else:
        out = s.egress_acl_items_host(arena, desc, port, item_src, bypass, pk, by)
    return dict(action=out["action"], port=out["port"], pk=pk, by=by)


def workgroup_tables(c, entry):
    """Per workgroup of 256 consecutive packets: table_sim of its denied ports in packet order."""
    denied = model(c, entry)["denied"]
    return [table_sim(c["port"][lo:lo + TABLE][denied[lo:lo + TABLE]]) for lo in range(0, c["n"], TABLE)]


def workgroup_sums(c, entry):
    """Per workgroup: {port: (packets, bytes)} of its denied packets, what the workgroup's table holds before it is added
    to the stripe."""
    denied = model(c, entry)["denied"]
    out = []
    for lo in range(0, c["n"], TABLE):
        d = denied[lo:lo + TABLE]
        ports, lens = c["port"][lo:lo + TABLE][d], c["length"][lo:lo + TABLE][d]
        out.append({int(p): (int((ports == p).sum()), int(lens[ports == p].sum())) for p in np.unique(ports)})
    return out
