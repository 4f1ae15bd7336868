"""Generate tests/golden/egress_acl_ref.npz from the REFERENCE implementation.

Compiles tests/golden/egress_acl_probe.cpp against the reference's headers in place (plus its acl_manager.cpp,
interface_manager.cpp, vlan_manager.cpp and qos_manager.cpp) into oracle/_ref/egress_acl_probe (git-ignored),
feeds it rule lists, port configs with their egress ACL bindings and a list of (frame, egress port) pairs in
processing order, and records what the reference's egress pipeline does with every pair (the probe's header
lists it) plus the ports' TX counters, the queue stats and the dequeue record.

Lists: 0 and 1 are lists a and b of tests/golden/acl_ref.npz (24 rules, and 25 with a catch-all REDIRECT);
2 and 5 are small lists of this file that name VLANs; 3 is bound and then deleted; 4 is empty.
Ports: 0 and 2 share list 0; 1 has list 1 and shallow queues (tail drops); 3 and 7 have lists 2 and 5;
4 is unbound; 5 is bound to the deleted list; 6 to the empty one. Every port but 3 pops its native VLAN.
Frames: those of acl_ref.npz (stored there, referred to by index) plus, stored here, frames tagged with the
ports' native VLANs: single-tagged, and double-tagged with an inner tag the rules name.
The dequeue record keeps the pair index, the length and the CRC-32 of the first 64 bytes of each frame.

The script checks, against the reference's output alone, the conditions listed in main().

    python tests/golden/make_egress_acl_golden.py [reference root, default oracle.REFERENCE_ROOT]
"""
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import oracle  # noqa: E402
from make_acl_golden import (DENY, IPS, MACS, NONE, PERMIT, REDIRECT, RULE, build_frame,  # noqa: E402
                             rule_record)

PROBE = os.path.join(ROOT, "oracle", "_ref", "egress_acl_probe")
SEED = 20265
ACCESS, TRUNK = 0, 1
NUM_PORTS = 9
Q = 8

PORT = np.dtype([("port_id", "<u4"), ("has_vlan_config", "u1"), ("type", "u1"), ("tag_native", "u1"), ("has_qos", "u1"),
                 ("native_vlan", "<u2"), ("num_queues", "u1"), ("pad", "u1"), ("max_queue_depth", "<u4"),
                 ("list", "<u4")])
assert PORT.itemsize == 20
# (port id, type, tag_native, native VLAN, queues, depth, bound list)
PORTS = [(0, ACCESS, 0, 40, 4, 100000, 0), (1, TRUNK, 0, 60, 8, 40, 1), (2, TRUNK, 0, 50, 2, 100000, 0),
         (3, TRUNK, 1, 40, 4, 100000, 2), (4, ACCESS, 0, 40, 4, 100000, NONE), (5, ACCESS, 0, 40, 2, 100000, 3),
         (6, TRUNK, 0, 50, 8, 100000, 4), (7, ACCESS, 0, 40, 4, 60, 5)]
LIST2 = [(1, DENY, None, dict(vlan_id=40)),             # port 3 keeps its native tag: this decides there
         (2, PERMIT, None, dict(protocol=17)),
         (3, REDIRECT, 2, dict(protocol=6, dst_port=443)),
         (4, DENY, None, dict(ethertype=0x0806)),
         (5, REDIRECT, None, dict(src_ip=IPS[0]))]      # REDIRECT without a port
LIST5 = [(1, DENY, None, dict(vlan_id=10)),             # the inner tag of a double-tagged frame, after the pop
         (2, REDIRECT, 6, dict(vlan_id=20)),
         (3, DENY, None, dict(ethertype=0x0800, protocol=6))]
LIST3 = [(1, DENY, None, dict()), (2, DENY, None, dict(protocol=6))]  # deleted: would deny everything


def port_records():
    rec = np.zeros(len(PORTS), PORT)
    for r, (pid, typ, tagn, native, nq, depth, lst) in zip(rec, PORTS):
        r["port_id"], r["has_vlan_config"], r["type"], r["tag_native"], r["has_qos"] = pid, 1, typ, tagn, 1
        r["native_vlan"], r["num_queues"], r["max_queue_depth"], r["list"] = native, nq, depth, lst
    return rec


def extra_frames(rng):
    """Frames tagged with the ports' native VLANs: single-tagged, and double-tagged with inner tag 10 / 20 / 30."""
    out = []
    for native in (40, 50, 60):
        for k in range(60):
            proto = int(rng.choice([6, 17, 1]))
            inner = build_frame(rng, MACS[int(rng.integers(0, 14))], MACS[int(rng.integers(0, 14))],
                                (None, 10, 20, 30)[k % 4], 0x0800, 5, proto, IPS[int(rng.integers(0, 20))],
                                IPS[int(rng.integers(0, 20))], int(rng.choice([22, 53, 80, 443, 1024])),
                                int(rng.choice([22, 53, 80, 443, 1025])))
            tci = (int(rng.integers(0, 8)) << 13) | native
            out.append(inner[:12] + b"\x81\x00" + tci.to_bytes(2, "big") + inner[12:])
    return out


def run_probe(lists, ports, pairs, frames):
    inp = [np.uint32(len(lists)).tobytes()]
    for lid, compiled, deleted, records in lists:
        inp.append(np.array([lid, compiled, deleted, len(records)], "<u4").tobytes() + records.tobytes())
    inp += [np.uint32(len(ports)).tobytes(), ports.tobytes(), np.uint32(NUM_PORTS).tobytes(),
            np.uint32(len(pairs)).tobytes()]
    for fi, port in pairs:
        inp.append(np.array([port, len(frames[fi])], "<u4").tobytes() + frames[fi])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.bin")
        subprocess.run([PROBE, path], input=b"".join(inp), stdout=subprocess.DEVNULL, check=True)
        res = open(path, "rb").read()
    pos = 0
    tables = []
    for _ in lists:
        nt = int(np.frombuffer(res, "<u4", 1, pos)[0])
        tables.append(np.frombuffer(res, RULE, nt, pos + 4).copy())
        pos += 4 + nt * RULE.itemsize
    per = np.frombuffer(res, "<u4", len(pairs) * 7, pos).reshape(len(pairs), 7).copy()
    pos += per.nbytes
    tx = np.frombuffer(res, "<u8", NUM_PORTS * 3, pos).reshape(NUM_PORTS, 3).copy()
    pos += tx.nbytes
    stats = np.frombuffer(res, "<u4", NUM_PORTS * Q * 3, pos).reshape(NUM_PORTS, Q, 3).copy()
    pos += stats.nbytes
    start, src, ln, crc = [0], [], [], []
    for _ in range(NUM_PORTS * Q):
        cnt = int(np.frombuffer(res, "<u4", 1, pos)[0])
        pos += 4
        for _ in range(cnt):
            s, l = np.frombuffer(res, "<u4", 2, pos)
            src.append(int(s))
            ln.append(int(l))
            crc.append(zlib.crc32(res[pos + 8:pos + 8 + min(int(l), 64)]))
            pos += 72
        start.append(len(src))
    assert pos == len(res)
    return tables, per, tx, stats, (np.array(start, np.uint32), np.array(src, np.uint32), np.array(ln, np.uint32),
                                    np.array(crc, np.uint32))


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else oracle.REFERENCE_ROOT
    os.makedirs(os.path.dirname(PROBE), exist_ok=True)
    src = os.path.join(ref_root, "src", "netflow++")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ref_root, "include"),
                    os.path.join(HERE, "egress_acl_probe.cpp")] +
                   [os.path.join(src, f) for f in ("acl_manager.cpp", "interface_manager.cpp", "vlan_manager.cpp",
                                                   "qos_manager.cpp")] + ["-pthread", "-o", PROBE], check=True)
    rng = np.random.default_rng(SEED)
    za = np.load(os.path.join(HERE, "acl_ref.npz"))
    base = [bytes(za["frames"][i, :int(ln)]) for i, ln in enumerate(za["lens"])]
    extra = extra_frames(rng)
    frames = base + extra

    def fixture_list(name):
        rec = np.zeros(len(za["rules_" + name]), RULE)
        raw = np.frombuffer(rec.tobytes(), np.uint8).reshape(len(rec), RULE.itemsize).copy()
        raw[:, :52] = za["rules_" + name]
        rec = np.frombuffer(raw.tobytes(), RULE).copy()
        rec["priority"] = za["priority_" + name]
        return rec

    own = lambda specs: np.array([rule_record(s, 0) for s in specs])  # noqa: E731  priority 0, never compiled
    lists = [(0, 1, 0, fixture_list("a")), (1, 1, 0, fixture_list("b")), (2, 0, 0, own(LIST2)), (3, 0, 1, own(LIST3)),
             (4, 0, 0, np.zeros(0, RULE)), (5, 0, 0, own(LIST5))]
    ports = port_records()
    # every fixture frame meets list 0 (on one of its two ports) and list 1; a third of them, and every extra
    # frame three times, go to a port drawn from all eight
    pairs = []
    for fi in range(len(base)):
        pairs.append((fi, int(rng.choice([0, 2]))))
        pairs.append((fi, 1))
        if fi % 3 == 0:
            pairs.append((fi, int(rng.integers(3, 8))))
    for fi in range(len(base), len(frames)):
        pairs += [(fi, int(p)) for p in rng.choice(8, size=3, replace=False)]
        pairs += [(fi, 7), (fi, 3)]
    # Packet::update_checksums, which pop_vlan ends with, sums IHL * 4 bytes of IPv4 header whatever the frame's
    # length: where the header so measured reaches past the popped frame's end the reference's bytes depend on
    # what lies behind the frame in its buffer. Such a pair goes to port 3 instead, which never pops.
    native_of = {pid: (native, typ == ACCESS or not tagn) for pid, typ, tagn, native, _, _, _ in PORTS}

    def pop_overhangs(f, pid):
        native, pops = native_of[pid]
        if not pops or len(f) < 18 or f[12:14] != b"\x81\x00" or (int.from_bytes(f[14:16], "big") & 0xFFF) != native:
            return False
        g = f[:12] + f[16:]
        l2 = 18 if g[12:14] == b"\x81\x00" else 14
        return len(g) >= l2 + 20 and (g[l2] >> 4) == 4 and l2 + 4 * (g[l2] & 15) > len(g)

    moved = sum(pop_overhangs(frames[fi], p) for fi, p in pairs)
    pairs = [(fi, 3 if pop_overhangs(frames[fi], p) else p) for fi, p in pairs]
    assert 0 < moved < 20, moved
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    assert 3000 <= len(pairs) <= 6000, len(pairs)
    tables, per, tx, stats, (dq_start, dq_src, dq_len, dq_crc) = run_probe(lists, ports, pairs, frames)
    for (lid, compiled, deleted, records), table in zip(lists, tables):
        sent = records.copy()
        sent["src_ip_mask"] = sent["dst_ip_mask"] = 0  # the probe does not hand the masks back
        assert np.array_equal(table, sent), lid  # lists 0 and 1 arrive in their compiled order and stay in it
    fidx = np.array([p[0] for p in pairs], np.uint32)
    port = np.array([p[1] for p in pairs], np.uint32)
    action, rule, redirect, len_out, action_raw, enq, queue = (per[:, k] for k in range(7))
    bound = {pid: lst for pid, *_, lst in PORTS}
    live = {0: 0, 1: 1, 2: 2, 5: 5}  # list id -> index into lists/tables of the lists that exist and hold rules
    table_of = {lid: tables[[l[0] for l in lists].index(lid)] for lid in live}
    lst = np.array([bound[int(p)] for p in port], np.int64)
    scanned = np.isin(lst, list(live))
    # every rule of every list decides at least one pair
    for lid, table in table_of.items():
        hits = np.bincount(rule[(lst == lid) & (rule != NONE)], minlength=len(table))
        assert (hits > 0).all(), (lid, np.nonzero(hits == 0)[0])
    deny_share = float((action[scanned] == DENY).mean())
    assert 0.15 <= deny_share <= 0.60, deny_share
    red = action == REDIRECT
    assert red.sum() >= 20 and (enq[red] == 1).all() and (redirect[red] != NONE).all()
    assert ((redirect != NONE) == red).all()
    no_port_deny = 0  # REDIRECT without a port, decided as DENY
    for lid, table in table_of.items():
        m = (lst == lid) & (rule != NONE)
        ra, rp = table["action"][rule[m]], table["redirect_port"][rule[m]]
        no_port_deny += int(((ra == REDIRECT) & (rp == NONE) & (action[m] == DENY)).sum())
    assert no_port_deny > 0
    for pid in (4, 5, 6):  # unbound, bound to the deleted list, bound to the empty list
        m = port == pid
        assert m.sum() >= 20 and (action[m] == PERMIT).all() and (rule[m] == NONE).all() and (enq[m] == 1).all(), pid
    assert ((action == DENY) == (enq == 0)).all()
    pop_matters = int((action_raw != action).sum())
    assert pop_matters >= 20, pop_matters
    lens_in = np.array([len(frames[i]) for i in fidx], np.uint32)
    popped = len_out != lens_in
    assert (lens_in[popped] - len_out[popped] == 4).all() and popped.sum() >= 100
    # the counters: a DENY raises tx_packets, tx_bytes and tx_drops alike, nothing else touches them
    for pid in range(NUM_PORTS):
        m = (port == pid) & (action == DENY)
        assert tx[pid, 0] == tx[pid, 2] == m.sum() and tx[pid, 1] == len_out[m].sum(), pid
    # a queue tail-drops, and there the enqueued set is not what it would be had the denied packets taken depth
    depth_of = {pid: depth for pid, _, _, _, _, depth, _ in PORTS}
    acl_before_enqueue = 0
    for pid in range(NUM_PORTS):
        for q in range(Q):
            if stats[pid, q, 0] == NONE or stats[pid, q, 1] == 0:
                continue
            k = pid * Q + q
            got = set(int(s) for s in dq_src[dq_start[k]:dq_start[k + 1]])
            everyone = np.flatnonzero((port == pid) & (queue == q))
            assert got == set(int(i) for i in everyone[action[everyone] != DENY][:depth_of[pid]])
            if got != set(int(i) for i in everyone[:depth_of[pid]]):
                acl_before_enqueue += 1
    assert acl_before_enqueue > 0
    assert len(dq_src) == int(stats[:, :, 0][stats[:, :, 0] != NONE].sum())
    assert bound[0] == bound[2]  # two ports share one list
    data = np.zeros((len(extra), max(len(f) for f in extra)), np.uint8)
    for i, f in enumerate(extra):
        data[i, :len(f)] = np.frombuffer(f, np.uint8)
    out = {"seed": np.uint64(SEED), "num_ports": np.uint32(NUM_PORTS), "n_base": np.uint32(len(base)),
           "extra_frames": data, "extra_lens": np.array([len(f) for f in extra], np.uint32),
           "ports": np.frombuffer(ports.tobytes(), np.uint8).reshape(len(ports), PORT.itemsize)[:, :16].copy(),
           "port_list": ports["list"].copy(), "deleted_list": np.uint32(3),
           "pair_frame": fidx, "pair_port": port, "action": action.astype(np.uint8), "rule": rule, "redirect": redirect,
           "len_out": len_out, "action_unpopped": action_raw.astype(np.uint8), "enqueued": enq.astype(np.uint8),
           "queue": queue.astype(np.uint8), "tx": tx, "stats": stats, "deq_start": dq_start, "deq_src": dq_src,
           "deq_len": dq_len, "deq_crc": dq_crc}
    for (lid, _, _, _), table in zip(lists, tables):
        t = table.copy()
        t["src_ip_mask"] = t["dst_ip_mask"] = 0xFFFFFFFF  # the reference has no masks: exact match
        out[f"rules_{lid}"] = np.frombuffer(t.tobytes(), np.uint8).reshape(len(t), RULE.itemsize)[:, :52].copy()
    path = os.path.join(HERE, "egress_acl_ref.npz")
    np.savez_compressed(path, **out)
    shares = "/".join(f"{float((action[scanned] == a).mean()):.3f}" for a in (PERMIT, DENY, REDIRECT))
    print(f"{len(pairs)} pairs, {int(scanned.sum())} meet a list, shares permit/deny/redirect {shares}; the pop changes "
          f"the action of {pop_matters}, {int(popped.sum())} popped; tail drops {int(stats[:, :, 1][stats[:, :, 0] != NONE].sum())}, "
          f"queues where the ACL's place shows {acl_before_enqueue}; redirect-without-port denies {no_port_deny}")
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
