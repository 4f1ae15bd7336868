"""Generate tests/golden/acl_ref.npz from the REFERENCE implementation.

Compiles tests/golden/acl_probe.cpp against the reference's headers in place (plus its
src/netflow++/acl_manager.cpp) into oracle/_ref/acl_probe (git-ignored), feeds it a rule list and a
list of frames, and records what the reference decides per frame: the rule vector as get_all_rules()
returns it, and per frame AclManager::evaluate's action and redirect port and the index of the rule
that decided (the probe's header says how it finds that one with the reference's own check_match).

Three rule lists over the same frames:
  a  the rules added in insertion order, then compile_rules (priority descending, then rule id); no
     catch-all, so the default PERMIT occurs
  b  the same rules with other priorities, plus a final rule without match fields (REDIRECT with a
     port) that catches everything, compiled
  c  list a NOT compiled: get_all_rules() is the insertion order, and evaluate walks it as it is

The script checks, against the reference alone: under each list every rule decides at least one frame;
PERMIT by rule, PERMIT by default (a and c), DENY, REDIRECT and REDIRECT-without-port-as-DENY occur; no
action exceeds 60% of the frames under any list; the default PERMIT is 10-50% under list a.

    python tests/golden/make_acl_golden.py [reference root, default oracle.REFERENCE_ROOT]
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402

PROBE = os.path.join(ROOT, "oracle", "_ref", "acl_probe")
SEED = 20262
FRAME_CAP = 128  # no frame is longer (the decision reads no byte past 81)
PERMIT, DENY, REDIRECT = 0, 1, 2
NONE = 0xFFFFFFFF
F_SRC_MAC, F_DST_MAC, F_VLAN, F_ETYPE, F_SRC_IP, F_DST_IP, F_PROTO, F_SPORT, F_DPORT = (1 << k for k in range(9))

# the probe's record: include/nfcs.h nfcs_acl_rule (52 bytes; the probe ignores the masks), then the priority
RULE = np.dtype([("fields", "<u4"), ("rule_id", "<u4"), ("src_mac", "u1", (6,)), ("dst_mac", "u1", (6,)),
                 ("vlan_id", "<u2"), ("ethertype", "<u2"), ("src_ip", "<u4"), ("dst_ip", "<u4"),
                 ("src_ip_mask", "<u4"), ("dst_ip_mask", "<u4"), ("src_port", "<u2"), ("dst_port", "<u2"),
                 ("protocol", "u1"), ("action", "u1"), ("pad", "u1", (2,)), ("redirect_port", "<u4"),
                 ("priority", "<i4")])
assert RULE.itemsize == 56


def ip(a):
    """Dotted address -> the host-order u32 AclRule holds."""
    return int.from_bytes(bytes(int(x) for x in a.split(".")), "big")


def mac(k):
    return bytes([0x02, 0xAC, 0, 0, 0, k])


# small pools, so rules hit; the later entries of each pool appear in no rule
MACS = [mac(k) for k in range(14)]
IPS = [ip(a) for a in ("10.0.0.1", "10.0.0.2", "10.0.1.1", "10.0.1.2", "10.0.2.1", "10.0.2.2", "10.0.3.1",
                       "10.0.3.2", "10.0.4.1",
                       "0.53.0.80",  # with IHL 4 the ports are the destination address: 53 and 80
                       "172.16.0.1", "172.16.0.2", "172.16.0.3", "172.16.0.4", "172.16.0.5", "172.16.0.6",
                       "172.16.0.7", "172.16.0.8", "172.16.0.9", "172.16.0.10")]
PORTS = [22, 53, 80, 443, 8080, 1024, 1025, 1026, 1027, 1028, 1029, 1030]
VLANS = [10, 20, 30, 40, 50, 60]
IHLS = [5, 0, 4, 6, 15]

# (rule id, action, redirect port or None, {field: value})
RULES = [
    (1, DENY, None, dict(src_mac=MACS[0])),
    (2, PERMIT, None, dict(dst_mac=MACS[1])),
    (3, REDIRECT, 7, dict(vlan_id=10)),
    (4, DENY, None, dict(ethertype=0x86DD)),
    (5, DENY, None, dict(src_ip=IPS[0])),
    (6, PERMIT, None, dict(dst_ip=IPS[1])),
    (7, REDIRECT, 3, dict(protocol=1)),
    (8, DENY, None, dict(src_port=53)),                    # a port without a protocol: TCP or UDP
    (9, DENY, None, dict(dst_port=80)),
    (10, REDIRECT, 9, dict(protocol=6, dst_port=443)),     # a port with its protocol
    (11, PERMIT, None, dict(protocol=17, src_port=8080)),
    (12, REDIRECT, None, dict(src_ip=IPS[2], dst_ip=IPS[3])),  # REDIRECT without a port: DENY, ahead of 13
    (13, PERMIT, None, dict(src_ip=IPS[2])),               #   which matches the same frames and more
    (14, DENY, None, dict(src_mac=MACS[2], dst_mac=MACS[3])),
    (15, PERMIT, None, dict(vlan_id=20, ethertype=0x0800)),
    (16, PERMIT, None, dict(ethertype=0x0806)),
    (17, REDIRECT, 12, dict(dst_ip=IPS[4], protocol=17, dst_port=53)),
    (18, DENY, None, dict(src_mac=MACS[4], dst_mac=MACS[5], vlan_id=30, ethertype=0x0800, src_ip=IPS[5],
                          dst_ip=IPS[7], protocol=6, src_port=22, dst_port=8080)),  # every field
    (19, PERMIT, None, dict(ethertype=0x0800, protocol=6, src_port=443)),
    (20, REDIRECT, 5, dict(dst_mac=MACS[5], ethertype=0x86DD)),  # ahead of 4, which matches the same and more
    (21, REDIRECT, None, dict(dst_ip=IPS[6])),             # REDIRECT without a port
    (22, DENY, None, dict(vlan_id=30, dst_port=22)),
    (23, PERMIT, None, dict(src_ip=IPS[7], dst_port=443)),
    (24, DENY, None, dict(protocol=6, src_ip=IPS[8])),
]
# rule x must stand ahead of rule y in every list, or x could never decide / y's shadowing would not show
AHEAD = [(12, 13), (20, 4)]
CATCH_ALL = (99, REDIRECT, 15, dict())
FIELD_BITS = dict(src_mac=F_SRC_MAC, dst_mac=F_DST_MAC, vlan_id=F_VLAN, ethertype=F_ETYPE, src_ip=F_SRC_IP,
                  dst_ip=F_DST_IP, protocol=F_PROTO, src_port=F_SPORT, dst_port=F_DPORT)


def rule_record(spec, priority):
    rid, action, port, fields = spec
    r = np.zeros((), dtype=RULE)
    r["rule_id"], r["action"], r["priority"] = rid, action, priority
    r["redirect_port"] = NONE if port is None else port
    r["src_ip_mask"] = r["dst_ip_mask"] = 0xFFFFFFFF
    for k, v in fields.items():
        r["fields"] |= FIELD_BITS[k]
        r[k] = np.frombuffer(v, np.uint8) if isinstance(v, bytes) else v
    return r


def orders(rng):
    """Insertion order and the two priority assignments, each keeping AHEAD."""
    ids = [s[0] for s in RULES]
    while True:
        order = [ids[i] for i in rng.permutation(len(ids))]
        if all(order.index(x) < order.index(y) for x, y in AHEAD):
            break
    prios = []
    for _ in range(2):
        while True:  # priorities from a small range, so the rule-id tie-break of the sort takes part
            pr = {i: int(rng.integers(0, 8)) for i in ids}
            if all((-pr[x], x) < (-pr[y], y) for x, y in AHEAD):
                break
        prios.append(pr)
    return order, prios[0], prios[1]


def build_frame(rng, smac, dmac, vlan, etype, ihl=5, proto=6, sip=0, dip=0, sport=0, dport=0, length=None):
    """vlan None = untagged. length None = the whole frame."""
    b = bytearray(rng.integers(0, 256, size=FRAME_CAP, dtype=np.uint8).tobytes())
    b[0:6], b[6:12] = dmac, smac
    l2 = 14
    if vlan is not None:
        b[12:14] = b"\x81\x00"
        b[14:16] = ((int(rng.integers(0, 8)) << 13) | vlan).to_bytes(2, "big")
        l2 = 18
    b[l2 - 2:l2] = etype.to_bytes(2, "big")
    full = l2 + 46
    if etype == 0x0800:
        b[l2] = 0x40 | ihl
        b[l2 + 9] = proto
        b[l2 + 12:l2 + 16] = sip.to_bytes(4, "big")
        b[l2 + 16:l2 + 20] = dip.to_bytes(4, "big")
        l4 = l2 + 4 * ihl
        if ihl >= 5:  # below that the ports lie inside the header: they are whatever it holds
            b[l4:l4 + 2] = sport.to_bytes(2, "big")
            b[l4 + 2:l4 + 4] = dport.to_bytes(2, "big")
        full = max(l2 + 20, l4 + 20) + int(rng.integers(0, 12))
    return bytes(b[:min(full if length is None else length, FRAME_CAP)])


def bound_lengths(vlan, ihl):
    l2 = 14 if vlan is None else 18
    l4 = l2 + 4 * ihl
    return sorted({13, 14, 17, 18, l2 + 19, l2 + 20, l4 + 7, l4 + 8, l4 + 18, l4 + 19})


def pick(rng, pool, named, p_named):
    """A draw from the pool's first `named` entries (those the rules name) with probability p_named."""
    return pool[int(rng.integers(0, named))] if rng.random() < p_named else pool[int(rng.integers(named, len(pool)))]


def make_frames(rng):
    frames = []

    def rand_fields():
        return dict(smac=pick(rng, MACS, 6, 0.25), dmac=pick(rng, MACS, 6, 0.25),
                    vlan=(pick(rng, VLANS, 3, 0.5) if rng.random() < 0.4 else None),
                    ihl=int(rng.choice(IHLS, p=[0.6, 0.1, 0.1, 0.1, 0.1])), proto=int(rng.choice([6, 17, 1], p=[0.45, 0.45, 0.1])),
                    sip=pick(rng, IPS, 10, 0.35), dip=pick(rng, IPS, 10, 0.35),
                    sport=pick(rng, PORTS, 5, 0.3), dport=pick(rng, PORTS, 5, 0.3))

    # 1. per rule, frames made to match it: its own values, everything else drawn as below
    for rid, _, _, fields in RULES:
        for _ in range(10):
            f = rand_fields()
            f["etype"] = fields.get("ethertype", 0x0800)
            for k, v in fields.items():
                key = dict(src_mac="smac", dst_mac="dmac", vlan_id="vlan", ethertype="etype", src_ip="sip", dst_ip="dip",
                           protocol="proto", src_port="sport", dst_port="dport")[k]
                f[key] = v
            if "src_port" in fields or "dst_port" in fields:
                f["ihl"] = int(rng.choice([5, 6, 15]))
                if "protocol" not in fields:
                    f["proto"] = int(rng.choice([6, 17]))
            frames.append(build_frame(rng, **f))
    # 2. every bound: frames that match rules at several layers (source MAC 0, VLAN 10 when tagged, source
    #    address 0, ports 53 -> 80), cut at each length where an accessor starts to return something;
    #    then the same with neutral MACs / VLAN, then with a neutral source address as well, so the deeper
    #    rules decide
    for smac, vl, sip, protos in ((MACS[0], 10, IPS[0], (6, 17)), (MACS[9], 40, IPS[0], (6, 17)),
                                  (MACS[9], 40, IPS[10], (6, 17, 1))):
        for vlan in (None, vl):
            for ihl in IHLS:
                for proto in protos:
                    for ln in bound_lengths(vlan, ihl):
                        frames.append(build_frame(rng, smac, MACS[10], vlan, 0x0800, ihl, proto, sip,
                                                  IPS[9] if ihl == 4 else IPS[11], 53, 80, length=ln))
    # 3. IPv6 and ARP, tagged and untagged, whole and cut at the L2 bounds
    for etype in (0x86DD, 0x0806):
        for vlan in (None, 10, 20, 50):
            for ln in (None, 13, 14, 17, 18, 40):
                for dmac in (MACS[5], MACS[11]):
                    frames.append(build_frame(rng, MACS[8], dmac, vlan, etype, length=ln))
    # 4. random draws from the pools
    for _ in range(300):
        f = rand_fields()
        f["etype"] = int(rng.choice([0x0800, 0x86DD, 0x0806], p=[0.84, 0.08, 0.08]))
        ln = None
        if rng.random() < 0.15:
            ln = int(rng.choice(bound_lengths(f["vlan"], f["ihl"])))
        frames.append(build_frame(rng, length=ln, **f))
    return frames


def run_probe(records, compile_rules, frames):
    inp = [np.uint32(len(records)).tobytes(), records.tobytes(), np.uint32(1 if compile_rules else 0).tobytes(),
           np.uint32(len(frames)).tobytes()]
    for f in frames:
        inp.append(np.uint32(len(f)).tobytes() + f)
    res = subprocess.run([PROBE], input=b"".join(inp), stdout=subprocess.PIPE, check=True).stdout
    nt = int(np.frombuffer(res, "<u4", 1)[0])
    table = np.frombuffer(res, dtype=RULE, count=nt, offset=4).copy()
    rec = np.frombuffer(res, dtype=np.dtype([("action", "<u4"), ("rule", "<u4"), ("redirect", "<u4")]),
                        count=len(frames), offset=4 + RULE.itemsize * nt)
    assert 4 + RULE.itemsize * nt + 12 * len(frames) == len(res)
    return table, rec


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else oracle.REFERENCE_ROOT
    os.makedirs(os.path.dirname(PROBE), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ref_root, "include"),
                    os.path.join(HERE, "acl_probe.cpp"),
                    os.path.join(ref_root, "src", "netflow++", "acl_manager.cpp"), "-o", PROBE], check=True)
    rng = np.random.default_rng(SEED)
    order, prio_a, prio_b = orders(rng)
    by_id = {s[0]: s for s in RULES}
    frames = make_frames(rng)
    assert 1000 <= len(frames) <= 1500, len(frames)
    assert max(len(f) for f in frames) <= FRAME_CAP
    lens = np.array([len(f) for f in frames], dtype=np.uint32)
    data = np.zeros((len(frames), FRAME_CAP), dtype=np.uint8)
    for i, f in enumerate(frames):
        data[i, :len(f)] = np.frombuffer(f, dtype=np.uint8)
    out = {"seed": np.uint64(SEED), "lens": lens, "frames": data}
    lists = {
        "a": (np.array([rule_record(by_id[i], prio_a[i]) for i in order]), True),
        "b": (np.array([rule_record(by_id[i], prio_b[i]) for i in order] + [rule_record(CATCH_ALL, -1)]), True),
        "c": (np.array([rule_record(by_id[i], prio_a[i]) for i in order]), False),
    }
    for name, (records, compiled) in lists.items():
        table, rec = run_probe(records, compiled, frames)
        assert len(table) == len(records)
        table["src_ip_mask"] = table["dst_ip_mask"] = 0xFFFFFFFF  # the reference has no masks: exact match
        if not compiled:
            assert np.array_equal(table, records)  # insertion order, untouched
        else:
            keys = [(-int(r["priority"]), int(r["rule_id"])) for r in table]
            assert keys == sorted(keys) and list(table["rule_id"]) != list(records["rule_id"])
        action, rule = rec["action"], rec["rule"]
        matched = rule != NONE
        # every rule decides at least one frame
        hits = np.bincount(rule[matched], minlength=len(table))
        assert (hits > 0).all(), (name, [int(table["rule_id"][i]) for i in np.nonzero(hits == 0)[0]])
        ra = np.where(matched, table["action"][np.where(matched, rule, 0)], 255)
        rp = np.where(matched, table["redirect_port"][np.where(matched, rule, 0)], 0)
        kinds = {"permit by rule": int(((action == PERMIT) & matched).sum()),
                 "permit by default": int(((action == PERMIT) & ~matched).sum()),
                 "deny": int(((action == DENY) & (ra == DENY)).sum()),
                 "redirect": int((action == REDIRECT).sum()),
                 "redirect without a port as deny": int(((action == DENY) & (ra == REDIRECT) & (rp == NONE)).sum())}
        for k, v in kinds.items():
            assert v > 0 or (k == "permit by default" and name == "b"), (name, k)
        if name == "b":
            assert kinds["permit by default"] == 0
        shares = [float((action == a).mean()) for a in (PERMIT, DENY, REDIRECT)]
        assert max(shares) <= 0.60, (name, shares)
        if name == "a":
            assert 0.10 <= kinds["permit by default"] / len(frames) <= 0.50, kinds
        assert ((rec["redirect"] != NONE) == (action == REDIRECT)).all()
        out["rules_" + name] = np.frombuffer(table.tobytes(), np.uint8).reshape(len(table), RULE.itemsize)[:, :52].copy()
        out["priority_" + name] = table["priority"].copy()
        out["action_" + name] = action.astype(np.uint8)
        out["rule_" + name] = rule.copy()
        out["redirect_" + name] = rec["redirect"].copy()
        print(f"list {name}: {len(table)} rules, {len(frames)} frames, shares permit/deny/redirect "
              + "/".join(f"{s:.3f}" for s in shares) + "; " + ", ".join(f"{k} {v}" for k, v in kinds.items())
              + f"; fewest frames decided by one rule {int(hits.min())}")
    assert not np.array_equal(out["rule_a"], out["rule_c"])  # the order matters to the fixture
    lens_seen = set(int(x) for x in lens)
    assert {13, 14, 17, 18, 33, 34, 37, 38} <= lens_seen
    path = os.path.join(HERE, "acl_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
