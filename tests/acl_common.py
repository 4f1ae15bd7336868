"""Shared inputs for the ACL tests: the reference-made fixture tests/golden/acl_ref.npz
(tests/golden/make_acl_golden.py), an Acl built from its rule lists, the decision of Acl.eval_host over a
list of frames, and a numpy restatement of AclManager::check_match / evaluate (acl_manager.cpp:161-278)
that shares no code with the library."""
import os

import numpy as np

import netflow_amd as nf

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LISTS = ("a", "b", "c")  # a: compiled, no catch-all; b: other priorities + a catch-all; c: a, not compiled
IP_FIELDS = nf.ACL_F_SRC_IP | nf.ACL_F_DST_IP | nf.ACL_F_PROTOCOL | nf.ACL_F_SRC_PORT | nf.ACL_F_DST_PORT


def acl_fixture():
    z = np.load(os.path.join(GOLD, "acl_ref.npz"))
    frames = [bytes(z["frames"][i, :int(ln)]) for i, ln in enumerate(z["lens"])]
    return z, frames


def fixture_rules(z, name: str) -> np.ndarray:
    """The list as get_all_rules() returned it, as ACL_RULE_DTYPE records (full address masks)."""
    return np.ascontiguousarray(z["rules_" + name]).view(nf.ACL_RULE_DTYPE).reshape(-1).copy()


def make_acl(rules) -> nf.Acl:
    return nf.Acl().set_rules(rules).commit()


def rule(action=nf.ACL_DENY, redirect_port=nf.IF_NONE, rule_id=0, src_ip_mask=0xFFFFFFFF, dst_ip_mask=0xFFFFFFFF,
         **fields) -> np.ndarray:
    """One ACL_RULE_DTYPE record; the keyword names are the record's (src_mac=bytes, dst_port=80, ...)."""
    bits = dict(src_mac=nf.ACL_F_SRC_MAC, dst_mac=nf.ACL_F_DST_MAC, vlan_id=nf.ACL_F_VLAN_ID,
                ethertype=nf.ACL_F_ETHERTYPE, src_ip=nf.ACL_F_SRC_IP, dst_ip=nf.ACL_F_DST_IP,
                protocol=nf.ACL_F_PROTOCOL, src_port=nf.ACL_F_SRC_PORT, dst_port=nf.ACL_F_DST_PORT)
    r = np.zeros(1, dtype=nf.ACL_RULE_DTYPE)
    r["action"], r["redirect_port"], r["rule_id"] = action, redirect_port, rule_id
    r["src_ip_mask"], r["dst_ip_mask"] = src_ip_mask, dst_ip_mask
    for k, v in fields.items():
        r["fields"] |= bits[k]
        r[k] = np.frombuffer(v, np.uint8) if isinstance(v, (bytes, bytearray)) else v
    return r


def eval_host(acl: nf.Acl, frames):
    """action (u8), deciding rule (u32), redirect port (u32) per frame, on the CPU."""
    n = len(frames)
    a, r, p = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for i, f in enumerate(frames):
        a[i], r[i], p[i] = acl.eval_host(f)
    return a, r, p


def model_eval(rules: np.ndarray, frames):
    """The same three arrays from a numpy restatement of check_match (with the address masks) and of
    evaluate's first-match walk."""
    n = len(frames)
    F = np.zeros((n, 160), np.int64)
    L = np.array([len(f) for f in frames], np.int64)
    for i, f in enumerate(frames):
        F[i, :min(len(f), 160)] = np.frombuffer(f[:160], np.uint8)
    at = lambda o: F[np.arange(n), o]  # noqa: E731  the byte at a per-frame offset
    be16 = lambda o: (at(o) << 8) | at(o + 1)  # noqa: E731
    be32 = lambda o: (be16(o) << 16) | be16(o + 2)  # noqa: E731
    zero = np.zeros(n, np.int64)
    eth = L >= 14                                   # ethernet(), src_mac(), dst_mac()
    tagged = eth & (be16(zero + 12) == 0x8100)      # has_vlan()
    vid_ok = tagged & (L >= 18)                     # vlan_id() / vlan()
    vid = be16(zero + 14) & 0x0FFF
    et_known = eth & (~tagged | (L >= 18))
    et = np.where(tagged, be16(zero + 16), be16(zero + 12))
    l2 = np.where(tagged, 18, 14)
    ipv4 = et_known & (et == 0x0800) & (l2 + 20 <= L)   # ipv4(): no version test
    sip, dip, proto = be32(l2 + 12), be32(l2 + 16), at(l2 + 9)
    l4 = l2 + (at(l2) & 15) * 4                     # whatever IHL says, 0-4 included
    ports_ok = ipv4 & (((proto == 6) & (l4 + 19 <= L)) | ((proto == 17) & (l4 + 8 <= L)))  # tcp() / udp()
    sport, dport = be16(l4), be16(l4 + 2)
    first = np.full(n, nf.ACL_NO_MATCH, np.uint32)
    for k in range(len(rules) - 1, -1, -1):  # last to first, so the first in order is what remains
        r = rules[k]
        f = int(r["fields"])
        m = np.ones(n, bool)
        if f & nf.ACL_F_SRC_MAC:
            m &= eth & (F[:, 6:12] == r["src_mac"].astype(np.int64)).all(axis=1)
        if f & nf.ACL_F_DST_MAC:
            m &= eth & (F[:, 0:6] == r["dst_mac"].astype(np.int64)).all(axis=1)
        if f & nf.ACL_F_VLAN_ID:
            m &= vid_ok & (vid == int(r["vlan_id"]))
        if f & (nf.ACL_F_ETHERTYPE | IP_FIELDS):
            m &= et_known
        if f & nf.ACL_F_ETHERTYPE:
            m &= et == int(r["ethertype"])
        if f & IP_FIELDS:
            m &= ipv4
        if f & nf.ACL_F_SRC_IP:
            m &= (sip & int(r["src_ip_mask"])) == (int(r["src_ip"]) & int(r["src_ip_mask"]))
        if f & nf.ACL_F_DST_IP:
            m &= (dip & int(r["dst_ip_mask"])) == (int(r["dst_ip"]) & int(r["dst_ip_mask"]))
        if f & nf.ACL_F_PROTOCOL:
            m &= proto == int(r["protocol"])
        if f & (nf.ACL_F_SRC_PORT | nf.ACL_F_DST_PORT):
            m &= ports_ok
        if f & nf.ACL_F_SRC_PORT:
            m &= sport == int(r["src_port"])
        if f & nf.ACL_F_DST_PORT:
            m &= dport == int(r["dst_port"])
        first[m] = k
    return (*decision_of(rules, first), )


def decision_of(rules: np.ndarray, first: np.ndarray):
    """(action, rule, redirect) from the index of the first matching rule: no match permits, a REDIRECT
    rule without a port decides DENY."""
    hit = first != nf.ACL_NO_MATCH
    idx = np.where(hit, first, 0).astype(np.int64)
    if len(rules) == 0:
        return np.zeros(len(first), np.uint8), first.copy(), np.full(len(first), nf.IF_NONE, np.uint32)
    act = np.where(hit, rules["action"][idx], nf.ACL_PERMIT).astype(np.uint8)
    port = np.where(hit & (act == nf.ACL_REDIRECT), rules["redirect_port"][idx], nf.IF_NONE).astype(np.uint32)
    act[(act == nf.ACL_REDIRECT) & (port == nf.IF_NONE)] = nf.ACL_DENY
    return act, first.copy(), port
