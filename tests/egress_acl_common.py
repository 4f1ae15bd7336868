"""Shared inputs for the egress-ACL tests: the reference-made fixture tests/golden/egress_acl_ref.npz
(tests/golden/make_egress_acl_golden.py; its frames are those of acl_ref.npz plus its own extra ones), an
AclSet and an Egress built from it, the frames as process_egress leaves them, a per-list use of
acl_common.model_eval, and small helpers to build sets and bursts."""
import os
import zlib

import numpy as np

import netflow_amd as nf
from acl_common import acl_fixture, model_eval, rule
from egress_common import Q
from egress_common import set_ports as set_egress_ports

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = 0xFFFFFFFF
LIST_IDS = (0, 1, 2, 3, 4, 5)
FILL = 0xEE


class Fixture:
    """z: the npz; frames_in / frames: per pair, the frame before / after the reference's process_egress;
    port: per pair; rules: {list id: ACL_RULE_DTYPE records} as get_all_rules returned them."""

    def __init__(self):
        self.z = z = np.load(os.path.join(GOLD, "egress_acl_ref.npz"))
        _, base = acl_fixture()
        assert len(base) == int(z["n_base"])
        pool = base + [bytes(z["extra_frames"][i, :int(ln)]) for i, ln in enumerate(z["extra_lens"])]
        self.port = z["pair_port"].astype(np.uint32)
        self.frames_in = [pool[int(i)] for i in z["pair_frame"]]
        # the pop of VlanManager::process_egress is Packet::pop_vlan: bytes 12..15 leave the frame
        self.frames = [f[:12] + f[16:] if int(ln) != len(f) else f for f, ln in zip(self.frames_in, z["len_out"])]
        assert all(len(f) == int(ln) for f, ln in zip(self.frames, z["len_out"]))
        self.rules = {lid: np.ascontiguousarray(z[f"rules_{lid}"]).view(nf.ACL_RULE_DTYPE).reshape(-1).copy()
                      for lid in LIST_IDS}
        self.deleted = int(z["deleted_list"])
        self.egress_ports = np.ascontiguousarray(z["ports"]).view(nf.EGRESS_PORT_DTYPE).reshape(-1)
        self.bound = {int(p["port_id"]): int(l) for p, l in zip(self.egress_ports, z["port_list"])}
        self.num_ports = int(z["num_ports"])

    def aclset(self) -> nf.AclSet:
        """Built the way the reference's state came about: every list set, the ports bound, one list removed."""
        s = nf.AclSet()
        for lid, r in self.rules.items():
            s.set_list(lid, r)
        for port, lid in self.bound.items():
            if lid != NONE:
                s.bind_port(port, lid)
        s.remove_list(self.deleted)
        return s.commit()

    def egress(self) -> nf.Egress:
        return set_egress_ports(nf.Egress(), self.egress_ports).commit()

    def list_of(self, port: int):
        """The rules the port's packets meet: none for an unbound port, the removed list or the empty one."""
        lid = self.bound.get(int(port), NONE)
        if lid == NONE or lid == self.deleted:
            return None
        return self.rules[lid] if len(self.rules[lid]) else None

    def denied_counters(self):
        """(tx_drops, tx_bytes) per port id below `ports` of the set, from the reference's get_port_stats."""
        return self.z["tx"][:, 2].astype(np.uint32), self.z["tx"][:, 1].astype(np.uint64)

    def reference_queues(self):
        """{key: [(pair index, length, crc32 of the first 64 bytes)]} in dequeue order, {key: tail drops}."""
        z, queues, drops = self.z, {}, {}
        for p in range(self.num_ports):
            for q in range(Q):
                k = p * Q + q
                if z["stats"][p, q, 0] != NONE:
                    drops[k] = int(z["stats"][p, q, 1])
                lo, hi = int(z["deq_start"][k]), int(z["deq_start"][k + 1])
                if hi > lo:
                    queues[k] = [(int(z["deq_src"][j]), int(z["deq_len"][j]), int(z["deq_crc"][j])) for j in range(lo, hi)]
        return queues, drops


def crc64(b: bytes) -> int:
    return zlib.crc32(bytes(b[:64]))


def model_per_list(port, frames, list_of):
    """action, rule, redirect per packet from acl_common.model_eval applied per port's list (list_of(port) ->
    records or None)."""
    n = len(frames)
    action, first, redirect = np.zeros(n, np.uint8), np.full(n, NONE, np.uint32), np.full(n, NONE, np.uint32)
    port = np.asarray(port)
    for p in np.unique(port):
        rules = None if p == NONE else list_of(int(p))
        if rules is None or len(rules) == 0:
            continue
        idx = np.flatnonzero(port == p)
        a, r, d = model_eval(rules, [frames[i] for i in idx])
        action[idx], first[idx], redirect[idx] = a, r, d
    return action, first, redirect


def pack(frames, align=16, fill=FILL, tail=0):
    """Frames packed at `align`-byte starts: (arena, desc). Padding (and `tail` more bytes) hold `fill`."""
    desc = np.zeros(len(frames), nf.DESC_DTYPE)
    pos = 0
    for i, f in enumerate(frames):
        desc[i] = (pos // 16, len(f))
        pos += (max(len(f), 1) + align - 1) // align * align
    arena = np.full(pos + tail, fill, np.uint8)
    for d, f in zip(desc, frames):
        o = int(d["off16"]) * 16
        arena[o:o + len(f)] = np.frombuffer(bytes(f), np.uint8)
    return arena, desc


def udp_frame(tag: int, ihl: int = 5, sport: int = 1000, dport: int = 2000, length=None) -> bytes:
    """An untagged IPv4 / UDP frame whose source address is 10.9.(tag >> 8).(tag & 255): `tag` is what the
    rules of marked_lists() tell frames apart by. With ihl above 8 the ports lie past byte 47."""
    l4 = 14 + 4 * ihl
    b = bytearray(max(l4 + 8, 60))
    b[0:6], b[6:12] = b"\x02\x00\x00\x00\x00\x01", b"\x02\x00\x00\x00\x00\x02"
    b[12:14] = b"\x08\x00"
    b[14], b[23] = 0x40 | ihl, 17
    b[26:30] = bytes([10, 9, (tag >> 8) & 255, tag & 255])
    b[30:34] = bytes([10, 8, 0, 1])
    b[l4:l4 + 2], b[l4 + 2:l4 + 4] = sport.to_bytes(2, "big"), dport.to_bytes(2, "big")
    return bytes(b if length is None else b[:length])


def src_of(tag: int) -> int:
    return (10 << 24) | (9 << 16) | tag


def marked_lists(lengths, by_port=False):
    """One list per entry of `lengths`. List k matches frame udp_frame(k) only at its LAST rule (action by k:
    DENY, REDIRECT to port 100 + k, PERMIT in turn). The first rule of list k + 1, which is laid out behind
    list k, matches udp_frame(k) too, with another action (a list of one rule has no room for it), and every
    other rule matches none of these frames: a scan of list k that runs past its range, or one that starts in
    the wrong place, gives a wrong index or action. With by_port the deciding rules name UDP destination port
    7000 + k as well (udp_frame(k, dport=7000 + k))."""
    out = []
    n = len(lengths)
    for k, ln in enumerate(lengths):
        rules = []
        prev = (k - 1) % n
        own_action = (nf.ACL_DENY, nf.ACL_REDIRECT, nf.ACL_PERMIT)[k % 3]
        trap_action = (nf.ACL_DENY, nf.ACL_REDIRECT, nf.ACL_PERMIT)[(prev + 1) % 3]  # not list prev's own action
        extra = dict(dst_port=7000 + k) if by_port else {}
        if ln > 1 and n > 1:
            rules.append(rule(action=trap_action, redirect_port=900 if trap_action == nf.ACL_REDIRECT else nf.IF_NONE,
                              src_ip=src_of(prev)))
        while len(rules) < ln - 1:
            rules.append(rule(action=nf.ACL_DENY, src_ip=0x7F000001, dst_port=len(rules)))  # matches nothing here
        rules.append(rule(action=own_action, redirect_port=100 + k if own_action == nf.ACL_REDIRECT else nf.IF_NONE,
                          src_ip=src_of(k), **extra))
        out.append(np.concatenate(rules))
    return out


def want_marked(k: int, ln: int):
    """(action, rule, redirect) of frame udp_frame(k) under list k of marked_lists."""
    a = (nf.ACL_DENY, nf.ACL_REDIRECT, nf.ACL_PERMIT)[k % 3]
    return a, ln - 1, (100 + k if a == nf.ACL_REDIRECT else NONE)


def host_decision(s: nf.AclSet, port, frames):
    """action, rule, redirect per packet from AclSet.eval_host; IF_NONE ports read ACL_NO_PORT."""
    n = len(frames)
    a, r, p = np.zeros(n, np.uint8), np.full(n, NONE, np.uint32), np.full(n, NONE, np.uint32)
    for i, (pt, f) in enumerate(zip(port, frames)):
        if int(pt) == NONE:
            a[i] = nf.ACL_NO_PORT
        else:
            a[i], r[i], p[i] = s.eval_host(int(pt), f)
    return a, r, p
