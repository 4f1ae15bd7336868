"""Shared inputs for the flood-replication tests: the reference-made fixture tests/golden/flood_ref.npz
(tests/golden/make_flood_golden.py), an Fdb and an Egress built from its ports, the reference's dequeue
record in the form the egress stage reports it, a dict/loop restatement of the expand that shares no code
with the library, and the numpy model of what the expand writes into the arena."""
import os

import numpy as np

import netflow_amd as nf
from egress_common import Q
from egress_common import set_ports as set_egress_ports
from l2_common import set_ports as set_l2_ports

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = 0xFFFFFFFF
FILL = 0xEE


def flood_fixture():
    z = np.load(os.path.join(GOLD, "flood_ref.npz"))
    frames = [bytes(z["frames"][i, :int(ln)]) for i, ln in enumerate(z["lens"])]
    return z, frames


def fixture_l2_ports(z):
    ports = np.ascontiguousarray(z["ports"]).view(nf.L2_PORT_DTYPE).reshape(-1)
    return [(p, [int(v) for v in z["allowed"][i, :int(z["allowed_n"][i])]]) for i, p in enumerate(ports)]


def fixture_fdb(z) -> nf.Fdb:
    entries = np.ascontiguousarray(z["entries"]).view(nf.FDB_ENTRY_DTYPE).reshape(-1)
    return set_l2_ports(nf.Fdb().set_entries(entries), fixture_l2_ports(z)).commit()


def fixture_egress(z) -> nf.Egress:
    return set_egress_ports(nf.Egress(), np.ascontiguousarray(z["egress_ports"]).view(nf.EGRESS_PORT_DTYPE).reshape(-1)).commit()


def round_up(x, a):
    return (int(x) + a - 1) // a * a


def reference_queues(z, r):
    """{key: [(source index, port, length, bytes)]} in dequeue order, and {key: tail drops}, of run r."""
    queues, drops = {}, {}
    num_ports = int(z["num_ports"])
    for p in range(num_ports):
        for q in range(Q):
            k = p * Q + q
            lo, hi = int(z[f"deq_start_{r}"][k]), int(z[f"deq_start_{r}"][k + 1])
            if z[f"stats_{r}"][p, q, 0] != NONE:
                drops[k] = int(z[f"stats_{r}"][p, q, 1])
            if hi > lo:
                queues[k] = [(int(z[f"deq_src_{r}"][j]), int(z[f"deq_port_{r}"][j]), int(z[f"deq_len_{r}"][j]),
                              bytes(z[f"deq_data_{r}"][j, :min(int(z[f"deq_len_{r}"][j]), 64)])) for j in range(lo, hi)]
    return queues, drops


# ---- the restatement ------------------------------------------------------------------------------

def model_flood_ports(ports, ingress, vlan, num_ports):
    """flood_packet's port loop from the configs: ports = [(L2_PORT_DTYPE record, allowed VLANs)]."""
    cfg = {int(p["port_id"]): (p, set(allowed)) for p, allowed in ports}

    def allows(port):
        if port not in cfg or not cfg[port][0]["has_vlan_config"]:
            return False
        p, allowed = cfg[port]
        return vlan == int(p["native_vlan"]) if int(p["type"]) == nf.L2_ACCESS else vlan in allowed

    out = []
    for p in range(num_ports):
        if p == ingress or p not in cfg:
            continue
        if not cfg[p][0]["link_up"] or not cfg[p][0]["stp_forwarding"] or not (allows(ingress) and allows(p)):
            continue
        out.append(p)
    return out


def model_expand(ports, ingress, num_ports, arena_bytes, copy_base, copy_align, desc, cap, l3_port=None, fwd_status=None,
                 l2_port=None, l2_verdict=None, l2_vlan=None):
    """The sequential walk with Python lists: the dict Fdb.flood_expand_host returns."""
    items, used, is_open = [], 0, True
    emitted = {"items": 0, "copies": 0, "copy_bytes": 0}
    flooded = needed = 0
    for i, d in enumerate(desc):
        off, ln = int(d["off16"]) * 16, int(d["len"])
        if off + round_up(ln, 16) > copy_base:
            continue
        port = NONE
        if l3_port is not None and int(l3_port[i]) != NONE and (fwd_status is None or int(fwd_status[i]) & nf.ST_FLAG_FWD):
            port = int(l3_port[i])
        elif l2_port is not None:
            port = int(l2_port[i])
        if port != NONE:
            todo = [(port, 0)]
        elif l2_verdict is not None and int(l2_verdict[i]) == nf.L2_FLOOD:
            flooded += 1
            todo = [(p, round_up(ln, copy_align)) for p in model_flood_ports(ports, ingress, int(l2_vlan[i]), num_ports)]
        else:
            continue
        for p, slot in todo:
            at = copy_base + used
            used += slot
            is_open = is_open and needed < cap and copy_base + used <= arena_bytes
            if is_open:
                items.append(((int(d["off16"]), ln) if port != NONE else (at // 16, ln), p, i))
                emitted["items"] += 1
                if port == NONE:
                    emitted["copies"] += 1
                    emitted["copy_bytes"] += slot
            needed += 1
    item_desc, item_port = np.zeros(cap, nf.DESC_DTYPE), np.full(cap, nf.IF_NONE, np.uint32)
    item_src = np.full(cap, nf.ITEM_NONE, np.uint32)
    for k, (dd, p, i) in enumerate(items):
        item_desc[k], item_port[k], item_src[k] = dd, p, i
    totals = np.zeros(1, nf.FLOOD_TOTALS_DTYPE)[0]
    totals["items"], totals["items_needed"], totals["copies"] = emitted["items"], needed, emitted["copies"]
    totals["flooded"], totals["copy_bytes"], totals["copy_bytes_needed"] = flooded, emitted["copy_bytes"], used
    return {"item_desc": item_desc, "item_port": item_port, "item_src": item_src, "totals": totals}


def assert_same_expand(got, want, what=""):
    for k in ("items", "items_needed", "copies", "flooded", "copy_bytes", "copy_bytes_needed"):
        assert int(got["totals"][k]) == int(want["totals"][k]), f"{what}totals.{k}: {got['totals'][k]} != {want['totals'][k]}"
    for k in ("item_desc", "item_port", "item_src"):
        assert np.array_equal(got[k], want[k]), f"{what}{k} differs"


def copy_model(arena, desc, out, copy_base):
    """The arena after the expand: every emitted copy holds its source's whole 16-byte chunks; no other byte
    changes. arena: the bytes before (numpy u8, arena_bytes long)."""
    after = arena.copy()
    n_items = int(out["totals"]["items"])
    at = out["item_desc"]["off16"][:n_items].astype(np.int64) * 16
    for k in np.flatnonzero(at >= copy_base):
        o = int(at[k])
        s = int(desc[int(out["item_src"][k])]["off16"]) * 16
        ln = round_up(int(out["item_desc"][k]["len"]), 16)
        after[o:o + ln] = arena[s:s + ln]
    return after


def pack_with_tail(frames, align, tail, fill=FILL):
    """Frames packed at `align`-byte starts, then `tail` bytes of copy region: (arena, desc, copy_base). The
    region and the padding between frames hold `fill`."""
    desc = np.zeros(len(frames), nf.DESC_DTYPE)
    pos = 0
    for i, f in enumerate(frames):
        desc[i] = (pos // 16, len(f))
        pos += round_up(max(len(f), 1), align)
    copy_base = round_up(pos, 128)
    arena = np.full(copy_base + tail, fill, np.uint8)
    for d, f in zip(desc, frames):
        o = int(d["off16"]) * 16
        arena[o:o + len(f)] = np.frombuffer(bytes(f), np.uint8)
    return arena, desc, copy_base


def packed(lens, align=16):
    """n descriptors packed at `align`-byte starts: (desc, bytes used)."""
    desc = np.zeros(len(lens), nf.DESC_DTYPE)
    pos = 0
    for i, ln in enumerate(lens):
        desc[i] = (pos // 16, ln)
        pos += round_up(max(int(ln), 1), align)
    return desc, pos


def small_burst():
    """Ports 0..3 ACCESS on VLAN 1, ingress 0: a flooded packet goes to ports 1, 2, 3. Packets: unicast, flood,
    unicast, flood, unicast, 20 bytes each: nine items, six copies of 32 bytes in 16-byte slots."""
    fdb = nf.Fdb()
    for p in range(4):
        fdb.set_port(p, native_vlan=1)
    desc, used = packed([20] * 5)
    l2 = np.array([2, NONE, 3, NONE, 1], np.uint32)
    verdict = np.where(l2 == NONE, nf.L2_FLOOD, nf.L2_FORWARD).astype(np.uint8)
    return fdb.commit(), desc, round_up(used, 128), dict(l2_port=l2, l2_verdict=verdict, l2_vlan=np.ones(5, np.uint16))


FULL_PORTS, FULL_SRC = [2, 1, 2, 3, 3, 1, 2, 3, 1], [0, 1, 1, 1, 2, 3, 3, 3, 4]
# (cap, bytes of copy region) -> items emitted
CUTS = {(0, 1000): 0, (2, 1000): 2, (9, 192): 9, (12, 200): 9, (12, 0): 1, (12, 64): 3, (12, 95): 3, (12, 96): 5,
        (5, 128): 5, (8, 191): 7, (4, 32): 2}
