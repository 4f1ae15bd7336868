"""Shared inputs for the egress tests: the reference-made fixture tests/golden/egress_ref.npz
(tests/golden/make_egress_golden.py) and what it says of the burst in the form the library reports it, an
Egress built from its ports, and a plain-Python restatement of process_egress, classify_packet_to_queue
and enqueue_packet that shares no code with the library."""
import os

import numpy as np

import netflow_amd as nf

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WARM = 0x80000000
Q = nf.QOS_MAX_QUEUES


def egress_fixture():
    z = np.load(os.path.join(GOLD, "egress_ref.npz"))
    frames = [bytes(z["frames_in"][i, :int(ln)]) for i, ln in enumerate(z["lens_in"])]
    return z, frames


def fixture_ports(z):
    return np.ascontiguousarray(z["ports"]).view(nf.EGRESS_PORT_DTYPE).reshape(-1)


def set_ports(eg: nf.Egress, ports):
    for p in ports:
        eg.set_port(int(p["port_id"]), int(p["has_vlan_config"]), int(p["type"]), int(p["tag_native"]),
                    int(p["native_vlan"]), int(p["has_qos"]), int(p["num_queues"]), int(p["max_queue_depth"]))
    return eg


def fixture_egress(z) -> nf.Egress:
    return set_ports(nf.Egress(), fixture_ports(z)).commit()


def fixture_want(z):
    """What the reference did with the burst, as the library reports it: ops, queue (its classify on the
    edited frame; the library says the same of a port without QoS: 0), depth before and after, result,
    the order per key, key_start, key_dropped. Keys = (highest port id + 1) * 8."""
    ports = fixture_ports(z)
    nports = int(ports["port_id"].max()) + 1
    keys = nports * Q
    n = len(z["port"])
    NONE = 0xFFFFFFFF
    depth0, depth1, dropped = np.zeros(keys, np.uint32), np.zeros(keys, np.uint32), np.zeros(keys, np.uint32)
    order = {}
    for i, p in enumerate(ports):
        for q in range(Q):
            k = int(p["port_id"]) * Q + q
            if z["stats_before"][i, q, 0] == NONE:
                continue
            depth0[k], depth1[k] = z["stats_before"][i, q, 2], z["stats_after"][i, q, 2]
            dropped[k] = z["stats_after"][i, q, 1] - z["stats_before"][i, q, 1]
            seq = z["deq_index"][int(z["deq_start"][i * Q + q]):int(z["deq_start"][i * Q + q + 1])]
            order[k] = seq[(seq & WARM) == 0].astype(np.uint32)
    has_qos = {int(p["port_id"]): bool(p["has_qos"]) for p in ports}
    result = np.full(n, nf.EQ_DROP_FULL, np.uint8)
    for i, port in enumerate(z["port"]):
        if not has_qos.get(int(port), False):
            result[i] = nf.EQ_DROP_NO_CONFIG
    for seq in order.values():
        result[seq] = nf.EQ_ENQUEUED
    key_start = np.zeros(keys + 1, np.uint32)
    for k in range(keys):
        key_start[k + 1] = key_start[k] + len(order.get(k, ()))
    flat = np.concatenate([order.get(k, np.zeros(0, np.uint32)) for k in range(keys)]).astype(np.uint32)
    ops = np.where(z["lens_out"] != z["lens_in"], nf.VLAN_POP, nf.VLAN_NOP).astype(np.uint32)
    return {"ops": ops, "queue": z["queue"].astype(np.uint8), "depth0": depth0, "depth": depth1, "result": result,
            "order": flat, "key_start": key_start, "key_dropped": dropped, "keys": keys}


def plan_host(eg: nf.Egress, ports, frames):
    n = len(frames)
    ops, queue = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    for i, (p, f) in enumerate(zip(ports, frames)):
        ops[i], queue[i] = eg.plan_host(int(p), f)
    return ops, queue


# ---- the restatement ------------------------------------------------------------------------------

def model_plan(cfg, port, f):
    """cfg: {port id: EGRESS_PORT_DTYPE record}. (op, queue) for frame f leaving through port."""
    if port == nf.IF_NONE:
        return nf.VLAN_NOP, nf.QUEUE_NONE
    p = cfg.get(port)
    f = bytes(f)

    def tagged(b):
        return len(b) >= 18 and b[12:14] == b"\x81\x00"

    pop = False
    if p is not None and p["has_vlan_config"] and tagged(f):
        vid = int.from_bytes(f[14:16], "big") & 0xFFF
        if vid == int(p["native_vlan"]) and (int(p["type"]) == nf.L2_ACCESS or not p["tag_native"]):
            pop = True
    after = f[:12] + f[16:] if pop else f
    if p is None or not p["has_qos"]:
        return (nf.VLAN_POP if pop else nf.VLAN_NOP), 0
    nq = max(int(p["num_queues"]), 1)
    if tagged(after):
        pcp = after[14] >> 5
        q = (0, 0, 1, 1, 2, 2, 3, 3)[7 - pcp] if nq == 4 else int(((7 - pcp) * nq) / 8.0)
        q = min(q, nq - 1)
    else:
        q = nq - 1
    return (nf.VLAN_POP if pop else nf.VLAN_NOP), q


def model_enqueue(cfg, keys, port, queue, depth):
    """The sequential walk with one Python list per queue."""
    depth = [int(d) for d in depth]
    queues = {}
    result = np.zeros(len(port), np.uint8)
    dropped = np.zeros(keys, np.uint32)
    for i, (pt, q) in enumerate(zip(port, queue)):
        pt, q = int(pt), int(q)
        p = cfg.get(pt)
        if pt == nf.IF_NONE:
            result[i] = nf.EQ_SKIP
        elif p is None or not p["has_qos"]:
            result[i] = nf.EQ_DROP_NO_CONFIG
        elif q >= max(int(p["num_queues"]), 1):
            result[i] = nf.EQ_BAD_QUEUE
        else:
            k = pt * Q + q
            if depth[k] >= max(int(p["max_queue_depth"]), 1):
                result[i] = nf.EQ_DROP_FULL
                dropped[k] += 1
            else:
                queues.setdefault(k, []).append(i)
                depth[k] += 1
                result[i] = nf.EQ_ENQUEUED
    key_start = np.zeros(keys + 1, np.uint32)
    for k in range(keys):
        key_start[k + 1] = key_start[k] + len(queues.get(k, ()))
    order = np.array([i for k in range(keys) for i in queues.get(k, ())], np.uint32)
    return {"depth": np.array(depth, np.uint32), "result": result, "order": order, "key_start": key_start,
            "key_dropped": dropped}


def random_table(rng, nports, p_set=0.8):
    """(Egress committed, cfg dict) over port ids below nports."""
    eg, cfg = nf.Egress(), {}
    for pid in range(nports):
        if rng.random() >= p_set:
            continue
        rec = np.zeros(1, nf.EGRESS_PORT_DTYPE)[0]
        rec["port_id"], rec["has_vlan_config"], rec["type"] = pid, rng.random() < 0.8, int(rng.integers(0, 3))
        rec["tag_native"], rec["has_qos"] = rng.random() < 0.5, rng.random() < 0.85
        rec["native_vlan"] = int(rng.choice([1, 10, 20, 4095, 0]))
        rec["num_queues"], rec["max_queue_depth"] = int(rng.integers(0, 9)), int(rng.choice([0, 1, 3, 7, 50, 100000]))
        cfg[pid] = rec
    set_ports(eg, cfg.values())
    return eg.commit(), cfg


def assert_same(got, want, what=""):
    for k in ("result", "key_start", "key_dropped", "depth", "order"):
        if got.get(k) is not None:
            assert np.array_equal(got[k], want[k]), f"{what}{k} differs"
