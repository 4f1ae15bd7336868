"""Shared inputs for the TX queue tests: the reference-made fixture tests/golden/txq_ref.npz
(tests/golden/make_txq_golden.py) cut into ticks, an Egress and its schedulers built from the fixture's
ports, and a plain-Python restatement of enqueue_packet's queues and select_packet_to_dequeue, one deque per
queue, that shares no code with the library."""
import os
from collections import deque

import numpy as np

import netflow_amd as nf

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Q = nf.QOS_MAX_QUEUES
NONE = 0xFFFFFFFF
UNSET_BUDGET = 7  # the budget the tests give to port ids the fixture never configures


def txq_fixture():
    return np.load(os.path.join(GOLD, "txq_ref.npz"))


def fixture_egress(z) -> nf.Egress:
    eg = nf.Egress()
    for pid, qos, nq, _sched, depth in z["ports"].tolist():
        eg.set_port(pid, has_vlan_config=False, has_qos=bool(qos), num_queues=nq, max_queue_depth=depth)
    return eg.commit()


def set_schedulers(txq: nf.TxQueues, z):
    for pid, _qos, _nq, sched, _depth in z["ports"].tolist():
        txq.set_scheduler(pid, sched)
    return txq


def fixture_ticks(z):
    """Per tick: the frames' global sequence numbers (lo, hi), port per frame, the reference's queue per
    frame, the budget per port id, and what the reference recorded: the dequeued sequence numbers per port
    id, and per key the counters {enqueued, dropped, dequeued, depth} after the burst and after the dequeues
    (zero for queues that do not exist)."""
    ports = z["ports"]
    nports = int(ports[:, 0].max()) + 1
    ticks = []
    for t in range(len(z["tick_start"]) - 1):
        lo, hi = int(z["tick_start"][t]), int(z["tick_start"][t + 1])
        budget = np.full(nports, UNSET_BUDGET, np.uint32)
        deq = {}
        stats = [np.zeros((nports * Q, 4), np.uint32) for _ in range(2)]
        for i, rec in enumerate(ports.tolist()):
            pid = rec[0]
            budget[pid] = z["budget"][t, i]
            a, b = int(z["deq_start"][t * len(ports) + i]), int(z["deq_start"][t * len(ports) + i + 1])
            deq[pid] = z["deq_seq"][a:b]
            for s, name in zip(stats, ("stats_enq", "stats_deq")):
                rows = z[name][t, i]
                s[pid * Q:(pid + 1) * Q] = np.where(rows == NONE, 0, rows)
        ticks.append({"lo": lo, "hi": hi, "port": z["port"][lo:hi], "queue": z["queue"][lo:hi], "budget": budget,
                      "deq": deq, "stats_enq": stats[0], "stats_deq": stats[1]})
    return nports, ticks


def want_tx(tick, nports, queue_of):
    """The reference's TX list of one tick as the library reports it: (tx handles = sequence numbers,
    tx_queue, tx_start)."""
    tx, start = [], [0]
    for pid in range(nports):
        tx += [int(s) for s in tick["deq"].get(pid, ())]
        start.append(len(tx))
    tx = np.array(tx, np.uint64)
    return tx, queue_of[tx.astype(np.int64)].astype(np.uint8), np.array(start, np.uint32)


# ---- the restatement ------------------------------------------------------------------------------

class ModelTxq:
    """cfg: {port id: (num_queues, max_queue_depth, sched)} for the ports with a QoS config."""

    def __init__(self, cfg, nports):
        self.cfg, self.nports = cfg, nports
        self.queues = {(p, q): deque() for p, (nq, _d, _s) in cfg.items() for q in range(nq)}
        self.last = {p: 0 for p in cfg}

    def enqueue(self, port, queue, handle):
        for pt, q, h in zip(port, queue, handle):
            pt, q = int(pt), int(q)
            if pt not in self.cfg or q >= self.cfg[pt][0]:
                continue
            dq = self.queues[(pt, q)]
            if len(dq) < self.cfg[pt][1]:
                dq.append(int(h))

    def select(self, p):
        if p not in self.cfg:
            return None
        nq, _d, sched = self.cfg[p]
        if sched == nf.SCHED_STRICT_PRIORITY:
            for q in range(nq):
                if self.queues[(p, q)]:
                    return q, self.queues[(p, q)].popleft()
            return None
        for i in range(nq):
            q = (self.last[p] + 1 + i) % nq
            if self.queues[(p, q)]:
                self.last[p] = q
                return q, self.queues[(p, q)].popleft()
        return None

    def dequeue(self, budget, tx_cap):
        tx, txq, start = [], [], []
        dequeued = np.zeros(self.nports * Q, np.uint32)
        for p in range(self.nports):
            start.append(len(tx))
            for _ in range(int(budget[p])):
                if len(tx) >= tx_cap:
                    break
                got = self.select(p)
                if got is None:
                    break
                tx.append(got[1])
                txq.append(got[0])
                dequeued[p * Q + got[0]] += 1
        start.append(len(tx))
        return {"tx": np.array(tx, np.uint64), "tx_queue": np.array(txq, np.uint8),
                "tx_start": np.array(start, np.uint32), "dequeued": dequeued}

    def depth(self):
        d = np.zeros(self.nports * Q, np.uint32)
        for (p, q), dq in self.queues.items():
            d[p * Q + q] = len(dq)
        return d

    def last_array(self):
        a = np.zeros(self.nports, np.uint8)
        for p, q in self.last.items():
            a[p] = q
        return a


def random_txq_table(rng, nports, depths=(1, 2, 5, 9), p_qos=0.85):
    """(Egress committed, cfg for ModelTxq) over port ids below nports; the last id is always set."""
    eg, cfg = nf.Egress(), {}
    for pid in range(nports):
        qos = rng.random() < p_qos
        nq, depth, sched = int(rng.integers(1, Q + 1)), int(rng.choice(depths)), int(rng.integers(0, 3))
        eg.set_port(pid, has_vlan_config=False, has_qos=qos, num_queues=nq, max_queue_depth=depth)
        if qos:
            cfg[pid] = (nq, depth, sched)
    return eg.commit(), cfg


def apply_schedulers(txq, cfg):
    for pid, (_nq, _d, sched) in cfg.items():
        txq.set_scheduler(pid, sched)
    return txq


def random_burst(rng, cfg, nports, n):
    """port and queue per packet: mostly valid (port, queue) pairs, some ports without QoS."""
    port = rng.integers(0, nports, n).astype(np.uint32)
    queue = np.array([int(rng.integers(0, cfg[int(p)][0])) if int(p) in cfg else 0 for p in port], np.uint8)
    return port, queue


def assert_tx_same(got, want, what=""):
    for k in ("tx_start", "tx", "tx_queue", "dequeued", "depth"):
        if k in want and k in got:
            assert np.array_equal(got[k], want[k]), f"{what}{k} differs"
