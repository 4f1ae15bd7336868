"""GPU tests of the TX queues (nfcs_txq_append_device / nfcs_txq_dequeue_device), all through the C ABI: the
device copy is held to the reference-made fixture or to the host copy driven in lockstep. Compared: d_tx,
d_tx_queue, d_tx_start, d_dequeued, d_depth, and head / last through the two state calls."""
import numpy as np
import pytest

import netflow_amd as nf
import oracle
from acl_common import eval_host, rule
from egress_common import plan_host
from flood_common import copy_model
from l2_common import decide_host as l2_decide_host
from l2_common import entries_of
from route_common import FWD_DSTS, decide_host as route_decide_host
from route_common import fixture_fib, route_fixture
from txq_common import (Q, apply_schedulers, fixture_egress, fixture_ticks, random_burst, random_txq_table, set_schedulers,
                        txq_fixture, want_tx)

pytestmark = pytest.mark.gpu

FILL = 0xEE
EE4, EE8 = 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE
BLOCK = 256  # the append's and the gather's workgroup


def up(engine, a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return engine.alloc(max(a.nbytes, 16)).upload(a)


def filled(engine, nbytes):
    return engine.alloc(nbytes + 16).upload(np.full(nbytes + 16, FILL, np.uint8))


class Lockstep:
    """One Egress and one TxQueues with a device copy; tick() runs enqueue -> append -> dequeue on the device
    and on the host copy and compares everything the two report, guard elements included."""

    def __init__(self, engine, eg, cfg=None):
        self.engine, self.eg = engine, eg
        eg.upload(engine)
        self.txq = nf.TxQueues(eg, engine)
        if cfg is not None:
            apply_schedulers(self.txq, cfg)
        self.ports, self.keys = self.txq.ports, self.txq.keys
        self.depth = np.zeros(self.keys, np.uint32)
        self.d_depth = engine.alloc(4 * self.keys + 32).upload(np.concatenate([self.depth, np.full(4, EE4, np.uint32)]))

    def close(self):
        self.txq.close()

    def enqueue_append(self, port, queue, handle=None, desc=None, what=""):
        e, n = self.engine, len(port)
        d_port, d_queue = up(e, port, np.uint32), up(e, queue, np.uint8)
        d_order, d_ks = filled(e, 4 * (n + 1)), filled(e, 4 * (self.keys + 2))
        d_handle = None if handle is None else up(e, handle, np.uint64)
        d_desc = None if desc is None else up(e, desc, nf.DESC_DTYPE)
        e.egress_enqueue_device(self.eg, d_port, d_queue, n, self.d_depth, d_order, d_ks)
        e.txq_append_device(self.txq, d_order, d_ks, self.d_depth, n, handle=d_handle, desc=d_desc)
        r = self.eg.enqueue_host(port, queue, self.depth)
        self.txq.append_host(r["order"], r["key_start"], r["depth"], n, handle=handle, desc=desc)
        self.depth = r["depth"]
        if n:
            e.sync()
            assert np.array_equal(d_ks.download(np.uint32, self.keys + 1), r["key_start"]), what + "key_start"
        return int(r["key_start"][self.keys])

    def dequeue(self, tx_cap, budget=None, budget_all=0, what="", optional=True):
        e = self.engine
        d_tx, d_txq = filled(e, 8 * (tx_cap + 1)), filled(e, tx_cap + 1)
        d_start, d_deq = filled(e, 4 * (self.ports + 2)), filled(e, 4 * (self.keys + 1))
        e.txq_dequeue_device(self.txq, self.d_depth, d_tx, tx_cap, d_start, budget=None if budget is None else up(e, budget, np.uint32),
                             budget_all=budget_all, tx_queue=d_txq if optional else None, dequeued=d_deq if optional else None)
        want = self.txq.dequeue_host(self.depth, tx_cap, budget=budget, budget_all=budget_all)
        self.depth = want["depth"]
        head, last = self.txq.state_device()
        hh, hl = self.txq.state_host()
        total = int(want["tx_start"][self.ports])
        start = d_start.download(np.uint32, self.ports + 2)
        assert np.array_equal(start[:self.ports + 1], want["tx_start"]) and start[self.ports + 1] == EE4, what + "tx_start"
        tx = d_tx.download(np.uint64, tx_cap + 1)
        assert np.array_equal(tx[:total], want["tx"]), what + "tx"
        assert (tx[total:] == EE8).all(), what + "entries of tx past the total must stay as they were"
        dep = self.d_depth.download(np.uint32, self.keys + 1)
        assert np.array_equal(dep[:self.keys], want["depth"]) and dep[self.keys] == EE4, what + "depth"
        if optional:
            tq = d_txq.download(np.uint8, tx_cap + 1)
            assert np.array_equal(tq[:total], want["tx_queue"]) and (tq[total:] == FILL).all(), what + "tx_queue"
            dq = d_deq.download(np.uint32, self.keys + 1)
            assert np.array_equal(dq[:self.keys], want["dequeued"]) and dq[self.keys] == EE4, what + "dequeued"
        assert np.array_equal(head, hh), what + "head"
        assert np.array_equal(last, hl), what + "last"
        want["tx_buf"] = tx
        return want


@pytest.fixture(scope="module")
def fx():
    return txq_fixture()


# ---- the fixture ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("handles", ["caller", "desc"])
def test_fixture_ticks_match_reference(engine, fx, handles):
    z = fx
    nports, ticks = fixture_ticks(z)
    flen = z["frames"].shape[1]
    with fixture_egress(z) as eg:
        ls = Lockstep(engine, eg)
        set_schedulers(ls.txq, z)
        enq, deq = np.zeros(nports * Q, np.uint32), np.zeros(nports * Q, np.uint32)
        for t, tk in enumerate(ticks):
            queue = np.array([eg.plan_host(int(p), z["frames"][tk["lo"] + i].tobytes())[1] for i, p in enumerate(tk["port"])],
                             np.uint8)
            seq = np.arange(tk["lo"], tk["hi"], dtype=np.uint64)
            before = ls.depth.copy()
            if handles == "caller":
                ls.enqueue_append(tk["port"], queue, handle=seq, what=f"tick {t}: ")
            else:
                desc = np.zeros(len(seq), nf.DESC_DTYPE)
                desc["off16"], desc["len"] = seq, flen
                ls.enqueue_append(tk["port"], queue, desc=desc, what=f"tick {t}: ")
            enq += ls.depth - before
            assert np.array_equal(enq, tk["stats_enq"][:, 0]) and np.array_equal(ls.depth, tk["stats_enq"][:, 3])
            got = ls.dequeue(4096, budget=tk["budget"], what=f"tick {t}: ")
            tx, tx_queue, tx_start = want_tx(tk, nports, z["queue"])
            if handles == "desc":
                tx = tx | np.uint64(flen << 32)
            assert np.array_equal(got["tx_start"], tx_start) and np.array_equal(got["tx"], tx), f"tick {t}"
            assert np.array_equal(got["tx_queue"], tx_queue), f"tick {t}"
            deq += got["dequeued"]
            assert np.array_equal(deq, tk["stats_deq"][:, 2]) and np.array_equal(ls.depth, tk["stats_deq"][:, 3]), f"tick {t}"
        ls.close()


# ---- launch geometry --------------------------------------------------------------------------------------

def deep_table(ports=4, depth=400, scheds=(nf.SCHED_WRR, nf.SCHED_STRICT_PRIORITY, nf.SCHED_DRR, nf.SCHED_WRR)):
    eg = nf.Egress()
    for p in range(ports):
        eg.set_port(p, has_vlan_config=False, num_queues=(8, 3, 5, 1)[p % 4], max_queue_depth=depth)
    return eg.commit(), {p: ((8, 3, 5, 1)[p % 4], depth, scheds[p % 4]) for p in range(ports)}


@pytest.mark.parametrize("total", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 65])
def test_totals_around_the_launch_geometry(engine, total):
    """`total` enqueued positions for the append (inside a burst of more packets, the others without a port)
    and `total` dequeued elements for the gather; then a second pair that leaves 65 behind."""
    rng = np.random.default_rng(total)
    eg, cfg = deep_table()
    with eg:
        ls = Lockstep(engine, eg, cfg)
        for rnd, leave in enumerate((0, 65)):
            port, queue = random_burst(rng, cfg, 4, total + leave)
            gaps = np.sort(rng.choice(len(port) + 40, 40, replace=False))
            port = np.insert(port, gaps - np.arange(40), nf.IF_NONE).astype(np.uint32)  # n > the positions
            queue = np.insert(queue, gaps - np.arange(40), nf.QUEUE_NONE).astype(np.uint8)
            handle = rng.integers(1, 1 << 63, len(port), dtype=np.uint64)
            assert ls.enqueue_append(port, queue, handle=handle) == total + leave
            got = ls.dequeue(total, budget_all=1 << 20, what=f"round {rnd}: ")  # tx_cap is the total exactly
            assert len(got["tx"]) == total
        ls.close()


def test_one_port_one_queue(engine):
    with nf.Egress().set_port(0, has_vlan_config=False, num_queues=1, max_queue_depth=3).commit() as eg:
        ls = Lockstep(engine, eg, {0: (1, 3, nf.SCHED_DRR)})
        for t in range(6):
            n = (2, 3, 0, 1, 5, 2)[t]
            ls.enqueue_append(np.zeros(n, np.uint32), np.zeros(n, np.uint8), handle=np.arange(n, dtype=np.uint64) + 100 * t)
            ls.dequeue(8, budget_all=(1, 0, 2, 9, 2, 9)[t], what=f"tick {t}: ")
        ls.close()


def test_whole_key_space(engine):
    """1,024 ports x 8 queues, 0-3 packets per key: the searches' full trip count, every port lane of the plan."""
    rng = np.random.default_rng(88)
    nports = nf.L2_MAX_PORTS
    eg, cfg = random_txq_table(rng, nports, depths=(1, 2, 3, 4), p_qos=0.95)
    with eg:
        ls = Lockstep(engine, eg, cfg)
        for t in range(2):
            counts = rng.integers(0, 4, nports * Q)
            key = rng.permutation(np.repeat(np.arange(nports * Q), counts))
            port, queue = (key // Q).astype(np.uint32), (key % Q).astype(np.uint8)
            ls.enqueue_append(port, queue, handle=rng.integers(1, 1 << 63, len(key), dtype=np.uint64))
            if t == 0:
                got = ls.dequeue(1 << 15, budget=rng.choice([0, 1, 2, 3, 7, 100], nports).astype(np.uint32), what="tick 0: ")
            else:
                got = ls.dequeue(1 << 15, budget_all=1000, what="tick 1: ")
                assert not ls.depth.any()
            assert len(got["tx"]) > 1000
        ls.close()


@pytest.mark.parametrize("sched", [nf.SCHED_STRICT_PRIORITY, nf.SCHED_WRR])
def test_small_rings_wrap(engine, sched):
    """Rings of cap 1, 2 and 5 through 10 ticks: head wraps several times; budgets per port and budget_all."""
    rng = np.random.default_rng(5 + sched)
    eg, cfg = nf.Egress(), {}
    for p, (nq, cap) in enumerate(((2, 1), (3, 2), (4, 5), (1, 5), (8, 2))):
        eg.set_port(p, has_vlan_config=False, num_queues=nq, max_queue_depth=cap)
        cfg[p] = (nq, cap, sched)
    with eg.commit():
        ls = Lockstep(engine, eg, cfg)
        moved = np.zeros(ls.keys, np.uint64)
        every_key = np.array([p * Q + q for p, (nq, _c, _s) in cfg.items() for q in range(nq)])
        for t in range(10):
            key = rng.permutation(np.repeat(every_key, 3))  # three packets for every queue: the small rings overflow
            ls.enqueue_append((key // Q).astype(np.uint32), (key % Q).astype(np.uint8),
                              handle=rng.integers(1, 1 << 63, len(key), dtype=np.uint64))
            if t % 2:
                got = ls.dequeue(200, budget=rng.integers(8, 14, 5).astype(np.uint32), what=f"tick {t}: ")
            else:
                got = ls.dequeue(200, budget_all=int(rng.integers(8, 12)), what=f"tick {t}: ", optional=t % 4 == 0)
            moved += got["dequeued"]
        assert (moved[:2] >= 10).all() and moved[2 * Q] >= 10  # the cap-1 rings wrapped every tick, a cap-5 ring twice
        ls.close()


@pytest.mark.parametrize("cap_at", ["zero", "mid_port", "port_edge", "total", "above"])
def test_tx_cap(engine, cap_at):
    rng = np.random.default_rng(17)
    eg, cfg = deep_table(depth=40)
    with eg:
        ls = Lockstep(engine, eg, cfg)
        port, queue = random_burst(rng, cfg, 4, 300)
        total = ls.enqueue_append(port, queue, handle=rng.integers(1, 1 << 63, 300, dtype=np.uint64))
        per_port = [int(ls.depth[p * Q:(p + 1) * Q].sum()) for p in range(4)]
        tx_cap = {"zero": 0, "mid_port": per_port[0] + per_port[1] // 2, "port_edge": per_port[0] + per_port[1], "total": total,
                  "above": total + 9}[cap_at]
        got = ls.dequeue(tx_cap, budget_all=1 << 30, what="capped: ")
        assert int(got["tx_start"][4]) == min(tx_cap, total)
        rest = ls.dequeue(512, budget_all=1 << 30, what="the rest: ")
        assert len(got["tx"]) + len(rest["tx"]) == total and not ls.depth.any()
        ls.close()


def test_a_tick_that_dequeues_nothing(engine):
    rng = np.random.default_rng(3)
    eg, cfg = deep_table(depth=10)
    with eg:
        ls = Lockstep(engine, eg, cfg)
        port, queue = random_burst(rng, cfg, 4, 100)
        ls.enqueue_append(port, queue, handle=np.arange(100, dtype=np.uint64))
        before = ls.depth.copy()
        for kw in (dict(budget_all=0), dict(budget=np.zeros(4, np.uint32))):
            got = ls.dequeue(64, what="nothing: ", **kw)
            assert len(got["tx"]) == 0 and not got["tx_start"].any() and np.array_equal(ls.depth, before)
        ls.enqueue_append(np.zeros(0, np.uint32), np.zeros(0, np.uint8), handle=np.zeros(0, np.uint64))  # n == 0: no launch
        ls.dequeue(64, budget_all=3, what="after: ")
        ls.close()


def test_dequeue_is_deterministic(engine):
    """The same dequeue on two copies of one state: identical outputs, the whole buffers."""
    rng = np.random.default_rng(29)
    eg, cfg = deep_table(ports=8, depth=60)
    with eg:
        a, b = Lockstep(engine, eg, cfg), Lockstep(engine, eg, cfg)
        port, queue = random_burst(rng, cfg, 8, 2000)
        handle = rng.integers(1, 1 << 63, 2000, dtype=np.uint64)
        budget = rng.integers(0, 90, 8).astype(np.uint32)
        outs = []
        for ls in (a, b):
            ls.enqueue_append(port, queue, handle=handle)
            outs.append(ls.dequeue(700, budget=budget))
        for k in ("tx_buf", "tx_queue", "tx_start", "dequeued", "depth"):
            assert np.array_equal(outs[0][k], outs[1][k]), k
        assert all(np.array_equal(x, y) for x, y in zip(a.txq.state_device(), b.txq.state_device()))
        a.close(), b.close()


def test_inconsistent_depths_append_nothing(engine):
    """depth > cap, depth < cnt and order entries >= n: the device appends what the host does, nothing else."""
    with nf.Egress().set_port(0, has_vlan_config=False, num_queues=2, max_queue_depth=4).commit() as eg:
        ls = Lockstep(engine, eg, {0: (2, 4, nf.SCHED_STRICT_PRIORITY)})
        ls.enqueue_append(np.zeros(4, np.uint32), np.array([0, 0, 1, 1], np.uint8), handle=np.array([1, 2, 3, 4], np.uint64))
        key_start = np.zeros(Q + 1, np.uint32)
        key_start[1:] = 3
        handle = np.array([91, 92, 93], np.uint64)
        for bad0 in (9, 2, 4):  # above the cap; below cnt; consistent with order entries >= n
            depth = ls.depth.copy()
            depth[0] = bad0
            order = np.array([0, 7, 2] if bad0 == 4 else [0, 1, 2], np.uint32)
            engine.txq_append_device(ls.txq, up(engine, order, np.uint32), up(engine, key_start, np.uint32),
                                     up(engine, depth, np.uint32), 3, handle=up(engine, handle, np.uint64))
            ls.txq.append_host(order, key_start, depth, 3, handle=handle)
        ls.depth[0], ls.depth[1] = 0xFFFFFFFF, 77  # read as the cap by the dequeue
        ls.d_depth.upload(ls.depth)
        got = ls.dequeue(16, budget_all=100)
        assert got["tx"].tolist() == [1, 91, 0, 93, 3, 4, 0, 0]
        ls.close()


def test_arguments(engine):
    L = nf.lib()
    with nf.Egress().set_port(1, has_vlan_config=False, num_queues=2, max_queue_depth=3).commit() as eg:
        ls = Lockstep(engine, eg)
        d = filled(engine, 256)
        c, x = engine.ctx, ls.txq.ptr
        assert L.nfcs_txq_append_device(c, x, d.ptr, d.ptr, d.ptr, None, None, 1, None) == -1  # both handle sources NULL
        assert L.nfcs_txq_append_device(c, x, None, None, None, None, None, 0, None) == 0      # n == 0
        assert L.nfcs_txq_append_device(c, x, None, d.ptr, d.ptr, d.ptr, None, 1, None) == -1
        assert L.nfcs_txq_append_device(c, x, d.ptr + 2, d.ptr, d.ptr, d.ptr, None, 1, None) == -1
        assert L.nfcs_txq_dequeue_device(c, x, None, 1, d.ptr, d.ptr, 4, None, None, None, None) == -1
        assert L.nfcs_txq_dequeue_device(c, x, None, 1, None, d.ptr, 4, None, d.ptr, None, None) == -1
        assert L.nfcs_txq_dequeue_device(c, x, None, 1, d.ptr, None, 4, None, d.ptr, None, None) == -1
        with nf.TxQueues(eg) as host_only:  # device calls on a host-only object
            assert L.nfcs_txq_dequeue_device(c, host_only.ptr, None, 1, d.ptr, d.ptr, 4, None, d.ptr, None, None) == -1
            assert L.nfcs_txq_append_device(c, host_only.ptr, d.ptr, d.ptr, d.ptr, d.ptr, None, 1, None) == -1
            assert L.nfcs_txq_state_device(host_only.ptr, None, None, None) == -1
        engine.sync()
        assert (d.download(np.uint8, 256) == FILL).all()
        ls.txq.reset()
        assert not ls.txq.state_device()[0].any()
        ls.close()
    with nf.Egress().commit() as eg:  # no port set: keys == 0
        ls = Lockstep(engine, eg)
        got = ls.dequeue(4, budget_all=5)
        assert got["tx_start"].tolist() == [0]
        ls.close()


# ---- the whole pipeline -------------------------------------------------------------------------------

def host_order(a: str) -> int:
    return int.from_bytes(bytes(int(x) for x in a.split(".")), "big")


def tagged_l2(rng, k):
    """k non-IP frames tagged with VLAN 1 and every PCP, to a dozen destination MACs: the FDB forwards half of
    them and floods the rest, and the ACCESS egress ports pop the tag."""
    out = []
    for i in range(k):
        tci = (int(rng.integers(0, 8)) << 13) | 1
        out.append(bytes([2, 0xAA, 0, 0, 0, i % 12]) + bytes([2, 0xBB, 0, 0, 0, 1]) + b"\x81\x00" + tci.to_bytes(2, "big") +
                   b"\x88\xb5" + bytes(rng.integers(0, 256, int(rng.integers(46, 200)), dtype=np.uint8)))
    return out


def test_whole_pipeline_over_two_bursts(engine):
    """route lookup -> ACL -> forward -> L2 lookup -> flood expand -> plan -> VLAN -> enqueue -> append -> dequeue: ten
    calls per burst on one stream with no host step between them, two bursts in a row on the same queues,
    against the oracle and the host functions chained on the CPU. The handles are the item descriptors as the
    VLAN edit left them."""
    z, fixture_frames = route_fixture()
    rng = np.random.default_rng(4)
    bursts = [tagged_l2(rng, 60) + fixture_frames[:400], tagged_l2(rng, 60) + fixture_frames[400:800]]
    frames_all = bursts[0] + bursts[1]
    cap, tail, tx_cap, budget_all, ingress, num_ports = 2048, 1 << 18, 4096, 40, 0, 4
    rules = np.concatenate([rule(nf.ACL_DENY, dst_ip=host_order(FWD_DSTS[0])), rule(nf.ACL_PERMIT)])
    with fixture_fib(z, "a") as fib, nf.Acl().set_rules(rules).commit() as acl, nf.Fdb() as fdb, nf.Egress() as eg:
        rt_all = route_decide_host(fib, frames_all)
        l2_frames = [f for f, v in zip(frames_all, rt_all[0]) if v == nf.RT_NOT_IPV4 and len(f) >= 14]
        macs = np.unique(np.array([np.frombuffer(f[:6], np.uint8) for f in l2_frames[::2]]), axis=0)
        fdb.set_entries(entries_of(macs, np.ones(len(macs)), 1 + np.arange(len(macs)) % 3))
        for p in range(num_ports):
            fdb.set_port(p, native_vlan=1)
        fdb.commit()
        ifs = sorted({int(x) for x in rt_all[2] if x != nf.IF_NONE} | {1, 2, 3})
        for k, p in enumerate(ifs):
            eg.set_port(p, type=(nf.L2_ACCESS, nf.L2_TRUNK)[k % 2], native_vlan=1, num_queues=(4, 8, 3)[k % 3],
                        max_queue_depth=(6, 25, 1000)[k % 3])
        eg.commit()
        for obj in (fib, acl, fdb, eg):
            obj.upload(engine)
        keys = eg.keys()[1]
        d_tab, tab_n = fib.nexthops()
        nht = fib.nexthops_host()
        with nf.TxQueues(eg, engine) as txq:
            for k, p in enumerate(ifs):
                txq.set_scheduler(p, (nf.SCHED_WRR, nf.SCHED_STRICT_PRIORITY, nf.SCHED_DRR)[k % 3])
            ports = txq.ports
            depth = np.zeros(keys, np.uint32)
            d_depth = up(engine, depth, np.uint32)
            launched = []
            for frames in bursts:  # both bursts are launched before anything is read back
                arena, desc = oracle.pack_frames(frames, align=128)
                copy_base = len(arena)
                arena = np.concatenate([arena, np.full(tail, FILL, np.uint8)])
                n = len(desc)
                d_arena, d_desc = up(engine, arena, np.uint8), up(engine, desc, nf.DESC_DTYPE)
                d_nh, d_if, d_rt, d_act, d_st = (engine.alloc(4 * n), engine.alloc(4 * n), engine.alloc(n), engine.alloc(n),
                                                 engine.alloc(n))
                d_l2, d_l2v, d_vlan = engine.alloc(4 * n), engine.alloc(n), engine.alloc(2 * n)
                d_idesc, d_iport, d_isrc, d_tot = engine.alloc(8 * cap), engine.alloc(4 * cap), engine.alloc(4 * cap), engine.alloc(32)
                d_port, d_ops, d_queue = engine.alloc(4 * cap), engine.alloc(4 * cap), engine.alloc(cap)
                d_order, d_ks = engine.alloc(4 * cap), engine.alloc(4 * (keys + 1))
                d_tx, d_txq, d_start, d_deq = filled(engine, 8 * tx_cap), filled(engine, tx_cap), engine.alloc(4 * (ports + 1)), engine.alloc(4 * keys)
                engine.route_lookup_device(fib, d_arena, copy_base, d_desc, n, d_nh, egress_if=d_if, verdict=d_rt)
                engine.acl_eval_device(acl, d_arena, copy_base, d_desc, n, d_act, nh=d_nh)
                engine.l3_forward_device(d_arena, copy_base, d_desc, d_nh, n, d_tab, tab_n, d_st)
                engine.l2_lookup_device(fdb, ingress, d_arena, copy_base, d_desc, n, d_l2, rt_verdict=d_rt, verdict=d_l2v, vlan=d_vlan)
                engine.flood_expand_device(fdb, ingress, num_ports, d_arena, arena.nbytes, copy_base, 128, d_desc, n, cap, d_idesc,
                                           d_iport, d_isrc, d_tot, l3_port=d_if, fwd_status=d_st, l2_port=d_l2, l2_verdict=d_l2v,
                                           l2_vlan=d_vlan)
                engine.egress_plan_device(eg, d_arena, arena.nbytes, d_idesc, cap, d_port, d_ops, d_queue, l2_port=d_iport)
                engine.vlan_device(d_arena, arena.nbytes, d_idesc, cap, d_ops, 0, None, 128)
                engine.egress_enqueue_device(eg, d_port, d_queue, cap, d_depth, d_order, d_ks)
                engine.txq_append_device(txq, d_order, d_ks, d_depth, cap, desc=d_idesc)
                engine.txq_dequeue_device(txq, d_depth, d_tx, tx_cap, d_start, budget_all=budget_all, tx_queue=d_txq, dequeued=d_deq)
                launched.append((arena, desc, copy_base, d_arena, d_idesc, d_tx, d_txq, d_start, d_deq))
            engine.sync()
            final_depth = d_depth.download(np.uint32, keys)
            # the CPU chain, burst by burst, on the host copy of the same object
            flooded = dropped = popped_handles = 0
            before_edit, by_bits = set(), set()  # over both bursts: the second dequeue also returns packets of the first
            for frames, (arena, desc, copy_base, d_arena, d_idesc, d_tx, d_txq, d_start, d_deq) in zip(bursts, launched):
                want_rt, want_nh, want_if = route_decide_host(fib, frames)
                want_action, _, _ = eval_host(acl, frames)
                masked = np.where(want_action == nf.ACL_PERMIT, want_nh, nf.NH_NONE).astype(np.uint32)
                ref, rdesc = arena.copy(), desc.copy()
                rst = oracle.l3_forward_batch(ref[:copy_base], rdesc, masked, nht.view(np.uint8).reshape(-1, 12))
                l2 = l2_decide_host(fdb, ingress, frames)
                skip = want_rt != nf.RT_NOT_IPV4
                l2_port = np.where(skip, nf.IF_NONE, l2[1]).astype(np.uint32)
                l2_verdict = np.where(skip, nf.L2_SKIP, l2[0]).astype(np.uint8)
                ex = fdb.flood_expand_host(ingress, num_ports, arena.nbytes, copy_base, 128, rdesc, cap, l3_port=want_if,
                                           fwd_status=rst, l2_port=l2_port, l2_verdict=l2_verdict, l2_vlan=l2[2])
                ref = copy_model(ref, rdesc, ex, copy_base)
                items = int(ex["totals"]["items"])
                assert items == int(ex["totals"]["items_needed"])
                flooded += int(ex["totals"]["flooded"])
                idesc = ex["item_desc"].copy()
                before_edit |= {int(d["off16"]) | int(d["len"]) << 32 for d in idesc[:items]}
                item_frames = oracle.unpack_frames(ref, idesc)
                ops, queue = plan_host(eg, ex["item_port"], item_frames)
                queue[ex["item_port"] == nf.IF_NONE] = nf.QUEUE_NONE
                oracle.vlan_batch(ref, idesc, ops, None, cap_all=128)
                r = eg.enqueue_host(ex["item_port"], queue, depth)
                dropped += int(r["key_dropped"].sum())
                txq.append_host(r["order"], r["key_start"], r["depth"], cap, desc=idesc)
                want = txq.dequeue_host(r["depth"], tx_cap, budget_all=budget_all)
                depth = want["depth"]
                total = int(want["tx_start"][ports])
                assert total > 30
                assert np.array_equal(d_arena.download(np.uint8, arena.nbytes), ref), "the frames differ from the oracle"
                assert np.array_equal(d_idesc.download(nf.DESC_DTYPE, cap), idesc)
                assert np.array_equal(d_start.download(np.uint32, ports + 1), want["tx_start"])
                tx = d_tx.download(np.uint64, tx_cap)
                assert np.array_equal(tx[:total], want["tx"]) and (tx[total:] == EE8).all()
                assert np.array_equal(d_txq.download(np.uint8, tx_cap)[:total], want["tx_queue"])
                assert np.array_equal(d_deq.download(np.uint32, keys), want["dequeued"])
                # a handle is its item's descriptor after the VLAN edit
                by_bits |= {int(d["off16"]) | int(d["len"]) << 32 for d in idesc[:items]}
                assert {int(h) for h in want["tx"]} <= by_bits
                popped_handles += len({int(h) for h in want["tx"]} - before_edit)
            assert flooded > 5 and dropped > 10 and popped_handles > 5
            assert np.array_equal(final_depth, depth)
            assert all(np.array_equal(x, y) for x, y in zip(txq.state_device(), txq.state_host()))
