"""CPU tests of the TX queues' host side (nfcs_txq_*_host): the rings and the dequeue scheduler against the
reference-made fixture, the closed form the kernels compute against a plain-Python literal walk, the tx_cap
rule, the argument errors and inconsistent depths. No GPU: the objects are host-only (ctx NULL)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import netflow_amd as nf
from egress_common import model_enqueue
from txq_common import (ModelTxq, Q, apply_schedulers, assert_tx_same, fixture_egress, fixture_ticks, random_burst,
                        random_txq_table, set_schedulers, txq_fixture, want_tx)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    if not os.path.exists(nf.LIB_PATH):
        nf.build()
    return txq_fixture()


def frame_queue(eg, z, lo, hi):
    return np.array([eg.plan_host(int(z["port"][i]), z["frames"][i].tobytes())[1] for i in range(lo, hi)], np.uint8)


@pytest.mark.parametrize("handles", ["caller", "desc"])
def test_host_chain_matches_reference(fx, handles):
    """enqueue_host -> append_host -> dequeue_host over the fixture's ticks: every recorded sequence, depth
    and counter. Caller handles are the sequence numbers; descriptor handles carry them as off16."""
    z = fx
    nports, ticks = fixture_ticks(z)
    qos_ports = {int(r[0]) for r in z["ports"] if r[1]}
    with fixture_egress(z) as eg, nf.TxQueues(eg) as txq:
        set_schedulers(txq, z)
        assert txq.info()[:2] == (nports, nports * Q)
        depth = np.zeros(nports * Q, np.uint32)
        enq, drop, deq = (np.zeros(nports * Q, np.uint32) for _ in range(3))
        for t, tk in enumerate(ticks):
            n = tk["hi"] - tk["lo"]
            queue = frame_queue(eg, z, tk["lo"], tk["hi"])
            has = np.isin(tk["port"], list(qos_ports))
            assert np.array_equal(queue[has], tk["queue"][has]), f"tick {t}: classify differs"
            r = eg.enqueue_host(tk["port"], queue, depth)
            seq = np.arange(tk["lo"], tk["hi"], dtype=np.uint64)
            if handles == "caller":
                txq.append_host(r["order"], r["key_start"], r["depth"], n, handle=seq)
                hmask = 0
            else:
                desc = np.zeros(n, nf.DESC_DTYPE)
                desc["off16"], desc["len"] = seq, z["frames"].shape[1]
                txq.append_host(r["order"], r["key_start"], r["depth"], n, desc=desc)
                hmask = z["frames"].shape[1] << 32
            enq += np.diff(r["key_start"]).astype(np.uint32)
            drop += r["key_dropped"]
            assert np.array_equal(np.stack([enq, drop, deq, r["depth"]], 1), tk["stats_enq"]), f"tick {t}: after the burst"
            d = txq.dequeue_host(r["depth"], 1 << 16, budget=tk["budget"])
            tx, tx_queue, tx_start = want_tx(tk, nports, z["queue"])
            assert np.array_equal(d["tx_start"], tx_start), f"tick {t}: tx_start"
            assert np.array_equal(d["tx"], tx | np.uint64(hmask)), f"tick {t}: tx"
            assert np.array_equal(d["tx_queue"], tx_queue), f"tick {t}: tx_queue"
            deq += d["dequeued"]
            depth = d["depth"]
            assert np.array_equal(np.stack([enq, drop, deq, depth], 1), tk["stats_deq"]), f"tick {t}: after the dequeues"


def test_fixture_covers_the_cases(fx):
    z = fx
    ports = z["ports"]
    for sched in (0, 1, 2):
        assert {1, 2, 3, 4, 8} <= set(ports[(ports[:, 3] == sched) & (ports[:, 1] == 1)][:, 2].tolist())
    assert (ports[:, 1] == 0).any() and {1, 5} <= set(ports[:, 4].tolist())
    assert len(z["tick_start"]) - 1 >= 12
    nports, ticks = fixture_ticks(z)
    # a round-robin port whose first dequeue comes from queue 1 while queue 0 holds packets
    hit = False
    for pid, qos, nq, sched, _d in ports.tolist():
        first = ticks[0]["deq"][pid]
        if qos and sched != 0 and len(first):
            hit |= int(z["queue"][int(first[0])]) == 1 and ticks[0]["stats_enq"][pid * Q, 3] > 0
    assert hit
    caps = np.zeros(nports * Q, np.uint32)
    for pid, qos, nq, _s, d in ports.tolist():
        if qos:
            caps[pid * Q:pid * Q + nq] = d
    total_deq = ticks[-1]["stats_deq"][:, 2]
    assert (total_deq[caps > 0] >= 2 * caps[caps > 0]).any()  # a ring that wraps twice


def literal_walk(sched, depth, last, budget):
    depth, nq, seq = [int(d) for d in depth], len(depth), []
    for _ in range(budget):
        if sched == nf.SCHED_STRICT_PRIORITY:
            order = range(nq)
        else:
            order = [(last + 1 + i) % nq for i in range(nq)]
        q = next((q for q in order if depth[q] > 0), None)
        if q is None:
            break
        depth[q] -= 1
        if sched != nf.SCHED_STRICT_PRIORITY:
            last = q
        seq.append(q)
    return seq, last


def test_closed_form_equals_the_literal_walk():
    """txq_take and txq_rank (what the kernels compute), through nfcs_txq_closed_form_host, against the
    literal select_packet_to_dequeue walk in plain Python: 1-8 queues, all three schedulers, budgets from 0
    to past the total."""
    rng = np.random.default_rng(1810)
    for case in range(6000):
        nq, sched = int(rng.integers(1, 9)), int(rng.integers(0, 3))
        hi = int(rng.choice([1, 2, 4, 12]))
        depth = rng.integers(0, hi + 1, nq)
        depth[rng.random(nq) < 0.2] = 0
        last = int(rng.integers(0, nq))
        budget = int(rng.integers(0, int(depth.sum()) + 4))
        take, new_last, seq = nf.txq_closed_form_host(sched, depth, last, budget)
        want_seq, want_last = literal_walk(sched, depth, last, budget)
        what = f"case {case}: sched {sched} depth {depth.tolist()} last {last} budget {budget}"
        assert seq.tolist() == want_seq, what
        assert new_last == want_last, what
        assert take.tolist() == np.bincount(want_seq, minlength=nq).tolist(), what


def test_closed_form_large_depths():
    """Depths near 2^32: the sums run in 64 bits."""
    big = 0xFFFFFFFF
    take, new_last, _ = nf.txq_closed_form_host(nf.SCHED_WRR, [big, big, 5, big], 3, 0xFFFFFFFE, want_seq=False)
    assert int(take.astype(np.uint64).sum()) == 0xFFFFFFFE and take[2] == 5
    assert int(take[[0, 1, 3]].max()) - int(take[[0, 1, 3]].min()) <= 1
    take, new_last, _ = nf.txq_closed_form_host(nf.SCHED_STRICT_PRIORITY, [big, big], 0, big, want_seq=False)
    assert take.tolist() == [big, 0] and new_last == 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_matches_plain_python_restatement(seed):
    """Random tables, bursts and budgets over several ticks: dequeue_host against one deque per queue."""
    rng = np.random.default_rng(900 + seed)
    nports = (6, 30, 1)[seed - 1]
    eg, cfg = random_txq_table(rng, nports)
    egcfg = {p: {"has_qos": True, "num_queues": nq, "max_queue_depth": d} for p, (nq, d, _s) in cfg.items()}
    with eg, nf.TxQueues(eg) as txq:
        apply_schedulers(txq, cfg)
        model = ModelTxq(cfg, nports)
        depth = np.zeros(nports * Q, np.uint32)
        nxt = 1
        for tick in range(10):
            n = int(rng.integers(0, 12 * nports))
            port, queue = random_burst(rng, cfg, nports, n)
            handle = np.arange(nxt, nxt + n, dtype=np.uint64) * np.uint64(0x100000001)
            nxt += n
            r = eg.enqueue_host(port, queue, depth)
            assert np.array_equal(r["result"], model_enqueue(egcfg, nports * Q, port, queue, depth)["result"])
            txq.append_host(r["order"], r["key_start"], r["depth"], n, handle=handle)
            model.enqueue(port, queue, handle)
            assert np.array_equal(r["depth"], model.depth())
            budget = rng.choice([0, 1, 2, 3, 5, 11, 1000], nports).astype(np.uint32)
            tx_cap = int(rng.choice([0, 3, 17, 1 << 12]))
            if tick % 2:
                d = txq.dequeue_host(r["depth"], tx_cap, budget=budget)
            else:
                budget[:] = budget[0]
                d = txq.dequeue_host(r["depth"], tx_cap, budget_all=int(budget[0]))
            want = model.dequeue(budget, tx_cap)
            want["depth"] = model.depth()
            assert_tx_same(d, want, f"tick {tick}: ")
            depth = d["depth"]
            head, last = txq.state_host()
            assert np.array_equal(last, model.last_array()), f"tick {tick}: last"
            caps = np.zeros(nports * Q, np.int64)
            for p, (nq, dp, _s) in cfg.items():
                caps[p * Q:p * Q + nq] = dp
            assert (head.astype(np.int64) < np.maximum(caps, 1)).all()


def filled(nq=3, depth=4, sched=nf.SCHED_WRR, per_queue=(4, 2, 3), ports=2):
    """Two ports of nq queues; port p's queue q holds per_queue[q] handles (p << 16 | q << 8 | j)."""
    eg = nf.Egress()
    for p in range(ports):
        eg.set_port(p, has_vlan_config=False, num_queues=nq, max_queue_depth=depth)
    eg.commit()
    txq = nf.TxQueues(eg)
    port, queue, handle = [], [], []
    for p in range(ports):
        txq.set_scheduler(p, sched)
        for q, c in enumerate(per_queue):
            for j in range(c):
                port.append(p), queue.append(q), handle.append(p << 16 | q << 8 | j)
    r = eg.enqueue_host(port, queue, np.zeros(ports * Q, np.uint32))
    txq.append_host(r["order"], r["key_start"], r["depth"], len(port), handle=np.array(handle, np.uint64))
    return eg, txq, r["depth"]


def test_tx_cap_rule():
    """A cap inside a port's segment, 0, and exactly the total: earlier ports whole, the crossing port the
    first part of its own sequence, later ports nothing."""
    eg, txq, depth = filled()
    with eg, txq:
        full = txq.dequeue_host(depth, 100, budget_all=100)
        assert full["tx_start"].tolist() == [0, 9, 18]
        assert full["tx_queue"][:9].tolist() == [1, 2, 0, 1, 2, 0, 2, 0, 0]  # queue 1 first: last starts at 0
    for cap in (0, 4, 9, 13, 18):
        eg, txq, depth = filled()
        with eg, txq:
            d = txq.dequeue_host(depth, cap, budget_all=100)
            assert d["tx_start"].tolist() == [0, min(cap, 9), cap]
            assert np.array_equal(d["tx"], full["tx"][:cap]) and np.array_equal(d["tx_queue"], full["tx_queue"][:cap])
            assert int(d["dequeued"].sum()) == cap and int(d["depth"].sum()) == 18 - cap
            rest = txq.dequeue_host(d["depth"], 100, budget_all=100)  # the state went on from where the cap cut
            if cap <= 9:
                assert np.array_equal(rest["tx"][:9 - cap], full["tx"][cap:9])
            assert sorted(np.concatenate([d["tx"], rest["tx"]]).tolist()) == sorted(full["tx"].tolist())


def test_argument_errors():
    L = nf.lib()
    p = ctypes.c_void_p()
    with nf.Egress().set_port(1, num_queues=2, max_queue_depth=3) as eg:
        assert L.nfcs_txq_create(None, eg.ptr, ctypes.byref(p)) == -1 and not p.value  # not committed
        eg.commit()
        assert L.nfcs_txq_create(None, eg.ptr, None) == -1
        assert L.nfcs_txq_create(None, None, ctypes.byref(p)) == -1
        with nf.TxQueues(eg) as txq:
            assert txq.info() == (2, 16, 6)
            assert L.nfcs_txq_set_scheduler(txq.ptr, 2, 0) == -1   # port_id >= ports
            assert L.nfcs_txq_set_scheduler(txq.ptr, 1, 3) == -1   # sched > 2
            assert L.nfcs_txq_set_scheduler(txq.ptr, 1, 2) == 0
            a4 = np.zeros(32, np.uint32)
            a8 = np.zeros(32, np.uint64)
            # device calls on a host-only object
            assert L.nfcs_txq_state_device(txq.ptr, a4.ctypes.data, None, None) == -1
            assert L.nfcs_txq_append_device(None, txq.ptr, a4.ctypes.data, a4.ctypes.data, a4.ctypes.data,
                                            a8.ctypes.data, None, 1, None) == -1
            assert L.nfcs_txq_dequeue_device(None, txq.ptr, None, 1, a4.ctypes.data, a8.ctypes.data, 4, None,
                                             a4.ctypes.data, None, None) == -1
            # both handle sources NULL
            assert L.nfcs_txq_append_host(txq.ptr, a4.ctypes.data, a4.ctypes.data, a4.ctypes.data, None, None, 1) == -1
            assert L.nfcs_txq_append_host(txq.ptr, None, None, None, None, None, 0) == 0  # n == 0
            assert L.nfcs_txq_dequeue_host(txq.ptr, None, 1, a4.ctypes.data, a8.ctypes.data, 4, None, None, None) == -1
    for fn in (L.nfcs_txq_destroy, L.nfcs_txq_reset):
        assert fn(None) == -1
    assert L.nfcs_txq_closed_form_host(3, 2, 0, a4.ctypes.data, 1, a4.ctypes.data, ctypes.byref(ctypes.c_uint32()), None, 0) == -1
    assert L.nfcs_txq_closed_form_host(0, 9, 0, a4.ctypes.data, 1, a4.ctypes.data, ctypes.byref(ctypes.c_uint32()), None, 0) == -1


def test_snapshot_and_reset():
    eg, txq, depth = filled()
    with eg, txq:
        eg.set_port(7, num_queues=8, max_queue_depth=9).commit()  # the txq keeps its snapshot
        assert txq.info() == (2, 16, 24)
        d = txq.dequeue_host(depth, 100, budget_all=2)
        head, last = txq.state_host()
        assert head[:3].tolist() == [0, 1, 1] and last.tolist() == [2, 2]
        txq.reset()
        head, last = txq.state_host()
        assert not head.any() and not last.any()


def test_inconsistent_depths_touch_nothing_out_of_range():
    """depth > cap and depth < cnt append nothing for that key; a depth above the cap is read as the cap by
    the dequeue; entries of order >= n are skipped."""
    eg, txq, depth = filled(nq=2, depth=4, sched=nf.SCHED_STRICT_PRIORITY, per_queue=(2, 2), ports=1)
    with eg, txq:
        before = txq.dequeue_host(depth.copy(), 0)  # nothing taken
        assert int(before["tx_start"][-1]) == 0
        order = np.array([0, 1, 2], np.uint32)
        key_start = np.zeros(Q + 1, np.uint32)
        key_start[1:] = 3  # three packets for key 0
        for bad in (9, 2):  # above the cap of 4; below cnt = 3
            bad_depth = depth.copy()
            bad_depth[0] = bad
            txq.append_host(order, key_start, bad_depth, 3, handle=np.array([91, 92, 93], np.uint64))
        ok_depth = depth.copy()
        ok_depth[0] = 4
        key_start[1:] = 2
        txq.append_host(np.array([5, 1], np.uint32), key_start, ok_depth, 2, handle=np.array([81, 82], np.uint64))
        huge = ok_depth.copy()
        huge[0], huge[1] = 0xFFFFFFFF, 77
        d = txq.dequeue_host(huge, 100, budget_all=100)
        # key 0: its 2 first handles, then slot 2 left as it was (order 5 >= n skipped: still 0), then 82
        assert d["tx"].tolist() == [0, 1, 0, 82, 0x100, 0x101, 0, 0]
        assert d["dequeued"][:2].tolist() == [4, 4] and d["depth"][:2].tolist() == [0xFFFFFFFF - 4, 73]


def test_txq_compile_standalone_under_host_sanitizers(tmp_path):
    """The tables, the append, the literal walk and the closed form as a stand-alone host program (its own
    main, no HIP, nothing loaded into Python) under AddressSanitizer + UBSan, rings and arrays in heap
    blocks of their exact sizes."""
    exe = str(tmp_path / "txq_compile_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "netflow_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "txq_compile_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "txq compile OK" in r.stdout


def test_python_constants_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "nfcs.h")).read()
    m = re.search(r"NFCS_SCHED_STRICT_PRIORITY = (\d+), NFCS_SCHED_WRR = (\d+), NFCS_SCHED_DRR = (\d+)", hdr)
    assert m and [int(x) for x in m.groups()] == [nf.SCHED_STRICT_PRIORITY, nf.SCHED_WRR, nf.SCHED_DRR]
