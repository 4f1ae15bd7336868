#!/usr/bin/env python3
"""Times the TX queues (nfcs_txq_append_device, nfcs_txq_dequeue_device) against the egress enqueue of the
same burst in the same run. Prints one JSON line.

    python tools/txq_bench.py [--steps 20] [--rounds 3] [--out profiles/txq_bench.json]

Per burst size (64K and 1M packets) and key distribution (the egress bench's: every packet on one key, 48
ports x 4 queues, 1,024 ports x 8 queues, uniform) the queues have room for the whole burst. The timed calls
rotate over `--states` separate TX queue objects, each with its own rings, depth array and enqueue outputs,
so no call finds its rings or its order list in the caches from the call before. Variants are timed
interleaved in one process, `rounds` times; each figure is the median over the rounds of (HIP-event ms over
`steps` calls) / steps, with the minimum beside it.

Variants:
  enqueue          nfcs_egress_enqueue_device from zeroed depths (the yardstick; the depths are copied from a
                   zeroed array on the stream before every call, inside the timed region, as in egress_bench)
  append           nfcs_txq_append_device of the burst the enqueue left (it only reads head and depth, so the
                   same call repeats on the same state)
  dequeue_all      nfcs_txq_dequeue_device with a budget above everything queued: every packet of the burst
                   leaves, round-robin on the odd ports and strict priority on the even ones (the depths are
                   copied back from the enqueue's on the stream before every call, inside the timed region)
  dequeue_64       the same with a budget of 64 per port: a TX tick that takes a slice
  append_dequeue   append and dequeue_all back to back
`x` is the variant's time over the enqueue's in the same run.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import netflow_amd as nf  # noqa: E402

DISTS = {"one_key": (1, 1), "48x4": (48, 4), "1024x8": (1024, 8)}


def event_ms(eng, step, steps: int) -> float:
    import torch
    st = torch.cuda.ExternalStream(eng.stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(steps):
        step()
    e1.record(st)
    e1.synchronize()
    return float(e0.elapsed_time(e1))


def med_min(xs):
    return {"ms": round(statistics.median(xs), 5), "ms_min": round(min(xs), 5)}


class State:
    """One TX queue object with everything a call touches."""

    def __init__(self, eng, eg, n, keys, ports, port, queue, rng):
        import torch
        self.txq = nf.TxQueues(eg, eng)
        for p in range(1, ports, 2):
            self.txq.set_scheduler(p, nf.SCHED_WRR)
        self.d_port, self.d_queue = eng.alloc(4 * n).upload(port), eng.alloc(n).upload(queue)
        self.d_handle = eng.alloc(8 * n).upload(rng.integers(1, 1 << 63, n, dtype=np.uint64))
        self.d_order, self.d_ks = eng.alloc(4 * n), eng.alloc(4 * (keys + 1))
        self.depth = torch.zeros(keys, dtype=torch.int32, device="cuda")
        self.full = torch.zeros(keys, dtype=torch.int32, device="cuda")
        self.d_tx, self.d_txq = eng.alloc(8 * n), eng.alloc(n)
        self.d_start, self.d_deq = eng.alloc(4 * (ports + 1)), eng.alloc(4 * keys)


def run_size(eng, n: int, steps: int, rounds: int, warmup: int, nstates: int):
    import torch
    st = torch.cuda.ExternalStream(eng.stream)
    out = {"packets": n, "states_rotated": nstates}
    rng = np.random.default_rng(n)
    for dname, (ports, queues) in DISTS.items():
        with nf.Egress() as eg:
            for p in range(ports):
                eg.set_port(p, has_vlan_config=False, num_queues=queues, max_queue_depth=2 * n // (ports * queues) + 64)
            eg.commit().upload(eng)
            keys = eg.keys()[1]
            zero = torch.zeros(keys, dtype=torch.int32, device="cuda")
            states = [State(eng, eg, n, keys, ports, rng.integers(0, ports, n).astype(np.uint32),
                            rng.integers(0, queues, n).astype(np.uint8), rng) for _ in range(nstates)]
            ctr = [0]

            def nxt():
                ctr[0] += 1
                return states[ctr[0] % nstates]

            def enqueue(s=None):
                s = s or nxt()
                with torch.cuda.stream(st):
                    s.depth.copy_(zero, non_blocking=True)
                eng.egress_enqueue_device(eg, s.d_port, s.d_queue, n, s.depth.data_ptr(), s.d_order, s.d_ks)

            def append(s=None):
                s = s or nxt()
                eng.txq_append_device(s.txq, s.d_order, s.d_ks, s.depth.data_ptr(), n, handle=s.d_handle)

            def dequeue(budget, s=None):
                s = s or nxt()
                with torch.cuda.stream(st):
                    s.depth.copy_(s.full, non_blocking=True)
                eng.txq_dequeue_device(s.txq, s.depth.data_ptr(), s.d_tx, n, s.d_start, budget_all=budget,
                                       tx_queue=s.d_txq, dequeued=s.d_deq)

            def both():
                s = nxt()
                with torch.cuda.stream(st):
                    s.depth.copy_(s.full, non_blocking=True)
                append(s)
                eng.txq_dequeue_device(s.txq, s.depth.data_ptr(), s.d_tx, n, s.d_start, budget_all=0xFFFFFFFF,
                                       tx_queue=s.d_txq, dequeued=s.d_deq)

            for s in states:  # the state every variant starts from: the burst enqueued and appended
                enqueue(s)
                append(s)
                with torch.cuda.stream(st):
                    s.full.copy_(s.depth, non_blocking=True)
            eng.sync()
            variants = {"enqueue": enqueue, "append": append, "dequeue_all": lambda: dequeue(0xFFFFFFFF),
                        "dequeue_64": lambda: dequeue(64), "append_dequeue": both}
            times = {k: [] for k in variants}
            for k, step in variants.items():
                for _ in range(warmup):
                    step()
                if k == "enqueue":  # the enqueue left the depths the other variants read
                    eng.sync()
            eng.sync()
            for _ in range(rounds):
                for k, step in variants.items():
                    times[k].append(event_ms(eng, step, steps) / steps)
            res = {"ports": ports, "queues": queues, "keys": keys}
            for k, xs in times.items():
                res[k] = med_min(xs)
                res[k]["gpkt_s"] = round(n / (res[k]["ms"] * 1e-3) / 1e9, 2)
                res[k]["x"] = round(res[k]["ms"] / statistics.median(times["enqueue"]), 3)
            dequeue(0xFFFFFFFF, states[0])
            eng.sync()
            res["dequeued_all"] = int(states[0].d_start.download(np.uint32, ports + 1)[ports])
            out[dname] = res
            for s in states:
                s.txq.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--states", type=int, default=4)
    ap.add_argument("--packets", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # the events and the depth arrays are torch's, on the runtime the engine shares
    torch.cuda.init()
    with nf.Engine(0) as eng:
        res = {"tool": "tools/txq_bench.py", "steps": args.steps, "rounds": args.rounds,
               "timing": "HIP events on the engine's stream around the rotated calls; median (and min) over rounds",
               "x_is": "the variant's ms over the enqueue's ms in the same run"}
        for n in args.packets:
            res[f"n{n}"] = run_size(eng, n, args.steps, args.rounds, args.warmup, args.states)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
