"""Generate tests/golden/txq_ref.npz from the REFERENCE implementation.

Compiles tests/golden/txq_probe.cpp against the reference's headers in place (plus its
src/netflow++/qos_manager.cpp) into oracle/_ref/txq_probe (git-ignored) and drives the reference's
QosManager through TICKS ticks: in each tick a burst of tagged frames with varied PCPs goes through
enqueue_packet, then every port gets a budget of select_packet_to_dequeue calls. Recorded per tick: what
classify_packet_to_queue says of each frame, every queue's get_queue_stats (packets_enqueued,
packets_dropped_full, packets_dequeued, current_depth) after the burst and after the dequeues, and per port
the sequence numbers of the dequeued frames in order. Every frame carries its sequence number (its index
over all ticks) in bytes 18..21.

Ports: each of the three schedulers with 1, 2, 3, 4 and 8 queues; one port without a QoS config; one never
mentioned (frames leave through it all the same); one with max_queue_depth 1 and two with 5, small enough
to wrap. Budgets: tick 0 is below one round everywhere, tick 1 is 0 everywhere, the rest are drawn from: 0,
below one round, past one round but not a whole number of them (so the port's last-serviced queue matters
to the next tick), above anything queued.

The script checks, against the reference alone: tail drops occur; every budget kind leaves its trace (a
port that dequeues nothing with packets queued, one that empties its queues, one that stops mid-round); at
least one round-robin port's first dequeue comes from queue 1 while queue 0 is non-empty; at least one
queue dequeues more than twice its depth (its ring wraps twice).

    python tests/golden/make_txq_golden.py [reference root, default oracle.REFERENCE_ROOT]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402

PROBE = os.path.join(ROOT, "oracle", "_ref", "txq_probe")
SEED = 20281
TICKS = 14
FRAME_LEN = 24
STRICT, WRR, DRR = range(3)
NONE = 0xFFFFFFFF

# (port id, has a QoS config, num_queues, scheduler, max_queue_depth)
PORTS = [(i, 1, nq, sched, depth)
         for i, (sched, nq, depth) in enumerate((s, nq, d) for s in (STRICT, WRR, DRR)
                                                for nq, d in ((1, 6), (2, 4), (3, 3), (4, 4), (8, 3)))]
PORTS += [
    (15, 0, 4, STRICT, 100),  # no QoS config
    # 16 is never mentioned
    (17, 1, 2, WRR, 1),
    (18, 1, 2, STRICT, 5),
    (19, 1, 3, DRR, 5),
]
DRAW_PORTS = [p[0] for p in PORTS] + [16]
NQ = {p[0]: p[2] for p in PORTS if p[1]}


def build_frame(rng, seq, tagged=True):
    b = bytearray(FRAME_LEN)
    b[0:6] = b"\x02\x00\x00\x00\x00\x01"
    b[6:12] = b"\x02\x00\x00\x00\x00\x02"
    if tagged:
        b[12:14] = b"\x81\x00"
        b[14:16] = ((int(rng.integers(0, 8)) << 13) | 100).to_bytes(2, "big")
        b[16:18] = b"\x88\xb5"
    else:
        b[12:14] = b"\x88\xb5"
    b[18:22] = int(seq).to_bytes(4, "little")
    return bytes(b)


def budget_for(rng, tick, pid):
    nq = NQ.get(pid, 4)
    below = int(rng.integers(1, max(nq, 2)))
    if tick == 0:
        return below
    if tick == 1:
        return 0
    kind = rng.choice(4, p=[0.15, 0.25, 0.35, 0.25])
    return (0, below, nq + int(rng.integers(1, max(nq, 2))), 10000)[int(kind)]


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else oracle.REFERENCE_ROOT
    os.makedirs(os.path.dirname(PROBE), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ref_root, "include"),
                    os.path.join(HERE, "txq_probe.cpp"), os.path.join(ref_root, "src", "netflow++", "qos_manager.cpp"),
                    "-o", PROBE], check=True)
    rng = np.random.default_rng(SEED)
    P = len(PORTS)
    inp = [np.uint32(P).tobytes()]
    for pid, qos, nq, sched, depth in PORTS:
        inp.append(np.uint32(pid).tobytes() + bytes([qos, nq, sched, 0]) + np.uint32(depth).tobytes())
    inp.append(np.uint32(TICKS).tobytes())
    port, frames, tick_start = [], [], [0]
    budget = np.zeros((TICKS, P), np.uint32)
    for t in range(TICKS):
        ports = []
        for pid in DRAW_PORTS:
            ports += [pid] * int(rng.integers(0, 2 * NQ.get(pid, 2) + 5))
        rng.shuffle(ports)
        inp.append(np.uint32(len(ports)).tobytes())
        for pid in ports:
            f = build_frame(rng, len(frames), tagged=rng.random() < 0.93)
            inp.append(np.uint32(pid).tobytes() + np.uint32(len(f)).tobytes() + f)
            port.append(pid)
            frames.append(f)
        tick_start.append(len(frames))
        for i, p in enumerate(PORTS):
            budget[t, i] = budget_for(rng, t, p[0])
        inp.append(budget[t].tobytes())
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.bin")
        subprocess.run([PROBE, path], input=b"".join(inp), stdout=subprocess.DEVNULL, check=True)
        res = open(path, "rb").read()
    pos = 0
    queue = np.zeros(len(frames), np.uint32)
    stats_enq, stats_deq = np.zeros((TICKS, P, 8, 4), np.uint32), np.zeros((TICKS, P, 8, 4), np.uint32)
    deq_start, deq_seq = [0], []
    for t in range(TICKS):
        nf = tick_start[t + 1] - tick_start[t]
        queue[tick_start[t]:tick_start[t + 1]] = np.frombuffer(res, "<u4", nf, pos)
        pos += 4 * nf
        stats_enq[t] = np.frombuffer(res, "<u4", P * 32, pos).reshape(P, 8, 4)
        pos += P * 128
        for _ in range(P):
            c = int(np.frombuffer(res, "<u4", 1, pos)[0])
            deq_seq.append(np.frombuffer(res, "<u4", c, pos + 4))
            pos += 4 + 4 * c
            deq_start.append(deq_start[-1] + c)
        stats_deq[t] = np.frombuffer(res, "<u4", P * 32, pos).reshape(P, 8, 4)
        pos += P * 128
    assert pos == len(res)
    deq_seq = np.concatenate(deq_seq).astype(np.uint32)
    deq_start = np.array(deq_start, np.uint32)

    # ---- what the fixture is meant to hold, read from the reference's results alone
    have = stats_deq[-1, :, :, 0] != NONE
    assert stats_deq[-1][have][:, 1].sum() >= 50, "too few tail drops"
    sched = np.array([p[3] for p in PORTS])
    depth_cap = np.array([p[4] for p in PORTS])
    count = np.diff(deq_start).reshape(TICKS, P)
    queued_before = np.where(stats_enq[:, :, :, 3] == NONE, 0, stats_enq[:, :, :, 3]).sum(axis=2)
    queued_after = np.where(stats_deq[:, :, :, 3] == NONE, 0, stats_deq[:, :, :, 3]).sum(axis=2)
    assert ((count == 0) & (queued_before > 0) & (budget == 0)).any(), "no tick with budget 0 over queued packets"
    assert ((budget > queued_before) & (queued_before > 0) & (queued_after == 0)).any(), "no port emptied"
    nq = np.array([p[2] for p in PORTS])
    assert ((count == budget) & (count % nq != 0) & (sched != STRICT) & (queued_after > 0))[2:].any(), "no mid-round stop"
    first_q1 = False
    for i, p in enumerate(PORTS):
        if p[3] == STRICT or not p[1] or count[0, i] == 0:
            continue
        first = int(deq_seq[deq_start[i]])
        q0_waiting = stats_enq[0, i, 0, 3] > 0
        first_q1 |= bool(queue[first] == 1 and q0_waiting)
    assert first_q1, "no round-robin port starts at queue 1 with queue 0 non-empty"
    wraps = np.where(have, stats_deq[-1, :, :, 2], 0) // depth_cap[:, None]
    assert wraps.max() >= 2, "no ring wraps twice"
    print(f"{len(frames)} frames, {int(stats_deq[-1][have][:, 0].sum())} enqueued, "
          f"{int(stats_deq[-1][have][:, 1].sum())} tail drops, {len(deq_seq)} dequeued, most wraps {int(wraps.max())}")

    out = {"seed": np.uint64(SEED), "ports": np.array(PORTS, np.uint32), "tick_start": np.array(tick_start, np.uint32),
           "port": np.array(port, np.uint32), "frames": np.frombuffer(b"".join(frames), np.uint8).reshape(-1, FRAME_LEN),
           "queue": queue.astype(np.uint8), "budget": budget, "stats_enq": stats_enq, "stats_deq": stats_deq,
           "deq_start": deq_start, "deq_seq": deq_seq}
    path = os.path.join(HERE, "txq_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "egress_ref.npz"))


if __name__ == "__main__":
    main()
