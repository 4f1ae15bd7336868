"""Generate tests/golden/egress_ref.npz from the REFERENCE implementation.

Compiles tests/golden/egress_probe.cpp against the reference's headers in place (plus its
src/netflow++/vlan_manager.cpp and qos_manager.cpp) into oracle/_ref/egress_probe (git-ignored), feeds it a
port configuration, a warm-up list and a burst of frames with an egress port each, and records what the
reference does with the burst: per frame the bytes and the length after VlanManager::process_egress and
what QosManager::classify_packet_to_queue says of the edited frame; per (port, queue) get_queue_stats
before and after the burst and the order in which dequeue_packet returns the frames.

Ports: ACCESS; TRUNK with tag_native set and clear; HYBRID with tag_native clear and set; one port without
a VLAN config; one without a QoS config; num_queues 1, 2, 3, 4 and 8; one port configured with num_queues 0
and max_queue_depth 0 (the reference reads each as 1); depths small enough to overflow; port 8 is never
mentioned and frames leave through it all the same. Port 11 receives exactly as many frames as its one
queue has room for. Frames: untagged, tagged with the port's native VLAN, tagged with another VLAN,
double-tagged; lengths 13, 14, 17, 18, 21, 22 and 64; every PCP. Every frame carries its index in bytes
0..3; warm-up frames have bit 31 of it set.

The script checks, against the reference alone: pops are 10-60% of the frames; every queue id 0..7
occurs; each of ENQUEUED, DROP_NO_CONFIG and DROP_FULL (the classes the reference can produce) occurs at
least 20 times; tail drops are 5-40% of the frames, over at least two queues; at least one queue ends
exactly at its depth without a drop; at least one queue starts at its depth.

    python tests/golden/make_egress_golden.py [reference root, default oracle.REFERENCE_ROOT]
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

PROBE = os.path.join(ROOT, "oracle", "_ref", "egress_probe")
SEED = 20264
FRAME_CAP = 64
ACCESS, TRUNK, HYBRID = range(3)
WARM = 0x80000000
N_FRAMES = 1200
EXACT_PORT, EXACT_WARM, EXACT_BURST = 11, 3, 17  # port 11: depth 20 = 3 warm-up frames + 17 of the burst

# (port id, has a VLAN config, type, tag_native, has a QoS config, native VLAN, num_queues, max_queue_depth)
PORTS = [
    (0, 1, ACCESS, 0, 1, 10, 4, 40),
    (1, 1, TRUNK, 1, 1, 10, 8, 12),
    (2, 1, TRUNK, 0, 1, 20, 3, 30),
    (3, 1, HYBRID, 0, 1, 10, 1, 60),
    (4, 0, ACCESS, 0, 1, 1, 8, 1000),     # no VLAN config
    (5, 1, ACCESS, 0, 0, 20, 4, 1000),    # no QoS config
    (6, 1, ACCESS, 0, 1, 10, 4, 5),       # the warm-up fills its queues
    (7, 1, HYBRID, 1, 1, 30, 2, 25),
    (9, 1, ACCESS, 1, 1, 30, 8, 1000),    # tag_native on an ACCESS port changes nothing
    (10, 1, ACCESS, 0, 1, 10, 0, 0),      # validate_and_prepare: one queue of depth one
    (EXACT_PORT, 1, TRUNK, 1, 1, 99, 1, EXACT_WARM + EXACT_BURST),
]
PORT_DTYPE = np.dtype([("port_id", "<u4"), ("has_vlan_config", "u1"), ("type", "u1"), ("tag_native", "u1"),
                       ("has_qos", "u1"), ("native_vlan", "<u2"), ("num_queues", "u1"), ("pad", "u1"),
                       ("max_queue_depth", "<u4")])
NATIVE = {p[0]: p[5] for p in PORTS}
DRAW_PORTS = [p[0] for p in PORTS if p[0] != EXACT_PORT] + [8]  # 8: never configured


def tag(rng, vlan):
    return b"\x81\x00" + ((int(rng.integers(0, 8)) << 13) | (int(rng.integers(0, 2)) << 12) | vlan).to_bytes(2, "big")


def build_frame(rng, index, port, length):
    b = bytearray(rng.integers(0, 256, size=FRAME_CAP, dtype=np.uint8).tobytes())
    b[0:4] = int(index).to_bytes(4, "little")
    native = NATIVE.get(port, 1)
    other = int(rng.choice([v for v in (1, 10, 20, 30, 40, 0) if v != native]))
    kind = rng.choice(5, p=[0.22, 0.36, 0.20, 0.16, 0.06])
    inner = (b"\x86\xdd", b"\x88\xb5", b"\x08\x00")[int(rng.integers(0, 3))]
    # pop_vlan ends in update_checksums(), which takes any frame whose byte behind the EtherType has the
    # version nibble 4 for IPv4, whatever the EtherType says. An IHL that reaches past the frame makes the
    # reference read past its data (undefined, NFCS_ST_OOB: outside the parity domain), so such a byte gets
    # an IHL of 5..10, which fits every 64-byte frame here; the IPv4 EtherType always gets one.
    ver = int(rng.integers(0, 256))
    if inner == b"\x08\x00" or ver >> 4 == 4:
        ver = 0x40 | int(rng.integers(5, 11))
    inner += bytes([ver])
    if kind == 0:
        h = inner
    elif kind == 1:
        h = tag(rng, native) + inner
    elif kind == 2:
        h = tag(rng, other) + inner
    elif kind == 3:
        h = tag(rng, native) + tag(rng, other) + inner
    else:
        h = tag(rng, other) + tag(rng, native) + inner
    b[12:12 + len(h)] = h
    return bytes(b[:length])


def make_list(rng, n, flag, exact):
    """n frames on random ports, then `exact` more on EXACT_PORT mixed in at random places."""
    ports = [int(rng.choice(DRAW_PORTS)) for _ in range(n - exact)] + [EXACT_PORT] * exact
    rng.shuffle(ports)
    out = []
    for i, port in enumerate(ports):
        if flag and rng.random() < 0.5:
            port = 6 if port != EXACT_PORT else port  # the warm-up leans on port 6: its queues start full
        length = int(rng.choice([13, 14, 17, 18, 21, 22, 64], p=[0.03, 0.04, 0.04, 0.05, 0.05, 0.05, 0.74]))
        out.append((port, build_frame(rng, i | flag, port, length)))
    return out


def run_probe(warm, frames):
    recs = np.zeros(len(PORTS), PORT_DTYPE)
    for i, (pid, cfg, typ, tn, qos, native, nq, depth) in enumerate(PORTS):
        recs[i] = (pid, cfg, typ, tn, qos, native, nq, 0, depth)
    inp = [np.uint32(len(PORTS)).tobytes(), recs.tobytes()]
    for lst in (warm, frames):
        inp.append(np.uint32(len(lst)).tobytes())
        for port, f in lst:
            inp.append(np.uint32(port).tobytes() + np.uint32(len(f)).tobytes() + f)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.bin")
        subprocess.run([PROBE, path], input=b"".join(inp), stdout=subprocess.DEVNULL, check=True)
        res = open(path, "rb").read()
    P, nf, pos = len(PORTS), len(frames), 0
    before = np.frombuffer(res, "<u4", P * 8 * 3, pos).reshape(P, 8, 3).copy()
    pos += before.nbytes
    rec = np.frombuffer(res, np.uint8, nf * 72, pos).reshape(nf, 72).copy()
    pos += rec.nbytes
    after = np.frombuffer(res, "<u4", P * 8 * 3, pos).reshape(P, 8, 3).copy()
    pos += after.nbytes
    start, idx = [0], []
    for _ in range(P * 8):
        c = int(np.frombuffer(res, "<u4", 1, pos)[0])
        idx.append(np.frombuffer(res, "<u4", c, pos + 4))
        pos += 4 + 4 * c
        start.append(start[-1] + c)
    assert pos == len(res)
    return recs, before, rec, after, np.array(start, np.uint32), np.concatenate(idx).astype(np.uint32)


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else oracle.REFERENCE_ROOT
    os.makedirs(os.path.dirname(PROBE), exist_ok=True)
    src = os.path.join(ref_root, "src", "netflow++")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ref_root, "include"),
                    os.path.join(HERE, "egress_probe.cpp"), os.path.join(src, "vlan_manager.cpp"),
                    os.path.join(src, "qos_manager.cpp"), "-o", PROBE], check=True)
    rng = np.random.default_rng(SEED)
    warm = make_list(rng, 70, WARM, EXACT_WARM)
    frames = make_list(rng, N_FRAMES, 0, EXACT_BURST)
    recs, before, rec, after, q_start, q_idx = run_probe(warm, frames)
    nf = len(frames)
    lens_in = np.array([len(f) for _, f in frames], np.uint32)
    port = np.array([p for p, _ in frames], np.uint32)
    data_in = np.zeros((nf, FRAME_CAP), np.uint8)
    for i, (_, f) in enumerate(frames):
        data_in[i, :len(f)] = np.frombuffer(f, np.uint8)
    lens_out = rec[:, 0:4].copy().view("<u4").reshape(nf)
    data_out = rec[:, 4:68].copy()
    queue = rec[:, 68:72].copy().view("<u4").reshape(nf)

    # ---- what the fixture is meant to hold, read from the reference's results alone
    NONE = 0xFFFFFFFF
    popped = lens_out != lens_in
    assert (lens_out[popped] == lens_in[popped] - 4).all()
    assert 0.10 <= popped.mean() <= 0.60, popped.mean()
    has_qos = {int(r["port_id"]): bool(r["has_qos"]) for r in recs}
    enqueued = np.zeros(nf, bool)
    enqueued[q_idx[(q_idx & WARM) == 0]] = True
    no_cfg = np.array([not has_qos.get(int(p), False) for p in port])
    full = ~enqueued & ~no_cfg
    assert not (enqueued & no_cfg).any()
    assert set(int(q) for q in queue[~no_cfg]) == set(range(8))
    for name, m in (("ENQUEUED", enqueued), ("DROP_NO_CONFIG", no_cfg), ("DROP_FULL", full)):
        assert m.sum() >= 20, (name, int(m.sum()))
    assert 0.05 <= full.mean() <= 0.40, full.mean()
    have = before[:, :, 0] != NONE
    assert (have == (after[:, :, 0] != NONE)).all()
    dropped = np.where(have, after[:, :, 1] - before[:, :, 1], 0)
    grown = np.where(have, after[:, :, 0] - before[:, :, 0], 0)
    assert dropped.sum() == full.sum() and (dropped > 0).sum() >= 2
    assert grown.sum() == enqueued.sum()
    depth_cap = np.array([max(int(r["max_queue_depth"]), 1) for r in recs])[:, None]
    exact = have & (after[:, :, 2] == depth_cap) & (dropped == 0) & (grown > 0)
    assert exact.any(), "no queue ends exactly at its depth without a drop"
    assert (have & (before[:, :, 2] >= depth_cap)).any(), "no queue starts at its depth"
    assert {13, 14, 17, 18, 21, 22, 64} <= set(int(x) for x in lens_in)
    print(f"pops {popped.mean():.2f}, enqueued {int(enqueued.sum())}, no config {int(no_cfg.sum())}, "
          f"tail drops {int(full.sum())} over {int((dropped > 0).sum())} queues, exact-fit queues {int(exact.sum())}")

    out = {"seed": np.uint64(SEED), "ports": np.frombuffer(recs.tobytes(), np.uint8).reshape(len(PORTS), 16).copy(),
           "port": port, "lens_in": lens_in, "frames_in": data_in, "lens_out": lens_out, "frames_out": data_out,
           "queue": queue.astype(np.uint8), "stats_before": before, "stats_after": after,
           "deq_start": q_start, "deq_index": q_idx}
    path = os.path.join(HERE, "egress_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
