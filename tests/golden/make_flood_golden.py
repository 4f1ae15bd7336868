"""Generate tests/golden/flood_ref.npz from the REFERENCE implementation.

Compiles tests/golden/flood_probe.cpp against the reference's headers in place (plus its
src/netflow++/forwarding_database.cpp, vlan_manager.cpp and qos_manager.cpp) into oracle/_ref/flood_probe
(git-ignored), feeds it an FDB, a port table with VLAN and QoS configurations and a burst of frames, and
records per ingress run what the reference's L2 block does with the burst, floods included: per frame the
verdict, the lookup VLAN and the flood ports; per (port, queue) the queue statistics and the order in which
dequeue_packet returns the packets, each as (source frame, port, length, first 64 bytes after the egress
edit).

The FDB, the L2 side of the ports and the frames' headers are those of make_l2_golden.py (ACCESS / TRUNK /
HYBRID ports, a TRUNK whose native VLAN is not allowed, a port without a VLAN config, link down, STP not
forwarding, port 11 never mentioned). Every port gets an egress side: tag_native set and clear, with and
without a QoS config, 1 to 8 queues, depths small enough to overflow. Behind the headers a frame holds one
repeated byte below 0x40, so that the recorded frames compress and a pop edits nothing but the tag. Runs: ingress 0 (ACCESS, VLAN 10), 3 (TRUNK, native VLAN
1) and 6 (no VLAN config).

The script checks, against the reference's output alone: 20-60% of the frames flood in the ACCESS run;
fan-outs of 0, 1 and >= 4 each occur at least 20 times; at least 20 copies are popped on egress and at least
20 are not; at least one queue holds a flood copy between two unicast packets; at least one tail drop hits a
flood copy; the run whose ingress port lacks a VLAN config floods to no port.

    python tests/golden/make_flood_golden.py [reference root, default oracle.REFERENCE_ROOT]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_l2_golden as l2g  # noqa: E402
import oracle  # noqa: E402

PROBE = os.path.join(ROOT, "oracle", "_ref", "flood_probe")
SEED = 20265
N_FRAMES = 1200
NUM_PORTS = 12
RUNS = (0, 3, 6)
FLOOD, FORWARD = 4, 0
NONE = 0xFFFFFFFF

# the egress side per port id: (tag_native, has a QoS config, num_queues, max_queue_depth)
EGRESS = {
    0: (0, 1, 4, 400),
    1: (0, 1, 4, 400),
    2: (0, 1, 3, 30),
    3: (1, 1, 8, 25),
    4: (0, 0, 4, 100),     # no QoS config: every packet is dropped there
    5: (0, 1, 1, 600),     # HYBRID, tag_native clear: pops its native VLAN
    6: (0, 1, 8, 1000),
    7: (0, 1, 4, 10),
    8: (0, 1, 4, 10),
    9: (0, 1, 2, 1000),
    10: (0, 1, 4, 6),      # shallow: tail drops
}
EGRESS_DTYPE = np.dtype([("port_id", "<u4"), ("has_vlan_config", "u1"), ("type", "u1"), ("tag_native", "u1"),
                         ("has_qos", "u1"), ("native_vlan", "<u2"), ("num_queues", "u1"), ("pad", "u1"),
                         ("max_queue_depth", "<u4")])


def make_frames(rng):
    held = {(m, vlan): port for _, m, vlan, port in l2g.fdb_ops()}
    frames = l2g.make_frames(rng, [(m, v, p) for (m, v), p in held.items()])[:N_FRAMES]
    out = []
    for i, f in enumerate(frames):
        b = bytearray(f)
        head = 18 if f[12:14] == b"\x81\x00" else 14
        for k in range(head, len(b)):
            b[k] = i % 61  # below 0x40: update_checksums(), which ends pop_vlan, takes no such frame for IPv4
        out.append(bytes(b))
    return out


def run_probe(frames):
    ops = l2g.fdb_ops()
    inp = [np.uint32(len(ops)).tobytes()]
    for kind, m, vlan, port in ops:
        inp.append(bytes([kind, 0]) + m + np.uint16(vlan).tobytes() + b"\0\0" + np.uint32(port).tobytes())
    inp.append(np.uint32(len(l2g.PORTS)).tobytes())
    for pid, link, stp, cfg, typ, native, allowed in l2g.PORTS:
        tn, qos, nq, depth = EGRESS[pid]
        inp.append(np.uint32(pid).tobytes() + bytes([link, stp, cfg, typ]) + np.uint16(native).tobytes()
                   + np.uint16(len(allowed)).tobytes() + np.array(allowed, "<u2").tobytes()
                   + (b"\0\0" if len(allowed) & 1 else b"") + bytes([tn, qos, nq, 0]) + np.uint32(depth).tobytes())
    inp.append(np.uint32(NUM_PORTS).tobytes())
    inp.append(np.uint32(len(RUNS)).tobytes() + np.array(RUNS, "<u4").tobytes())
    inp.append(np.uint32(len(frames)).tobytes())
    for f in frames:
        inp.append(np.uint32(len(f)).tobytes() + f)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.bin")
        subprocess.run([PROBE, path], input=b"".join(inp), stdout=subprocess.DEVNULL, check=True)
        res = open(path, "rb").read()
    u32 = lambda pos, c=1: np.frombuffer(res, "<u4", c, pos)  # noqa: E731
    ne = int(u32(0)[0])
    pos = 4
    entries = np.frombuffer(res, np.uint8, ne * 16, pos).reshape(ne, 16).copy()
    pos += ne * 16
    runs = []
    for _ in RUNS:
        nf = len(frames)
        verdict, egress, vlan = np.zeros(nf, np.uint8), np.zeros(nf, np.uint32), np.zeros(nf, np.uint16)
        fstart, fports = [0], []
        for i in range(nf):
            v, e, vl, c = (int(x) for x in u32(pos, 4))
            verdict[i], egress[i], vlan[i] = v, e, vl
            fports.append(u32(pos + 16, c))
            fstart.append(fstart[-1] + c)
            pos += 16 + 4 * c
        stats = u32(pos, NUM_PORTS * 8 * 3).reshape(NUM_PORTS, 8, 3).copy()
        pos += stats.nbytes
        dstart, recs = [0], []
        for _ in range(NUM_PORTS * 8):
            c = int(u32(pos)[0])
            recs.append(np.frombuffer(res, np.uint8, c * 76, pos + 4).reshape(c, 76))
            dstart.append(dstart[-1] + c)
            pos += 4 + 76 * c
        rec = np.concatenate(recs)
        runs.append({"verdict": verdict, "egress": egress, "vlan": vlan, "flood_start": np.array(fstart, np.uint32),
                     "flood_port": np.concatenate(fports).astype(np.uint32), "stats": stats,
                     "deq_start": np.array(dstart, np.uint32),
                     "deq_src": rec[:, 0:4].copy().view("<u4").reshape(-1), "deq_port": rec[:, 4:8].copy().view("<u4").reshape(-1),
                     "deq_len": rec[:, 8:12].copy().view("<u4").reshape(-1), "deq_data": rec[:, 12:76].copy()})
    assert pos == len(res)
    return entries, runs


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else oracle.REFERENCE_ROOT
    os.makedirs(os.path.dirname(PROBE), exist_ok=True)
    src = os.path.join(ref_root, "src", "netflow++")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ref_root, "include"),
                    os.path.join(HERE, "flood_probe.cpp"), os.path.join(src, "forwarding_database.cpp"),
                    os.path.join(src, "vlan_manager.cpp"), os.path.join(src, "qos_manager.cpp"), "-o", PROBE], check=True)
    rng = np.random.default_rng(SEED)
    frames = make_frames(rng)
    entries, runs = run_probe(frames)
    nf = len(frames)
    lens = np.array([len(f) for f in frames], np.uint32)
    data = np.zeros((nf, l2g.FRAME_CAP), np.uint8)
    for i, f in enumerate(frames):
        data[i, :len(f)] = np.frombuffer(f, np.uint8)

    # ---- what the fixture is meant to hold, read from the reference's results alone
    fan_all, popped, kept, interleaved, copy_drops = [], 0, 0, 0, 0
    for r, run in enumerate(runs):
        flood = run["verdict"] == FLOOD
        fan = np.diff(run["flood_start"].astype(np.int64))
        assert (fan[~flood] == 0).all()
        assert ((run["egress"] != NONE) == (run["verdict"] == FORWARD)).all()
        fan_all.append(fan[flood])
        if r == 0:
            assert 0.20 <= flood.mean() <= 0.60, flood.mean()
        if r == 2:
            assert flood.sum() >= 20 and fan.sum() == 0, "an ingress port without a VLAN config floods to no port"
        is_copy = flood[run["deq_src"]]
        short = run["deq_len"] != lens[run["deq_src"]]
        assert (run["deq_len"][short] == lens[run["deq_src"]][short] - 4).all()
        popped += int((is_copy & short).sum())
        kept += int((is_copy & ~short).sum())
        for k in range(NUM_PORTS * 8):
            c = is_copy[int(run["deq_start"][k]):int(run["deq_start"][k + 1])]
            uni = np.flatnonzero(~c)
            if len(uni) >= 2 and c[uni[0]:uni[-1]].any():
                interleaved += 1
        # copies the reference made and did not enqueue at a port that has queues: tail drops
        made = {}
        for i in np.flatnonzero(flood):
            for p in run["flood_port"][int(run["flood_start"][i]):int(run["flood_start"][i + 1])]:
                made[(int(i), int(p))] = True
        got = set(zip(run["deq_src"][is_copy].tolist(), run["deq_port"][is_copy].tolist()))
        copy_drops += sum(1 for (i, p) in made if (i, p) not in got and EGRESS[p][1])
        dropped = np.where(run["stats"][:, :, 0] != NONE, run["stats"][:, :, 1], 0).sum()
        print(f"ingress {RUNS[r]}: flood {flood.mean():.2f}, fan-outs {np.bincount(fan[flood]).tolist()}, "
              f"dequeued {len(run['deq_src'])}, tail drops {int(dropped)}")
    fan_all = np.concatenate(fan_all)
    for name, m in (("0", fan_all == 0), ("1", fan_all == 1), (">= 4", fan_all >= 4)):
        assert m.sum() >= 20, (name, int(m.sum()))
    assert popped >= 20 and kept >= 20, (popped, kept)
    assert interleaved >= 1, "no queue holds a copy between two unicast packets"
    assert copy_drops >= 1, "no tail drop hits a flood copy"
    assert {13, 14, 17, 18, 64} <= set(int(x) for x in lens)
    print(f"copies popped {popped}, not popped {kept}, interleaved queues {interleaved}, copies tail-dropped {copy_drops}")

    ports = np.zeros(len(l2g.PORTS), dtype=[("port_id", "<u4"), ("link_up", "u1"), ("stp_forwarding", "u1"),
                                            ("has_vlan_config", "u1"), ("type", "u1"), ("native_vlan", "<u2"),
                                            ("pad", "<u2")])
    eports = np.zeros(len(l2g.PORTS), EGRESS_DTYPE)
    allowed = np.full((len(l2g.PORTS), 8), 0xFFFF, np.uint16)
    allowed_n = np.zeros(len(l2g.PORTS), np.uint32)
    for i, (pid, link, stp, cfg, typ, native, al) in enumerate(l2g.PORTS):
        tn, qos, nq, depth = EGRESS[pid]
        ports[i] = (pid, link, stp, cfg, typ, native, 0)
        eports[i] = (pid, cfg, typ, tn, qos, native, nq, 0, depth)
        allowed[i, :len(al)] = al
        allowed_n[i] = len(al)
    out = {"seed": np.uint64(SEED), "lens": lens, "frames": data, "entries": entries,
           "ports": np.frombuffer(ports.tobytes(), np.uint8).reshape(len(ports), 12).copy(),
           "egress_ports": np.frombuffer(eports.tobytes(), np.uint8).reshape(len(eports), 16).copy(),
           "allowed": allowed, "allowed_n": allowed_n, "num_ports": np.uint32(NUM_PORTS),
           "ingress": np.array(RUNS, np.uint32)}
    for r, run in enumerate(runs):
        for k, v in run.items():
            out[f"{k}_{r}"] = v
    path = os.path.join(HERE, "flood_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
