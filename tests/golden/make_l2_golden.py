"""Generate tests/golden/l2_ref.npz from the REFERENCE implementation.

Compiles tests/golden/l2_probe.cpp against the reference's headers in place (plus its
src/netflow++/forwarding_database.cpp and vlan_manager.cpp) into oracle/_ref/l2_probe (git-ignored),
feeds it an FDB build, a port configuration and a list of frames, and records what the reference
decides per frame: the entries as get_all_entries() returns them and, per frame and ingress port, the
verdict of the L2 block (switch.hpp:305-326), the egress port, the VLAN used for the lookup and the
class of what learn_mac(src_mac, ingress, vlan) does; per (ingress, VLAN) the ports flood_packet sends to.

The FDB is built through learn_mac and add_static_entry and includes a dynamic entry moved by a second
learn_mac, a static entry that a learn_mac does not move, the all-zero MAC on VLAN 0 and one MAC on two
VLANs. Ports: two ACCESS ports on VLAN 10 (and a spare), ACCESS on VLAN 20, TRUNK with and without its
native VLAN allowed, HYBRID, one port without a VLAN config, one link-down port, one port not
STP-forwarding; port 11 is never mentioned. Three runs over the same frames: ingress = an ACCESS port
(0), a TRUNK port (3) and the unconfigured port (6).

The script checks, against the reference alone: every verdict of the block occurs at least 20 times in
some run; FORWARD and FLOOD each make up 10-60% of the ACCESS run; every learn class occurs at least 20
times; no verdict exceeds 60% in any run.

    python tests/golden/make_l2_golden.py [reference root, default oracle.REFERENCE_ROOT]
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402

PROBE = os.path.join(ROOT, "oracle", "_ref", "l2_probe")
SEED = 20263
FRAME_CAP = 64  # no frame is longer (the decision reads no byte past 15)
FORWARD, NO_ETH, FLOOD, SAME_PORT, LINK_DOWN, STP, VLAN = 0, 3, 4, 5, 6, 7, 8
LEARN_NONE, LEARN_NEW, LEARN_REFRESH, LEARN_MOVED = range(4)
ACCESS, TRUNK, HYBRID = range(3)
NONE = 0xFFFFFFFF
NUM_PORTS = 12
RUNS = (0, 3, 6)  # ACCESS on VLAN 10, TRUNK (native 1), no VLAN config
FLOOD_VLANS = (0, 1, 10, 20, 30, 40, 50, 99)

# (port id, link up, STP forwarding, has a VLAN config, type, native VLAN, allowed VLANs)
PORTS = [
    (0, 1, 1, 1, ACCESS, 10, ()),
    (1, 1, 1, 1, ACCESS, 10, (20, 30)),           # an ACCESS port's set is ignored (configure_port clears it)
    (2, 1, 1, 1, ACCESS, 20, ()),
    (3, 1, 1, 1, TRUNK, 1, (1, 10, 20, 30)),      # native VLAN allowed
    (4, 1, 1, 1, TRUNK, 99, (10, 20)),            # native VLAN not allowed
    (5, 1, 1, 1, HYBRID, 10, (10, 30)),
    (6, 1, 1, 0, ACCESS, 1, ()),                  # no VLAN config
    (7, 0, 1, 1, ACCESS, 10, ()),                 # link down
    (8, 1, 0, 1, ACCESS, 10, ()),                 # not STP-forwarding
    (9, 1, 1, 1, TRUNK, 1, (1, 10, 40)),
    (10, 1, 1, 1, ACCESS, 10, ()),
]


def mac(k):
    return bytes([0x02, 0xFD, 0, 0, k >> 8, k & 0xFF])


ZERO_MAC, BCAST = bytes(6), b"\xff" * 6


def fdb_ops():
    """(kind, mac, vlan, port): kind 0 learn_mac, 1 add_static_entry."""
    ops = []
    for k in range(40):   # VLAN 10 over every kind of port; every fourth entry static
        ops.append((1 if k % 4 == 0 else 0, mac(k), 10, (0, 1, 5, 7, 8, 10, 3, 9, 2, 6)[k % 10]))
    for k in range(40, 60):  # VLAN 20
        ops.append((1 if k % 4 == 0 else 0, mac(k), 20, (2, 3, 4, 0, 7)[k % 5]))
    for k in range(60, 80):  # VLAN 1, the TRUNKs' native VLAN and the default without a config
        ops.append((1 if k % 4 == 0 else 0, mac(k), 1, (3, 9, 6, 0, 8)[k % 5]))
    for k in range(80, 90):  # VLAN 30
        ops.append((0, mac(k), 30, (3, 5)[k % 2]))
    ops.append((0, mac(0), 20, 2))            # one MAC on two VLANs (VLAN 10 above, port 0)
    ops.append((1, ZERO_MAC, 0, 1))           # the all-zero MAC on VLAN 0
    ops.append((0, mac(90), 10, 1))
    ops.append((0, mac(90), 10, 5))           # a dynamic entry moved by a second learn_mac
    ops.append((1, mac(91), 10, 1))
    ops.append((0, mac(91), 10, 5))           # a static entry that a learn_mac does not move
    return ops


def build_frame(rng, dmac, smac, vlan, length):
    """vlan None = untagged."""
    b = bytearray(rng.integers(0, 256, size=FRAME_CAP, dtype=np.uint8).tobytes())
    b[0:6], b[6:12] = dmac, smac
    if vlan is not None:
        b[12:14] = b"\x81\x00"
        b[14:16] = ((int(rng.integers(0, 8)) << 13) | vlan).to_bytes(2, "big")
        b[16:18] = b"\x86\xdd"
    else:
        b[12:14] = (b"\x86\xdd", b"\x88\xb5", b"\x08\x00")[int(rng.integers(0, 3))]
    return bytes(b[:length])


def make_frames(rng, entries):
    """entries: the (mac, vlan, port) the FDB holds. Most destinations and sources are drawn from them
    together with a VLAN that makes them hit under at least one run: the entry's VLAN as a tag, or no tag
    when it is a run's native VLAN (10 for the ACCESS run, 1 for the other two)."""
    frames = []
    absent = [mac(k) for k in range(200, 230)]

    def draw(p_entry):
        if rng.random() < p_entry:
            m, v, _ = entries[int(rng.integers(0, len(entries)))]
            return m, v
        return absent[int(rng.integers(0, len(absent)))], None

    for _ in range(1500):
        dmac, dv = draw(0.85)
        if rng.random() < 0.07:
            dmac, dv = BCAST, None
        smac, sv = draw(0.75)
        want = dv if (dv is not None and rng.random() < 0.85) else sv
        if want is None or rng.random() < 0.05:
            want = int(rng.choice([10, 20, 30, 40, 1, 0, 50]))
        # an untagged frame means VLAN 10 on the ACCESS run and 1 on the others
        vlan = None if (want in (1, 10) and rng.random() < 0.45) else want
        length = int(rng.choice([13, 14, 17, 18, 64], p=[0.03, 0.05, 0.05, 0.07, 0.80]))
        frames.append(build_frame(rng, dmac, smac, vlan, length))
    return frames


def run_probe(ops, frames):
    inp = [np.uint32(len(ops)).tobytes()]
    for kind, m, vlan, port in ops:
        inp.append(bytes([kind, 0]) + m + np.uint16(vlan).tobytes() + b"\0\0" + np.uint32(port).tobytes())
    inp.append(np.uint32(len(PORTS)).tobytes())
    for pid, link, stp, cfg, typ, native, allowed in PORTS:
        inp.append(np.uint32(pid).tobytes() + bytes([link, stp, cfg, typ]) + np.uint16(native).tobytes()
                   + np.uint16(len(allowed)).tobytes() + np.array(allowed, "<u2").tobytes()
                   + (b"\0\0" if len(allowed) & 1 else b""))
    inp.append(np.uint32(NUM_PORTS).tobytes())
    inp.append(np.uint32(len(RUNS)).tobytes() + np.array(RUNS, "<u4").tobytes())
    inp.append(np.uint32(len(FLOOD_VLANS)).tobytes() + np.array(FLOOD_VLANS, "<u2").tobytes()
               + (b"\0\0" if len(FLOOD_VLANS) & 1 else b""))
    inp.append(np.uint32(len(frames)).tobytes())
    for f in frames:
        inp.append(np.uint32(len(f)).tobytes() + f)
    res = subprocess.run([PROBE], input=b"".join(inp), stdout=subprocess.PIPE, check=True).stdout
    ne = int(np.frombuffer(res, "<u4", 1)[0])
    pos = 4
    entries = np.frombuffer(res, np.uint8, ne * 16, pos).reshape(ne, 16).copy()
    pos += ne * 16
    nf = len(frames)
    rec = np.frombuffer(res, "<u4", len(RUNS) * nf * 4, pos).reshape(len(RUNS), nf, 4).copy()
    pos += rec.nbytes
    flood_n = np.zeros((len(RUNS), len(FLOOD_VLANS)), np.uint32)
    flood = np.full((len(RUNS), len(FLOOD_VLANS), NUM_PORTS), NONE, np.uint32)
    for r in range(len(RUNS)):
        for k in range(len(FLOOD_VLANS)):
            c = int(np.frombuffer(res, "<u4", 1, pos)[0])
            flood_n[r, k] = c
            flood[r, k, :c] = np.frombuffer(res, "<u4", c, pos + 4)
            pos += 4 + 4 * c
    assert pos == len(res)
    return entries, rec, flood_n, flood


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else oracle.REFERENCE_ROOT
    os.makedirs(os.path.dirname(PROBE), exist_ok=True)
    src = os.path.join(ref_root, "src", "netflow++")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ref_root, "include"),
                    os.path.join(HERE, "l2_probe.cpp"), os.path.join(src, "forwarding_database.cpp"),
                    os.path.join(src, "vlan_manager.cpp"), "-o", PROBE], check=True)
    rng = np.random.default_rng(SEED)
    ops = fdb_ops()
    # the keys the FDB holds after the build, here only to draw frames that hit
    held = {(m, vlan): port for _, m, vlan, port in ops}
    frames = make_frames(rng, [(m, v, p) for (m, v), p in held.items()])
    assert max(len(f) for f in frames) <= FRAME_CAP
    entries, rec, flood_n, flood = run_probe(ops, frames)
    # the build did what the fixture is meant to hold (read from the reference's entries alone)
    by_key = {(bytes(e[:6]), int(e[6]) | int(e[7]) << 8): (int.from_bytes(bytes(e[8:12]), "little"), int(e[12]))
              for e in entries}
    assert len(by_key) == len(entries) == len(held)
    assert by_key[(mac(90), 10)] == (5, 0)         # moved by the second learn_mac
    assert by_key[(mac(91), 10)] == (1, 1)         # static: the learn_mac left it
    assert (ZERO_MAC, 0) in by_key and (mac(0), 10) in by_key and (mac(0), 20) in by_key
    lens = np.array([len(f) for f in frames], dtype=np.uint32)
    data = np.zeros((len(frames), FRAME_CAP), dtype=np.uint8)
    for i, f in enumerate(frames):
        data[i, :len(f)] = np.frombuffer(f, dtype=np.uint8)
    ports = np.zeros(len(PORTS), dtype=[("port_id", "<u4"), ("link_up", "u1"), ("stp_forwarding", "u1"),
                                        ("has_vlan_config", "u1"), ("type", "u1"), ("native_vlan", "<u2"),
                                        ("pad", "<u2")])
    allowed = np.full((len(PORTS), 8), 0xFFFF, np.uint16)
    allowed_n = np.zeros(len(PORTS), np.uint32)
    for i, (pid, link, stp, cfg, typ, native, al) in enumerate(PORTS):
        ports[i] = (pid, link, stp, cfg, typ, native, 0)
        allowed[i, :len(al)] = al
        allowed_n[i] = len(al)
    out = {"seed": np.uint64(SEED), "lens": lens, "frames": data, "entries": entries,
           "ports": np.frombuffer(ports.tobytes(), np.uint8).reshape(len(PORTS), 12).copy(),
           "allowed": allowed, "allowed_n": allowed_n, "num_ports": np.uint32(NUM_PORTS),
           "ingress": np.array(RUNS, np.uint32), "flood_vlans": np.array(FLOOD_VLANS, np.uint32),
           "flood_n": flood_n, "flood_ports": flood}
    best = {v: 0 for v in (FORWARD, NO_ETH, FLOOD, SAME_PORT, LINK_DOWN, STP, VLAN)}
    learn_best = {c: 0 for c in range(4)}
    for r, ingress in enumerate(RUNS):
        verdict, egress, vlan, learn = (rec[r, :, k] for k in range(4))
        counts = np.bincount(verdict, minlength=9)
        assert counts[1] == 0 and counts[2] == 0
        assert counts.max() <= 0.60 * len(frames), (ingress, counts)
        for v in best:
            best[v] = max(best[v], int(counts[v]))
        decided = verdict != NO_ETH
        for c in learn_best:
            learn_best[c] = max(learn_best[c], int(((learn == c) & decided).sum()))
        assert ((egress != NONE) == (verdict == FORWARD)).all()
        assert (verdict == NO_ETH).sum() == (lens < 14).sum() and (vlan[~decided] == 0).all()
        if r == 0:
            for v in (FORWARD, FLOOD):
                assert 0.10 <= counts[v] / len(frames) <= 0.60, (v, counts)
        out[f"verdict_{r}"], out[f"egress_{r}"] = verdict.astype(np.uint8), egress.copy()
        out[f"vlan_{r}"], out[f"learn_{r}"] = vlan.astype(np.uint16), learn.astype(np.uint8)
        print(f"ingress {ingress}: verdicts " + " ".join(f"{v}:{c}" for v, c in enumerate(counts))
              + "; learn " + " ".join(str(int(((learn == c) & decided).sum())) for c in range(4)))
    assert min(best.values()) >= 20, best
    assert min(learn_best.values()) >= 20, learn_best
    assert {13, 14, 17, 18, 64} <= set(int(x) for x in lens)
    assert flood_n.max() >= 4 and (flood_n[2] == 0).all()  # without a config on the ingress port nothing floods
    print("flood ports per (ingress, VLAN):", flood_n.tolist())
    path = os.path.join(HERE, "l2_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
