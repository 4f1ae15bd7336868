#!/usr/bin/env python3
"""Times flood replication (nfcs_flood_expand_device) against two yardsticks timed in the same run: the
flow-key kernel (hashes only: one header line per frame), the comparison at 0% floods, where the call only
reads descriptors and small arrays; and a device-to-device hipMemcpyAsync of as many bytes as the copies
occupy, the comparison at 100% floods (the kernel reads each source once and writes it fan-out times, so that
plain copy is the honest bound). Prints one JSON line.

    python tools/flood_bench.py [--steps 10] [--rounds 3] [--out profiles/flood_bench.json]

Workloads: C1 (1,500-byte frames) and the C3 mix, 128-byte frame starts and 128-byte copy slots. Flood shares
0%, 10% and 100% of the packets (the others leave through a random port), fan-outs 1, 4 and 23 ports (a table
of fan-out + 1 ACCESS ports on one VLAN, ingress port 0). A case whose copies would exceed --max-copy-gib
runs on as many of the workload's first packets as fit; `packets` says how many. The timed calls rotate over
two separately generated arenas, each with its own copy region, as bench.py's do. Variants are timed
interleaved in one process, `rounds` times; each figure is the median over the rounds of (HIP-event ms over
`steps` calls) / steps, with the minimum beside it.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import netflow_amd as nf  # noqa: E402

SEED = 20250620
SHARES = (0.0, 0.1, 1.0)
FANS = (1, 4, 23)
NROT = 2
NONE = 0xFFFFFFFF


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


def run_case(eng, hip, config, hdesc_all, share, fan, steps, rounds, warmup, max_copy):
    rng = np.random.default_rng(int(share * 100) * 64 + fan)
    n = len(hdesc_all)
    with nf.Fdb() as fdb:
        for p in range(fan + 1):
            fdb.set_port(p, native_vlan=1)
        fdb.commit().upload(eng)

        def arrays(m):
            flood = rng.random(m) < share if share < 1.0 else np.ones(m, bool)
            l2 = np.where(flood, NONE, rng.integers(1, fan + 1, m)).astype(np.uint32)
            return l2, np.where(flood, nf.L2_FLOOD, nf.L2_FORWARD).astype(np.uint8), np.ones(m, np.uint16)

        def need(m, arr):
            d = hdesc_all[:m]
            frames = (int(d["off16"][-1]) * 16 + int(d["len"][-1]) + 127) // 128 * 128
            t = fdb.flood_expand_host(0, fan + 1, 1 << 50, frames, 128, d, 0, l2_port=arr[0], l2_verdict=arr[1],
                                      l2_vlan=arr[2])["totals"]
            return frames, int(t["items_needed"]), int(t["copy_bytes_needed"])

        arr = arrays(n)
        frames, items, cbytes = need(n, arr)
        if cbytes > max_copy:  # as many of the first packets as fit
            n = max(int(n * max_copy / cbytes) // 1024 * 1024, 1024)
            arr = tuple(a[:n] for a in arr)
            frames, items, cbytes = need(n, arr)
        hdesc = hdesc_all[:n]
        arena_bytes = frames + cbytes
        d_desc = eng.alloc(hdesc.nbytes).upload(hdesc)
        arenas = [eng.alloc(arena_bytes + 16) for _ in range(NROT)]
        for a in arenas:
            eng.gen_config_device(config, SEED, 0, n, a, frames, d_desc)
        d_l2, d_verdict, d_vlan = (eng.alloc(max(a.nbytes, 16)).upload(a) for a in arr)
        d_idesc, d_iport, d_isrc, d_tot = eng.alloc(8 * items + 16), eng.alloc(4 * items + 16), eng.alloc(4 * items + 16), eng.alloc(32)
        d_hash = eng.alloc(4 * n)
        d_src = eng.alloc(cbytes + 16) if cbytes else None
        eng.sync()
        ctr = [0]

        def nxt():
            ctr[0] += 1
            return arenas[ctr[0] % NROT]

        def expand():
            eng.flood_expand_device(fdb, 0, fan + 1, nxt(), arena_bytes, frames, 128, d_desc, n, items, d_idesc, d_iport,
                                    d_isrc, d_tot, l2_port=d_l2, l2_verdict=d_verdict, l2_vlan=d_vlan)

        def memcpy():
            rc = hip.hipMemcpyAsync(ctypes.c_void_p(nxt().ptr + frames), ctypes.c_void_p(d_src.ptr), ctypes.c_size_t(cbytes),
                                    3, ctypes.c_void_p(eng.stream))  # 3: hipMemcpyDeviceToDevice
            if rc:
                raise RuntimeError(f"hipMemcpyAsync: {rc}")

        variants = {"flowkey_hash": lambda: eng.flow_keys_device(nxt(), frames, d_desc, n, None, d_hash), "expand": expand}
        if cbytes:
            variants["memcpy_d2d"] = memcpy
        times = {k: [] for k in variants}
        for step in variants.values():
            for _ in range(warmup):
                step()
        eng.sync()
        for _ in range(rounds):
            for k, step in variants.items():
                times[k].append(event_ms(eng, step, steps) / steps)
        tot = d_tot.download(nf.FLOOD_TOTALS_DTYPE, 1)[0]
        assert int(tot["items"]) == items and int(tot["copy_bytes"]) == cbytes, "the timed call cut its burst"
        res = {"packets": n, "flood_share": share, "fan_out": fan, "items": items, "copies": int(tot["copies"]),
               "copy_bytes": cbytes, "frame_bytes": frames}
        for k, xs in times.items():
            res[k] = med_min(xs)
        res["expand"]["x_flowkey"] = round(res["expand"]["ms"] / res["flowkey_hash"]["ms"], 3)
        if cbytes:
            res["expand"]["x_memcpy"] = round(res["expand"]["ms"] / res["memcpy_d2d"]["ms"], 3)
            res["expand"]["copy_gb_s"] = round(cbytes / (res["expand"]["ms"] * 1e-3) / 1e9, 1)
            res["memcpy_d2d"]["copy_gb_s"] = round(cbytes / (res["memcpy_d2d"]["ms"] * 1e-3) / 1e9, 1)
        for b in arenas + [d_desc, d_l2, d_verdict, d_vlan, d_idesc, d_iport, d_isrc, d_tot, d_hash] + ([d_src] if d_src else []):
            b.free()
        return res


def run_workload(eng, hip, config, n, args):
    hdesc, _ = nf.layout_config(config, SEED, 0, n, 128)
    out = {}
    for share in SHARES:
        for fan in (FANS if share else (4,)):
            out[f"flood{int(share * 100)}_fan{fan}"] = run_case(eng, hip, config, hdesc, share, fan, args.steps, args.rounds,
                                                                args.warmup, int(args.max_copy_gib * (1 << 30)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--c1-packets", type=int, default=1 << 20)
    ap.add_argument("--c3-packets", type=int, default=1 << 22)
    ap.add_argument("--max-copy-gib", type=float, default=4.0)
    ap.add_argument("--workloads", default="c1,c3", help="which of c1, c3 to run")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # the events are torch's, on the runtime the engine shares
    torch.cuda.init()
    try:  # the runtime the engine and torch already loaded
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.restype = ctypes.c_int
    with nf.Engine(0) as eng:
        res = {"tool": "tools/flood_bench.py", "steps": args.steps, "rounds": args.rounds,
               "timing": "HIP events on the engine's stream around the rotated calls; median (and min) over rounds",
               "x_flowkey_is": "expand ms over flowkey_hash ms in the same run",
               "x_memcpy_is": "expand ms over the ms of a device-to-device hipMemcpyAsync of copy_bytes in the same run",
               "library": os.path.basename(os.path.dirname(os.path.abspath(nf.LIB_PATH))) + "/" + os.path.basename(nf.LIB_PATH)}
        for name, config, n in (("c1", nf.CFG_C1, args.c1_packets), ("c3", nf.CFG_C3, args.c3_packets)):
            if name in args.workloads.split(","):
                res[name] = run_workload(eng, hip, config, n, args)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
