#!/usr/bin/env python3
"""Times nfcs_acl_eval_device against the flow-key kernel (hashes only: the same read pattern, one
header line per frame) in the same run. Prints one JSON line.

    python tools/acl_bench.py [--steps 20] [--rounds 3] [--out profiles/acl_eval_bench.json]

Per workload (1M C1 frames, the 4M C3 mix; 128-byte frame starts as bench.py's default) the timed
calls rotate over separately generated batches (4 up to 1M packets, 2 above) as bench.py's do, so no
call finds its header lines in the memory-side cache. Variants are timed interleaved in one process,
`rounds` times; each figure is the median over the rounds of (HIP-event ms over `steps` calls) / steps,
with the minimum beside it.

Rule lists:
  worst(N)   N - 1 rules no frame matches (a random source address and a destination port each), then
             a PERMIT rule without match fields: every frame scans all N rules (the linear scan's worst
             case) and is decided by the last one. N = 16, 64, 512. A compiled rule costs the same
             whatever fields it sets (eight masked dword compares), so the fields chosen do not matter.
worst16 is also timed writing actions only (no rule index, no redirect port). The per-rule cost once the
scan dominates is (worst512 - worst64) / 448 per batch.
  worst(N)_l2  the same lists with EtherType 0x0800 also set in every rule but the last, so that every trip
             of the scan reads the MAC / VLAN / EtherType halves of its rules as well (a list of address
             and port rules alone never does). N = 16, 512.
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

SEED = 20250620
HBM_PEAK_GBS = 8000.0


def acl_worst(n_rules: int, l2: bool = False) -> nf.Acl:
    rng = np.random.default_rng(n_rules)
    r = np.zeros(n_rules, dtype=nf.ACL_RULE_DTYPE)
    r["fields"][:-1] = nf.ACL_F_SRC_IP | nf.ACL_F_DST_PORT | (nf.ACL_F_ETHERTYPE if l2 else 0)
    r["ethertype"] = 0x0800
    r["src_ip"][:-1] = rng.integers(0xE0000000, 0xF0000000, size=n_rules - 1, dtype=np.uint64).astype(np.uint32)
    r["src_ip_mask"] = r["dst_ip_mask"] = 0xFFFFFFFF
    r["dst_port"][:-1] = rng.integers(1, 1 << 16, size=n_rules - 1)
    r["action"][:-1] = nf.ACL_DENY
    r["action"][-1] = nf.ACL_PERMIT  # no fields: matches every frame, last
    r["redirect_port"] = nf.IF_NONE
    r["rule_id"] = np.arange(n_rules)
    return nf.Acl().set_rules(r).commit()


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


def run_workload(eng, config: int, n: int, steps: int, rounds: int, warmup: int):
    nrot = 4 if n <= (1 << 20) else 2
    batches = [eng.config_batch(config, SEED, 0, n, 128) for _ in range(nrot)]
    hdesc = batches[0][3]
    hdr = float(np.minimum(hdesc["len"].astype(np.float64), 128.0).sum())
    d_act, d_rule, d_red, d_hash = eng.alloc(n), eng.alloc(4 * n), eng.alloc(4 * n), eng.alloc(4 * n)
    ctr = [0]

    def nxt():
        ctr[0] += 1
        return batches[ctr[0] % nrot][:3]

    acls = {"worst16": acl_worst(16), "worst64": acl_worst(64), "worst512": acl_worst(512),
            "worst16_l2": acl_worst(16, True), "worst512_l2": acl_worst(512, True)}
    for a in acls.values():
        a.upload(eng)
    variants = {"flowkey_hash": lambda: eng.flow_keys_device(*nxt(), n, None, d_hash)}
    for name, a in acls.items():
        variants["acl_" + name] = (lambda a=a: eng.acl_eval_device(a, *nxt(), n, d_act, d_rule, d_red))
    variants["acl_worst16_actions_only"] = lambda: eng.acl_eval_device(acls["worst16"], *nxt(), n, d_act)
    times = {k: [] for k in variants}
    for k, step in variants.items():
        for _ in range(warmup):
            step()
    eng.sync()
    for _ in range(rounds):
        for k, step in variants.items():
            times[k].append(event_ms(eng, step, steps) / steps)
    out = {"packets": n, "batches_rotated": nrot, "frame_align": 128}
    per_packet = {"flowkey_hash": 12.0, "acl_worst16_actions_only": 9.0}
    for k, xs in times.items():
        bytes_moved = hdr + per_packet.get(k, 17.0) * n
        out[k] = med_min(xs)
        out[k]["frac"] = round(bytes_moved / (out[k]["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        out[k]["gpkt_s"] = round(n / (out[k]["ms"] * 1e-3) / 1e9, 2)
    out["ns_per_rule_per_1M_packets"] = round(
        (out["acl_worst512"]["ms"] - out["acl_worst64"]["ms"]) / 448.0 * 1e6 * (1 << 20) / n, 2)
    # what the lists decide on this workload: every frame by the last rule
    for name, a in acls.items():
        eng.acl_eval_device(a, *batches[0][:3], n, d_act, d_rule, d_red)
        eng.sync()
        rule = d_rule.download(np.uint32, n)
        out["acl_" + name]["decided_by_last_rule"] = round(float((rule == int(name[5:].split("_")[0]) - 1).mean()), 4)
    for a in acls.values():
        a.close()
    for b in batches:
        b[0].free()
        b[2].free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--c1-packets", type=int, default=1 << 20)
    ap.add_argument("--c3-packets", type=int, default=1 << 22)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # the events below are torch's, on the runtime the engine shares
    torch.cuda.init()
    with nf.Engine(0) as eng:
        res = {"tool": "tools/acl_bench.py", "steps": args.steps, "rounds": args.rounds,
               "timing": "HIP events on the engine's stream around the rotated calls; median (and min) over rounds",
               "frac_is_on": "min(len, 128) header line + 8 descriptor + outputs (ACL 1 + 4 + 4, actions only 1, "
                             "hash 4) per packet, against 8000 GB/s",
               "c1": run_workload(eng, nf.CFG_C1, args.c1_packets, args.steps, args.rounds, args.warmup),
               "c3": run_workload(eng, nf.CFG_C3, args.c3_packets, args.steps, args.rounds, args.warmup)}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
