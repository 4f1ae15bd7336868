#!/usr/bin/env python3
"""Times nfcs_egress_acl_device (one rule list per egress port, chosen per packet) against the flow-key
kernel (hashes only: the same read pattern, one header line per frame) and against nfcs_acl_eval_device
with one worst(16) list, all in the same run. Prints one JSON line.

    python tools/egress_acl_bench.py [--steps 20] [--rounds 3] [--out profiles/egress_acl_bench.json]

Per workload (1M C1 frames, the 4M C3 mix; 128-byte frame starts as bench.py's default) the timed calls
rotate over separately generated batches (4 up to 1M packets, 2 above) as tools/acl_bench.py's do. Variants
are timed interleaved in one process, `rounds` times; each figure is the median over the rounds of (HIP-event
ms over `steps` calls) / steps, with the minimum beside it.

Rule lists: worst(N) of tools/acl_bench.py (N - 1 rules no frame matches, then a PERMIT rule without match
fields: every frame scans the whole list), one per port with its own random rules. Every packet is permitted
by its list's last rule, so the calls leave d_port as it was and every call of a variant does the same work.

  a_unbound          a set without any binding: no packet has a list, no frame is read
  b_one_port         every packet leaves by port 0, bound to worst(16): the single-list call plus the port read
  c_P{2,8,64}_random P ports, each with its own worst(16) (P = 64: worst(8), so that 512 rules fit), the egress
                     port drawn per packet uniformly: a wave scans up to P lists
  c_P{..}_runs64     the same lists, the port constant over runs of 64 packets: a wave scans one list
  d_P{2,8,64}        what a caller did without this call: P single-list nfcs_acl_eval_device calls over the
                     whole burst (the merge on the host is not even counted)
  e_P8_half_denied   c_P8_random with the last rule of every odd port's list a DENY, and the deny counters:
                     d_port is written and the counters are added to. Every call gets a fresh copy of the
                     port array (uploaded before the timed region), since the call overwrites it.
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


def worst_rules(n_rules: int, seed: int, last_action=nf.ACL_PERMIT) -> np.ndarray:
    rng = np.random.default_rng(seed)
    r = np.zeros(n_rules, dtype=nf.ACL_RULE_DTYPE)
    r["fields"][:-1] = nf.ACL_F_SRC_IP | nf.ACL_F_DST_PORT
    r["src_ip"][:-1] = rng.integers(0xE0000000, 0xF0000000, size=n_rules - 1, dtype=np.uint64).astype(np.uint32)
    r["src_ip_mask"] = r["dst_ip_mask"] = 0xFFFFFFFF
    r["dst_port"][:-1] = rng.integers(1, 1 << 16, size=n_rules - 1)
    r["action"][:-1] = nf.ACL_DENY
    r["action"][-1] = last_action  # no fields: matches every frame, last
    r["redirect_port"] = nf.IF_NONE
    r["rule_id"] = np.arange(n_rules)
    return r


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
    d_act, d_rule, d_red, d_hash = eng.alloc(n), eng.alloc(4 * n), eng.alloc(4 * n), eng.alloc(4 * n)
    ctr = [0]

    def nxt():
        ctr[0] += 1
        return batches[ctr[0] % nrot][:3]

    rng = np.random.default_rng(n)
    keep = []  # objects that must outlive the timed calls
    variants = {"flowkey_hash": lambda: eng.flow_keys_device(*nxt(), n, None, d_hash)}
    single = nf.Acl().set_rules(worst_rules(16, 16)).commit().upload(eng)
    keep.append(single)
    variants["acl_worst16"] = lambda: eng.acl_eval_device(single, *nxt(), n, d_act, d_rule, d_red)

    def up(a):
        return eng.alloc(a.nbytes).upload(np.ascontiguousarray(a))

    def egress(s, d_port, pk=None, by=None):
        return lambda: eng.egress_acl_device(s, *nxt(), n, d_port, d_act, d_rule, d_red, pk, by)

    unbound = nf.AclSet().commit().upload(eng)
    keep.append(unbound)
    variants["a_unbound"] = egress(unbound, up(rng.integers(0, 8, n).astype(np.uint32)))
    one = nf.AclSet().set_list(0, worst_rules(16, 16)).bind_port(0, 0).commit().upload(eng)
    keep.append(one)
    variants["b_one_port"] = egress(one, up(np.zeros(n, np.uint32)))
    ports_of, sets = {}, {}
    for P in (2, 8, 64):
        per = 8 if P == 64 else 16
        lists = [worst_rules(per, 1000 * P + k) for k in range(P)]
        s = nf.AclSet()
        for k, r in enumerate(lists):
            s.set_list(k, r).bind_port(k, k)
        s.commit().upload(eng)
        keep.append(s)
        sets[P] = s
        random_ports = rng.integers(0, P, n).astype(np.uint32)
        runs = np.repeat(rng.integers(0, P, (n + 63) // 64).astype(np.uint32), 64)[:n]
        ports_of[P] = random_ports
        variants[f"c_P{P}_random"] = egress(s, up(random_ports))
        variants[f"c_P{P}_runs64"] = egress(s, up(runs))
        acls = [nf.Acl().set_rules(r).commit().upload(eng) for r in lists]
        keep += acls

        def p_calls(acls=acls):
            for a in acls:
                eng.acl_eval_device(a, *nxt(), n, d_act, d_rule, d_red)
        variants[f"d_P{P}"] = p_calls
    # half of the packets denied, counted: a fresh port array per call
    s_deny = nf.AclSet()
    for k in range(8):
        s_deny.set_list(k, worst_rules(16, 8000 + k, nf.ACL_DENY if k % 2 else nf.ACL_PERMIT)).bind_port(k, k)
    s_deny.commit().upload(eng)
    keep.append(s_deny)
    calls = warmup + steps * rounds
    fresh = [up(ports_of[8]) for _ in range(calls)]
    d_pk, d_by = up(np.zeros(8, np.uint32)), up(np.zeros(8, np.uint64))
    used = [0]

    def denied():
        eng.egress_acl_device(s_deny, *nxt(), n, fresh[used[0]], d_act, d_rule, d_red, d_pk, d_by)
        used[0] += 1
    variants["e_P8_half_denied"] = denied

    times = {k: [] for k in variants}
    for k, step in variants.items():
        for _ in range(warmup):
            step()
    eng.sync()
    for _ in range(rounds):
        for k, step in variants.items():
            times[k].append(event_ms(eng, step, steps) / steps)
    out = {"packets": n, "batches_rotated": nrot, "frame_align": 128}
    for k, xs in times.items():
        out[k] = med_min(xs)
        out[k]["gpkt_s"] = round(n / (out[k]["ms"] * 1e-3) / 1e9, 2)
        out[k]["vs_flowkey_hash"] = round(out[k]["ms"] / statistics.median(times["flowkey_hash"]), 3)
    out["b_over_single_list"] = round(out["b_one_port"]["ms"] / out["acl_worst16"]["ms"], 3)
    for P in (2, 8, 64):
        out[f"c_P{P}_random_over_d"] = round(out[f"c_P{P}_random"]["ms"] / out[f"d_P{P}"]["ms"], 3)
        out[f"c_P{P}_runs64_over_d"] = round(out[f"c_P{P}_runs64"]["ms"] / out[f"d_P{P}"]["ms"], 3)
    # what the calls decided: every packet by its list's last rule; the counted variant half denied
    eng.sync()
    pk = d_pk.download(np.uint32, 8)
    want = np.bincount(ports_of[8], minlength=8) * calls
    out["e_P8_half_denied"]["denied_share"] = round(float(pk.sum()) / (n * calls), 4)
    out["e_P8_half_denied"]["counters_exact"] = bool((pk[1::2] == (want[1::2] & 0xFFFFFFFF)).all() and not pk[0::2].any())
    eng.egress_acl_device(sets[64], *batches[0][:3], n, up(ports_of[64]), d_act, d_rule, d_red)
    eng.sync()
    out["c_P64_random"]["decided_by_last_rule"] = round(float((d_rule.download(np.uint32, n) == 7).mean()), 4)
    for o in keep:
        o.close()
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
        res = {"tool": "tools/egress_acl_bench.py", "steps": args.steps, "rounds": args.rounds,
               "timing": "HIP events on the engine's stream around the rotated calls; median (and min) over rounds",
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
