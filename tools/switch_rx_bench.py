#!/usr/bin/env python3
"""Times the ingress dispatch stage (nfcs_ingress_dispatch_device) and the one-call RX pipeline
(nfcs_switch_rx_device) against the flow-key kernel (hashes only: one header line per frame) in the same run.
Prints one JSON line.

    python tools/switch_rx_bench.py [--steps 10] [--rounds 3] [--out profiles/switch_rx_bench.json]

Per workload (1M C1 frames, the 4M C3 mix; 128-byte frame starts as bench.py's default) the timed calls rotate
over separately generated batches (4 up to 1M packets, 2 above) as bench.py's do, so no call finds its frames in
the memory-side cache. Variants are timed interleaved in one process, `rounds` times; each figure is the median
over the rounds of (HIP-event ms over `steps` calls) / steps, with the minimum beside it. `x` is the variant's
time over the yardstick's (flowkey_hash) in the same run.

The dispatch stage is fed the route lookup's and the L2 lookup's real outputs for the batch and an ingress-ACL
action array that is drawn: all PERMIT ("live"), or 5% DENY and 5% REDIRECT, half of those to a port that is
down ("mixed"); each with the counters given ("count") and not given ("nocount").
The pipeline: switch_rx (one call) beside the same eleven stages launched one by one on the same stream with no
host work between them (stages), and plan (the egress plan alone over the burst, the stage the dispatch was
expected to cost as much as). The queue depths are zeroed on the stream before every pipeline call (a copy of
`keys` words inside the timed region of both variants), so that the queues never fill.
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
PORTS, QUEUES, DEPTH = 8, 4, 1 << 16
COPY_ROOM = 64 << 20


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


def make_tables(eng):
    """A default route through one gateway (every transit IPv4 frame forwards to port 1), eight ports on VLAN 1 with
    port 5 down, an ingress list and one egress list of a few rules that match little, four queues per port."""
    fib = nf.Fib()
    routes = np.zeros(1, nf.FIB_ROUTE_DTYPE)
    routes["next_hop_ip"], routes["egress_if"] = nf.ip4("10.255.0.1"), 1
    arp = np.zeros(1, nf.FIB_ARP_DTYPE)
    arp["ip"], arp["mac"] = nf.ip4("10.255.0.1"), [2, 0, 0, 0, 0, 0x77]
    ifm = np.zeros(PORTS, nf.FIB_IF_MAC_DTYPE)
    ifm["egress_if"], ifm["mac"] = np.arange(PORTS), [[2, 0, 0, 0, 1, p] for p in range(PORTS)]
    fib.set_routes(routes).set_arp(arp).set_if_macs(ifm).set_local_ips(np.array([nf.ip4("10.255.0.254")], np.uint32)).commit()
    fdb, eg, aclset, acl = nf.Fdb(), nf.Egress(), nf.AclSet(), nf.Acl()
    rules = np.zeros(4, nf.ACL_RULE_DTYPE)
    rules["fields"], rules["dst_port"], rules["action"] = nf.ACL_F_DST_PORT, [7, 9, 13, 19], nf.ACL_DENY
    for p in range(PORTS):
        fdb.set_port(p, link_up=p != 5, native_vlan=1)
        eg.set_port(p, native_vlan=1, num_queues=QUEUES, max_queue_depth=DEPTH)
        aclset.bind_port(p, 0)
    aclset.set_list(0, rules)
    acl.set_rules(rules)
    tabs = dict(fib=fib, fdb=fdb.commit(), eg=eg.commit(), aclset=aclset.commit(), acl=acl.commit())
    for t in tabs.values():
        t.upload(eng)
    return tabs


def run_workload(eng, tabs, config: int, n: int, steps: int, rounds: int, warmup: int):
    import torch
    st = torch.cuda.ExternalStream(eng.stream)
    nrot = 4 if n <= (1 << 20) else 2
    hdesc, frames_bytes = nf.layout_config(config, SEED, 0, n, 128)
    copy_base = (frames_bytes + 127) & ~127
    nbytes = copy_base + COPY_ROOM
    cap = 2 * n
    d_desc = eng.alloc(max(hdesc.nbytes, 16)).upload(hdesc)
    arenas = [eng.alloc(nbytes) for _ in range(nrot)]
    for a in arenas:
        eng.gen_config_device(config, SEED, 0, n, a, frames_bytes, d_desc)
    eng.sync()
    ctr = [0]

    def nxt():
        ctr[0] += 1
        return arenas[ctr[0] % nrot]

    A = eng.alloc
    d_hash, d_nh, d_if, d_rt, d_st = A(4 * n), A(4 * n), A(4 * n), A(n), A(n)
    d_l2p, d_l2v, d_vlan, d_cls, d_byp, d_act, d_red = A(4 * n), A(n), A(2 * n), A(n), A(n), A(n), A(4 * n)
    d_ared = A(4 * n)  # the ACL stage's own redirect ports, beside the drawn ones
    d_idesc, d_iport, d_isrc, d_tot = A(8 * cap), A(4 * cap), A(4 * cap), A(32)
    d_port, d_ops, d_queue, d_eact, d_order = A(4 * cap), A(4 * cap), A(cap), A(cap), A(4 * cap)
    ports, keys = tabs["eg"].keys()
    acl_ports = max(tabs["aclset"].info()[0], 1)
    d_ks, d_kd, d_dpk, d_dby = A(4 * (keys + 1)), A(4 * keys), A(4 * acl_ports).upload(np.zeros(acl_ports, np.uint32)), \
        A(8 * acl_ports).upload(np.zeros(acl_ports, np.uint64))
    d_rx = A(24 * PORTS).upload(np.zeros(PORTS, nf.RX_STATS_DTYPE))
    ws_bytes = nf.switch_rx_workspace_bytes(n, cap)
    d_ws = A(ws_bytes)
    depth = torch.zeros(keys, dtype=torch.int32, device="cuda")
    zero = torch.zeros(keys, dtype=torch.int32, device="cuda")
    fib, fdb, eg, aclset, acl = (tabs[k] for k in ("fib", "fdb", "eg", "aclset", "acl"))
    d_tab, tab_n = fib.nexthops()
    txq = nf.TxQueues(eg, eng)
    # the dispatch's inputs: the two lookups' outputs for the batch (every rotated batch holds the same frames)
    eng.route_lookup_device(fib, arenas[0], copy_base, d_desc, n, d_nh, egress_if=d_if, verdict=d_rt)
    eng.l2_lookup_device(fdb, 0, arenas[0], copy_base, d_desc, n, d_l2p, rt_verdict=d_rt, verdict=d_l2v, vlan=d_vlan)
    eng.sync()
    keep = [b.download(np.uint8, b.nbytes) for b in (d_nh, d_l2p, d_l2v)]
    rng = np.random.default_rng(n)
    draw = rng.random(n)
    acts = {"live": np.zeros(n, np.uint8),
            "mixed": np.where(draw < 0.05, nf.ACL_DENY, np.where(draw < 0.10, nf.ACL_REDIRECT, nf.ACL_PERMIT)).astype(np.uint8)}
    red = np.where(rng.random(n) < 0.5, 5, 3).astype(np.uint32)  # port 5 is down
    d_red.upload(red)
    d_acts = {k: A(n).upload(v) for k, v in acts.items()}

    def restore():  # the dispatch masks its in/out arrays: put the lookups' outputs back (outside the timed region)
        for b, a in zip((d_nh, d_l2p, d_l2v), keep):
            b.upload(a)

    def dispatch(kind, count):
        eng.ingress_dispatch_device(fdb, 0, PORTS, nxt(), copy_base, d_desc, n, d_rt, d_nh, d_l2p, d_l2v, action=d_acts[kind],
                                    redirect=d_red, cls=d_cls, bypass=d_byp, rx_stats=d_rx if count else None)

    def zero_depth():
        with torch.cuda.stream(st):
            depth.copy_(zero, non_blocking=True)

    def composite():
        zero_depth()
        eng.switch_rx_device(fib, fdb, eg, 0, PORTS, nxt(), nbytes, copy_base, 128, d_desc, n, cap, depth.data_ptr(), d_idesc, d_port,
                             d_isrc, d_tot, d_order, d_ks, d_ws, ws_bytes, ingress_acl=acl, aclset=aclset, txq=txq, denied_pkts=d_dpk,
                             denied_bytes=d_dby, rx_stats=d_rx, key_dropped=d_kd, cls=d_cls, handle_base=0)

    def stages():
        zero_depth()
        a = nxt()
        eng.route_lookup_device(fib, a, copy_base, d_desc, n, d_nh, egress_if=d_if, verdict=d_rt)
        eng.acl_eval_device(acl, a, copy_base, d_desc, n, d_act, redirect=d_ared, nh=d_nh)
        eng.l2_lookup_device(fdb, 0, a, copy_base, d_desc, n, d_l2p, rt_verdict=d_rt, verdict=d_l2v, vlan=d_vlan)
        eng.ingress_dispatch_device(fdb, 0, PORTS, a, copy_base, d_desc, n, d_rt, d_nh, d_l2p, d_l2v, action=d_act, redirect=d_ared,
                                    cls=d_cls, bypass=d_byp, rx_stats=d_rx)
        eng.l3_forward_device(a, copy_base, d_desc, d_nh, n, d_tab, tab_n, d_st)
        eng.flood_expand_device(fdb, 0, PORTS, a, nbytes, copy_base, 128, d_desc, n, cap, d_idesc, d_iport, d_isrc, d_tot, l3_port=d_if,
                                fwd_status=d_st, l2_port=d_l2p, l2_verdict=d_l2v, l2_vlan=d_vlan)
        eng.egress_plan_device(eg, a, nbytes, d_idesc, cap, d_port, d_ops, d_queue, l2_port=d_iport)
        eng.vlan_device(a, nbytes, d_idesc, cap, d_ops, 0, None, 0)
        eng.egress_acl_items_device(aclset, a, nbytes, d_idesc, cap, d_port, d_eact, item_src=d_isrc, bypass=d_byp, n_src=n,
                                    denied_pkts=d_dpk, denied_bytes=d_dby)
        eng.egress_enqueue_device(eg, d_port, d_queue, cap, depth.data_ptr(), d_order, d_ks, key_dropped=d_kd)
        eng.txq_append_device(txq, d_order, d_ks, depth.data_ptr(), cap, desc=d_idesc)

    def plan():
        eng.egress_plan_device(eg, nxt(), copy_base, d_desc, n, d_port, d_ops, d_queue, l2_port=d_if)

    variants = {"flowkey_hash": lambda: eng.flow_keys_device(nxt(), copy_base, d_desc, n, None, d_hash), "plan": plan}
    for kind in acts:
        for count in (True, False):
            variants[f"dispatch_{kind}_{'count' if count else 'nocount'}"] = (lambda k=kind, c=count: dispatch(k, c))
    variants["switch_rx"], variants["stages"] = composite, stages
    times = {k: [] for k in variants}
    for k, step in variants.items():
        if k.startswith("dispatch"):
            restore()
        for _ in range(warmup):
            step()
    eng.sync()
    for _ in range(rounds):
        for k, step in variants.items():
            if k.startswith("dispatch"):
                restore()
                eng.sync()
            times[k].append(event_ms(eng, step, steps) / steps)
    out = {"packets": n, "batches_rotated": nrot, "frame_align": 128, "cap": cap}
    for k, xs in times.items():
        out[k] = med_min(xs)
        out[k]["gpkt_s"] = round(n / (out[k]["ms"] * 1e-3) / 1e9, 2)
        out[k]["x"] = round(out[k]["ms"] / out["flowkey_hash"]["ms"], 3)
    out["switch_rx_over_stages"] = round(out["switch_rx"]["ms"] / out["stages"]["ms"], 3)
    composite()
    eng.sync()
    tot = d_tot.download(nf.FLOOD_TOTALS_DTYPE, 1)[0]
    cls = d_cls.download(np.uint8, n)
    out["items"], out["items_needed"] = int(tot["items"]), int(tot["items_needed"])
    out["classes"] = {str(c): int(k) for c, k in zip(*np.unique(cls, return_counts=True))}
    txq.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--c1-packets", type=int, default=1 << 20)
    ap.add_argument("--c3-packets", type=int, default=1 << 22)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # the events and the depth arrays are torch's, on the runtime the engine shares
    torch.cuda.init()
    with nf.Engine(0) as eng:
        tabs = make_tables(eng)
        res = {"tool": "tools/switch_rx_bench.py", "steps": args.steps, "rounds": args.rounds,
               "timing": "HIP events on the engine's stream around the rotated calls; median (and min) over rounds",
               "x_is": "the variant's ms over flowkey_hash's ms in the same run",
               "c1": run_workload(eng, tabs, nf.CFG_C1, args.c1_packets, args.steps, args.rounds, args.warmup),
               "c3": run_workload(eng, tabs, nf.CFG_C3, args.c3_packets, args.steps, args.rounds, args.warmup)}
        for t in tabs.values():
            t.close()
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
