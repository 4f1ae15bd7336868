#!/usr/bin/env python3
"""The every-packet-stores case of the plain update: bench.py's timed calls rotate over
batches its warm-up already updated, so they find every checksum right and, since the store skipping,
write no frame byte. Here every timed nfcs_update_device call finds freshly generated frames, whose
checksum fields are wrong, and so stores both fields of every packet.

The calls rotate over 4 batches; each batch is regenerated on the device (gen_config_device, untimed)
right after its timed call, three other batches' calls before it is used again, so the timed call does not
find its frames in the memory-side cache; a read-only pass over another batch follows each regeneration,
so the generator's dirty lines are written back before the next timed call and not during it (without it
a C1 call measured 0.40 ms in both builds). Each call is timed with HIP events (nfcs_time_update_device,
one call). A second loop without the regeneration gives the no-store figure from the same process. Before timing, one batch is digested fresh and updated: the digests must differ (the
generator's checksum fields are not the updated ones), else the script stops.

With --stale-every k the timed calls instead find an updated batch in which every k-th packet's checksum
fields were made stale again (stale_every_device, untimed, in place of the regeneration): a fraction 1/k of
the packets stores; k = 0 is the no-store case. --store-policy auto | deferred | sparse sets the form of the
calls (nfcs_ctx_set_store_policy), --split-compare adds the no-store rotation timed
as one launch per call against two launches of half the packets each (back to back, HIP events around 10
rounds, the median of 9 alternating repetitions). The line carries the forms the timed calls ran in.

  python3 tools/store_case_bench.py --config 1 --steps 40
  python3 tools/store_case_bench.py --config 1 --stale-every 16 --store-policy sparse
  NFCS_LIB=/path/to/another/libnfcs.so python3 tools/store_case_bench.py ...   # an A/B build

prints one JSON line. tools/store_case_ab.sh alternates two builds."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import netflow_amd as nf  # noqa: E402

SEED = 20250620
PACKETS = {1: 1 << 20, 3: 1 << 22}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=1, choices=sorted(PACKETS))
    ap.add_argument("--packets", type=int, default=0)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--align", type=int, default=128)
    ap.add_argument("--batches", type=int, default=0)
    ap.add_argument("--stale-every", type=int, default=-1,
                    help="k: every k-th packet stale before each timed call (0: none); default: regenerate")
    ap.add_argument("--store-policy", choices=["auto", "deferred", "sparse"], default="auto")
    ap.add_argument("--split-compare", action="store_true")
    ap.add_argument("--back-to-back", action="store_true",
                    help="with --stale-every: also the wall time per call of calls issued back to back")
    a = ap.parse_args()
    n = a.packets or PACKETS[a.config]
    nrot = a.batches or (4 if n <= (1 << 20) else 2)
    with nf.Engine(0) as eng:
        has_forms = hasattr(nf.lib(), "nfcs_ctx_set_store_policy")  # an earlier build (NFCS_LIB) has one form
        if has_forms:
            eng.set_store_policy({"auto": nf.STORE_AUTO, "deferred": nf.STORE_DEFERRED,
                                  "sparse": nf.STORE_SPARSE}[a.store_policy])
        elif a.store_policy != "auto" or a.stale_every >= 0:
            raise SystemExit("this libnfcs.so has no store policy")
        batches = [eng.config_batch(a.config, SEED, 0, n, a.align) for _ in range(nrot)]
        forms = {}

        def timed(b):
            t = eng.time_update_device(b[0], b[1], b[2], n, 1)
            f = eng.store_state()[0] if has_forms else nf.STORE_DEFERRED
            forms[f] = forms.get(f, 0) + 1
            return t

        def regen(b):
            if a.stale_every >= 0:
                eng.stale_every_device(b[0], b[1], b[2], n, a.stale_every)
            else:
                eng.gen_config_device(a.config, SEED, 0, n, b[0], b[1], b[2])
            # a read-only pass over another batch, so that the generator's dirty lines have left the
            # memory-side cache before the next timed call (else their write-back lands in it)
            o = batches[(batches.index(b) + 1) % nrot]
            eng.digest_device(o[0], o[1], o[2], n, 0)

        fresh = eng.digest_device(batches[0][0], batches[0][1], batches[0][2], n, 0)
        eng.update_device(batches[0][0], batches[0][1], batches[0][2], n)
        eng.sync()
        updated = eng.digest_device(batches[0][0], batches[0][1], batches[0][2], n, 0)
        if fresh == updated:
            raise SystemExit("the generated frames already hold the updated checksums: nothing to store")
        if a.stale_every >= 0:  # every batch updated first: the stale packets are then exactly every k-th
            for b in batches:
                eng.update_device(b[0], b[1], b[2], n)
            eng.sync()
            for b in batches:
                regen(b)
        else:
            regen(batches[0])
            assert eng.digest_device(batches[0][0], batches[0][1], batches[0][2], n, 0) == fresh
        ms = []
        for s in range(a.warmup + a.steps):
            b = batches[s % nrot]
            if s == a.warmup:
                forms.clear()
            t = timed(b)
            if s >= a.warmup:
                ms.append(t)
            regen(b)
        forms_stores = dict(forms)
        if a.stale_every >= 0:
            for b in batches:
                eng.update_device(b[0], b[1], b[2], n)
            eng.sync()
        # the same loop without the regeneration, for the no-store figure from the same process
        ms_skip = []
        for s in range(nrot + a.steps):
            b = batches[s % nrot]
            t = timed(b)
            if s >= nrot:
                ms_skip.append(t)
        # Single calls with a host sync after each leave the GPU idle while an inline store's write-back
        # drains; a ring issues its calls back to back. Here every call is followed on its stream by the
        # untimed-elsewhere staling of its own batch (used again nrot - 1 calls later) and nothing waits:
        # the staling kernel is in the figure, the same in either form, so forms compare by difference.
        b2b = None
        if a.back_to_back and a.stale_every >= 0:
            per = []
            for _ in range(7):
                eng.sync()
                t0 = time.perf_counter()
                for s in range(a.steps):
                    b = batches[s % nrot]
                    eng.update_device(b[0], b[1], b[2], n)
                    eng.stale_every_device(b[0], b[1], b[2], n, a.stale_every)
                eng.sync()
                per.append((time.perf_counter() - t0) / a.steps * 1e3)
            b2b = {"median": round(statistics.median(per[2:]), 4), "min": round(min(per[2:]), 4),
                   "max": round(max(per[2:]), 4)}
            for b in batches:
                eng.update_device(b[0], b[1], b[2], n)
            eng.sync()
        split = None
        if a.split_compare:
            h = n // 2
            whole = [(b[0], b[1], b[2]) for b in batches]
            halves = [(b[0], b[1], b[2].ptr + 8 * k * h) for b in batches for k in (0, 1)]
            one, two = [], []
            for _ in range(9):
                one.append(eng.time_update_batches(whole, n, 10 * nrot) / (10 * nrot))
                two.append(eng.time_update_batches(halves, h, 20 * nrot) / (10 * nrot))
            split = {"one_launch_ms": round(statistics.median(one), 4), "two_launches_ms": round(statistics.median(two), 4),
                     "one_launch_range": [round(min(one), 4), round(max(one), 4)],
                     "two_launches_range": [round(min(two), 4), round(max(two), 4)]}
        final = eng.digest_device(batches[0][0], batches[0][1], batches[0][2], n, 0)
        for b in batches:
            b[0].free()
            b[2].free()
    q = lambda v, p: sorted(v)[min(len(v) - 1, int(p * len(v)))]
    print(json.dumps({"tool": "store_case_bench", "lib": nf.LIB_PATH, "config": a.config, "packets": n,
                      "align": a.align, "batches_rotated": nrot, "steps": a.steps,
                      "stale_every": a.stale_every, "store_policy": a.store_policy, "split_compare": split, "back_to_back_ms": b2b,
                      "forms_timed": {("sparse" if k == nf.STORE_SPARSE else "deferred" if k == nf.STORE_DEFERRED
                                       else "none"): v for k, v in forms_stores.items()},
                      "fresh_differs_from_updated": True, "digest_ok": final == updated,
                      "every_packet_stores_ms": {"median": round(statistics.median(ms), 4),
                                                 "p10": round(q(ms, 0.1), 4), "p90": round(q(ms, 0.9), 4),
                                                 "mean": round(statistics.fmean(ms), 4)},
                      "no_store_ms": {"median": round(statistics.median(ms_skip), 4),
                                      "p10": round(q(ms_skip, 0.1), 4), "p90": round(q(ms_skip, 0.9), 4),
                                      "mean": round(statistics.fmean(ms_skip), 4)}}), flush=True)


if __name__ == "__main__":
    main()
