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

  python3 tools/store_case_bench.py --config 1 --steps 40
  NFCS_LIB=/path/to/another/libnfcs.so python3 tools/store_case_bench.py ...   # an A/B build

prints one JSON line. tools/store_case_ab.sh alternates two builds."""
import argparse
import json
import os
import statistics
import sys

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
    a = ap.parse_args()
    n = a.packets or PACKETS[a.config]
    nrot = a.batches or (4 if n <= (1 << 20) else 2)
    with nf.Engine(0) as eng:
        batches = [eng.config_batch(a.config, SEED, 0, n, a.align)[:3] for _ in range(nrot)]

        def regen(b):
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
        regen(batches[0])
        assert eng.digest_device(batches[0][0], batches[0][1], batches[0][2], n, 0) == fresh
        ms = []
        for s in range(a.warmup + a.steps):
            b = batches[s % nrot]
            t = eng.time_update_device(b[0], b[1], b[2], n, 1)
            if s >= a.warmup:
                ms.append(t)
            regen(b)
        # the same loop without the regeneration, for the no-store figure from the same process
        ms_skip = []
        for s in range(nrot + a.steps):
            b = batches[s % nrot]
            t = eng.time_update_device(b[0], b[1], b[2], n, 1)
            if s >= nrot:
                ms_skip.append(t)
        final = eng.digest_device(batches[0][0], batches[0][1], batches[0][2], n, 0)
        for b in batches:
            b[0].free()
            b[2].free()
    q = lambda v, p: sorted(v)[min(len(v) - 1, int(p * len(v)))]
    print(json.dumps({"tool": "store_case_bench", "lib": nf.LIB_PATH, "config": a.config, "packets": n,
                      "align": a.align, "batches_rotated": nrot, "steps": a.steps,
                      "fresh_differs_from_updated": True, "digest_ok": final == updated,
                      "every_packet_stores_ms": {"median": round(statistics.median(ms), 4),
                                                 "p10": round(q(ms, 0.1), 4), "p90": round(q(ms, 0.9), 4),
                                                 "mean": round(statistics.fmean(ms), 4)},
                      "no_store_ms": {"median": round(statistics.median(ms_skip), 4),
                                      "p10": round(q(ms_skip, 0.1), 4), "p90": round(q(ms_skip, 0.9), 4),
                                      "mean": round(statistics.fmean(ms_skip), 4)}}), flush=True)


if __name__ == "__main__":
    main()
