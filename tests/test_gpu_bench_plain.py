"""A plain `bench.py` run (no --full): set-up, warm-up, the timed steps, the line with the headline
figure and nothing that takes runs of its own; `--dump-outputs DIR` writes what the last timed step
left — checked here byte for byte against the oracle's update of the same seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

N = 20000  # not a power of two; more packets than the dump samples, several workgroups


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dump"))
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--packets", str(N), "--dump-outputs", out]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    return json.loads(lines[0]), out


def test_plain_line_is_the_headline_only(plain_run):
    d, _ = plain_run
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "GB/s" and d["higher_is_better"] is True and d["dtype"].startswith("u16")
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value is frame bytes per timed step over ms_per_step
    assert abs(d["value"] - d["config"]["frame_bytes_per_gpu"] / d["ms_per_step"] / 1e6) <= 0.02 * d["value"]
    for k in ("roofline", "parity", "stream_ceiling", "replay", "c4_shard", "c3", "host", "more", "cpu_baseline"):
        assert k not in d, k


def test_dump_outputs_are_the_oracles_updated_batch(plain_run, oracle_lib):
    import bench
    _, out = plain_run
    files = sorted(os.listdir(out))
    assert files == ["frame_byte_sums.npy", "frame_index.npy", "frame_len.npy", "frames.npy"]
    arrs = {f[:-4]: np.load(os.path.join(out, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    arena, desc = oracle_lib.gen_config(1, bench.SEED, 0, N, 128)
    oracle_lib.update_batch(arena, desc)
    off = desc["off16"].astype(np.int64) * 16
    ln = desc["len"].astype(np.int64)
    idx = arrs["frame_index"].astype(np.int64)
    k = min(N, bench.DUMP_SAMPLE_BYTES // (4 * int(ln.max())))
    assert len(idx) == k and len(np.unique(idx)) == k and idx.min() >= 0 and idx.max() < N
    assert np.array_equal(idx, np.sort(np.random.default_rng(bench.SEED).choice(N, size=k, replace=False)))
    assert np.array_equal(arrs["frame_len"], ln[idx])
    assert arrs["frames"].shape == (k, int(ln.max()))
    for row, i in zip(arrs["frames"], idx):
        want = arena[off[i]: off[i] + ln[i]]
        assert np.array_equal(row[: ln[i]], want) and not row[ln[i]:].any(), int(i)
    want_sums = np.array([int(arena[o: o + l].sum(dtype=np.uint64)) for o, l in zip(off, ln)])
    assert np.array_equal(arrs["frame_byte_sums"], want_sums)
