"""The C++ host API's flood replication (include/netflow_amd/packet.hpp: ChecksumEngine::upload_fdb,
l2_lookup_batch, flood_expand_batch) over netflow_amd::Packet objects on the GPU, on a slice of the fixture's
frames, against Fdb.flood_expand_host on the reference's decisions."""
import os
import subprocess

import numpy as np
import pytest

import netflow_amd as nf
from flood_common import fixture_fdb, flood_fixture, packed, round_up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "flood_test.cpp")


@pytest.mark.gpu
def test_cpp_l2_lookup_then_flood_expand_batch(tmp_path):
    if not os.path.exists(nf.LIB_PATH):
        nf.build()
    exe, libdir = str(tmp_path / "flood_test"), os.path.dirname(nf.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L" + libdir, "-l:" + os.path.basename(nf.LIB_PATH), "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    z, frames = flood_fixture()
    run, n = 0, 400
    frames = frames[:n]
    ingress, num_ports = int(z["ingress"][run]), int(z["num_ports"])
    lines = [f"I {ingress}", f"N {num_ports}"]
    lines += [f"E {bytes(e).hex()}" for e in z["entries"]]
    for i, p in enumerate(z["ports"]):
        lines.append(" ".join([f"P {bytes(p).hex()}"] + [str(int(v)) for v in z["allowed"][i, :int(z["allowed_n"][i])]]))
    lines += [f"F {f.hex()}" for f in frames]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[:2000] + r.stderr
    out = r.stdout.strip().split("\n")
    desc, used = packed([len(f) for f in frames])
    with fixture_fdb(z) as fdb:
        want = fdb.flood_expand_host(ingress, num_ports, 1 << 30, round_up(used, 128), 16, desc, 8192,
                                     l2_port=z[f"egress_{run}"][:n], l2_verdict=z[f"verdict_{run}"][:n],
                                     l2_vlan=z[f"vlan_{run}"][:n])
    t = want["totals"]
    m = int(t["items"])
    assert out[0].split() == ["T"] + [str(int(t[k])) for k in ("items", "items_needed", "copies", "flooded", "copy_bytes")]
    flood = z[f"verdict_{run}"][:n] == nf.L2_FLOOD
    assert flood.sum() >= 100 and (z[f"egress_{run}"][:n] != nf.IF_NONE).sum() >= 40  # the slice holds both kinds
    assert len(out) == 1 + m and m - int(t["copies"]) == (z[f"egress_{run}"][:n] != nf.IF_NONE).sum()
    for k, line in enumerate(out[1:]):
        f = line.split()
        src = int(want["item_src"][k])
        assert (int(f[0]), int(f[1]), int(f[2])) == (src, int(want["item_port"][k]), len(frames[src])), k
        assert int(f[3]) == int(flood[src]) and (f[4] if len(f) > 4 else "") == frames[src].hex(), k
    assert np.array_equal(want["item_desc"]["len"][:m], [len(frames[int(s)]) for s in want["item_src"][:m]])
