"""The C++ host API's L2 path (include/netflow_amd/packet.hpp: ChecksumEngine::upload_fdb and
l2_lookup_batch) over netflow_amd::Packet objects on the GPU, against the reference's decisions on the
fixture frames."""
import os
import subprocess

import numpy as np
import pytest

import netflow_amd as nf
from l2_common import l2_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "l2_lookup_test.cpp")


@pytest.mark.gpu
def test_cpp_upload_fdb_and_l2_lookup_batch(tmp_path):
    if not os.path.exists(nf.LIB_PATH):
        nf.build()
    exe, libdir = str(tmp_path / "l2_lookup_test"), os.path.dirname(nf.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L" + libdir, "-l:" + os.path.basename(nf.LIB_PATH), "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    z, frames = l2_fixture()
    run = 1  # ingress = the TRUNK port
    rt = (np.arange(len(frames)) % 3 == 0) * nf.RT_FORWARD + (np.arange(len(frames)) % 3 != 0) * nf.RT_NOT_IPV4
    lines = [f"I {int(z['ingress'][run])}"]
    lines += [f"E {bytes(e).hex()}" for e in z["entries"]]
    for i, p in enumerate(z["ports"]):
        lines.append(" ".join([f"P {bytes(p).hex()}"] + [str(int(v)) for v in z["allowed"][i, :int(z["allowed_n"][i])]]))
    lines += [f"F {int(v)} {f.hex()}" for v, f in zip(rt, frames)]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[:2000] + r.stderr
    rows = np.array([[int(x) for x in ln.split()] for ln in r.stdout.strip().split("\n")], dtype=np.int64)
    assert rows.shape == (len(frames), 5)
    for k, name in enumerate(("verdict", "egress", "vlan", "learn")):  # the reference's decisions
        assert np.array_equal(rows[:, k], z[f"{name}_{run}"].astype(np.int64)), name
    assert np.array_equal(rows[:, 4], np.where(rt == nf.RT_NOT_IPV4, z[f"verdict_{run}"], nf.L2_SKIP))
