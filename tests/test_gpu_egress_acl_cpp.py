"""The egress ACLs through the C ABI from C++ (tests/cpp/egress_acl_test.cpp: nfcs_aclset_*, upload,
nfcs_egress_acl_device beside nfcs_egress_acl_host) on the GPU, against the reference's answers on the fixture."""
import os
import subprocess

import numpy as np
import pytest

import netflow_amd as nf
from egress_acl_common import NONE, Fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "egress_acl_test.cpp")


@pytest.mark.gpu
def test_cpp_aclset_upload_and_egress_acl(tmp_path):
    if not os.path.exists(nf.LIB_PATH):
        nf.build()
    exe, libdir = str(tmp_path / "egress_acl_test"), os.path.dirname(nf.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L" + libdir, "-l:" + os.path.basename(nf.LIB_PATH), "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    fx = Fixture()
    z = fx.z
    lines = [f"L {lid} {r.tobytes().hex()}" for lid, r in fx.rules.items()]
    lines += [f"B {port} {lid}" for port, lid in fx.bound.items() if lid != NONE]
    lines += [f"R {fx.deleted}"]
    lines += [f"F {int(p)} {f.hex()}" for p, f in zip(fx.port, fx.frames)]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[:2000] + r.stderr
    out = r.stdout.strip().split("\n")
    n = len(fx.frames)
    rows = np.array([[int(x) for x in ln.split(" ")[1:]] for ln in out[:n]], np.uint32)
    assert all(ln.startswith("F ") for ln in out[:n]) and rows.shape == (n, 4)
    assert np.array_equal(rows[:, 0], z["action"]) and np.array_equal(rows[:, 1], z["rule"])
    assert np.array_equal(rows[:, 2], z["redirect"])
    assert np.array_equal(rows[:, 3], np.where(z["action"] == nf.ACL_DENY, NONE, fx.port))
    tail = {ln.split(" ")[0]: [int(x) for x in ln.split(" ")[1:]] for ln in out[n:]}
    assert tail["I"] == [8, 4, 64]
    drops, nbytes = fx.denied_counters()
    assert tail["P"] == [int(x) for x in drops[:8]] and tail["Y"] == [int(x) for x in nbytes[:8]]
