"""The C++ host API's egress path (include/netflow_amd/packet.hpp: make_egress_from,
ChecksumEngine::upload_egress, egress_plan_batch, vlan_batch with the plan's edits, egress_enqueue_batch)
over netflow_amd::Packet objects on the GPU, against the reference's results on the fixture burst."""
import os
import subprocess

import numpy as np
import pytest

import netflow_amd as nf
from egress_common import egress_fixture, fixture_want

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "egress_test.cpp")


@pytest.mark.gpu
def test_cpp_make_egress_plan_vlan_enqueue(tmp_path):
    if not os.path.exists(nf.LIB_PATH):
        nf.build()
    exe, libdir = str(tmp_path / "egress_test"), os.path.dirname(nf.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L" + libdir, "-l:" + os.path.basename(nf.LIB_PATH), "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    z, frames = egress_fixture()
    want = fixture_want(z)
    lines = [f"P {bytes(p).hex()}" for p in z["ports"]]
    lines += [f"D {k} {int(d)}" for k, d in enumerate(want["depth0"]) if d]
    lines += [f"F {int(p)} {f.hex()}" for p, f in zip(z["port"], frames)]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[:2000] + r.stderr
    out = r.stdout.strip().split("\n")
    n, keys = len(frames), want["keys"]
    rows = [ln.split(" ") for ln in out[:n]]
    assert all(row[0] == "F" and len(row) == 5 for row in rows)
    assert np.array_equal(np.array([int(row[1]) for row in rows], np.uint32), want["ops"])
    assert np.array_equal(np.array([int(row[2]) for row in rows], np.uint8), want["queue"])
    assert np.array_equal(np.array([int(row[3]) for row in rows], np.uint8), want["result"])
    for i, row in enumerate(rows):  # the bytes and lengths after process_egress
        assert bytes.fromhex(row[4]) == bytes(z["frames_out"][i, :int(z["lens_out"][i])]), i
    tail = {ln.split(" ")[0]: np.array([int(x) for x in ln.split(" ")[1:]], np.uint32) for ln in out[n:]}
    assert set(tail) == {"K", "O", "X", "Z"} and len(tail["K"]) == keys + 1
    for tag, name in (("K", "key_start"), ("O", "order"), ("X", "key_dropped"), ("Z", "depth")):
        assert np.array_equal(tail[tag], want[name]), name
