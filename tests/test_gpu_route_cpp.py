"""The C++ host API's lookup -> forward path (include/netflow_amd/packet.hpp: ChecksumEngine::upload_fib,
route_lookup_batch, then l3_forward_batch with the fib's own next-hop table) over netflow_amd::Packet
objects on the GPU, against the CPU decision of the same tables and the oracle's forward."""
import os
import subprocess

import numpy as np
import pytest

import netflow_amd as nf
import oracle
from route_common import decide_host, fixture_fib, route_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "route_lookup_test.cpp")


@pytest.mark.gpu
def test_cpp_route_lookup_then_forward(tmp_path):
    if not os.path.exists(nf.LIB_PATH):
        nf.build()
    exe, libdir = str(tmp_path / "route_lookup_test"), os.path.dirname(nf.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L" + libdir, "-l:" + os.path.basename(nf.LIB_PATH), "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    z, frames = route_fixture()
    lines = [f"R {r[0]} {r[1]} {r[2]} {r[3]}" for r in z["routes_b"]]
    lines += [f"A {a} {bytes(m).hex()}" for a, m in zip(z["arp_ip"], z["arp_mac"])]
    lines += [f"I {i} {bytes(m).hex()}" for i, m in zip(z["if_id"], z["if_mac"])]
    lines += [f"L {a}" for a in z["local_ip"]]
    lines += [f"F {f.hex()}" for f in frames]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[:2000] + r.stderr
    out = r.stdout.strip().split("\n")
    with fixture_fib(z, "b") as fib:
        want_v, want_nh, want_if = decide_host(fib, frames)
        nht = fib.nexthops_host()
    assert out[0].split()[1] == nht.tobytes().hex()
    rows = [ln.split() for ln in out[1:]]
    assert len(rows) == len(frames)
    assert [int(x[0]) for x in rows] == [int(v) for v in z["verdict_b"]]  # the reference's verdicts
    assert [int(x[1]) for x in rows] == [int(v) for v in want_nh]
    assert [int(x[2]) for x in rows] == [int(v) for v in z["egress_b"]]
    arena, desc = oracle.pack_frames(frames)
    rst = oracle.l3_forward_batch(arena, desc, want_nh, nht.view(np.uint8).reshape(-1, 12))
    assert [int(x[3]) for x in rows] == [int(s) for s in rst]
    assert [x[4] if len(x) > 4 else "" for x in rows] == [f.hex() for f in oracle.unpack_frames(arena, desc)]
    assert sum(1 for s in rst if s & nf.ST_FLAG_FWD) > len(frames) // 4
