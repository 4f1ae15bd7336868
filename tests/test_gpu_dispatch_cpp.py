"""The C++ host API's ingress dispatch (include/netflow_amd/packet.hpp: ChecksumEngine::upload_fdb,
ingress_dispatch_batch and the free function of that name) over netflow_amd::Packet objects on the GPU: burst 0 of
tests/golden/switch_ref.npz and the hand-built edges, against the Python host result. The counters are compared on
frames longer than the 32 bytes the C++ path stages, which is where they could go wrong."""
import os
import subprocess

import numpy as np
import pytest

import netflow_amd as nf
import dispatch_common as dc
import switch_common as sw
from flood_common import pack_with_tail

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "dispatch_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not os.path.exists(nf.LIB_PATH):
        nf.build()
    out, libdir = str(tmp_path_factory.mktemp("dispatch") / "dispatch_test"), os.path.dirname(nf.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC, "-o", out,
                    "-L" + libdir, "-l:" + os.path.basename(nf.LIB_PATH), "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


def run(exe, ingress, num_ports, link_up, frames, s):
    has_list = s["action"] is not None
    n = len(frames)
    action = s["action"] if has_list else np.zeros(n, np.uint8)
    redirect = s["redirect"] if has_list else np.zeros(n, np.uint32)
    lines = [f"I {ingress}", f"N {num_ports}", f"A {int(has_list)}"]
    for p, up in enumerate(link_up):
        rec = np.zeros(1, nf.L2_PORT_DTYPE)
        rec["port_id"], rec["link_up"], rec["stp_forwarding"], rec["has_vlan_config"], rec["native_vlan"] = p, bool(up), True, True, 1
        lines.append("P " + rec.tobytes().hex())
    for i, f in enumerate(frames):
        lines.append(f"F {s['rt'][i]} {action[i]} {redirect[i]} {s['nh'][i]} {s['l2p'][i]} {s['l2v'][i]} {bytes(f).hex() or '-'}")
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[:2000] + r.stderr
    out = r.stdout.strip().split("\n")
    rx = tuple(int(x) for x in out[0].split()[1:])
    a = np.array([[int(x) for x in ln.split()] for ln in out[1:]], np.int64).reshape(-1, 5)
    assert len(a) == n
    return dict(cls=a[:, 0].astype(np.uint8), bypass=a[:, 1].astype(np.uint8), nh=a[:, 2].astype(np.uint32),
                l2_port=a[:, 3].astype(np.uint32), l2_verdict=a[:, 4].astype(np.uint8)), rx


@pytest.mark.gpu
def test_cpp_ingress_dispatch_batch_on_burst_0(exe):
    fx = sw.Fixture()
    t = sw.tables(fx.z)
    try:
        ingress, _, frames, _ = fx.bursts[0]
        s = dc.stage_inputs(t, ingress, frames)
        arena, desc, copy_base = pack_with_tail(frames, 16, 0)
        rx = np.zeros(t["num_ports"], nf.RX_STATS_DTYPE)
        want = dc.dispatch_host(t, ingress, arena, copy_base, desc, s, rx_stats=rx)
        got, grx = run(exe, ingress, t["num_ports"], t["link_up"], frames, s)
    finally:
        sw.close_tables(t)
    dc.assert_dispatch(got, want, want["cls"])
    assert grx == tuple(int(rx[ingress][k]) for k in rx.dtype.names) and grx[2] > 50
    assert max(len(f) for f in frames) > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("with_list", [True, False])
def test_cpp_ingress_dispatch_batch_on_the_edges(exe, with_list):
    e = dc.Edges()
    s = dict(e.s)
    if not with_list:
        s["action"] = s["redirect"] = None
    cls = e.cls if with_list else e.cls_no_acl
    got, grx = run(exe, dc.EDGE_INGRESS, dc.EDGE_PORTS, [p != dc.EDGE_DOWN for p in range(dc.EDGE_PORTS)], e.frames, s)
    # the C++ path stages each packet's own bytes only: what lies behind a frame in EDGES is zero padding there
    want = e.want(cls, with_acl=with_list)
    dc.assert_dispatch(got, want, cls)
    assert grx == want["rx"]
