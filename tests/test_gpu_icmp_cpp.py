"""The C++ host API's ICMP responder (include/netflow_amd/packet.hpp: ChecksumEngine::upload_icmp,
route_lookup_batch, icmp_respond_batch, make_icmp_from) over netflow_amd::Packet objects on the GPU: the fixture's
first run against what the reference sent, and the reference's own ReceiveEchoRequestAndSendReply expectations
(tests/icmp_processor_test.cpp:313-338 of the reference) on a device-built reply."""
import os
import struct
import subprocess

import numpy as np
import pytest

import netflow_amd as nf
from icmp_common import icmp_fixture, run_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "icmp_respond_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not os.path.exists(nf.LIB_PATH):
        nf.build()
    out, libdir = str(tmp_path_factory.mktemp("icmp") / "icmp_respond_test"), os.path.dirname(nf.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC, "-o", out,
                    "-L" + libdir, "-l:" + os.path.basename(nf.LIB_PATH), "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


def run(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[:2000] + r.stderr
    out = r.stdout.strip().split("\n")
    totals = [int(x) for x in out[0].split()[1:]]
    status = [int(x) for x in out[1].split()[1:]]
    msgs = [(int(f[0]), int(f[1]), bytes.fromhex(f[3])) for f in (ln.split() for ln in out[2:]) if int(f[2]) == len(f[3]) // 2]
    assert len(msgs) == len(out) - 2
    return totals, status, msgs


@pytest.mark.gpu
def test_cpp_route_lookup_then_icmp_respond_batch(exe):
    z, frames = icmp_fixture()
    r0 = run_of(z, frames, 0)
    lines = [f"I {r0['ingress']}", f"N {int(z['num_ports'])}"]
    for net, mask, nh, ifid in z["routes"]:
        lines.append("R " + struct.pack("<IIII", int(net), int(mask), int(nh), int(ifid)).hex())
    for ip, m in zip(z["arp_ip"], z["arp_mac"]):
        lines.append("A " + (struct.pack("<I", int(ip)) + bytes(m) + b"\0\0").hex())
    for k, ifid in enumerate(z["if_id"]):
        ips = z["if_ips"][int(z["if_ip_start"][k]):int(z["if_ip_start"][k + 1])]
        lines.append("M " + (struct.pack("<I", int(ifid)) + bytes(z["if_mac"][k]) + b"\0\0").hex())
        lines.append(" ".join([f"C {int(ifid)} {int(z['if_up'][k])} {bytes(z['if_mac'][k]).hex()}"] + [str(int(ip)) for ip in ips]))
        lines += [f"L {int(ip)}" for ip in ips]
    lines += [f"L {int(ip)}" for ip in z["extra_local"]]
    lines += [f"F {int(i)} {f.hex()}" for i, f in zip(r0["ip_id"], r0["frames"])]
    totals, status, msgs = run(exe, lines)
    assert msgs == r0["sent"]  # source, port and every byte, in the reference's order
    ours = np.isin(r0["verdict"], (nf.RT_LOCAL, nf.RT_TTL_EXPIRED, nf.RT_NO_ROUTE))
    assert np.array_equal(np.array(status)[ours], r0["status"][ours]) and not np.array(status)[~ours].any()
    echoes = int((r0["status"] == nf.ICMP_ST_ECHO_REPLY).sum())
    assert totals[:4] == [len(msgs), len(msgs), echoes, len(msgs) - echoes]
    assert totals[4] == sum((len(m) + 15) // 16 * 16 for _, _, m in msgs)


@pytest.mark.gpu
def test_cpp_the_references_echo_reply_expectations(exe):
    """ReceiveEchoRequestAndSendReply: interface 0 = 192.168.0.1 / 00:AA:BB:CC:DD:EE, a request from 192.168.0.100 /
    11:22:33:44:55:66 with identifier 1234, sequence number 1 and the payload "hello"."""
    my_mac, req_mac = bytes.fromhex("00aabbccddee"), bytes.fromhex("112233445566")
    my_ip, req_ip = bytes([192, 168, 0, 1]), bytes([192, 168, 0, 100])
    icmp = struct.pack(">BBHHH", 8, 0, 0, 1234, 1) + b"hello"
    ip = struct.pack(">BBHHHBBH", 0x45, 0, 20 + len(icmp), 0, 0, 64, 1, 0) + req_ip + my_ip
    request = my_mac + req_mac + b"\x08\x00" + ip + icmp
    me = struct.unpack("<I", my_ip)[0]
    lines = ["I 0", "N 4", f"C 0 1 {my_mac.hex()} {me}", f"L {me}", "M " + (struct.pack("<I", 0) + my_mac + b"\0\0").hex(),
             f"F 0 {request.hex()}"]
    totals, status, msgs = run(exe, lines)
    assert status == [nf.ICMP_ST_ECHO_REPLY] and len(msgs) == 1      # ASSERT_TRUE(last_sent_packet_.has_value())
    src, port, reply = msgs[0]
    assert port == 0                                                  # ASSERT_EQ(last_sent_port_, ingress_port)
    assert reply[0:6] == req_mac and reply[6:12] == my_mac            # dst_mac == requester_mac, src_mac == my_mac
    assert reply[12:14] == b"\x08\x00"                                # ethertype IPv4
    assert reply[26:30] == my_ip and reply[30:34] == req_ip           # src_ip == my_ip_net, dst_ip == requester_ip_net
    assert reply[23] == 1                                             # protocol ICMP
    assert reply[34] == 0 and reply[35] == 0                          # TYPE_ECHO_REPLY, code 0
    assert struct.unpack(">HH", reply[38:42]) == (1234, 1)            # identifier, sequence number
    assert len(reply) >= 42 + 5 and reply[42:47] == b"hello"          # the payload
