"""CPU tests of the value-edge frames (tests/value_edge_common.py): the oracle against what the
reference recorded for every crafted frame and operation (tests/golden/value_edges_ref.npz), each tuned class's
share of each burst, a plain-Python-integer restatement of Packet::calculate_checksum against the oracle's sum on
the saturated regions, and the ICMP responder's host walk on the requests whose replies carry the values."""
import os

import numpy as np
import pytest

import netflow_amd as nf
import oracle
import value_edge_common as ve
from icmp_common import small_tables

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "value_edges_ref.npz")


def oracle_run(op, f):
    if op == "upd":
        out, st = oracle.update_frame(f)
        return st, out
    if op == "fwd":
        out, st = oracle.l3_forward_frame(f, bytes(ve.NH_TABLE[1]))
        return (1 if st & nf.ST_FLAG_FWD else 0), out
    out, st, _ = oracle.vlan_frame(f, ve.PUSH_OP if op == "push" else ve.POP_OP, len(f) + 4)
    return (0 if st == 16 else 1), out  # 16: the edit was refused (no room, nothing to pop)


def test_oracle_equals_the_reference_on_every_frame_and_operation():
    z = np.load(GOLD)
    got = ve.record(oracle_run)
    assert int(z["n"]) == len(ve.named_frames()) >= 2000 and int(z["seed"]) == ve.SEED
    assert np.array_equal(z["h_in"], got["h_in"]), "the builder no longer makes the frames the fixture was recorded on"
    for op in ve.OPS:
        for k in ("ip", "l4", "len", "hash"):
            assert np.array_equal(z[f"{op}_{k}"], got[f"{op}_{k}"]), (op, k)
        ret = z[f"{op}_ret"]
        assert np.array_equal(ret if op == "upd" else (ret != 0), got[f"{op}_ret"] if op == "upd" else (got[f"{op}_ret"] != 0)), op
    # the fixture holds the values the frames were made for: the reference itself wrote them
    names = list(ve.named_frames())
    want = {"udp4_zero_to_ffff": ("upd_l4", 0xFFFF), "udp6_zero_to_ffff": ("upd_l4", 0xFFFF), "tcp_zero": ("upd_l4", 0),
            "icmp_zero": ("upd_l4", 0), "ip_zero": ("upd_ip", 0), "ip_zero:fwd": ("fwd_ip", 0), "icmp_sum_zero": ("upd_l4", 0xFFFF),
            "ip_zero_and_udp_ffff": ("upd_ip", 0), "ip_zero_and_udp_ffff:fwd": ("fwd_ip", 0)}
    seen = dict.fromkeys(want, 0)
    for i, nm in enumerate(names):
        slot = nm.split("/")[1]
        if slot in want:
            key, v = want[slot]
            assert int(z[key][i]) == v, (nm, key, hex(int(z[key][i])))
            if slot.startswith("ip_zero_and"):
                assert int(z[key[:4] + "l4"][i]) == 0xFFFF, nm
            seen[slot] += 1
    assert min(seen.values()) >= 12, seen
    # the forward and the edits keep those L4 values: push and pop move the region, they do not change its sum
    for i, nm in enumerate(names):
        if nm.split("/")[1] in ("tcp_zero", "icmp_zero") and "ihl3" not in nm and "ihl4" not in nm:
            tagged = "/t-" in nm  # a pop without a tag is refused: the stale field stays
            assert int(z["push_l4"][i]) == 0 and int(z["pop_l4"][i]) == (0 if tagged else 0xFFFF), nm
    sat = [i for i, nm in enumerate(names) if nm.startswith("sat/max")]
    assert len(sat) == 8 and all(int(z["upd_l4"][i]) >= 0 for i in sat)


@pytest.mark.parametrize("kind", ["tiny", "short", "long", "deferred"])
def test_every_class_has_its_share_of_every_burst(kind):
    names, frames = ve.burst_names(kind), ve.burst_frames(kind)
    assert len(frames) == (ve.DEFERRED_N if kind == "deferred" else ve.BURST_N)
    arena, desc = oracle.pack_frames(frames)
    ref = arena.copy()
    st, _ = oracle.update_batch(ref, desc, nthreads=8)
    sh = ve.shares(names, frames, oracle.unpack_frames(ref, desc), st)
    print(kind, "update", {k: round(v, 3) for k, v in sh.items()})
    for c in ve.CLASSES:
        assert sh[c] >= 0.05, (kind, c, sh[c])
    fwd = arena.copy()
    fst = oracle.l3_forward_batch(fwd, desc, ve.nh_index(len(desc)), ve.NH_TABLE)
    keep = (fst & nf.ST_FLAG_FWD) != 0
    assert 0.6 < keep.mean() < 0.8
    sh = ve.shares(names, frames, oracle.unpack_frames(fwd, desc), fst & 0x7F, keep)
    print(kind, "forwarded", {k: round(v, 3) for k, v in sh.items()})
    for c in ve.CLASSES:
        if c != "udp6_zero_to_ffff":  # the IPv4 forward leaves IPv6 frames as they are
            assert sh[c] >= 0.05, (kind, c, sh[c])
    assert {f[ve.geom(f)["l2"] + 8] for f in frames[:600] if ve.geom(f)["v4"]} >= set(ve.TTLS)


def regions():
    """(what, bytes): the L4 regions and IPv4 headers of the saturated frames, and random ones of every length class."""
    out = []
    for nm, f in ve.saturated_frames().items():
        g = ve.geom(f)
        out.append((nm, f[g["l4"]:g["re"]]))
        if g["v4"]:
            out.append((nm + "/ip", f[g["l2"]:g["l4"]]))
    rng = np.random.default_rng(ve.SEED)
    for n in list(range(0, 70)) + [1499, 1500, 9000, 9001, 65515, 65535]:
        out.append((f"random {n}", rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
        out.append((f"ff {n}", b"\xff" * n))
    return out


def test_python_integer_sum_equals_the_oracle_sum():
    """Python integers cannot overflow: where the oracle's 32-bit accumulation agrees with them on the saturated
    regions (65,535 bytes of 0xFF: the largest sum a region can have), its accumulator did not wrap. The last byte
    of an odd region counts as the LOW byte of its word, as the reference counts it (an RFC 1071 sum gives 0x00FF
    on the saturated 65,515-byte ICMP region where the reference gives 0xFF00)."""
    L = oracle.lib()
    top = 0
    for what, r in regions():
        buf = np.frombuffer(bytes(r) + bytes(2), np.uint8).copy()
        assert L.nfo_calculate_checksum(oracle._ptr(buf), len(r)) == ve.py_checksum(r), what
        top = max(top, ve.py_sum(r))
    assert top == 32767 * 0xFFFF + 0xFF  # 65,535 bytes of 0xFF
    f = ve.saturated_frames()["sat/max-v4-p1-u"]
    odd = bytearray(f[34:])  # the 65,515-byte ICMP region, its field as zero
    odd[2] = odd[3] = 0
    rfc = ve.py_finish(ve.py_sum(odd[:-1]) + (odd[-1] << 8))
    assert len(odd) == 65515 and (ve.py_checksum(odd), rfc) == (0xFF00, 0x00FF)
    # whole frames: pseudo-header and region, the exact sum past 2^31 for IPv6 and just below for IPv4
    sat = ve.saturated_frames()
    s6, s4 = ve.l4_exact_sum(sat["sat/max-v6-p17-u"]), ve.l4_exact_sum(sat["sat/max-v4-p17-u"])
    assert s6 > 1 << 31 and (1 << 31) - (1 << 20) < s4 < 1 << 31, (hex(s6), hex(s4))
    for nm, f in sat.items():
        g = ve.geom(f)
        out, st = oracle.update_frame(f)
        c = ve.py_finish(ve.l4_exact_sum(f))
        assert ve.get16(out, g["l4_f"]) == (0xFFFF if g["proto"] == 17 and c == 0 else c), nm
        if g["v4"]:
            assert ve.get16(out, g["ip_f"]) == ve.py_finish(ve.ip_exact_sum(f)), nm


def test_python_integer_sum_on_the_tuned_frames():
    for nm, f in ve.named_frames().items():
        g = ve.geom(f)
        if g["overlap"]:
            continue
        out, st = oracle.update_frame(f)
        c = ve.py_finish(ve.l4_exact_sum(f))
        assert ve.get16(out, g["l4_f"]) == (0xFFFF if g["proto"] == 17 and c == 0 else c), nm
        if g["v4"]:
            assert ve.get16(out, g["ip_f"]) == ve.py_finish(ve.ip_exact_sum(f)), nm


def test_icmp_replies_carry_the_values():
    fib, icmp = small_tables()
    with fib, icmp:
        cases = ve.icmp_cases(icmp, fib)
        count = {}
        for cls, f, verdict, ip_id in cases:
            m = ve.reply_of(icmp, fib, f, verdict, ip_id)
            # both fields, recomputed over the message's own bytes by the Python sum
            hdr, body = bytearray(m[14:34]), bytearray(m[34:])
            hdr[10] = hdr[11] = body[2] = body[3] = 0
            assert ve.get16(m, 24) == ve.py_checksum(hdr), cls
            assert ve.get16(m, 36) == ve.py_checksum(body), cls
            s = ve.py_sum(body)
            if cls == "icmp_zero":
                assert ve.get16(m, 36) == 0x0000
            elif cls == "icmp_sum_zero":
                assert ve.get16(m, 36) == 0xFFFF and s == 0 and not any(body)
            elif cls == "second_fold":
                assert ve.first_fold(s) >= 0x10000
            elif cls == "second_fold_le":
                assert ve.first_fold(ve.le_sum(body)) >= 0x10000
            elif cls == "odd_tail_ff":
                assert len(m) & 1 and m[-1] == 0xFF
            elif cls == "saturated":
                assert set(m[42:]) == {0xFF}
            else:
                assert m[34] == 11 and ve.get16(m, 18) in (0xFFFF, 0xFF00 + 0, 0xFF02, 0xFF04, 0xFF06)
            assert oracle.update_frame(m)[0] == m  # update_checksums() changes nothing
            count[cls] = count.get(cls, 0) + 1
        assert count == {"icmp_zero": 16, "icmp_sum_zero": 8, "second_fold": 16, "second_fold_le": 16, "odd_tail_ff": 8, "saturated": 2001,
                         "saturated_error": 14}, count
        lens = {len(ve.reply_of(icmp, fib, f, v, i)) for c, f, v, i in cases if c == "second_fold"}
        assert {(n - 1) % 16 for n in lens} == set(range(16))
