"""The yardsticks of the burst-scale GPU tests, checked without a GPU: the sequential host walks
Egress.enqueue_host, Fdb.flood_expand_host and Icmp.respond_host equal the numpy models of burst_scale_common.py,
which share no code with them, at every size and pattern tests/test_gpu_burst_scale.py runs; every burst holds the
shares of each class that the GPU tests rely on; and every cut case cuts where it says."""
import os
import re

import numpy as np
import pytest

import burst_scale_common as bs
import netflow_amd as nf
from egress_common import assert_same as assert_same_enqueue
from flood_common import assert_same_expand, model_flood_ports
from icmp_common import small_tables

T = bs.T
FLOOD_SIZES = [(t, False) for t in bs.SCAN_TILES] + [(256, True)]
ICMP_SIZES = [(256, True), (257, False), (513, False)]
CASES = ["full", "cap_cut", "region_cut"]


def test_the_tile_counts_follow_the_kernels_constants():
    src = open(os.path.join(nf.HERE, "csrc", "nfcs_kernels.hip")).read()
    assert int(re.search(r"constexpr uint32_t kEgSegs = (\d+);", src).group(1)) == bs.EG_SEGS
    assert int(re.search(r"constexpr uint32_t kFloodScanThreads = (\d+);", src).group(1)) == bs.SCAN
    assert f"for (uint32_t t = t0; t < t1; t += {bs.EG_GROUP}u)" in src and f"uint32_t v[{bs.EG_GROUP}];" in src
    per = {t: bs.eq_segments(t)[0] for t in bs.EQ_TILES}
    assert per == {16: 1, 17: 2, 33: 3, 128: 8, 129: 9, 137: 9, 145: 10, 257: 17}
    held = {t: sum(1 for a, b in bs.eq_segments(t)[1] if b > a) for t in bs.EQ_TILES}
    assert held == {16: 16, 17: 9, 33: 11, 128: 16, 129: 15, 137: 16, 145: 15, 257: 16}
    assert bs.eq_last_segment(129) == (126, 129) and bs.eq_last_segment(145) == (140, 145)
    assert 15 * per[145] > 145  # the kernel's seg * per passes `tiles`: only min(seg * per, tiles) keeps t0 in range
    assert [(-(-t // bs.SCAN)) for t in bs.SCAN_TILES] == [1, 1, 2, 2, 3]


# ---- the enqueue -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table,tiles,exact", bs.EQ_RANDOM_CASES)
def test_enqueue_host_equals_model_random(table, tiles, exact):
    rows, port, queue, depth = bs.eq_random_case(table, tiles, exact)
    assert len(port) == tiles * T - (0 if exact else 959)
    model = bs.eq_model(port, queue, depth, *bs.eq_port_arrays(rows))
    with bs.make_egress(rows) as eg:
        assert eg.keys()[1] == len(depth)
        host = eg.enqueue_host(port, queue, depth)
    assert_same_enqueue(host, model, f"{table} {tiles}: ")
    # all five results occur, and the key in use most has packets in every tile
    assert set(model["result"].tolist()) == {nf.EQ_ENQUEUED, nf.EQ_SKIP, nf.EQ_DROP_NO_CONFIG, nf.EQ_DROP_FULL, nf.EQ_BAD_QUEUE}
    keyed = np.isin(model["result"], (nf.EQ_ENQUEUED, nf.EQ_DROP_FULL))
    key = port.astype(np.int64) * bs.Q + queue
    hot = np.bincount(key[keyed]).argmax()
    assert len(np.unique(np.flatnonzero(keyed & (key == hot)) // T)) == tiles
    if table == "keys65":
        assert len(np.unique(key[keyed])) == 65 and key[keyed].max() == 64
    if table == "keys64":
        assert len(np.unique(key[keyed])) == 64
    if table == "one_key":
        assert len(np.unique(key[keyed])) == 1


@pytest.mark.parametrize("pattern", bs.EQ_PATTERNS)
@pytest.mark.parametrize("tiles", bs.EQ_PATTERN_TILES)
def test_enqueue_host_equals_model_patterns(tiles, pattern):
    port, queue, depth, meta = bs.eq_pattern(tiles, pattern)
    rows = bs.eq_table("small12")
    model = bs.eq_model(port, queue, depth, *bs.eq_port_arrays(rows))
    with bs.make_egress(rows) as eg:
        host = eg.enqueue_host(port, queue, depth)
    assert_same_enqueue(host, model, f"{pattern} {tiles}: ")
    keyed = np.isin(model["result"], (nf.EQ_ENQUEUED, nf.EQ_DROP_FULL))
    key = np.where(keyed, port.astype(np.int64) * bs.Q + queue, -1)
    mine = np.flatnonzero(key == meta["key"])
    assert np.array_equal(mine, np.flatnonzero(meta["put"]))
    per, segs = bs.eq_segments(tiles)
    last = bs.eq_last_segment(tiles)
    other = np.bincount(np.flatnonzero(keyed & (key != meta["key"])) // T, minlength=tiles)
    assert (other > 0).all()  # every tile holds packets of other keys
    k = meta["key"]
    if pattern == "late_key":
        assert set(np.unique(mine // T).tolist()) == set(range(*last)) and last[0] > 0
        assert model["key_dropped"][k] == 0 and model["key_start"][k + 1] - model["key_start"][k] == len(mine)
    elif pattern == "gap_key":
        lo, hi = meta["gap"]
        assert (lo, hi) == (3 * per, 10 * per)
        assert set(np.unique(mine // T).tolist()) == set(range(tiles)) - set(range(lo, hi))
    else:
        cut, nxt = meta["cut"], meta["next"]
        assert model["result"][cut] == nf.EQ_ENQUEUED and model["result"][nxt] == nf.EQ_DROP_FULL
        assert (model["result"][mine[mine <= cut]] == nf.EQ_ENQUEUED).all()
        assert (model["result"][mine[mine > cut]] == nf.EQ_DROP_FULL).all() and (mine > cut).sum() >= 10
        assert model["key_start"][k + 1] - model["key_start"][k] == meta["room"] and model["depth"][k] == 100000
        full = bs.eq_last_full_segment(tiles)
        assert full[1] - full[0] == per > bs.EG_GROUP
        if pattern == "room_cut_group2":  # a tile of the second 8-group of a segment of per > 8 tiles
            assert cut // T == full[0] + bs.EG_GROUP < full[1] and nxt // T == cut // T
        elif pattern == "room_cut_seg_last":  # the key's next packet is the next segment's first
            assert cut // T == full[1] - 1 and nxt // T == full[1]
        else:  # a tile of the last segment that holds one
            assert last[0] <= cut // T < last[1] and cut // T == tiles - 1 and last[0] >= full[1]


# ---- flood replication ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fdb():
    with bs.make_fdb() as f:
        yield f, bs.flood_lists(f)


def test_flood_lists_are_the_restatements(fdb):
    f, lists = fdb
    ports = []
    for p in range(bs.FLOOD_PORTS):
        rec = np.zeros(1, nf.L2_PORT_DTYPE)[0]
        rec["port_id"], rec["link_up"], rec["stp_forwarding"], rec["has_vlan_config"] = p, 1, 1, 1
        rec["type"], rec["native_vlan"] = (nf.L2_ACCESS, 10) if 1 <= p <= 5 else (nf.L2_TRUNK, 1)
        ports.append((rec, {0: [10, 20, 30], 6: [10, 20], 7: [20]}.get(p, [])))
    for v in bs.FLOOD_VLANS:
        assert lists[v].tolist() == model_flood_ports(ports, bs.FLOOD_INGRESS, v, bs.FLOOD_PORTS), v
    assert [len(lists[v]) for v in bs.FLOOD_VLANS] == [6, 2, 0, 0]


@pytest.mark.parametrize("tiles,exact", FLOOD_SIZES)
def test_flood_host_equals_model(fdb, tiles, exact):
    f, lists = fdb
    b = bs.flood_burst(tiles, exact)
    n = b["n"]
    assert n == tiles * T - (0 if exact else 959) and len(b["frames"]) == 64 * n <= b["copy_base"]
    share = lambda m: m.sum() / n  # noqa: E731
    uni = b["uni_port"] != bs.NONE
    assert share(b["flood"]) >= 0.05 and share(uni) >= 0.05 and share(~b["flood"] & ~uni) >= 0.05
    per_tile = np.bincount(np.flatnonzero(b["flood"] | uni) // T, minlength=tiles)
    assert (per_tile > 0).all()  # every tile holds items
    for align in (16, 128):
        for case in CASES:
            arena_bytes, cap, p = bs.flood_case(b, lists, align, case)
            model = bs.flood_model(b, lists, align, arena_bytes, cap)
            host = f.flood_expand_host(bs.FLOOD_INGRESS, bs.FLOOD_PORTS, arena_bytes, b["copy_base"], align, b["desc"], cap,
                                       **b["arrays"])
            assert_same_expand(host, model, f"{tiles} {align} {case}: ")
            t = model["totals"]
            items, needed = int(t["items"]), int(t["items_needed"])
            if case == "full":
                assert items == needed == cap - 3 and int(t["copy_bytes"]) == int(t["copy_bytes_needed"])
                assert int(t["copies"]) > n // 5
                continue
            # the cut lies inside the items of packet p of the burst's last tile: three of its six items are in
            assert p // T == tiles - 1 and (tiles <= bs.SCAN or p // T >= bs.SCAN) and model["cnt"][p] == 6
            assert items == int(model["k0"][p]) + (3 if case == "cap_cut" else 2) < needed
            assert (model["item_src"][items - 2:items] == p).all() and model["item_flood"][items - 1]
            assert (case == "cap_cut") == (items == cap)
            if case == "region_cut":  # the region ends inside the third copy's slot
                third = b["copy_base"] + int(model["b0"][p]) + 2 * int(model["slot"][p])
                assert third < arena_bytes < third + int(model["slot"][p])


# ---- the ICMP responder ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def icmp_tables():
    fib, icmp = small_tables()
    with fib, icmp:
        yield fib, icmp


@pytest.mark.parametrize("tiles,exact", ICMP_SIZES)
def test_icmp_host_equals_model(icmp_tables, tiles, exact):
    fib, icmp = icmp_tables
    b = bs.icmp_burst(tiles, exact)
    n = b["n"]
    share = lambda c: (b["cls"] == c).sum() / n  # noqa: E731
    assert share("echo") >= 0.05 and share("ttl") >= 0.05 and share("noroute") >= 0.05 and share("none") >= 0.2
    assert (np.bincount(np.flatnonzero(b["msg_len"] > 0) // T, minlength=tiles) > 0).all()  # every tile holds messages
    want_status = {"echo": nf.ICMP_ST_ECHO_REPLY, "ttl": nf.ICMP_ST_TIME_EXCEEDED, "noroute": nf.ICMP_ST_UNREACHABLE}
    for align in (16, 128):
        for case in CASES:
            arena_bytes, cap, p = bs.icmp_case(b, align, case)
            model = bs.icmp_model(b, align, arena_bytes, cap)
            arena = bs.with_region(b["frames"], b["msg_base"], arena_bytes)
            host = icmp.respond_host(fib, bs.ICMP_INGRESS, arena, b["msg_base"], align, b["desc"], b["verdict"], cap,
                                     ip_id=b["ip_id"])
            what = f"{tiles} {align} {case}: "
            for k in ("messages", "messages_needed", "echo_replies", "errors", "msg_bytes", "msg_bytes_needed"):
                assert int(host["totals"][k]) == int(model["totals"][k]), what + k
            assert np.array_equal(host["msg_desc"], model["msg_desc"]), what + "msg_desc"
            assert np.array_equal(host["msg_src"], model["msg_src"]), what + "msg_src"
            m = int(model["totals"]["messages"])
            assert (host["msg_port"][:m] == 1).all() and (host["msg_port"][m:] == nf.IF_NONE).all()
            # the statuses: the template's own, OVERFLOW from the cut on
            for c, st in want_status.items():
                sel = (b["cls"] == c) & ~model["overflow"]
                assert (host["status"][sel] == st).all(), what + c
            assert (host["status"][model["overflow"]] == nf.ICMP_ST_OVERFLOW).all()
            quiet = host["status"][b["cls"] == "none"]
            assert set(quiet.tolist()) == {nf.ICMP_ST_NONE, nf.ICMP_ST_TO_CPU, nf.ICMP_ST_IGNORED, nf.ICMP_ST_SRC_NO_ROUTE}
            assert np.array_equal(arena[:b["msg_base"]], bs.with_region(b["frames"], b["msg_base"], b["msg_base"]))
            if case == "full":
                assert m == int(model["totals"]["messages_needed"]) == cap - 3 and not model["overflow"].any()
                continue
            assert p // T == tiles - 1 and (tiles <= bs.SCAN or p // T >= bs.SCAN)
            assert model["overflow"][p] and not model["overflow"][:p].any() and m == int(model["index"][p])
            assert model["overflow"].sum() >= 3 and (case == "cap_cut") == (m == cap)
            if case == "region_cut":
                at = b["msg_base"] + int(model["off"][p])
                assert at < arena_bytes < at + int(model["slot"][p])
