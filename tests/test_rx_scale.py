"""CPU checks of the inputs of tests/test_gpu_rx_scale.py: the tile counts follow the kernel's constants,
every burst holds the classes, enqueues, tail drops and egress denies the cases need (conditions on the host chain's
result, not measurements), the cuts lie where the cases say, the scratch growth is triggered by the chosen n, and the
conservation identities hold on the host chain itself."""
import os
import re

import numpy as np
import pytest

import netflow_amd as nf
import rx_scale_common as rs
import switch_common as sw


@pytest.fixture(scope="module")
def sc():
    s = rs.Scale()
    yield s
    s.close()


def test_the_tile_counts_follow_the_kernels_constants():
    src = open(os.path.join(nf.HERE, "csrc", "nfcs_kernels.hip")).read()
    internal = open(os.path.join(nf.HERE, "csrc", "nfcs_internal.h")).read()
    api = open(os.path.join(os.path.dirname(nf.HERE), "include", "nfcs.h")).read()
    assert "constexpr uint32_t kEgTile = NFCS_EGRESS_TILE_PKTS;" in internal
    assert int(re.search(r"#define NFCS_EGRESS_TILE_PKTS (\d+)u", api).group(1)) == rs.TILE
    assert "const uint32_t per = (tiles + kEgSegs - 1u) / kEgSegs;" in src
    segs = int(re.search(r"constexpr uint32_t kEgSegs = (\d+);", src).group(1))
    for tiles, n in rs.SIZES.items():
        assert rs.tiles_of(sw.FANOUT * n) == tiles and n % 2 == 1
    per = {tiles: (tiles + segs - 1) // segs for tiles in rs.SIZES}
    assert per == {17: 2, 129: 9} and 129 // segs == 8 and 17 // segs == 1  # what a floor in the place of the ceiling gives
    # the scratch: tiles x keys + 2 keys words against the 2^18 the first acquire allocates
    assert "return tiles * keys + 2ull * keys;" in internal
    assert rs.growth_words(rs.GROW_N) > 1 << 18 >= rs.growth_words(rs.GROW_N, keys=64)


@pytest.mark.parametrize("kind,tiles,align", [("fits", *c) for c in rs.FITS] + [("tight", *c) for c in rs.TIGHT])
def test_every_burst_holds_what_the_cases_need(sc, kind, tiles, align):
    h = sc.host(kind, tiles, align)
    t, bursts, kw = sc.case(kind, tiles, align)
    n = len(bursts[0][2])
    s = rs.shares(h)
    for k in ("l3", "l2", "flood", "ingress", "early"):
        assert s[k] >= 0.05, f"{k}: {s[k]:.3f} of the frames"
    assert s["enqueued"] >= 0.10 and s["tail"] >= 0.10 and s["denied"] >= 0.01, s
    assert int(h["totals"][0]["items"]) == int(h["totals"][0]["items_needed"])
    # the most used key has items in every enqueue tile that holds items at all
    items, cap = s["items"], kw.get("cap", sw.FANOUT * n)
    assert rs.tiles_of(cap) == tiles
    # the key of every item that reaches the enqueue with a port and a queue: port * 8 + the plan's queue
    iport, iqueue = h["iport"][0][:items].astype(np.int64), h["iqueue"][0][:items].astype(np.int64)
    keyed = (iport != nf.IF_NONE) & (iqueue < nf.QOS_MAX_QUEUES) & ~np.isin(iport, sc.skip_ports)
    item_key = np.where(keyed, iport * nf.QOS_MAX_QUEUES + iqueue, -1)
    ks = h["key_start"][0].astype(np.int64)
    per_key = np.bincount(item_key[keyed], minlength=len(ks) - 1)
    assert np.array_equal(per_key, np.diff(ks) + h["key_dropped"][0]), "the keys are the enqueue's: enqueued + tail-dropped per key"
    key = int(np.argmax(per_key))
    held = rs.tiles_of(items)
    in_tile = np.add.reduceat((item_key == key).astype(np.int64), np.arange(0, items, rs.TILE))
    assert len(in_tile) == held and (in_tile > 0).all(), f"key {key} is absent from tiles {np.flatnonzero(in_tile == 0)}"
    if kind == "tight":
        assert held == tiles and items > (tiles - 1) * rs.TILE and cap - items < sw.FANOUT  # the last tile holds items
        assert int(h["totals"][0]["copy_bytes"]) == kw["region"]                             # and the region is exact
    else:
        assert held < tiles  # cap = 4 n: the later tiles hold padding only, which is why the tight cases exist
    rs.identities(h, n, nf.QOS_MAX_QUEUES, sc.skip_ports)


@pytest.mark.parametrize("tiles,align", rs.CUTS)
def test_the_cuts_lie_where_the_cases_say(sc, tiles, align):
    full = sc.host("fits", tiles, align)
    n = rs.SIZES[tiles]
    p = rs.planted(full, align)
    assert p["frame"] >= (n - 1) // rs.TILE * rs.TILE and p["copies"] >= 3  # in the burst's last tile of frames
    assert int(full["cls"][0][p["frame"]]) == nf.SW_L2_FLOOD
    items = int(full["totals"][0]["items"])
    for kind in ("cap_cut", "region_cut"):
        h = sc.host(kind, tiles, align)
        tot = h["totals"][0]
        assert int(tot["items"]) == p["item"] + 2 < int(tot["items_needed"]) == items, kind
        inert = slice(int(tot["items"]), None)
        assert (h["iport"][0][inert] == nf.IF_NONE).all() and (h["isrc"][0][inert] == nf.ITEM_NONE).all()
        for k in ("idesc", "isrc"):  # what was emitted is what the uncut burst emitted
            assert np.array_equal(h[k][0][:p["item"] + 2], full[k][0][:p["item"] + 2])
    assert len(sc.host("region_cut", tiles, align)["arena"][0]) == p["copy_base"] + p["region"]
    third = full["idesc"][0][p["third"]]
    assert int(third["off16"]) * 16 + rs.round_up(int(third["len"]), align) - 16 == p["copy_base"] + p["region"]
