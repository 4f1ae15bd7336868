"""Shared by tests/test_rx_scale.py and tests/test_gpu_rx_scale.py: nfcs_switch_rx_device at bursts whose
enqueue has 17 and 129 tiles of 1,024 items, where egress_scan_tiles_kernel walks several tiles per segment and a
second group of 8 (§24), with the expand cut by `cap` and by the copy region, the workspace reused, optional outputs
NULL and the shared scratch growing inside the call.

Tables: switch_common.tables() on a copy of the fixture's dump (tests/golden/switch_ref.npz) whose qos depth column is
raised to `depth`, so that a large burst both enqueues and tail-drops. Frames: the fixture's frames of one ingress port
tiled to n, every frame's last four bytes stamped with its index as the fixture itself does (make_switch_golden.py: no
header reaches into them), so a copy or a TX handle taken from the wrong frame differs in bytes."""
import struct

import numpy as np

import netflow_amd as nf
import dispatch_common as dc
import switch_common as sw
from flood_common import round_up

TILE = 1024                      # items per enqueue tile, frames per expand tile (nfcs_kernels.hip kEgTile, kFloodTile)
SIZES = {17: 4161, 129: 32833}   # tiles of cap = 4 n items -> n frames
ALIGNS = (16, 128)
INGRESS, OTHER = 0, 1            # the fixture's ports with an ingress list; 0 gives every class at least 5%


GROW_PORT, GROW_N = 1023, 8321   # an egress table of 8,192 keys; cap = 4 n = 33,284 items: 33 tiles


def growth_words(n, keys=(GROW_PORT + 1) * nf.QOS_MAX_QUEUES):
    """nfcs_internal.h egress_scratch_words(cap, keys) for the burst's enqueue: tiles x keys + 2 keys."""
    return tiles_of(sw.FANOUT * n) * keys + 2 * keys


def tiles_of(cap):
    return (cap + TILE - 1) // TILE


def scaled_tables(fx, depth):
    z = {k: fx.z[k] for k in fx.z.files}
    z["qos"] = z["qos"].copy()
    z["qos"][:, 3] = np.where(z["qos"][:, 0] != 0, depth, z["qos"][:, 3])
    return sw.tables(z)


def depth_for(n):
    """The queue depth of the scaled tables: a sixty-fourth of the burst, so the busy keys fill and the others do not."""
    return max(1, n // 64)


def frames_of(fx, ingress, n, first=0):
    """n frames: the fixture's burst of `ingress` in turn, frame i stamped with first + i."""
    base = [f for p, _, frames, _ in fx.bursts if p == ingress for f in frames]
    return [base[i % len(base)][:-4] + struct.pack("<I", first + i) for i in range(n)]


def burst(fx, ingress, n, first=0, budget=None):
    """One entry of the bursts list; the dequeue takes n / 16 handles per port unless told otherwise."""
    return (ingress, first, frames_of(fx, ingress, n, first), np.full(fx.num_ports, n // 16 if budget is None else budget, np.uint32))


def profile(fx, t, ingress, copy_align):
    """Per frame of the fixture's burst of `ingress`: (items, bytes of copy slots), from the chain over that burst. The
    tiled bursts repeat it: what a frame yields does not depend on its stamp."""
    base = [(p, 0, frames, budget) for p, _, frames, budget in fx.bursts if p == ingress][:1]
    h = dc.host_switch_rx(t, base, copy_align=copy_align)
    items, n = int(h["totals"][0]["items"]), len(base[0][2])
    isrc, idesc = h["isrc"][0][:items], h["idesc"][0][:items]
    copy_base = len(h["arena"][0]) - sw.region_bytes(base[0][2], copy_align)
    is_copy = idesc["off16"].astype(np.int64) * 16 >= copy_base
    lens = np.array([len(f) for f in base[0][2]], np.int64)[isrc]  # a copy's slot holds the frame as it came in, before the VLAN edit
    slot = (lens + copy_align - 1) // copy_align * copy_align
    return np.bincount(isrc, minlength=n), np.bincount(isrc[is_copy], weights=slot[is_copy], minlength=n).astype(np.int64)


def tight(fx, t, ingress, tiles, copy_align):
    """(n, cap, region) of a burst whose items fill `tiles` enqueue tiles, 65 entries in the last one: cap = 4 n leaves
    the later tiles to padding (a frame yields 1.15 items on average), so this is where the last tile of the scan
    holds items. The region is exactly what the copies need."""
    items, copy_bytes = profile(fx, t, ingress, copy_align)
    cap = tiles * TILE - 959
    reps = cap // max(int(items.sum()), 1) + 2
    cum = np.cumsum(np.tile(items, reps))
    n = int(np.searchsorted(cum, cap, side="right"))
    return n, cap, int(np.tile(copy_bytes, reps)[:n].sum())


def planted(host, copy_align):
    """Where the cut cases cut, from the chain's result for the uncut burst: the last frame flooded to FANOUT ports.
    Returns dict(frame, item: its first item, cap: a capacity that ends after two of its items, region: the bytes of a
    copy region that ends 16 bytes short of the end of its third copy's slot, copy_base)."""
    items = int(host["totals"][0]["items"])
    isrc, idesc, arena_bytes = host["isrc"][0][:items], host["idesc"][0][:items], len(host["arena"][0])
    per = np.bincount(isrc)
    frame = int(np.flatnonzero(per == sw.FANOUT)[-1])
    ks = np.flatnonzero(isrc == frame)
    offs = idesc["off16"][ks].astype(np.int64) * 16
    copy_base = arena_bytes - host["region_bytes"]
    copies = ks[offs >= copy_base]
    third = copies[2]
    end = int(idesc["off16"][third]) * 16 + round_up(int(idesc["len"][third]), copy_align)
    return dict(frame=frame, item=int(ks[0]), cap=int(ks[0]) + 2, region=end - 16 - copy_base, copy_base=copy_base, third=int(third),
                copies=len(copies))


def shares(host, b=0):
    """The conditions on a burst, from the chain's result: the share of the frames in each group of classes, of the
    items with a port that are enqueued / tail-dropped, of the items denied on egress."""
    cls = host["cls"][b]
    n = len(cls)
    share = lambda *c: float(np.isin(cls, c).sum()) / n
    items = int(host["totals"][b]["items"])
    enq = int(host["key_start"][b][-1])
    tail = int(host["key_dropped"][b].sum())
    denied = int(host["denied_pkts"][b].sum()) - (int(host["denied_pkts"][b - 1].sum()) if b else 0)
    with_port = int((host["iport"][b] != nf.IF_NONE).sum())
    return dict(l3=share(nf.SW_L3_FWD), l2=share(nf.SW_L2_FWD), flood=share(nf.SW_L2_FLOOD),
                ingress=share(nf.SW_IN_DENY, nf.SW_RED_OK, nf.SW_RED_DOWN, nf.SW_RED_RANGE), early=share(nf.SW_LLDP, nf.SW_ZERO_MAC, nf.SW_ARP),
                enqueued=enq / max(with_port, 1), tail=tail / max(with_port, 1), denied=denied / max(items, 1), items=items,
                with_port=with_port, enq=enq, tail_n=tail, denied_n=denied)


def host_chain(t, bursts, copy_align=128, **kw):
    """dispatch_common.host_switch_rx, with the bytes of burst 0's copy region added for planted()."""
    res = dc.host_switch_rx(t, bursts, copy_align=copy_align, **kw)
    res["region_bytes"] = dc.per_burst(kw.get("region"), 0, sw.region_bytes(bursts[0][2], copy_align))
    return res


def no_queue_ports(fx):
    """The ports without a QoS configuration: the enqueue drops their items without a key (EQ_DROP_NO_CONFIG): neither enqueued nor counted in key_dropped."""
    return np.flatnonzero(fx.z["qos"][:, 0] == 0)


def identities(got, n, keys_per_port, skip_ports, b=0):
    """The conservation identities of one burst, from the device's own arrays alone. skip_ports: no_queue_ports()."""
    cls, tot = got["cls"][b], got["totals"][b]
    items = int(tot["items"])
    ingress_rx = got["rx_stats"][b]
    drops = int(np.isin(cls, dc.DROPS).sum())
    before = got["rx_stats"][b - 1] if b else np.zeros_like(ingress_rx)
    assert int(ingress_rx["rx_packets"].sum() - before["rx_packets"].sum()) == n + drops, "rx_packets = n + drops"
    per = np.bincount(got["isrc"][b][:items], minlength=n)
    one = np.isin(cls, (nf.SW_L3_FWD, nf.SW_L2_FWD, nf.SW_RED_OK))
    flood = cls == nf.SW_L2_FLOOD
    assert (per[one] == 1).all() and (per[~one & ~flood] == 0).all() and (per[flood] <= sw.FANOUT).all(), "items per class"
    assert int(per[one].sum() + per[flood].sum()) == items == int(tot["items_needed"]), "items = the sum over the classes"
    iport = got["iport"][b]
    assert (iport[items:] == nf.IF_NONE).all()
    with_port = int((iport != nf.IF_NONE).sum())
    denied = int(got["denied_pkts"][b].sum()) - (int(got["denied_pkts"][b - 1].sum()) if b else 0)
    ks, kd = got["key_start"][b].astype(np.int64), got["key_dropped"][b].astype(np.int64)
    enq = int(ks[-1])
    assert items == with_port + denied, "every item keeps its port or is denied on egress"
    skipped = int(np.isin(iport, skip_ports).sum())
    assert with_port == enq + int(kd.sum()) + skipped, "items with a port = enqueued + tail-dropped + on a port without queues"
    order = got["order"][b][:enq]
    assert len(np.unique(order)) == enq and (iport[order] != nf.IF_NONE).all(), "order names every enqueued item once"
    tx, start, txq = got["tx_raw"][b]
    assert len(np.unique(tx)) == len(tx), "a handle was dequeued twice"
    hb, hk = (tx >> 32).astype(np.int64), (tx & 0xFFFFFFFF).astype(np.int64)  # the burst and the item of a handle
    port_of = np.repeat(np.arange(len(start) - 1), np.diff(start.astype(np.int64)))
    assert (hb <= b).all()
    for c in range(b + 1):
        m = hb == c
        assert np.isin(hk[m], got["order"][c][:int(got["key_start"][c][-1])]).all(), "a dequeued handle is no enqueued item"
        assert np.array_equal(got["iport"][c][hk[m]], port_of[m]), "a handle left by another port than its item's"
        assert c == b or not np.isin(tx, got["tx_raw"][c][0]).any(), "a handle was dequeued in an earlier burst already"
    deq = np.bincount(port_of * keys_per_port + txq, minlength=len(ks) - 1)
    d0 = got["depth"][b - 1].astype(np.int64) if b else np.zeros(len(ks) - 1, np.int64)
    assert np.array_equal(got["depth"][b].astype(np.int64), d0 + np.diff(ks) - deq), "depth = before + enqueued - dequeued"


class Scale:
    """The cases both modules share, with the scaled tables and the host chain's results computed once each."""

    def __init__(self):
        self.fx, self.tables, self.hosts = sw.Fixture(), {}, {}
        self.skip_ports = no_queue_ports(self.fx)

    def t(self, depth):
        if depth not in self.tables:
            self.tables[depth] = scaled_tables(self.fx, depth)
        return self.tables[depth]

    def close(self):
        for t in self.tables.values():
            sw.close_tables(t)

    def case(self, kind, tiles, align):
        """(t, bursts, keywords of host_switch_rx / device_switch_rx) of `fits` (cap = 4 n, the issue's sizes), `tight`
        (items up to the last tile), `cap_cut` and `region_cut` (on `fits`'s burst)."""
        n = SIZES[tiles]
        t = self.t(depth_for(n))
        kw = dict(align=align, copy_align=align)
        if kind == "tight":
            n, cap, region = tight(self.fx, t, INGRESS, tiles, align)
            t = self.t(depth_for(n))
            kw.update(cap=cap, region=region)
        bursts = [burst(self.fx, INGRESS, n)]
        if kind in ("cap_cut", "region_cut"):
            p = planted(self.host("fits", tiles, align), align)
            kw.update(cap=p["cap"]) if kind == "cap_cut" else kw.update(region=p["region"])
        return t, bursts, kw

    def host(self, kind, tiles, align):
        key = (kind, tiles, align)
        if key not in self.hosts:
            t, bursts, kw = self.case(kind, tiles, align)
            self.hosts[key] = host_chain(t, bursts, cut=kind.endswith("_cut"), **kw)
        return self.hosts[key]


FITS = [(17, 16), (17, 128), (129, 16), (129, 128)]
TIGHT = [(17, 16), (17, 128), (129, 16)]
CUTS = [(17, 16), (17, 128), (129, 128)]


def growth_tables(fx, depth):
    """The scaled tables with egress port GROW_PORT configured: 1,024 ports, 8,192 keys, and a histogram of tiles x
    keys words, past the 2^18 words the scratch starts with from 31 tiles on."""
    t = scaled_tables(fx, depth)
    t["eg"].set_port(GROW_PORT, has_vlan_config=False, has_qos=True, num_queues=nf.QOS_MAX_QUEUES, max_queue_depth=depth)
    t["eg"].commit()
    return t


def growth_burst(fx, n=GROW_N):
    ingress, first, frames, _ = burst(fx, INGRESS, n)
    return (ingress, first, frames, np.full(GROW_PORT + 1, n // 16, np.uint32))
