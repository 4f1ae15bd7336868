"""Shared inputs for the L2 tests: the reference-made fixture tests/golden/l2_ref.npz
(tests/golden/make_l2_golden.py), an Fdb built from its entries and ports, the decision of
Fdb.lookup_host over a list of frames, a dict restatement of the L2 block (switch.hpp:305-326) that shares
no code with the library, and the search for a table whose probe sequences wrap."""
import os

import numpy as np

import netflow_amd as nf

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RUNS = (0, 1, 2)  # ingress = an ACCESS port, a TRUNK port, a port without a VLAN config
WRAP_SEED_LIMIT = 200


def l2_fixture():
    z = np.load(os.path.join(GOLD, "l2_ref.npz"))
    frames = [bytes(z["frames"][i, :int(ln)]) for i, ln in enumerate(z["lens"])]
    return z, frames


def fixture_ports(z):
    """[(L2_PORT_DTYPE record, allowed VLANs)] as the fixture configured them."""
    ports = np.ascontiguousarray(z["ports"]).view(nf.L2_PORT_DTYPE).reshape(-1)
    return [(p, [int(v) for v in z["allowed"][i, :int(z["allowed_n"][i])]]) for i, p in enumerate(ports)]


def set_ports(fdb: nf.Fdb, ports):
    for p, allowed in ports:
        fdb.set_port(int(p["port_id"]), int(p["link_up"]), int(p["stp_forwarding"]), int(p["has_vlan_config"]),
                     int(p["type"]), int(p["native_vlan"]), allowed)
    return fdb


def fixture_fdb(z) -> nf.Fdb:
    entries = np.ascontiguousarray(z["entries"]).view(nf.FDB_ENTRY_DTYPE).reshape(-1)
    return set_ports(nf.Fdb().set_entries(entries), fixture_ports(z)).commit()


def entries_of(macs, vlans, ports, static=None) -> np.ndarray:
    """FDB_ENTRY_DTYPE records from a (n, 6) u8 array and per-entry VLANs / ports / static flags."""
    e = np.zeros(len(macs), dtype=nf.FDB_ENTRY_DTYPE)
    e["mac"], e["vlan_id"], e["port"] = macs, vlans, ports
    e["is_static"] = 0 if static is None else static
    return e


def frame_of(dmac, smac, vlan=None, length=64) -> bytes:
    """A non-IP frame; vlan None = untagged."""
    b = bytearray(max(length, 18))
    b[0:6], b[6:12] = bytes(dmac), bytes(smac)
    b[12:14] = b"\x88\xb5"
    if vlan is not None:
        b[12:14], b[14:16], b[16:18] = b"\x81\x00", (0xA000 | vlan).to_bytes(2, "big"), b"\x88\xb5"
    return bytes(b[:length])


def decide_host(fdb: nf.Fdb, ingress: int, frames):
    """verdict (u8), egress port (u32), VLAN (u16), learn class (u8) per frame, on the CPU."""
    n = len(frames)
    v, e, vl, le = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    for i, f in enumerate(frames):
        v[i], e[i], vl[i], le[i] = fdb.lookup_host(ingress, f)
    return v, e, vl, le


def model_decide(entries, ports, ingress: int, frames):
    """The same four arrays from a dict restatement: the first entry per (mac, vlan) as find_if returns it,
    the port state by id with the reference's defaults, should_forward from the configs."""
    table = {}
    for e in entries:
        table.setdefault((bytes(e["mac"]), int(e["vlan_id"])), (int(e["port"]), bool(e["is_static"])))
    cfg = {int(p["port_id"]): (p, set(allowed)) for p, allowed in ports}

    def state(port, field):
        return port in cfg and bool(cfg[port][0][field])

    def allows(port, vlan):
        if not state(port, "has_vlan_config"):
            return False
        p, allowed = cfg[port]
        return vlan == int(p["native_vlan"]) if int(p["type"]) == nf.L2_ACCESS else vlan in allowed

    native = int(cfg[ingress][0]["native_vlan"]) if state(ingress, "has_vlan_config") else 1
    n = len(frames)
    v, eg = np.zeros(n, np.uint8), np.full(n, nf.IF_NONE, np.uint32)
    vl, le = np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    for i, f in enumerate(frames):
        if len(f) < 14:
            v[i] = nf.L2_NO_ETH
            continue
        vlan = int.from_bytes(f[14:16], "big") & 0xFFF if f[12:14] == b"\x81\x00" and len(f) >= 18 else native
        vl[i] = vlan
        hit = table.get((f[0:6], vlan))
        if hit is None:
            v[i] = nf.L2_FLOOD
        else:
            port = hit[0]
            if port == ingress:
                v[i] = nf.L2_DROP_SAME_PORT
            elif not state(port, "link_up"):
                v[i] = nf.L2_DROP_LINK_DOWN
            elif not state(port, "stp_forwarding"):
                v[i] = nf.L2_DROP_STP
            elif not (allows(ingress, vlan) and allows(port, vlan)):
                v[i] = nf.L2_DROP_VLAN
            else:
                v[i], eg[i] = nf.L2_FORWARD, port
        src = table.get((f[6:12], vlan))
        le[i] = nf.L2_LEARN_NEW if src is None else nf.L2_LEARN_NONE if src[1] else \
            nf.L2_LEARN_REFRESH if src[0] == ingress else nf.L2_LEARN_MOVED
    return v, eg, vl, le


def random_macs(rng, n) -> np.ndarray:
    """n distinct random MACs as a (n, 6) u8 array."""
    m = np.unique(rng.integers(0, 256, size=(2 * n + 8, 6), dtype=np.uint8), axis=0)
    assert len(m) >= n
    return m[rng.permutation(len(m))[:n]]


def wrapping_table(entries_n=30):
    """(seed, macs, vlans, ports) of the first seed below WRAP_SEED_LIMIT whose table of entries_n random
    entries has wrapped > 0 and max_probe >= 3. The bound is asserted."""
    for seed in range(WRAP_SEED_LIMIT):
        rng = np.random.default_rng(9000 + seed)
        macs = random_macs(rng, entries_n)
        vlans = rng.integers(0, 4096, entries_n)
        ports = rng.integers(0, 8, entries_n)
        with nf.Fdb().set_entries(entries_of(macs, vlans, ports)).commit() as fdb:
            st = fdb.stats()
        if st["wrapped"] > 0 and st["max_probe"] >= 3:
            return seed, macs, vlans, ports
    raise AssertionError(f"no table with wrapped > 0 and max_probe >= 3 within {WRAP_SEED_LIMIT} seeds")
