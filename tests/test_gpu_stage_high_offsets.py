"""Maximum-size addressing in the device stages: a descriptor's off16 counts 16-byte units, so a frame's byte
offset needs 36 bits. Frames past 32 GiB (off16 >= 2^31: a 32-bit byte offset wraps, a signed one goes negative)
through the route lookup, the ACL, the L2 lookup, the egress plan, the egress ACL and the flood expand; waves
whose frames lie 32 GiB apart (even packets at the arena's start, odd ones past 32 GiB, the last wave partial);
flood copies laid out past 32 GiB, so that the item descriptors the expand writes carry off16 >= 2^31, with plan,
VLAN pop and egress ACL over those items; and a copy region that ends inside a packet's copies past 32 GiB.
Outputs equal the host functions' for the same frames; the regions download as the copy model and the oracle's
pops leave them, and the guard behind them untouched. Only the regions are ever uploaded or downloaded."""
import numpy as np
import pytest

import netflow_amd as nf
import oracle
import stage_edge_common as sc
from acl_common import acl_fixture, eval_host, fixture_rules, make_acl, rule
from egress_acl_common import Fixture as EgressAclFixture
from egress_acl_common import host_decision
from egress_common import egress_fixture, plan_host
from egress_common import fixture_egress as plan_fixture_egress
from flood_common import (assert_same_expand, copy_model, fixture_egress, fixture_fdb, fixture_l2_ports, flood_fixture,
                          model_expand, round_up)
from l2_common import decide_host as l2_decide_host
from l2_common import fixture_fdb as l2_fixture_fdb
from l2_common import l2_fixture
from route_common import decide_host as route_decide_host
from route_common import dst_pool, rewrite_dsts

pytestmark = pytest.mark.gpu
BASE = (32 << 30) + 4096  # byte offset of the high region: off16 = 2^31 + 256
LO = 4096                 # byte offset of the low region
GUARD = 1 << 20           # bytes behind the high region (checked untouched)
N = 20001                 # 312 waves and a partial one
MODES = ["high", "split"]


@pytest.fixture(scope="module")
def big(engine):
    b = engine.alloc(BASE + (96 << 20) + GUARD)
    yield b
    b.free()


@pytest.fixture(scope="module")
def T(engine):
    with sc.Tables() as t:
        yield t.upload(engine)


def tiled(a, n=N):
    return [a[i % len(a)] for i in range(n)] if isinstance(a, list) else np.asarray(a)[np.arange(n) % len(a)]


class Placed:
    """Frames in the big arena. mode "high": all past 32 GiB; "low": all at the arena's start; "split": even
    packets low, odd ones high, so every wave spans both. desc holds the device's offsets, cdesc the same
    frames' offsets in `compact`: the regions one after the other as one small host arena."""

    def __init__(self, engine, big, frames, mode):
        self.big, self.n = big, len(frames)
        self.desc = np.zeros(self.n, nf.DESC_DTYPE)
        self.cdesc = np.zeros(self.n, nf.DESC_DTYPE)
        parts = {"high": [(BASE, slice(None))], "low": [(LO, slice(None))], "split": [(LO, slice(0, None, 2)), (BASE, slice(1, None, 2))]}
        self.segs, cbase = [], 0  # (device base, compact base, bytes)
        for dbase, which in parts[mode]:
            arena, d = oracle.pack_frames(frames[which], align=16)
            for dst, base in ((self.desc, dbase), (self.cdesc, cbase)):
                dst["off16"][which] = d["off16"].astype(np.uint64) + base // 16
                dst["len"][which] = d["len"]
            big.upload(arena, dbase)
            self.segs.append((dbase, cbase, arena))
            cbase += round_up(arena.nbytes, 128)
        self.cbytes = cbase
        self.end = max(d + a.nbytes for d, _, a in self.segs)
        assert self.end + GUARD <= big.nbytes and LO + self.segs[0][2].nbytes < BASE
        if mode != "low":
            assert int(self.desc["off16"].max()) >= 1 << 31
            big.upload(np.full(GUARD, sc.GAP, np.uint8), self.end)
        self.arena_bytes = self.end + GUARD
        self.d_desc = sc.up(engine, self.desc, nf.DESC_DTYPE)

    def args(self):
        return self.big, self.arena_bytes, self.d_desc, self.n

    def compact(self):
        c = np.zeros(self.cbytes, np.uint8)
        for _, cb, a in self.segs:
            c[cb:cb + a.nbytes] = a
        return c

    def unchanged(self):
        for dbase, _, a in self.segs:
            assert np.array_equal(self.big.download(np.uint8, a.nbytes, dbase), a), "the call wrote into the frames"
        assert (self.big.download(np.uint8, GUARD, self.end) == sc.GAP).all(), "a store behind the region"
        assert np.array_equal(self.d_desc.download(nf.DESC_DTYPE, self.n), self.desc)
        self.d_desc.free()


# ---- the read-only stages -------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_route_lookup(engine, big, T, mode):
    frames = rewrite_dsts(oracle.fuzz_frames(71, 0, N), dst_pool(), np.random.default_rng(72))
    want = route_decide_host(T.fib, frames)  # table a of the route fixture
    assert (want[0] == nf.RT_FORWARD).mean() > 0.25
    p = Placed(engine, big, frames, mode)
    got = sc.dev_route(engine, T, *p.args())
    p.unchanged()
    sc.same(got, want, ("verdict", "nh", "egress_if"))


@pytest.mark.parametrize("mode", MODES)
def test_acl_eval(engine, big, mode):
    z, fr = acl_fixture()
    frames = tiled(fr)
    with make_acl(fixture_rules(z, "a")) as acl:
        action, first, redirect = (tiled(a) for a in eval_host(acl, fr))
        assert np.array_equal(action, tiled(z["action_a"])) and np.array_equal(first, tiled(z["rule_a"]))
        acl.upload(engine)
        nh_in = np.arange(N, dtype=np.uint32)
        p = Placed(engine, big, frames, mode)
        got = sc.dev_acl(engine, acl, *p.args(), nh_in)
    p.unchanged()
    sc.same(got, (action, first, redirect, np.where(action == nf.ACL_PERMIT, nh_in, nf.NH_NONE)), ("action", "rule", "redirect", "nh"))


@pytest.mark.parametrize("mode", MODES)
def test_l2_lookup(engine, big, mode):
    z, fr = l2_fixture()
    frames, ingress = tiled(fr), int(z["ingress"][0])
    with l2_fixture_fdb(z) as fdb:
        want = tuple(tiled(a) for a in l2_decide_host(fdb, ingress, fr))
        assert np.array_equal(want[0], tiled(z["verdict_0"])) and np.array_equal(want[1], tiled(z["egress_0"]))
        fdb.upload(engine)
        p = Placed(engine, big, frames, mode)
        got = sc.dev_l2(engine, fdb, ingress, *p.args())
    p.unchanged()
    sc.same(got, want, ("verdict", "port", "vlan", "learn"))


@pytest.mark.parametrize("mode", MODES)
def test_egress_plan(engine, big, mode):
    z, fr = egress_fixture()
    frames, ports = tiled(fr), tiled(z["port"].astype(np.uint32))
    with plan_fixture_egress(z) as eg:
        ops, queue = (tiled(a) for a in plan_host(eg, z["port"], fr))
        assert (ops == nf.VLAN_POP).mean() > 0.05 and len(set(queue.tolist())) >= 4
        eg.upload(engine)
        p = Placed(engine, big, frames, mode)
        got = sc.dev_plan(engine, eg, *p.args(), ports)
    p.unchanged()
    sc.same(got, (ports, ops, queue), ("port", "ops", "queue"))


@pytest.mark.parametrize("mode", MODES)
def test_egress_acl(engine, big, mode):
    fx = EgressAclFixture()
    frames, ports = tiled(fx.frames), tiled(fx.port)
    with fx.aclset() as s:
        action, first, redirect = (tiled(a) for a in host_decision(s, fx.port, fx.frames))
        assert np.array_equal(action, tiled(fx.z["action"])) and np.array_equal(first, tiled(fx.z["rule"]))
        nports = s.info()[0]
        s.upload(engine)
        p = Placed(engine, big, frames, mode)
        got = sc.dev_eacl(engine, s, *p.args(), ports, nports)
    p.unchanged()
    gone = action == nf.ACL_DENY
    pk = np.bincount(ports[gone], minlength=nports).astype(np.uint32)
    by = np.bincount(ports[gone], weights=p.desc["len"][gone], minlength=nports).astype(np.uint64)
    assert gone.sum() > 1000
    sc.same(got, (np.where(gone, sc.NONE, ports), action, first, redirect, pk, by),
         ("port", "action", "rule", "redirect", "denied_pkts", "denied_bytes"))


# ---- the flood expand and what runs over its items ------------------------------------------------------------------

class Flood:
    """The flood fixture's burst (run 0, tiled) placed in the big arena, a copy region behind it past 32 GiB."""

    def __init__(self, engine, big, mode, align=16):
        z, fr = flood_fixture()
        self.z, self.engine, self.big, self.align = z, engine, big, align
        self.ingress, self.num_ports = int(z["ingress"][0]), int(z["num_ports"])
        self.arrays = dict(l2_port=tiled(z["egress_0"]).astype(np.uint32), l2_verdict=tiled(z["verdict_0"]).astype(np.uint8),
                           l2_vlan=tiled(z["vlan_0"]).astype(np.uint16))
        self.p = p = Placed(engine, big, tiled(fr), mode)
        self.copy_base = BASE if mode == "low" else round_up(p.end, 128)
        self.ccopy = p.cbytes  # the copy region's place in the compact arena
        self.fdb = fixture_fdb(z)
        self.fdb.upload(engine)
        need = self.host(1 << 40, 1 << 20)["totals"]
        self.cap, self.room = int(need["items_needed"]) + 7, int(need["copy_bytes_needed"])
        assert int(need["copies"]) > 5000 and self.copy_base + self.room + GUARD <= big.nbytes

    def host(self, arena_bytes, cap):
        return self.fdb.flood_expand_host(self.ingress, self.num_ports, arena_bytes, self.copy_base, self.align, self.p.desc, cap,
                                          **self.arrays)

    def to_compact(self, off16):
        """Device off16 of frames and copies -> off16 in the compact arena."""
        off = off16.astype(np.int64) * 16
        out = off.copy()
        for dbase, cbase, a in self.p.segs:
            out = np.where((off >= dbase) & (off < dbase + a.nbytes), off - dbase + cbase, out)
        out = np.where(off >= self.copy_base, off - self.copy_base + self.ccopy, out)
        return (out // 16).astype(np.uint32)

    def expand(self, room):
        """One expand with `room` bytes of copy region (arena_bytes = copy_base + room) and the guard behind them.
        Returns (the host's items, the compact arena as the copy model leaves it, the items' compact descriptors)."""
        arena_bytes = self.copy_base + room
        self.big.upload(np.full(room, sc.FILL, np.uint8), self.copy_base)
        self.big.upload(np.full(GUARD, sc.GAP, np.uint8), arena_bytes)
        want = self.host(arena_bytes, self.cap)
        model = model_expand(fixture_l2_ports(self.z), self.ingress, self.num_ports, arena_bytes, self.copy_base, self.align,
                             self.p.desc, self.cap, **self.arrays)
        assert_same_expand(want, model, "host against model: ")
        got = sc.dev_expand(self.engine, self.fdb, self.ingress, self.num_ports, self.big, arena_bytes, self.copy_base, self.align,
                            self.p.d_desc, self.p.n, self.cap, self.arrays)
        assert_same_expand(got, want)
        m = int(want["totals"]["items"])
        copies = want["item_desc"]["off16"][:m].astype(np.int64) * 16 >= self.copy_base
        assert int(want["totals"]["copies"]) == copies.sum() and (want["item_desc"]["off16"][:m][copies] >= 1 << 31).all()
        cidesc = want["item_desc"].copy()
        cidesc["off16"][:m] = self.to_compact(want["item_desc"]["off16"][:m])
        compact = np.concatenate([self.p.compact(), np.full(room, sc.FILL, np.uint8)])
        after = copy_model(compact, self.p.cdesc, dict(want, item_desc=cidesc), self.ccopy)
        self.check_regions(after, room)
        return want, after, cidesc

    def check_regions(self, compact, room):
        for dbase, cbase, a in self.p.segs:
            assert np.array_equal(self.big.download(np.uint8, a.nbytes, dbase), compact[cbase:cbase + a.nbytes]), "the frames differ"
        back = self.big.download(np.uint8, room + GUARD, self.copy_base)
        assert (back[room:] == sc.GAP).all(), "a store past arena_bytes"
        bad = np.flatnonzero(back[:room] != compact[self.ccopy:self.ccopy + room])
        assert len(bad) == 0, f"the copy region differs from the model at {len(bad)} bytes, the first at {bad[0]}"

    def close(self):
        self.p.d_desc.free()
        self.fdb.close()


def flood_aclset() -> nf.AclSet:
    """Three lists over the flood fixture's frame kinds (VLANs 10 / 20, IPv6, IPv4 and 0x88B5 payloads), port p bound
    to list p % 3, ports 4 and 9 left without one."""
    lists = [np.concatenate([rule(action=nf.ACL_DENY, vlan_id=10), rule(action=nf.ACL_REDIRECT, redirect_port=40, ethertype=0x86DD),
                             rule(action=nf.ACL_DENY, ethertype=0x0800)]),
             np.concatenate([rule(action=nf.ACL_REDIRECT, redirect_port=41, vlan_id=20), rule(action=nf.ACL_DENY, ethertype=0x86DD)]),
             np.concatenate([rule(action=nf.ACL_DENY, ethertype=0x88B5), rule(action=nf.ACL_PERMIT, vlan_id=10),
                             rule(action=nf.ACL_DENY, ethertype=0x86DD)])]
    s = nf.AclSet()
    for k, r in enumerate(lists):
        s.set_list(k, r)
    for p in range(12):
        if p not in (4, 9):
            s.bind_port(p, p % 3)
    return s.commit()


@pytest.mark.parametrize("mode", ["low", "high", "split"])
def test_flood_expand_and_the_stages_over_its_items(engine, big, mode):
    """Copies past 32 GiB from frames at the arena's start, past 32 GiB, and from both in every wave; then
    plan -> VLAN (pops on copies and on frames) -> egress ACL over the item list, whose descriptors carry
    off16 >= 2^31."""
    f = Flood(engine, big, mode)
    want, compact, cidesc = f.expand(f.room)
    tot, cap = want["totals"], f.cap
    m = int(tot["items"])
    assert m == int(tot["items_needed"]) == cap - 7 and int(tot["copy_bytes"]) == f.room
    idesc, iport = want["item_desc"], want["item_port"]
    arena_bytes = f.copy_base + f.room
    # the host: plan, pops and the egress ACL on the compact arena
    item_frames = [bytes(compact[int(d["off16"]) * 16:int(d["off16"]) * 16 + int(d["len"])]) for d in cidesc]
    with fixture_egress(f.z) as eg, flood_aclset() as aclset:
        ops, queue = plan_host(eg, iport, item_frames)
        assert (ops[:m] == nf.VLAN_POP).sum() > 1000
        vst = oracle.vlan_batch(compact, cidesc, ops, None, cap_all=64)
        nports = aclset.info()[0]
        pk, by = np.zeros(nports, np.uint32), np.zeros(nports, np.uint64)
        eacl = aclset.egress_acl_host(compact, cidesc, iport, pk, by)
        assert pk.sum() > 500 and (eacl["action"] == nf.ACL_REDIRECT).sum() > 500 and (eacl["action"] == nf.ACL_PERMIT).sum() > 500
        # the device, over the items the expand left (uploaded again: the expand's own buffers are checked and freed)
        eg.upload(engine)
        aclset.upload(engine)
        d_idesc, d_iport = sc.up(engine, idesc, nf.DESC_DTYPE), sc.up(engine, iport, np.uint32)
        F = lambda size: sc.filled(engine, size * (cap + 1))  # noqa: E731
        d_port, d_ops, d_queue, d_vst, d_ea, d_er, d_ed = F(4), F(4), F(1), F(1), F(1), F(4), F(4)
        d_pk, d_by = sc.up(engine, np.zeros(nports, np.uint32), np.uint32), sc.up(engine, np.zeros(nports, np.uint64), np.uint64)
        engine.egress_plan_device(eg, big, arena_bytes, d_idesc, cap, d_port, d_ops, d_queue, l2_port=d_iport)
        engine.vlan_device(big, arena_bytes, d_idesc, cap, d_ops, 0, None, 64, d_vst)
        engine.egress_acl_device(aclset, big, arena_bytes, d_idesc, cap, d_port, d_ea, d_er, d_ed, d_pk, d_by)
        engine.sync()
    tk = sc.take
    sc.same((tk(d_ops, np.uint32, cap, "ops"), tk(d_queue, np.uint8, cap, "queue"), tk(d_vst, np.uint8, cap, "vst")), (ops, queue, vst),
         ("ops", "queue", "vlan status"))
    got_idesc = d_idesc.download(nf.DESC_DTYPE, cap)
    sc.same((got_idesc["off16"], got_idesc["len"]), (idesc["off16"], cidesc["len"]), ("item off16", "item len after the pops"))
    sc.same((tk(d_port, np.uint32, cap, "port"), tk(d_ea, np.uint8, cap, "ea"), tk(d_er, np.uint32, cap, "er"), tk(d_ed, np.uint32, cap, "ed"),
          d_pk.download(np.uint32, nports), d_by.download(np.uint64, nports)),
         (eacl["port"], eacl["action"], eacl["rule"], eacl["redirect"], pk, by),
         ("port", "egress action", "egress rule", "egress redirect", "denied_pkts", "denied_bytes"))
    f.check_regions(compact, f.room)
    for b in (d_idesc, d_iport, d_pk, d_by):
        b.free()
    f.close()


def test_flood_copy_region_ends_inside_a_packets_copies(engine, big):
    """arena_bytes one byte short of the slot of a packet's second copy, past 32 GiB: the first copy is the last
    item, totals and items equal the host's, nothing is written from there on."""
    f = Flood(engine, big, "high")
    full = f.host(f.copy_base + f.room, f.cap)
    m = int(full["totals"]["items"])
    at = full["item_desc"]["off16"][:m].astype(np.int64) * 16
    k = next(k for k in range(m * 2 // 3, m - 1) if full["item_src"][k] == full["item_src"][k + 1] and at[k] >= f.copy_base
             and int(full["item_desc"][k]["len"]) >= 16)
    room = int(at[k + 1]) - f.copy_base + round_up(int(full["item_desc"][k + 1]["len"]), f.align) - 1
    want, _, _ = f.expand(room)
    tot = want["totals"]
    assert int(tot["items"]) == k + 1 < int(tot["items_needed"]) == m and int(want["item_src"][k]) > N // 2
    assert int(tot["copy_bytes"]) == int(at[k + 1]) - f.copy_base < int(tot["copy_bytes_needed"]) == f.room
    f.close()
