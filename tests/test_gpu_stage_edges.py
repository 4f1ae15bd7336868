"""GPU tests of the device stages at the places where a frame-reading kernel goes wrong: the truncation sweep of
stage_edge_common.py (every length 0..97 and 127..129 of twelve header kinds, at each of the 8 line offsets, the
rest of the original frame left behind the descriptor's length, 0xA5 between the slots) through every
frame-reading entry point, the whole chain over the sweep in one stream, and the maximum-size frames of
test_gpu_edges through the six stages. A kernel that ignores one of its length bounds reads a header the tables
know and answers as for the whole frame; the expected values come from the host functions on full[:t] as bytes,
which test_stage_edges.py holds against the Python models."""
import numpy as np
import pytest

import netflow_amd as nf
import oracle
import stage_edge_common as sc
from flood_common import assert_same_expand, copy_model, model_expand
from test_gpu_edges import max_frames

pytestmark = pytest.mark.gpu

GUARD = 256  # canary bytes behind arena_bytes


@pytest.fixture(scope="module")
def T(engine):
    with sc.Tables() as t:
        yield t.upload(engine)


class Sweep:
    def __init__(self, engine, room=0):
        self.full, self.lens, self.arena, self.desc = sc.placed_sweep(room=room)
        self.frames = sc.cut(self.full, self.lens)
        self.n = len(self.desc)
        self.engine = engine
        self.d_arena = sc.up(engine, np.concatenate([self.arena, np.full(GUARD, sc.FILL, np.uint8)]), np.uint8)
        self.d_desc = sc.up(engine, self.desc, nf.DESC_DTYPE)

    def args(self):
        return self.d_arena, self.arena.nbytes, self.d_desc, self.n

    def unchanged(self):
        back = self.d_arena.download(np.uint8, self.arena.nbytes + GUARD)
        assert np.array_equal(back[:self.arena.nbytes], self.arena), "the call wrote into the arena"
        assert (back[self.arena.nbytes:] == sc.FILL).all(), "a store past arena_bytes"
        assert np.array_equal(self.d_desc.download(nf.DESC_DTYPE, self.n), self.desc), "the call wrote a descriptor"

    def free(self):
        self.d_arena.free()
        self.d_desc.free()


@pytest.fixture(scope="module")
def sweep(engine):
    s = Sweep(engine)
    yield s
    s.free()


# ---- the read-only stages over the sweep -------------------------------------------------------------------

def test_route_lookup_sweep(engine, T, sweep):
    want = sc.route_host(T, sweep.frames)
    got = sc.dev_route(engine, T, *sweep.args())
    sweep.unchanged()
    sc.same(got, want, ("verdict", "nh", "egress_if"))
    assert {nf.RT_FORWARD, nf.RT_NOT_IPV4} <= set(want[0].tolist())


def test_acl_eval_sweep(engine, T, sweep):
    action, first, redirect = sc.acl_host(T, sweep.frames)
    nh_in = (np.arange(sweep.n) * 3 + 1).astype(np.uint32)
    got = sc.dev_acl(engine, T.acl, *sweep.args(), nh_in)
    sweep.unchanged()
    sc.same(got, (action, first, redirect, np.where(action == nf.ACL_PERMIT, nh_in, nf.NH_NONE)), ("action", "rule", "redirect", "nh"))


@pytest.mark.parametrize("routed", [False, True])
@pytest.mark.parametrize("learn", [True, False])
def test_l2_lookup_sweep(engine, T, sweep, learn, routed):
    """Both instantiations of the kernel's LEARN template; with `routed`, a route verdict that takes a third of
    the frames away from the L2 decision."""
    want = [a.copy() for a in sc.l2_host(T, sweep.frames)]
    rt = None
    if routed:
        rt = np.where(np.arange(sweep.n) % 3 == 0, nf.RT_FORWARD, nf.RT_NOT_IPV4).astype(np.uint8)
        for a, none in zip(want, (nf.L2_SKIP, nf.IF_NONE, 0, nf.L2_LEARN_NONE)):
            a[rt != nf.RT_NOT_IPV4] = none
    got = sc.dev_l2(engine, T.fdb, sc.INGRESS, *sweep.args(), rt_verdict=rt, learn=learn)
    sweep.unchanged()
    sc.same(got[:3], want[:3], ("verdict", "port", "vlan"))
    if learn:
        sc.same(got[3:], want[3:], ("learn",))


def test_egress_plan_sweep(engine, T, sweep):
    ports = sc.plan_ports(sweep.n)
    ops, queue = sc.plan_host(T, ports, sweep.frames)
    got = sc.dev_plan(engine, T.egress, *sweep.args(), ports)
    sweep.unchanged()
    sc.same(got, (ports, ops, queue), ("port", "ops", "queue"))


def test_egress_acl_sweep(engine, T, sweep):
    """Thirteen ports in turn: every wave holds the four lists and lanes without one. The deny counters add up
    the descriptors' lengths, not the slots'."""
    ports = sc.acl_ports(sweep.n)
    action, first, redirect = sc.eacl_host(T, ports, sweep.frames)
    nports = T.aclset.info()[0]
    gone = action == nf.ACL_DENY
    pk = np.bincount(ports[gone], minlength=nports).astype(np.uint32)
    by = np.bincount(ports[gone], weights=sweep.lens[gone], minlength=nports).astype(np.uint64)
    assert pk.sum() > 1000 and (pk > 0).sum() >= 4
    got = sc.dev_eacl(engine, T.aclset, *sweep.args(), ports, nports)
    sweep.unchanged()
    sc.same(got, (np.where(gone, sc.NONE, ports), action, first, redirect, pk, by),
         ("port", "action", "rule", "redirect", "denied_pkts", "denied_bytes"))
    hpk, hby = np.zeros(nports, np.uint32), np.zeros(nports, np.uint64)
    host = T.aclset.egress_acl_host(sweep.arena, sweep.desc, ports, hpk, hby)
    sc.same((host["action"], host["rule"], host["redirect"], hpk, hby), (action, first, redirect, pk, by),
         ("host action", "host rule", "host redirect", "host denied_pkts", "host denied_bytes"))


# ---- the flood copies ----------------------------------------------------------------------------------------

def expand_case(engine, frames_arena, desc, fan, align, cap):
    """Every packet flooded to `fan` ports: device against host against model, the arena against the copy model."""
    n = len(desc)
    copy_base = sc.round_up(frames_arena.nbytes, 128)
    room = fan * int(sum(sc.round_up(int(t), align) for t in desc["len"]))
    arena = np.full(copy_base + room, sc.FILL, np.uint8)
    arena[:frames_arena.nbytes] = frames_arena
    arrays = sc.all_flooded(n)
    fdb, ports = sc.flood_table(fan + 1)
    with fdb:
        fdb.upload(engine)
        want = fdb.flood_expand_host(0, fan + 1, arena.nbytes, copy_base, align, desc, cap, **arrays)
        model = model_expand(ports, 0, fan + 1, arena.nbytes, copy_base, align, desc, cap, **arrays)
        assert_same_expand(want, model, "host against model: ")
        d_arena = sc.up(engine, np.concatenate([arena, np.full(GUARD, sc.FILL, np.uint8)]), np.uint8)
        d_desc = sc.up(engine, desc, nf.DESC_DTYPE)
        got = sc.dev_expand(engine, fdb, 0, fan + 1, d_arena, arena.nbytes, copy_base, align, d_desc, n, cap, arrays)
    back = d_arena.download(np.uint8, arena.nbytes + GUARD)
    d_arena.free()
    d_desc.free()
    assert_same_expand(got, want)
    assert (back[arena.nbytes:] == sc.FILL).all(), "a store past arena_bytes"
    assert np.array_equal(back[:arena.nbytes], copy_model(arena, desc, want, copy_base)), "the arena differs from the copy model"
    assert int(want["totals"]["items"]) == int(want["totals"]["copies"]) == fan * n and int(want["totals"]["copy_bytes"]) == room
    return want, back, copy_base


@pytest.mark.parametrize("align", [16, 128])
def test_flood_expand_sweep(engine, align):
    """Every sweep frame flooded to three ports, the frames of 0..13 bytes included: a copy holds the
    round_up(t, 16) bytes of its slot, whatever lies behind them, and a frame of no bytes gets items without
    a byte copied."""
    _, lens, frames_arena, desc = sc.placed_sweep()
    want, back, copy_base = expand_case(engine, frames_arena, desc, 3, align, 3 * len(desc) + 5)
    m = 3 * len(desc)
    assert np.array_equal(want["item_desc"]["len"][:m], np.repeat(lens, 3))
    assert np.array_equal(want["item_src"][:m], np.repeat(np.arange(len(desc)), 3))
    assert (want["item_desc"]["off16"][:m].astype(np.int64) * 16 >= copy_base).all()
    for k in (0, 1, 2, 3 * 13 + 1, 3 * 96, m - 1):  # spot checks in the test's own words
        o, s, t = int(want["item_desc"][k]["off16"]) * 16, int(desc[k // 3]["off16"]) * 16, int(lens[k // 3])
        assert np.array_equal(back[o:o + sc.round_up(t, 16)], frames_arena[s:s + sc.round_up(t, 16)])
        assert (back[o + sc.round_up(t, 16):o + sc.round_up(t, align)] == sc.FILL).all()


# ---- the four original entry points on the live-tail arena -------------------------------------------------------

def test_update_sweep(engine, sweep):
    ref = sweep.arena.copy()
    rst, _ = oracle.update_batch(ref, sweep.desc)
    d_arena = sc.up(engine, sweep.arena, np.uint8)
    d_st = sc.filled(engine, sweep.n)
    engine.update_device(d_arena, sweep.arena.nbytes, sweep.d_desc, sweep.n, d_st)
    engine.sync()
    got = d_arena.download(np.uint8, sweep.arena.nbytes)
    d_arena.free()
    sc.same((sc.take(d_st, np.uint8, sweep.n, "status"),), (rst,), ("status",))
    assert np.array_equal(got, ref)
    assert not np.array_equal(ref, sweep.arena)


def test_l3_forward_sweep(engine, T, sweep):
    _, nh, _ = sc.route_host(T, sweep.frames)
    nh[1::5] = nf.NH_NONE
    table = T.fib.nexthops_host()
    ref = sweep.arena.copy()
    rst = oracle.l3_forward_batch(ref, sweep.desc, nh, table.view(np.uint8))
    assert (rst & nf.ST_FLAG_FWD).astype(bool).sum() > 1000
    d_arena = sc.up(engine, sweep.arena, np.uint8)
    d_nh = sc.up(engine, nh, np.uint32)
    d_st = sc.filled(engine, sweep.n)
    ptr, count = T.fib.nexthops()
    assert count == len(table)
    engine.l3_forward_device(d_arena, sweep.arena.nbytes, sweep.d_desc, d_nh, sweep.n, ptr, count, d_st)
    engine.sync()
    got = d_arena.download(np.uint8, sweep.arena.nbytes)
    d_arena.free()
    d_nh.free()
    sc.same((sc.take(d_st, np.uint8, sweep.n, "status"),), (rst,), ("status",))
    assert np.array_equal(got, ref)


def test_vlan_sweep(engine):
    """Push, pop, pop over slots with room for the push: what lies behind a frame's length moves, or stays, as
    the reference's memmove leaves it."""
    s = Sweep(engine, room=4)
    arena, desc = s.arena.copy(), s.desc.copy()
    caps = np.full(s.n, sc.BASE_LEN + 4, np.uint32)
    d_caps = sc.up(engine, caps, np.uint32)
    d_st = engine.alloc(s.n)
    seen = set()
    for op in (nf.vlan_push_op(4094, 6), nf.VLAN_POP, nf.VLAN_POP):
        rst = oracle.vlan_batch(arena, desc, None, caps, op_all=op)
        engine.vlan_device(s.d_arena, arena.nbytes, s.d_desc, s.n, None, op, d_caps, 0, d_st)
        engine.sync()
        sc.same((d_st.download(np.uint8, s.n),), (rst,), ("status",))
        assert np.array_equal(s.d_desc.download(nf.DESC_DTYPE, s.n), desc)
        back = s.d_arena.download(np.uint8, arena.nbytes + GUARD)
        assert np.array_equal(back[:arena.nbytes], arena) and (back[arena.nbytes:] == sc.FILL).all()
        seen |= set(rst.tolist())
    assert nf.ST_VLAN_FAIL in seen and any(x & nf.ST_FLAG_VLAN for x in seen if x != nf.ST_VLAN_FAIL)
    for b in (d_caps, d_st):
        b.free()
    s.free()


def test_flow_keys_sweep(engine, sweep):
    keys, hashes = oracle.flow_keys_batch(sweep.arena, sweep.desc)
    d_keys, d_hash = sc.filled(engine, 64 * sweep.n), sc.filled(engine, 4 * (sweep.n + 1))
    engine.flow_keys_device(*sweep.args(), d_keys, d_hash)
    engine.sync()
    sweep.unchanged()
    sc.same((sc.take(d_hash, np.uint32, sweep.n, "hashes"),), (hashes,), ("hashes",))
    got = d_keys.download(np.uint8, 64 * sweep.n + 16)
    d_keys.free()
    assert (got[64 * sweep.n:] == sc.FILL).all()
    assert np.array_equal(got[:64 * sweep.n].reshape(sweep.n, 64), np.asarray(keys).reshape(sweep.n, 64))


# ---- the whole chain ---------------------------------------------------------------------------------------------

def test_chain_over_the_sweep_in_one_stream(engine, T):
    """lookup -> ACL -> forward -> L2 -> expand -> plan -> VLAN -> egress ACL -> enqueue over the sweep on one stream
    with no host step, each stage's outputs against the host chain, the arena at the end against the oracle's
    forward, the copy model and the oracle's pops."""
    full, lens, frames_arena, desc = sc.placed_sweep()
    frames = sc.cut(full, lens)
    n, num_ports = len(desc), 6
    cap = n + 1000
    copy_base = sc.round_up(frames_arena.nbytes, 128)
    arena = np.full(copy_base + (64 << 10), sc.FILL, np.uint8)
    arena[:frames_arena.nbytes] = frames_arena
    nbytes = arena.nbytes
    # the host chain
    v, nh, eif = sc.route_host(T, frames)
    action, first, redirect = sc.acl_host(T, frames, T.chain_acl)
    for g, w in zip((action, first, redirect), sc.acl_model(T, frames, T.chain_rules)):
        assert np.array_equal(g, w)
    nh2 = np.where(action == nf.ACL_PERMIT, nh, nf.NH_NONE).astype(np.uint32)
    table = T.fib.nexthops_host()
    ref = arena.copy()
    st = oracle.l3_forward_batch(ref, desc, nh2, table.view(np.uint8))
    l2 = [a.copy() for a in sc.l2_host(T, frames)]
    for a, none in zip(l2, (nf.L2_SKIP, nf.IF_NONE, 0, nf.L2_LEARN_NONE)):
        a[v != nf.RT_NOT_IPV4] = none
    lv, lp, lvl, lle = l2
    arrays = dict(l3_port=eif, fwd_status=st, l2_port=lp, l2_verdict=lv, l2_vlan=lvl)
    items = T.fdb.flood_expand_host(sc.INGRESS, num_ports, nbytes, copy_base, 16, desc, cap, **arrays)
    assert_same_expand(items, model_expand(T.l2_ports, sc.INGRESS, num_ports, nbytes, copy_base, 16, desc, cap, **arrays),
                       "host against model: ")
    tot = items["totals"]
    m = int(tot["items"])
    assert m == int(tot["items_needed"]) and int(tot["copies"]) == 3 * int(tot["flooded"]) >= 300
    assert (st & nf.ST_FLAG_FWD).astype(bool).sum() >= 300 and (lv == nf.L2_FORWARD).sum() >= 300
    ref = copy_model(ref, desc, items, copy_base)
    idesc, iport = items["item_desc"].copy(), items["item_port"]
    item_frames = [bytes(ref[int(d["off16"]) * 16:int(d["off16"]) * 16 + int(d["len"])]) for d in idesc]
    ops, queue = sc.plan_host(T, iport, item_frames)
    for g, w in zip((ops, queue), sc.plan_model(T, iport, item_frames)):
        assert np.array_equal(g, w)
    assert (ops[:m] == nf.VLAN_POP).sum() >= 100
    vst = oracle.vlan_batch(ref, idesc, ops, None, cap_all=64)
    nports = T.aclset.info()[0]
    pk, by = np.zeros(nports, np.uint32), np.zeros(nports, np.uint64)
    eacl = T.aclset.egress_acl_host(ref, idesc, iport, pk, by)
    popped = [bytes(ref[int(d["off16"]) * 16:int(d["off16"]) * 16 + int(d["len"])]) for d in idesc]
    for g, w in zip((eacl["action"], eacl["rule"], eacl["redirect"]), sc.eacl_model(T, iport, popped)):
        assert np.array_equal(g, w)
    assert pk.sum() >= 100
    _, keys = T.egress.keys()
    enq = T.egress.enqueue_host(eacl["port"], queue, np.zeros(keys, np.uint32))
    assert (enq["result"] == nf.EQ_ENQUEUED).sum() >= 300
    # the device chain
    d_arena = sc.up(engine, np.concatenate([arena, np.full(GUARD, sc.FILL, np.uint8)]), np.uint8)
    d_desc = sc.up(engine, desc, nf.DESC_DTYPE)
    F = lambda size, count: sc.filled(engine, size * (count + 1))  # noqa: E731
    d_nh, d_if, d_v = F(4, n), F(4, n), F(1, n)
    d_action, d_rule, d_redirect, d_st = F(1, n), F(4, n), F(4, n), F(1, n)
    d_lp, d_lv, d_lvl, d_lle = F(4, n), F(1, n), F(2, n), F(1, n)
    d_idesc, d_iport, d_isrc, d_tot = F(8, cap), F(4, cap), F(4, cap), sc.filled(engine, 32)
    d_port, d_ops, d_queue, d_vst = F(4, cap), F(4, cap), F(1, cap), F(1, cap)
    d_ea, d_er, d_ed = F(1, cap), F(4, cap), F(4, cap)
    d_pk, d_by = sc.up(engine, np.zeros(nports, np.uint32), np.uint32), sc.up(engine, np.zeros(nports, np.uint64), np.uint64)
    d_depth = sc.up(engine, np.zeros(keys, np.uint32), np.uint32)
    d_order, d_ks, d_drop, d_res = F(4, cap), F(4, keys + 1), F(4, keys), F(1, cap)
    tptr, tcount = T.fib.nexthops()
    engine.route_lookup_device(T.fib, d_arena, nbytes, d_desc, n, d_nh, d_if, d_v)
    engine.acl_eval_device(T.chain_acl, d_arena, nbytes, d_desc, n, d_action, d_rule, d_redirect, d_nh)
    engine.l3_forward_device(d_arena, nbytes, d_desc, d_nh, n, tptr, tcount, d_st)
    engine.l2_lookup_device(T.fdb, sc.INGRESS, d_arena, nbytes, d_desc, n, d_lp, rt_verdict=d_v, verdict=d_lv, vlan=d_lvl,
                            learn=d_lle)
    engine.flood_expand_device(T.fdb, sc.INGRESS, num_ports, d_arena, nbytes, copy_base, 16, d_desc, n, cap, d_idesc, d_iport,
                               d_isrc, d_tot, l3_port=d_if, fwd_status=d_st, l2_port=d_lp, l2_verdict=d_lv, l2_vlan=d_lvl)
    engine.egress_plan_device(T.egress, d_arena, nbytes, d_idesc, cap, d_port, d_ops, d_queue, l2_port=d_iport)
    engine.vlan_device(d_arena, nbytes, d_idesc, cap, d_ops, 0, None, 64, d_vst)
    engine.egress_acl_device(T.aclset, d_arena, nbytes, d_idesc, cap, d_port, d_ea, d_er, d_ed, d_pk, d_by)
    engine.egress_enqueue_device(T.egress, d_port, d_queue, cap, d_depth, d_order, d_ks, result=d_res, key_dropped=d_drop)
    engine.sync()
    tk = sc.take
    sc.same((tk(d_v, np.uint8, n, "v"), tk(d_if, np.uint32, n, "if")), (v, eif), ("route verdict", "egress_if"))
    sc.same((tk(d_action, np.uint8, n, "a"), tk(d_rule, np.uint32, n, "r"), tk(d_redirect, np.uint32, n, "d"), tk(d_nh, np.uint32, n, "nh")),
         (action, first, redirect, nh2), ("acl action", "acl rule", "acl redirect", "nh"))
    sc.same((tk(d_st, np.uint8, n, "st"),), (st,), ("forward status",))
    sc.same((tk(d_lv, np.uint8, n, "lv"), tk(d_lp, np.uint32, n, "lp"), tk(d_lvl, np.uint16, n, "lvl"), tk(d_lle, np.uint8, n, "lle")),
         (lv, lp, lvl, lle), ("l2 verdict", "l2 port", "l2 vlan", "l2 learn"))
    got_tot = d_tot.download(np.uint8, 32).view(nf.FLOOD_TOTALS_DTYPE)[0]
    d_tot.free()
    got_idesc = d_idesc.download(nf.DESC_DTYPE, cap + 1)
    d_idesc.free()
    assert got_idesc[cap]["off16"] == sc.EE4
    got_items = {"totals": got_tot, "item_port": tk(d_iport, np.uint32, cap, "iport"), "item_src": tk(d_isrc, np.uint32, cap, "isrc"),
                 "item_desc": items["item_desc"]}
    assert_same_expand(got_items, items)
    sc.same((got_idesc[:cap]["off16"], got_idesc[:cap]["len"]), (idesc["off16"], idesc["len"]), ("item off16", "item len after the pops"))
    want_port = eacl["port"]
    sc.same((tk(d_ops, np.uint32, cap, "ops"), tk(d_queue, np.uint8, cap, "q"), tk(d_vst, np.uint8, cap, "vst")), (ops, queue, vst),
         ("ops", "queue", "vlan status"))
    sc.same((tk(d_port, np.uint32, cap, "port"), tk(d_ea, np.uint8, cap, "ea"), tk(d_er, np.uint32, cap, "er"), tk(d_ed, np.uint32, cap, "ed")),
         (want_port, eacl["action"], eacl["rule"], eacl["redirect"]), ("port", "egress action", "egress rule", "egress redirect"))
    sc.same((d_pk.download(np.uint32, nports), d_by.download(np.uint64, nports)), (pk, by), ("denied_pkts", "denied_bytes"))
    ks = tk(d_ks, np.uint32, keys + 1, "ks")
    total = int(ks[keys])
    sc.same((ks, tk(d_drop, np.uint32, keys, "drop"), tk(d_res, np.uint8, cap, "res"), d_depth.download(np.uint32, keys)),
         (enq["key_start"], enq["key_dropped"], enq["result"], enq["depth"]), ("key_start", "key_dropped", "result", "depth"))
    sc.same((tk(d_order, np.uint32, cap, "order")[:total],), (enq["order"],), ("order",))
    back = d_arena.download(np.uint8, nbytes + GUARD)
    assert (back[nbytes:] == sc.FILL).all(), "a store past arena_bytes"
    bad = np.flatnonzero(back[:nbytes] != ref)
    assert len(bad) == 0, f"the arena differs from the host chain's at {len(bad)} bytes, the first at {bad[0]}"
    for b in (d_arena, d_desc, d_pk, d_by, d_depth):
        b.free()


# ---- maximum-size frames -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big_frames(engine):
    frames = max_frames(np.random.default_rng(5))
    arena, desc = oracle.pack_frames(frames)
    d_arena, d_desc = sc.up(engine, arena, np.uint8), sc.up(engine, desc, nf.DESC_DTYPE)
    yield frames, arena, desc, (d_arena, arena.nbytes, d_desc, len(desc))
    assert np.array_equal(d_arena.download(np.uint8, arena.nbytes), arena), "a stage wrote into the arena"
    d_arena.free()
    d_desc.free()


def test_max_size_frames_through_the_read_only_stages(engine, T, big_frames):
    frames, arena, desc, args = big_frames
    n = len(frames)
    assert sorted(set(len(f) for f in frames)) == [65549, 65553, 65589, 65593]
    sc.same(sc.dev_route(engine, T, *args), sc.route_host(T, frames), ("verdict", "nh", "egress_if"))
    action, first, redirect = sc.acl_host(T, frames)
    nh_in = np.arange(n, dtype=np.uint32)
    sc.same(sc.dev_acl(engine, T.acl, *args, nh_in), (action, first, redirect, np.where(action == nf.ACL_PERMIT, nh_in, nf.NH_NONE)),
         ("action", "rule", "redirect", "nh"))
    lv, lp, lvl, lle = sc.l2_host(T, frames)
    sc.same(sc.dev_l2(engine, T.fdb, sc.INGRESS, *args), (lv, lp, lvl, lle), ("verdict", "port", "vlan", "learn"))
    ports = np.array([0, 2, 1, 5, 8, 8, 0, 1], np.uint32)  # port 8 pops the tagged frames' VLAN
    ops, queue = sc.plan_host(T, ports, frames)
    sc.same(sc.dev_plan(engine, T.egress, *args, ports), (ports, ops, queue), ("port", "ops", "queue"))
    assert (ops == nf.VLAN_POP).any() and len(set(queue.tolist())) >= 2
    ports = np.array([0, 2, 1, 5, 5, 2, 0, 1], np.uint32)  # list 2 denies TCP
    ea, er, ed = sc.eacl_host(T, ports, frames)
    nports = T.aclset.info()[0]
    gone = ea == nf.ACL_DENY
    pk = np.bincount(ports[gone], minlength=nports).astype(np.uint32)
    by = np.bincount(ports[gone], weights=desc["len"][gone], minlength=nports).astype(np.uint64)
    assert gone.any()
    sc.same(sc.dev_eacl(engine, T.aclset, *args, ports, nports), (np.where(gone, sc.NONE, ports), ea, er, ed, pk, by),
         ("port", "action", "rule", "redirect", "denied_pkts", "denied_bytes"))


def test_max_size_frames_flooded(engine, big_frames):
    """65,549 to 65,593 bytes to two ports each: 43 passes of the copy's rows per frame, byte for byte."""
    frames, arena, desc, _ = big_frames
    want, back, copy_base = expand_case(engine, arena, desc, 2, 16, 2 * len(desc))
    for k in range(2 * len(desc)):
        o, f = int(want["item_desc"][k]["off16"]) * 16, frames[k // 2]
        assert o >= copy_base and bytes(back[o:o + len(f)]) == f, k
