"""CPU tests under the stage edge tests: the truncation sweep of stage_edge_common.py through the library's host
functions (Fib.lookup_host behind the IPv4 predicate, Acl.eval_host, Fdb.lookup_host, Egress.plan_host,
AclSet.eval_host) against the independent Python models, on full[:t] as bytes. The GPU tests compare the
kernels with these values on an arena that keeps the rest of every frame behind its length; here the sweep is
shown not to be vacuous: per stage, the answer with the length ignored (the whole frame) differs from the true
one on at least 5% of the sweep, and the true answers hold every class the stage's length thresholds separate.
route_common.model_lookup is pinned to the reference's fixture first."""
import numpy as np
import pytest

import netflow_amd as nf
import stage_edge_common as sc
from route_common import TABLES, fixture_model_inputs, model_decide, route_fixture

MIN_SHARE = 0.05


@pytest.fixture(scope="module")
def T():
    with sc.Tables() as t:
        yield t


@pytest.fixture(scope="module")
def sweep():
    full, lens = sc.sweep_frames()
    return full, lens, sc.cut(full, lens)


@pytest.mark.parametrize("table", TABLES)
def test_route_model_matches_the_reference(table):
    z, frames = route_fixture()
    v, eif, macs = model_decide(*fixture_model_inputs(z, table), frames)
    assert np.array_equal(v, z["verdict_" + table])
    assert np.array_equal(eif, z["egress_" + table])
    fwd = v == nf.RT_FORWARD
    assert fwd.any() and np.array_equal(macs[fwd], z["macs_" + table][fwd])


def test_sweep_shape(sweep):
    full, lens, frames = sweep
    assert len(full) == 12 * 101 and len(full) % 64 != 0
    assert all(len(f) == sc.BASE_LEN for f in full) and [len(f) for f in frames] == lens.tolist()
    assert set(lens.tolist()) == set(range(98)) | {127, 128, 129}


def test_place_live_keeps_the_tail(sweep):
    full, lens, _ = sweep
    arena, desc = sc.place_live(full, lens, np.arange(len(full)) % 8)
    seen = np.zeros(arena.nbytes, bool)
    for i, (d, f) in enumerate(zip(desc, full)):
        o = int(d["off16"]) * 16
        assert o % 128 == 16 * (i % 8) and int(d["len"]) == int(lens[i])
        assert bytes(arena[o:o + len(f)]) == f and not seen[o:o + len(f)].any()
        seen[o:o + len(f)] = True
    assert (arena[~seen] == sc.GAP).all() and (~seen).any()


def share(true, ignored):
    return float(sc.differs(true, ignored).mean())


def test_route_sweep(T, sweep):
    full, _, frames = sweep
    v, nh, eif = sc.route_host(T, frames)
    mv, meif, mmacs = sc.route_model(T, frames)
    nht = T.fib.nexthops_host()
    assert np.array_equal(v, mv) and np.array_equal(eif, meif)
    fwd = v == nf.RT_FORWARD
    assert (nh[~fwd] == nf.NH_NONE).all()
    assert np.array_equal(np.concatenate([nht["dst_mac"][nh[fwd]], nht["src_mac"][nh[fwd]]], axis=1), mmacs[fwd])
    assert {nf.RT_FORWARD, nf.RT_NOT_IPV4} <= set(v.tolist())
    whole = sc.route_host(T, full)
    ipv4 = [i for i, f in enumerate(full) if whole[0][i] != nf.RT_NOT_IPV4]
    assert len(ipv4) == 7 * 101 and (whole[0][ipv4] == nf.RT_FORWARD).all()  # the cut is what changes the answer
    assert share((v, nh, eif), whole) >= MIN_SHARE


def test_acl_sweep(T, sweep):
    full, _, frames = sweep
    got, want = sc.acl_host(T, frames), sc.acl_model(T, frames)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    action, first, _ = got
    assert ((action == nf.ACL_DENY) & (first <= 1)).any()                 # a port rule denies
    assert ((first >= 2) & (first != nf.ACL_NO_MATCH)).any()              # a rule that needs no ports
    assert set(range(7)) <= set(first.tolist())                           # in fact every rule decides somewhere
    assert (first == nf.ACL_NO_MATCH).any()
    whole = sc.acl_host(T, full)
    v4 = [k for k, name in enumerate(sc.base_frames()) if name not in ("qinq", "ipv6_udp", "arp", "q_arp", "q_ipv6_udp")]
    assert all(whole[0][101 * k] == nf.ACL_DENY and whole[1][101 * k] <= 1 for k in v4)
    assert share(got, whole) >= MIN_SHARE


def test_l2_sweep(T, sweep):
    full, _, frames = sweep
    got, want = sc.l2_host(T, frames), sc.l2_model(T, frames)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    verdict, _, vlan, learn = got
    assert {nf.L2_FORWARD, nf.L2_FLOOD, nf.L2_NO_ETH} <= set(verdict.tolist())
    decided = verdict != nf.L2_NO_ETH
    assert {1, sc.VID} <= set(vlan[decided].tolist())                    # a native and a tagged lookup VLAN
    assert len(set(learn[decided].tolist())) >= 2
    whole = sc.l2_host(T, full)
    assert (whole[0] == nf.L2_FORWARD).all()                              # every base is an FDB hit
    assert share(got, whole) >= MIN_SHARE


def test_plan_sweep(T, sweep):
    full, _, frames = sweep
    ports = sc.plan_ports(len(frames))
    got, want = sc.plan_host(T, ports, frames), sc.plan_model(T, ports, frames)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    ops, queue = got
    assert {nf.VLAN_POP, nf.VLAN_NOP} <= set(ops.tolist())
    assert len(set(queue[ports != sc.NONE].tolist())) >= 3
    assert (queue[ports == sc.NONE] == nf.QUEUE_NONE).all()
    whole = sc.plan_host(T, ports, full)
    assert (whole[0] == nf.VLAN_POP).any()
    assert share(got, whole) >= MIN_SHARE


def test_egress_acl_sweep(T, sweep):
    full, _, frames = sweep
    ports = sc.acl_ports(len(frames))
    got, want = sc.eacl_host(T, ports, frames), sc.eacl_model(T, ports, frames)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    action = got[0]
    assert {nf.ACL_PERMIT, nf.ACL_DENY, nf.ACL_REDIRECT, nf.ACL_NO_PORT} <= set(action.tolist())
    for p in (0, 1, 2, 5):                                                # every list decides, and by several rules
        assert len(set(got[1][ports == p].tolist())) >= 3, p
    for p in (3, 4, 6):                                                   # no list: permitted unread
        assert (action[ports == p] == nf.ACL_PERMIT).all() and (got[1][ports == p] == nf.ACL_NO_MATCH).all()
    whole = sc.eacl_host(T, ports, full)
    assert share(got, whole) >= MIN_SHARE


def test_models_see_what_the_max_size_frames_are(T):
    """The maximum-size frames of test_gpu_edges.max_frames through host and model: the GPU test runs them
    through the kernels."""
    from test_gpu_edges import max_frames
    frames = max_frames(np.random.default_rng(5))
    assert sorted(set(len(f) for f in frames)) == [65549, 65553, 65589, 65593]
    for g, w in zip(sc.acl_host(T, frames), sc.acl_model(T, frames)):
        assert np.array_equal(g, w)
    for g, w in zip(sc.l2_host(T, frames), sc.l2_model(T, frames)):
        assert np.array_equal(g, w)
    ports = sc.plan_ports(len(frames))
    for g, w in zip(sc.plan_host(T, ports, frames), sc.plan_model(T, ports, frames)):
        assert np.array_equal(g, w)
    for g, w in zip(sc.eacl_host(T, ports, frames), sc.eacl_model(T, ports, frames)):
        assert np.array_equal(g, w)
    v, _, eif = sc.route_host(T, frames)
    mv, meif, _ = sc.route_model(T, frames)
    assert np.array_equal(v, mv) and np.array_equal(eif, meif)
