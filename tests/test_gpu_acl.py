"""GPU tests of the ACL evaluation kernel (nfcs_acl_eval_device) through the C ABI: against the
reference's decisions on the fixture frames (tests/golden/acl_ref.npz), against the CPU decision of the
same rules (Acl.eval_host) at the sizes where the kernel changes path, the in/out next-hop vector, and
in one stream between the route lookup and the fused forward against the oracle."""
import numpy as np
import pytest

import netflow_amd as nf
import oracle
from acl_common import LISTS, acl_fixture, eval_host, fixture_rules, make_acl, rule
from route_common import FWD_DSTS, decide_host, fixture_fib, route_fixture

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF


@pytest.fixture(scope="module")
def fx():
    return acl_fixture()


def pack_at(frames, starts):
    """Frames at the given byte offsets (multiples of 16, ascending, not overlapping)."""
    desc = np.zeros(len(frames), dtype=nf.DESC_DTYPE)
    end = 0
    for i, (f, o) in enumerate(zip(frames, starts)):
        assert o % 16 == 0 and o >= end
        desc[i] = (o // 16, len(f))
        end = o + (len(f) + 15) // 16 * 16
    arena = np.zeros(max(end, 16), dtype=np.uint8)
    for f, o in zip(frames, starts):
        arena[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    return arena, desc


def run_eval(engine, acl, arena, desc, arena_bytes=None, want=("rule", "redirect", "nh"), nh_in=None):
    """(action, rule, redirect, nh) from the device; the optional outputs not named in `want` are
    passed as NULL and come back as None. nh starts as nh_in (default: a sentinel everywhere)."""
    n = len(desc)
    acl.upload(engine)
    d_arena = engine.alloc(arena.nbytes).upload(arena)
    d_desc = engine.alloc(max(desc.nbytes, 16)).upload(desc)
    d_action = engine.alloc(max(n, 16)).upload(np.full(max(n, 16), 0xEE, np.uint8))
    d_rule = engine.alloc(max(4 * n, 16)) if "rule" in want else None
    d_red = engine.alloc(max(4 * n, 16)) if "redirect" in want else None
    d_nh = None
    if "nh" in want:
        d_nh = engine.alloc(max(4 * n, 16)).upload(np.full(n, SENTINEL, np.uint32) if nh_in is None else nh_in)
    engine.acl_eval_device(acl, d_arena, arena.nbytes if arena_bytes is None else arena_bytes, d_desc, n, d_action,
                           d_rule, d_red, d_nh)
    engine.sync()
    assert np.array_equal(d_arena.download(np.uint8, arena.nbytes), arena), "the evaluation wrote into the frames"
    get = lambda b: None if b is None else b.download(np.uint32, n)  # noqa: E731
    return d_action.download(np.uint8, n), get(d_rule), get(d_red), get(d_nh)


def check(got, want_action, want_rule, want_port, nh_in=None):
    action, first, port, nh = got
    assert np.array_equal(action, want_action)
    if first is not None:
        assert np.array_equal(first, want_rule)
    if port is not None:
        assert np.array_equal(port, want_port)
    if nh is not None:
        before = np.full(len(action), SENTINEL, np.uint32) if nh_in is None else nh_in
        assert np.array_equal(nh, np.where(want_action == nf.ACL_PERMIT, before, nf.NH_NONE).astype(np.uint32))


@pytest.mark.parametrize("align", [16, 128])
@pytest.mark.parametrize("name", LISTS)
def test_fixture_matches_reference(engine, fx, name, align):
    z, frames = fx
    arena, desc = oracle.pack_frames(frames, align=align)
    with make_acl(fixture_rules(z, name)) as acl:
        got = run_eval(engine, acl, arena, desc)
    check(got, z["action_" + name], z["rule_" + name], z["redirect_" + name])


@pytest.mark.parametrize("want", [(), ("rule",), ("redirect",), ("nh",), ("redirect", "nh")])
def test_optional_outputs_left_out(engine, fx, want):
    z, frames = fx
    arena, desc = oracle.pack_frames(frames)
    with make_acl(fixture_rules(z, "b")) as acl:
        got = run_eval(engine, acl, arena, desc, want=want)
    assert [g is not None for g in got[1:]] == [k in want for k in ("rule", "redirect", "nh")]
    check(got, z["action_b"], z["rule_b"], z["redirect_b"])


@pytest.mark.parametrize("first_start", [80, 96, 112])
@pytest.mark.parametrize("name", LISTS)
def test_frame_starts_late_in_their_lines(engine, fx, name, first_start):
    """Frames whose headers begin 80, 96 or 112 bytes into a 128-byte line, so that header bytes 0..47
    (and the late chunks of IPv4 options) cross into the next line."""
    z, frames = fx
    starts = [256 * i + (80, 96, 112)[(i + first_start // 16) % 3] for i in range(len(frames))]
    arena, desc = pack_at(frames, starts)
    assert all(int(d["off16"]) * 16 % 128 >= 80 for d in desc)
    with make_acl(fixture_rules(z, name)) as acl:
        got = run_eval(engine, acl, arena, desc)
    check(got, z["action_" + name], z["rule_" + name], z["redirect_" + name])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_sizes_and_bad_descriptors(engine, fx, n):
    """Wave and workgroup edges (64 packets per wave, 256 per workgroup) on slices of the fixture, then
    the first and the last descriptor reaching outside the arena: NFCS_ACL_BAD_DESC for those two, their
    neighbours as before."""
    z, frames = fx
    sel = [(5 * i) % len(frames) for i in range(n)]
    frames = [frames[i] for i in sel]
    arena, desc = oracle.pack_frames(frames)
    want = [z[k + "_c"][sel].copy() for k in ("action", "rule", "redirect")]
    with make_acl(fixture_rules(z, "c")) as acl:
        check(run_eval(engine, acl, arena, desc), *want)
        bad = desc.copy()
        bad[0]["off16"] = arena.nbytes // 16  # starts at the arena's end
        if int(bad[0]["len"]) == 0:
            bad[0]["len"] = 1
        bad[n - 1]["len"] = arena.nbytes - int(bad[n - 1]["off16"]) * 16 + 1  # one byte past it
        got = run_eval(engine, acl, arena, bad)
    for i in {0, n - 1}:
        want[0][i], want[1][i], want[2][i] = nf.ACL_BAD_DESC, nf.ACL_NO_MATCH, nf.IF_NONE
    check(got, *want)
    assert (got[3][[0, n - 1]] == nf.NH_NONE).all()  # not permitted: no next hop either


def test_no_frames_is_ok_without_a_launch(engine):
    with make_acl(rule(nf.ACL_DENY)) as acl:
        acl.upload(engine)
        engine.acl_eval_device(acl, None, 0, None, 0, None)  # n == 0: nothing is looked at
        engine.sync()


def test_not_uploaded_is_an_argument_error(engine):
    buf = engine.alloc(64)
    with make_acl(rule(nf.ACL_DENY)) as acl:
        with pytest.raises(nf.NfcsError):
            engine.acl_eval_device(acl, buf, 64, buf, 1, buf)
        acl.upload(engine)
        # a setter invalidates the commit, not the upload: the device keeps serving the uploaded rules
        acl.set_rules(rule(nf.ACL_PERMIT))
        arena, desc = oracle.pack_frames([bytes(64)])
        with pytest.raises(nf.NfcsError):
            acl.eval_host(bytes(64))
        d_arena, d_desc, d_action = engine.alloc(64).upload(arena), engine.alloc(16).upload(desc), engine.alloc(16)
        engine.acl_eval_device(acl, d_arena, 64, d_desc, 1, d_action)
        engine.sync()
        assert d_action.download(np.uint8, 1)[0] == nf.ACL_DENY


def udp_frame(dport: int, tagged: bool, ihl: int = 5) -> bytes:
    b = bytearray(110)
    l2 = 18 if tagged else 14
    b[12:14] = b"\x81\x00" if tagged else b"\x08\x00"
    if tagged:
        b[16:18] = b"\x08\x00"
    b[l2], b[l2 + 9] = 0x40 | ihl, 17
    l4 = l2 + 4 * ihl
    b[l4 + 2:l4 + 4] = dport.to_bytes(2, "big")
    return bytes(b)


@pytest.mark.parametrize("rules_n", [0, 1, nf.ACL_GROUP - 1, nf.ACL_GROUP, nf.ACL_GROUP + 1, 2 * nf.ACL_GROUP + 1,
                                     nf.ACL_MAX_RULES])
def test_rule_counts_match_at_last_rule(engine, rules_n):
    """Rule i matches UDP destination port 1000 + i only, so frames to port 1000 + rules_n - 1 prove the
    scan reached the last rule: the last of a full group (4, 512) and the only real rule of a padded
    group (1, 5, 9). Then the same rule is given again at index 1: the earlier index must win. Frames
    with IPv4 options (IHL 15) have their ports past byte 47."""
    last = rules_n - 1
    ports = [1000, 1000 + max(last, 0), 1000 + rules_n // 2, 999]
    frames = [udp_frame(p, tagged=bool(k & 1), ihl=15 if k & 2 else 5) for k, p in enumerate(ports * 40)]
    arena, desc = oracle.pack_frames(frames)
    rules = np.concatenate([rule(1 + i % 2, rule_id=i, dst_port=1000 + i) for i in range(rules_n)]) if rules_n \
        else np.zeros(0, nf.ACL_RULE_DTYPE)
    with make_acl(rules) as acl:
        want = eval_host(acl, frames)
        got = run_eval(engine, acl, arena, desc)
    check(got, *want)
    if rules_n == 0:
        assert (got[0] == nf.ACL_PERMIT).all() and (got[1] == nf.ACL_NO_MATCH).all()
        return
    first = got[1].reshape(40, 4)
    assert (first[:, 0] == 0).all() and (first[:, 1] == last).all() and (first[:, 3] == nf.ACL_NO_MATCH).all()
    if rules_n > 2:  # the last rule's match, given again at index 1 with another action
        rules[1] = rule(nf.ACL_REDIRECT, 77, rule_id=1, dst_port=1000 + last)[0]
        with make_acl(rules) as acl:
            want = eval_host(acl, frames)
            got = run_eval(engine, acl, arena, desc)
        check(got, *want)
        assert (got[1].reshape(40, 4)[:, 1] == 1).all() and (got[2].reshape(40, 4)[:, 1] == 77).all()


@pytest.mark.parametrize("pos", range(2 * nf.ACL_GROUP))
def test_one_l2_rule_among_address_rules(engine, pos):
    """A trip of the scan reads the MAC / VLAN / EtherType halves of its rules only when one of them tests
    those. Here a single rule that does (a VLAN id, a source MAC or an EtherType) sits at every position
    of the first two trips among rules that test ports only, and only it matches the frames."""
    n_rules = 3 * nf.ACL_GROUP
    tagged, untagged = bytearray(udp_frame(7, True)), bytearray(udp_frame(7, False))
    tagged[14:16] = (0x6000 | 123).to_bytes(2, "big")
    untagged[6:12] = bytes([2, 0, 0, 0, 0, 9])
    arp = bytearray(untagged)
    arp[6:12], arp[12:14] = bytes(6), b"\x08\x06"
    frames = [bytes(tagged), bytes(untagged), bytes(arp), udp_frame(7, False), udp_frame(1000 + n_rules - 1, True)] * 30
    arena, desc = oracle.pack_frames(frames)
    for k, special in enumerate((rule(nf.ACL_REDIRECT, 4, vlan_id=123), rule(nf.ACL_DENY, src_mac=bytes([2, 0, 0, 0, 0, 9])),
                                 rule(nf.ACL_DENY, ethertype=0x0806))):
        rules = np.concatenate([special if i == pos else rule(nf.ACL_DENY, dst_port=1000 + i) for i in range(n_rules)])
        with make_acl(rules) as acl:
            want = eval_host(acl, frames)
            got = run_eval(engine, acl, arena, desc)
        check(got, *want)
        first = got[1].reshape(30, 5)
        assert (first[:, k] == pos).all() and (first[:, 3] == nf.ACL_NO_MATCH).all() and (first[:, 4] == n_rules - 1).all()


def test_next_hops_of_permitted_packets_keep_their_bits(engine, fx):
    z, frames = fx
    arena, desc = oracle.pack_frames(frames)
    rng = np.random.default_rng(5)
    nh_in = rng.integers(0, 1 << 32, len(frames), dtype=np.uint64).astype(np.uint32)
    nh_in[::7] = nf.NH_NONE
    nh_in[1::7] = 0
    with make_acl(fixture_rules(z, "a")) as acl:
        got = run_eval(engine, acl, arena, desc, nh_in=nh_in)
    check(got, z["action_a"], z["rule_a"], z["redirect_a"], nh_in=nh_in)
    permit = z["action_a"] == nf.ACL_PERMIT
    assert permit.any() and (~permit).any()
    assert np.array_equal(got[3][permit], nh_in[permit]) and (got[3][~permit] == nf.NH_NONE).all()


def host_order(a: str) -> int:
    return int.from_bytes(bytes(int(x) for x in a.split(".")), "big")


@pytest.mark.parametrize("table", ["a", "b"])
def test_lookup_acl_forward_in_one_stream(engine, table):
    """route_lookup_device -> acl_eval_device(d_nh) -> l3_forward_device on one stream with no host step,
    on the route fixture's frames, with an ACL that denies or redirects some forwarded destinations:
    frames and statuses equal the oracle's forward given the host's next hops masked by the host's ACL
    decision."""
    z, frames = route_fixture()
    rules = np.concatenate([rule(nf.ACL_DENY, dst_ip=host_order(FWD_DSTS[0])),
                            rule(nf.ACL_REDIRECT, 3, dst_ip=host_order("172.16.0.0"), dst_ip_mask=0xFFF00000),
                            rule(nf.ACL_PERMIT, ethertype=0x0800),
                            rule(nf.ACL_DENY)])
    arena, desc = oracle.pack_frames(frames)
    n = len(desc)
    with fixture_fib(z, table) as fib, make_acl(rules) as acl:
        want_v, want_nh, _ = decide_host(fib, frames)
        want_action, _, _ = eval_host(acl, frames)
        nht = fib.nexthops_host()
        fib.upload(engine)
        acl.upload(engine)
        d_tab, tab_n = fib.nexthops()
        d_arena = engine.alloc(arena.nbytes).upload(arena)
        d_desc = engine.alloc(desc.nbytes).upload(desc)
        d_nh, d_act, d_st = engine.alloc(4 * n), engine.alloc(n), engine.alloc(n)
        engine.route_lookup_device(fib, d_arena, arena.nbytes, d_desc, n, d_nh)
        engine.acl_eval_device(acl, d_arena, arena.nbytes, d_desc, n, d_act, nh=d_nh)
        engine.l3_forward_device(d_arena, arena.nbytes, d_desc, d_nh, n, d_tab, tab_n, d_st)
        engine.sync()
        out, st = d_arena.download(np.uint8, arena.nbytes), d_st.download(np.uint8, n)
        act, nh = d_act.download(np.uint8, n), d_nh.download(np.uint32, n)
    masked = np.where(want_action == nf.ACL_PERMIT, want_nh, nf.NH_NONE).astype(np.uint32)
    # the ACL takes forwarded packets away, and leaves more than a quarter of all frames forwarded
    taken = (want_nh != nf.NH_NONE) & (masked == nf.NH_NONE)
    assert taken.sum() >= 20 and {int(a) for a in want_action[taken]} == {nf.ACL_DENY, nf.ACL_REDIRECT}
    ref = arena.copy()
    rst = oracle.l3_forward_batch(ref, desc, masked, nht.view(np.uint8).reshape(-1, 12))
    assert ((rst & nf.ST_FLAG_FWD) != 0).sum() > n // 4
    assert np.array_equal(act, want_action) and np.array_equal(nh, masked)
    assert np.array_equal(st, rst)
    assert np.array_equal(out, ref)
