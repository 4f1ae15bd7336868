"""GPU tests of the L2 lookup kernel (nfcs_l2_lookup_device) through the C ABI: against the reference's
decisions on the fixture frames (tests/golden/l2_ref.npz), against the CPU decision of the same tables
(Fdb.lookup_host) on the hash table's paths and at the sizes where the kernel changes path, the optional
arguments, the upload rules, and in one stream behind the route lookup and in front of the fused forward."""
import numpy as np
import pytest

import netflow_amd as nf
import oracle
from l2_common import (RUNS, decide_host, entries_of, fixture_fdb, fixture_ports, frame_of, l2_fixture, random_macs,
                       set_ports, wrapping_table)
from route_common import decide_host as route_decide_host
from route_common import fixture_fib, route_fixture

pytestmark = pytest.mark.gpu

OUTS = ("verdict", "vlan", "learn")


@pytest.fixture(scope="module")
def fx():
    return l2_fixture()


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


def run_l2(engine, fdb, ingress, arena, desc, want=OUTS, rt_verdict=None, upload=True):
    """(egress port, verdict, vlan, learn) from the device; the optional outputs not named in `want` are
    passed as NULL and come back as None. Every output buffer starts as 0xEE bytes and has one element
    more than n, which must stay as it was."""
    n = len(desc)
    if upload:
        fdb.upload(engine)
    d_arena = engine.alloc(arena.nbytes).upload(arena)
    d_desc = engine.alloc(max(desc.nbytes, 16)).upload(desc)
    size = {"port": 4, "verdict": 1, "vlan": 2, "learn": 1}
    bufs = {k: engine.alloc(size[k] * (n + 1) + 16).upload(np.full(size[k] * (n + 1) + 16, 0xEE, np.uint8))
            for k in ("port",) + tuple(want)}
    d_rt = None if rt_verdict is None else engine.alloc(max(n, 16)).upload(np.asarray(rt_verdict, np.uint8))
    engine.l2_lookup_device(fdb, ingress, d_arena, arena.nbytes, d_desc, n, bufs["port"], rt_verdict=d_rt,
                            verdict=bufs.get("verdict"), vlan=bufs.get("vlan"), learn=bufs.get("learn"))
    engine.sync()
    assert np.array_equal(d_arena.download(np.uint8, arena.nbytes), arena), "the lookup wrote into the frames"
    dt = {"port": np.uint32, "verdict": np.uint8, "vlan": np.uint16, "learn": np.uint8}
    out = []
    for k in ("port",) + OUTS:
        if k not in bufs:
            out.append(None)
            continue
        a = bufs[k].download(dt[k], n + 1)
        assert a[n] == np.array(0xEEEEEEEE).astype(dt[k]), f"{k}: a store past element n"
        out.append(a[:n].copy())
    return tuple(out)


def check(got, want):
    """want = (verdict, egress, vlan, learn) as decide_host and the fixture give them."""
    port, verdict, vlan, learn = got
    assert np.array_equal(port, want[1])
    for g, w in ((verdict, want[0]), (vlan, want[2]), (learn, want[3])):
        if g is not None:
            assert np.array_equal(g, w)


def fixture_want(z, run):
    return tuple(z[f"{k}_{run}"] for k in ("verdict", "egress", "vlan", "learn"))


@pytest.mark.parametrize("align", [16, 128])
@pytest.mark.parametrize("run", RUNS)
def test_fixture_matches_reference(engine, fx, run, align):
    z, frames = fx
    arena, desc = oracle.pack_frames(frames, align=align)
    with fixture_fdb(z) as fdb:
        got = run_l2(engine, fdb, int(z["ingress"][run]), arena, desc)
    check(got, fixture_want(z, run))


@pytest.mark.parametrize("first_start", [96, 112])
@pytest.mark.parametrize("run", RUNS)
def test_frame_starts_late_in_their_lines(engine, fx, run, first_start):
    """Frames whose headers begin 96 or 112 bytes into a 128-byte line: bytes 0..31 cross into the next
    line, bytes 0..15 end at the line's last byte."""
    z, frames = fx
    starts = [256 * i + (96, 112)[(i + first_start // 16) % 2] for i in range(len(frames))]
    arena, desc = pack_at(frames, starts)
    assert all(int(d["off16"]) * 16 % 128 >= 96 for d in desc)
    with fixture_fdb(z) as fdb:
        got = run_l2(engine, fdb, int(z["ingress"][run]), arena, desc)
    check(got, fixture_want(z, run))


@pytest.mark.parametrize("left_out", ["verdict", "vlan", "learn", "rt_verdict", "all"])
def test_optional_arguments_left_out(engine, fx, left_out):
    """Each optional output NULL in turn (and all of them): the others keep their meaning. rt_verdict NULL
    decides every frame; given as all-NOT_IPV4 it decides every frame too."""
    z, frames = fx
    arena, desc = oracle.pack_frames(frames)
    want = tuple(k for k in OUTS if k != left_out and left_out != "all")
    rt = None if left_out in ("rt_verdict", "all") else np.full(len(frames), nf.RT_NOT_IPV4, np.uint8)
    with fixture_fdb(z) as fdb:
        got = run_l2(engine, fdb, int(z["ingress"][0]), arena, desc, want=want, rt_verdict=rt)
    assert [g is not None for g in got[1:]] == [k in want for k in OUTS]
    check(got, fixture_want(z, 0))


def test_route_verdicts_select_the_frames(engine, fx):
    """Every NFCS_RT_* value in turn over the fixture: NOT_IPV4 is decided here, BAD_DESC reads
    NFCS_L2_BAD_DESC, every other value NFCS_L2_SKIP; neither reads a frame's learn class or VLAN."""
    z, frames = fx
    arena, desc = oracle.pack_frames(frames)
    rt = (np.arange(len(frames)) % 8).astype(np.uint8)
    want = [a.copy() for a in fixture_want(z, 0)]
    for k, none in enumerate((nf.L2_SKIP, nf.IF_NONE, 0, nf.L2_LEARN_NONE)):
        want[k][rt != nf.RT_NOT_IPV4] = none
    want[0][rt == nf.RT_BAD_DESC] = nf.L2_BAD_DESC
    with fixture_fdb(z) as fdb:
        got = run_l2(engine, fdb, int(z["ingress"][0]), arena, desc, rt_verdict=rt)
    check(got, want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_sizes_and_bad_descriptors(engine, fx, n):
    """Wave and workgroup edges (64 packets per wave, 256 per workgroup) on slices of the fixture, then
    the first and the last descriptor reaching outside the arena: NFCS_L2_BAD_DESC for those two, their
    neighbours as before."""
    z, frames = fx
    sel = [(7 * i) % len(frames) for i in range(n)]
    frames = [frames[i] for i in sel]
    arena, desc = oracle.pack_frames(frames)
    want = [a[sel].copy() for a in fixture_want(z, 1)]
    with fixture_fdb(z) as fdb:
        check(run_l2(engine, fdb, int(z["ingress"][1]), arena, desc), want)
        bad = desc.copy()
        bad[0]["off16"] = arena.nbytes // 16  # starts at the arena's end
        if int(bad[0]["len"]) == 0:
            bad[0]["len"] = 1
        bad[n - 1]["len"] = arena.nbytes - int(bad[n - 1]["off16"]) * 16 + 1  # one byte past it
        got = run_l2(engine, fdb, int(z["ingress"][1]), arena, bad)
    for i in {0, n - 1}:
        want[0][i], want[1][i], want[2][i], want[3][i] = nf.L2_BAD_DESC, nf.IF_NONE, 0, nf.L2_LEARN_NONE
    check(got, want)


def test_no_frames_is_ok_without_a_launch(engine):
    with nf.Fdb().commit() as fdb:
        fdb.upload(engine)
        engine.l2_lookup_device(fdb, 0, None, 0, None, 0, None)  # n == 0: nothing is looked at
        engine.sync()


def test_upload_semantics(engine):
    """Not uploaded: an argument error. After a setter without a new upload the device still answers from
    the old table; after commit and upload from the new one."""
    m = random_macs(np.random.default_rng(3), 2)
    frames = [frame_of(m[0], m[1]), frame_of(m[1], m[0])]
    arena, desc = oracle.pack_frames(frames)
    ports = [1, 2]
    buf = engine.alloc(64)
    with nf.Fdb().set_entries(entries_of(m[:1], [1], [1])) as fdb:
        for p in (0, 1, 2):
            fdb.set_port(p, native_vlan=1)
        fdb.commit()
        with pytest.raises(nf.NfcsError):
            engine.l2_lookup_device(fdb, 0, buf, 64, buf, 1, buf)
        old = decide_host(fdb, 0, frames)
        assert list(old[0]) == [nf.L2_FORWARD, nf.L2_FLOOD] and list(old[3]) == [nf.L2_LEARN_NEW, nf.L2_LEARN_MOVED]
        check(run_l2(engine, fdb, 0, arena, desc), old)
        fdb.set_entries(entries_of(m, [1, 1], ports))  # invalidates the commit, not the upload
        with pytest.raises(nf.NfcsError):
            fdb.lookup_host(0, frames[0])
        check(run_l2(engine, fdb, 0, arena, desc, upload=False), old)
        fdb.commit()
        check(run_l2(engine, fdb, 0, arena, desc, upload=False), old)  # committed, not yet uploaded
        new = decide_host(fdb, 0, frames)
        assert list(new[0]) == [nf.L2_FORWARD, nf.L2_FORWARD] and list(new[1]) == ports
        check(run_l2(engine, fdb, 0, arena, desc), new)


def hit_and_miss_frames(rng, macs, vlans, absent):
    """Frames whose destination and source hit every entry, in both roles, and frames that miss."""
    frames = []
    for k in range(len(macs)):
        j = int(rng.integers(0, len(macs)))
        frames.append(frame_of(macs[k], macs[j], int(vlans[k])))           # destination hits entry k
        frames.append(frame_of(macs[j], macs[k], int(vlans[k])))           # source hits entry k
        frames.append(frame_of(macs[k], macs[k], int(vlans[k]) ^ 1))       # the MAC on another VLAN: both miss
        frames.append(frame_of(absent[k % len(absent)], macs[k], int(vlans[k])))
    return frames


def open_ports(fdb, n=8):
    """Ports 0 .. n-1 as TRUNKs that allow every VLAN, so a hit forwards unless it is on the ingress port."""
    for p in range(n):
        fdb.set_port(p, type=nf.L2_TRUNK, native_vlan=1, allowed_vlans=range(4096))
    return fdb


def test_wrapped_probe_sequences(engine):
    seed, macs, vlans, ports = wrapping_table()
    rng = np.random.default_rng(seed)
    frames = hit_and_miss_frames(rng, macs, vlans, random_macs(rng, 40))
    arena, desc = oracle.pack_frames(frames)
    with open_ports(nf.Fdb().set_entries(entries_of(macs, vlans, ports))).commit() as fdb:
        st = fdb.stats()
        assert st["wrapped"] > 0 and st["max_probe"] >= 3
        want = decide_host(fdb, 3, frames)
        assert {nf.L2_FORWARD, nf.L2_FLOOD, nf.L2_DROP_SAME_PORT} <= set(int(v) for v in want[0])
        assert set(int(v) for v in want[3]) == {nf.L2_LEARN_NEW, nf.L2_LEARN_REFRESH, nf.L2_LEARN_MOVED}
        check(run_l2(engine, fdb, 3, arena, desc), want)


def test_sixteen_slots_half_full(engine):
    rng = np.random.default_rng(17)
    macs = random_macs(rng, 8)
    vlans, ports = rng.integers(0, 4096, 8), rng.integers(0, 8, 8)
    frames = hit_and_miss_frames(rng, macs, vlans, random_macs(rng, 8))
    arena, desc = oracle.pack_frames(frames)
    with open_ports(nf.Fdb().set_entries(entries_of(macs, vlans, ports, [1, 0] * 4))).commit() as fdb:
        assert fdb.stats()["slots"] == 16 and fdb.stats()["entries"] == 8
        want = decide_host(fdb, int(ports[1]), frames)
        assert (want[0][0:32:4] != nf.L2_FLOOD).all() and (want[3][1:32:4] != nf.L2_LEARN_NEW).all()
        check(run_l2(engine, fdb, int(ports[1]), arena, desc), want)


def test_empty_table_floods_and_learns_everything(engine, fx):
    z, frames = fx
    frames = [f for f in frames if len(f) >= 14][:300]
    arena, desc = oracle.pack_frames(frames)
    with set_ports(nf.Fdb(), fixture_ports(z)).commit() as fdb:
        assert fdb.stats()["max_probe"] == 0
        port, verdict, _, learn = run_l2(engine, fdb, 0, arena, desc)
    assert (verdict == nf.L2_FLOOD).all() and (learn == nf.L2_LEARN_NEW).all() and (port == nf.IF_NONE).all()


def test_large_table_against_host(engine):
    """65,536 random entries (a 2 MiB table) and 8,192 frames, half of whose destinations and sources hit."""
    rng = np.random.default_rng(65536)
    n_e, n_f = 65536, 8192
    macs = random_macs(rng, n_e + n_f)
    vlans, ports = rng.integers(0, 4096, n_e), rng.integers(0, 8, n_e)
    pick_d, pick_s = rng.integers(0, n_e, n_f), rng.integers(0, n_e, n_f)
    frames = []
    for i in range(n_f):
        d = macs[pick_d[i]] if i % 2 == 0 else macs[n_e + i]      # even frames: the destination hits
        s = macs[pick_s[i]] if i % 4 < 2 else macs[n_e + i]       # frames 0, 1 of four: the source is a known MAC
        frames.append(frame_of(d, s, int(vlans[pick_d[i]]), length=18))
    arena, desc = oracle.pack_frames(frames)
    with open_ports(nf.Fdb().set_entries(entries_of(macs[:n_e], vlans, ports, rng.integers(0, 2, n_e)))).commit() as fdb:
        st = fdb.stats()
        assert st["entries"] == n_e and st["slots"] == 2 * n_e and st["max_probe"] >= 3
        want = decide_host(fdb, 5, frames)
        assert ((want[0] == nf.L2_FLOOD) == (np.arange(n_f) % 2 == 1)).all()
        check(run_l2(engine, fdb, 5, arena, desc), want)


@pytest.mark.parametrize("table", ["a", "b"])
def test_behind_the_route_lookup_in_one_stream(engine, table):
    """route_lookup_device(verdict) -> l2_lookup_device(rt_verdict = that) -> l3_forward_device on one
    stream with no host step, on the route fixture's frames: SKIP exactly where the route verdict is
    neither NOT_IPV4 nor BAD_DESC, the rest equal lookup_host, and the forward's bytes equal the oracle's."""
    z, frames = route_fixture()
    arena, desc = oracle.pack_frames(frames)
    n = len(desc)
    with fixture_fib(z, table) as fib:
        want_rt, want_nh, _ = route_decide_host(fib, frames)
        l2_frames = [f for f, v in zip(frames, want_rt) if v == nf.RT_NOT_IPV4 and len(f) >= 14]
        assert len(l2_frames) >= 40
        # an FDB that knows the destination of every other such frame, over three ports
        macs = np.unique(np.array([np.frombuffer(f[:6], np.uint8) for f in l2_frames[::2]]), axis=0)
        with nf.Fdb().set_entries(entries_of(macs, np.ones(len(macs)), 1 + np.arange(len(macs)) % 3)) as fdb:
            for p in range(4):
                fdb.set_port(p, native_vlan=1)
            fdb.commit()
            want = [a.copy() for a in decide_host(fdb, 0, frames)]
            mine = want_rt == nf.RT_NOT_IPV4
            for k, none in enumerate((nf.L2_SKIP, nf.IF_NONE, 0, nf.L2_LEARN_NONE)):
                want[k][~mine] = none
            assert (want[0] == nf.L2_SKIP).sum() > n // 4 and (want[0] == nf.L2_FORWARD).sum() >= 10
            nht = fib.nexthops_host()
            fib.upload(engine)
            fdb.upload(engine)
            d_tab, tab_n = fib.nexthops()
            d_arena = engine.alloc(arena.nbytes).upload(arena)
            d_desc = engine.alloc(desc.nbytes).upload(desc)
            d_nh, d_rt, d_st = engine.alloc(4 * n), engine.alloc(n), engine.alloc(n)
            d_port, d_v, d_vl, d_le = engine.alloc(4 * n), engine.alloc(n), engine.alloc(2 * n), engine.alloc(n)
            engine.route_lookup_device(fib, d_arena, arena.nbytes, d_desc, n, d_nh, verdict=d_rt)
            engine.l2_lookup_device(fdb, 0, d_arena, arena.nbytes, d_desc, n, d_port, rt_verdict=d_rt, verdict=d_v,
                                    vlan=d_vl, learn=d_le)
            engine.l3_forward_device(d_arena, arena.nbytes, d_desc, d_nh, n, d_tab, tab_n, d_st)
            engine.sync()
            got = (d_port.download(np.uint32, n), d_v.download(np.uint8, n), d_vl.download(np.uint16, n),
                   d_le.download(np.uint8, n))
            rt, out, st = d_rt.download(np.uint8, n), d_arena.download(np.uint8, arena.nbytes), d_st.download(np.uint8, n)
    assert np.array_equal(rt, want_rt)
    check(got, want)
    ref = arena.copy()
    rst = oracle.l3_forward_batch(ref, desc, want_nh, nht.view(np.uint8).reshape(-1, 12))
    assert ((rst & nf.ST_FLAG_FWD) != 0).sum() > n // 4
    assert np.array_equal(st, rst) and np.array_equal(out, ref)
