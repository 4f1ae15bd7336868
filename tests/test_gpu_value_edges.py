"""Checksum value edges on the device: the frames of tests/value_edge_common.py (checksums that come
out as exactly 0x0000 and 0xFFFF, a region whose exact sum is 0, sums that need the second fold step, odd tails of
0xFF, saturated frames whose exact sum passes 2^31) through every site that finishes a checksum and every
instantiation of it: the plain update in its three shapes with inline stores, caller's records, the deferred write
pass and the sparse form; the fused forward inline and through its deferred records; VLAN push / pop / pop in its
three store forms; the ICMP responder; flow keys for the saturated frames. Every case compares the whole arena and
the status bytes with the oracle (pinned to the reference on these very frames by tests/test_value_edges.py), and
every device buffer carries guard bytes behind it that must stay as they were."""
import functools

import numpy as np
import pytest

import netflow_amd as nf
import oracle
import test_gpu_store_skip as ss
import value_edge_common as ve
from icmp_common import assert_same_respond, device_respond, messages_of, pack_with_region, round_up, small_tables

pytestmark = pytest.mark.gpu

GUARD = 256
SHAPE_HINT = {"tiny": 128, "short": 1024, "long": 4096}  # nfcs_ctx_set_slot_bytes: 8-lane rows / 16-lane rows / long waves


@pytest.fixture(scope="module")
def eng():
    """An engine of this module's own: the store form of large updates follows the context's history."""
    with nf.Engine(0) as e:
        yield e


class Buf:
    """A device buffer with GUARD bytes of 0xA5 behind it; free() asserts they are untouched."""

    def __init__(self, eng, src, fill=None):
        self.n = int(src) if isinstance(src, (int, np.integer)) else src.nbytes
        self.size = max(self.n, 16)
        self.d = eng.alloc(self.size + GUARD)
        host = np.full(self.size + GUARD, 0xA5, np.uint8)
        if not isinstance(src, (int, np.integer)):
            host[:self.n] = np.ascontiguousarray(src).view(np.uint8).reshape(-1)
        elif fill is not None:
            host[:self.n] = fill
        self.d.upload(host)

    def put(self, arr):
        self.d.upload(np.ascontiguousarray(arr).view(np.uint8).reshape(-1))

    def get(self, dtype, count):
        return self.d.download(dtype, count)

    def free(self):
        tail = self.d.download(np.uint8, GUARD, self.size)
        self.d.free()
        assert (tail == 0xA5).all(), "guard bytes behind a buffer were written"


def freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def packed(kind, align, room=0):
    return freeze(*oracle.pack_frames(ve.burst_frames(kind), align=align, room=room))


@functools.lru_cache(maxsize=None)
def update_case(kind, align):
    """(arena, desc, ref, rst, ref2, rst2): the burst and the oracle's bytes after one update and after a second."""
    arena, desc = packed(kind, align)
    ref = arena.copy()
    rst, _ = oracle.update_batch(ref, desc, nthreads=8)
    ref2 = ref.copy()
    rst2, _ = oracle.update_batch(ref2, desc, nthreads=8)
    return freeze(arena, desc, ref, rst, ref2, rst2)


@functools.lru_cache(maxsize=None)
def forward_case(kind, align):
    arena, desc = packed(kind, align)
    nh = ve.nh_index(len(desc))
    ref = arena.copy()
    rst = oracle.l3_forward_batch(ref, desc, nh, ve.NH_TABLE)
    ref2 = ref.copy()
    rst2 = oracle.l3_forward_batch(ref2, desc, nh, ve.NH_TABLE)
    return freeze(arena, desc, nh, ref, rst, ref2, rst2)


def run_update(eng, kind, align, hint, want_patch=False, policy=None):
    arena, desc, ref, rst, ref2, rst2 = update_case(kind, align)
    n = len(desc)
    bufs = []
    eng.set_slot_bytes(hint)
    if policy is not None:
        eng.set_store_policy(policy)
    try:
        d_arena, d_desc, d_st = Buf(eng, arena), Buf(eng, desc), Buf(eng, n)
        bufs = [d_arena, d_desc, d_st]
        d_pt = None
        if want_patch:
            d_pt = Buf(eng, 8 * n, fill=0xA5)
            bufs.append(d_pt)
        for exp, est in ((ref, rst), (ref2, rst2)):
            d_st.put(np.full(n, 0xEE, np.uint8))
            eng.update_device(d_arena.d, arena.nbytes, d_desc.d, n, d_st.d, None if d_pt is None else d_pt.d)
            eng.sync()
            if policy is not None:
                assert eng.store_state()[0] == (nf.STORE_DEFERRED if want_patch else policy)
            assert np.array_equal(d_st.get(np.uint8, n), est)
            assert np.array_equal(d_arena.get(np.uint8, arena.nbytes), exp)
            if want_patch and exp is ref:  # the records name the bytes now in the frames
                ss.check_records(d_pt.get(nf.PATCH_DTYPE, n), arena, desc, ref, rst)
        assert np.array_equal(d_desc.get(nf.DESC_DTYPE, n), desc)
    finally:
        eng.set_slot_bytes(0)
        eng.set_store_policy(nf.STORE_AUTO)
        for b in bufs:
            b.free()


def run_forward(eng, kind, align, hint):
    arena, desc, nh, ref, rst, ref2, rst2 = forward_case(kind, align)
    n = len(desc)
    bufs = []
    eng.set_slot_bytes(hint)
    try:
        d_arena, d_desc, d_nh, d_tab, d_st = Buf(eng, arena), Buf(eng, desc), Buf(eng, nh), Buf(eng, ve.NH_TABLE), Buf(eng, n)
        bufs = [d_arena, d_desc, d_nh, d_tab, d_st]
        for exp, est in ((ref, rst), (ref2, rst2)):
            d_st.put(np.full(n, 0xEE, np.uint8))
            eng.l3_forward_device(d_arena.d, arena.nbytes, d_desc.d, d_nh.d, n, d_tab.d, 4, d_st.d)
            eng.sync()
            assert np.array_equal(d_st.get(np.uint8, n), est)
            assert np.array_equal(d_arena.get(np.uint8, arena.nbytes), exp)
        assert np.array_equal(d_tab.get(np.uint8, 48), ve.NH_TABLE.reshape(-1))
    finally:
        eng.set_slot_bytes(0)
        for b in bufs:
            b.free()


def run_vlan(eng, frames, align, hint):
    """push (vid 4094, prio 6), pop, pop again, each against the oracle applied as many times."""
    arena, desc = oracle.pack_frames(frames, align=align, room=4)
    n = len(desc)
    caps = desc["len"].astype(np.uint32) + 4
    bufs = []
    eng.set_slot_bytes(hint)
    try:
        d_arena, d_desc, d_caps, d_st = Buf(eng, arena), Buf(eng, desc), Buf(eng, caps), Buf(eng, n)
        bufs = [d_arena, d_desc, d_caps, d_st]
        for op in (nf.vlan_push_op(4094, 6), nf.VLAN_POP, nf.VLAN_POP):
            rst = oracle.vlan_batch(arena, desc, None, caps, op_all=op)
            d_st.put(np.full(n, 0xEE, np.uint8))
            eng.vlan_device(d_arena.d, arena.nbytes, d_desc.d, n, None, op, d_caps.d, 0, d_st.d)
            eng.sync()
            assert np.array_equal(d_st.get(np.uint8, n), rst)
            assert np.array_equal(d_desc.get(nf.DESC_DTYPE, n), desc)
            assert np.array_equal(d_arena.get(np.uint8, arena.nbytes), arena)
    finally:
        eng.set_slot_bytes(0)
        for b in bufs:
            b.free()


# ---- the plain update ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("align", [16, 128])
@pytest.mark.parametrize("kind", ["tiny", "short", "long"])
def test_update_own_shape(eng, kind, align):
    """Each band in the shape its frames call for: 8-lane rows, 16-lane rows, long waves (at 16-byte starts their
    line-aligned windows begin off the frames)."""
    run_update(eng, kind, align, SHAPE_HINT[kind])


@pytest.mark.parametrize("kind,shape", [("long", "short"), ("long", "tiny"), ("short", "long"), ("tiny", "long"), ("tiny", "short")])
def test_update_other_shape(eng, kind, shape):
    """Long frames through the short shapes (several row passes per frame) and short ones through the long shape."""
    run_update(eng, kind, 16, SHAPE_HINT[shape])


@pytest.mark.parametrize("want_patch", [False, True])
def test_update_deferred(eng, want_patch):
    """66,000 long frames: above the inline limit, the values travel through the records and the write pass."""
    run_update(eng, "deferred", 16, 0, want_patch=want_patch)


@pytest.mark.parametrize("policy", [nf.STORE_SPARSE, nf.STORE_DEFERRED])
def test_update_deferred_forced_form(eng, policy):
    run_update(eng, "deferred", 16, 0, policy=policy)


# ---- the fused forward -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("align", [16, 128])
@pytest.mark.parametrize("kind", ["tiny", "short", "long"])
def test_forward_own_shape(eng, kind, align):
    run_forward(eng, kind, align, SHAPE_HINT[kind])


@pytest.mark.parametrize("kind,shape", [("long", "short"), ("long", "tiny"), ("short", "long"), ("tiny", "long"), ("tiny", "short")])
def test_forward_other_shape(eng, kind, shape):
    run_forward(eng, kind, 16, SHAPE_HINT[shape])


def test_forward_deferred(eng):
    """66,000 long frames: the values travel through the forward's 8-byte records and apply_fwd_kernel."""
    run_forward(eng, "deferred", 16, 0)


# ---- VLAN ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hint", [128, 512, 4096])
@pytest.mark.parametrize("kind", ["tiny", "short", "long"])
def test_vlan_push_pop_pop(eng, kind, hint):
    """A footprint below kVlanWtMeanBytes (8-lane rows, write-through), between it and kTinyMeanBytes (8-lane rows,
    stores past the caches) and above (16-lane rows)."""
    run_vlan(eng, ve.burst_frames(kind), 16, hint)


@pytest.mark.parametrize("align", [16, 128])
def test_vlan_packed_mix_follows_its_sample(eng, align):
    """Tiny and short frames in turn, packed, no hint: a mean footprint between kVlanWtMeanBytes and kTinyMeanBytes,
    so the push runs 8-lane rows storing past the caches and samples; the sample finds mixed lengths, and the pops
    store write-through."""
    frames = [f for pair in zip(ve.burst_frames("tiny")[:2048], ve.burst_frames("short")[:2048]) for f in pair]
    arena, _ = oracle.pack_frames(frames, align=align, room=4)
    assert 256 <= arena.nbytes // len(frames) < 800
    run_vlan(eng, frames, align, 0)


# ---- saturated frames ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("align", [16, 128])
@pytest.mark.parametrize("shape", ["tiny", "short", "long"])
def test_saturated_update(eng, shape, align):
    """All-0xFF frames up to the maximum sizes: the exact sum passes 2^31 (IPv6, payload_length 65535), so no
    accumulator, row sum or fold may take bit 31 for a sign, and the corrections must still come out exact."""
    run_update(eng, "saturated", align, SHAPE_HINT[shape])


@pytest.mark.parametrize("shape", ["tiny", "short", "long"])
def test_saturated_forward(eng, shape):
    run_forward(eng, "saturated", 16, SHAPE_HINT[shape])


@pytest.mark.parametrize("hint", [128, 512, 4096])
def test_saturated_vlan(eng, hint):
    run_vlan(eng, ve.burst_frames("saturated"), 16, hint)


def test_saturated_flow_keys(eng):
    """Flow keys compute no checksum; their records on the saturated frames must still match."""
    arena, desc = packed("saturated", 16)
    n = len(desc)
    recs, hashes = oracle.flow_keys_batch(arena, desc)
    bufs = [Buf(eng, arena), Buf(eng, desc), Buf(eng, 64 * n), Buf(eng, 4 * n)]
    try:
        eng.flow_keys_device(bufs[0].d, arena.nbytes, bufs[1].d, n, bufs[2].d, bufs[3].d)
        eng.sync()
        assert np.array_equal(bufs[2].get(np.uint8, 64 * n).reshape(n, 64), recs)
        assert np.array_equal(bufs[3].get(np.uint32, n), hashes)
        assert np.array_equal(bufs[0].get(np.uint8, arena.nbytes), arena)
    finally:
        for b in bufs:
            b.free()


# ---- ICMP ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def icmp_setup(eng):
    fib, icmp = small_tables()
    with fib, icmp:
        cases = ve.icmp_cases(icmp, fib)
        fib.upload(eng)
        icmp.upload(eng)
        yield fib, icmp, cases


def icmp_pick(cases, n, q):
    """n of the cases: one tuned reply alone; else every tuned request and error, the 65,507-byte payload, and the
    saturated payload lengths 4 j + q + 1 (mod 2,000), so that the four bursts of a size cover 1..2,000."""
    if n == 1:
        cls = ("icmp_zero", "icmp_sum_zero", "second_fold", "odd_tail_ff")[q]
        return [next(c for c in cases if c[0] == cls)]
    special = [c for c in cases if c[0] != "saturated"] + [cases[-15]]
    assert cases[-15][0] == "saturated" and len(cases[-15][1]) == 42 + 65507
    sat = [c for c in cases if c[0] == "saturated"]
    picked = special + [sat[(4 * j + q) % 2000] for j in range(n - len(special))]
    return [picked[(i * 7) % n] for i in range(n)] if n % 7 else picked


@pytest.mark.parametrize("msg_align", [16, 128])
@pytest.mark.parametrize("n,q", [(1, 0), (1, 3), (1024, 0), (1024, 2), (1025, 1), (1025, 3)])
def test_icmp_replies(eng, icmp_setup, n, q, msg_align):
    fib, icmp, cases = icmp_setup
    q = (q + (msg_align == 128)) % 4
    pick = icmp_pick(cases, n, q)
    frames = [c[1] for c in pick]
    verdict = np.array([c[2] for c in pick], np.uint8)
    ip_id = np.array([c[3] for c in pick], np.uint16)
    region = sum(round_up(len(f) + 64, msg_align) for f in frames)
    arena, desc, msg_base = pack_with_region(frames, 16, region, msg_align)
    host_arena = arena.copy()
    want = icmp.respond_host(fib, 1, host_arena, msg_base, msg_align, desc, verdict, n, ip_id=ip_id)
    got = device_respond(eng, icmp, fib, 1, arena, msg_base, msg_align, desc, verdict, n, ip_id=ip_id)
    assert_same_respond(got, want)
    assert np.array_equal(got["arena"], host_arena)
    msgs = messages_of(got["arena"], got)
    assert len(msgs) == n
    for (cls, _, _, _), (_, _, m) in zip(pick, msgs):
        hdr, body = bytearray(m[14:34]), bytearray(m[34:])
        hdr[10] = hdr[11] = body[2] = body[3] = 0
        assert ve.get16(m, 24) == ve.py_checksum(hdr) and ve.get16(m, 36) == ve.py_checksum(body), cls
        if cls == "icmp_zero":
            assert ve.get16(m, 36) == 0x0000
        if cls == "icmp_sum_zero":
            assert ve.get16(m, 36) == 0xFFFF and not any(body)
