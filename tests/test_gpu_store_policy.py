"""The form of large long-frame updates (netflow_amd/csrc/nfcs_store_policy.h, nfcs_api.hip
update_device): deferred (sub-batches, records, a write pass) or sparse (one inline launch), chosen from the
store demand that the read pass counts and the next call forwards to the host. The form changes speed only,
so every case compares the whole arena and the status bytes with the oracle.

The smallest burst that reaches the forms is just over 65,536 long frames: 66,005 frames of 1400-1500 bytes
(not a multiple of 16) at 16-byte and at 128-byte starts. The frames are test_gpu_store_skip's: the fuzz
generator's, their checksum fields set per class.

  stale   the nine field classes of test_gpu_store_skip, each at least 5% of the burst, with IP options,
          IHL < 5, tagged frames and a bad descriptor;
  quiet   the same without uncommon headers (the cold path counts as a store whatever its bytes, and the
          IHL < 5 update is not idempotent): after one update nothing in it needs a store;
  needy   quiet frames that all have a checksum field, all wrong: every packet needs a store.

When an observation can arrive: a call's count is forwarded by the NEXT call's first wave, so with a sync
after every call the host sees call k's count when it launches call k + 2. Call 1 (stale frames) observes
"high"; calls 2 and 3 observe "nothing to store", which calls 4 and 5 read: call 5, the fourth repeat on the
now-right frames, is the first that can run sparse, and must. Likewise a stale burst on a sparse context is
read two calls later."""
import ctypes
import functools

import numpy as np
import pytest

import netflow_amd as nf
import oracle
import test_gpu_store_skip as ss

pytestmark = pytest.mark.gpu

N = 66005
LO, HI = 1400, 1500


def sampled_packets(n):
    """The packets one launch over n packets samples: workgroups 0, 64, 128, ... of 16 packets each."""
    return n // 1024 * 16 + min(n % 1024, 16)


def common_header(f):
    """Whether the update takes the frame as anything but IPv4 with an uncommon header (IP options, IHL < 5):
    by the oracle's status, since what counts as IPv4 is the reference's decision."""
    _, st = oracle.update_frame(f)
    if st & nf.ST_FLAG_OVERLAP:
        return False
    if not (nf.ST_V4 <= (st & 0x3F) <= nf.ST_V4_L4SKIP):
        return True
    l2 = 18 if (f[12] == 0x81 and f[13] == 0x00) else 14
    return (f[l2] & 15) == 5


@functools.lru_cache(maxsize=None)
def spoiled(kind):
    """About N / 16 distinct frames of 1400-1500 bytes, their checksum fields set per class."""
    pick = [f for f in ss.pool() if LO <= len(f) <= HI and (kind == "stale" or common_header(f))]
    m = (N + 15) // 16
    assert len(pick) >= m, (kind, len(pick))
    return ss.spoil(pick[:m], 1000 + m)


def freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def burst(kind, align):
    """(arena, desc, ref, rst, ref2, rst2): the burst, the oracle's bytes and status after one call and
    after a second one. Shared, never modified."""
    frames = (spoiled(kind) * 16)[:N]
    arena, desc = oracle.pack_frames(frames, align=align)
    desc = desc.copy()
    desc[N // 3]["off16"] = arena.nbytes // 16  # a bad descriptor: starts at the end of the arena
    ref = arena.copy()
    rst, _ = oracle.update_batch(ref, desc, nthreads=8)
    assert rst[N // 3] == nf.ST_BAD_DESC
    ref2 = ref.copy()
    rst2, _ = oracle.update_batch(ref2, desc, nthreads=8)
    if kind == "quiet":
        assert np.array_equal(ref2, ref) and np.array_equal(rst2, rst)
    else:
        live = np.arange(N) != N // 3
        shares = ss.class_shares(arena, ref, desc[live], rst[live])
        for k in ss.CLASSES:
            assert shares[k] >= 0.05, (k, shares[k])
        assert (rst & nf.ST_FLAG_OVERLAP).any()  # IHL < 5
    return freeze(arena, desc, ref, rst, ref2, rst2)


@functools.lru_cache(maxsize=None)
def needy(align):
    """(arena, desc, ref, rst): quiet frames that have a checksum field, one byte of it wrong in each."""
    keep = []
    for f in spoiled("quiet"):
        g, st = oracle.update_frame(f)
        if (st & 0x3F) not in (nf.ST_NONE,) and g != f:
            keep.append(g)
    frames = (keep * (N // len(keep) + 1))[:N]
    ref, desc = oracle.pack_frames(frames, align=align)
    rst, _ = oracle.update_batch(ref.copy(), desc, nthreads=8)
    ip, l4, _, _, ov = ss.fields(ref, desc, rst)
    assert not ov.any() and ((ip >= 0) | (l4 >= 0)).all()
    arena = ref.copy()
    pos = np.where(ip >= 0, ip, l4)
    arena[pos] ^= 0x5A
    chk = arena.copy()
    cst, _ = oracle.update_batch(chk, desc, nthreads=8)
    assert np.array_equal(chk, ref) and np.array_equal(cst, rst)
    return freeze(arena, desc, ref, rst)


class Dev:
    """A burst on the device."""

    def __init__(self, eng, arena, desc):
        self.eng, self.n, self.nbytes = eng, len(desc), arena.nbytes
        self.arena = eng.alloc(arena.nbytes).upload(arena)
        self.desc = eng.alloc(desc.nbytes).upload(desc)
        self.st = eng.alloc(self.n)

    def update(self, patch=None, stream=None):
        self.st.upload(np.full(self.n, 0xEE, dtype=np.uint8))
        self.eng.update_device(self.arena, self.nbytes, self.desc, self.n, self.st, patch, stream=stream)
        self.eng.sync(stream)
        return self.eng.store_state()[0]

    def check(self, ref, rst):
        assert np.array_equal(self.st.download(np.uint8, self.n), rst)
        assert np.array_equal(self.arena.download(np.uint8, self.nbytes), ref)

    def free(self):
        for b in (self.arena, self.desc, self.st):
            b.free()


def make_sparse(eng, dev):
    """Synchronised calls on a burst with nothing to store until the context runs sparse: the fourth on
    frames that are already right (two observations, each read two calls after its own)."""
    forms = [dev.update() for _ in range(4)]
    assert forms[-1] == nf.STORE_SPARSE, forms
    return forms


@pytest.fixture()
def eng():
    with nf.Engine(0) as e:
        yield e


@pytest.mark.parametrize("align", [16, 128])
def test_auto_turns_sparse_on_no_store_calls(eng, align):
    arena, desc, ref, rst, _, _ = burst("quiet", align)
    d = Dev(eng, arena, desc)
    try:
        assert eng.store_state() == (0, 0, 0)
        forms = [d.update()]
        assert forms[0] == nf.STORE_DEFERRED
        d.check(ref, rst)
        for _ in range(4):  # the repeats, on frames that are now right
            forms.append(d.update())
            d.check(ref, rst)  # unchanged
        print("forms", forms, "observation", eng.store_state()[1:])
        assert forms[4] == nf.STORE_SPARSE, forms
        assert forms[:3] == [nf.STORE_DEFERRED] * 3, forms  # never on fewer than two low observations
    finally:
        d.free()


@pytest.mark.parametrize("align", [16, 128])
def test_auto_turns_back_on_a_stale_burst(eng, align):
    qa, qd, qref, qrst, _, _ = burst("quiet", align)
    arena, desc, ref, rst, _, _ = burst("stale", align)
    q = Dev(eng, qref, qd)
    d = Dev(eng, arena, desc)
    try:
        make_sparse(eng, q)
        # the stale burst in the sparse form: inline stores in the long shape above 65,536 packets
        assert d.update() == nf.STORE_SPARSE
        d.check(ref, rst)
        forms = [q.update() for _ in range(3)]
        print("forms after the stale burst", forms)
        assert nf.STORE_DEFERRED in forms, forms
        q.check(qref, qrst)
    finally:
        q.free()
        d.free()


@functools.lru_cache(maxsize=None)
def one_in_20(align):
    """The stale burst updated, with every 20th packet's original (stale) frame put back."""
    arena, desc, ref, _, _, _ = burst("stale", align)
    mixed = ref.copy()
    for i in range(0, N, 20):
        o, ln = int(desc[i]["off16"]) * 16, int(desc[i]["len"])
        if o + ln <= arena.size:
            mixed[o:o + ln] = arena[o:o + ln]
    exp = mixed.copy()
    est, _ = oracle.update_batch(exp, desc, nthreads=8)
    return freeze(mixed, desc, exp, est)


@pytest.mark.parametrize("align", [16, 128])
def test_forced_forms_are_bit_identical(eng, align):
    mixed, desc, exp, est = one_in_20(align)
    out = {}
    for policy in (nf.STORE_DEFERRED, nf.STORE_SPARSE):
        eng.set_store_policy(policy)
        d = Dev(eng, mixed, desc)
        try:
            assert d.update() == policy
            out[policy] = (d.arena.download(np.uint8, mixed.nbytes), d.st.download(np.uint8, N))
        finally:
            d.free()
    assert np.array_equal(out[nf.STORE_DEFERRED][0], out[nf.STORE_SPARSE][0])
    assert np.array_equal(out[nf.STORE_DEFERRED][1], out[nf.STORE_SPARSE][1])
    assert np.array_equal(out[nf.STORE_SPARSE][0], exp) and np.array_equal(out[nf.STORE_SPARSE][1], est)
    with pytest.raises(nf.NfcsError):
        eng.set_store_policy(3)


def test_caller_patch_stays_deferred(eng):
    """A call with d_patch runs deferred on a context that AUTO turned sparse and under forced SPARSE, and
    its records hold every field, changed or not."""
    qa, qd, qref, qrst, _, _ = burst("quiet", 16)
    arena, desc, ref, rst, _, _, _ = ss.burst("deferred")
    n = len(desc)
    q = Dev(eng, qref, qd)
    try:
        make_sparse(eng, q)
        for policy in (nf.STORE_AUTO, nf.STORE_SPARSE):
            eng.set_store_policy(policy)
            assert q.update() == nf.STORE_SPARSE
            d = Dev(eng, arena, desc)
            pt = eng.alloc(8 * n).upload(np.full(8 * n, 0xA5, dtype=np.uint8))
            try:
                assert d.update(patch=pt) == nf.STORE_DEFERRED
                d.check(ref, rst)
                ss.check_records(pt.download(nf.PATCH_DTYPE, n), arena, desc, ref, rst)
            finally:
                pt.free()
                d.free()
    finally:
        q.free()


def boundary_burst():
    """(arena, desc, ref, rst) of 2^19 + 36 frames of 1400 bytes, UDP over IPv4 with random payloads; every
    other packet's checksum fields are stale. 2,048 distinct frames, repeated."""
    n, ln, slot, m = (1 << 19) + 36, 1400, 1408, 2048
    rng = np.random.default_rng(77)
    fr = rng.integers(0, 256, (m, slot), dtype=np.uint8)
    fr[:, ln:] = 0
    fr[:, 12:14] = (0x08, 0x00)
    fr[:, 14] = 0x45
    fr[:, 16:18] = ((ln - 14) >> 8, (ln - 14) & 0xFF)
    fr[:, 20:22] = 0  # no fragments
    fr[:, 23] = 17
    fr[:, 38:40] = ((ln - 34) >> 8, (ln - 34) & 0xFF)
    good = fr.reshape(-1).copy()
    d0 = np.zeros(m, dtype=oracle.DESC_DTYPE)
    d0["off16"] = np.arange(m) * (slot // 16)
    d0["len"] = ln
    st0, _ = oracle.update_batch(good, d0, nthreads=8)
    assert (st0 == nf.ST_V4_UDP).all()
    good = good.reshape(m, slot)
    base = np.where((np.arange(m) % 2 == 0)[:, None], fr, good)  # even rows stale, odd rows right
    assert (base[0::2] != good[0::2]).any(axis=1).all()
    reps = (n + m - 1) // m
    arena = np.tile(base, (reps, 1))[:n].reshape(-1)
    ref = np.tile(good, (reps, 1))[:n].reshape(-1)
    desc = np.zeros(n, dtype=oracle.DESC_DTYPE)
    desc["off16"] = np.arange(n, dtype=np.int64) * (slot // 16)
    desc["len"] = ln
    chk = arena[:m * slot].copy()
    cst, _ = oracle.update_batch(chk, desc[:m], nthreads=8)  # the oracle on the distinct frames (the rest repeat them)
    assert np.array_equal(chk, ref[:m * slot]) and (cst == nf.ST_V4_UDP).all()
    return arena, desc, ref, np.full(n, nf.ST_V4_UDP, dtype=np.uint8)


def test_across_the_sub_batch_boundary(eng):
    """Forced SPARSE runs as one launch across what DEFERRED splits into two sub-batches."""
    arena, desc, ref, rst = boundary_burst()
    d = Dev(eng, arena, desc)
    try:
        for policy in (nf.STORE_SPARSE, nf.STORE_DEFERRED):
            eng.set_store_policy(policy)
            d.arena.upload(arena)
            assert d.update() == policy
            d.check(ref, rst)
    finally:
        d.free()


@pytest.mark.parametrize("policy", [nf.STORE_AUTO, nf.STORE_SPARSE])
def test_observation_reports_what_was_stored(eng, policy):
    arena, desc, ref, rst = needy(16)
    eng.set_store_policy(policy)
    d = Dev(eng, arena, desc)
    try:
        d.update()  # every packet stores
        d.check(ref, rst)
        assert eng.store_state()[1:] == (0, 0)  # nothing forwarded yet
        d.update()  # nothing to store; forwards the first call's count
        form, sampled, storing = eng.store_state()
        print("all stale:", sampled, storing)
        assert sampled == sampled_packets(N) and storing == sampled
        d.update()  # forwards the second call's
        form, sampled, storing = eng.store_state()
        print("all right:", sampled, storing)
        assert sampled == sampled_packets(N) and storing == 0
        d.check(ref, rst)
    finally:
        d.free()


def test_stream_change_resets_the_form(eng):
    qa, qd, qref, qrst, _, _ = burst("quiet", 16)
    hip = ctypes.CDLL("libamdhip64.so.7")
    st = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(st)) == 0
    q = Dev(eng, qref, qd)
    try:
        make_sparse(eng, q)
        assert q.update(stream=st.value) == nf.STORE_DEFERRED  # a second stream after calls on the first
        q.check(qref, qrst)
        assert q.update(stream=st.value) == nf.STORE_DEFERRED  # and its observations start over
        forms = [q.update(stream=st.value) for _ in range(4)]
        assert forms[-1] == nf.STORE_SPARSE, forms
        assert q.update() == nf.STORE_DEFERRED  # back on the context's own stream
        q.check(qref, qrst)
    finally:
        q.free()
        hip.hipStreamDestroy(st)
