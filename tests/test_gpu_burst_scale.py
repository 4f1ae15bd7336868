"""The enqueue, flood and ICMP stages on the device at bursts past one trip of the code that joins their tiles
(DESIGN.md §24): egress_scan_tiles_kernel with several tiles per segment, a second 8-group, segments that end inside a
group and trailing empty segments (17..257 tiles); flood_scan_kernel's second and third trip with a carry (257..513
tiles), for the flood stage and the ICMP responder; and the grow branch of the scratch buffer the three stages share.
Every comparison covers whole arrays, against the host walk and against the numpy model of burst_scale_common.py
(tests/test_burst_scale.py holds the two to each other without a GPU); the arena is compared whole where frames are
written; every device buffer carries guard bytes behind it that must stay as they were."""
import ctypes

import numpy as np
import pytest

import burst_scale_common as bs
import netflow_amd as nf
from egress_common import assert_same as assert_same_enqueue
from flood_common import assert_same_expand
from icmp_common import assert_same_respond, small_tables

pytestmark = pytest.mark.gpu

T = bs.T
GUARD = 256
EE = 0xEEEEEEEE
# tile-major, so that one burst serves the cases that follow it
FLOOD_CASES = [(t, x, a, c) for t, x in [(255, False), (256, False), (256, True), (257, False), (512, False), (513, False)]
               for a in (16, 128) for c in ("full", "cap_cut", "region_cut")]
ICMP_CASES = [(t, x, a, c) for t, x in [(256, True), (257, False), (513, False)]
              for a in (16, 128) for c in ("full", "cap_cut", "region_cut")]


class Buf:
    """A device buffer with GUARD bytes of 0xA5 behind it; free() asserts they are untouched."""

    def __init__(self, eng, src, fill=0xEE):
        """src: an array to upload, or a byte count to fill with `fill`."""
        whole = isinstance(src, (int, np.integer))
        self.n = int(src) if whole else src.nbytes
        self.size = max(self.n, 16)
        self.d = eng.alloc(self.size + GUARD)
        host = np.full(self.size + GUARD, 0xA5, np.uint8)
        host[:self.n] = fill if whole else np.ascontiguousarray(src).view(np.uint8).reshape(-1)
        self.d.upload(host)

    @property
    def ptr(self):
        return self.d.ptr

    def get(self, dtype, count):
        return self.d.download(dtype, count)

    def free(self):
        tail = self.d.download(np.uint8, GUARD, self.size)
        self.d.free()
        assert (tail == 0xA5).all(), "guard bytes behind a buffer were written"


def free_all(bufs):
    for b in bufs:
        b.free()


# ---- the enqueue -------------------------------------------------------------------------------------------

class Enqueue:
    """One egress_enqueue_device call: launch() uploads and launches, result() waits, downloads, checks the guards and
    returns the dict Egress.enqueue_host returns. d_depth: the depth buffer of an earlier call, to chain on."""

    def __init__(self, eng, eg, port, queue, depth=None, d_depth=None, stream=None):
        self.eng, self.n, self.keys = eng, len(port), eg.keys()[1]
        n, keys = self.n, self.keys
        self.d_port, self.d_queue = Buf(eng, np.ascontiguousarray(port, np.uint32)), Buf(eng, np.ascontiguousarray(queue, np.uint8))
        self.d_depth = d_depth if d_depth is not None else Buf(eng, np.ascontiguousarray(depth, np.uint32))
        self.d_order, self.d_ks = Buf(eng, 4 * n), Buf(eng, 4 * (keys + 1))
        self.d_res, self.d_drop = Buf(eng, n), Buf(eng, 4 * keys)
        self.eg, self.stream = eg, stream

    def launch(self):
        self.eng.egress_enqueue_device(self.eg, self.d_port.d, self.d_queue.d, self.n, self.d_depth.d, self.d_order.d,
                                       self.d_ks.d, result=self.d_res.d, key_dropped=self.d_drop.d, stream=self.stream)
        return self

    def result(self, keep_depth=False):
        n, keys = self.n, self.keys
        self.eng.sync()
        ks, order = self.d_ks.get(np.uint32, keys + 1), self.d_order.get(np.uint32, n)
        total = int(ks[keys])
        assert total <= n and (order[total:] == EE).all(), "entries of d_order past the total must stay as they were"
        out = {"key_start": ks, "order": order[:total], "depth": self.d_depth.get(np.uint32, keys),
               "result": self.d_res.get(np.uint8, n), "key_dropped": self.d_drop.get(np.uint32, keys)}
        free_all([self.d_port, self.d_queue, self.d_order, self.d_ks, self.d_res, self.d_drop] +
                 ([] if keep_depth else [self.d_depth]))
        return out


def check_enqueue(eng, eg, rows, port, queue, depth, what=""):
    """Device against the host walk and against the model."""
    host = eg.enqueue_host(port, queue, depth)
    model = bs.eq_model(port, queue, depth, *bs.eq_port_arrays(rows))
    got = Enqueue(eng, eg, port, queue, depth).launch().result()
    assert_same_enqueue(got, host, what + "against enqueue_host: ")
    assert_same_enqueue(got, model, what + "against the model: ")
    return model


@pytest.fixture(scope="module")
def tables(engine):
    made = {name: bs.make_egress(bs.eq_table(name)) for name in bs.EQ_TABLES}
    yield made
    for eg in made.values():
        eg.close()


@pytest.mark.parametrize("table,tiles,exact", bs.EQ_RANDOM_CASES)
def test_enqueue_random(engine, tables, table, tiles, exact):
    """Skewed keys with bad ports, bad queues and IF_NONE among the packets, at every tile count of EQ_TILES on the
    12-port table and on 65 keys, and at the sizes the other tables meet (burst_scale_common.EQ_RANDOM_CASES)."""
    rows, port, queue, depth = bs.eq_random_case(table, tiles, exact)
    eg = tables[table]
    eg.upload(engine)
    model = check_enqueue(engine, eg, rows, port, queue, depth, f"{table} {tiles}: ")
    assert len(set(model["result"].tolist())) == 5


@pytest.mark.parametrize("pattern", bs.EQ_PATTERNS)
@pytest.mark.parametrize("tiles", bs.EQ_PATTERN_TILES)
def test_enqueue_patterns(engine, tables, tiles, pattern):
    """A key only in the last segment's tiles, a key absent from segments 3..9, and a queue whose room ends in the
    second 8-group of a segment, at that segment's last tile, and in the burst's last tile."""
    port, queue, depth, meta = bs.eq_pattern(tiles, pattern)
    eg = tables["small12"]
    eg.upload(engine)
    model = check_enqueue(engine, eg, bs.eq_table("small12"), port, queue, depth, f"{pattern} {tiles}: ")
    if "cut" in meta:
        assert model["result"][meta["cut"]] == nf.EQ_ENQUEUED and model["result"][meta["next"]] == nf.EQ_DROP_FULL


def test_enqueue_second_call_chains_on_the_first_calls_depths_at_129_tiles(engine, tables):
    rows = bs.eq_table("small12")
    eg = tables["small12"]
    eg.upload(engine)
    _, port, queue, depth = bs.eq_random_case("small12", 129, False)
    has = bs.eq_port_arrays(rows)
    want1 = bs.eq_model(port, queue, depth, *has)
    want2 = bs.eq_model(port[::-1], queue[::-1], want1["depth"], *has)
    host2 = eg.enqueue_host(port[::-1], queue[::-1], eg.enqueue_host(port, queue, depth)["depth"])
    first = Enqueue(engine, eg, port, queue, depth).launch()
    second = Enqueue(engine, eg, port[::-1].copy(), queue[::-1].copy(), d_depth=first.d_depth).launch()  # no host step
    got1 = first.result(keep_depth=True)
    got2 = second.result()
    for k in ("result", "key_start", "key_dropped", "order"):  # the depth buffer by now holds the second call's
        assert np.array_equal(got1[k], want1[k]), "first: " + k
    assert_same_enqueue(got2, want2, "second against the model: ")
    assert_same_enqueue(got2, host2, "second against enqueue_host: ")
    assert want2["key_dropped"].sum() > want1["key_dropped"].sum() > 0


# ---- flood replication ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fdb(engine):
    with bs.make_fdb() as f:
        f.upload(engine)
        yield f, bs.flood_lists(f)


class Expand:
    """One flood_expand_device call over a flood_burst: the item arrays have `cap` entries."""

    def __init__(self, eng, f, b, align, arena_bytes, cap):
        self.eng, self.cap, self.arena_bytes = eng, cap, arena_bytes
        self.before = bs.with_region(b["frames"], b["copy_base"], arena_bytes)
        self.d_arena, self.d_desc = Buf(eng, self.before), Buf(eng, b["desc"])
        self.d_in = {k: Buf(eng, v) for k, v in b["arrays"].items()}
        self.d_idesc, self.d_iport, self.d_isrc, self.d_tot = Buf(eng, 8 * cap), Buf(eng, 4 * cap), Buf(eng, 4 * cap), Buf(eng, 32)
        eng.flood_expand_device(f, bs.FLOOD_INGRESS, bs.FLOOD_PORTS, self.d_arena.d, arena_bytes, b["copy_base"], align,
                                self.d_desc.d, b["n"], cap, self.d_idesc.d, self.d_iport.d, self.d_isrc.d, self.d_tot.d,
                                **{k: v.d for k, v in self.d_in.items()})

    def result(self, keep=()):
        self.eng.sync()
        cap = self.cap
        out = {"item_desc": self.d_idesc.get(nf.DESC_DTYPE, cap), "item_port": self.d_iport.get(np.uint32, cap),
               "item_src": self.d_isrc.get(np.uint32, cap), "totals": self.d_tot.get(nf.FLOOD_TOTALS_DTYPE, 1)[0],
               "arena": self.d_arena.get(np.uint8, self.arena_bytes)}
        free_all([x for x in [self.d_arena, self.d_desc, self.d_idesc, self.d_iport, self.d_isrc, self.d_tot] +
                  list(self.d_in.values()) if x not in keep])
        return out


def check_expand(eng, f, lists, b, align, arena_bytes, cap, what=""):
    """Device against the host walk and the model: items, totals, the inert padding, the whole arena."""
    host = f.flood_expand_host(bs.FLOOD_INGRESS, bs.FLOOD_PORTS, arena_bytes, b["copy_base"], align, b["desc"], cap, **b["arrays"])
    model = bs.flood_model(b, lists, align, arena_bytes, cap)
    run = Expand(eng, f, b, align, arena_bytes, cap)
    got = run.result()
    assert_same_expand(got, host, what + "against flood_expand_host: ")
    assert_same_expand(got, model, what + "against the model: ")
    want = bs.flood_arena_model(run.before, b, model)
    bad = np.flatnonzero(got["arena"] != want)
    assert len(bad) == 0, f"{what}the arena differs from the copy model at {bad[:8].tolist()} (copy_base {b['copy_base']})"
    return model


@pytest.mark.parametrize("tiles,exact,align,case", FLOOD_CASES)
def test_flood_expand(engine, fdb, tiles, exact, align, case):
    """One, two and three trips of the scan over the tile sums. full: cap and region hold everything; cap_cut: cap
    ends inside the items of a flooded packet of the last tile; region_cut: the region ends inside its copies."""
    f, lists = fdb
    b = bs.flood_burst(tiles, exact)
    arena_bytes, cap, p = bs.flood_case(b, lists, align, case)
    model = check_expand(engine, f, lists, b, align, arena_bytes, cap, f"{tiles} {align} {case}: ")
    items = int(model["totals"]["items"])
    if case == "full":
        assert items == int(model["totals"]["items_needed"]) == cap - 3
    else:
        assert 0 < items < int(model["totals"]["items_needed"]) and int(model["item_src"][items - 1]) == p
        assert p // T == tiles - 1


# ---- the ICMP responder ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def icmp_tables(engine):
    fib, icmp = small_tables()
    with fib, icmp:
        fib.upload(engine)
        icmp.upload(engine)
        yield fib, icmp


@pytest.mark.parametrize("tiles,exact,align,case", ICMP_CASES)
def test_icmp_respond(engine, icmp_tables, tiles, exact, align, case):
    """The same scan under the ICMP responder: status, message list, totals and the whole arena (every message's bytes)
    against respond_host, list and totals against the model."""
    fib, icmp = icmp_tables
    b = bs.icmp_burst(tiles, exact)
    n = b["n"]
    arena_bytes, cap, p = bs.icmp_case(b, align, case)
    model = bs.icmp_model(b, align, arena_bytes, cap)
    before = bs.with_region(b["frames"], b["msg_base"], arena_bytes)
    host_arena = before.copy()
    host = icmp.respond_host(fib, bs.ICMP_INGRESS, host_arena, b["msg_base"], align, b["desc"], b["verdict"], cap, ip_id=b["ip_id"])
    d_arena, d_desc, d_v, d_id = Buf(engine, before), Buf(engine, b["desc"]), Buf(engine, b["verdict"]), Buf(engine, b["ip_id"])
    d_md, d_mp, d_ms, d_st, d_tot = Buf(engine, 8 * cap), Buf(engine, 4 * cap), Buf(engine, 4 * cap), Buf(engine, n), Buf(engine, 32)
    engine.icmp_respond_device(icmp, fib, bs.ICMP_INGRESS, d_arena.d, arena_bytes, b["msg_base"], align, d_desc.d, n, d_v.d,
                               cap, d_md.d, d_mp.d, d_ms.d, d_tot.d, ip_id=d_id.d, status=d_st.d)
    engine.sync()
    got = {"msg_desc": d_md.get(nf.DESC_DTYPE, cap), "msg_port": d_mp.get(np.uint32, cap), "msg_src": d_ms.get(np.uint32, cap),
           "status": d_st.get(np.uint8, n), "totals": d_tot.get(nf.ICMP_TOTALS_DTYPE, 1)[0]}
    arena = d_arena.get(np.uint8, arena_bytes)
    free_all([d_arena, d_desc, d_v, d_id, d_md, d_mp, d_ms, d_st, d_tot])
    what = f"{tiles} {align} {case}: "
    assert_same_respond(got, host, what + "against respond_host: ")
    for k in ("messages", "messages_needed", "echo_replies", "errors", "msg_bytes", "msg_bytes_needed"):
        assert int(got["totals"][k]) == int(model["totals"][k]), what + "against the model: " + k
    assert np.array_equal(got["msg_desc"], model["msg_desc"]) and np.array_equal(got["msg_src"], model["msg_src"]), what
    assert (got["status"][model["overflow"]] == nf.ICMP_ST_OVERFLOW).all()
    assert not (got["status"][~model["overflow"]] == nf.ICMP_ST_OVERFLOW).any()
    bad = np.flatnonzero(arena != host_arena)
    assert len(bad) == 0, f"{what}the arena differs from the host walk's at {bad[:8].tolist()} (msg_base {b['msg_base']})"
    if case != "full":
        assert model["overflow"][p] and p // T == tiles - 1


# ---- one chain at 513 tiles --------------------------------------------------------------------------------------

def test_chain_expand_enqueue_append_dequeue_at_513_tiles(engine, fdb):
    """expand -> enqueue over the item list -> TX-queue append -> dequeue of everything, on one stream with no host
    step: item_port is the port, the queue a fixed function of the item index (k % 5: queue 4 is a bad queue), the
    handles the item descriptors. Against the same chain of host calls on a TxQueues object of this test's own."""
    f, lists = fdb
    b = bs.flood_burst(513)
    arena_bytes, cap, _ = bs.flood_case(b, lists, 16, "full")
    queue = (np.arange(cap) % 5).astype(np.uint8)
    rows = [(p, True, 4, 9000) for p in range(bs.FLOOD_PORTS)]
    with bs.make_egress(rows) as eg:
        eg.upload(engine)
        keys = eg.keys()[1]
        with nf.TxQueues(eg, engine) as txq:
            ports = txq.ports
            # the host chain
            ex = f.flood_expand_host(bs.FLOOD_INGRESS, bs.FLOOD_PORTS, arena_bytes, b["copy_base"], 16, b["desc"], cap, **b["arrays"])
            r = eg.enqueue_host(ex["item_port"], queue, np.zeros(keys, np.uint32))
            model = bs.eq_model(ex["item_port"], queue, np.zeros(keys, np.uint32), *bs.eq_port_arrays(rows))
            tx_cap, budget = int(r["key_start"][keys]), 4 * 9000
            txq.append_host(r["order"], r["key_start"], r["depth"], cap, desc=ex["item_desc"])
            want = txq.dequeue_host(r["depth"], tx_cap, budget_all=budget)
            assert int(want["tx_start"][ports]) == tx_cap > 100000 and not want["depth"].any()
            assert r["key_dropped"].sum() > 10000 and (r["result"] == nf.EQ_BAD_QUEUE).sum() > 50000
            assert (r["result"][int(ex["totals"]["items"]):] == nf.EQ_SKIP).all()
            # the device chain
            run = Expand(engine, f, b, 16, arena_bytes, cap)
            d_queue, d_depth = Buf(engine, queue), Buf(engine, np.zeros(keys, np.uint32))
            d_order, d_ks, d_res, d_drop = Buf(engine, 4 * cap), Buf(engine, 4 * (keys + 1)), Buf(engine, cap), Buf(engine, 4 * keys)
            d_tx, d_txq, d_start, d_deq = Buf(engine, 8 * tx_cap), Buf(engine, tx_cap), Buf(engine, 4 * (ports + 1)), Buf(engine, 4 * keys)
            engine.egress_enqueue_device(eg, run.d_iport.d, d_queue.d, cap, d_depth.d, d_order.d, d_ks.d, result=d_res.d,
                                         key_dropped=d_drop.d)
            engine.txq_append_device(txq, d_order.d, d_ks.d, d_depth.d, cap, desc=run.d_idesc.d)
            engine.txq_dequeue_device(txq, d_depth.d, d_tx.d, tx_cap, d_start.d, budget_all=budget, tx_queue=d_txq.d, dequeued=d_deq.d)
            got_ex = run.result()
            assert_same_expand(got_ex, ex, "expand: ")
            ks = d_ks.get(np.uint32, keys + 1)
            got = {"key_start": ks, "order": d_order.get(np.uint32, cap)[:int(ks[keys])], "result": d_res.get(np.uint8, cap),
                   "key_dropped": d_drop.get(np.uint32, keys)}
            assert_same_enqueue(got, r, "enqueue against enqueue_host: ")
            assert_same_enqueue(got, model, "enqueue against the model: ")
            assert np.array_equal(d_tx.get(np.uint64, tx_cap), want["tx"]), "tx"
            assert np.array_equal(d_txq.get(np.uint8, tx_cap), want["tx_queue"]), "tx_queue"
            assert np.array_equal(d_start.get(np.uint32, ports + 1), want["tx_start"]), "tx_start"
            assert np.array_equal(d_deq.get(np.uint32, keys), want["dequeued"]), "dequeued"
            assert np.array_equal(d_depth.get(np.uint32, keys), want["depth"]), "depth"
            head, last = txq.state_device()
            hh, hl = txq.state_host()
            assert np.array_equal(head, hh) and np.array_equal(last, hl)
            # the handles are the item descriptors of the enqueued items
            assert set(want["tx"].tolist()) == set(ex["item_desc"][r["order"]].view(np.uint64).tolist())
            free_all([d_queue, d_depth, d_order, d_ks, d_res, d_drop, d_tx, d_txq, d_start, d_deq])


# ---- the scratch buffer's grow branch ---------------------------------------------------------------------------

def growth_sequence(two_streams):
    """On a context of its own (the session's scratch may already be large): a 4-tile enqueue, the 129-tile enqueue on
    8,192 keys whose 129 * 8192 histogram words pass the scratch's first 2^18 and grow it, a 513-tile flood that fits
    the grown buffer, a 4-tile enqueue. With two_streams the first call runs on a caller's stream and the second
    follows on the context's own with no sync between: the grow branch then waits on the host for the first call
    before it frees the buffer that call uses."""
    hip = ctypes.CDLL("libamdhip64.so.7")
    small, big = bs.eq_table("small12"), bs.eq_table("big8192")
    with nf.Engine(0) as eng:
        st = ctypes.c_void_p()
        if two_streams:
            assert hip.hipStreamCreate(ctypes.byref(st)) == 0
        try:
            with bs.make_egress(small) as eg_s, bs.make_egress(big) as eg_b, bs.make_fdb() as f:
                for obj in (eg_s, eg_b, f):
                    obj.upload(eng)
                lists = bs.flood_lists(f)
                p1, q1, dep1 = bs.eq_random(small, bs.burst_n(4), 41)
                _, p2, q2, dep2 = bs.eq_random_case("big8192", 129, False)
                assert (4 + 2) * eg_s.keys()[1] < (1 << 18) < 129 * eg_b.keys()[1]
                first = Enqueue(eng, eg_s, p1, q1, dep1, stream=st.value if two_streams else None)
                second = Enqueue(eng, eg_b, p2, q2, dep2)
                eng.sync()
                first.launch()
                second.launch()  # grows the scratch
                if two_streams:
                    assert hip.hipStreamSynchronize(st) == 0
                got2 = second.result()
                got1 = first.result()
                for got, rows, eg, (p, q, d), what in ((got1, small, eg_s, (p1, q1, dep1), "call 1: "),
                                                       (got2, big, eg_b, (p2, q2, dep2), "call 2: ")):
                    assert_same_enqueue(got, eg.enqueue_host(p, q, d), what + "against enqueue_host: ")
                    assert_same_enqueue(got, bs.eq_model(p, q, d, *bs.eq_port_arrays(rows)), what + "against the model: ")
                b = bs.flood_burst(513)
                arena_bytes, cap, _ = bs.flood_case(b, lists, 16, "full")
                check_expand(eng, f, lists, b, 16, arena_bytes, cap, "call 3: ")
                p4, q4, dep4 = bs.eq_random(small, bs.burst_n(4), 44)
                check_enqueue(eng, eg_s, small, p4, q4, dep4, "call 4: ")
        finally:
            if two_streams:
                hip.hipStreamDestroy(st)


def test_scratch_grows_on_a_fresh_context():
    growth_sequence(False)


def test_scratch_grows_while_a_callers_stream_uses_it():
    """A missing wait in the grow branch would show only by timing (the first call is short); this pins the path's
    results, not the race."""
    growth_sequence(True)
