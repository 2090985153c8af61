"""Cases of the keyed score-and-ingest (gk_rank_ingest_keyed through
StreamSet.rank_ingest_keyed / score_ingest_keyed and KeyedStreamSet.score_add),
shared by tests/test_gpu_rank_ingest.py (device engine, k_rank_ingest_keyed) and
tests/test_cpu_rank_ingest.py (host engine); the engine is the ``dev``
parameter.

Two checks apply to every call (``fused``):
 * Oracle.  The occurring ``OracleGK``s are flushed, ``expected_rows`` of
   rankkeyed_cases gives lo / hi / n, then the batch is added to the oracles in
   arrival order; the rows are compared by bytes, every stream by
   ``select_cases.assert_all``.
 * Composition.  A twin set, built identically, is fed ``ranks_keyed`` then
   ``ingest_keyed``: ``rollup_cases.assert_sets_equal`` with the fused set and
   identical output bytes, fused quantiles included.
Test infrastructure only."""
import ctypes

import numpy as np
import pytest
import torch

import parity_util as U
import rank_cases as K
import rankkeyed_cases as Q
import rollup_cases as R
import select_cases as C
from gk_oracle import OracleGK

EPS = C.EPS
NAN = float("nan")
INF = float("inf")
I32_MIN = -2 ** 31
Q3 = [0.5, 0.9, 0.99]


def _bytes(t):
    return t.cpu().numpy().tobytes()


def oracle_step(oracles, ids, xs):
    """The definition on the oracles: flush the occurring streams, the expected
    rows, then the batch in arrival order.  Returns (lo, hi, n)."""
    K.flush_covered(oracles, {s for s in ids if s >= 0})
    rows = Q.expected_rows(oracles, ids, xs)
    for s, x in zip(ids, xs):
        if s >= 0:
            oracles[s].add(x)
    return rows


def twin_step(twin, ti, tx, quantiles=None, single=False):
    """The two-call spelling on the twin: (lo, hi, n, q)."""
    lo, hi, n = twin.ranks_keyed(ti, tx, n=True)
    q = twin.ingest_keyed(ti, tx, quantiles=quantiles, single=single)
    return lo, hi, n, q


def fused(ss, twin, oracles, ids, xs, what, before=True, quantiles=None, single=False):
    """rank_ingest_keyed(n=True) on `ss` against the oracles (a list, one per
    stream) and against the two calls on `twin` (None: no twin).  Returns the
    engine's tuple."""
    live = {s for s in ids if s >= 0}
    if before is True:
        before = R.snapshot(ss)
    elo, ehi, en = oracle_step(oracles, ids, xs)
    ti, tx = Q.tensors(ss, ids, xs)
    got = ss.rank_ingest_keyed(ti, tx, n=True, quantiles=quantiles, single=single)
    assert len(got) == (3 if quantiles is None else 4), what
    Q.same_i64(got[0], elo, what + " lo")
    Q.same_i64(got[1], ehi, what + " hi")
    Q.same_i64(got[2], en, what + " n")
    if quantiles is not None:
        exp = C.oracle_answers(oracles, range(len(oracles)), list(quantiles), single)
        assert tuple(got[3].shape) == (len(oracles), len(quantiles)), what
        U.assert_same_quantiles(got[3].cpu().numpy(), exp, what + " fused quantiles", None)
        live = set(range(len(oracles)))  # (quantiles() flushes every stream)
    C.assert_all(ss, oracles, what, before, live)
    if twin is not None:
        exp = twin_step(twin, ti, tx, quantiles, single)
        for g, e, name in zip(got, exp, ("lo", "hi", "n", "q")):
            assert _bytes(g) == _bytes(e), "%s: %s differs from the two calls" % (what, name)
        R.assert_sets_equal(ss, twin, what + ": fused vs ranks_keyed + ingest_keyed")
        if not ss.is_cpu:
            assert ss.num_promoted == twin.num_promoted, what
    return got


# ----------------------------------------- case 1: chunk and run boundaries
def case_boundaries(dev, setenv):
    """rankkeyed_cases.boundary_batch (runs of 0, 1, 63, 64, 65, 129, 200 samples,
    shuffled) at 64 samples per wave and at the default chunk: the values land
    at their own grouped positions, in arrival order."""
    ids, xs = Q.boundary_batch()
    sets = []
    for chunk, what in (("64", "chunk 64"), (None, "default chunk")):
        setenv("GK_RANKK_CHUNK", chunk)
        ss, orc, _ = K.make_set1(dev)
        twin, _, _ = K.make_set1(dev)
        sets.append((ss, fused(ss, twin, orc, ids, xs, what)))
    setenv("GK_RANKK_CHUNK", None)
    (a, ga), (b, gb) = sets
    for x, y, name in zip(ga, gb, ("lo", "hi", "n")):
        assert _bytes(x) == _bytes(y), name
    R.assert_sets_equal(a, b, "chunk 64 vs default chunk")


# ------------------------------------------------------ case 2: repeated calls
def case_repeated(dev):
    ss, orc = C.make(dev, C.MIXED)
    twin, _ = C.make(dev, C.MIXED)
    P = ss.flush_period
    rng = np.random.default_rng(61)
    ids = [C.MIXED_IDS[k] for k in rng.integers(0, len(C.MIXED_IDS), 120)]
    xs = [float(x) for x in rng.lognormal(0.0, 1.0, len(ids))]
    runs = {s: ids.count(s) for s in set(ids)}
    n1 = fused(ss, twin, orc, ids, xs, "first call")[2].cpu().numpy()
    n2 = fused(ss, twin, orc, ids, xs, "the same batch again")[2].cpu().numpy()
    # the second call's ranks see the first call's values
    assert np.array_equal(n2, n1 + np.asarray([runs[s] for s in ids], dtype=np.int64))
    crossed = exact = 0
    uniq = sorted(set(C.MIXED_IDS))
    for batch in range(4):
        ids = [uniq[k] for k in rng.integers(0, len(uniq), 300)]
        # stream 1's run is topped up so that its count ends on a period boundary
        n_end = orc[1].n + ids.count(1)
        ids += [1] * ((-n_end) % P or P)
        xs = [float(x) for x in rng.lognormal(0.0, 1.0, len(ids))]
        order = rng.permutation(len(ids))
        ids, xs = [ids[k] for k in order], [xs[k] for k in order]
        for s in set(ids):
            run, room = ids.count(s), P - orc[s].n % P
            crossed += room < run       # a flush point strictly inside the run
            exact += room == run        # the period boundary at the end of the run
        fused(ss, twin, orc, ids, xs, "batch %d" % batch)
        assert orc[1].n % P == 0 and not orc[1].pending
    assert crossed >= 4 and exact >= 4, (crossed, exact)


# ------------------------------------------------------ case 3: special values
def case_special(dev):
    ss, orc = C.make(dev, C.MIXED)
    twin, _ = C.make(dev, C.MIXED)
    ids = [10, -1, 3, -7, 11, I32_MIN, 3, 0, -1, 8]
    xs = [3900.0, NAN, 0.5, NAN, 1.0, NAN, 0.25, 1.0, 2.0, 0.5]
    lo, hi, n = fused(ss, twin, orc, ids, xs, "negative ids among live ones")
    neg = [k for k, s in enumerate(ids) if s < 0]
    assert not lo.cpu().numpy()[neg].any() and not hi.cpu().numpy()[neg].any() and not n.cpu().numpy()[neg].any()
    # all negative: zero rows, nothing ingested, every stream as before
    before = R.snapshot(ss)
    ids = [-1, -7, I32_MIN] * 30
    lo, hi, n = fused(ss, twin, orc, ids, [NAN] * len(ids), "all negative", before)
    assert not lo.any() and not hi.any() and not n.any()
    st = R.snapshot(ss)
    for s in range(len(orc)):
        R.assert_stream(R.stream_of_snapshot(st, s), R.stream_of_snapshot(before, s), "all negative: stream %d" % s)
    # count == 0 (with and without a query) and count == 1
    got = ss.rank_ingest_keyed(C.i32([]), torch.zeros(0, dtype=torch.float64), n=True)
    for t in got:
        assert tuple(t.shape) == (0,) and t.dtype == torch.int64
    assert tuple(ss.score_ingest_keyed(torch.zeros(0, dtype=torch.int64), []).shape) == (0,)
    st = R.snapshot(ss)
    for s in range(len(orc)):
        R.assert_stream(R.stream_of_snapshot(st, s), R.stream_of_snapshot(before, s), "count == 0: stream %d" % s)
    fused(ss, twin, orc, [], [], "count == 0 with a query", quantiles=Q3)
    fused(ss, twin, orc, [12], [1.0], "one sample")
    fused(ss, twin, orc, [-1], [NAN], "one negative sample")
    # all three rank outputs left out: ingest_keyed
    ids, xs = [11, 3, -1, 10, 3, 8, 12, 5], [0.5, 1.0, NAN, 2.0, 0.25, 0.5, 1.5, 3.0]
    ti, tx = Q.tensors(ss, ids, xs)
    assert ss.rank_ingest_keyed(ti, tx, lo=False, hi=False, n=False) == (None, None, None)
    twin.ingest_keyed(ti, tx)
    for s, x in zip(ids, xs):
        if s >= 0:
            orc[s].add(x)
    C.assert_all(ss, orc, "no rank output")
    R.assert_sets_equal(ss, twin, "no rank output vs ingest_keyed")
    got = ss.rank_ingest_keyed(ti, tx, lo=False, hi=False, n=False, quantiles=Q3)
    assert got[:3] == (None, None, None)
    assert _bytes(got[3]) == _bytes(twin.ingest_keyed(ti, tx, quantiles=Q3))
    R.assert_sets_equal(ss, twin, "no rank output, fused quantiles vs ingest_keyed")
    # signed zeros, infinities, denormals: bit for bit into the pending lists
    # (streams 0 and 15 are empty; each infinity comes last in its stream, so
    # that neither _sum nor _avg meets inf - inf)
    ss, orc = C.make(dev, C.MIXED)
    twin, _ = C.make(dev, C.MIXED)
    tiny = 5e-324
    ids = [0, 15, 0, 0, 15, 0, 0, 15]
    xs = [-0.0, -tiny, 0.0, tiny, -2.2250738585072009e-308, 2.2250738585072009e-308, INF, -INF]
    fused(ss, twin, orc, ids, xs, "special values")
    poffs, pv = ss.pending()
    poffs, pv = poffs.cpu().numpy(), pv.cpu().numpy()
    for s in (0, 15):
        mine = np.asarray([x for k, x in zip(ids, xs) if k == s], dtype=np.float64)
        assert pv[poffs[s]:poffs[s + 1]].tobytes() == mine.tobytes(), s


# ------------------------------------------------------- case 4: radix passes
def case_radix(dev, S):
    """S = 1, 257, 65537: one, two and three passes of the ONE group-by; about
    300 samples, the first and the last stream among them."""
    rng = np.random.default_rng(S)
    fed = sorted({0, S - 1} | {int(s) for s in rng.integers(0, S, 5)})
    ss, twin = U._ss(S, EPS, dev), U._ss(S, EPS, dev)
    orc = {s: OracleGK(EPS) for s in fed}
    fid, fval = [], []
    for k, s in enumerate(fed):
        x = R.seq(k % 6, 120 + 37 * k, 500 + k)
        orc[s].add_many(x)
        fid += [s] * len(x)
        fval += list(x)
    for x in (ss, twin):
        x.ingest_keyed(torch.tensor(fid, dtype=torch.int32), torch.tensor(fval, dtype=torch.float64))
    pool = fed + [int(s) for s in rng.integers(0, S, 6)]  # (unfed streams: empty before the call)
    ids = [pool[k] for k in rng.integers(0, len(pool), 300)] + [0, S - 1, -1]
    xs = [float(x) for x in rng.choice(np.asarray(fval), len(ids))]
    for s in set(ids) - {-1}:
        orc.setdefault(s, OracleGK(EPS))
    elo, ehi, en = oracle_step(orc, ids, xs)
    ti, tx = Q.tensors(ss, ids, xs)
    got = ss.rank_ingest_keyed(ti, tx, n=True)
    for g, e, name in zip(got, (elo, ehi, en), ("lo", "hi", "n")):
        Q.same_i64(g, e, "S = %d %s" % (S, name))
    st = R.snapshot(ss)
    for s, o in orc.items():
        R.assert_stream(R.stream_of_snapshot(st, s), R.stream_of_oracle(o), "S = %d stream %d" % (S, s))
    assert int(np.asarray(st["n"]).sum()) == sum(o.n for o in orc.values())
    exp = twin_step(twin, ti, tx)
    for g, e, name in zip(got, exp, ("lo", "hi", "n")):
        assert _bytes(g) == _bytes(e), "S = %d: %s differs from the two calls" % (S, name)
    tw = R.snapshot(twin)
    for k in st:  # (every array of the state, all S streams at once)
        assert np.asarray(st[k]).tobytes() == np.asarray(tw[k]).tobytes(), "S = %d: %s vs the two calls" % (S, k)
    if S <= 257:
        R.assert_sets_equal(ss, twin, "S = %d: fused vs the two calls" % S)


# -------------------------------- case 5: long tables and promoted streams
def case_long_table(dev):
    """rankkeyed_cases.case_long_table's 2079-entry table (beyond every LDS
    tile) and its 70 samples, which then join the stream."""
    eps = 0.001
    specs = [("D", 4000, 0), (1, 150, 981)]
    ss, orc = C.make(dev, specs, eps=eps)
    twin, _ = C.make(dev, specs, eps=eps)
    probe = C.oracle_of(eps, ("D", 4000, 0))
    probe.size()
    assert len(probe.v) == 2079
    xs = [float(x) for x in np.linspace(probe.min - 3.0, probe.max + 3.0, 50)]
    xs += [probe.v[k] for k in (0, 63, 64, 127, 128, 255, 256, 257, 511, 512, 1023, 1024, 2047, 2048, 2077, 2078)]
    xs += [np.nextafter(probe.v[256], -np.inf), (probe.v[255] + probe.v[256]) / 2, probe.min, probe.max]
    assert len(xs) == 70
    ids = [0] * 70 + [1, 1, 1]
    _, _, n = fused(ss, twin, orc, ids, xs + [0.5, 1.0, 50.0], "long table")
    assert int(n[0]) == 4000 and orc[0].n == 4070


def case_promoted(dev):
    """(GK_CAPS=128,256,512,4096 set by the caller) D(750) climbs from the 256
    class to 512 in the rank half's flush; stream 1 (150 lognormal values, a
    table below 128 entries) gets 260 new minima in descending order and leaves
    the 128 class in the ingest half."""
    ss, orc = C.make(dev, C.PROMOTED)
    twin, _ = C.make(dev, C.PROMOTED)
    if dev != "cpu":
        assert ss.capacity(0) == 128 and ss.capacity(1) == 256 and ss.capacity(2) == 512
    assert C.sizes(ss, 0) == (227, 43)
    _, xs = Q.probe_thresholds(C.PROMOTED)
    rng = np.random.default_rng(67)
    ids = [[2, 0, 4, 0][k] for k in rng.integers(0, 4, 240)] + [1] * 260
    vals = [xs[k] for k in rng.integers(0, len(xs), 240)] + [0.0] * 260
    order = rng.permutation(len(ids))
    ids, vals = [ids[k] for k in order], [vals[k] for k in order]
    down = iter(-1.0 - j for j in range(260))
    vals = [next(down) if s == 1 else x for s, x in zip(ids, vals)]
    promoted = 0 if dev == "cpu" else ss.num_promoted
    probe = [C.oracle_of(EPS, sp) for sp in C.PROMOTED[:2]]
    K.flush_covered(probe, range(2))
    assert len(probe[0].v) == 270 and len(probe[1].v) < 128  # (what the rank half's flush leaves)
    fused(ss, twin, orc, ids, vals, "promoted")
    assert len(orc[1].v) > 128
    if dev != "cpu":
        assert ss.num_promoted >= promoted + 1  # (stream 1 left class 0; stream 0 was promoted before)


# ----------------------------------------------------- case 6: fused quantiles
def case_quantiles(dev, run):
    qs, single = {"sorted": (Q3, False), "unsorted": ([0.9, 0.5, 0.99], False), "single": (Q3, True)}[run]
    ss, orc = C.make(dev, C.MIXED)
    twin, _ = C.make(dev, C.MIXED)
    rng = np.random.default_rng(71)
    ids = [C.MIXED_IDS[k] for k in rng.integers(0, len(C.MIXED_IDS), 300)] + [-1]
    xs = [float(x) for x in rng.lognormal(0.0, 1.0, 300)] + [NAN]
    fused(ss, twin, orc, ids, xs, "fused quantiles, " + run, quantiles=qs, single=single)


# ---------------------------------------------------- case 7: deferral (GPU only)
DEFER_SPECS = [("D", 600 + 75 * k, 0) if k % 4 else (k % 8, 150 + 50 * k, 960 + k) for k in range(14)]
DEFER_IDS = [13, 1, 4, 2, 9, 1, -1, 13]
DEFER_XS = [0.5, 3000.5, 1.0, 3500.0, 3999.0, -1.0, NAN, 5000.0]


def _defer_batch(dev):
    flat, offs = U.csr([C.seq(sp) for sp in DEFER_SPECS])
    sid = np.repeat(np.arange(len(DEFER_SPECS), dtype=np.int32), np.diff(offs))
    return torch.from_numpy(sid).to(dev), torch.from_numpy(flat).to(dev)


def case_deferred_before(dev):
    """(GK_POOL_SLOTS=2 set by the caller) (a): a keyed ingest left in flight
    defers most of its overflowing streams; the fused call settles it first."""
    ti, tv = _defer_batch(dev)
    ss, twin = U._ss(len(DEFER_SPECS), EPS, dev), U._ss(len(DEFER_SPECS), EPS, dev)
    for x in (ss, twin):
        x.ingest_keyed(ti, tv, sync=False)
    orc = [C.oracle_of(EPS, sp) for sp in DEFER_SPECS]
    fused(ss, twin, orc, DEFER_IDS, DEFER_XS, "deferred before", before=None)
    assert ss.num_promoted > 2


def case_deferred_own(dev, then):
    """(GK_POOL_SLOTS=2) (b): the fused call's own ingest defers streams and is
    left in flight; the next call -- ranks_keyed, or ingest_keyed -- settles it
    first: the re-run reads the set-owned grouped values that call is about to
    overwrite."""
    ti, tv = _defer_batch(dev)
    ss = U._ss(len(DEFER_SPECS), EPS, dev)
    orc = [OracleGK(EPS) for _ in DEFER_SPECS]
    ids, xs = ti.cpu().tolist(), tv.cpu().tolist()
    # (the streams interleaved, each keeping its own order -- the descending runs
    # are what makes the tables grow: the grouped order is not the arrival order)
    runs = {s: iter([x for k, x in zip(ids, xs) if k == s]) for s in set(ids)}
    ids = [ids[k] for k in np.random.default_rng(73).permutation(len(ids))]
    xs = [next(runs[s]) for s in ids]
    exp = oracle_step(orc, ids, xs)
    si, sx = Q.tensors(ss, ids, xs)
    got = ss.rank_ingest_keyed(si, sx, n=True, sync=False)
    if then == "ranks_keyed":
        Q.check_keyed(ss, orc, DEFER_IDS, DEFER_XS, "ranks_keyed after a deferring fused call", before=None)
    else:
        ui, ux = Q.tensors(ss, DEFER_IDS, [0.0 if x != x else x for x in DEFER_XS])
        ss.ingest_keyed(ui, ux)
        for s, x in zip(DEFER_IDS, ux.cpu().tolist()):
            if s >= 0:
                orc[s].add(x)
        C.assert_all(ss, orc, "ingest_keyed after a deferring fused call")
    for g, e, name in zip(got, exp, ("lo", "hi", "n")):
        Q.same_i64(g, e, "deferring fused call " + name)
        assert not e.any()  # (every stream was empty)
    assert ss.num_promoted > 2  # more streams than the 2 slots a class started with: some were deferred


# ---------------------------------------------------- case 8: overflow (GPU only)
def case_overflow(dev):
    """(GK_CAPS=128,256 set by the caller) the rank half's flush of D(750) needs
    270 entries and the last class holds 255: GK_E_OVERFLOW, the outputs
    untouched, nothing of the batch ingested."""
    from gkarray_amd._lib import GK_E_OVERFLOW, GKBackendError
    specs = [(1, 150, 951), ("D", 750, 0), (1, 150, 952), (2, 50, 953)]
    ss, orc = C.make(dev, specs)
    assert ss.capacity(1) == 256 and ss.capacity(2) == -1
    assert C.sizes(ss, 1) == (227, 43)
    ids, xs = [1, 0, -1, 1, 0], [3500.0, 1.0, NAN, 0.5, 0.5]
    ti, tx = Q.tensors(ss, ids, xs)
    out = [torch.full((len(ids),), -7, dtype=torch.int64, device=ss.device) for _ in range(3)]
    before = R.snapshot(ss)
    with pytest.raises(GKBackendError) as ei:
        ss.rank_ingest_keyed(ti, tx, lo=out[0], hi=out[1], n=out[2], quantiles=Q3)
    assert ei.value.code == GK_E_OVERFLOW, ei.value
    for t in out:
        assert bool((t == -7).all())
    assert orc[0].pending
    orc[0].size()  # (the other occurring stream has been flushed)
    st = C.assert_all(ss, orc, "after GK_E_OVERFLOW", before, {0, 1})
    assert [int(x) for x in st["n"]] == [int(x) for x in before["n"]]  # nothing ingested
    assert C.sizes(ss, 1) == (227, 43)
    twin, _ = C.make(dev, specs)
    twin.flush_select(C.i32([0]))
    fused(ss, twin, orc, [3, 0, 2, 3, -1], [0.5, 1.0, 2.0, 3.0, NAN], "valid call after GK_E_OVERFLOW")


# ---------------------------------------------------------- case 9: refusals
def case_refusals(dev, setenv):
    from gkarray_amd._lib import GK_E_ARG, GK_Q_LIST, GKBackendError
    ss, orc = C.make(dev, C.MIXED)
    twin, _ = C.make(dev, C.MIXED)
    S = len(C.MIXED)
    ids = [11, 3, -1, 10, 3, 8, 12, 5]
    xs = [0.5, 1.0, NAN, 2.0, 0.25, 0.5, 1.5, 3.0]
    N = len(ids)
    out = [torch.full((N,), -7, dtype=torch.int64, device=ss.device) for _ in range(3)]
    qout = torch.full((S, 3), -7.0, dtype=torch.float64, device=ss.device)
    st0 = R.snapshot(ss)

    def untouched(what):
        st1 = R.snapshot(ss)
        for s in range(S):
            R.assert_stream(R.stream_of_snapshot(st1, s), R.stream_of_snapshot(st0, s),
                            "after '%s': stream %d" % (what, s))
        for t in out:
            assert bool((t == -7).all()), what
        assert bool((qout == -7.0).all()), what

    def refused(what, ids, xs, text, absent=None, quantiles=None):
        ti, tx = Q.tensors(ss, ids, xs)
        with pytest.raises(GKBackendError) as ei:
            ss.rank_ingest_keyed(ti, tx, lo=out[0], hi=out[1], n=out[2], quantiles=quantiles)
        assert ei.value.code == GK_E_ARG, (what, ei.value)
        assert text in str(ei.value), (what, ei.value)
        assert absent is None or absent not in str(ei.value), (what, ei.value)
        untouched(what)

    def put(seq, k, v):
        seq = list(seq)
        seq[k] = v
        return seq

    refused("id == S", put(ids, 3, S), xs, "ids[3] = %d" % S)
    refused("NaN on a live row", ids, put(xs, 6, NAN), "xs[6]")
    assert "NaN" in ss._lib.gk_last_error().decode()
    refused("NaN first, id later", put(ids, 7, S + 9), put(xs, 4, NAN), "xs[4]")
    refused("id first, NaN later", put(ids, 1, S), put(xs, 4, NAN), "ids[1] = %d" % S)
    refused("both at one index", put(ids, 5, S), put(xs, 5, NAN), "ids[5] = %d" % S, absent="xs[")
    refused("a NaN in qs", ids, xs, "NaN", quantiles=[0.5, NAN, 0.9])
    # count < 0, NULL arrays and a NULL `out` have no Python spelling: the C call itself
    ti, tx = Q.tensors(ss, ids, xs)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    o = [p(t) for t in out]
    q3 = (ctypes.c_double * 3)(*Q3)
    qbad = (ctypes.c_double * 3)(0.5, NAN, 0.9)

    def call(pi, px, count, qs=None, nq=0, qo=None, mode=GK_Q_LIST):
        return ss._lib.gk_rank_ingest_keyed(ss.handle, pi, px, count, o[0], o[1], o[2], qs, nq, qo, mode, ss._sp())

    assert call(p(ti), p(tx), -1) == GK_E_ARG
    assert call(p(ti), p(tx), 2 ** 31) == GK_E_ARG
    assert call(None, p(tx), N) == GK_E_ARG
    assert call(p(ti), None, N) == GK_E_ARG
    assert call(p(ti), p(tx), N, q3, 3, None) == GK_E_ARG       # nq > 0 with out NULL
    assert call(p(ti), p(tx), N, None, 3, p(qout)) == GK_E_ARG  # nq > 0 with qs NULL
    assert call(p(ti), p(tx), N, qbad, 3, p(qout)) == GK_E_ARG
    assert call(p(ti), p(tx), N, q3, -1, p(qout)) == GK_E_ARG
    assert call(p(ti), p(tx), N, q3, 3, p(qout), 7) == GK_E_ARG  # bad mode
    assert call(None, None, 0, qbad, 3, p(qout)) == GK_E_ARG     # (the checks run at count == 0 too)
    untouched("count < 0 / NULL arrays / bad query arguments")
    with pytest.raises(ValueError):
        ss.rank_ingest_keyed(ti, tx[:-1])
    with pytest.raises(ValueError):
        ss.rank_ingest_keyed(ti, tx, lo=torch.zeros(N + 1, dtype=torch.int64, device=ss.device))
    with pytest.raises(ValueError):
        ss.rank_ingest_keyed(torch.tensor([1.0, 2.0]), tx[:2])
    untouched("Python argument errors")
    if dev != "cpu":  # (the chunk is the device kernel's)
        for bad in ("65", "0", "32", "x"):
            setenv("GK_RANKK_CHUNK", bad)
            refused("GK_RANKK_CHUNK=" + bad, ids, xs, "GK_RANKK_CHUNK")
        setenv("GK_RANKK_CHUNK", None)
    # the empty call touches nothing; then a valid call
    assert call(None, None, 0) == 0
    ss.sync()
    untouched("count == 0")
    C.assert_all(ss, orc, "after the refused calls")
    fused(ss, twin, orc, ids, xs, "valid call after the refusals", quantiles=Q3)


# ------------------------------------------------------ case 10: Python layer
def case_python(dev):
    from gkarray_amd import KeyedStreamSet
    from gkarray_amd._lib import GK_E_OVERFLOW, GKBackendError
    from gkarray_amd.keydir import NO_KEY
    ss, orc = C.make(dev, C.MIXED)
    ids = [10, 0, -1, 3, 9, 3, 15, 8]
    xs = [3900.0, 1.0, NAN, 0.5, 1.0, 0.25, 2.0, 0.5]
    ti, tx = Q.tensors(ss, ids, xs)
    lo, hi, n = oracle_step(orc, ids, xs)
    score = ss.score_ingest_keyed(ti.to(torch.int64), xs).cpu().numpy()
    assert score.dtype == np.float64 and score.shape == (len(ids),)
    for k in range(len(ids)):
        if n[k] == 0:
            assert np.isnan(score[k]), k
        else:
            assert score[k] == (lo[k] + hi[k]) / (2.0 * n[k]), k
    assert np.isnan(score[2]) and np.isnan(score[1]) and not np.isnan(score[0])
    C.assert_all(ss, orc, "score_ingest_keyed")
    score, q = ss.score_ingest_keyed(ti, tx, quantiles=Q3)
    assert tuple(score.shape) == (len(ids),) and tuple(q.shape) == (len(orc), 3)
    # KeyedStreamSet.score_add against the dict-of-oracles loop and a twin driven by score + add
    rng = np.random.default_rng(59)
    ks = KeyedStreamSet(EPS, capacity=8, device=dev)
    twin = KeyedStreamSet(EPS, capacity=8, device=dev)
    orc = {}
    for batch in range(4):
        N = 400
        keys = rng.integers(1000, 1000 + 6 + 3 * batch, N).astype(np.int64)
        keys[rng.random(N) < 0.05] = NO_KEY
        vals = rng.lognormal(0.0, 1.0, N)
        for k in {int(k) for k in keys} & set(orc):
            if orc[k].n > 0:
                orc[k].size()
        lo = np.zeros(N, np.int64)
        hi = np.zeros(N, np.int64)
        n = np.zeros(N, np.int64)
        for i, (k, x) in enumerate(zip(keys.tolist(), vals.tolist())):
            if k in orc:
                l, h = K.expected_ranks(orc[k], [x])
                lo[i], hi[i], n[i] = l[0], h[0], orc[k].n
        with np.errstate(invalid="ignore", divide="ignore"):
            exp = (lo + hi).astype(np.float64) / (2.0 * n.astype(np.float64))
        new = np.asarray([int(k) not in orc for k in keys])
        assert new.any() and (keys == NO_KEY).any()
        tk, tv = torch.from_numpy(keys), torch.from_numpy(vals)
        if batch % 2:
            got, q = ks.score_add(tk, tv, quantiles=Q3)
            assert tuple(q.shape) == (ks.directory.bound, 3)
        else:
            got = ks.score_add(tk, tv)
        got = got.cpu().numpy()
        assert np.array_equal(np.isnan(got), n == 0) and np.array_equal(got, exp, equal_nan=True), \
            "score_add, batch %d" % batch
        assert np.isnan(got[new]).all()  # (a key bound by this batch has no history yet)
        two = twin.score(tk, tv).cpu().numpy()
        tq = twin.add(tk, tv, quantiles=Q3 if batch % 2 else None)
        assert np.array_equal(got, two, equal_nan=True), "score_add vs score + add, batch %d" % batch
        if batch % 2:
            assert _bytes(q) == _bytes(tq)
        for k, x in zip(keys.tolist(), vals.tolist()):
            if k != NO_KEY:
                orc.setdefault(k, OracleGK(EPS)).add(x)
        if batch % 2:
            for o in orc.values():  # (the fused quantiles flushed every stream)
                if o.n > 0:
                    o.size()
    assert ks.keys().cpu().tolist() == twin.keys().cpu().tolist() and len(ks) == len(twin) == len(orc)
    R.assert_sets_equal(ks.streams, twin.streams, "score_add vs score + add")
    sid = ks.directory.lookup(torch.tensor(sorted(orc), dtype=torch.int64)).cpu().tolist()
    st = R.snapshot(ks.streams)
    for k, s in zip(sorted(orc), sid):
        R.assert_stream(R.stream_of_snapshot(st, s), R.stream_of_oracle(orc[k]), "key %d" % k)
    ks.close()
    twin.close()
    # the max_streams refusal leaves the object unchanged
    ks = KeyedStreamSet(EPS, capacity=4, device=dev, max_streams=6)
    ks.score_add(torch.tensor([1, 2, 3, 1]), torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64))
    keys0, st0 = ks.keys().cpu().tolist(), R.snapshot(ks.streams)
    with pytest.raises(GKBackendError) as ei:
        ks.score_add(torch.arange(1, 9), torch.ones(8, dtype=torch.float64))
    assert ei.value.code == GK_E_OVERFLOW
    assert ks.keys().cpu().tolist() == keys0 and ks.directory.capacity == 4 and ks.streams.num_streams == 4
    st1 = R.snapshot(ks.streams)
    for s in range(4):
        R.assert_stream(R.stream_of_snapshot(st1, s), R.stream_of_snapshot(st0, s), "max_streams refusal: stream %d" % s)
    got = ks.score_add(torch.tensor([1, 4, 5, 6]), torch.tensor([0.5, 1.0, 1.0, 1.0], dtype=torch.float64))
    assert len(ks) == 6 and not np.isnan(got.cpu().numpy()[0]) and np.isnan(got.cpu().numpy()[1:]).all()
    ks.close()


def case_symbols():
    from gkarray_amd import _lib
    assert "gk_rank_ingest_keyed" in _lib.SYMBOLS and "gk_rank_ingest_keyed" in _lib.CPU_SYMBOLS
    assert hasattr(_lib.load_cpu(), "gk_rank_ingest_keyed")
