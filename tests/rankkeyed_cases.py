"""Cases of the keyed rank queries (gk_ranks_keyed through StreamSet.ranks_keyed
/ cdf_keyed and KeyedStreamSet.ranks_keyed / score), shared by
tests/test_gpu_rank_keyed.py (device engine, k_rank_keyed) and
tests/test_cpu_rank_keyed.py (host engine); the engine is the ``dev``
parameter.

Row i of a call belongs to the sample (ids[i], xs[i]).  The expected pair is
``rank_cases.expected_ranks`` -- the contract of include/gk_capi.h, a plain
linear loop -- on the ``OracleGK`` of stream ids[i], flushed by
``rank_cases.flush_covered`` if it occurs in the batch; (0, 0) and n = 0 for a
negative id.  Answers are int64 and compared by bytes.  After every call every
stream of the set is compared bit for bit with its oracle
(``select_cases.assert_all``), streams that do not occur also with a snapshot
from before the call.  Test infrastructure only."""
import ctypes

import numpy as np
import pytest
import torch

import parity_util as U
import rank_cases as K
import rollup_cases as R
import select_cases as C
from gk_oracle import OracleGK

EPS = C.EPS
NAN = float("nan")
I32_MIN = -2 ** 31


def expected_rows(oracles, ids, xs):
    """(lo, hi, n) int64[len(ids)] from the (flushed) oracles; zeros for a negative id."""
    lo = np.zeros(len(ids), np.int64)
    hi = np.zeros(len(ids), np.int64)
    n = np.zeros(len(ids), np.int64)
    rows = {}
    for k, s in enumerate(ids):
        if s >= 0:
            rows.setdefault(s, []).append(k)
    for s, ks in rows.items():
        o = oracles[s]
        l, h = K.expected_ranks(o, [xs[k] for k in ks])
        lo[ks], hi[ks], n[ks] = l, h, o.n
    return lo, hi, n


def same_i64(got, exp, what):
    got = got.cpu().numpy()
    assert got.dtype == np.int64 and got.shape == exp.shape, (what, got.dtype, got.shape, exp.shape)
    if got.tobytes() != exp.tobytes():
        bad = np.flatnonzero(got != exp)
        raise AssertionError("%s: %d mismatches, first at row %d: %d vs %d"
                             % (what, len(bad), bad[0], got[bad[0]], exp[bad[0]]))


def tensors(ss, ids, xs):
    return (torch.tensor(list(ids), dtype=torch.int32, device=ss.device),
            torch.tensor(list(xs), dtype=torch.float64, device=ss.device))


def check_keyed(ss, oracles, ids, xs, what, before=True, check_state=True):
    """ranks_keyed(n=True) on the engine against expected_rows on the oracles,
    whose occurring streams are flushed first; then every stream's state.
    Returns the engine's three tensors."""
    live = {s for s in ids if s >= 0}
    if before is True:
        before = R.snapshot(ss)
    K.flush_covered(oracles, live)
    elo, ehi, en = expected_rows(oracles, ids, xs)
    ti, tx = tensors(ss, ids, xs)
    glo, ghi, gn = ss.ranks_keyed(ti, tx, n=True)
    same_i64(glo, elo, what + " lo")
    same_i64(ghi, ehi, what + " hi")
    same_i64(gn, en, what + " n")
    if check_state:
        C.assert_all(ss, oracles, what, before, live)
    return glo, ghi, gn


def probe_thresholds(specs, eps=EPS):
    probe = [C.oracle_of(eps, sp) for sp in specs]
    K.flush_covered(probe, range(len(probe)))
    return probe, K.thresholds(probe)


# ----------------------------------------- case 1: chunk and run boundaries
# samples per stream of rank_cases.SET1, in stream order = grouped order; the
# run of stream s starts at sum(COUNTS[:s]) (a 64-sample chunk: GK_RANKK_CHUNK=64)
COUNTS = [64, 64, 1, 1, 1, 1, 1, 1, 1, 1, 200, 0, 65, 63, 129, 0, 1, 63, 65, 129, 200, 64, 200, 129]


def _chunk_layout(counts, chunk=64):
    starts = np.concatenate([[0], np.cumsum(counts)])
    on_boundary = straddles = three = 0
    for s, c in enumerate(counts):
        a, b = int(starts[s]), int(starts[s + 1])
        if c and a and a % chunk == 0:
            on_boundary += 1
        if c and a % chunk and a // chunk != (b - 1) // chunk:
            straddles += 1
        if c and (b - 1) // chunk - a // chunk >= 2:
            three += 1
    per_chunk = np.bincount([int(starts[s]) // chunk for s, c in enumerate(counts) if c])
    return on_boundary, straddles, three, int(per_chunk.max())


def boundary_batch():
    assert len(COUNTS) == len(K.SET1) and set(COUNTS) == {0, 1, 63, 64, 65, 129, 200}
    on_boundary, straddles, three, crowd = _chunk_layout(COUNTS)
    assert on_boundary >= 1 and straddles >= 3 and three >= 3 and crowd >= 8
    _, xs = probe_thresholds(K.SET1)
    ids, vals = [], []
    for s, c in enumerate(COUNTS):
        ids += [s] * c
        vals += [xs[(7 * j + s) % len(xs)] for j in range(c)]
    order = np.random.default_rng(41).permutation(len(ids))
    return [ids[k] for k in order], [vals[k] for k in order]


def case_boundaries(dev, setenv):
    """The same shuffled batch at 64 samples per wave and at the default chunk."""
    ids, xs = boundary_batch()
    setenv("GK_RANKK_CHUNK", "64")
    a, a_o, _ = K.make_set1(dev)
    got64 = check_keyed(a, a_o, ids, xs, "chunk 64")
    setenv("GK_RANKK_CHUNK", None)
    b, b_o, _ = K.make_set1(dev)
    got = check_keyed(b, b_o, ids, xs, "default chunk")
    for x, y, name in zip(got64, got, ("lo", "hi", "n")):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), name
    R.assert_sets_equal(a, b, "chunk 64 vs default chunk")


# --------------------------------------------------------- case 2: thresholds
def case_thresholds(dev):
    """Every stream of SET1 against every threshold of rank_cases.thresholds
    (+-inf, signed zeros, every stream's min, max, entries, midpoints, below
    every min, above every max), some twice, shuffled."""
    ss, orc, xs = K.make_set1(dev)
    ids, vals = [], []
    for s in range(len(K.SET1)):
        mine = xs + xs[s % 5::9]  # (repeats)
        ids += [s] * len(mine)
        vals += mine
    order = np.random.default_rng(43).permutation(len(ids))
    check_keyed(ss, orc, [ids[k] for k in order], [vals[k] for k in order], "thresholds")


# -------------------------------------------------------- case 3: equivalence
def case_equivalence(dev):
    a, orc = C.make(dev, C.MIXED)
    b, _ = C.make(dev, C.MIXED)
    c, _ = C.make(dev, C.MIXED)
    _, allx = probe_thresholds(C.MIXED)
    allx = allx[:40]
    rng = np.random.default_rng(47)
    uniq = sorted(set(C.MIXED_IDS))
    rows = rng.integers(0, len(uniq), 500)
    cols = rng.integers(0, len(allx), 500)
    ids = [uniq[r] for r in rows]
    xs = [allx[k] for k in cols]
    ti, tx = tensors(a, ids, xs)
    lo, hi, _ = a.ranks_keyed(ti, tx)
    slo, shi = b.ranks_select(C.i32(uniq), allx)
    same_i64(lo, slo.cpu().numpy()[rows, cols], "ranks_keyed vs ranks_select, lo")
    same_i64(hi, shi.cpu().numpy()[rows, cols], "ranks_keyed vs ranks_select, hi")
    c.flush_select(C.i32(uniq))
    R.assert_sets_equal(a, c, "ranks_keyed vs flush_select")
    R.assert_sets_equal(a, b, "ranks_keyed vs ranks_select")
    st1 = R.snapshot(a)
    lo2, hi2, _ = a.ranks_keyed(ti, tx)
    same_i64(lo2, lo.cpu().numpy(), "second call, lo")
    same_i64(hi2, hi.cpu().numpy(), "second call, hi")
    st2 = R.snapshot(a)
    for s in range(a.num_streams):
        R.assert_stream(R.stream_of_snapshot(st2, s), R.stream_of_snapshot(st1, s), "second call, stream %d" % s)
    K.flush_covered(orc, uniq)
    C.assert_all(a, orc, "after two calls")


# ------------------------------------------------------- case 4: negative ids
def case_negative(dev):
    ss, orc = C.make(dev, C.MIXED)
    ids = [10, -1, 3, -7, 11, I32_MIN, 3, 0, -1, 8]
    xs = [3900.0, NAN, 0.5, NAN, 1.0, NAN, 0.25, 1.0, 2.0, 0.5]
    lo, hi, n = check_keyed(ss, orc, ids, xs, "negative ids among live ones")
    neg = [k for k, s in enumerate(ids) if s < 0]
    assert not lo.cpu().numpy()[neg].any() and not hi.cpu().numpy()[neg].any() and not n.cpu().numpy()[neg].any()
    # all negative: no stream is touched (12 still holds its pending values)
    before = R.snapshot(ss)
    ids = [-1, -7, I32_MIN] * 30
    lo, hi, n = check_keyed(ss, orc, ids, [NAN] * len(ids), "all negative", before)
    assert not lo.any() and not hi.any() and not n.any()
    assert C.sizes(ss, 12) == (51, 49)
    st = R.snapshot(ss)
    for s in range(len(orc)):
        R.assert_stream(R.stream_of_snapshot(st, s), R.stream_of_snapshot(before, s), "all negative: stream %d" % s)
    # count == 0 and count == 1
    for t in ss.ranks_keyed(C.i32([]), torch.zeros(0, dtype=torch.float64), n=True):
        assert tuple(t.shape) == (0,) and t.dtype == torch.int64
    assert tuple(ss.cdf_keyed(torch.zeros(0, dtype=torch.int64), []).shape) == (0,)
    check_keyed(ss, orc, [12], [1.0], "one sample")
    assert C.sizes(ss, 12)[1] == 0
    check_keyed(ss, orc, [-1], [NAN], "one negative sample")


# ------------------------------------- case 5: radix passes, index payloads
def case_radix(dev, S):
    """S = 1, 257, 65537: one, two and three passes of the group-by; a few
    hundred samples, the first and the last stream among them."""
    rng = np.random.default_rng(S)
    fed = sorted({0, S - 1} | {int(s) for s in rng.integers(0, S, 5)})
    ss = U._ss(S, EPS, dev)
    orc = {s: OracleGK(EPS) for s in fed}
    fid, fval = [], []
    for k, s in enumerate(fed):
        x = R.seq(k % 6, 120 + 37 * k, 500 + k)
        orc[s].add_many(x)
        fid += [s] * len(x)
        fval += list(x)
    ss.ingest_keyed(torch.tensor(fid, dtype=torch.int32), torch.tensor(fval, dtype=torch.float64))
    pool = fed + [int(s) for s in rng.integers(0, S, 6)]  # (unfed streams answer as empty ones)
    ids = [pool[k] for k in rng.integers(0, len(pool), 300)] + [0, S - 1, -1]
    xs = [float(x) for x in rng.choice(np.asarray(fval), len(ids))]
    live = set(ids) - {-1}
    for s in live & set(fed):
        orc[s].size()
    lo = np.zeros(len(ids), np.int64)
    hi = np.zeros(len(ids), np.int64)
    n = np.zeros(len(ids), np.int64)
    for k, s in enumerate(ids):
        if s in orc:
            l, h = K.expected_ranks(orc[s], [xs[k]])
            lo[k], hi[k], n[k] = l[0], h[0], orc[s].n
    ti, tx = tensors(ss, ids, xs)
    glo, ghi, gn = ss.ranks_keyed(ti, tx, n=True)
    same_i64(glo, lo, "S = %d lo" % S)
    same_i64(ghi, hi, "S = %d hi" % S)
    same_i64(gn, n, "S = %d n" % S)
    st = R.snapshot(ss)
    for s in fed:
        R.assert_stream(R.stream_of_snapshot(st, s), R.stream_of_oracle(orc[s]), "S = %d stream %d" % (S, s))
    assert int(np.asarray(st["n"]).sum()) == sum(o.n for o in orc.values())


# -------------------------------- case 6: long tables and promoted streams
def case_long_table(dev):
    """rank_cases.case_long_table's 2079-entry table (beyond every LDS tile) gets
    70 samples: its range, both ends, entries at multiples of 64 and 256."""
    eps = 0.001
    ss, orc = C.make(dev, [("D", 4000, 0), (1, 150, 981)], eps=eps)
    probe = C.oracle_of(eps, ("D", 4000, 0))
    probe.size()
    assert len(probe.v) == 2079
    xs = [float(x) for x in np.linspace(probe.min - 3.0, probe.max + 3.0, 50)]
    xs += [probe.v[k] for k in (0, 63, 64, 127, 128, 255, 256, 257, 511, 512, 1023, 1024, 2047, 2048, 2077, 2078)]
    xs += [np.nextafter(probe.v[256], -np.inf), (probe.v[255] + probe.v[256]) / 2, probe.min, probe.max]
    assert len(xs) == 70
    ids = [0] * 70 + [1, 1, 1]
    check_keyed(ss, orc, ids, xs + [0.5, 1.0, 50.0], "long table")
    assert C.sizes(ss, 0) == (2079, 0)


def case_promoted(dev):
    """(GK_CAPS=128,256,512,4096 set by the caller) D(750) climbs from the 256
    class to 512 inside the call; D(1500) is answered where it stands."""
    ss, orc = C.make(dev, C.PROMOTED)
    if dev != "cpu":
        assert ss.capacity(1) == 256 and ss.capacity(2) == 512
    assert C.sizes(ss, 0) == (227, 43)
    _, xs = probe_thresholds(C.PROMOTED)
    rng = np.random.default_rng(53)
    ids = [[2, 0, 4, 0][k] for k in rng.integers(0, 4, 240)]
    check_keyed(ss, orc, ids, [xs[k] for k in rng.integers(0, len(xs), 240)], "promoted")
    assert C.sizes(ss, 0) == (270, 0)


# ---------------------------------------------------------- case 7: refusals
def case_refusals(dev, setenv):
    from gkarray_amd._lib import GK_E_ARG, GKBackendError
    ss, orc = C.make(dev, C.MIXED)
    S = len(C.MIXED)
    ids = [11, 3, -1, 10, 3, 8, 12, 5]
    xs = [0.5, 1.0, NAN, 2.0, 0.25, 0.5, 1.5, 3.0]
    N = len(ids)
    out = [torch.full((N,), -7, dtype=torch.int64, device=ss.device) for _ in range(3)]
    st0 = R.snapshot(ss)

    def untouched(what):
        st1 = R.snapshot(ss)
        for s in range(S):
            R.assert_stream(R.stream_of_snapshot(st1, s), R.stream_of_snapshot(st0, s),
                            "after '%s': stream %d" % (what, s))
        for t in out:
            assert bool((t == -7).all()), what

    def refused(what, ids, xs, text, absent=None):
        ti, tx = tensors(ss, ids, xs)
        with pytest.raises(GKBackendError) as ei:
            ss.ranks_keyed(ti, tx, lo=out[0], hi=out[1], n=out[2])
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
    ti, tx = tensors(ss, ids, xs)
    with pytest.raises(GKBackendError) as ei:
        ss.ranks_keyed(ti, tx, lo=False, hi=False, n=False)
    assert ei.value.code == GK_E_ARG
    untouched("all outputs NULL")
    # count < 0 and NULL arrays have no Python spelling: the C call itself
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    call = ss._lib.gk_ranks_keyed
    assert call(ss.handle, p(ti), p(tx), -1, p(out[0]), p(out[1]), p(out[2]), ss._sp()) == GK_E_ARG
    assert call(ss.handle, p(ti), p(tx), 2 ** 31, p(out[0]), p(out[1]), p(out[2]), ss._sp()) == GK_E_ARG
    assert call(ss.handle, None, p(tx), N, p(out[0]), p(out[1]), p(out[2]), ss._sp()) == GK_E_ARG
    assert call(ss.handle, p(ti), None, N, p(out[0]), p(out[1]), p(out[2]), ss._sp()) == GK_E_ARG
    assert call(ss.handle, p(ti), p(tx), N, None, None, None, ss._sp()) == GK_E_ARG
    assert call(ss.handle, None, None, 0, None, None, None, ss._sp()) == GK_E_ARG
    untouched("count < 0 / NULL arrays")
    with pytest.raises(ValueError):
        ss.ranks_keyed(ti, tx[:-1])
    with pytest.raises(ValueError):
        ss.ranks_keyed(ti, tx, lo=torch.zeros(N + 1, dtype=torch.int64, device=ss.device))
    with pytest.raises(ValueError):
        ss.ranks_keyed(torch.tensor([1.0, 2.0]), tx[:2])
    if dev != "cpu":  # (the chunk is the device kernel's)
        for bad in ("65", "0", "32", "x"):
            setenv("GK_RANKK_CHUNK", bad)
            with pytest.raises(GKBackendError) as ei:
                ss.ranks_keyed(ti, tx, lo=out[0], hi=out[1], n=out[2])
            assert ei.value.code == GK_E_ARG and "GK_RANKK_CHUNK" in str(ei.value), (bad, ei.value)
            untouched("GK_RANKK_CHUNK=" + bad)
        setenv("GK_RANKK_CHUNK", None)
    # the empty call touches nothing; then a valid call
    assert call(ss.handle, None, None, 0, p(out[0]), None, None, ss._sp()) == 0
    untouched("count == 0")
    C.assert_all(ss, orc, "after the refused calls")
    check_keyed(ss, orc, ids, xs, "valid call after the refusals")


# ------------------------------------- case 8: overflow and deferral (GPU only)
def case_overflow(dev):
    """(GK_CAPS=128,256 set by the caller) D(750)'s flush needs 270 entries and
    the last class holds 255: GK_E_OVERFLOW, the outputs untouched, D(750) keeps
    its 227 + 43 state, the other occurring stream has been flushed."""
    from gkarray_amd._lib import GK_E_OVERFLOW, GKBackendError
    specs = [(1, 150, 951), ("D", 750, 0), (1, 150, 952), (2, 50, 953)]
    ss, orc = C.make(dev, specs)
    assert ss.capacity(1) == 256 and ss.capacity(2) == -1
    assert C.sizes(ss, 1) == (227, 43)
    ids, xs = [1, 0, -1, 1, 0], [3500.0, 1.0, NAN, 0.5, 0.5]
    ti, tx = tensors(ss, ids, xs)
    out = [torch.full((len(ids),), -7, dtype=torch.int64, device=ss.device) for _ in range(3)]
    before = R.snapshot(ss)
    with pytest.raises(GKBackendError) as ei:
        ss.ranks_keyed(ti, tx, lo=out[0], hi=out[1], n=out[2])
    assert ei.value.code == GK_E_OVERFLOW, ei.value
    for t in out:
        assert bool((t == -7).all())
    assert orc[0].pending
    orc[0].size()
    C.assert_all(ss, orc, "after GK_E_OVERFLOW", before, {0, 1})
    assert C.sizes(ss, 1) == (227, 43)
    check_keyed(ss, orc, [3, 0, 2, 3, -1], [0.5, 1.0, 2.0, 3.0, NAN], "valid call after GK_E_OVERFLOW")


def case_deferred(dev):
    """(GK_POOL_SLOTS=2 set by the caller) a keyed ingest left in flight defers
    most of its overflowing streams -- it is re-run from the set's grouped
    buffers, the ones this call groups into -- before the ranks are read."""
    specs = [("D", 600 + 75 * k, 0) if k % 4 else (k % 8, 150 + 50 * k, 960 + k) for k in range(14)]
    ss = U._ss(len(specs), EPS, dev)
    flat, offs = U.csr([C.seq(sp) for sp in specs])
    sid = np.repeat(np.arange(len(specs), dtype=np.int32), np.diff(offs))
    ti, tv = torch.from_numpy(sid).to(dev), torch.from_numpy(flat).to(dev)
    ss.ingest_keyed(ti, tv, sync=False)
    orc = [C.oracle_of(EPS, sp) for sp in specs]
    ids = [13, 1, 4, 2, 9, 1, -1, 13]
    xs = [0.5, 3000.5, 1.0, 3500.0, 3999.0, -1.0, NAN, 5000.0]
    check_keyed(ss, orc, ids, xs, "deferred", before=None)
    assert ss.num_promoted > 2  # more streams than the 2 slots a class started with: some were deferred


# ------------------------------------------------------ case 9: Python layer
def case_python(dev):
    from gkarray_amd import KeyedStreamSet
    from gkarray_amd.keydir import NO_KEY
    ss, orc = C.make(dev, C.MIXED)
    ids = [10, 0, -1, 3, 9, 3, 15, 8]
    xs = [3900.0, 1.0, NAN, 0.5, 1.0, 0.25, 2.0, 0.5]
    ti, tx = tensors(ss, ids, xs)
    cdf = ss.cdf_keyed(ti.to(torch.int64), xs).cpu().numpy()
    lo, hi, n = check_keyed(ss, orc, ids, xs, "cdf_keyed")
    lo, hi, n = lo.cpu().numpy(), hi.cpu().numpy(), n.cpu().numpy()
    assert cdf.dtype == np.float64 and cdf.shape == (len(ids),)
    for k in range(len(ids)):
        if n[k] == 0:
            assert np.isnan(cdf[k]), k
        else:
            assert cdf[k] == (lo[k] + hi[k]) / (2.0 * n[k]), k
    assert np.isnan(cdf[2]) and np.isnan(cdf[1]) and not np.isnan(cdf[0])
    # KeyedStreamSet: score-then-add against the oracle loop
    rng = np.random.default_rng(59)
    ks = KeyedStreamSet(EPS, capacity=8, device=dev)
    orc = {}
    for batch in range(4):
        N = 400
        keys = rng.integers(1000, 1000 + 6 + 3 * batch, N).astype(np.int64)
        keys[rng.random(N) < 0.05] = NO_KEY
        vals = rng.lognormal(0.0, 1.0, N)
        known = {int(k) for k in keys} & set(orc)
        for k in known:
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
        size0 = len(ks.directory)
        if batch % 2:
            glo, ghi = ks.ranks_keyed(torch.from_numpy(keys), torch.from_numpy(vals))
            same_i64(glo, lo, "KeyedStreamSet.ranks_keyed lo, batch %d" % batch)
            same_i64(ghi, hi, "KeyedStreamSet.ranks_keyed hi, batch %d" % batch)
        got = ks.score(torch.from_numpy(keys), torch.from_numpy(vals)).cpu().numpy()
        assert np.array_equal(np.isnan(got), n == 0) and np.array_equal(got, exp, equal_nan=True), \
            "score, batch %d" % batch
        assert len(ks.directory) == size0  # (a query binds no key)
        unknown = np.asarray([int(k) not in orc for k in keys])
        assert unknown.any() and np.isnan(got[unknown]).all()
        ks.add(torch.from_numpy(keys), torch.from_numpy(vals))
        for k, x in zip(keys.tolist(), vals.tolist()):
            if k != NO_KEY:
                orc.setdefault(k, OracleGK(EPS)).add(x)
    ids = ks.directory.lookup(torch.tensor(sorted(orc), dtype=torch.int64)).cpu().tolist()
    st = R.snapshot(ks.streams)
    for k, s in zip(sorted(orc), ids):
        R.assert_stream(R.stream_of_snapshot(st, s), R.stream_of_oracle(orc[k]), "key %d" % k)
    ks.close()


def case_symbols():
    from gkarray_amd import _lib
    assert "gk_ranks_keyed" in _lib.SYMBOLS and "gk_ranks_keyed" in _lib.CPU_SYMBOLS
    assert hasattr(_lib.load_cpu(), "gk_ranks_keyed")
