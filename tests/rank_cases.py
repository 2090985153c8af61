"""Cases of the rank queries (gk_ranks / gk_ranks_select through
StreamSet.ranks / ranks_select / cdf / cdf_select and GKArray.rank / cdf),
shared by tests/test_gpu_rank.py (device engine, k_rank) and
tests/test_cpu_rank.py (host engine); the engine is the ``dev`` parameter.

The reference has no rank(): the expected pair is the contract of
include/gk_capi.h applied to the ORACLE's state (``OracleGK.v/g/d``, ``n``,
``min``, ``max``) by ``expected_ranks``, a plain linear loop.  Answers are
int64 and compared by bytes.  After every call every stream of the set is
compared bit for bit with its oracle, on which only the covered streams were
flushed (``o.size()``); unlisted streams also with a snapshot from before the
call (``select_cases.assert_all``).  Test infrastructure only."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import parity_util as U
import rollup_cases as R
import select_cases as C
from gk_oracle import OracleGK

EPS = C.EPS
INF = float("inf")


def expected_ranks(o, xs):
    """(lo, hi), int64 arrays of len(xs): the four rules on the oracle's table,
    which the caller has flushed (``o.size()``) if n > 0.  No bisection."""
    lo, hi = [], []
    E = len(o.v)
    for x in xs:
        if o.n == 0:
            l = h = 0
        elif x < o.min:
            l = h = 0
        elif x >= o.max:
            l = h = o.n
        else:
            i = 0
            for k in range(E):
                if o.v[k] <= x:
                    i += 1
            G = 0
            for k in range(i):
                G += o.g[k]
            l = max(G, 1)
            h = min(G + o.g[i] + o.d[i] - 1 if i < E else o.n, o.n - 1)
        lo.append(l)
        hi.append(h)
    return np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)


def flush_covered(oracles, ids):
    """The flush rule on the oracles: a covered stream with n > 0 runs size() (gk:45-46)."""
    for s in set(ids):
        if oracles[s].n > 0:
            oracles[s].size()


def expected_rows(oracles, ids, xs):
    rows = [expected_ranks(oracles[s], xs) for s in ids]
    lo = np.asarray([r[0] for r in rows], dtype=np.int64).reshape(len(ids), len(xs))
    hi = np.asarray([r[1] for r in rows], dtype=np.int64).reshape(len(ids), len(xs))
    return lo, hi


def same_i64(got, exp, what):
    got = got.cpu().numpy()
    assert got.dtype == np.int64 and got.shape == exp.shape, (what, got.dtype, got.shape, exp.shape)
    if got.tobytes() != exp.tobytes():
        bad = np.argwhere(got != exp)
        r, c = bad[0]
        raise AssertionError("%s: %d mismatches, first at row %d x %d: %d vs %d"
                             % (what, len(bad), r, c, got[r, c], exp[r, c]))


def check_ranks(ss, oracles, ids, xs, what, lo=True, hi=True, before=True):
    """ranks (ids None) / ranks_select on the engine against expected_ranks on
    the covered oracles; then every stream's state.  Returns the engine's pair.
    `before` as in select_cases.check_query."""
    covered = list(range(len(oracles))) if ids is None else list(ids)
    if before is True:
        before = R.snapshot(ss)
    flush_covered(oracles, covered)
    elo, ehi = expected_rows(oracles, covered, xs)
    if ids is None:
        glo, ghi = ss.ranks(xs, lo=lo, hi=hi)
    else:
        glo, ghi = ss.ranks_select(C.i32(ids), xs, lo=lo, hi=hi)
    assert (glo is None) == (not lo) and (ghi is None) == (not hi), what
    if lo:
        same_i64(glo, elo, what + " lo")
    if hi:
        same_i64(ghi, ehi, what + " hi")
    C.assert_all(ss, oracles, what, before, set(covered))
    return glo, ghi


def _bits(x):
    return struct.pack("<d", float(x))


def thresholds(oracles, seed=5):
    """+-inf, -0.0, 0.0, every (flushed) stream's min, max, v[0], v[E//2],
    v[E-1] and a midpoint of two adjacent entries, one value below every min and
    one above every max; distinct bit patterns, shuffled with a fixed seed."""
    xs = [INF, -INF, -0.0, 0.0]
    live = [o for o in oracles if o.n > 0]
    for o in live:
        E = len(o.v)
        xs += [o.min, o.max, o.v[0], o.v[E // 2], o.v[E - 1]]
        if E >= 2:
            k = E // 3
            xs.append((o.v[k] + o.v[k + 1]) / 2.0)
    xs += [min(o.min for o in live) - 1.0, max(o.max for o in live) + 1.0]
    seen, out = set(), []
    for x in xs:
        if _bits(x) not in seen:
            seen.add(_bits(x))
            out.append(float(x))
    order = np.random.default_rng(seed).permutation(len(out))
    return [out[k] for k in order]


# ------------------------------------------------------ case 1: the mixed set
# select_cases.MIXED plus descending runs that flush, at eps = 0.01, to 63, 64,
# 65, 127, 128, 129, 192 and 193 entries: the boundaries of the 64-lane stride
# and of the 128-entry class
EDGE_RUNS = [(63, 63), (64, 64), (65, 65), (179, 127), (180, 128), (181, 129), (337, 192), (338, 193)]
SET1 = C.MIXED + [("D", L, 0) for L, _ in EDGE_RUNS]


def make_set1(dev):
    ss, orc = C.make(dev, SET1)
    probe = [C.oracle_of(EPS, sp) for sp in SET1]
    flush_covered(probe, range(len(probe)))
    for k, (L, E) in enumerate(EDGE_RUNS):
        assert len(probe[len(C.MIXED) + k].v) == E, (L, E, len(probe[len(C.MIXED) + k].v))
    return ss, orc, thresholds(probe)


def case_mixed(dev, run):
    ss, orc, xs = make_set1(dev)
    assert len(xs) > 64  # (more than one wave of thresholds, several passes of k_rank)
    if run == "all":
        check_ranks(ss, orc, None, xs, "mixed, all thresholds")
    elif run == "nx1":
        check_ranks(ss, orc, None, xs[:1], "mixed, nx = 1")
    elif run == "nx3":
        check_ranks(ss, orc, None, xs[7:10], "mixed, nx = 3")
    elif run == "lo_only":
        check_ranks(ss, orc, None, xs[:11], "mixed, lo only", hi=False)
    else:
        assert run == "hi_only"
        check_ranks(ss, orc, None, xs[:11], "mixed, hi only", lo=False)


MIXED_RUNS = ["all", "nx1", "nx3", "lo_only", "hi_only"]


# ------------------------------------------------------- case 2: ranks_select
def case_select(dev):
    """MIXED_IDS: unsorted, stream 3 twice, stream 0 empty, stream 5 with nothing
    pending; neighbours 11 (listed) and 12 (unlisted) hold 49 pending values
    each; D(190) leaves the 128 class inside the call.  Then 253 more values
    into every stream."""
    ss, orc = C.make(dev, C.MIXED)
    probe = [C.oracle_of(EPS, sp) for sp in C.MIXED]
    flush_covered(probe, range(len(probe)))
    xs = thresholds(probe)
    assert len(orc[11].pending) == 49 and len(orc[12].pending) == 49 and not orc[5].pending and orc[0].n == 0
    assert C.sizes(ss, 10) == (51, 89)
    check_ranks(ss, orc, C.MIXED_IDS, xs, "ranks_select")
    assert C.sizes(ss, 10) == (138, 0) and len(orc[10].v) == 138
    assert C.sizes(ss, 12) == (51, 49) and len(orc[12].pending) == 49
    if dev != "cpu":
        assert ss.num_promoted >= 1
    extra = [C.more_values(s) for s in range(len(C.MIXED))]
    U.ingest_np(ss, extra)
    for o, x in zip(orc, extra):
        o.add_many(x)
    C.assert_all(ss, orc, "ranks_select, continued")
    check_ranks(ss, orc, None, xs[:9], "ranks after the continuation")


# ---------------------------------------------------------- case 3: twin sets
def case_equivalences(dev):
    a, orc = C.make(dev, C.MIXED)
    b, _ = C.make(dev, C.MIXED)
    c, _ = C.make(dev, C.MIXED)
    probe = [C.oracle_of(EPS, sp) for sp in C.MIXED]
    flush_covered(probe, range(len(probe)))
    xs = thresholds(probe)[:20]
    lo, hi = a.ranks(xs)
    slo, shi = b.ranks_select(C.i32(C.MIXED_IDS), xs)
    same_i64(slo, lo.cpu().numpy()[C.MIXED_IDS], "ranks_select vs ranks()[ids], lo")
    same_i64(shi, hi.cpu().numpy()[C.MIXED_IDS], "ranks_select vs ranks()[ids], hi")
    c.flush()
    R.assert_sets_equal(a, c, "ranks vs flush")
    st1 = R.snapshot(a)
    lo2, hi2 = a.ranks(xs)
    same_i64(lo2, lo.cpu().numpy(), "second ranks, lo")
    same_i64(hi2, hi.cpu().numpy(), "second ranks, hi")
    st2 = R.snapshot(a)
    for s in range(a.num_streams):
        R.assert_stream(R.stream_of_snapshot(st2, s), R.stream_of_snapshot(st1, s), "second ranks, stream %d" % s)
    flush_covered(orc, range(len(orc)))
    C.assert_all(a, orc, "after two ranks")


# ---------------------------------------------------------- case 4: promotion
def case_promoted(dev):
    """(GK_CAPS=128,256,512,4096 set by the caller) D(750), 227 entries + 43
    pending in the 256 class, climbs to 512 inside the call (270 entries);
    D(1500) (275 entries) is answered where it stands."""
    ss, orc = C.make(dev, C.PROMOTED)
    if dev != "cpu":
        assert ss.capacity(1) == 256 and ss.capacity(2) == 512
    assert C.sizes(ss, 0) == (227, 43) and len(orc[2].v) == 275
    probe = [C.oracle_of(EPS, sp) for sp in C.PROMOTED]
    flush_covered(probe, range(len(probe)))
    check_ranks(ss, orc, [2, 0, 4, 0], thresholds(probe), "promoted")
    assert C.sizes(ss, 0) == (270, 0)


# ------------------------------------------------------- case 5: a long table
def case_long_table(dev):
    """One stream whose flushed table lies beyond the 2048 class: 70 thresholds
    over its range (and both ends) in one call."""
    eps = 0.001
    ss, orc = C.make(dev, [("D", 4000, 0), (1, 150, 981)], eps=eps)
    probe = C.oracle_of(eps, ("D", 4000, 0))
    probe.size()
    assert len(probe.v) == 2079
    xs = [float(x) for x in np.linspace(probe.min - 3.0, probe.max + 3.0, 70)]
    check_ranks(ss, orc, None, xs, "long table")
    assert C.sizes(ss, 0) == (2079, 0)
    check_ranks(ss, orc, [0, 0], [probe.v[1039], probe.v[2078], probe.v[0]], "long table, selected")


# --------------------------------------------------- case 6: bracket property
def case_bracket(dev):
    """Ingest-only streams: lo <= #{values <= x} <= hi, for the definition
    (expected_ranks on the oracle) and for the engine, and hi - lo <= 2 eps n."""
    ss, orc, xs = make_set1(dev)
    glo, ghi = check_ranks(ss, orc, None, xs, "bracket")
    glo, ghi = glo.cpu().numpy(), ghi.cpu().numpy()
    elo, ehi = expected_rows(orc, range(len(orc)), xs)
    xa = np.asarray(xs)
    for s, sp in enumerate(SET1):
        vals = np.sort(C.seq(sp))
        true = np.searchsorted(vals, xa, "right")
        assert np.all(elo[s] <= true) and np.all(true <= ehi[s]), "the definition misses the count, stream %d" % s
        assert np.all(glo[s] <= true) and np.all(true <= ghi[s]), "the engine misses the count, stream %d" % s
        assert np.all(ehi[s] - elo[s] <= 2 * EPS * len(vals)), "the definition is wider than 2 eps n, stream %d" % s


# --------------------------------------------------- case 7: merged histories
MERGE_A = [(1, 1000, 971), (0, 57, 972), (2, 640, 973), (0, 0, 974), (5, 1000, 975), ("D", 700, 0)]
MERGE_B = [(3, 1500, 976), (1, 150, 977), (0, 0, 978), (4, 333, 979), (5, 101, 980), ("D", 338, 0)]


def case_merged(dev):
    """After merge_from and after rollup_from the ranks of the destination are
    the formula on the oracle's merged table; lo <= hi.  (No bracket claim: the
    reference's conversion, gk:135-147, does not keep it.)"""
    a, a_o = C.make(dev, MERGE_A)
    b, b_o = C.make(dev, MERGE_B)
    a.merge_from([b])
    for x, y in zip(a_o, b_o):
        x.merge(y)
    R.assert_set_matches(a, a_o, "merge_from dst")
    xs = thresholds(a_o)
    lo, hi = check_ranks(a, a_o, None, xs, "after merge_from")
    assert bool((lo <= hi).all())
    # one roll-up: groups of b's streams into a fresh set
    groups = [[0, 4, 1], [], [5, 3]]
    dst = U._ss(len(groups), EPS, dev)
    d_o = [OracleGK(EPS) for _ in groups]
    go, mem = R.csr_of(groups)
    dst.rollup_from(b, go, mem)
    R.oracle_fold(d_o, b_o, groups)
    R.assert_set_matches(dst, d_o, "rollup_from dst")
    lo, hi = check_ranks(dst, d_o, None, thresholds(d_o), "after rollup_from")
    assert bool((lo <= hi).all())
    slo, shi = check_ranks(dst, d_o, [2, 1, 0], xs[:5], "after rollup_from, selected")
    assert bool((slo <= shi).all())


# ------------------------------------------------------------- case 8: errors
def case_errors(dev):
    from gkarray_amd._lib import GK_E_ARG, GKBackendError
    ss, orc = C.make(dev, C.MIXED)
    S = len(C.MIXED)
    X3 = [0.5, 1.0, 2.0]
    good = [11, 3]
    nan = float("nan")
    f2 = torch.tensor([[11, 3]], dtype=torch.int32)
    bad = [
        ("NaN in xs", lambda: ss.ranks([0.5, nan]), GKBackendError, "NaN"),
        ("NaN in xs, select", lambda: ss.ranks_select(C.i32(good), [nan, 0.5]), GKBackendError, "NaN"),
        ("id == S", lambda: ss.ranks_select(C.i32([11, 3, S, -5]), X3), GKBackendError, "ids[2] = %d" % S),
        ("id == -1", lambda: ss.ranks_select(C.i32([11, -1, 3]), X3), GKBackendError, "ids[1] = -1"),
        ("id == S, int64", lambda: ss.ranks_select(torch.tensor([S, 3], dtype=torch.int64), X3), GKBackendError,
         "ids[0] = %d" % S),
        ("id == S, cdf", lambda: ss.cdf_select(C.i32([11, S]), X3), GKBackendError, "ids[1] = %d" % S),
        ("2-D ids", lambda: ss.ranks_select(f2, X3), ValueError, None),
        ("float ids", lambda: ss.ranks_select(torch.tensor([11.0, 3.0]), X3), ValueError, None),
        ("both outputs NULL", lambda: ss.ranks(X3, lo=False, hi=False), GKBackendError, "rank arguments"),
        ("both outputs NULL, select", lambda: ss.ranks_select(C.i32(good), X3, lo=False, hi=False), GKBackendError,
         "rank arguments"),
        ("an output of the wrong shape", lambda: ss.ranks(X3, lo=torch.zeros((S, 2), dtype=torch.int64,
                                                                           device=ss.device)), ValueError, None),
    ]
    st0 = R.snapshot(ss)

    def unchanged(what):
        st1 = R.snapshot(ss)
        for s in range(S):
            R.assert_stream(R.stream_of_snapshot(st1, s), R.stream_of_snapshot(st0, s),
                            "after '%s': stream %d" % (what, s))

    for what, call, exc, text in bad:
        with pytest.raises(exc) as ei:
            call()
        if exc is GKBackendError:
            assert ei.value.code == GK_E_ARG, (what, ei.value)
            assert text in str(ei.value), (what, ei.value)
        unchanged(what)
    # nx < 0 has no Python spelling: the C calls themselves, outputs prefilled
    arr = (ctypes.c_double * 3)(*X3)
    lo = torch.full((S, 3), -7, dtype=torch.int64, device=ss.device)
    hi = torch.full((S, 3), -7, dtype=torch.int64, device=ss.device)
    ids = C.i32(good).to(ss.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert ss._lib.gk_ranks(ss.handle, arr, -1, p(lo), p(hi), ss._sp()) == GK_E_ARG
    assert ss._lib.gk_ranks_select(ss.handle, p(ids), 2, arr, -1, p(lo), p(hi), ss._sp()) == GK_E_ARG
    assert ss._lib.gk_ranks(ss.handle, None, 3, p(lo), p(hi), ss._sp()) == GK_E_ARG
    assert ss._lib.gk_ranks_select(ss.handle, None, 2, arr, 3, p(lo), p(hi), ss._sp()) == GK_E_ARG
    unchanged("nx < 0 / NULL xs / NULL ids")
    # a refused call into caller tensors wrote nothing
    with pytest.raises(GKBackendError):
        ss.ranks([0.5, nan, 1.0], lo=lo, hi=hi)
    with pytest.raises(GKBackendError):
        ss.ranks_select(C.i32([11, S]), X3, lo=lo[:2], hi=hi[:2])
    assert bool((lo == -7).all()) and bool((hi == -7).all())
    # count == 0 and nx == 0: GK_OK, nothing touched
    for t in ss.ranks_select(C.i32([]), X3):
        assert tuple(t.shape) == (0, 3) and t.dtype == torch.int64
    for t in ss.ranks_select(C.i32(good), []):
        assert tuple(t.shape) == (2, 0) and t.dtype == torch.int64
    for t in ss.ranks([]):
        assert tuple(t.shape) == (S, 0)
    assert tuple(ss.cdf_select(C.i32([]), X3).shape) == (0, 3)
    assert tuple(ss.cdf([]).shape) == (S, 0)
    unchanged("count == 0 / nx == 0")
    C.assert_all(ss, orc, "after the refused calls")
    check_ranks(ss, orc, C.MIXED_IDS, X3, "valid call after the errors")


# --------------------------------------------------- case 9: overflow (GPU only)
def case_overflow(dev):
    """(GK_CAPS=128,256 set by the caller) D(750)'s flush needs 270 entries and
    the last class holds 255: GK_E_OVERFLOW, lo / hi untouched, D(750) keeps its
    227 + 43 state, the other listed stream has been flushed."""
    from gkarray_amd._lib import GK_E_OVERFLOW, GKBackendError
    specs = [(1, 150, 951), ("D", 750, 0), (1, 150, 952), (2, 50, 953)]
    ss, orc = C.make(dev, specs)
    assert ss.capacity(1) == 256 and ss.capacity(2) == -1
    assert C.sizes(ss, 1) == (227, 43)
    X3 = [0.5, 1.0, 3500.0]
    lo = torch.full((2, 3), -7, dtype=torch.int64, device=ss.device)
    hi = torch.full((2, 3), -7, dtype=torch.int64, device=ss.device)
    before = R.snapshot(ss)
    with pytest.raises(GKBackendError) as ei:
        ss.ranks_select(C.i32([1, 0]), X3, lo=lo, hi=hi)
    assert ei.value.code == GK_E_OVERFLOW, ei.value
    assert bool((lo == -7).all()) and bool((hi == -7).all())
    assert orc[0].pending
    orc[0].size()
    C.assert_all(ss, orc, "after GK_E_OVERFLOW", before, {0, 1})
    assert C.sizes(ss, 1) == (227, 43)
    # the set-wide call: the same refusal, every other stream flushed
    lo4 = torch.full((4, 3), -7, dtype=torch.int64, device=ss.device)
    with pytest.raises(GKBackendError) as ei:
        ss.ranks(X3, lo=lo4, hi=False)
    assert ei.value.code == GK_E_OVERFLOW, ei.value
    assert bool((lo4 == -7).all())
    for s in (2, 3):
        orc[s].size()
    C.assert_all(ss, orc, "after the set-wide GK_E_OVERFLOW")
    check_ranks(ss, orc, [3, 0, 2], X3, "valid call after GK_E_OVERFLOW")


# ------------------------------------------ case 10: deferred work (GPU only)
def case_deferred(dev):
    """(GK_POOL_SLOTS=2 set by the caller) an ingest left in flight defers most
    of its overflowing streams; ranks_select re-runs them before it reads."""
    specs = [("D", 600 + 75 * k, 0) if k % 4 else (k % 8, 150 + 50 * k, 960 + k) for k in range(14)]
    ss = U._ss(len(specs), EPS, dev)
    flat, offs = U.csr([C.seq(sp) for sp in specs])
    tf, to = torch.from_numpy(flat).to(dev), torch.from_numpy(offs).to(dev)
    ss.ingest(tf, to, sync=False)
    orc = [C.oracle_of(EPS, sp) for sp in specs]
    ids = [13, 1, 4, 2, 9, 1]
    xs = [0.5, 1.0, 3000.5, 3500.0, 3999.0, -1.0, 5000.0]
    flush_covered(orc, ids)
    elo, ehi = expected_rows(orc, ids, xs)
    lo, hi = ss.ranks_select(C.i32(ids), xs)
    same_i64(lo, elo, "deferred lo")
    same_i64(hi, ehi, "deferred hi")
    assert ss.num_promoted > 2  # more streams than the 2 slots a class started with: some were deferred
    C.assert_all(ss, orc, "deferred")


# --------------------------------------- case 11: drop-in and point estimate
def case_dropin(dev):
    from gkarray_amd import GKArray
    vals = R.seq(1, 777, 991)
    sk, o = GKArray(EPS, device=dev), OracleGK(EPS)
    assert sk.rank(1.0) == (0, 0) and np.isnan(sk.cdf(1.0))  # n == 0
    for v in vals[:300]:
        sk.add(v)
    sk.add_many(vals[300:])
    o.add_many(vals)
    o.size()
    for x in (o.min, o.max, o.v[len(o.v) // 2], 1.0, -1.0, 1e9, (o.v[3] + o.v[4]) / 2):
        lo, hi = expected_ranks(o, [x])
        got = sk.rank(x)
        assert got == (int(lo[0]), int(hi[0])) and all(type(t) is int for t in got), (x, got, lo, hi)
        assert sk.cdf(x) == (int(lo[0]) + int(hi[0])) / (2.0 * o.n), x
    assert sk._n == o.n and [(e.val, e.g, e.delta) for e in sk.entries] == o.table()
    # StreamSet.cdf / cdf_select == (lo + hi) / (2 n), NaN where n == 0
    ss, orc = C.make(dev, C.MIXED)
    xs = [0.5, 1.0, 2.0, -5.0, 1e9]
    cdf = ss.cdf(xs).cpu().numpy()
    lo, hi = ss.ranks(xs)
    n = ss.stats()["n"].cpu().numpy()
    assert cdf.dtype == np.float64 and cdf.shape == (len(C.MIXED), len(xs))
    for s in range(len(C.MIXED)):
        if n[s] == 0:
            assert np.all(np.isnan(cdf[s])), s
        else:
            exp = (lo[s].cpu().numpy() + hi[s].cpu().numpy()).astype(np.float64) / (2.0 * float(n[s]))
            assert cdf[s].tobytes() == exp.tobytes(), s
    sel = ss.cdf_select(C.i32(C.MIXED_IDS), xs).cpu().numpy()
    assert np.array_equal(sel, cdf[C.MIXED_IDS], equal_nan=True)
    flush_covered(orc, range(len(orc)))
    C.assert_all(ss, orc, "after cdf")


# ----------------------------------------------------------- case 12: symbols
def case_symbols():
    from gkarray_amd import _lib
    for name in ("gk_ranks", "gk_ranks_select"):
        assert name in _lib.SYMBOLS and name in _lib.CPU_SYMBOLS, name
        assert hasattr(_lib.load_cpu(), name), name
