"""Cases of the per-stream selection (gk_quantiles_select / gk_flush_select /
gk_reset_select / gk_stats_select through StreamSet.quantiles_select /
flush_select / reset_select / stats_select), shared by
tests/test_gpu_select.py (device engine) and tests/test_cpu_select.py (host
engine); the engine is the ``dev`` parameter.

The expected state is the oracle's: one ``OracleGK`` per stream, on which ONLY
the listed streams are queried, flushed or replaced by a fresh oracle -- what
the reference's user does on a dict of GKArray objects.  After every call
EVERY stream of the set, listed or not, is compared bit for bit: table (v by
bit pattern, g, delta), pending values, n / min / max / sum / avg; unlisted
streams also against an ``export_state()`` snapshot taken before the call.
Test infrastructure only."""
import copy
import functools

import numpy as np
import pytest
import torch

import parity_util as U
import rollup_cases as R
from gk_oracle import OracleGK

EPS = 0.01
Q3 = [0.5, 0.9, 0.99]


def D(n):
    """The first n values of a descending run: tables grow fastest on it."""
    return np.arange(4000.)[::-1][:n].copy()


def seq(spec):
    dist, L, seed = spec
    return D(L) if dist == "D" else R.seq(dist, L, seed)


@functools.lru_cache(maxsize=None)
def _ingested(eps, spec):
    o = OracleGK(eps)
    o.add_many(seq(spec))
    return o


def oracle_of(eps, spec):
    """A fresh oracle stream holding spec = (dist, L, seed) (ingested once, then copied)."""
    return copy.deepcopy(_ingested(eps, spec))


def make(dev, specs, eps=EPS):
    ss = U._ss(len(specs), eps, dev)
    U.ingest_np(ss, [seq(sp) for sp in specs])
    return ss, [oracle_of(eps, sp) for sp in specs]


def i32(ids):
    return torch.tensor(list(ids), dtype=torch.int32)


def assert_all(ss, oracles, what, before=None, listed=()):
    """Every stream against its oracle; the unlisted ones also against `before`."""
    st = R.snapshot(ss)
    for s, o in enumerate(oracles):
        got = R.stream_of_snapshot(st, s)
        role = "listed" if s in listed else "unlisted"
        R.assert_stream(got, R.stream_of_oracle(o), "%s stream %d (%s)" % (what, s, role))
        if before is not None and s not in listed:
            R.assert_stream(got, R.stream_of_snapshot(before, s),
                            "%s unlisted %d vs its state before the call" % (what, s))
    return st


def oracle_answers(oracles, ids, qs, single):
    rows = [[oracles[s].quantile(q) for q in qs] if single else oracles[s].quantiles(qs) for s in ids]
    return np.asarray(rows, dtype=np.float64).reshape(len(ids), len(qs))


def check_query(ss, oracles, ids, qs, single, what, before=True):
    """quantiles_select on the engine, quantile()/quantiles() on the listed oracles only.
    `before`: True takes the snapshot that unlisted streams are compared with; a
    snapshot the caller holds is used as it is; None makes quantiles_select the
    first call the set sees (no comparison with the state before)."""
    if before is True:
        before = R.snapshot(ss)
    got = ss.quantiles_select(i32(ids), qs, single=single).cpu().numpy()
    assert got.shape == (len(ids), len(qs))
    U.assert_same_quantiles(got, oracle_answers(oracles, ids, qs, single), what + " answers", None)
    return assert_all(ss, oracles, what, before, set(ids))


def sizes(ss, s):
    st = ss.stats_select(i32([s]))
    return int(st["size"][0]), int(st["pending"][0])


# ---------------------------------------------------------------- case 1 data
# lengths 0, 1, 50, 99, 100, 101, 150, 202, 1000, 1500 over parity_util.gen's
# distributions, D(190), and two lognormal neighbours of 150 values (11 listed,
# 12 not: both hold 49 pending values)
MIXED = [(0, 0, 900), (1, 1, 901), (2, 50, 902), (3, 99, 903), (4, 100, 904), (5, 101, 905), (6, 150, 906),
         (7, 202, 907), (0, 1000, 908), (1, 1500, 909), ("D", 190, 0), (1, 150, 911), (1, 150, 912), (1, 50, 913),
         (5, 1000, 914), (0, 0, 915)]
# unsorted, stream 3 twice, stream 0 has n = 0, streams 5 (101 values) has no pending value
MIXED_IDS = [10, 3, 11, 8, 0, 6, 3, 9, 5, 1]
MIXED_RUNS = {
    "sorted_list": ([0.0, 0.25, 0.5, 0.9, 0.99, 1.0], False),
    "unsorted_list": ([0.9, 0.1, 0.5, 1.0, 0.0], False),
    "single": ([0.0, 0.5, 0.99, 1.0], True),
    "out_of_range": ([-0.1, 0.5, 1.5], False),
    "nq70": ([float(x) for x in np.linspace(0.0, 1.0, 70)], False),  # wave_quantiles' q += 64 loop wraps
}


def case_mixed(dev, run):
    qs, single = MIXED_RUNS[run]
    ss, orc = make(dev, MIXED)
    assert orc[11].pending and orc[12].pending and not orc[5].pending and orc[0].n == 0
    assert (len(orc[10].v), len(orc[10].pending)) == (51, 89)
    assert sizes(ss, 10) == (51, 89)
    check_query(ss, orc, MIXED_IDS, qs, single, "mixed " + run)
    # D(190) left the 128-entry class inside the call
    assert sizes(ss, 10) == (138, 0) and len(orc[10].v) == 138
    if dev != "cpu":
        assert ss.num_promoted >= 1
    return ss, orc


def more_values(s, L=253):
    return R.seq(1, L, 7000 + s)


def case_continuation(dev):
    """After case 1: 253 more values into every stream, then quantiles() of the
    whole set.  Queried and never-queried streams each continue their own
    history -- a compression at a point that is no flush point changes every
    later table."""
    ss, orc = case_mixed(dev, "sorted_list")
    never = [oracle_of(EPS, sp) for sp in MIXED]  # the history of a set-wide-unqueried stream
    extra = [more_values(s) for s in range(len(MIXED))]
    U.ingest_np(ss, extra)
    for o, m, x in zip(orc, never, extra):
        o.add_many(x)
        m.add_many(x)
    # the query of case 1 is visible in the later table of stream 11 (150
    # lognormal values, queried, 253 more), not in its unqueried neighbour's
    assert orc[11].table() != never[11].table()
    assert orc[12].table() == never[12].table()
    assert_all(ss, orc, "continuation")
    got = ss.quantiles(R.QS).cpu().numpy()
    exp = np.asarray([o.quantiles(R.QS) for o in orc], dtype=np.float64).reshape(len(orc), len(R.QS))
    U.assert_same_quantiles(got, exp, "continuation quantiles", None)
    assert_all(ss, orc, "continuation after quantiles()")


# ------------------------------------------------------- case 3: promoted streams
PROMOTED = [("D", 750, 0), (1, 150, 921), ("D", 1500, 0), (2, 640, 923), (1, 150, 924), (0, 57, 925)]


def case_promoted(dev):
    """(GK_CAPS=128,256,512,4096 set by the caller) D(750) sits in the 256 class
    (227 entries + 43 pending) and climbs to 512 inside the call (270 entries);
    D(1500) (275 entries) is queried where it stands."""
    ss, orc = make(dev, PROMOTED)
    if dev != "cpu":
        assert ss.capacity(1) == 256 and ss.capacity(2) == 512
    assert sizes(ss, 0) == (227, 43) and (len(orc[0].v), len(orc[0].pending)) == (227, 43)
    assert len(orc[2].v) == 275
    check_query(ss, orc, [2, 0, 4, 0], Q3, False, "promoted")
    assert sizes(ss, 0) == (270, 0)
    # and the set goes on: more values into every stream, set-wide query
    extra = [more_values(s, 300) for s in range(len(PROMOTED))]
    U.ingest_np(ss, extra)
    for o, x in zip(orc, extra):
        o.add_many(x)
    assert_all(ss, orc, "promoted, continued")
    got = ss.quantiles(Q3).cpu().numpy()
    exp = np.asarray([o.quantiles(Q3) for o in orc], dtype=np.float64).reshape(len(orc), len(Q3))
    U.assert_same_quantiles(got, exp, "promoted, continued quantiles", None)


# ------------------------------------------------------------------ case 4: reset
RESET = [(1, 150, 931), ("D", 1500, 0), (0, 0, 933), (2, 640, 934), ("D", 1500, 0), (1, 50, 935), (3, 333, 936)]


def case_reset(dev):
    ss, orc = make(dev, RESET)
    ids = [1, 0, 2, 1]  # class 0, D(1500) (class 1 on the default ladder), n = 0; one repeat
    promoted = ss.num_promoted
    if dev != "cpu":
        assert promoted >= 2  # (both D(1500) streams at least)
    before = R.snapshot(ss)
    ss.reset_select(i32(ids))
    for s in set(ids):
        orc[s] = OracleGK(EPS)
    assert_all(ss, orc, "reset", before, set(ids))
    assert ss.num_promoted == promoted  # a reset stream keeps its class
    # new values into the reset streams only: they equal fresh oracles
    fresh = {0: R.seq(1, 380, 941), 1: D(700), 2: R.seq(2, 101, 942)}
    batch = [fresh.get(s, np.zeros(0)) for s in range(len(RESET))]
    before = R.snapshot(ss)
    U.ingest_np(ss, batch)
    for s, x in fresh.items():
        orc[s].add_many(x)
    assert_all(ss, orc, "ingest after reset", before, set(fresh))
    check_query(ss, orc, [2, 1, 0, 4], Q3, False, "query after reset")
    assert ss.num_promoted == promoted
    # stats_select == stats()[ids]
    want = [6, 1, 1, 0, 4, 2]
    full = ss.stats()
    sel = ss.stats_select(i32(want))
    assert sorted(sel) == sorted(full)
    for k in full:
        a = sel[k].cpu().numpy()
        b = full[k].cpu().numpy()[want]
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    orc_n = [orc[s].n for s in want]
    assert sel["n"].cpu().tolist() == orc_n


# ----------------------------------------------------------- case 5: flush_select
def case_flush(dev):
    a, orc = make(dev, MIXED)
    b, _ = make(dev, MIXED)
    a.quantiles_select(i32(MIXED_IDS), Q3)
    before = R.snapshot(b)
    b.flush_select(i32(MIXED_IDS))
    for s in set(MIXED_IDS):
        orc[s].size()  # gk:45-46
    R.assert_sets_equal(a, b, "flush_select vs quantiles_select")
    st1 = assert_all(b, orc, "flush_select", before, set(MIXED_IDS))
    b.flush_select(i32(MIXED_IDS))  # nothing pending any more: no re-compression
    st2 = R.snapshot(b)
    for s in range(b.num_streams):
        R.assert_stream(R.stream_of_snapshot(st2, s), R.stream_of_snapshot(st1, s), "second flush_select, stream %d" % s)


# ----------------------------------------------------------------- case 6: errors
def case_errors(dev):
    from gkarray_amd._lib import GK_E_ARG, GKBackendError
    ss, orc = make(dev, MIXED)
    S = len(MIXED)
    good = [11, 3]
    bad = [
        ("query id == S", lambda: ss.quantiles_select(i32([11, 3, S, -5]), Q3), GKBackendError, "ids[2] = %d" % S),
        ("query id == -1", lambda: ss.quantiles_select(i32([11, -1, 3]), Q3), GKBackendError, "ids[1] = -1"),
        ("query id == S, int64", lambda: ss.quantiles_select(torch.tensor([S, 3], dtype=torch.int64), Q3),
         GKBackendError, "ids[0] = %d" % S),
        ("flush id == S", lambda: ss.flush_select(i32([11, S])), GKBackendError, "ids[1] = %d" % S),
        ("reset id == S", lambda: ss.reset_select(i32([11, 8, S])), GKBackendError, "ids[2] = %d" % S),
        ("reset id == -1", lambda: ss.reset_select(i32([-1, 8])), GKBackendError, "ids[0] = -1"),
        ("stats id == S", lambda: ss.stats_select(i32([S])), GKBackendError, "ids[0] = %d" % S),
        ("NaN in qs", lambda: ss.quantiles_select(i32(good), [0.5, float("nan")]), GKBackendError, "NaN"),
        ("2-D ids", lambda: ss.quantiles_select(torch.tensor([[11, 3]], dtype=torch.int32), Q3), ValueError, None),
        ("2-D ids, reset", lambda: ss.reset_select(torch.tensor([[11, 3]], dtype=torch.int32)), ValueError, None),
        ("float ids", lambda: ss.quantiles_select(torch.tensor([11.0, 3.0]), Q3), ValueError, None),
        ("float ids, stats", lambda: ss.stats_select(torch.tensor([11.0, 3.0], dtype=torch.float64)), ValueError, None),
        ("id beyond int32", lambda: ss.flush_select(torch.tensor([2 ** 32 + 3], dtype=torch.int64)), ValueError, None),
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
    # count == 0 and nq == 0: GK_OK, nothing touched
    out = ss.quantiles_select(i32([]), Q3)
    assert tuple(out.shape) == (0, 3)
    out = ss.quantiles_select(i32(good), [])
    assert tuple(out.shape) == (2, 0)
    ss.flush_select(i32([]))
    ss.reset_select(torch.zeros(0, dtype=torch.int64))
    assert all(v.numel() == 0 for v in ss.stats_select(i32([])).values())
    unchanged("count == 0 / nq == 0")
    assert_all(ss, orc, "after the refused calls")
    check_query(ss, orc, MIXED_IDS, Q3, False, "valid call after the errors")


# --------------------------------------------------- case 7: overflow (GPU only)
def case_overflow(dev):
    """(GK_CAPS=128,256 set by the caller) D(750)'s flush needs 270 entries and
    the last class holds 255: GK_E_OVERFLOW, D(750) keeps its 227 + 43 state,
    the other listed stream has been flushed."""
    from gkarray_amd._lib import GK_E_OVERFLOW, GKBackendError
    specs = [(1, 150, 951), ("D", 750, 0), (1, 150, 952), (2, 50, 953)]
    ss, orc = make(dev, specs)
    assert ss.capacity(1) == 256 and ss.capacity(2) == -1
    assert sizes(ss, 1) == (227, 43)
    before = R.snapshot(ss)
    with pytest.raises(GKBackendError) as ei:
        ss.quantiles_select(i32([1, 0]), Q3)
    assert ei.value.code == GK_E_OVERFLOW, ei.value
    assert orc[0].pending
    orc[0].size()
    assert_all(ss, orc, "after GK_E_OVERFLOW", before, {0, 1})
    assert sizes(ss, 1) == (227, 43)
    with pytest.raises(GKBackendError) as ei:
        ss.flush_select(i32([1, 2]))
    assert ei.value.code == GK_E_OVERFLOW, ei.value
    orc[2].size()
    assert_all(ss, orc, "after the second GK_E_OVERFLOW")
    check_query(ss, orc, [3, 0, 2], Q3, False, "valid call after GK_E_OVERFLOW")


# ------------------------------------------ case 8: deferred work first (GPU only)
def case_deferred(dev):
    """(GK_POOL_SLOTS=2 set by the caller) an ingest left in flight defers most
    of its overflowing streams; quantiles_select re-runs them before it reads."""
    specs = [("D", 600 + 75 * k, 0) if k % 4 else (k % 8, 150 + 50 * k, 960 + k) for k in range(14)]
    S = len(specs)
    ss = U._ss(S, EPS, dev)
    flat, offs = U.csr([seq(sp) for sp in specs])
    tf, to = torch.from_numpy(flat).to(dev), torch.from_numpy(offs).to(dev)
    ss.ingest(tf, to, sync=False)
    orc = [oracle_of(EPS, sp) for sp in specs]
    ids = [13, 1, 4, 2, 9, 1]
    got = ss.quantiles_select(i32(ids), Q3).cpu().numpy()
    U.assert_same_quantiles(got, oracle_answers(orc, ids, Q3, False), "deferred answers", None)
    assert ss.num_promoted > 2  # more streams than the 2 slots a class started with: some were deferred
    assert_all(ss, orc, "deferred")


# ------------- case 9: a fused query left in flight, then reset() (found by the
# random sequences of opseq_cases: tiny arenas, eps = 0.01, seed 23, step 104)
def case_reset_after_fused_query_in_flight(dev):
    """(GK_POOL_SLOTS=2 set by the caller) ``ingest(quantiles=..., sync=False)``
    defers most of its overflowing streams, and ``reset()`` follows directly.
    The reset voids the streams' state, not the answers of the call before it:
    every row of the fused query's output is the oracle's, the deferred streams'
    rows included, which only the re-run writes."""
    specs = [("D", 600 + 75 * k, 0) if k % 4 else (k % 8, 150 + 50 * k, 960 + k) for k in range(14)]
    S = len(specs)
    ss = U._ss(S, EPS, dev)
    flat, offs = U.csr([seq(sp) for sp in specs])
    tf, to = torch.from_numpy(flat).to(dev), torch.from_numpy(offs).to(dev)
    # (the output is allocated uninitialised: leave a block of that size behind that holds no answer)
    junk = torch.full((S, len(Q3)), -7.0, dtype=torch.float64, device=tf.device)
    del junk
    got = ss.ingest(tf, to, quantiles=Q3, sync=False)
    ss.reset()
    ss.sync()
    orc = [oracle_of(EPS, sp) for sp in specs]
    U.assert_same_quantiles(got.cpu().numpy(), oracle_answers(orc, range(S), Q3, False),
                            "answers of the call before reset()", None)
    fresh = [OracleGK(EPS) for _ in range(S)]
    assert_all(ss, fresh, "after reset()")
    # and the set starts over: the same batch again, settled by a selection
    ss.ingest(tf, to, sync=False)
    again = [oracle_of(EPS, sp) for sp in specs]
    check_query(ss, again, [13, 1, 4, 2, 9, 1], Q3, False, "the same batch after reset()")
