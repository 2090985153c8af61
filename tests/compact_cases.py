"""Cases of compaction (gk_compact / gk_class_usage through StreamSet.compact /
class_usage and KeyedStreamSet.compact), shared by tests/test_gpu_compact.py
(device engine) and tests/test_cpu_compact.py (host engine); the engine is the
``dev`` parameter.

A compaction may change where a stream lives, never what it holds: after every
``compact()`` EVERY stream is compared bit for bit with its oracle (one
``OracleGK`` per stream, or one ``OracleSet`` for the 4099-stream case) and
with an ``export_state()`` snapshot taken before the call -- table (v by bit
pattern, g, delta), pending values in order, n / min / max / sum / avg -- and
the streams then go on ingesting against the same oracles.  What does change
is read through ``class_usage()``.  The GPU cases run on the ladder
GK_CAPS=128,256,512,4096 (set by the caller) unless they say otherwise; the
table sizes they rest on are the ones transfer_cases.case_promotion asserts:
D(190) 138 entries (class 1), D(1500) 285 (class 2), DL(60000) 512..4094
(class 3).  Test infrastructure only."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import parity_util as U
import rank_cases as K
import rollup_cases as R
import select_cases as C
import transfer_cases as T
from gk_oracle import OracleGK

EPS = C.EPS
ZERO = {"demoted": 0, "bytes_freed": 0}


def is_gpu(dev):
    return torch.device(dev).type != "cpu"


def per_class(ss, key="streams"):
    return [u[key] for u in ss.class_usage()]


def held_bytes(usage):
    return sum(u["arena_bytes"] + u["workspace_bytes"] for u in usage)


def check_usage(ss, what):
    """The invariants of class_usage() on any set; returns the list."""
    use = ss.class_usage()
    S = ss.num_streams
    assert sum(u["streams"] for u in use) == S, what
    assert sum(u["streams"] for u in use[1:]) == ss.num_promoted, what
    assert (use[0]["slots_used"], use[0]["slots_alloc"]) == (S, S), what
    for c, u in enumerate(use):
        assert sorted(u) == ["arena_bytes", "capacity", "slots_alloc", "slots_used", "streams", "workspace_bytes"]
        assert u["capacity"] == ss.capacity(c) and 0 <= u["slots_used"] <= u["slots_alloc"], (what, c, u)
        assert u["streams"] <= u["slots_used"] and u["workspace_bytes"] >= 0, (what, c, u)
        if not ss.is_cpu:
            assert u["arena_bytes"] == u["slots_alloc"] * u["capacity"] * 16, (what, c, u)
    assert ss.capacity(len(use)) == -1
    return use


def compact_checked(ss, oracles, what):
    """compact() with everything that must hold around it; returns its result."""
    before = R.snapshot(ss)
    use0 = check_usage(ss, what + " before")
    res = ss.compact()
    assert sorted(res) == ["bytes_freed", "demoted"], what
    use1 = check_usage(ss, what + " after")
    T.same_snapshot(ss, before, what)
    if oracles is not None:
        C.assert_all(ss, oracles, what)
    assert res["bytes_freed"] == held_bytes(use0) - held_bytes(use1), (what, res, use0, use1)
    if ss.is_cpu:
        assert res["demoted"] == 0 and res["bytes_freed"] >= 0 and len(use1) == 1, (what, res)
        return res
    moved_down = sum(a["streams"] - b["streams"] for a, b in zip(use0[1:], use1[1:]))
    assert use1[0]["streams"] - use0[0]["streams"] == moved_down <= res["demoted"], (what, res, use0, use1)
    for c, u in enumerate(use1[1:], 1):
        # dense slots; twice the members (or what a new set starts with) and never more than before
        assert u["slots_used"] == u["streams"], (what, c, u)
        assert u["slots_alloc"] <= max(use0[c]["slots_alloc"], u["streams"]), (what, c, u, use0[c])
    return res


@functools.lru_cache(maxsize=None)
def _dl_oracle():
    o = OracleGK(EPS)
    o.add_many(T.DL(60000))
    o.size()
    return o


# ------------------------------------------------- case 1: a reset gives back (GPU)
def case_reset_gives_back(dev):
    small = [(1, 150, 1101), (2, 50, 1102), (0, 0, 1103), (5, 101, 1104)]
    seqs = [C.D(190), C.D(1500), T.DL(60000)] + [C.seq(sp) for sp in small]
    ss = U._ss(7, EPS, dev)
    U.ingest_np(ss, seqs)
    ss.flush()
    orc = [C.oracle_of(EPS, ("D", 190, 0)), C.oracle_of(EPS, ("D", 1500, 0)), copy.deepcopy(_dl_oracle())]
    orc += [C.oracle_of(EPS, sp) for sp in small]
    for o in orc:
        o.size()
    assert [len(o.v) for o in orc[:2]] == [138, 285] and 512 <= len(orc[2].v) < 4095
    C.assert_all(ss, orc, "reset gives back: ingested")
    assert per_class(ss) == [4, 1, 1, 1] and ss.num_promoted == 3
    ss.reset_select(C.i32([1, 2]))
    orc[1], orc[2] = OracleGK(EPS), OracleGK(EPS)
    assert per_class(ss) == [4, 1, 1, 1] and ss.num_promoted == 3  # a reset stream keeps its class
    res = compact_checked(ss, orc, "reset gives back")
    assert res["demoted"] == 2, res
    use = ss.class_usage()
    assert [(u["streams"], u["slots_used"]) for u in use[1:]] == [(1, 1), (0, 0), (0, 0)], use
    assert ss.num_promoted == 1
    # one of them is promoted again, through the classes the compaction emptied
    batch = [np.zeros(0)] * 7
    batch[2] = C.D(1500)
    U.ingest_np(ss, batch)
    ss.flush_select(C.i32([2]))
    orc[2].add_many(C.D(1500))
    orc[2].size()
    C.assert_all(ss, orc, "promoted again after the compaction")
    assert per_class(ss) == [5, 1, 1, 0] and ss.num_promoted == 2
    R.assert_quantiles(ss, orc, "promoted again after the compaction")
    C.assert_all(ss, orc, "promoted again, after quantiles()")
    # straight after a compaction a second one finds nothing to do
    compact_checked(ss, orc, "first of two")
    use = ss.class_usage()
    assert compact_checked(ss, orc, "second of two") == ZERO
    assert ss.class_usage() == use


# ----------------------------------------------------- case 2: fit boundaries (GPU)
FIT_E = [0, 1, 127, 128, 255, 256, 511, 512]
FIT_P = [0, 1, 100, 0, 1, 100, 0, 1]


def case_fit_boundaries(dev):
    rng = np.random.default_rng(12)
    ss = U._ss(8, EPS, dev)
    assert [ss.capacity(c) for c in range(5)] == [128, 256, 512, 4096, -1]
    ids = torch.arange(8, dtype=torch.int32)
    # 600 entries: every stream into class 3
    ss.put(ids, T.import_synthetic("cpu", T.synthetic_state(rng, [600] * 8, [0] * 8)))
    assert per_class(ss) == [0, 0, 0, 8]
    exp = T.synthetic_state(rng, FIT_E, FIT_P)
    ss.put(ids, T.import_synthetic("cpu", exp))
    assert per_class(ss) == [0, 0, 0, 8]  # unpack_select never demotes
    T.assert_state_arrays(R.snapshot(ss), np.arange(8), exp, "fit boundaries, installed")
    res = compact_checked(ss, None, "fit boundaries")
    assert res["demoted"] == 7, res
    assert per_class(ss) == [3, 2, 2, 1]
    T.assert_state_arrays(R.snapshot(ss), np.arange(8), exp, "fit boundaries, compacted")
    # every stream can still be read through the selection calls and packed again
    t = ss.take(ids)
    T.assert_state_arrays(R.snapshot(t), np.arange(8), exp, "fit boundaries, taken after the compaction")


# ------------------------------------------------- case 3: no-op and idempotence
def case_noop(dev):
    gpu = is_gpu(dev)
    # a set nothing was promoted in
    ss, orc = C.make(dev, [(1, 150, 1111), (2, 50, 1112), (0, 0, 1113), (5, 101, 1114), (3, 99, 1115)])
    use = check_usage(ss, "fresh set")
    res = compact_checked(ss, orc, "fresh set")
    if gpu:
        assert res == ZERO and ss.class_usage() == use
    use = ss.class_usage()
    assert compact_checked(ss, orc, "fresh set, again") == ZERO and ss.class_usage() == use
    # promoted streams that all still need their class: two tables of 138 entries grown by
    # ingest (class 1) and one of 285 installed by put (straight into class 2)
    ss, orc = C.make(dev, [("D", 190, 0), (1, 150, 1116), ("D", 190, 0), (0, 57, 1117)])
    ss.flush_select(C.i32([0, 2]))
    orc[0].size()
    orc[2].size()
    src, so = C.make("cpu", [("D", 1500, 0)])
    src.flush()
    so[0].size()
    ss.put(C.i32([3]), src)
    orc[3] = so[0]
    assert (len(orc[0].v), len(orc[3].v)) == (138, 285)
    if gpu:
        assert per_class(ss) == [1, 2, 1, 0]
    use = check_usage(ss, "all still needed")
    res = compact_checked(ss, orc, "all still needed")
    if gpu:
        assert res == ZERO and ss.class_usage() == use
    use = ss.class_usage()
    assert compact_checked(ss, orc, "all still needed, again") == ZERO and ss.class_usage() == use
    # an empty set
    none = U._ss(0, EPS, dev)
    assert none.compact() == ZERO and per_class(none)[0] == 0
    # and the streams go on
    extra = [C.more_values(20 + s, 120) for s in range(4)]
    U.ingest_np(ss, extra)
    for o, x in zip(orc, extra):
        o.add_many(x)
    C.assert_all(ss, orc, "all still needed, continued")


# ------------------------- case 4: more than one workgroup, partial waves (GPU)
def case_many_streams(dev, S=4099):
    """(default ladder: class 0 holds 128 entries, class 1 2048) every third
    stream is promoted with D(190), every second of those reset again; the
    others hold 1..150 random values, pending ones among them."""
    rng = np.random.default_rng(S)
    ss = U._ss(S, EPS, dev)
    assert ss.capacity(0) == 128
    prom = np.arange(0, S, 3)
    gone = prom[::2]
    kept = prom[1::2]
    empty = np.zeros(0)

    def batch(ids, make):
        sel = set(int(s) for s in ids)
        return U.csr([make(s) if s in sel else empty for s in range(S)])

    d190 = batch(prom, lambda s: C.D(190))
    ss.ingest(torch.from_numpy(d190[0]), torch.from_numpy(d190[1]))
    ss.flush()
    assert per_class(ss)[:2] == [S - len(prom), len(prom)]
    ss.reset_select(torch.from_numpy(gone.astype(np.int32)))
    others = np.setdiff1d(np.arange(S), prom)
    lens = rng.integers(1, 151, S)
    rest = batch(others, lambda s: U.gen(int(s) % 8, int(lens[s]), rng))
    ss.ingest(torch.from_numpy(rest[0]), torch.from_numpy(rest[1]))
    # the oracle: the reset streams are fresh ones
    osx = U.OracleSet(S, EPS)
    osx.ingest(*batch(kept, lambda s: C.D(190)))
    osx.flush()
    osx.ingest(*rest)
    U.assert_same_state(ss, osx, "many streams, before")
    st = ss.stats()
    assert int((st["pending"] > 0).sum()) > S // 4 and int((st["size"] > 0).sum()) > S // 4
    assert per_class(ss)[:2] == [S - len(prom), len(prom)]
    res = compact_checked(ss, None, "many streams")
    assert res["demoted"] == len(gone), res
    use = ss.class_usage()
    assert [u["streams"] for u in use] == [S - len(kept), len(kept)] + [0] * (len(use) - 2)
    assert use[1]["slots_used"] == len(kept)
    U.assert_same_state(ss, osx, "many streams, compacted")
    # one more ingest on every stream: a descending run each
    more = U.csr([-1.0 - np.arange(40 + s % 90, dtype=np.float64) for s in range(S)])
    ss.ingest(torch.from_numpy(more[0]), torch.from_numpy(more[1]))
    osx.ingest(*more)
    U.assert_same_state(ss, osx, "many streams, continued")
    got = ss.quantiles(C.Q3).cpu().numpy()
    U.assert_same_quantiles(got, osx.quantiles(C.Q3), "many streams, continued quantiles", None)


# ----------------------------------------- case 5: arenas shrink and regrow (GPU)
def case_arenas(dev):
    """(GK_POOL_SLOTS=2 set by the caller) 12 streams in class 1 have grown its
    arena; 11 are reset and the compaction shrinks it to the 2 slots a new set
    starts with; 5 streams then come back."""
    specs = [("D", 190, 0)] * 12 + [(1, 150, 1121), (0, 57, 1122)]
    ss, orc = C.make(dev, specs)
    ss.flush()
    for o in orc:
        o.size()
    C.assert_all(ss, orc, "arenas: promoted")
    use = check_usage(ss, "arenas: promoted")
    assert use[1]["streams"] == 12 and use[1]["slots_alloc"] >= 12 and use[2]["slots_alloc"] == 2, use
    ss.reset_select(torch.arange(1, 12, dtype=torch.int32))
    for s in range(1, 12):
        orc[s] = OracleGK(EPS)
    res = compact_checked(ss, orc, "arenas")
    use = ss.class_usage()
    assert res["demoted"] == 11 and res["bytes_freed"] > 0, res
    assert (use[1]["streams"], use[1]["slots_used"], use[1]["slots_alloc"]) == (1, 1, 2), use
    # an empty batch goes through grow_pools: no arena is regrown
    U.ingest_np(ss, [np.zeros(0)] * 14)
    assert ss.class_usage() == use
    # 5 streams come back: 1 free slot, so most are deferred and the arena grows again
    batch = [C.D(190) if 1 <= s <= 5 else np.zeros(0) for s in range(14)]
    U.ingest_np(ss, batch)
    ss.flush()
    for s in range(1, 6):
        orc[s].add_many(C.D(190))
    for o in orc:
        o.size()
    C.assert_all(ss, orc, "arenas: promoted again")
    again = check_usage(ss, "arenas: promoted again")
    assert again[1]["streams"] == 6 and again[1]["slots_alloc"] >= 6, again
    U.ingest_np(ss, [np.zeros(0)] * 14)
    later = ss.class_usage()
    for c in (2, 3):  # nobody entered these
        assert later[c] == use[c], (c, later, use)
    R.assert_quantiles(ss, orc, "arenas: promoted again")


# ------------------------------------------------- case 6: settles first (GPU)
def case_deferred(dev):
    """(GK_POOL_SLOTS=2 set by the caller) an ingest left in flight defers most of
    its overflowing streams; compact() re-runs them before it places anything."""
    specs = [("D", 600 + 75 * k, 0) if k % 4 else (k % 8, 150 + 50 * k, 960 + k) for k in range(14)]
    ss = U._ss(len(specs), EPS, dev)
    flat, offs = U.csr([C.seq(sp) for sp in specs])
    tf, to = torch.from_numpy(flat).to(dev), torch.from_numpy(offs).to(dev)
    ss.ingest(tf, to, sync=False)
    res = ss.compact()
    orc = [C.oracle_of(EPS, sp) for sp in specs]
    C.assert_all(ss, orc, "deferred, compacted")
    assert ss.num_promoted > 2  # more streams than the 2 slots a class started with: some were deferred
    assert ss.num_promoted == sum(1 for o in orc if len(o.v) > 127), res
    use = check_usage(ss, "deferred, compacted")
    assert all(u["slots_used"] == u["streams"] for u in use[1:]), use
    R.assert_quantiles(ss, orc, "deferred, compacted")


def case_sticky_error(dev):
    """(GK_CAPS=128,256 set by the caller) D(1500) needs 275 entries and the last
    class holds 255: the ingest left in flight ends in a sticky GK_E_OVERFLOW,
    which compact() returns instead of compacting."""
    from gkarray_amd._lib import GK_E_OVERFLOW, GKBackendError
    ss, _ = C.make(dev, [("D", 190, 0), (1, 150, 1131), (0, 57, 1132), ("D", 190, 0)])
    assert ss.capacity(1) == 256 and ss.capacity(2) == -1
    ss.flush_select(C.i32([0, 3]))
    ss.reset_select(C.i32([3]))
    assert per_class(ss) == [2, 2]
    flat, offs = U.csr([np.zeros(0), C.D(1500), np.zeros(0), np.zeros(0)])
    tf, to = torch.from_numpy(flat).to(dev), torch.from_numpy(offs).to(dev)
    ss.ingest(tf, to, sync=False)
    use = check_usage(ss, "sticky error")  # (settles the set; the error stays for the next call that reports one)
    assert use[1]["streams"] >= 2
    with pytest.raises(GKBackendError) as ei:
        ss.compact()
    assert ei.value.code == GK_E_OVERFLOW, ei.value
    assert ss.class_usage() == use
    # the error is spent: the next compaction does the work
    res = ss.compact()
    assert res["demoted"] >= 1 and per_class(ss)[0] >= 2, res  # (the reset stream at least)


# ----------------------------------------------------- case 7: random sequences
def case_random(dev, seed):
    gpu = is_gpu(dev)
    rng = np.random.default_rng(seed)
    S = 24
    ss = U._ss(S, EPS, dev)
    orc = [OracleGK(EPS) for _ in range(S)]
    top = [1e6] * S  # descending runs go on below everything the stream has seen
    cap0 = ss.capacity(0) if gpu else None
    xs = [-1.0, 0.5, 3.0, 100.0, 5e5]
    demoted = 0

    def compact(what):
        nonlocal demoted
        res = compact_checked(ss, orc, what)
        demoted += res["demoted"]
        if gpu:
            assert ss.num_promoted == sum(1 for o in orc if len(o.v) > cap0 - 1), what
        R.assert_quantiles(ss, orc, what)
        C.assert_all(ss, orc, what + ", after quantiles()")

    for step in range(40):
        what = "seed %d step %d" % (seed, step)
        op = rng.choice(["ingest", "reset", "flush", "put", "ranks", "compact"], p=[0.4, 0.14, 0.1, 0.1, 0.08, 0.18])
        ids = [int(s) for s in rng.integers(0, S, int(rng.integers(1, 7)))]
        if op == "ingest":
            batch = [np.zeros(0)] * S
            for s in set(ids):
                if rng.random() < 0.5:
                    L = int(rng.choice([138, 190, 400, 750, 1500]))  # lengths that cross class boundaries
                    batch[s] = top[s] - np.arange(L, dtype=np.float64)
                    top[s] -= L
                else:
                    batch[s] = np.asarray(U.gen(int(rng.integers(0, 8)), int(rng.integers(0, 300)), rng), np.float64)
            U.ingest_np(ss, batch)
            for s in set(ids):
                orc[s].add_many(batch[s])
        elif op == "reset":
            ss.reset_select(C.i32(ids))
            for s in set(ids):
                orc[s] = OracleGK(EPS)
                top[s] = 1e6
        elif op == "flush":
            ss.flush_select(C.i32(ids))
            for s in set(ids):
                orc[s].size()
        elif op == "put":
            # small tables into promoted streams (any stream while none is promoted)
            big = [s for s in range(S) if len(orc[s].v) > 127]
            where = sorted(set(big[:3] if big else ids[:2]))
            specs = [(int(rng.integers(0, 8)), int(rng.integers(0, 150)), 5000 + 100 * step + k)
                     for k in range(len(where))]
            src, so = C.make("cpu", specs)
            ss.put(C.i32(where), src)
            for s, o in zip(where, so):
                orc[s] = o
                top[s] = 1e6
        elif op == "ranks":
            K.check_ranks(ss, orc, ids, xs, what, before=None)
            continue
        else:
            compact(what)
            continue
        C.assert_all(ss, orc, what + " " + op)
    compact("seed %d, the end" % seed)
    return demoted


# ------------------------------------------------ case 8: KeyedStreamSet churn
def case_keyed_churn(dev):
    import gkarray_amd as P
    gpu = is_gpu(dev)
    kss = P.KeyedStreamSet(EPS, capacity=16, device=dev)
    old = np.arange(100, 106, dtype=np.int64)
    # six series of 190 descending values each, interleaved sample by sample
    ks = np.tile(old, 190)
    vs = np.repeat(C.D(190), 6)
    kss.add(torch.from_numpy(ks), torch.from_numpy(vs))
    kss.flush(torch.from_numpy(old))
    assert kss.streams.num_promoted == (6 if gpu else 0)
    kss.remove(torch.from_numpy(old))
    new = np.arange(200, 206, dtype=np.int64)
    rng = np.random.default_rng(8)
    ks = new[rng.integers(0, 6, 300)]
    vs = np.round(rng.lognormal(0, 1, 300), 3)
    kss.add(torch.from_numpy(ks), torch.from_numpy(vs))
    assert sorted(kss.directory.lookup(torch.from_numpy(new)).cpu().tolist()) == list(range(6))  # the ids, recycled
    assert kss.streams.num_promoted == (6 if gpu else 0)  # removal reset the streams, their class stayed
    orc = {int(k): OracleGK(EPS) for k in new}
    for k, v in zip(ks, vs):
        orc[int(k)].add(float(v))
    before = R.snapshot(kss.streams)
    res = kss.compact()
    assert res["demoted"] == (6 if gpu else 0), res
    assert kss.streams.num_promoted == 0
    T.same_snapshot(kss.streams, before, "keyed churn")
    got = kss.quantiles(torch.from_numpy(new), R.QS).cpu().numpy()
    exp = np.asarray([orc[int(k)].quantiles(R.QS) for k in new], dtype=np.float64)
    U.assert_same_quantiles(got, exp, "keyed churn: quantiles by key", None)
    kss.close()


# ------------------------------------------------------------ case 9: arguments
def case_arguments(dev):
    from gkarray_amd import _lib as L
    ss, orc = C.make(dev, [(1, 150, 1141), (0, 0, 1142), ("D", 190, 0)])
    lib, h, sp = ss._lib, ss.handle, ss._sp()
    nclass = len(ss.class_usage())
    assert nclass == (1 if ss.is_cpu else 4)
    x = ctypes.c_int64(-7)
    null = None
    for cls in (-1, nclass):
        assert lib.gk_class_usage(h, cls, ctypes.byref(x), null, null, null, null, sp) == L.GK_E_ARG, cls
        assert x.value == -7
    assert lib.gk_class_usage(h, 0, null, null, null, null, null, sp) == L.GK_OK
    assert lib.gk_class_usage(h, 0, ctypes.byref(x), null, null, null, null, sp) == L.GK_OK and x.value == 3
    assert lib.gk_compact(h, null, null, sp) == L.GK_OK
    # a NULL set: what every call answers for one
    want = lib.gk_sync(None, sp)
    assert want == L.GK_E_ARG
    assert lib.gk_compact(None, ctypes.byref(x), null, sp) == want
    assert lib.gk_class_usage(None, 0, ctypes.byref(x), null, null, null, null, sp) == want
    C.assert_all(ss, orc, "after the argument checks")


def case_symbols():
    from gkarray_amd import _lib
    for name in ("gk_compact", "gk_class_usage"):
        assert name in _lib.SYMBOLS and name in _lib.CPU_SYMBOLS, name
        assert hasattr(_lib.load_cpu(), name), name
