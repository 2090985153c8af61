"""Cases of the group-by roll-up (gk_rollup / StreamSet.rollup_from /
rollup_by_key), shared by tests/test_gpu_rollup.py (device engine) and
tests/test_cpu_rollup.py (host engine); the engine is the ``dev`` parameter.

The expected state is the oracle's: one ``OracleGK`` per source and
destination stream, ``add_many``, then ``dst.merge(member)`` in member order
(gk:111-154).  Every destination stream, every member and every non-member is
compared bit for bit: table (v by bit pattern, g, delta), pending values,
n / min / max / sum / avg, then ``quantiles([0, .5, .9, .99, 1])``;
non-members also against a snapshot of ``src.export_state()`` taken before
the call.  Test infrastructure only."""
import copy
import functools
import struct

import numpy as np
import pytest
import torch

import parity_util as U
from gk_oracle import OracleGK

QS = [0.0, 0.5, 0.9, 0.99, 1.0]

# the 17-member group of the issue: lengths, distributions parity_util.gen(k % 8)
LENS17 = [1000, 0, 1, 100, 101, 102, 1500, 999, 202, 303, 1000, 1000, 50, 707, 1313, 1000, 1000]


def _bits(x):
    return struct.pack("<d", float(x))


def seq(dist, L, seed):
    return np.asarray(U.gen(dist, L, np.random.default_rng(seed)), dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _ingested(eps, dist, L, seed):
    o = OracleGK(eps)
    o.add_many(seq(dist, L, seed))
    return o


def oracle_of(eps, spec):
    """A fresh oracle stream holding spec = (dist, L, seed) (ingested once, then copied)."""
    return copy.deepcopy(_ingested(eps, *spec))


def make_set(dev, eps, specs):
    ss = U._ss(len(specs), eps, dev)
    U.ingest_np(ss, [seq(*sp) for sp in specs])
    return ss


def csr_of(groups):
    go = np.zeros(len(groups) + 1, np.int64)
    go[1:] = np.cumsum([len(g) for g in groups])
    mem = np.asarray([m for g in groups for m in g], dtype=np.int64)
    return torch.from_numpy(go), torch.from_numpy(mem)


def snapshot(ss):
    """export_state() as host arrays (no flush)."""
    return {k: (v.cpu().numpy().copy() if torch.is_tensor(v) else v) for k, v in ss.export_state().items()}


def stream_of_snapshot(st, s):
    a, b = int(st["offs"][s]), int(st["offs"][s + 1])
    c, e = int(st["poffs"][s]), int(st["poffs"][s + 1])
    return dict(v=[_bits(x) for x in st["v"][a:b]], g=[int(x) for x in st["g"][a:b]],
                d=[int(x) for x in st["d"][a:b]], pending=[_bits(x) for x in st["pv"][c:e]],
                n=int(st["n"][s]), min=_bits(st["min"][s]), max=_bits(st["max"][s]),
                sum=_bits(st["sum"][s]), avg=_bits(st["avg"][s]))


def stream_of_oracle(o):
    return dict(v=[_bits(x) for x in o.v], g=[int(x) for x in o.g], d=[int(x) for x in o.d],
                pending=[_bits(x) for x in o.pending], n=int(o.n), min=_bits(o.min), max=_bits(o.max),
                sum=_bits(o.sum), avg=_bits(o.avg))


def assert_stream(got, exp, what):
    for k in ("n", "min", "max", "sum", "avg", "pending", "g", "d", "v"):
        assert got[k] == exp[k], "%s: %s differs (table %d vs %d entries, pending %d vs %d)" % (
            what, k, len(got["v"]), len(exp["v"]), len(got["pending"]), len(exp["pending"]))


def assert_set_matches(ss, oracles, what):
    st = snapshot(ss)
    for s, o in enumerate(oracles):
        assert_stream(stream_of_snapshot(st, s), stream_of_oracle(o), "%s stream %d" % (what, s))


def assert_sets_equal(a, b, what):
    sa, sb = snapshot(a), snapshot(b)
    assert a.num_streams == b.num_streams
    for s in range(a.num_streams):
        assert_stream(stream_of_snapshot(sa, s), stream_of_snapshot(sb, s), "%s stream %d" % (what, s))


def assert_quantiles(ss, oracles, what):
    got = ss.quantiles(QS).cpu().numpy()
    exp = np.asarray([o.quantiles(QS) for o in oracles], dtype=np.float64).reshape(len(oracles), len(QS))
    U.assert_same_quantiles(got, exp, what + " quantiles", None)


def oracle_fold(dst_o, src_o, groups):
    """dst[j].merge(src[m]) in member order; returns the largest table any destination held on the way."""
    sizes = []
    for j, g in enumerate(groups):
        top = len(dst_o[j].v)
        for m in g:
            dst_o[j].merge(src_o[m])
            top = max(top, len(dst_o[j].v))
        sizes.append(top)
    return sizes


def check_rollup(dst, src, dst_o, src_o, groups, what, call=None, quantiles=True):
    """One roll-up of `groups` on the engine and on the oracle, then every comparison."""
    members = {m for g in groups for m in g}
    before = snapshot(src)
    if call is None:
        go, mem = csr_of(groups)
        dst.rollup_from(src, go, mem)
    else:
        call()
    tops = oracle_fold(dst_o, src_o, groups)
    assert_set_matches(dst, dst_o, what + " dst")
    after = snapshot(src)
    for s, o in enumerate(src_o):
        got = stream_of_snapshot(after, s)
        role = "member" if s in members else "non-member"
        assert_stream(got, stream_of_oracle(o), "%s src %d (%s)" % (what, s, role))
        if s not in members:
            assert_stream(got, stream_of_snapshot(before, s),
                          "%s non-member %d vs its state before the call" % (what, s))
    if quantiles:  # (they flush the pending values: state comparisons come first)
        assert_quantiles(dst, dst_o, what + " dst")
        assert_quantiles(src, src_o, what + " src")
    return tops


# ---------------------------------------------------------------- case 1 data
def mixed_specs():
    """Source streams (dist, L, seed) and groups of case 1."""
    specs = [(k % 8, L, 100 + k) for k, L in enumerate(LENS17)]           # 0..16: the 17-member group
    specs += [(1, 450, 200)]                                               # 17: group of 1
    specs += [(2, 1000, 201), (0, 57, 202)]                                # 18, 19: group of 2 (taken as 19, 18)
    specs += [(3, 300, 203), (0, 0, 204), (7, 1212, 205), (5, 99, 206), (6, 101, 207)]  # 20..24: group of 5
    specs += [(0, 0, 208), (0, 0, 209), (1, 640, 210)]                     # 25..27: two empty members first
    specs += [(0, 0, 211), (0, 0, 212)]                                    # 28, 29: only empty members
    specs += [(0, 57, 213), (1, 157, 214), (2, 1033, 215), (5, 5, 216), (6, 250, 217), (7, 99, 218)]  # non-members
    groups = [list(range(17)), [], [17], [19, 18], [20, 21, 22, 23, 24], [25, 26, 27], [28, 29]]
    return specs, groups


# destination lengths of the pre-ingested run: 0, 57 (pending only) and 1000;
# the empty group's destination holds pending values that must stay pending
DST_LENS = [1000, 57, 57, 0, 1000, 0, 57]


def case_mixed(dev, pre):
    eps = 0.01
    specs, groups = mixed_specs()
    dspecs = [(s % 8, DST_LENS[s] if pre else 0, 300 + s) for s in range(len(groups))]
    src, dst = make_set(dev, eps, specs), make_set(dev, eps, dspecs)
    src_o = [oracle_of(eps, sp) for sp in specs]
    dst_o = [oracle_of(eps, sp) for sp in dspecs]
    assert sum(1 for s in range(30, 36) if src_o[s].pending) >= 5
    # (pre: the empty group's destination holds 57 pending values; the oracle's
    # copy is never merged, so the comparison below requires them still pending)
    assert len(dst_o[1].pending) == (57 if pre else 0)
    tops = check_rollup(dst, src, dst_o, src_o, groups, "mixed pre=%s" % pre)
    # the 17-member fold crosses the 128-entry class (and, into a fresh
    # destination, comes back below it)
    assert tops[0] > 128 and (pre or len(dst_o[0].v) < 128), (tops, len(dst_o[0].v))
    return tops


def case_small_eps(dev):
    eps = 0.001
    lens = [5000, 4000, 0, 5003, 1001, 2500]
    specs = [(SMALL_EPS_DISTS[k], L, 400 + k) for k, L in enumerate(lens)]
    specs += [(0, 300, 410), (1, 1500, 411), (2, 2002, 412), (7, 700, 413)]
    groups = [list(range(6)), [6, 7], [8]]
    dspecs = [(0, 0, 420), (3, 1500, 421), (0, 0, 422)]
    src, dst = make_set(dev, eps, specs), make_set(dev, eps, dspecs)
    src_o = [oracle_of(eps, sp) for sp in specs]
    dst_o = [oracle_of(eps, sp) for sp in dspecs]
    tops = check_rollup(dst, src, dst_o, src_o, groups, "eps=0.001")
    assert tops[0] > 2048, tops  # beyond the largest on-chip class
    return tops


SMALL_EPS_DISTS = [3, 4, 0, 3, 1, 4]


def case_narrow_ladder(dev):
    """(GK_CAPS=128,256,512,4096 set by the caller) the 17-member group climbs two levels in one call."""
    eps = 0.01
    specs, groups = mixed_specs()
    specs, groups = specs[:17] + specs[30:33], [groups[0], []]  # (streams 17..19: non-members)
    dspecs = [(0, 0, 300), (1, 57, 301)]
    src, dst = make_set(dev, eps, specs), make_set(dev, eps, dspecs)
    assert dst.capacity(1) == 256 and dst.capacity(2) == 512
    src_o = [oracle_of(eps, sp) for sp in specs]
    dst_o = [oracle_of(eps, sp) for sp in dspecs]
    tops = check_rollup(dst, src, dst_o, src_o, groups, "narrow ladder")
    assert tops[0] > 256, tops
    return tops


def case_merge_ladder(dev):
    """(GK_CAPS=128,256,512,4096 set by the caller) the other two folds of the
    capacity-level ladder, each with a class-0 stream that climbs inside the
    call beside one that stays below 128 entries: merge_from (stream 0, a
    descending run of 190 values -- 51 entries and 89 pending values -- takes
    150 lognormal values from the source) and merge_compress(entries) (stream
    0 takes 300 records that its threshold of 1 keeps apart)."""
    eps = 0.01
    # (dist 3: a descending run, whose entries carry deltas that no later threshold removes)
    sspecs, dspecs = [(1, 150, 831), (0, 57, 832), (0, 0, 833)], [(3, 190, 834), (2, 250, 835), (5, 101, 836)]
    src, dst = make_set(dev, eps, sspecs), make_set(dev, eps, dspecs)
    if dev != "cpu":
        assert dst.capacity(1) == 256 and dst.capacity(2) == 512
    src_o = [oracle_of(eps, sp) for sp in sspecs]
    dst_o = [oracle_of(eps, sp) for sp in dspecs]
    assert all(len(o.v) < 128 for o in dst_o)  # (every destination stream starts in class 0)
    dst.merge_from([src])
    for o, m in zip(dst_o, src_o):
        o.merge(m)
    assert len(dst_o[0].v) > 128 > len(dst_o[1].v) > 0, [len(o.v) for o in dst_o]
    assert_set_matches(dst, dst_o, "merge ladder dst")
    assert_set_matches(src, src_o, "merge ladder src")
    # merge_compress(entries): n = 57 gives the threshold floor(2 eps (n - 1)) = 1, no two records combine
    mspecs = [(1, 57, 837), (0, 57, 838), (5, 101, 836)]
    mc, mc_o = make_set(dev, eps, mspecs), [oracle_of(eps, sp) for sp in mspecs]
    recs = [[(0.5 + k, 1, 1) for k in range(300)], [(2.5, 1, 0), (7.0, 2, 1)], []]
    flat = [r for rs in recs for r in rs]
    offs = np.concatenate([[0], np.cumsum([len(rs) for rs in recs])])
    mc.merge_compress(torch.tensor([r[0] for r in flat], dtype=torch.float64),
                      torch.tensor([r[1] for r in flat], dtype=torch.int32),
                      torch.tensor([r[2] for r in flat], dtype=torch.int32), torch.from_numpy(offs.astype(np.int64)))
    for o, rs in zip(mc_o, recs):
        o.flush(rs)
    assert len(mc_o[0].v) > 128 > len(mc_o[1].v) > 0, [len(o.v) for o in mc_o]
    assert_set_matches(mc, mc_o, "merge_compress ladder")
    if dev != "cpu":
        assert dst.num_promoted >= 1 and mc.num_promoted >= 1
    assert_quantiles(dst, dst_o, "merge ladder dst")
    assert_quantiles(mc, mc_o, "merge_compress ladder")


def case_merge_overflow(dev):
    """(GK_CAPS=128,200 set by the caller: the last class holds 199 entries)
    GK_E_OVERFLOW of merge_from and of merge_compress(entries): the stream that
    did not fit keeps its state from before the call -- table, pending values,
    n, min, max, sum, avg -- the other stream is complete, the source flushed.
    Stream 0 of merge_from: 51 entries and 89 pending values take a source that
    flushes to 138 entries (it fits); the merge would have 221.  The source's
    min lies below the destination's and its max above, so a header written
    before the overflow is known would show."""
    from gkarray_amd._lib import GK_E_OVERFLOW, GKBackendError
    eps = 0.01
    sspecs, dspecs = [(3, 190, 840), (0, 57, 832)], [(3, 190, 834), (2, 250, 835)]
    src, dst = make_set(dev, eps, sspecs), make_set(dev, eps, dspecs)
    assert dst.capacity(1) == 200 and dst.capacity(2) == -1
    limit = dst.capacity(1) - 1  # (one slot of a class is padding)
    src_o = [oracle_of(eps, sp) for sp in sspecs]
    dst_o = [oracle_of(eps, sp) for sp in dspecs]
    assert [(len(o.v), len(o.pending)) for o in dst_o] == [(51, 89), (94, 48)]
    assert src_o[0].min < dst_o[0].min and src_o[0].max > dst_o[0].max
    merged = copy.deepcopy((dst_o, src_o))
    for o, m in zip(*merged):
        o.merge(m)  # (flushes m, gk:126 / gk:137)
    assert [len(o.v) for o in merged[1]] == [138, 57] and [len(o.v) for o in merged[0]] == [221, 123]
    assert 138 <= limit < 221
    before = snapshot(dst)
    with pytest.raises(GKBackendError) as ei:
        dst.merge_from([src])
    assert ei.value.code == GK_E_OVERFLOW, ei.value
    after = snapshot(dst)
    assert_stream(stream_of_snapshot(after, 0), stream_of_snapshot(before, 0),
                  "merge_from overflow: dst 0 vs its state before the call")
    assert_stream(stream_of_snapshot(after, 0), stream_of_oracle(dst_o[0]), "merge_from overflow: dst 0")
    assert_stream(stream_of_snapshot(after, 1), stream_of_oracle(merged[0][1]), "merge_from overflow: dst 1")
    assert_set_matches(src, merged[1], "merge_from overflow: src")
    # merge_compress(entries): 150 records fit the carve (at most cap + 1), so
    # it is the walk's output of 207 entries that does not fit
    mspecs = [(1, 57, 837), (0, 57, 838)]
    mc, mc_o = make_set(dev, eps, mspecs), [oracle_of(eps, sp) for sp in mspecs]
    recs = [[(0.5 + k, 1, 1) for k in range(150)], [(2.5, 1, 0), (7.0, 2, 1)]]
    flat = [r for rs in recs for r in rs]
    offs = np.concatenate([[0], np.cumsum([len(rs) for rs in recs])])
    flushed = copy.deepcopy(mc_o)
    for o, rs in zip(flushed, recs):
        o.flush(rs)
    assert len(flushed[0].v) == 207 > limit and len(recs[0]) <= limit + 2, len(flushed[0].v)
    before = snapshot(mc)
    with pytest.raises(GKBackendError) as ei:
        mc.merge_compress(torch.tensor([r[0] for r in flat], dtype=torch.float64),
                          torch.tensor([r[1] for r in flat], dtype=torch.int32),
                          torch.tensor([r[2] for r in flat], dtype=torch.int32), torch.from_numpy(offs.astype(np.int64)))
    assert ei.value.code == GK_E_OVERFLOW, ei.value
    after = snapshot(mc)
    assert_stream(stream_of_snapshot(after, 0), stream_of_snapshot(before, 0),
                  "merge_compress overflow: stream 0 vs its state before the call")
    assert_stream(stream_of_snapshot(after, 0), stream_of_oracle(mc_o[0]), "merge_compress overflow: stream 0")
    assert_stream(stream_of_snapshot(after, 1), stream_of_oracle(flushed[1]), "merge_compress overflow: stream 1")


def case_equivalence(dev):
    """keys = s % G: round r's members are the source slice [rG, (r+1)G); the
    same tables as one set per slice, folded by merge_from, give the same bits."""
    eps, G, R = 0.01, 8, 6
    rng = np.random.default_rng(77)
    lens = rng.integers(0, 1201, G * R)
    lens[[3, 20]] = 0
    lens[5] = 1200
    specs = [(int(s % 8), int(lens[s]), 500 + s) for s in range(G * R)]
    src = make_set(dev, eps, specs)
    st = src.export_state()
    sets = []
    for r in range(R):
        lo, hi = r * G, (r + 1) * G
        ss = U._ss(G, eps, dev)
        pv = st["pv"] if st["pv"].numel() else torch.zeros(1, dtype=torch.float64, device=st["pv"].device)
        ss.import_arrays(st["offs"][lo:hi + 1].contiguous(), st["v"], st["g"], st["d"],
                         st["poffs"][lo:hi + 1].contiguous(), pv, st["n"][lo:hi].contiguous(),
                         st["min"][lo:hi].contiguous(), st["max"][lo:hi].contiguous(),
                         st["sum"][lo:hi].contiguous(), st["avg"][lo:hi].contiguous())
        sets.append(ss)
    dst, dst2 = U._ss(G, eps, dev), U._ss(G, eps, dev)
    dst.rollup_by_key(src, torch.arange(G * R, dtype=torch.int64) % G)
    dst2.merge_from(sets)
    assert_sets_equal(dst, dst2, "rollup_by_key vs merge_from")
    # (every source stream is a member here: also against the oracle's loop)
    src_o = [oracle_of(eps, sp) for sp in specs]
    dst_o = [OracleGK(eps) for _ in range(G)]
    oracle_fold(dst_o, src_o, [list(range(j, G * R, G)) for j in range(G)])
    assert_set_matches(dst, dst_o, "every stream a member: dst")
    assert_set_matches(src, src_o, "every stream a member: src")
    for r in range(R):  # the members were flushed exactly as merge_from flushes its sources
        sr = snapshot(sets[r])
        ssrc = snapshot(src)
        for i in range(G):
            assert_stream(stream_of_snapshot(ssrc, r * G + i), stream_of_snapshot(sr, i), "member %d" % (r * G + i))
    q1, q2 = dst.quantiles(QS).cpu().numpy(), dst2.quantiles(QS).cpu().numpy()
    U.assert_same_quantiles(q1, q2, "rollup_by_key vs merge_from quantiles", None)


def case_by_key_order(dev):
    """Permuted keys with -1: the same result as rollup_from with hand-built CSR
    (members of a group in ascending source index), and as the oracle."""
    eps, G = 0.01, 4
    keys = [2, -1, 0, 3, 0, -1, 2, 2, 0, 3, -1, 2]
    groups = [[2, 4, 8], [], [0, 6, 7, 11], [3, 9]]
    specs = [(s % 8, [640, 57, 0, 1000, 333, 99, 101, 250, 1, 777, 1200, 480][s], 600 + s) for s in range(len(keys))]
    dspecs = [(1, 57, 620), (2, 57, 621), (0, 0, 622), (3, 300, 623)]
    a_src, a_dst = make_set(dev, eps, specs), make_set(dev, eps, dspecs)
    b_src, b_dst = make_set(dev, eps, specs), make_set(dev, eps, dspecs)
    src_o = [oracle_of(eps, sp) for sp in specs]
    dst_o = [oracle_of(eps, sp) for sp in dspecs]
    check_rollup(a_dst, a_src, dst_o, src_o, groups, "by key",
                 call=lambda: a_dst.rollup_by_key(a_src, torch.tensor(keys, dtype=torch.int64)), quantiles=False)
    go, mem = csr_of(groups)
    b_dst.rollup_from(b_src, go, mem)
    assert_sets_equal(a_dst, b_dst, "rollup_by_key vs hand-built CSR")
    assert_sets_equal(a_src, b_src, "rollup_by_key vs hand-built CSR, sources")
    assert_quantiles(a_dst, dst_o, "by key dst")
    assert_quantiles(a_src, src_o, "by key src")
    with pytest.raises(ValueError):
        a_dst.rollup_by_key(a_src, torch.tensor([G] + keys[1:], dtype=torch.int64))
    with pytest.raises(ValueError):
        a_dst.rollup_by_key(a_src, torch.tensor(keys[:-1], dtype=torch.int64))


def case_errors(dev):
    from gkarray_amd import UnequalEpsilonException
    from gkarray_amd._lib import GK_E_ARG, GKBackendError
    eps = 0.01
    specs = [(s % 8, [640, 57, 0, 1000, 333, 1099][s], 700 + s) for s in range(6)]
    dspecs = [(1, 57, 720), (2, 1000, 721), (0, 0, 722)]
    src, dst = make_set(dev, eps, specs), make_set(dev, eps, dspecs)
    other_eps = make_set(dev, 0.02, specs)
    S = len(specs)
    i64 = lambda x: torch.tensor(x, dtype=torch.int64)  # noqa: E731
    bad = [
        ("duplicate member", lambda: dst.rollup_from(src, i64([0, 2, 3, 4]), i64([0, 1, 2, 0])), GKBackendError),
        ("member == S", lambda: dst.rollup_from(src, i64([0, 2, 3, 4]), i64([0, 1, 2, S])), GKBackendError),
        ("member == -1", lambda: dst.rollup_from(src, i64([0, 2, 3, 4]), i64([0, -1, 2, 3])), GKBackendError),
        ("dst is src", lambda: dst.rollup_from(dst, i64([0, 1, 1, 1]), i64([1])), GKBackendError),
        ("eps mismatch", lambda: dst.rollup_from(other_eps, i64([0, 2, 3, 4]), i64([0, 1, 2, 3])),
         UnequalEpsilonException),
        ("offsets of the wrong length", lambda: dst.rollup_from(src, i64([0, 2, 3]), i64([0, 1, 2])), ValueError),
        ("decreasing offsets", lambda: dst.rollup_from(src, i64([0, 3, 2, 4]), i64([0, 1, 2, 3])), GKBackendError),
        ("offsets not starting at 0", lambda: dst.rollup_from(src, i64([1, 2, 3, 4]), i64([0, 1, 2, 3])),
         GKBackendError),
    ]
    for what, call, exc in bad:
        b_dst, b_src = snapshot(dst), snapshot(src)
        with pytest.raises(exc) as ei:
            call()
        if exc is GKBackendError:
            assert ei.value.code == GK_E_ARG, (what, ei.value)
        for ss, st0, name in ((dst, b_dst, "dst"), (src, b_src, "src")):
            st1 = snapshot(ss)
            for s in range(ss.num_streams):
                assert_stream(stream_of_snapshot(st1, s), stream_of_snapshot(st0, s),
                              "after '%s': %s stream %d" % (what, name, s))
    src_o = [oracle_of(eps, sp) for sp in specs]
    dst_o = [oracle_of(eps, sp) for sp in dspecs]
    check_rollup(dst, src, dst_o, src_o, [[4, 0], [], [2, 5, 3]], "valid roll-up after the errors")


def case_repeat(dev):
    """A second rollup_from on the same dst with other members continues the fold."""
    eps = 0.01
    specs, _ = mixed_specs()
    specs = specs[:17]
    first = [[0, 1, 2, 3], [4], []]
    second = [[6, 5, 7, 9, 10, 11], [], [12, 13, 14]]
    dspecs = [(0, 0, 800), (1, 57, 801), (2, 1000, 802)]
    src, dst = make_set(dev, eps, specs), make_set(dev, eps, dspecs)
    src_o = [oracle_of(eps, sp) for sp in specs]
    dst_o = [oracle_of(eps, sp) for sp in dspecs]
    check_rollup(dst, src, dst_o, src_o, first, "first call")
    tops = check_rollup(dst, src, dst_o, src_o, second, "second call")
    assert tops[0] > 128, tops  # (the continued fold is promoted in the second call)


def case_overflow(dev, member):
    """GK_E_OVERFLOW and the state gk_capi.h documents for it (the caller sets
    the ladder).  member=False (GK_CAPS=128,264): the 17-member fold outgrows
    the last class -- every member flushed, the destination holding the fold of
    the members before the one that did not fit, the other destinations
    complete.  member=True (GK_CAPS=128,256): member 11's own flush does not fit
    the last class (256 entries; a class holds one less) -- it keeps its state,
    the other members are flushed, no destination is touched."""
    from gkarray_amd._lib import GK_E_OVERFLOW, GKBackendError
    eps = 0.01
    specs, groups = mixed_specs()
    specs, groups = specs[:20], [groups[0], [17], []]  # (streams 18, 19: non-members)
    dspecs = [(0, 0, 300), (1, 57, 301), (2, 57, 302)]
    src, dst = make_set(dev, eps, specs), make_set(dev, eps, dspecs)
    assert dst.capacity(2) == -1
    limit = dst.capacity(1) - 1  # (one slot of a class is padding)
    src_o = [oracle_of(eps, sp) for sp in specs]
    dst_o = [oracle_of(eps, sp) for sp in dspecs]
    flushed = copy.deepcopy(src_o)
    for o in flushed:
        if o.n:
            o.flush()
    too_big = [m for m in groups[0] + groups[1] if len(flushed[m].v) > limit]
    if member:
        assert too_big == [11], too_big
        for m in groups[0] + groups[1]:
            if m != 11:
                src_o[m] = flushed[m]
    else:
        assert not too_big, too_big
        # the oracle's fold stops before the first member whose merge leaves
        # more entries than the last class holds
        stop = None
        for k, m in enumerate(groups[0]):
            trial = copy.deepcopy((dst_o[0], src_o[m]))
            trial[0].merge(trial[1])
            if len(trial[0].v) > limit:
                stop = k
                break
            dst_o[0], src_o[m] = trial
        assert stop is not None and stop > 0
        for m in groups[0][stop:]:  # flushed before the fold (gk:126 / gk:137), then not merged
            src_o[m] = flushed[m]
        dst_o[1].merge(src_o[17])
    go, mem = csr_of(groups)
    with pytest.raises(GKBackendError) as ei:
        dst.rollup_from(src, go, mem)
    assert ei.value.code == GK_E_OVERFLOW, ei.value
    assert_set_matches(dst, dst_o, "after GK_E_OVERFLOW: dst")
    assert_set_matches(src, src_o, "after GK_E_OVERFLOW: src")


def case_merge_source_with_records_below_min(dev):
    """Found by the random sequences of opseq_cases (moves through the host
    engine, eps = 0.01, seed 1004, step 10): merge_compress(entries) gave a
    source stream records below its _min, so that its table starts below
    other._min and the converted list (other._min, ...), (v_0, ...), ... of
    gk:136-147 is not sorted as it stands; gk:72 sorts it.  Sources: a 1-value
    stream with 11 records around its value (the sequence's own), one with 70
    records below _min (more than a wave of records move), one with records
    equal to _min (the sort is stable: _min's record stays ahead of them), and
    an untouched one.  Both folds: merge_from and rollup_from."""
    eps = 0.01
    for fold in ("merge", "rollup"):
        src_vals = [np.asarray([1.3505]), np.asarray([100.0, 101.0]), np.asarray([5.0, 6.0, 7.0]), seq(1, 150, 861)]
        recs = [[(0.2489, 1, 1), (0.9105, 3, 5), (1.0683, 4, 2), (1.3505, 4, 5), (1.3505, 3, 3), (1.3505, 2, 0),
                 (1.3505, 1, 5), (1.3505, 3, 0), (1.4288, 3, 5), (1.5422, 4, 1), (1.5982, 2, 0)],
                [(float(k), 1 + k % 3, k % 4) for k in range(70)],
                [(5.0, 2, 1), (5.0, 1, 3), (5.5, 2, 0)],
                []]
        dspecs = [(7, 10, 862), (1, 57, 863), (0, 0, 864), (2, 250, 865)]
        src = U._ss(len(src_vals), eps, dev)
        U.ingest_np(src, src_vals)
        src_o = []
        for x in src_vals:
            o = OracleGK(eps)
            o.add_many(x)
            src_o.append(o)
        flat = [r for rs in recs for r in rs]
        offs = np.concatenate([[0], np.cumsum([len(rs) for rs in recs])]).astype(np.int64)
        src.merge_compress(torch.tensor([r[0] for r in flat], dtype=torch.float64),
                           torch.tensor([r[1] for r in flat], dtype=torch.int32),
                           torch.tensor([r[2] for r in flat], dtype=torch.int32), torch.from_numpy(offs))
        for o, rs in zip(src_o, recs):
            o.flush(rs)
        assert all(o.v[0] < o.min for o in src_o[:2]) and src_o[2].v[0] == src_o[2].min
        assert_set_matches(src, src_o, "records below _min: src")
        dst = make_set(dev, eps, dspecs)
        dst_o = [oracle_of(eps, sp) for sp in dspecs]
        groups = [[0], [1], [2], [3]]
        if fold == "merge":
            dst.merge_from([src])
            oracle_fold(dst_o, src_o, groups)
            assert_set_matches(dst, dst_o, "records below _min, merge_from: dst")
            assert_set_matches(src, src_o, "records below _min, merge_from: src")
        else:
            check_rollup(dst, src, dst_o, src_o, [[1, 0], [2], [], [3]], "records below _min, rollup", quantiles=False)
        assert all(dst_o[j].v == sorted(dst_o[j].v) for j in range(4))
        assert_quantiles(dst, dst_o, "records below _min, %s" % fold)
