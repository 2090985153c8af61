"""Random operation sequences on a few StreamSets against one ``OracleGK`` per
stream, shared by tests/test_gpu_opseq.py (device engine) and
tests/test_cpu_opseq.py (host engine); the engine is the ``dev`` parameter.

``run_sequence`` draws ``nops`` operations from a generator seeded by
``(eps, seed)`` alone -- no choice depends on the engine's answers, on hash
order or on time -- applies each to the sets and to the model, and compares
after EVERY operation: every stream of every set with its oracle (table v by
bit pattern, g, delta, pending values, n / min / max / sum / avg by bit
pattern; ``select_cases.assert_all``), every stream the operation must not
touch also with the ``export_state()`` snapshot from before the call, and every
answer strictly (``unpinned=None``).  The one exception is an ``ingest``,
``ingest_keyed`` or ``rank_ingest_keyed`` left in flight (``sync=False``):
nothing is read after it, its rank rows and fused answers wait, the next operation goes to
the same set without a ``sync()`` or a snapshot, and the comparison after THAT
operation covers both.  The driver checks that the first C ABI call the set
then sees is that operation's own (``FIRST_CALL``): it is the call that
settles the deferred streams.

The model side restates nothing: the rules are those of select_cases,
rank_cases, rollup_cases, transfer_cases, rankkeyed_cases, rankingest_cases,
keyed_cases and compact_cases (``check_query``, ``check_ranks``,
``check_rollup``, ``oracle_fold``, ``copy.deepcopy`` for moved streams,
``expected_rows``, ``oracle_step``, ``oracle_loop``, ``compact_checked``,
``check_usage``).

Where a stream lives is modelled by a lower bound only, ``floor[set][stream]``
(``Sequence.update_floors``): the class a stream has reached and cannot have
left.  A compaction must bring every stream to exactly ``fit`` of its table and
count every stream whose floor lay above it (``compact_with_floors``); after
every operation no class may hold fewer streams than the floors put at or above
it (``usage_above_floors``).

The event counters are counted on the model only, so the host-engine test can
require them for exactly the sequences the device test runs.  "Large" is an
oracle table longer than class 0's capacity on the device's ladder.

``model_fault`` makes the MODEL wrong in one small way (tests/test_cpu_opseq.py
requires that every such fault is noticed).  Test infrastructure only."""
import collections
import copy
import os
import tempfile

import numpy as np
import pytest
import torch

import compact_cases as CC
import keyed_cases as KC
import parity_util as U
import rank_cases as K
import rankingest_cases as RI
import rankkeyed_cases as Q
import rollup_cases as R
import select_cases as C
from gk_oracle import OracleGK, flush_period

ALL = "all"

# operation kinds and their weights in the draw (reset() of a whole set is kept rare, so that histories
# grow long: once per sequence, at a step drawn with the seed, and in its turn after an ingest left in flight)
WEIGHTS = collections.OrderedDict([
    ("ingest", 22.0), ("ingest_keyed", 8.0), ("flush_select", 5.0), ("reset_select", 4.0),
    ("quantiles_select", 5.0), ("stats_select", 2.5), ("ranks", 2.5), ("ranks_select", 4.0), ("cdf_select", 2.5),
    ("flush", 3.0), ("quantiles", 3.0), ("reset", 0.0), ("merge_from", 6.0), ("rollup_from", 5.0),
    ("rollup_by_key", 3.0), ("merge_compress", 4.0), ("take_put", 7.0), ("pack_unpack", 5.0), ("resized", 2.5),
    ("roundtrip_state", 2.0), ("roundtrip_file", 2.0), ("roundtrip_pack", 2.0), ("void", 4.0),
    ("compact", 6.0), ("ranks_keyed", 4.0), ("cdf_keyed", 2.5), ("rank_ingest_keyed", 8.0)])
KINDS = list(WEIGHTS)
READ_ONLY = {"stats_select", "void", "compact"}  # (a compaction changes where streams live, not what the model holds)
STATE_CHANGING = [k for k in KINDS if k not in READ_ONLY and not k.startswith("roundtrip")]

VOID_CALLS = ["select_id_S", "unpack_duplicate", "nan_q", "nan_threshold", "merge_other_eps", "keyed_id_S"]

# model faults: the named ones, and "drop:<kind>", which forgets the effect
# of an operation of that kind on one stream it changed
NAMED_FAULTS = {
    "flush_select_skips_one": "flush_select", "merge_source_not_flushed": "merge_from",
    "reset_one_too_few": "reset_select", "put_sorted_order": "take_put",
    "rollup_ascending_members": "rollup_from", "ingest_query_no_flush": "ingest",
    "rank_ingest_ranks_after_add": "rank_ingest_keyed", "ranks_keyed_no_flush": "ranks_keyed",
    "rank_ingest_adds_negative_rows": "rank_ingest_keyed"}
# and "drop_after_async:<kind>", the same only where the operation directly
# follows an ingest left in flight
AFTER_ASYNC_FAULTS = ["drop_after_async:" + k for k in ("quantiles_select", "ranks", "ranks_select", "flush_select",
                                                        "merge_from", "ranks_keyed", "cdf_keyed", "rank_ingest_keyed")]
FAULTS = sorted(NAMED_FAULTS) + ["drop:" + k for k in STATE_CHANGING] + AFTER_ASYNC_FAULTS
REPLACED = "fold_replaced_by_reset"  # counter key of a fold that guard_fold replaced

# The C ABI call that a set must see FIRST when an operation directly follows
# its ingest left in flight: the operation's own, so that it is this call that
# settles the deferred streams (checked on both engines, see Sequence.step).
FIRST_CALL = {
    "ingest": {"gk_ingest", "gk_ingest_quantiles"}, "ingest_keyed": {"gk_ingest_keyed"},
    "flush_select": {"gk_flush_select"}, "reset_select": {"gk_reset_select"},
    "quantiles_select": {"gk_quantiles_select"}, "stats_select": {"gk_stats_select"}, "ranks": {"gk_ranks"},
    "ranks_select": {"gk_ranks_select"}, "cdf_select": {"gk_ranks_select"}, "flush": {"gk_flush"},
    "quantiles": {"gk_quantiles"}, "reset": {"gk_reset"}, "merge_from": {"gk_merge"}, "rollup_from": {"gk_rollup"},
    "rollup_by_key": {"gk_rollup"}, "merge_compress": {"gk_merge_compress"},
    "take_put": {"gk_pack_select_bytes"}, "pack_unpack": {"gk_pack_select_bytes"},
    "resized": {"gk_pack_select_bytes"}, "roundtrip_state": {"gk_export_sizes"}, "roundtrip_file": {"gk_save"},
    "roundtrip_pack": {"gk_pack_bytes"}, "compact": {"gk_compact"}, "ranks_keyed": {"gk_ranks_keyed"},
    "cdf_keyed": {"gk_ranks_keyed"}, "rank_ingest_keyed": {"gk_rank_ingest_keyed"},
    "void": {"gk_quantiles_select", "gk_flush_select", "gk_reset_select", "gk_stats_select", "gk_ranks_select",
             "gk_pack_select_bytes", "gk_quantiles", "gk_ranks", "gk_ingest_keyed"},
    REPLACED: {"gk_reset_select"}}


class _Recorder:
    """Stands in for a set's library handle and notes the names of the calls made through it."""

    def __init__(self, lib):
        self.lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self.lib, name)

EVENTS = ["reset_large", "ingest_after_reset_large", "move_large_onto_small", "move_small_onto_large",
          "keyed_into_large", "fold_dst_large", "fold_member_large_dst_small", "flush_pending_P_minus_1",
          "flush_pending_1", "compact_demotes", "compact_with_pending", "compact_empties_class",
          "promoted_again_after_compact", "fold_dst_large_after_compact", "move_after_compact",
          "keyed_rank_of_large", "rank_ingest_into_large", "rank_ingest_flush_inside_run",
          "rank_ingest_new_values_only_negative"]
# the calls that can be left in flight (sync=False); every kind follows each of them
ASYNC_SOURCES = ["ingest", "ingest_keyed", "rank_ingest_keyed"]

MAX_N = 1 << 24  # (the engines hold g and delta in int32; self-merges double n)


def class0_capacity(eps):
    """Class 0 of the device's default ladder (gk_create): the 128-entry class
    while a flush period fits two values per lane, else 2048.  The short ladder
    of the tests starts at 128 as well."""
    return 128 if flush_period(eps) <= 128 else 2048


def ladder(eps, caps=None):
    """The capacities of the device's classes as the model holds them: `caps`
    in the spelling of GK_CAPS, else the default ladder of gk_create for a
    flush period of at most 1024."""
    if caps is not None:
        return [int(c.rstrip("b")) for c in caps.split(",")]
    return [128, 2048, 32768, 1 << 20] if flush_period(eps) <= 128 else [2048, 32768, 1 << 20]


def fit(E, caps):
    """The smallest class that holds a table of E entries: E <= cap[t] - 1
    (DESIGN.md "k_compact": a class keeps one entry free)."""
    for t, cap in enumerate(caps):
        if E <= cap - 1:
            return t
    raise ValueError("%d entries fit no class of %r" % (E, caps))


def _fp(o):
    return (o.n, tuple(o.v), tuple(o.g), tuple(o.d), tuple(o.pending))


def _short(x):
    x = [int(i) for i in x]
    return x if len(x) <= 48 else x[:48] + ["... %d in all" % len(x)]


def compact_with_floors(ss, oracles, floor, caps, what, settles=False, again=False):
    """compact() of `ss`, whose stream s the model holds as oracles[s], in a class
    of at least floor[s] on the ladder `caps`.  With `settles` (an ingest is in
    flight) the bare call comes first, as the call that settles, and the checks
    after it; else compact_cases.compact_checked.  On the device engine the
    classes afterwards are predicted exactly -- class after = min(class before,
    fit(E)), and a stream always fits its class: fit(E) -- and every stream
    whose floor lies above its fit must be counted in `demoted`.  With `again`
    a second compaction follows, which finds nothing to do.  Returns the
    first call's result."""
    fits = [fit(len(o.v), caps) for o in oracles]
    down = sum(1 for f, t in zip(floor, fits) if f > t)
    if settles:
        res = ss.compact()
        assert sorted(res) == ["bytes_freed", "demoted"], what
        use = CC.check_usage(ss, what)
        assert all(u["slots_used"] == u["streams"] for u in use[1:]), (what, use)
    else:
        res = CC.compact_checked(ss, oracles, what)
    if not ss.is_cpu:
        assert CC.per_class(ss) == [fits.count(c) for c in range(len(caps))], (what, fits)
        assert ss.num_promoted == sum(1 for f in fits if f > 0), what
        assert res["demoted"] >= down, (what, res, down)
    if again:
        use = ss.class_usage()
        assert CC.compact_checked(ss, oracles, what + ", again") == CC.ZERO, what
        assert ss.class_usage() == use, what
    return res


def usage_above_floors(ss, floor, caps, what):
    """class_usage() of `ss`: its invariants, and no stream below its floor -- for every class c at least as
    many streams in the classes >= c as the model holds there."""
    use = CC.check_usage(ss, what)
    if ss.is_cpu:
        return
    assert len(use) == len(caps), (what, use)
    for c in range(len(use)):
        at_least = sum(1 for f in floor if f >= c)
        got = sum(u["streams"] for u in use[c:])
        assert got >= at_least, "%s: %d streams in classes >= %d, the model holds %d there" % (what, got, c, at_least)


class Sequence:
    def __init__(self, dev, eps, seed, nops, sizes, async_ingest, via_host, stop_after, model_fault, caps=None,
                 weights=None):
        from gkarray_amd import StreamSet
        self.StreamSet = StreamSet
        self.dev, self.eps, self.seed, self.nops = dev, eps, seed, nops
        self.async_ingest, self.via_host = async_ingest, via_host
        self.caps = ladder(eps, caps)
        w = dict(WEIGHTS, **(weights or {}))
        assert set(w) == set(KINDS), sorted(set(w) - set(KINDS))
        self.weights = np.asarray([w[x] for x in KINDS])
        self.steps = nops if stop_after is None else min(nops, stop_after)
        assert model_fault is None or model_fault in FAULTS, model_fault
        self.fault = model_fault
        self.P = flush_period(eps)
        self.cap0 = class0_capacity(eps)
        # tables stay well inside the last class of every ladder the tests use
        self.limit = 3000 if self.cap0 == 128 else 8000
        # descending runs, in flush periods: short ones, long ones, and the table entries a long one can add
        self.run_units = (20, 321) if self.cap0 == 128 else (8, 25)
        self.run_growth = 700 if self.cap0 == 128 else 4000
        self.rng = np.random.default_rng([int(seed), self.P])
        self.reset_step = int(self.rng.integers(nops // 3, max(nops, nops // 3 + 1)))
        self.sets = [U._ss(S, eps, dev) for S in sizes]
        assert self.caps[0] == self.cap0
        if dev != "cpu":
            for ss in self.sets:  # the model's ladder is the device's
                assert [ss.capacity(c) for c in range(len(self.caps) + 1)] == self.caps + [-1]
        self.orc = [[OracleGK(eps) for _ in range(S)] for S in sizes]
        # floor[set][stream]: a class the stream has reached and cannot have left (see update_floors)
        self.floor = [[0] * S for S in sizes]
        self.renew_floor = set()     # sets that came back new (resized, a round trip) or gave everything back
        self.compacted = set()       # sets that have been compacted since they were made
        self.demoted = set()         # (set, stream) positions a compaction demoted, until they are promoted again
        self.snap = [None] * len(sizes)
        self.after_async = None      # index of the set whose ingest was left in flight
        self.async_source = None     # and the kind of that ingest
        self.follows_async = False   # this step is the one right after it
        self.replaced = False        # this step's fold was replaced by a reset (guard_fold)
        self.async_count = collections.Counter()  # per source
        self.late_answers = []       # (tensor, expected, what) of fused queries left in flight
        self.was_reset_large = set()  # (set, stream) positions
        self.nruns = 0
        self.log = []
        self.ran = collections.Counter()
        self.effective = collections.Counter()
        self.events = collections.Counter()
        self.max_table = 0
        self.max_large = 0

    # ------------------------------------------------------------- small helpers
    def large(self, o):
        return len(o.v) > self.cap0

    def large_ids(self, a):
        return [s for s, o in enumerate(self.orc[a]) if self.large(o)]

    def grow_target(self, a):
        """The stream of set a that a descending run or a burst of records goes to:
        the one with the longest table half of the time, so that one table keeps growing."""
        orc = self.orc[a]
        if self.rng.random() < 0.5:
            return max(range(len(orc)), key=lambda s: (len(orc[s].v), -s))
        return int(self.rng.integers(0, len(orc)))

    def other(self, a):
        return int(self.rng.choice([i for i in range(len(self.sets)) if i != a]))

    def t(self, x, dtype):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype))).to(self.dev)

    def ids_t(self, ids):
        return self.t(ids, np.int64 if self.rng.random() < 0.2 else np.int32)

    def pick_ids(self, a, distinct=False, count=None, prefer=None, p=0.45):
        """Unsorted ids of set a; unless `distinct`, one repeats at times and the
        list is empty at times.  A stream of `prefer` (the large ones unless
        given) is put in front at times."""
        rng, S = self.rng, self.sets[a].num_streams
        if not distinct and count is None and rng.random() < 0.05:
            return []
        K_ = int(rng.integers(1, min(S, 9) + 1)) if count is None else count
        ids = [int(s) for s in rng.choice(S, K_, replace=False)]
        big = self.large_ids(a) if prefer is None else prefer
        if big and rng.random() < p:
            b = int(rng.choice(big))
            if b in ids:
                ids.remove(b)
            else:
                ids.pop()
            ids.insert(0, b)
        if not distinct and rng.random() < 0.35:
            ids.insert(int(rng.integers(0, len(ids) + 1)), int(rng.choice(ids)))
        return ids

    def qs(self):
        rng = self.rng
        inside = [0.0, 1.0] + [float(q) for q in rng.random(3)]
        out = [-0.1 if rng.random() < 0.5 else 1.5]
        qs = [float(q) for q in rng.choice(inside, int(rng.integers(1, 5)), replace=False)]
        if rng.random() < 0.5:
            qs += out
        if rng.random() < 0.5:
            qs.sort()
        else:
            qs = [qs[k] for k in rng.permutation(len(qs))]
        return qs, bool(rng.random() < 0.4)

    def xs(self, a, ids):
        """Rank thresholds: values the covered streams hold, +-inf, zeros, a few others."""
        rng = self.rng
        pool = [float("inf"), float("-inf"), 0.0, -0.0] + [float(x) for x in rng.normal(0, 3, 3)]
        for s in ids[:4]:
            o = self.orc[a][s]
            if o.n:
                pool += [o.min, o.max]
            if o.v:
                pool += [o.v[len(o.v) // 2], o.v[0]]
            if o.pending:
                pool.append(o.pending[-1])
        return [pool[k] for k in rng.integers(0, len(pool), int(rng.integers(1, 7)))]

    def values(self, vr, L):
        return np.asarray(U.gen(int(vr.integers(0, 8)), int(L), vr), dtype=np.float64)

    def note_flush(self, oracles):
        for o in oracles:
            if len(o.pending) == self.P - 1:
                self.events["flush_pending_P_minus_1"] += 1
            if len(o.pending) == 1:
                self.events["flush_pending_1"] += 1

    def fold_bound(self, dst, members):
        """Upper bounds of the table and of n after dst.merge(m) for m in members."""
        size = len(dst.v) + len(dst.pending) + sum(len(m.v) + len(m.pending) + 1 for m in members)
        return size, dst.n + sum(m.n for m in members)

    def replace_set(self, a, new, oracles=None):
        self.sets[a].close()
        self.sets[a] = new
        if oracles is not None:
            self.orc[a] = oracles
        self.snap[a] = None
        self.forget_classes(a)
        self.compacted.discard(a)

    def forget_classes(self, a):
        """Set a is a new one, or gave every class back: its floors start again."""
        self.renew_floor.add(a)
        self.was_reset_large = {(i, s) for i, s in self.was_reset_large if i != a}
        self.demoted = {(i, s) for i, s in self.demoted if i != a}

    def left_in_flight(self, a, source):
        self.after_async, self.async_source = a, source
        self.async_count[source] += 1

    def late(self, check):
        """A comparison of outputs left in flight: made after the next operation."""
        self.late_answers.append(check)

    def note_ingest(self, a, streams):
        for s in streams:
            if (a, s) in self.was_reset_large:
                self.was_reset_large.discard((a, s))
                self.events["ingest_after_reset_large"] += 1

    def note_fold_dst_large(self, a):
        self.events["fold_dst_large"] += 1
        if a in self.compacted:
            self.events["fold_dst_large_after_compact"] += 1

    def note_move(self, src_o, dst_o):
        if self.large(src_o) and not self.large(dst_o):
            self.events["move_large_onto_small"] += 1
        if self.large(dst_o) and not self.large(src_o):
            self.events["move_small_onto_large"] += 1

    # ------------------------------------------------------------------ ingest
    def lens(self, vr, S):
        P, out = self.P, []
        for x in vr.random(S):
            if x < 0.35:
                L = 0
            elif x < 0.41:
                L = 1
            elif x < 0.60:
                L = int(vr.integers(1, max(P, 2)))
            elif x < 0.85:
                L = int(vr.choice([P - 1, P, P + 1, 2 * P]))
            else:
                L = int(vr.integers(2, 5)) * P + int(vr.integers(0, 3))
            out.append(L)
        return out

    def op_ingest(self, a, args):
        rng, ss, orc = self.rng, self.sets[a], self.orc[a]
        S = ss.num_streams
        vseed = int(rng.integers(1 << 30))
        vr = np.random.default_rng(vseed)
        lens = self.lens(vr, S)
        seqs = [self.values(vr, L) for L in lens]
        if rng.random() < 0.2:
            # a descending run; successive runs go further down, so a stream
            # that gets several keeps growing its table
            s = self.grow_target(a)
            if len(orc[s].v) < self.limit - self.run_growth:
                units = int(rng.integers(2, 7)) if rng.random() < 0.6 else int(rng.integers(*self.run_units))
                L = units * self.P + int(rng.integers(0, self.P))
                self.nruns += 1
                seqs[s] = -1e6 * self.nruns - np.arange(float(L))
                lens[s] = L
                args["run"] = (s, L)
        query = rng.random() < 0.3
        qs, single = self.qs() if query else (None, False)
        sync = not (self.async_ingest and rng.random() < 0.7)
        args.update(vseed=vseed, lens=_short(lens), qs=qs, single=single, sync=sync)
        flat, offs = U.csr(seqs)
        got = ss.ingest(self.t(flat, np.float64), self.t(offs, np.int64), quantiles=qs, single=single, sync=sync)
        self.note_ingest(a, [s for s, L in enumerate(lens) if L])
        for o, x in zip(orc, seqs):
            o.add_many(x)
        if query:
            if self.fault == "ingest_query_no_flush":
                exp = C.oracle_answers(copy.deepcopy(orc), range(S), qs, single)
            else:
                exp = C.oracle_answers(orc, range(S), qs, single)
            self.fused_answers(got, exp, sync)
        if not sync:
            self.left_in_flight(a, "ingest")
        return {a: ALL}, any(lens)

    def fused_answers(self, got, exp, sync):
        what = "fused answers of step %d" % (len(self.log) - 1)
        check = lambda: U.assert_same_quantiles(got.cpu().numpy(), exp, what, None)  # noqa: E731
        if sync:
            check()
        else:
            self.late(check)

    def keyed_ids(self, a, vr, N, none=0.0):
        """The stream ids of N keyed samples: random ones, one stream (a large one
        preferred) or a subset of the streams, about 3 % of them negative; with
        probability `none` every one is negative."""
        rng, orc = self.rng, self.orc[a]
        S = len(orc)
        mode = ["random", "one", "subset"][int(rng.integers(0, 3))]
        if mode == "random":
            ids = vr.integers(0, S, N)
        elif mode == "one":
            big = self.large_ids(a)
            ids = np.full(N, int(rng.choice(big)) if big and rng.random() < 0.6 else int(rng.integers(0, S)))
        else:
            ids = vr.choice(vr.choice(S, max(1, S // 3), replace=False), N)
        ids = np.asarray(ids, dtype=np.int64)
        ids[vr.random(N) < 0.03] = -1  # (skipped by the call)
        if rng.random() < none:
            mode = "none"
            ids = -1 - np.asarray(vr.integers(0, 9, N), dtype=np.int64)
        return mode, ids

    def op_ingest_keyed(self, a, args):
        rng, ss, orc = self.rng, self.sets[a], self.orc[a]
        S = ss.num_streams
        vseed = int(rng.integers(1 << 30))
        vr = np.random.default_rng(vseed)
        r = rng.random()
        N = 0 if r < 0.1 else int(vr.integers(1, 4)) if r < 0.2 else int(vr.integers(S, 6 * self.P + S))
        mode, ids = self.keyed_ids(a, vr, N)
        vals = self.values(vr, N)
        query = rng.random() < 0.3
        qs, single = self.qs() if query else (None, False)
        sync = not (self.async_ingest and rng.random() < 0.7)
        args.update(vseed=vseed, N=N, mode=mode, streams=_short(sorted(set(ids[ids >= 0].tolist()))), qs=qs,
                    single=single, sync=sync)
        hit = sorted(set(ids[ids >= 0].tolist()))
        if any(self.large(orc[s]) for s in hit):
            self.events["keyed_into_large"] += 1
        got = ss.ingest_keyed(self.ids_t(ids), self.t(vals, np.float64), quantiles=qs, single=single, sync=sync)
        self.note_ingest(a, hit)
        KC.oracle_loop(orc, ids, vals)
        if query:
            self.fused_answers(got, C.oracle_answers(orc, range(S), qs, single), sync)
        if not sync:
            self.left_in_flight(a, "ingest_keyed")
        return {a: ALL}, bool(hit)

    # ---------------------------------------------------------------- selection
    def op_flush_select(self, a, args):
        orc = self.orc[a]
        edge = [s for s, o in enumerate(orc) if len(o.pending) in (1, self.P - 1)]
        ids = self.pick_ids(a, prefer=edge + [s for s, o in enumerate(orc) if o.pending][:2], p=0.8)
        args["ids"] = ids
        self.note_flush([orc[s] for s in set(ids)])
        self.sets[a].flush_select(self.ids_t(ids))
        flushed = ids[:-1] if self.fault == "flush_select_skips_one" else ids
        for s in set(flushed):
            if orc[s].n > 0:
                orc[s].size()
        return {a: set(ids)}, None

    def op_reset_select(self, a, args):
        ids = self.pick_ids(a)
        args["ids"] = ids
        self.reset_streams(a, ids)
        return {a: set(ids)}, None

    def reset_streams(self, a, ids):
        orc = self.orc[a]
        for s in set(ids):
            if self.large(orc[s]):
                self.events["reset_large"] += 1
                self.was_reset_large.add((a, s))
        self.sets[a].reset_select(self.ids_t(ids))
        done = sorted(set(ids))
        if self.fault == "reset_one_too_few":
            done = done[:-1]
        for s in done:
            orc[s] = OracleGK(self.eps)

    def op_quantiles_select(self, a, args):
        ids = self.pick_ids(a)
        qs, single = self.qs()
        args.update(ids=ids, qs=qs, single=single)
        # (the driver's own snapshot, None after an ingest left in flight: the helper reads nothing first)
        C.check_query(self.sets[a], self.orc[a], ids, qs, single, "quantiles_select", before=self.snap[a])
        return {a: set(ids)}, any(self.orc[a][s].n for s in ids)

    def op_stats_select(self, a, args):
        ids = self.pick_ids(a)
        args["ids"] = ids
        orc = self.orc[a]
        st = {k: v.cpu().numpy() for k, v in self.sets[a].stats_select(self.ids_t(ids)).items()}
        for k, f in (("n", lambda o: o.n), ("size", lambda o: len(o.v)), ("pending", lambda o: len(o.pending))):
            assert st[k].tolist() == [f(orc[s]) for s in ids], "stats_select " + k
        for k in ("min", "max", "sum", "avg"):
            exp = np.asarray([getattr(orc[s], k) for s in ids], dtype=np.float64)
            assert st[k].tobytes() == exp.tobytes(), "stats_select " + k
        return {a: set()}, any(orc[s].n for s in ids)

    def op_ranks(self, a, args, select=False):
        rng = self.rng
        ids = self.pick_ids(a) if select else None
        covered = ids if select else list(range(self.sets[a].num_streams))
        xs = self.xs(a, covered)
        lo, hi = [(True, True), (True, True), (True, False), (False, True)][int(rng.integers(0, 4))]
        args.update(ids=ids, xs=xs, lo=lo, hi=hi)
        K.check_ranks(self.sets[a], self.orc[a], ids, xs, "ranks", lo=lo, hi=hi, before=self.snap[a])
        return {a: set(covered)}, any(self.orc[a][s].n for s in covered)

    def op_ranks_select(self, a, args):
        return self.op_ranks(a, args, select=True)

    def op_cdf_select(self, a, args):
        ids = self.pick_ids(a)
        xs = self.xs(a, ids)
        args.update(ids=ids, xs=xs)
        orc = self.orc[a]
        got = self.sets[a].cdf_select(self.ids_t(ids), xs).cpu().numpy()
        K.flush_covered(orc, ids)
        lo, hi = K.expected_rows(orc, ids, xs)
        n = np.asarray([orc[s].n for s in ids], dtype=np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            exp = (lo + hi).astype(np.float64) / (2.0 * n.astype(np.float64))[:, None]
        U.assert_same_quantiles(got, exp.reshape(got.shape), "cdf_select", None)
        return {a: set(ids)}, any(orc[s].n for s in ids)

    # ------------------------------------------------------- keyed rank queries
    def keyed_batch(self, a, args, thresholds, none=0.05):
        """(ids, xs) of a keyed rank query or score-and-ingest on set a.  The x of
        a row is one of self.xs of its stream (`thresholds`) or a value to be
        ingested; a negative row has a NaN x at times."""
        rng, orc = self.rng, self.orc[a]
        S, P = len(orc), self.P
        vseed = int(rng.integers(1 << 30))
        vr = np.random.default_rng(vseed)
        r = rng.random()
        top = 3 * P if P <= 128 else 2 * P  # (a few flush periods)
        N = 0 if r < 0.1 else int(vr.integers(1, 4)) if r < 0.2 else int(vr.integers(S, top + S))
        mode, ids = self.keyed_ids(a, vr, N, none=none)
        live = sorted(set(ids[ids >= 0].tolist()))
        if thresholds:
            per = {s: self.xs(a, [s]) for s in live}
            pick = vr.integers(0, 6, N)
            xs = np.asarray([per[s][k % len(per[s])] if s >= 0 else 0.5 for s, k in zip(ids.tolist(), pick.tolist())],
                            dtype=np.float64)
        else:
            xs = self.values(vr, N)
        xs[(ids < 0) & (vr.random(N) < 0.5)] = float("nan")
        args.update(vseed=vseed, N=N, mode=mode, streams=_short(live))
        return ids, xs, live

    def rank_outputs(self, allow_none):
        combos = [(True, True, False), (True, True, True), (True, False, True), (False, True, False),
                  (False, False, True)] + ([(False, False, False)] if allow_none else [])
        return combos[int(self.rng.integers(0, len(combos)))]

    def same_rows(self, got, exp, want, what):
        for g, e, w, name in zip(got, exp or (None,) * 3, want, ("lo", "hi", "n")):
            assert (g is None) == (not w), (what, name)
            if w:
                Q.same_i64(g, e, what + " " + name)

    def score_of(self, rows):
        lo, hi, n = rows
        with np.errstate(invalid="ignore", divide="ignore"):
            return (lo + hi).astype(np.float64) / (2.0 * n.astype(np.float64))

    def op_ranks_keyed(self, a, args, cdf=False):
        ss, orc = self.sets[a], self.orc[a]
        ids, xs, live = self.keyed_batch(a, args, thresholds=True)
        want = (True, True, True) if cdf else self.rank_outputs(False)
        args.update(want=want)
        if any(self.large(orc[s]) for s in live):
            self.events["keyed_rank_of_large"] += 1
        self.note_flush([orc[s] for s in live])
        ti, tx = self.ids_t(ids), self.t(xs, np.float64)
        if cdf:
            got = ss.cdf_keyed(ti, tx)
        else:
            got = ss.ranks_keyed(ti, tx, lo=want[0], hi=want[1], n=want[2])
        model = copy.deepcopy(orc) if self.fault == "ranks_keyed_no_flush" else orc
        K.flush_covered(model, live)  # (the state change: the occurring streams are flushed)
        exp = Q.expected_rows(model, ids.tolist(), xs.tolist())
        if cdf:
            assert got.dtype == torch.float64 and tuple(got.shape) == (len(ids),)
            U.assert_same_quantiles(got.cpu().numpy(), self.score_of(exp), "cdf_keyed", None)
        else:
            self.same_rows(got, exp, want, "ranks_keyed")
        return {a: set(live)}, any(orc[s].n for s in live)

    def op_cdf_keyed(self, a, args):
        return self.op_ranks_keyed(a, args, cdf=True)

    def op_rank_ingest_keyed(self, a, args):
        rng, ss, orc = self.rng, self.sets[a], self.orc[a]
        S = len(orc)
        ids, xs, live = self.keyed_batch(a, args, thresholds=False, none=0.12)
        query = rng.random() < 0.3
        qs, single = self.qs() if query else (None, False)
        score = bool(rng.random() < 0.5)
        want = (True, True, True) if score else self.rank_outputs(True)
        sync = not (self.async_ingest and rng.random() < 0.7)
        args.update(qs=qs, single=single, score=score, want=want, sync=sync)
        if any(self.large(orc[s]) for s in live):
            self.events["rank_ingest_into_large"] += 1
        if live and np.bincount(ids[ids >= 0]).max() >= self.P:
            self.events["rank_ingest_flush_inside_run"] += 1
        if len(ids) and not live:
            self.events["rank_ingest_new_values_only_negative"] += 1
        ranked = any(want)  # (with no rank output the call is ingest_keyed: nothing is flushed first)
        if ranked:
            self.note_flush([orc[s] for s in live])
        ti, tx = self.ids_t(ids), self.t(xs, np.float64)
        if score:
            got = ss.score_ingest_keyed(ti, tx, quantiles=qs, single=single, sync=sync)
            got = got if query else (got,)
        else:
            got = ss.rank_ingest_keyed(ti, tx, lo=want[0], hi=want[1], n=want[2], quantiles=qs, single=single,
                                       sync=sync)
        self.note_ingest(a, live)
        il, xl = ids.tolist(), xs.tolist()
        if not ranked:
            exp = None
            KC.oracle_loop(orc, ids, xs)
        elif self.fault == "rank_ingest_ranks_after_add":
            ahead = copy.deepcopy(orc)
            KC.oracle_loop(ahead, ids, xs)
            K.flush_covered(ahead, live)
            exp = Q.expected_rows(ahead, il, xl)
            RI.oracle_step(orc, il, xl)
        else:
            exp = RI.oracle_step(orc, il, xl)  # every row against the state before the batch, then the batch
        if self.fault == "rank_ingest_adds_negative_rows":
            for s, x in zip(il, xl):
                if s < 0 and x == x:
                    orc[(-1 - s) % S].add(x)
        checks = []
        if score:
            exp_score = self.score_of(exp)
            checks.append(lambda: U.assert_same_quantiles(got[0].cpu().numpy(), exp_score, "score_ingest_keyed", None))
        else:
            checks.append(lambda: self.same_rows(got[:3], exp, want, "rank_ingest_keyed"))
        if query:
            exp_q = C.oracle_answers(orc, range(S), qs, single)
            checks.append(lambda: U.assert_same_quantiles(got[-1].cpu().numpy(), exp_q, "fused answers", None))
        for check in checks:
            if sync:
                check()
            else:
                self.late(check)
        if not sync:
            self.left_in_flight(a, "rank_ingest_keyed")
        return {a: ALL if query else set(live)}, bool(live)

    # --------------------------------------------------------------- compaction
    def fits(self, a):
        return [fit(len(o.v), self.caps) for o in self.orc[a]]

    def op_compact(self, a, args):
        rng, ss, orc = self.rng, self.sets[a], self.orc[a]
        fits, floor = self.fits(a), self.floor[a]
        down = [s for s in range(len(orc)) if floor[s] > fits[s]]
        again = bool(rng.random() < 1.0 / 3.0)
        args.update(demotes=_short(down), again=again)
        if down:
            self.events["compact_demotes"] += 1
        if any(o.pending for o, f in zip(orc, floor) if f > 0):
            self.events["compact_with_pending"] += 1
        if any(c not in fits for c in set(floor) if c > 0):
            self.events["compact_empties_class"] += 1
        compact_with_floors(ss, orc, floor, self.caps, "compact of set %d" % a, settles=self.follows_async, again=again)
        self.floor[a] = list(fits)
        self.demoted |= {(a, s) for s in down}
        self.was_reset_large = {(i, s) for i, s in self.was_reset_large if i != a}
        self.compacted.add(a)
        return {a: set()}, bool(down)

    def update_floors(self):
        """floor[set][stream] after an operation: the maximum of itself and fit of
        the oracle's table -- classes only grow, and a stream always fits its
        class.  A set that came back new or gave everything back starts at fit of
        the present tables (a sound lower bound whatever an import chose); a
        compaction has set its floors itself.  reset_select, put and
        unpack_select demote nothing: the floor stays."""
        for a, orc in enumerate(self.orc):
            fits = self.fits(a)
            if a in self.renew_floor:
                self.floor[a] = fits
                continue
            floor = self.floor[a]
            for s, f in enumerate(fits):
                if f > floor[s]:
                    floor[s] = f
                    if (a, s) in self.demoted:
                        self.demoted.discard((a, s))
                        self.events["promoted_again_after_compact"] += 1
        self.renew_floor.clear()
        # the model's own books agree: a stream fits the class of its floor, and
        # a stream that was reset while large still holds a class above 0
        for a, orc in enumerate(self.orc):
            for s, o in enumerate(orc):
                assert len(o.v) <= self.caps[self.floor[a][s]] - 1, \
                    "model: stream %d of set %d outgrew its floor" % (s, a)
                if len(o.v) in self.caps:
                    self.events["table_at_capacity"] += 1
        for a, s in self.was_reset_large:
            assert self.floor[a][s] > 0, "model: stream %d of set %d was reset while large, floor 0" % (s, a)

    def check_classes(self, a, what):
        usage_above_floors(self.sets[a], self.floor[a], self.caps, what)

    # ---------------------------------------------------------------- whole set
    def op_flush(self, a, args):
        self.note_flush(self.orc[a])
        self.sets[a].flush()
        for o in self.orc[a]:
            o.size()
        return {a: ALL}, None

    def op_quantiles(self, a, args):
        qs, single = self.qs()
        args.update(qs=qs, single=single)
        S = self.sets[a].num_streams
        got = self.sets[a].quantiles(qs, single=single).cpu().numpy()
        U.assert_same_quantiles(got, C.oracle_answers(self.orc[a], range(S), qs, single), "quantiles", None)
        return {a: ALL}, any(o.n for o in self.orc[a])

    def op_reset(self, a, args):
        self.sets[a].reset()
        self.orc[a] = [OracleGK(self.eps) for _ in self.orc[a]]
        self.forget_classes(a)  # (a whole-set reset gives every class back)
        return {a: ALL}, None

    # -------------------------------------------------------------------- folds
    def guard_fold(self, a, pairs, args):
        """pairs: (destination stream of set a, [member oracles]).  A fold that
        would leave the range the engines hold is replaced by a reset of the
        destination streams concerned."""
        bad = []
        for s, members in pairs:
            size, n = self.fold_bound(self.orc[a][s], members)
            if size > self.limit or n > MAX_N:
                bad.append(s)
        if bad:
            self.replaced = True
            args["replaced_by_reset"] = bad
            self.reset_streams(a, bad)
            return {a: set(bad)}
        return None

    def op_merge_from(self, a, args):
        rng = self.rng
        b = self.other(a)
        if self.follows_async:
            # merge_from itself, not the take of a slice, is the call that follows: a source at least as large
            fits = [i for i in range(len(self.sets)) if i != a and self.sets[i].num_streams >= self.sets[a].num_streams]
            if fits:
                b = int(rng.choice(fits))
        plan = [["b"], ["b", "a", "b"], ["a"], ["b", "b"], ["a", "b"]][int(rng.integers(0, 5))]
        if self.follows_async and not fits:
            plan = ["a"]  # (no such source: the self-merge needs no slice)
        A, B = self.sets[a], self.sets[b]
        m = min(A.num_streams, B.num_streams) if "b" in plan else A.num_streams  # (a plain self-merge: the whole set)
        # the larger of the two goes through take of a slice and put back
        ids_a = list(range(A.num_streams)) if A.num_streams == m else \
            [int(s) for s in (rng.choice(A.num_streams, m, replace=False) if rng.random() < 0.5 else
                              np.arange(m) + int(rng.integers(0, A.num_streams - m + 1)))]
        ids_b = list(range(m))
        if "b" not in plan:
            ids_b = []
        elif B.num_streams != m:
            off = int(rng.integers(0, B.num_streams - m + 1))
            ids_b = [s + off for s in range(m)]
        args.update(src=b, plan=plan, ids_dst=ids_a, ids_src=ids_b)
        oa, ob = self.orc[a], self.orc[b]
        pairs = [(ids_a[k], [ob[ids_b[k]] if p == "b" else oa[ids_a[k]] for p in plan] * 2) for k in range(m)]
        # (* 2: a self-merge doubles what the earlier steps of the plan left)
        touched = self.guard_fold(a, pairs, args)
        if touched is not None:
            return touched, None
        for k in range(m):
            d = oa[ids_a[k]]
            if self.large(d):
                self.note_fold_dst_large(a)
            elif "b" in plan and self.large(ob[ids_b[k]]):
                self.events["fold_member_large_dst_small"] += 1
        ta = A if A.num_streams == m else A.take(C.i32(ids_a))
        tb = B if B.num_streams == m or "b" not in plan else B.take(C.i32(ids_b))
        ta.merge_from([tb if p == "b" else ta for p in plan])
        if ta is not A:
            A.put(C.i32(ids_a), ta)
            ta.close()
        if tb is not B:
            B.put(C.i32(ids_b), tb)
            tb.close()
        for p in plan:
            for k in range(m):
                d = oa[ids_a[k]]
                src = ob[ids_b[k]] if p == "b" else d
                if self.fault == "merge_source_not_flushed" and p == "b":
                    src = copy.deepcopy(src)
                d.merge(src)
        return {a: set(ids_a), b: set(ids_b) if "b" in plan else set()}, None

    def groups(self, a, b):
        rng = self.rng
        G, S = self.sets[a].num_streams, self.sets[b].num_streams
        r = rng.random()
        groups = [[] for _ in range(G)]
        if r < 0.1:
            pass                                     # every group empty
        elif r < 0.25:
            groups[int(rng.integers(0, G))] = [int(s) for s in rng.permutation(S)]  # one group holds every member
        else:
            for s in rng.permutation(S):
                if rng.random() < 0.6:
                    j = int(rng.integers(0, G)) if rng.random() < 0.5 else int(rng.integers(0, min(G, 3)))
                    groups[j].append(int(s))
        return groups

    def op_rollup(self, a, args, by_key=False):
        b = self.other(a)
        groups = self.groups(a, b)
        if by_key:
            groups = [sorted(g) for g in groups]  # (members of a key's group go in ascending source index)
        args.update(src=b, groups=[(j, g) for j, g in enumerate(groups) if g])
        oa, ob = self.orc[a], self.orc[b]
        touched = self.guard_fold(a, [(j, [ob[m] for m in g]) for j, g in enumerate(groups) if g], args)
        if touched is not None:
            return touched, None
        for j, g in enumerate(groups):
            if g and self.large(oa[j]):
                self.note_fold_dst_large(a)
            elif any(self.large(ob[m]) for m in g):
                self.events["fold_member_large_dst_small"] += 1
        dst, src = self.sets[a], self.sets[b]
        call = None
        if by_key:
            keys = np.full(src.num_streams, -1, np.int64)
            for j, g in enumerate(groups):
                keys[g] = j
            call = lambda: dst.rollup_by_key(src, self.t(keys, np.int64))  # noqa: E731
        model_groups = groups
        if self.fault == "rollup_ascending_members":
            go, mem = R.csr_of(groups)
            call = lambda: dst.rollup_from(src, go, mem)  # noqa: E731
            model_groups = [sorted(g) for g in groups]
        R.check_rollup(dst, src, oa, ob, model_groups, "rollup", call=call, quantiles=False)
        return {a: {j for j, g in enumerate(groups) if g}, b: {m for g in groups for m in g}}, None

    def op_rollup_from(self, a, args):
        return self.op_rollup(a, args)

    def op_rollup_by_key(self, a, args):
        return self.op_rollup(a, args, by_key=True)

    def op_merge_compress(self, a, args):
        rng, ss, orc = self.rng, self.sets[a], self.orc[a]
        S = ss.num_streams
        if rng.random() < 0.3:
            args["records"] = None
            ss.merge_compress()
            for o in orc:
                o.flush()
            return {a: ALL}, None
        vseed = int(rng.integers(1 << 30))
        vr = np.random.default_rng(vseed)
        burst = -1
        if rng.random() < 0.3:
            burst = self.grow_target(a)
        recs = []
        for s, o in enumerate(orc):
            k = int(vr.integers(0, 30)) if vr.random() < 0.5 else 0
            if o.n == 0:
                k = 0
            elif s == burst and len(o.v) + len(o.pending) < self.limit - self.cap0 - 100:
                k = self.cap0 + int(vr.integers(5, 60))
            if k == 0:
                recs.append([])
                continue
            base = np.asarray(o.v + o.pending, dtype=np.float64)
            v = np.sort(np.concatenate([vr.choice(base, size=k // 2), vr.lognormal(0, 1, k - k // 2)]))
            if s == burst:
                # records past the table's last entry keep the deltas they come with (gk:85-92), and
                # deltas well above the stream's removal threshold keep them apart until n has grown
                # several times: a large table at once
                v = (o.v[-1] if o.v else 0.0) + np.cumsum(vr.lognormal(0, 1, k))
                T = int(2.0 * self.eps * o.n)
                g = np.ones(k, np.int64)
                d = 3 * T + 20 + vr.integers(0, 20, k)
            else:
                g = vr.integers(1, 3 + int(0.02 / self.eps), k)
                d = vr.integers(0, 2 + int(0.04 / self.eps), k)
            recs.append(list(zip(v.tolist(), g.tolist(), d.tolist())))
        args.update(vseed=vseed, records=[len(r) for r in recs], burst=burst)
        flat = [r for rs in recs for r in rs]
        offs = np.concatenate([[0], np.cumsum([len(rs) for rs in recs])]).astype(np.int64)
        ss.merge_compress(torch.tensor([r[0] for r in flat], dtype=torch.float64),
                          torch.tensor([r[1] for r in flat], dtype=torch.int32),
                          torch.tensor([r[2] for r in flat], dtype=torch.int32), torch.from_numpy(offs))
        for o, rs in zip(orc, recs):
            o.flush(rs)
        return {a: ALL}, None

    # -------------------------------------------------------------------- moves
    def move_ids(self, a, b):
        """(source ids of a, which may repeat; distinct destination ids of b)."""
        src = self.pick_ids(a, count=int(self.rng.integers(1, min(self.sets[a].num_streams,
                                                                  self.sets[b].num_streams, 8) + 1)))
        src = src[:self.sets[b].num_streams]
        dst = self.pick_ids(b, distinct=True, count=len(src))
        for s, d in zip(src, dst):
            self.note_move(self.orc[a][s], self.orc[b][d])
        if src and (a in self.compacted or b in self.compacted):
            self.events["move_after_compact"] += 1
        return src, dst

    def model_move(self, a, b, src, dst, sorted_order=False):
        moved = [copy.deepcopy(self.orc[a][s]) for s in src]
        for k, d in enumerate(sorted(dst) if sorted_order else dst):
            self.orc[b][d] = moved[k]
        for d in dst:
            self.was_reset_large.discard((b, d))

    def op_take_put(self, a, args):
        rng = self.rng
        b = a if rng.random() < 0.3 else self.other(a)
        src, dst = self.move_ids(a, b)
        host = bool(self.via_host and rng.random() < 0.6)
        more = host and rng.random() < 0.5
        vseed = int(rng.integers(1 << 30))
        args.update(to=b, src=src, dst=dst, via_host=host, host_ingest=vseed if more else None)
        t = self.sets[a].take(self.ids_t(src), device="cpu" if host else None)
        moved = [copy.deepcopy(self.orc[a][s]) for s in src]
        if more:  # the host set goes on for a while before it comes back
            vr = np.random.default_rng(vseed)
            seqs = [self.values(vr, L) for L in self.lens(vr, len(src))]
            U.ingest_np(t, seqs)
            for o, x in zip(moved, seqs):
                o.add_many(x)
        R.assert_set_matches(t, moved, "the taken set")
        self.sets[b].put(self.ids_t(dst), t)
        t.close()
        order = sorted(dst) if self.fault == "put_sorted_order" else dst
        for k, d in enumerate(order):
            self.orc[b][d] = moved[k]
            self.was_reset_large.discard((b, d))
        return ({a: set(dst)} if a == b else {a: set(), b: set(dst)}), None

    def op_pack_unpack(self, a, args):
        rng = self.rng
        b = a if rng.random() < 0.3 else self.other(a)
        src, dst = self.move_ids(a, b)
        args.update(to=b, src=src, dst=dst)
        A = self.sets[a]
        i = self.ids_t(src)
        nbytes = A.pack_select_bytes(i)
        buf = torch.zeros(nbytes + int(rng.integers(0, 3)) * 256, dtype=torch.uint8, device=A.device)
        assert A.pack_select(i, buf) is buf
        self.sets[b].unpack_select(self.ids_t(dst), buf)
        self.model_move(a, b, src, dst)
        return ({a: set(dst)} if a == b else {a: set(), b: set(dst)}), None

    def op_resized(self, a, args):
        rng = self.rng
        S = self.sets[a].num_streams
        r = rng.random()
        S2 = S if r < 0.2 else max(3, S - int(rng.integers(1, 6))) if (r < 0.6 or S > 40) else S + int(rng.integers(1, 6))
        args["streams"] = (S, S2)
        new = self.sets[a].resized(S2)
        kept = self.orc[a][:S2]
        fill = [OracleGK(self.eps) for _ in range(S2 - len(kept))]
        if self.fault == "drop:resized" and S2 != S:
            # (the list changes its length: the generic fault has no stream to restore)
            if fill:
                fill[-1] = copy.deepcopy(kept[0])
            else:
                kept[-1] = OracleGK(self.eps)
        self.replace_set(a, new, kept + fill)
        return {a: ALL}, S2 != S

    # -------------------------------------------------------- state round trips
    def op_roundtrip_state(self, a, args):
        old = self.sets[a]
        new = U._ss(old.num_streams, self.eps, self.dev)
        new.import_state(old.export_state())
        self.replace_set(a, new)
        return {a: ALL}, any(o.n for o in self.orc[a])

    def op_roundtrip_file(self, a, args):
        old = self.sets[a]
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "set.gkstate")
            old.save(path)
            new = self.StreamSet.load(path, device=self.dev)
        assert new.num_streams == old.num_streams and new.eps == self.eps
        self.replace_set(a, new)
        return {a: ALL}, any(o.n for o in self.orc[a])

    def op_roundtrip_pack(self, a, args):
        old = self.sets[a]
        new = U._ss(old.num_streams, self.eps, self.dev)
        new.fold_packed([old.pack()])
        self.replace_set(a, new)
        return {a: ALL}, any(o.n for o in self.orc[a])

    # --------------------------------------------------------------- void calls
    def op_void(self, a, args):
        from gkarray_amd import UnequalEpsilonException
        from gkarray_amd._lib import GKBackendError
        rng, ss = self.rng, self.sets[a]
        S = ss.num_streams
        calls = [c for c in VOID_CALLS if c not in ("unpack_duplicate", "merge_other_eps")] if self.follows_async \
            else VOID_CALLS  # (those two start with a valid call or never reach the engine)
        what = calls[int(rng.integers(0, len(calls)))]
        ids = self.pick_ids(a, count=int(rng.integers(1, min(S, 5) + 1)))
        args.update(call=what, ids=ids)
        exc = GKBackendError
        if what == "select_id_S":
            bad = list(ids)
            bad.insert(int(rng.integers(0, len(bad) + 1)), S)
            which = ["quantiles_select", "flush_select", "reset_select", "stats_select", "ranks_select",
                     "pack_select"][int(rng.integers(0, 6))]
            args.update(ids=bad, which=which)
            i = self.ids_t(bad)
            call = {"quantiles_select": lambda: ss.quantiles_select(i, [0.5]), "flush_select": lambda: ss.flush_select(i),
                    "reset_select": lambda: ss.reset_select(i), "stats_select": lambda: ss.stats_select(i),
                    "ranks_select": lambda: ss.ranks_select(i, [0.5]), "pack_select": lambda: ss.pack_select(i)}[which]
        elif what == "unpack_duplicate":
            good = self.pick_ids(a, distinct=True, count=min(S, 3))
            buf = ss.pack_select(C.i32(good))
            dup = [good[0]] + good[1:-1] + [good[0]] if len(good) > 1 else good
            if len(good) == 1:
                buf, dup = ss.pack_select(C.i32(good * 2)), good * 2
            args["ids"] = dup
            call = lambda: ss.unpack_select(C.i32(dup), buf)  # noqa: E731
        elif what == "nan_q":
            i = self.ids_t(ids)
            if rng.random() < 0.5:
                call = lambda: ss.quantiles([0.5, float("nan")])  # noqa: E731
            else:
                call = lambda: ss.quantiles_select(i, [float("nan"), 0.5])  # noqa: E731
        elif what == "nan_threshold":
            i = self.ids_t(ids)
            if rng.random() < 0.5:
                call = lambda: ss.ranks([1.0, float("nan")])  # noqa: E731
            else:
                call = lambda: ss.ranks_select(i, [float("nan")])  # noqa: E731
        elif what == "merge_other_eps":
            exc = UnequalEpsilonException
            tmp = U._ss(S, self.eps * 2, self.dev)
            U.ingest_np(tmp, [np.arange(3.0)] * S)
            call = lambda: ss.merge_from([tmp])  # noqa: E731
        else:
            assert what == "keyed_id_S"
            n = int(rng.integers(1, 40))
            kid = rng.integers(0, S, n)
            kid[int(rng.integers(0, n))] = S
            call = lambda: ss.ingest_keyed(self.t(kid, np.int32), self.t(np.arange(float(n)), np.float64),  # noqa: E731
                                           sync=True)
        with pytest.raises(exc):
            call()
        if what == "merge_other_eps":
            tmp.close()
        return {a: set()}, True

    # --------------------------------------------------------------- the driver
    def step(self, k):
        rng = self.rng
        w = self.weights
        kind = KINDS[int(rng.choice(len(KINDS), p=w / w.sum()))]
        a = int(rng.integers(0, len(self.sets)))
        if k == self.reset_step:
            kind = "reset"
        if kind in ("flush", "flush_select") and rng.random() < 0.7:
            # (a flush matters where values are pending: the set with most such streams)
            a = max(range(len(self.sets)), key=lambda i: (sum(1 for o in self.orc[i] if o.pending), -i))
        if kind == "compact" and rng.random() < 0.7:
            # (a compaction matters where streams have shrunk: the set with most of them)
            a = max(range(len(self.sets)),
                    key=lambda i: (sum(1 for f, t in zip(self.floor[i], self.fits(i)) if f > t), -i))
        follows_async = self.follows_async = self.after_async is not None
        self.replaced = False
        if follows_async:
            # straight to the set whose ingest is in flight, every kind in turn
            a, source = self.after_async, self.async_source
            kind = KINDS[(7 * self.seed + self.async_count[source]) % len(KINDS)]
            self.after_async = None
        args = {"set": a}
        self.log.append((k, kind, args))
        saved = None
        if self.fault == "drop:" + kind or (follows_async and self.fault == "drop_after_async:" + kind):
            saved = copy.deepcopy(self.orc)
        before = [[_fp(o) for o in os_] for os_ in self.orc]
        if follows_async:
            target = self.sets[a]
            rec = target._lib = _Recorder(target._lib)
            try:
                touched, effective = getattr(self, "op_" + kind)(a, args)
            finally:
                target._lib = rec.lib
            first = REPLACED if self.replaced else kind
            assert rec.names and rec.names[0] in FIRST_CALL[first], \
                "the first call after the ingest left in flight was %s" % rec.names[:3]
        else:
            touched, effective = getattr(self, "op_" + kind)(a, args)
        # (a fold that guard_fold replaced by a reset counts as neither that fold nor a reset_select)
        counted = REPLACED if self.replaced else kind
        self.ran[counted] += 1
        if follows_async:
            self.events["after_async:" + counted] += 1
            self.events["after_async:%s:%s" % (source, counted)] += 1
        if effective is None:  # a state-changing kind: did the model change?
            effective = [[_fp(o) for o in os_] for os_ in self.orc] != before
        self.effective[counted] += bool(effective)
        if saved is not None and kind != "resized" and not self.replaced:
            self.forget_one(saved, before)
        sizes = [len(o.v) for os_ in self.orc for o in os_]
        self.max_table = max(self.max_table, max(sizes))
        self.max_large = max(self.max_large, sum(1 for x in sizes if x > self.cap0))
        if kind != "compact":
            self.update_floors()
        if self.after_async is not None:
            # nothing is read between an ingest left in flight and the next operation,
            # and that operation finds no snapshot of the set to compare with
            self.snap[self.after_async] = None
            return
        for i, ss in enumerate(self.sets):
            listed = touched.get(i, set())
            if listed is ALL or follows_async and i == a:
                listed = set(range(ss.num_streams))
            self.snap[i] = C.assert_all(ss, self.orc[i], "after %s, set %d" % (kind, i), self.snap[i], listed)
            self.check_classes(i, "after %s, set %d" % (kind, i))
        self.check_late_answers()

    def check_late_answers(self):
        late, self.late_answers = self.late_answers, []
        for check in late:
            check()

    def forget_one(self, saved, before):
        """The generic model fault: the last stream this operation changed goes back to its state before."""
        for i in reversed(range(len(self.orc))):
            if len(saved[i]) != len(self.orc[i]):
                continue
            for s in reversed(range(len(self.orc[i]))):
                if _fp(self.orc[i][s]) != before[i][s]:
                    self.orc[i][s] = saved[i][s]
                    return

    def describe(self, upto):
        return "\n".join("  %3d %s %r" % (k, kind, args) for k, kind, args in self.log[:upto])

    def run(self):
        try:
            for k in range(self.steps):
                try:
                    self.step(k)
                except Exception as e:
                    _, kind, args = self.log[-1]
                    raise AssertionError(
                        "opseq eps=%g seed=%d step=%d of %d, %s %r: %s: %s\n(replay the steps before it with "
                        "stop_after=%d) operations so far:\n%s"
                        % (self.eps, self.seed, k, self.nops, kind, args, type(e).__name__, e, k,
                           self.describe(len(self.log)))) from e
            if self.after_async is not None:  # the sequence ended on an ingest left in flight
                a, self.after_async = self.after_async, None
                self.sets[a].sync()
                C.assert_all(self.sets[a], self.orc[a], "eps=%g seed=%d: after the last sync" % (self.eps, self.seed))
                self.check_late_answers()
        finally:
            for ss in self.sets:
                ss.close()
        return dict(ran=self.ran, effective=self.effective, events=self.events, max_table=self.max_table,
                    max_large=self.max_large, log=self.log)


def run_sequence(dev, eps, seed, nops, sizes=(24, 16, 7), async_ingest=False, via_host=False, stop_after=None,
                 model_fault=None, caps=None, weights=None):
    """One sequence of `nops` operations, reproducible from (eps, seed) and the
    keyword settings; `stop_after` ends it after that many steps (replay of a
    failure up to the step before it).  Returns the model-side counters."""
    return Sequence(dev, eps, seed, nops, tuple(sizes), async_ingest, via_host, stop_after, model_fault, caps,
                    weights).run()


# ------------------------------------------------------------- configurations
# name -> settings of run_sequence, the environment of the device test, and the
# seeds: `gpu_seeds` run on both engines, `cpu_seeds` on the host engine only
SHORT_LADDER = "128,256,512,4096b"
CONFIGS = collections.OrderedDict([
    ("default", dict(eps=[0.1, 0.01], env={}, kw={}, nops=130, gpu_seeds=[1, 2, 3], cpu_seeds=[4, 5])),
    ("short_ladder", dict(eps=[0.01], env={"GK_CAPS": SHORT_LADDER}, kw=dict(caps=SHORT_LADDER), nops=130,
                          gpu_seeds=[11, 12, 13, 14], cpu_seeds=[15, 16])),
    # (six seeds: every kind follows each of the three calls left in flight, 81 pairs)
    ("tiny_arenas", dict(eps=[0.01], env={"GK_CAPS": SHORT_LADDER, "GK_POOL_SLOTS": "2"},
                         kw=dict(async_ingest=True, caps=SHORT_LADDER,
                                 weights=dict(ingest=18.0, ingest_keyed=15.0, rank_ingest_keyed=14.0)),
                         nops=130, gpu_seeds=[21, 22, 23, 24, 27, 37], cpu_seeds=[25, 26])),
    ("no_small_class", dict(eps=[0.001], env={}, kw=dict(sizes=(8, 6, 4)), nops=120, gpu_seeds=[31, 32, 33, 36, 41],
                            cpu_seeds=[34, 35])),
    ("via_host", dict(eps=[0.01], env={}, kw=dict(via_host=True), nops=130, gpu_seeds=[41, 42, 43, 44, 48],
                      cpu_seeds=[45])),
    # 64-sample chunks of k_rank_keyed / k_rank_ingest_keyed at batches of a few hundred samples: runs of one
    # stream start on, straddle and span a chunk; the keyed kinds weighted up, ingests left in flight
    ("keyed_chunks", dict(eps=[0.01], env={"GK_CAPS": SHORT_LADDER, "GK_RANKK_CHUNK": "64"},
                          kw=dict(async_ingest=True, caps=SHORT_LADDER,
                                  weights=dict(ingest_keyed=14.0, ranks_keyed=10.0, cdf_keyed=5.0,
                                               rank_ingest_keyed=18.0)),
                          nops=130, gpu_seeds=[51, 53, 55, 56, 58], cpu_seeds=[52])),
])
LAST_BOUNDED_CAPACITY = 512  # of SHORT_LADDER: the class above it is the unbounded kernel's


def runs(name, seeds):
    cfg = CONFIGS[name]
    return [(eps, seed) for eps in cfg["eps"] for seed in cfg[seeds]]


def required_events(name):
    ev = list(EVENTS)
    if all(class0_capacity(eps) == 128 for eps in CONFIGS[name]["eps"]):
        ev.append("table_at_capacity")  # (a table of exactly cap[t] entries: the first that does not fit class t)
    if CONFIGS[name]["kw"].get("async_ingest"):
        ev += ["after_async:" + k for k in KINDS]
        ev += ["after_async:%s:%s" % (src, k) for src in ASYNC_SOURCES for k in KINDS]
    return ev
