"""Random operation sequences on one ``KeyedStreamSet`` against ``{key:
OracleGK}`` and ``dirremove_cases.Model`` for the ids, shared by
tests/test_gpu_keyedseq.py (device engine) and tests/test_cpu_keyedseq.py (host
engine); the engine is the ``dev`` parameter.  The scheme is that of
opseq_cases: a generator seeded by ``(eps, seed)`` alone, every answer compared
strictly, and after EVERY operation ``keys()`` by bytes, ``len`` / ``bound`` /
``capacity`` / ``streams.num_streams`` against the model and EVERY id of the
stream set bit for bit against an oracle (``select_cases.assert_all``): the
key's own, or a fresh ``OracleGK`` for a free id and for every id >= bound -- a
removed key leaves nothing behind.  New keys get the smallest free ids in order
of first occurrence and ids survive growth, on both engines alike.

The object starts at ``capacity=8`` and doubles several times, also with holes;
keys come from a pool of 60 ``spread`` keys, so that removed keys come back.
Value batches mix short random series with descending runs aimed at a few keys
(one that has just inherited a recycled id preferred), whose tables climb
classes.  ``compact`` and the check after every operation are those of
opseq_cases (``compact_with_floors``, ``usage_above_floors``) on
``kss.streams`` with a class floor per id.

The model side restates nothing: ``dirremove_cases.Model``,
``keyed_cases.oracle_loop``, ``rankingest_cases.oracle_step``,
``rankkeyed_cases.expected_rows``, ``rank_cases.expected_rows`` /
``flush_covered``, ``select_cases.oracle_answers``,
``rollup_cases.assert_set_matches``.  Events are counted on the model only.
``model_fault`` makes the MODEL wrong in one small way
(tests/test_cpu_keyedseq.py requires that each is noticed).  Test
infrastructure only."""
import collections
import copy
import os
import tempfile

import numpy as np
import pytest
import torch

import dirremove_cases as DR
import keyed_cases as KC
import opseq_cases as O
import parity_util as U
import rank_cases as K
import rankingest_cases as RI
import rankkeyed_cases as Q
import rollup_cases as R
import select_cases as C
from gk_oracle import OracleGK, flush_period

NONE = DR.NONE
POOL = DR.spread(np.arange(60))
STRANGERS = DR.spread(np.arange(1000, 1012))  # never bound

WEIGHTS = collections.OrderedDict([
    ("add", 24.0), ("score_add", 12.0), ("score", 5.0), ("ranks_keyed", 4.0), ("quantiles", 5.0), ("ranks", 3.5),
    ("cdf", 3.0), ("stats", 3.0), ("flush", 4.0), ("reset", 3.0), ("remove", 7.0), ("discard", 5.0), ("pop", 5.0),
    ("compact", 6.0), ("save_load", 3.0)])
KINDS = list(WEIGHTS)
EVENTS = ["recycled_id_inherits_large_class", "growth_with_holes", "key_returns_after_removal",
          "compact_demotes_after_removal", "score_add_binds_new_key", "pop_large_to_host",
          "grows_class_on_recycled_id"]
FAULTS = ["remove_keeps_state", "recycle_largest_free_id", "score_add_scores_after_add", "growth_renumbers_ids"]
QS = [0.0, 0.25, 0.5, 0.9, 1.0]


class KeyedSequence:
    def __init__(self, dev, eps, seed, nops, max_streams, caps, stop_after, model_fault):
        import gkarray_amd as P
        self.pkg = P
        self.dev, self.eps, self.seed, self.nops, self.max_streams = dev, eps, seed, nops, max_streams
        self.steps = nops if stop_after is None else min(nops, stop_after)
        assert model_fault is None or model_fault in FAULTS, model_fault
        self.fault = model_fault
        self.P = flush_period(eps)
        self.caps = O.ladder(eps, caps)
        self.cap0 = self.caps[0]
        self.limit = 3000
        self.rng = np.random.default_rng([int(seed), self.P, 77])
        self.kss = P.KeyedStreamSet(eps, capacity=8, device=dev, max_streams=max_streams)
        self.check_ladder()
        self.m = DR.Model(8)
        self.orc = {}                 # key -> OracleGK
        self.ghost = {}               # id -> oracle a faulty model keeps at a free id
        self.floor = [0] * 8          # per id, as opseq_cases holds it per stream
        self.renew_floor = False
        self.was_removed = set()      # keys removed at some time
        self.recycled = set()         # ids that went to a new key after a removal (on this stream set)
        self.fresh_heirs = []         # keys that have just inherited a recycled id: targets of the next runs
        self.removal_ids = set()      # ids freed since the last compaction
        self.nruns = 0
        self.log = []
        self.ran = collections.Counter()
        self.events = collections.Counter()
        self.max_table = 0
        self.max_capacity = 8

    # ------------------------------------------------------------- small helpers
    def check_ladder(self):
        ss = self.kss.streams
        if not ss.is_cpu:
            assert [ss.capacity(c) for c in range(len(self.caps) + 1)] == self.caps + [-1]

    def fresh(self):
        return OracleGK(self.eps)

    def by_id(self):
        """One oracle per id of the stream set: the key's, or a fresh one."""
        out = []
        for i in range(self.m.capacity):
            k = self.m.keys[i] if i < self.m.bound else NONE
            out.append(self.orc[k] if k != NONE else self.ghost.get(i) or self.fresh())
        return out

    def live(self):
        return [k for k in self.m.keys if k != NONE]

    def large(self, o):
        return len(o.v) > self.cap0

    def t64(self, ks):
        return DR.t64(ks).to(self.dev)

    def tf(self, x):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).to(self.dev)

    def some_live(self, lo=1, hi=8, repeat=True, large=0.4):
        """A few live keys, unsorted; one repeats at times."""
        rng, live = self.rng, self.live()
        if not live:
            return np.zeros(0, np.int64)
        n = int(rng.integers(lo, min(len(live), hi) + 1))
        ks = [int(k) for k in rng.choice(live, n, replace=False)]
        big = [k for k in live if self.large(self.orc[k])]
        if big and rng.random() < large:
            b = int(rng.choice(big))
            ks = [b] + [k for k in ks if k != b][:max(n - 1, 0)]
        if repeat and rng.random() < 0.3:
            ks.insert(int(rng.integers(0, len(ks) + 1)), int(rng.choice(ks)))
        return np.asarray(ks, dtype=np.int64)

    def with_unknown(self, ks):
        """ks with a key the object does not hold put in; returns (keys, the first unknown one)."""
        rng = self.rng
        gone = [int(k) for k in POOL if int(k) not in self.m.d]
        pool = gone[:6] + [int(k) for k in STRANGERS]
        bad = [int(k) for k in rng.choice(pool, int(rng.integers(1, 3)), replace=False)]
        out = [int(k) for k in ks]
        for b in bad:
            out.insert(int(rng.integers(0, len(out) + 1)), b)
        first = next(k for k in out if k not in self.m.d)
        return np.asarray(out, dtype=np.int64), first

    def unchanged(self, call, exc, what):
        """A refused call: raises `exc` and leaves the objects and the keys as they were
        (the states are compared after every operation anyway)."""
        d0, s0 = self.kss.directory, self.kss.streams
        keys0 = self.kss.keys().cpu().numpy().tobytes()
        with pytest.raises(exc) as ei:
            call()
        assert self.kss.directory is d0 and self.kss.streams is s0, what
        assert self.kss.keys().cpu().numpy().tobytes() == keys0, what
        return ei.value

    # ---------------------------------------------------------- the id model
    def model_assign(self, ks):
        """The ids of a batch as _assign_growing gives them: both halves double
        until the batch fits; None when max_streams refuses it (nothing changes)."""
        m = self.m
        free0 = set(m.free)
        grew = False
        while True:
            ids = m.assign(ks)
            if ids is not None:
                break
            cap = m.capacity
            if self.max_streams is not None and cap >= self.max_streams:
                return None
            new_cap = 2 * cap if self.max_streams is None else min(2 * cap, self.max_streams)
            if self.fault == "growth_renumbers_ids":
                grown = DR.Model(new_cap)
                grown.import_sparse([k for k in m.keys if k != NONE])
                m = grown
            else:
                m = m.copy(new_cap)
            grew = True
        new = [k for k in dict.fromkeys(np.asarray(ks, dtype=np.int64).tolist()) if k != NONE and k not in self.orc]
        if self.fault == "recycle_largest_free_id" and m.free:
            took = [k for k in new if m.d[k] in free0]
            if took and max(m.free) > m.d[took[-1]]:
                k, j = took[-1], max(m.free)
                i = m.d[k]
                m.keys[i], m.keys[j], m.d[k] = NONE, k, j
                m.free.remove(j)
                m.free.add(i)
                ids = m.lookup(ks)
        if grew:
            if free0:
                self.events["growth_with_holes"] += 1
            # (streams.resized: a new stream set, whose classes start at fit of the tables)
            self.renew_floor = True
            self.recycled.clear()
            self.removal_ids.clear()
            self.ghost = {}
            self.max_capacity = max(self.max_capacity, m.capacity)
        floor = [0] * m.capacity if grew else self.floor
        for k in new:
            i = m.d[k]
            self.orc[k] = self.fresh()
            self.ghost.pop(i, None)
            if k in self.was_removed:
                self.events["key_returns_after_removal"] += 1
            if i in free0 and not grew:
                self.recycled.add(i)
                self.fresh_heirs.append(k)
                if floor[i] > 0:
                    self.events["recycled_id_inherits_large_class"] += 1
        self.m = m
        return ids

    def model_remove(self, ks):
        gone = self.m.remove(ks)
        for k, i in zip(np.asarray(ks, dtype=np.int64).tolist(), gone.tolist()):
            if i >= 0:
                o = self.orc.pop(k)
                if self.fault == "remove_keeps_state":
                    self.ghost[i] = o
                self.was_removed.add(k)
                self.removal_ids.add(i)
                self.recycled.discard(i)
        self.fresh_heirs = [k for k in self.fresh_heirs if k in self.orc]

    # ------------------------------------------------------------- value batches
    def batch(self, args, nan_row=False):
        """(keys, values) of an add / score_add: samples of a window of the pool
        (new, known and returning keys), a few NO_KEY, at times every key of the
        pool; at times a descending run for one or two keys among them."""
        rng = self.rng
        vseed = int(rng.integers(1 << 30))
        vr = np.random.default_rng(vseed)
        r = rng.random()
        N = 0 if r < 0.06 else int(vr.integers(1, 4)) if r < 0.14 else int(vr.integers(8, 3 * self.P + 8))
        r = rng.random()
        holes = bool(self.m.free) and self.m.capacity < (self.max_streams or len(POOL))
        if r < (0.3 if holes else 0.06):
            # every key of the pool (the more often while free ids wait below a capacity that can still double)
            window, mode = POOL, "flood"
        elif r < 0.45 and self.live():
            live = np.asarray(self.live(), dtype=np.int64)
            window, mode = vr.choice(live, min(len(live), int(rng.integers(1, 9))), replace=False), "known"
        else:
            w = int(rng.integers(2, 14))
            lo = int(rng.integers(0, len(POOL) - w + 1))
            window, mode = POOL[lo:lo + w], "window"
        ks = np.asarray(window, dtype=np.int64)[vr.integers(0, len(window), N)]
        vs = np.asarray(U.gen(int(vr.integers(0, 8)), N, vr), dtype=np.float64)
        runs = []
        if N and rng.random() < 0.4 and not nan_row:
            # descending runs below everything seen so far: the tables of their keys climb classes
            heirs = [k for k in self.fresh_heirs if len(self.orc[k].v) < self.limit - 700]
            known = [k for k in self.live() if len(self.orc[k].v) < self.limit - 700]
            for _ in range(int(rng.integers(1, 3))):
                if heirs and rng.random() < 0.7:
                    k = heirs.pop(0)
                    self.fresh_heirs.remove(k)
                elif known and rng.random() < 0.8:
                    k = max(known, key=lambda k: len(self.orc[k].v)) if rng.random() < 0.5 else int(rng.choice(known))
                else:
                    k = int(rng.choice(POOL))
                units = int(rng.integers(2, 8)) if rng.random() < 0.85 else int(rng.integers(20, 60))
                L = units * self.P + int(rng.integers(0, self.P))
                self.nruns += 1
                runs.append((int(k), L))
                where = np.sort(vr.integers(0, len(ks) + 1, L))
                ks = np.insert(ks, where, k)
                vs = np.insert(vs, where, -1e6 * self.nruns - np.arange(float(L)))
        if len(ks):
            ks[vr.random(len(ks)) < 0.04] = NONE
        args.update(vseed=vseed, N=len(ks), mode=mode, runs=runs)
        return ks, vs

    def check_fused(self, q, qs, single, what):
        """Row id of the fused answers for keys()[id]; the row of a free id answers as an empty stream."""
        by = self.by_id()[:self.m.bound]
        assert tuple(q.shape) == (self.m.bound, len(qs)), (what, q.shape)
        U.assert_same_quantiles(q.cpu().numpy(), C.oracle_answers(by, range(len(by)), qs, single), what, None)

    def qs(self):
        rng = self.rng
        qs = [float(q) for q in rng.choice(QS + [float(rng.random())], int(rng.integers(1, 5)), replace=False)]
        return qs, bool(rng.random() < 0.4)

    def refused_by_max(self, call, args):
        from gkarray_amd._lib import GK_E_OVERFLOW, GKBackendError
        args["refused"] = True
        self.events["refused_by_max_streams"] += 1
        e = self.unchanged(call, GKBackendError, "refused by max_streams")
        assert e.code == GK_E_OVERFLOW, e

    # --------------------------------------------------------------- operations
    def op_add(self, args):
        rng, kss = self.rng, self.kss
        ks, vs = self.batch(args)
        query = rng.random() < 0.3
        qs, single = self.qs() if query else (None, False)
        args.update(qs=qs, single=single)
        call = lambda: kss.add(self.t64(ks), self.tf(vs), quantiles=qs, single=single)  # noqa: E731
        ids = self.model_assign(ks)
        if ids is None:
            return self.refused_by_max(call, args)
        got = call()
        KC.oracle_loop(self.by_id(), ids, vs)
        if query:
            self.check_fused(got, qs, single, "add: fused answers")
        else:
            assert got is None

    def op_score_add(self, args):
        from gkarray_amd._lib import GK_E_ARG, GKBackendError
        rng, kss = self.rng, self.kss
        nan_row = bool(rng.random() < 0.12)
        ks, vs = self.batch(args, nan_row=nan_row)
        query = rng.random() < 0.3
        qs, single = self.qs() if query else (None, False)
        keyed = np.flatnonzero(ks != NONE)
        nan_row = nan_row and len(keyed) > 0
        if nan_row:
            vs[int(rng.choice(keyed))] = float("nan")
        args.update(qs=qs, single=single, nan_row=nan_row)
        call = lambda: kss.score_add(self.t64(ks), self.tf(vs), quantiles=qs, single=single)  # noqa: E731
        new = {k for k in ks.tolist() if k != NONE and k not in self.orc}
        ids = self.model_assign(ks)
        if ids is None:
            return self.refused_by_max(call, args)
        if new:
            self.events["score_add_binds_new_key"] += 1
        if nan_row:
            # GK_E_ARG from the call itself: nothing is added, the new keys stay bound with empty sketches
            with pytest.raises(GKBackendError) as ei:
                call()
            assert ei.value.code == GK_E_ARG, ei.value
            return
        got = call()
        by = self.by_id()
        il, xl = ids.tolist(), vs.tolist()
        if self.fault == "score_add_scores_after_add":
            ahead = copy.deepcopy(by)
            KC.oracle_loop(ahead, ids, vs)
            K.flush_covered(ahead, {i for i in il if i >= 0})
            rows = Q.expected_rows(ahead, il, xl)
            RI.oracle_step(by, il, xl)
        else:
            rows = RI.oracle_step(by, il, xl)  # every sample against its key's history, then the batch
        score = got[0] if query else got
        exp = self.score_of(rows)
        born = np.asarray([k in new for k in ks.tolist()], dtype=bool)
        assert np.isnan(exp[born]).all()  # (a key new in the batch scores NaN on all its samples)
        U.assert_same_quantiles(score.cpu().numpy(), exp, "score_add", None)
        if query:
            self.check_fused(got[1], qs, single, "score_add: fused answers")

    @staticmethod
    def score_of(rows):
        lo, hi, n = rows
        with np.errstate(invalid="ignore", divide="ignore"):
            return (lo + hi).astype(np.float64) / (2.0 * n.astype(np.float64))

    def sample_query(self, args):
        """(keys, xs) of score / ranks_keyed: live keys, unknown ones and NO_KEY; thresholds the sketches hold."""
        rng = self.rng
        live = self.live()
        pool = live + [int(k) for k in STRANGERS[:3]] + [int(k) for k in POOL[:4]] + [NONE]
        N = int(rng.integers(0, 4)) if rng.random() < 0.2 else int(rng.integers(4, 3 * self.P))
        ks = np.asarray([pool[j] for j in rng.integers(0, len(pool), N)], dtype=np.int64)
        xs = np.zeros(N)
        for j, k in enumerate(ks.tolist()):
            o = self.orc.get(k)
            cand = [0.0, float("inf"), float("-inf"), float(rng.normal(0, 3))]
            if o is not None and o.n:
                cand += [o.min, o.max] + ([o.v[len(o.v) // 2]] if o.v else []) + o.pending[-1:]
            xs[j] = cand[int(rng.integers(0, len(cand)))]
            if o is None and rng.random() < 0.4:
                xs[j] = float("nan")
        args.update(N=N, unknown=int(sum(1 for k in ks.tolist() if k not in self.m.d)))
        return ks, xs

    def op_score(self, args, ranks=False):
        ks, xs = self.sample_query(args)
        if ranks:
            got = self.kss.ranks_keyed(self.t64(ks), self.tf(xs))
        else:
            got = self.kss.score(self.t64(ks), self.tf(xs))
        ids = self.m.lookup(ks)  # (no key is bound: an unknown key and NO_KEY are "no stream")
        by = self.by_id()
        K.flush_covered(by, {i for i in ids.tolist() if i >= 0})
        rows = Q.expected_rows(by, ids.tolist(), xs.tolist())
        if ranks:
            Q.same_i64(got[0], rows[0], "ranks_keyed lo")
            Q.same_i64(got[1], rows[1], "ranks_keyed hi")
        else:
            U.assert_same_quantiles(got.cpu().numpy(), self.score_of(rows), "score", None)

    def op_ranks_keyed(self, args):
        self.op_score(args, ranks=True)

    def by_key(self, args, call, expect):
        """A query by key: on live keys `expect(ids)` checks the answer; with an
        unknown key among them it raises KeyError naming the first, nothing changed."""
        ks = self.some_live()
        if self.rng.random() < 0.2 or not len(ks):
            ks, first = self.with_unknown(ks)
            args.update(keys=len(ks), unknown=first)
            e = self.unchanged(lambda: call(self.t64(ks)), KeyError, "unknown key")
            assert e.args[0] == first, (e.args, first)
            return None
        args.update(keys=len(ks))
        got = call(self.t64(ks))
        expect(got, self.m.lookup(ks).tolist())
        return ks

    def op_quantiles(self, args):
        qs, single = self.qs()
        args.update(qs=qs, single=single)

        def expect(got, ids):
            exp = C.oracle_answers(self.by_id(), ids, qs, single)
            U.assert_same_quantiles(got.cpu().numpy(), exp, "quantiles", None)
        self.by_key(args, lambda k: self.kss.quantiles(k, qs, single=single), expect)

    def thresholds(self):
        rng = self.rng
        pool = [float("inf"), float("-inf"), 0.0, -0.0] + [float(x) for x in rng.normal(0, 3, 3)]
        for o in list(self.orc.values())[:4]:
            if o.n:
                pool += [o.min, o.max]
        return [pool[j] for j in rng.integers(0, len(pool), int(rng.integers(1, 6)))]

    def op_ranks(self, args, cdf=False):
        xs = self.thresholds()
        args.update(xs=xs)

        def expect(got, ids):
            by = self.by_id()
            K.flush_covered(by, ids)
            lo, hi = K.expected_rows(by, ids, xs)
            if cdf:
                n = np.asarray([by[i].n for i in ids], dtype=np.int64)
                with np.errstate(invalid="ignore", divide="ignore"):
                    exp = (lo + hi).astype(np.float64) / (2.0 * n.astype(np.float64))[:, None]
                U.assert_same_quantiles(got.cpu().numpy(), exp.reshape(tuple(got.shape)), "cdf", None)
            else:
                K.same_i64(got[0], lo, "ranks lo")
                K.same_i64(got[1], hi, "ranks hi")
        self.by_key(args, (lambda k: self.kss.cdf(k, xs)) if cdf else (lambda k: self.kss.ranks(k, xs)), expect)

    def op_cdf(self, args):
        self.op_ranks(args, cdf=True)

    def op_stats(self, args):
        def expect(got, ids):
            by = self.by_id()
            st = {k: v.cpu().numpy() for k, v in got.items()}
            for k, f in (("n", lambda o: o.n), ("size", lambda o: len(o.v)), ("pending", lambda o: len(o.pending))):
                assert st[k].tolist() == [f(by[i]) for i in ids], "stats " + k
            for k in ("min", "max", "sum", "avg"):
                exp = np.asarray([getattr(by[i], k) for i in ids], dtype=np.float64)
                assert st[k].tobytes() == exp.tobytes(), "stats " + k
        self.by_key(args, self.kss.stats, expect)

    def op_flush(self, args):
        def expect(got, ids):
            K.flush_covered(self.by_id(), ids)
        self.by_key(args, self.kss.flush, expect)

    def op_reset(self, args):
        ks = self.by_key(args, self.kss.reset, lambda got, ids: None)
        for k in set([] if ks is None else ks.tolist()):
            self.orc[k] = self.fresh()  # (the key keeps its binding, and its stream its class)

    def op_remove(self, args):
        ks = self.some_live(hi=10)
        if self.rng.random() < 0.25 and len(self.live()) > 12:
            ks = np.asarray(self.rng.permutation(self.live())[:len(self.live()) // 2], dtype=np.int64)
        if self.rng.random() < 0.15 or not len(ks):
            ks, first = self.with_unknown(ks)
            args.update(keys=len(ks), unknown=first)
            e = self.unchanged(lambda: self.kss.remove(self.t64(ks)), KeyError, "remove of an unknown key")
            assert e.args[0] == first, (e.args, first)
            return
        args.update(keys=len(ks))
        self.kss.remove(self.t64(ks))  # (a key listed twice is removed once)
        self.model_remove(ks)

    def op_discard(self, args):
        rng = self.rng
        ks = [int(k) for k in self.some_live(hi=10)]
        for extra in [int(k) for k in STRANGERS[:int(rng.integers(0, 4))]] + [NONE] * int(rng.integers(0, 3)):
            ks.insert(int(rng.integers(0, len(ks) + 1)), extra)
        ks = np.asarray(ks, dtype=np.int64)
        args.update(keys=len(ks))
        self.kss.discard(self.t64(ks))  # (strangers and NO_KEY are ignored)
        self.model_remove(ks)

    def op_pop(self, args):
        ks = self.some_live(hi=8, repeat=False, large=0.8)
        if not len(ks):
            return self.op_remove(args)
        host = bool(self.rng.random() < 0.5)
        args.update(keys=len(ks), host=host)
        moved = [self.orc[k] for k in ks.tolist()]
        if host and any(self.large(o) for o in moved):
            self.events["pop_large_to_host"] += 1
        out = self.kss.pop(self.t64(ks), device="cpu" if host else None)
        try:
            assert out.num_streams == len(ks) and out.is_cpu == (host or self.kss.streams.is_cpu)
            R.assert_set_matches(out, moved, "the popped set")
        finally:
            out.close()
        self.model_remove(ks)

    def op_compact(self, args):
        by = self.by_id()
        fits = [O.fit(len(o.v), self.caps) for o in by]
        down = {i for i in range(len(by)) if self.floor[i] > fits[i]}
        again = bool(self.rng.random() < 1.0 / 3.0)
        args.update(demotes=sorted(down), again=again)
        if down & self.removal_ids:
            self.events["compact_demotes_after_removal"] += 1
        O.compact_with_floors(self.kss.streams, by, self.floor, self.caps, "compact", again=again)
        self.floor = fits
        self.removal_ids.clear()
        self.recycled.clear()

    def op_save_load(self, args):
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "keyed.gk")
            self.kss.save(path)
            new = self.pkg.KeyedStreamSet.load(path, device=self.dev, max_streams=self.max_streams)
        self.kss.close()
        self.kss = new  # (replaces the object: a new stream set)
        self.check_ladder()
        self.renew_floor = True
        self.recycled.clear()
        self.removal_ids.clear()

    # --------------------------------------------------------------- the driver
    def update_floors(self):
        by = self.by_id()
        fits = [O.fit(len(o.v), self.caps) for o in by]
        if self.renew_floor or len(self.floor) != len(fits):
            self.floor, self.renew_floor = fits, False
        for i, f in enumerate(fits):
            if f > self.floor[i]:
                self.floor[i] = f
                if i in self.recycled:
                    self.events["grows_class_on_recycled_id"] += 1
        self.max_table = max(self.max_table, max(len(o.v) for o in by))
        return by

    def check(self, what):
        kss, m = self.kss, self.m
        got = kss.keys()
        assert got.dtype == torch.int64 and got.numel() == m.bound, what
        assert got.cpu().numpy().tobytes() == np.asarray(m.keys, dtype=np.int64).tobytes(), what + ": keys()"
        assert (len(kss), kss.directory.bound, kss.directory.capacity, kss.streams.num_streams) == \
            (len(m), m.bound, m.capacity, m.capacity), what
        by = self.update_floors()
        C.assert_all(kss.streams, by, what)
        O.usage_above_floors(kss.streams, self.floor, self.caps, what)

    def step(self, k):
        rng = self.rng
        w = np.asarray([WEIGHTS[x] for x in KINDS])
        kind = KINDS[int(rng.choice(len(KINDS), p=w / w.sum()))]
        if kind in ("remove", "discard", "pop") and len(self.m) < 5:
            kind = "add"
        elif kind in ("add", "score_add") and not self.m.free and len(self.m) >= 5 and rng.random() < 0.35 \
                and self.m.capacity < (self.max_streams or len(POOL)):
            kind = "remove"  # (while the object can still double, keys leave early: it doubles with holes)
        args = {}
        self.log.append((k, kind, args))
        getattr(self, "op_" + kind)(args)
        self.ran[kind] += 1
        self.check("after " + kind)

    def describe(self):
        return "\n".join("  %3d %s %r" % (k, kind, args) for k, kind, args in self.log)

    def run(self):
        try:
            for k in range(self.steps):
                try:
                    self.step(k)
                except Exception as e:
                    _, kind, args = self.log[-1]
                    raise AssertionError(
                        "keyedseq eps=%g seed=%d step=%d of %d, %s %r: %s: %s\n(replay the steps before it with "
                        "stop_after=%d) operations so far:\n%s"
                        % (self.eps, self.seed, k, self.nops, kind, args, type(e).__name__, e, k,
                           self.describe())) from e
        finally:
            self.kss.close()
        return dict(ran=self.ran, events=self.events, max_table=self.max_table, max_capacity=self.max_capacity,
                    log=self.log)


def run_sequence(dev, eps, seed, nops, max_streams=None, caps=None, stop_after=None, model_fault=None):
    """One sequence of `nops` operations on a KeyedStreamSet, reproducible from
    (eps, seed) and the keyword settings; `stop_after` ends it after that many
    steps.  Returns the model-side counters."""
    return KeyedSequence(dev, eps, seed, nops, max_streams, caps, stop_after, model_fault).run()


# ------------------------------------------------------------- configurations
CONFIGS = collections.OrderedDict([
    ("default", dict(eps=[0.01, 0.1], env={}, kw={}, nops=100, gpu_seeds=[1, 2, 3], cpu_seeds=[4, 5])),
    ("short_ladder", dict(eps=[0.01], env={"GK_CAPS": O.SHORT_LADDER, "GK_POOL_SLOTS": "2", "GK_RANKK_CHUNK": "64"},
                          kw=dict(caps=O.SHORT_LADDER), nops=100, gpu_seeds=[11, 12, 13], cpu_seeds=[14, 15])),
    ("max_streams", dict(eps=[0.01], env={}, kw=dict(max_streams=48), nops=100, gpu_seeds=[21, 22, 23],
                         cpu_seeds=[24, 25])),
])


def runs(name, seeds):
    cfg = CONFIGS[name]
    return [(eps, seed) for eps in cfg["eps"] for seed in cfg[seeds]]


def required_events(name):
    return EVENTS + (["refused_by_max_streams"] if "max_streams" in CONFIGS[name]["kw"] else [])
