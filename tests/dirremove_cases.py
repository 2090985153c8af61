"""Shared cases of key removal and id recycling (gk_dir_remove, gk_dir_bound,
gk_dir_import_sparse; KeyDirectory.remove / KeyedStreamSet.remove, discard,
pop), run by tests/test_cpu_dir_remove.py on the host engine and
tests/test_gpu_dir_remove.py on the MI355X.  Test infrastructure only.

The reference is ``Model``: the loops of include/gk_capi.h on a dict, a list
with holes and a set of free ids.  Everything is compared bit for bit: int32
ids, int64 keys, len, bound, last_new, last_removed.  The end-to-end case
compares every live key's stream with an ``OracleGK`` of its own.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import dir_cases as D
import parity_util as U

NONE = D.NONE
spread, t64, new_dir, same_ids = D.spread, D.t64, D.new_dir, D.same_ids


def _L():
    from gkarray_amd import _lib
    return _lib


class Model:
    """gk_dir_assign / gk_dir_remove / gk_dir_import_sparse of gk_capi.h."""

    def __init__(self, capacity):
        self.capacity = capacity
        self.d = {}
        self.keys = []     # keys[id], NONE at free ids; len(keys) is bound
        self.free = set()

    def copy(self, capacity=None):
        m = Model(self.capacity if capacity is None else capacity)
        m.d, m.keys, m.free = dict(self.d), list(self.keys), set(self.free)
        return m

    @property
    def bound(self):
        return len(self.keys)

    def __len__(self):
        return len(self.d)

    def assign(self, ks):
        """ids (int32 array), or None for a void call (the model stays as it was)."""
        d, keys, free = dict(self.d), list(self.keys), set(self.free)
        ascending = iter(sorted(free))  # (the call only takes ids from the set: min(free) is the next of these)
        out = []
        for k in np.asarray(ks, dtype=np.int64).tolist():
            if k == NONE:
                out.append(-1)
                continue
            i = d.get(k)
            if i is None:
                if free:
                    i = next(ascending)
                    free.remove(i)
                    keys[i] = k
                elif len(keys) < self.capacity:
                    i = len(keys)
                    keys.append(k)
                else:
                    return None
                d[k] = i
            out.append(i)
        self.d, self.keys, self.free = d, keys, free
        return np.asarray(out, dtype=np.int32)

    def remove(self, ks):
        out = []
        for k in np.asarray(ks, dtype=np.int64).tolist():
            if k == NONE or k not in self.d:
                out.append(-1)
                continue
            i = self.d.pop(k)
            self.keys[i] = NONE
            self.free.add(i)
            out.append(i)
        return np.asarray(out, dtype=np.int32)

    def lookup(self, ks):
        return np.asarray([self.d.get(k, -1) for k in np.asarray(ks, dtype=np.int64).tolist()], dtype=np.int32)

    def import_sparse(self, ks):
        ks = np.asarray(ks, dtype=np.int64).tolist()
        self.keys = list(ks)
        self.d = {k: i for i, k in enumerate(ks) if k != NONE}
        self.free = {i for i, k in enumerate(ks) if k == NONE}


def check_same(d, m, what):
    """len, bound and keys() of the directory against the model."""
    assert len(d) == len(m), (what, len(d), len(m))
    assert d.bound == m.bound, (what, d.bound, m.bound)
    assert len(m) + len(m.free) == m.bound <= m.capacity
    got = d.keys()
    assert got.dtype == torch.int64 and got.numel() == m.bound, what
    assert got.cpu().numpy().tobytes() == np.asarray(m.keys, dtype=np.int64).tobytes(), what + ": keys()"


def check_assign(d, m, ks, what, must_fit=False):
    L = _L()
    before = len(m)
    exp = m.assign(ks)
    assert exp is not None or not must_fit, what + ": the model refuses a batch that must fit"
    if exp is None:
        with pytest.raises(L.GKBackendError) as e:
            d.assign(t64(ks))
        assert e.value.code == L.GK_E_OVERFLOW, (what, e.value)
    else:
        same_ids(d.assign(t64(ks)), exp, what)
        assert d.last_new == len(m) - before, (what, d.last_new)
    check_same(d, m, what)
    return exp


def check_remove(d, m, ks, what):
    before = len(m)
    exp = m.remove(ks)
    same_ids(d.remove(t64(ks)), exp, what + " remove")
    assert d.last_removed == before - len(m), (what, d.last_removed)
    check_same(d, m, what + " after remove")
    return exp


def check_lookup(d, m, ks, what):
    same_ids(d.lookup(t64(ks)), m.lookup(ks), what + " lookup")
    check_same(d, m, what + " after lookup")


# ---------------------------------------------------------------- 1. sizes
COUNTS = [0, 1, 63, 64, 65, 2047, 2048, 2049, 200000]
CAPACITIES = [1, 32, 2 ** 17]


def case_sizes(dev, count):
    """Fill; remove `count` samples, half known keys and half strangers with
    GK_DIR_NONE mixed in; assign old, removed and fresh keys; look all up."""
    rng = np.random.default_rng(3000 + count)
    for capacity in CAPACITIES:
        what = "count %d capacity %d" % (count, capacity)
        d, m = new_dir(capacity, dev), Model(capacity)
        check_assign(d, m, spread(np.arange(capacity)), what + " fill", must_fit=True)
        victims = spread(rng.integers(0, 2 * capacity, count))
        if count:
            victims[rng.integers(0, count, 1 + count // 50)] = NONE
        gone = check_remove(d, m, victims, what)
        removed = victims[gone >= 0]
        back = removed[: len(removed) // 2]
        fresh = spread(np.arange(5 * capacity, 5 * capacity + len(removed) - len(back)))
        held = np.asarray(list(m.d), dtype=np.int64)
        old = held[rng.integers(0, len(held), min(count, 1000))] if len(held) else held
        batch = rng.permutation(np.concatenate([old, back, fresh, back, [NONE]]))
        check_assign(d, m, batch, what + " assign", must_fit=True)
        # more new keys than there are ids left: void
        check_assign(d, m, np.concatenate([old[:5], spread(np.arange(9 * capacity, 9 * capacity + 3))]), what + " void")
        probe = np.concatenate([victims[:2000], batch[:2000], spread(np.arange(capacity)[:2000]), [NONE]])
        check_lookup(d, m, probe, what)
        d.close()


# ------------------------------------------------------- 2. recycling order
def case_recycling(dev):
    rng = np.random.default_rng(2)
    base = spread(np.arange(32))
    fresh = spread(np.arange(100, 106))
    orders = {"ascending": np.sort(fresh), "descending": np.sort(fresh)[::-1].copy(), "shuffled": rng.permutation(fresh)}
    for name, order in orders.items():
        for split in (False, True):
            d, m = new_dir(64, dev), Model(64)
            check_assign(d, m, base, name + " fill", must_fit=True)
            # ids 3, 17, 4, 30 freed in this order, over two calls
            assert check_remove(d, m, base[[3, 17]], name).tolist() == [3, 17]
            assert check_remove(d, m, base[[4, 30]], name).tolist() == [4, 30]
            assert len(d) == 28 and d.bound == 32
            # each fresh key twice, old keys in between
            batch = np.concatenate([order[:3], base[5:9], order[:3][::-1], order[3:], base[20:22], order[3:]])
            parts = [batch[:10], batch[10:]] if split else [batch]
            got = {}
            for c, part in enumerate(parts):
                ids = check_assign(d, m, part, "%s split %s call %d" % (name, split, c), must_fit=True)
                for k, i in zip(part.tolist(), ids.tolist()):
                    got.setdefault(k, i)
            assert [got[k] for k in order.tolist()] == [3, 4, 17, 30, 32, 33], (name, split)
            assert len(d) == 34 and d.bound == 34
            d.close()


# ------------------------------------------- 3. duplicates in a remove batch
def case_duplicates(dev, which):
    if which == "one":
        d, m = new_dir(32, dev), Model(32)
        check_assign(d, m, spread(np.arange(10)), which, must_fit=True)
        ks = np.full(200000, spread([6])[0], dtype=np.int64)
        got = check_remove(d, m, ks, which)
        assert got[0] == 6 and (got[1:] == -1).all() and d.last_removed == 1
        check_remove(d, m, ks[:70], which + " again")  # (nothing left to remove)
        assert d.last_removed == 0
    elif which == "twice":
        a = spread(np.arange(65536))
        d, m = new_dir(2 ** 17, dev), Model(2 ** 17)
        check_assign(d, m, np.concatenate([a, spread(np.arange(70000, 70100))]), which, must_fit=True)
        got = check_remove(d, m, np.concatenate([a, a[::-1]]), which)
        assert np.array_equal(got[:65536], np.arange(65536)) and (got[65536:] == -1).all()
        assert len(d) == 100 and d.bound == 65636
        check_lookup(d, m, np.concatenate([a[:1000], spread(np.arange(70000, 70100))]), which)
    else:  # one key removed and assigned again across five calls: the smallest free id each time
        d, m = new_dir(32, dev), Model(32)
        base = spread(np.arange(12))
        check_assign(d, m, base, which, must_fit=True)
        check_remove(d, m, base[[9, 2, 5]], which)
        k = base[5:6]
        for c, also in enumerate([[7], [0, 1], [], [11], [3]]):
            smallest = min(m.free)
            assert check_assign(d, m, k, "%s call %d" % (which, c), must_fit=True).tolist() == [smallest]
            check_remove(d, m, np.concatenate([k, base[also], k]), "%s call %d" % (which, c))
        check_lookup(d, m, base, which)
    d.close()


# ------------------------------------------------------ 4. tombstone chains
def case_chains(dev, half):
    """The caller has set GK_DIR_HASH_BITS: capacity 32 (64 slots), generations
    of keys that come and go.  Removed keys keep their slots until a rebuild:
    without one the third generation finds no slot."""
    d, m = new_dir(32, dev), Model(32)
    strangers = spread(np.arange(5000, 5032))
    if not half:
        for g in range(5):
            keys = spread(np.arange(32 * g, 32 * g + 32))
            check_assign(d, m, np.concatenate([keys[:20], keys[10:]]), "generation %d" % g, must_fit=True)
            assert len(d) == 32
            check_lookup(d, m, np.concatenate([keys, strangers]), "generation %d" % g)
            check_remove(d, m, keys[::-1].copy(), "generation %d" % g)
            assert len(d) == 0 and d.bound == 32
    else:
        check_assign(d, m, spread(np.arange(32)), "first keys", must_fit=True)
        for r in range(8):
            check_remove(d, m, spread(np.arange(16 * r, 16 * r + 16)), "round %d" % r)
            check_assign(d, m, spread(np.arange(16 * r + 32, 16 * r + 48)), "round %d" % r, must_fit=True)
            assert len(d) == 32 and d.bound == 32
            check_lookup(d, m, np.concatenate([spread(np.arange(16 * r, 16 * r + 48)), strangers]), "round %d" % r)
    d.close()


# ------------------------------------------- 5. overflow stays void with holes
def case_overflow(dev):
    L = _L()
    d, m = new_dir(32, dev), Model(32)
    base = spread(np.arange(32))
    check_assign(d, m, base, "fill", must_fit=True)
    check_remove(d, m, base[[20, 1, 8, 31, 14]], "five")
    before = d.keys().cpu().numpy().tobytes()
    probe = np.concatenate([base, spread(np.arange(900, 910))])
    ids_before = d.lookup(t64(probe)).cpu().numpy().tobytes()
    six = np.concatenate([base[2:5], spread(np.arange(900, 903)), base[:2], spread(np.arange(903, 906))])
    assert m.copy().assign(six) is None
    with pytest.raises(L.GKBackendError) as e:
        d.assign(t64(six))
    assert e.value.code == L.GK_E_OVERFLOW
    assert d.keys().cpu().numpy().tobytes() == before
    assert d.bound == 32 and len(d) == 27
    assert d.lookup(t64(probe)).cpu().numpy().tobytes() == ids_before
    check_same(d, m, "after the void call")
    five = spread(np.arange(903, 908))
    got = check_assign(d, m, np.concatenate([five, base[2:5], five[::-1]]), "five new keys", must_fit=True)
    assert got[:5].tolist() == [1, 8, 14, 20, 31]
    assert d.bound == 32 and len(d) == 32
    check_assign(d, m, spread([999]), "one key too many")
    d.close()


# ----------------------------------------------------------- 6. sparse import
def _with_holes(dev, capacity, rng):
    d, m = new_dir(capacity, dev), Model(capacity)
    check_assign(d, m, spread(rng.integers(0, 400, 3000)), "fill", must_fit=True)
    check_remove(d, m, spread(rng.integers(0, 800, 300)), "holes")
    assert 0 < len(m.free) < m.bound
    return d, m


def case_sparse_import(dev):
    L = _L()
    rng = np.random.default_rng(6)
    d, m = _with_holes(dev, 600, rng)
    other = new_dir(600, dev)
    check_assign(other, Model(600), spread(np.arange(900, 950)), "other's old contents", must_fit=True)
    other.import_keys(d.keys(), sparse=True)
    m2 = m.copy()
    check_same(other, m2, "round trip")
    probe = np.concatenate([spread(np.arange(0, 400)), spread(np.arange(900, 950))])
    check_lookup(other, m2, probe, "round trip")
    for c in range(3):  # both continue alike
        ks = spread(rng.integers(300, 500, 400))
        check_assign(d, m, ks, "original continues %d" % c, must_fit=True)
        check_assign(other, m2, ks, "copy continues %d" % c, must_fit=True)
        ks = spread(rng.integers(0, 500, 60))
        check_remove(d, m, ks, "original continues %d" % c)
        check_remove(other, m2, ks, "copy continues %d" % c)
        assert m.keys == m2.keys
    other.close()

    # resized: larger, and exactly bound
    for cap in (2048, d.bound):
        r = d.resized(cap)
        mr = m.copy(cap)
        assert r.capacity == cap
        check_same(r, mr, "resized to %d" % cap)
        check_lookup(r, mr, probe, "resized to %d" % cap)
        check_assign(r, mr, spread(np.arange(2000, 2000 + len(m.free))), "resized to %d fills its holes" % cap,
                     must_fit=True)
        assert r.bound == m.bound
        r.close()

    # refusals: GK_E_ARG, the old contents stay
    keys = np.asarray([k for k in m.keys if k != NONE][:50], dtype=np.int64)
    repeat = np.concatenate([keys[:9], [NONE, NONE], keys[9:30], keys[10:12], keys[3:4]])
    for call, needle in ((lambda: d.import_keys(t64(repeat), sparse=True), "keys[32] repeats key %d" % keys[10]),
                         (lambda: d.import_keys(t64(np.full(601, NONE)), sparse=True), "601"),
                         (lambda: d.resized(d.bound - 1), str(d.bound)),
                         (lambda: d.import_keys(t64(repeat[:20])), "keys[9] is GK_DIR_NONE")):
        with pytest.raises(L.GKBackendError) as e:
            call()
        assert e.value.code == L.GK_E_ARG and needle in str(e.value), (needle, str(e.value))
        check_same(d, m, "after a refusal")
        check_lookup(d, m, probe, "after a refusal")

    # only holes, and nothing at all
    d.import_keys(t64([NONE, NONE, NONE]), sparse=True)
    m.import_sparse([NONE, NONE, NONE])
    check_same(d, m, "three free ids")
    assert check_assign(d, m, spread([1, 2, 1, 3, 4]), "into three free ids", must_fit=True).tolist() == [0, 1, 0, 2, 3]
    d.import_keys(t64([]), sparse=True)
    assert len(d) == 0 and d.bound == 0 and d.keys().numel() == 0
    d.close()


# ------------------------------------------------------- 7. argument errors
NAMES = ["gk_dir_remove", "gk_dir_bound", "gk_dir_import_sparse"]


def case_arguments(dev):
    L = _L()
    cpu = torch.device(dev).type == "cpu"
    lib = L.load_cpu() if cpu else L.load()
    d = new_dir(8, dev)
    d.assign(t64([1, 2, 3]))
    k = t64([1, 2, 3]).to(d.device)
    out = torch.empty(3, dtype=torch.int32, device=d.device)
    kp, op = ctypes.c_void_p(k.data_ptr()), ctypes.c_void_p(out.data_ptr())
    assert lib.gk_dir_remove(d.handle, kp, -1, op, None, None) == L.GK_E_ARG
    assert lib.gk_dir_remove(d.handle, kp, 2 ** 31, op, None, None) == L.GK_E_ARG
    assert lib.gk_dir_remove(d.handle, None, 3, op, None, None) == L.GK_E_ARG
    assert lib.gk_dir_remove(d.handle, kp, 3, None, None, None) == L.GK_E_ARG
    assert lib.gk_dir_remove(None, kp, 3, op, None, None) == L.GK_E_ARG
    assert lib.gk_dir_import_sparse(d.handle, None, 3, None) == L.GK_E_ARG
    assert lib.gk_dir_import_sparse(d.handle, kp, -1, None) == L.GK_E_ARG
    assert lib.gk_dir_import_sparse(d.handle, kp, 2 ** 31, None) == L.GK_E_ARG
    assert lib.gk_dir_import_sparse(None, kp, 3, None) == L.GK_E_ARG
    assert lib.gk_dir_bound(None) == -1
    assert len(d) == 3 and d.bound == 3
    # count == 0 with NULL arrays is valid
    gone = ctypes.c_int64(-5)
    assert lib.gk_dir_remove(d.handle, None, 0, None, ctypes.byref(gone), None) == L.GK_OK and gone.value == 0
    assert d.remove(t64([])).numel() == 0 and d.last_removed == 0
    assert len(d) == 3
    assert lib.gk_dir_remove(d.handle, kp, 3, op, None, None) == L.GK_OK  # (num_removed may be NULL)
    assert out.cpu().tolist() == [0, 1, 2]
    assert len(d) == 0 and d.bound == 3
    assert lib.gk_dir_remove(d.handle, kp, 3, op, ctypes.byref(gone), None) == L.GK_OK and gone.value == 0
    assert out.cpu().tolist() == [-1, -1, -1]
    assert lib.gk_dir_import_sparse(d.handle, None, 0, None) == L.GK_OK
    assert len(d) == 0 and d.bound == 0
    assert lib.gk_dir_keys(d.handle, None, None) == L.GK_OK
    d.close()


def case_symbols():
    L = _L()
    for n in NAMES:
        assert n in L.SYMBOLS and n in L.CPU_SYMBOLS, n
    cpu = ctypes.CDLL(L.CPU_LIB_PATH)
    for n in NAMES:
        assert hasattr(cpu, n), n


# ------------------------------------------- 8. random operation sequences
def _seq_batch(rng, capacity):
    """0 to 3000 samples over a window of the key pool (3 x capacity keys)."""
    n = int(rng.integers(0, 3001)) if rng.random() < 0.3 else int(rng.integers(0, 200))
    width = int(rng.integers(1, capacity + 1))
    lo = int(rng.integers(0, 3 * capacity - width + 1))
    ks = spread(rng.integers(lo, lo + width, n))
    if n and rng.random() < 0.5:
        ks[rng.integers(0, n, 3)] = NONE
    return ks


def case_sequences(dev, capacity, seed):
    L = _L()
    rng = np.random.default_rng(8000 + 10 * capacity + seed)
    d, m = new_dir(capacity, dev), Model(capacity)
    voids = 0
    for step in range(200):
        what = "capacity %d seed %d step %d" % (capacity, seed, step)
        op = rng.choice(["assign", "assign", "remove", "remove", "lookup", "keys", "resized", "sparse", "void"])
        if op == "assign":
            voids += check_assign(d, m, _seq_batch(rng, capacity), what) is None
        elif op == "remove":
            check_remove(d, m, _seq_batch(rng, capacity), what)
        elif op == "lookup":
            check_lookup(d, m, _seq_batch(rng, capacity), what)
        elif op == "keys":
            check_same(d, m, what)
        elif op == "resized":
            cap = int(rng.integers(max(m.bound, 1), 2 * capacity + 1))
            r = d.resized(cap)
            d.close()
            d, m = r, m.copy(cap)
            check_same(d, m, what + " resized")
        elif op == "sparse":
            other = new_dir(m.capacity, dev)
            other.import_keys(d.keys(), sparse=True)
            d.close()
            d = other
            check_same(d, m, what + " sparse round trip")
        else:  # more distinct strangers than ids are left, old keys among them
            left = m.capacity - len(m)
            ks = np.concatenate([_seq_batch(rng, capacity)[:50], spread(np.arange(10 ** 6, 10 ** 6 + left + 1))])
            assert check_assign(d, m, rng.permutation(ks), what + " void") is None
            voids += 1
    assert voids > 0
    check_lookup(d, m, spread(np.arange(3 * capacity)), "capacity %d seed %d: the whole pool" % (capacity, seed))
    d.close()


# ------------------------------------------------------------ 9. cross-engine
def case_cross_engine(dev):
    rng = np.random.default_rng(9)
    g, c = new_dir(4096, dev), new_dir(4096, "cpu")

    def both(op, ks):
        res = []
        for x in (g, c):
            try:
                res.append(getattr(x, op)(t64(ks)).cpu().numpy().tobytes())
            except _L().GKBackendError as e:
                res.append(e.code)
        assert res[0] == res[1], (op, len(ks))
        assert (g.last_new, g.last_removed, len(g), g.bound) == (c.last_new, c.last_removed, len(c), c.bound)
        assert g.keys().cpu().numpy().tobytes() == c.keys().numpy().tobytes(), op

    for pool, n in [(3000, 5000), (6000, 2049), (3000, 70000), (9000, 900), (9000, 9000)]:
        ks = spread(rng.integers(0, pool, n))
        ks[rng.integers(0, n, 3)] = NONE
        both("assign", ks)
        both("remove", spread(rng.integers(0, pool, n // 2)))
        both("lookup", ks)
    g.close()
    c.close()


# ------------------------------------------ 10. KeyedStreamSet end to end
QS, XS = D.QS, D.XS


class _Live:
    """A KeyedStreamSet as dir_cases.check_keyed reads one, free ids left out."""

    def __init__(self, kss):
        self.kss = kss
        self.quantiles, self.ranks, self.stats = kss.quantiles, kss.ranks, kss.stats

    def __len__(self):
        return len(self.kss)

    def keys(self):
        k = self.kss.keys()
        return k[k != NONE]


def check_keyed(kss, oracles, what):
    assert kss.directory.capacity == 128 and kss.streams.num_streams == 128, what
    assert kss.keys().numel() == kss.directory.bound
    D.check_keyed(_Live(kss), oracles, what)


def _check_fused(kss, q, oracles, what):
    keys = kss.keys().cpu().tolist()
    assert q.shape == (kss.directory.bound, len(QS)), (what, q.shape)
    live = [i for i, k in enumerate(keys) if k != NONE]
    assert len(live) == len(oracles)
    exp = np.asarray([oracles[keys[i]].quantiles(QS) for i in live], dtype=np.float64)
    U.assert_same_quantiles(q[live], exp, what, None)


def case_end_to_end(dev, eps, tmp_path):
    import gkarray_amd as P
    rng = np.random.default_rng(10 + int(1 / eps))
    kss = P.KeyedStreamSet(eps, capacity=128, device=dev)
    oracles = {}
    keepers = spread(np.arange(100000, 100010))  # never removed
    strangers = spread(np.arange(200000, 200020))

    def feed(x, ks, n=2500, fused=False):
        ks = ks[rng.integers(0, len(ks), n)]
        ks[rng.integers(0, n, 5)] = NONE
        vs = np.round(rng.lognormal(0, 1, n), 3)
        for s in x:
            q = s.add(t64(ks), torch.from_numpy(vs), quantiles=QS if fused else None)
        D._oracle_add(oracles, eps, ks, vs)
        return q

    for g in range(10):
        # 100 keys, 40 of them the generation before's: removed keys that come back
        gen = spread(np.arange(60 * g, 60 * g + 100))
        q = feed([kss], np.concatenate([gen, keepers]), fused=g == 7)
        what = "generation %d" % g
        if g == 7:
            _check_fused(kss, q.cpu().numpy(), oracles, what + " fused query")
        check_keyed(kss, oracles, what)
        live = np.asarray([k for k in oracles if k not in set(keepers.tolist())], dtype=np.int64)
        assert 90 <= len(live) <= 100
        if g == 2:
            # an unknown key: KeyError names it, nothing changes
            for call in (kss.remove, kss.pop):
                with pytest.raises(KeyError) as e:
                    call(t64(np.concatenate([live[:3], strangers[4:6], live[3:]])))
                assert e.value.args[0] == int(strangers[4])
            check_keyed(kss, oracles, what + " after refused removals")
        if g == 4:
            out = kss.pop(t64(live), device="cpu")
            assert out.device.type == "cpu" and out.num_streams == len(live)
            exp = np.asarray([oracles[k].quantiles(QS) for k in live.tolist()], dtype=np.float64)
            U.assert_same_quantiles(out.quantiles(QS).numpy(), exp, what + " popped streams", None)
            st = out.stats()
            for j, k in enumerate(live.tolist()):
                o = oracles[k]
                assert int(st["n"][j]) == o.n and float(st["sum"][j]) == o.sum, (what, k)
            out.close()
        elif g % 2:
            kss.discard(t64(np.concatenate([strangers[:5], live, [NONE], live[:7], strangers])))
        else:
            kss.remove(t64(np.concatenate([live, live[:9]])))  # (a key listed twice is removed once)
        for k in live.tolist():
            del oracles[k]
        assert len(kss) == 10 and int(live[0]) not in kss and int(keepers[0]) in kss
        check_keyed(kss, oracles, what + " after removal")

    # save / load with holes continues bit for bit
    feed([kss], np.concatenate([spread(np.arange(700, 730)), keepers]), n=700)
    assert len(kss) < kss.directory.bound
    path = os.path.join(str(tmp_path), "holes.gk")
    kss.save(path)
    back = P.KeyedStreamSet.load(path, device=dev)
    assert back.keys().cpu().numpy().tobytes() == kss.keys().cpu().numpy().tobytes()
    assert (len(back), back.directory.bound) == (len(kss), kss.directory.bound)
    q = feed([kss, back], np.concatenate([spread(np.arange(715, 780)), keepers]), n=1500, fused=True)
    _check_fused(back, q.cpu().numpy(), oracles, "loaded copy fused query")
    assert back.keys().cpu().numpy().tobytes() == kss.keys().cpu().numpy().tobytes()
    check_keyed(back, oracles, "loaded copy")
    check_keyed(kss, oracles, "original after save")
    back.close()
    kss.close()


def case_growth(dev):
    """_assign_growing on a directory with holes: both halves double, the
    holes are filled first and the streams of surviving keys move with their ids."""
    import gkarray_amd as P
    kss = P.KeyedStreamSet(0.01, capacity=4, device=dev)
    kss.add(t64([10, 11, 12, 13]), torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64))
    kss.remove(t64([11, 13]))
    assert (len(kss), kss.directory.bound, kss.directory.capacity) == (2, 4, 4)
    kss.add(t64([20, 21, 22, 23, 24]), torch.tensor([5.0, 6.0, 7.0, 8.0, 9.0], dtype=torch.float64))
    assert (len(kss), kss.directory.bound, kss.directory.capacity, kss.streams.num_streams) == (7, 7, 8, 8)
    assert kss.keys().cpu().tolist() == [10, 20, 12, 21, 22, 23, 24]
    got = kss.quantiles(t64([10, 12, 20, 21, 24]), [0.5]).cpu().flatten().tolist()
    assert got == [1.0, 3.0, 5.0, 6.0, 9.0]
    kss.add(t64([11]), torch.tensor([42.0], dtype=torch.float64))  # a removed key comes back: a new sketch
    assert kss.quantiles(t64([11]), [0.5]).cpu().tolist() == [[42.0]]
    assert kss.stats(t64([11]))["n"].cpu().tolist() == [1]
    kss.close()
