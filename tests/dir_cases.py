"""Shared cases of the key directory (gk_dir_* / KeyDirectory / KeyedStreamSet),
run by tests/test_cpu_dir.py on the host engine and tests/test_gpu_dir.py on
the MI355X.  Test infrastructure only.

The reference for ids is ``Model``: a Python dict that literally runs the loop
of include/gk_capi.h; answers are compared bit for bit (int32 ids, int64
keys).  The end-to-end case compares every key's stream with an ``OracleGK``
fed that key's values in arrival order, under parity_util's strict comparison.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import parity_util as U
from gk_oracle import OracleGK
from rank_cases import expected_ranks

NONE = -2 ** 63
I64_MAX = 2 ** 63 - 1


def _pkg():
    import gkarray_amd
    return gkarray_amd


def _L():
    from gkarray_amd import _lib
    return _lib


def new_dir(capacity, dev):
    return _pkg().KeyDirectory(capacity, device=dev)


def t64(ks):
    return torch.from_numpy(np.asarray(ks, dtype=np.int64).reshape(-1))


def spread(r):
    """Pool indices to keys all over int64 (both signs), one to one."""
    r = np.asarray(r, dtype=np.uint64)
    return (r * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x7F4A7C15)).view(np.int64)


class Model:
    """The loop of gk_capi.h on a dict."""

    def __init__(self, capacity):
        self.capacity = capacity
        self.d = {}
        self.keys = []

    def assign(self, ks):
        """ids (int32 array), or None for a void call (the model stays as it was)."""
        d, keys = dict(self.d), list(self.keys)
        out = []
        for k in np.asarray(ks, dtype=np.int64).tolist():
            if k == NONE:
                out.append(-1)
                continue
            i = d.get(k)
            if i is None:
                if len(keys) == self.capacity:
                    return None
                i = d[k] = len(keys)
                keys.append(k)
            out.append(i)
        self.d, self.keys = d, keys
        return np.asarray(out, dtype=np.int32)

    def lookup(self, ks):
        return np.asarray([self.d.get(k, -1) for k in np.asarray(ks, dtype=np.int64).tolist()], dtype=np.int32)


def same_ids(got, exp, what):
    assert got.dtype == torch.int32, (what, got.dtype)
    got = got.cpu().numpy()
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if got.tobytes() != exp.tobytes():
        bad = np.flatnonzero(got != exp)
        raise AssertionError("%s: %d ids differ, first at %d: %d vs %d"
                             % (what, len(bad), bad[0], got[bad[0]], exp[bad[0]]))


def check_same(d, m, what):
    """size and keys() of the directory against the model."""
    assert len(d) == len(m.keys), (what, len(d), len(m.keys))
    got = d.keys()
    assert got.dtype == torch.int64
    assert got.cpu().numpy().tobytes() == np.asarray(m.keys, dtype=np.int64).tobytes(), what + ": keys()"


def check_assign(d, m, ks, what):
    """One batch through directory and model: ids, num_new, size, keys(); a
    batch the model refuses must be refused as GK_E_OVERFLOW and change nothing."""
    L = _L()
    before = len(m.keys)
    exp = m.assign(ks)
    if exp is None:
        with pytest.raises(L.GKBackendError) as e:
            d.assign(t64(ks))
        assert e.value.code == L.GK_E_OVERFLOW, (what, e.value)
    else:
        same_ids(d.assign(t64(ks)), exp, what)
        assert d.last_new == len(m.keys) - before, (what, d.last_new)
    check_same(d, m, what)
    return exp


def check_lookup(d, m, ks, what):
    same_ids(d.lookup(t64(ks)), m.lookup(ks), what + " lookup")
    check_same(d, m, what + " after lookup")


# ---------------------------------------------------------------- 1. sizes
COUNTS = [0, 1, 63, 64, 65, 2047, 2048, 2049, 200000]
CAPACITIES = [1, 32, 2 ** 17]


def case_sizes(dev, count):
    """One count, every capacity, a pool smaller and one larger than the count."""
    rng = np.random.default_rng(1000 + count)
    for capacity in CAPACITIES:
        for pool in (max(count // 7, 1), 3 * count + 5):
            d, m = new_dir(capacity, dev), Model(capacity)
            assert d.capacity == capacity
            ks = spread(rng.integers(0, pool, count))
            what = "count %d capacity %d pool %d" % (count, capacity, pool)
            check_assign(d, m, ks, what)
            # a second batch over the same pool: known and new keys mixed
            check_assign(d, m, spread(rng.integers(0, pool, min(count, 3000))), what + " second")
            probe = np.concatenate([ks[:500], spread(np.arange(pool, pool + 50))])
            check_lookup(d, m, probe, what)
            d.close()


# ------------------------------------------------------------- 2. ordering
def case_ordering(dev):
    rng = np.random.default_rng(2)
    multiset = spread(rng.integers(0, 700, 5000))
    orders = [np.sort(multiset), np.sort(multiset)[::-1].copy(), rng.permutation(multiset), rng.permutation(multiset)]
    for j, ks in enumerate(orders):
        d, m = new_dir(1024, dev), Model(1024)
        for c, part in enumerate(np.array_split(ks, 3)):  # three calls continue the numbering
            exp = check_assign(d, m, part, "order %d call %d" % (j, c))
            # ids follow first occurrence: the ids this call created, in batch order, are consecutive
            _, first = np.unique(exp, return_index=True)
            fresh = exp[np.sort(first)]
            fresh = fresh[fresh >= len(m.keys) - d.last_new]
            assert np.array_equal(fresh, np.arange(len(m.keys) - d.last_new, len(m.keys))), (j, c)
        d.close()


# ----------------------------------------------------------- 3. contention
def case_contention(dev, which):
    if which == "one":
        ks, capacity = np.full(200000, 77, dtype=np.int64), 32
    elif which == "three":
        ks, capacity = np.tile(np.asarray([5, -9, 1 << 40], dtype=np.int64), 66667)[:200000], 32
    else:  # 65 536 distinct keys, each exactly twice, the second copies in reverse order
        a = spread(np.arange(65536))
        ks, capacity = np.concatenate([a, a[::-1]]), 2 ** 17
    d, m = new_dir(capacity, dev), Model(capacity)
    check_assign(d, m, ks, which)
    check_assign(d, m, ks[::-1].copy(), which + " again")  # every key known
    check_lookup(d, m, ks[:1000], which)
    d.close()


# ------------------------------------------------- 4. worst-case chains
def case_chains(dev):
    """The caller has set GK_DIR_HASH_BITS: capacity 32 (64 slots) filled to
    exactly 32 keys over 3 calls, then all of them and 32 strangers looked up."""
    d, m = new_dir(32, dev), Model(32)
    keys = spread(np.arange(32))
    check_assign(d, m, keys[:11], "chain call 0")
    check_assign(d, m, np.concatenate([keys[5:22], keys[:3]]), "chain call 1")
    check_assign(d, m, np.concatenate([keys[31:21:-1], keys[:32]]), "chain call 2")
    assert len(d) == 32
    check_lookup(d, m, np.concatenate([keys, spread(np.arange(100, 132))]), "chain")
    check_assign(d, m, keys[::-1].copy(), "chain known keys on a full directory")
    check_assign(d, m, np.concatenate([keys[:4], spread([999])]), "chain overflow")  # void, rebuilt
    check_lookup(d, m, np.concatenate([keys, spread(np.arange(100, 132))]), "chain after the void call")
    d.close()


# ---------------------------------------------------------- 5. GK_DIR_NONE
def case_none(dev):
    d, m = new_dir(32, dev), Model(32)
    check_assign(d, m, [NONE, NONE, NONE], "only NONE")
    assert len(d) == 0 and d.last_new == 0
    ks = [NONE, -1, 0, I64_MAX, NONE + 1, NONE, -1, 0, I64_MAX, NONE + 1, NONE]
    exp = check_assign(d, m, ks, "special keys")
    assert exp.tolist() == [-1, 0, 1, 2, 3, -1, 0, 1, 2, 3, -1]
    assert d.last_new == 4
    check_assign(d, m, [NONE] * 70, "only NONE on a filled directory")
    assert len(d) == 4 and d.last_new == 0
    check_lookup(d, m, [NONE, 0, -1, NONE + 1, I64_MAX, 1, NONE + 2, I64_MAX - 1], "special keys")
    d.close()


# ------------------------------------------------------ 6. overflow is void
def case_overflow(dev):
    L = _L()
    d, m = new_dir(32, dev), Model(32)
    old = spread(np.arange(20))
    check_assign(d, m, old, "fill 20")
    for n_new in (13, 1000):
        fresh = spread(np.arange(5000, 5000 + n_new))
        ks = np.concatenate([old[:7], fresh[: n_new // 2], old[7:], fresh[n_new // 2:]])
        assert m.assign(ks) is None  # (the model refuses it too)
        with pytest.raises(L.GKBackendError) as e:
            d.assign(t64(ks))
        assert e.value.code == L.GK_E_OVERFLOW
        check_same(d, m, "after a void call of %d new keys" % n_new)
        assert len(d) == 20
        check_lookup(d, m, np.concatenate([old, fresh[:40]]), "after a void call of %d new keys" % n_new)
    exp = check_assign(d, m, spread(np.arange(7000, 7012)), "12 new keys")
    assert exp.tolist() == list(range(20, 32))
    check_assign(d, m, np.concatenate([old, spread(np.arange(7000, 7012))]), "known keys on a full directory")
    check_assign(d, m, spread([8000]), "one key too many")
    d.close()


# ---------------------------------------------------------------- 7. import
def case_import(dev):
    L = _L()
    rng = np.random.default_rng(7)
    d, m = new_dir(600, dev), Model(600)
    check_assign(d, m, spread(rng.integers(0, 400, 3000)), "fill")
    other = new_dir(600, dev)
    check_assign(other, Model(600), spread(np.arange(900, 950)), "other's old contents")
    other.import_keys(d.keys())
    check_same(other, m, "round trip")
    probe = np.concatenate([np.asarray(m.keys[:300], dtype=np.int64), spread(np.arange(900, 950))])
    check_lookup(other, m, probe, "round trip")
    m2 = Model(600)
    m2.d, m2.keys = dict(m.d), list(m.keys)
    batch = spread(rng.integers(300, 500, 500))
    check_assign(d, m, batch, "original continues")
    check_assign(other, m2, batch, "copy continues")
    assert m.keys == m2.keys

    # refusals: GK_E_ARG, the old contents stay
    keys = np.asarray(m.keys[:50], dtype=np.int64)
    for bad, needle in ((np.concatenate([keys[:30], keys[10:12], keys[3:4]]), "keys[30] repeats key %d" % keys[10]),
                        (np.concatenate([keys[:9], [NONE], keys[9:]]), "keys[9] is GK_DIR_NONE"),
                        (spread(np.arange(601)), "601")):
        with pytest.raises(L.GKBackendError) as e:
            d.import_keys(t64(bad))
        assert e.value.code == L.GK_E_ARG and needle in str(e.value), (needle, str(e.value))
        check_same(d, m, "after a refused import")
        check_lookup(d, m, probe, "after a refused import")

    # resized: larger, equal, too small
    for cap in (2048, len(d)):
        r = d.resized(cap)
        assert r.capacity == cap
        check_same(r, m, "resized to %d" % cap)
        check_lookup(r, m, probe, "resized to %d" % cap)
        r.close()
    with pytest.raises(L.GKBackendError) as e:
        d.resized(len(d) - 1)
    assert e.value.code == L.GK_E_ARG
    check_same(d, m, "after a refused resize")
    d.import_keys(t64([]))
    assert len(d) == 0 and d.keys().numel() == 0
    d.close()
    other.close()


# ------------------------------------------------------- 8. argument errors
def case_arguments(dev):
    L = _L()
    cpu = torch.device(dev).type == "cpu"
    lib = L.load_cpu() if cpu else L.load()
    index = 0 if cpu else torch.device(dev).index or 0
    for capacity in (0, -1, 2 ** 30 + 1):
        h = ctypes.c_void_p()
        assert lib.gk_dir_create(capacity, index, ctypes.byref(h)) == L.GK_E_ARG and not h.value, capacity
    d = new_dir(8, dev)
    k = t64([1, 2, 3]).to(d.device)
    out = torch.empty(3, dtype=torch.int32, device=d.device)
    kp, op = ctypes.c_void_p(k.data_ptr()), ctypes.c_void_p(out.data_ptr())
    assert lib.gk_dir_assign(d.handle, kp, -1, op, None, None) == L.GK_E_ARG
    assert lib.gk_dir_assign(d.handle, kp, 2 ** 31, op, None, None) == L.GK_E_ARG
    assert lib.gk_dir_assign(d.handle, None, 3, op, None, None) == L.GK_E_ARG
    assert lib.gk_dir_assign(d.handle, kp, 3, None, None, None) == L.GK_E_ARG
    assert lib.gk_dir_lookup(d.handle, kp, -1, op, None) == L.GK_E_ARG
    assert lib.gk_dir_lookup(d.handle, None, 3, op, None) == L.GK_E_ARG
    assert lib.gk_dir_lookup(d.handle, kp, 3, None, None) == L.GK_E_ARG
    assert lib.gk_dir_import(d.handle, None, 3, None) == L.GK_E_ARG
    assert lib.gk_dir_import(d.handle, kp, -1, None) == L.GK_E_ARG
    assert lib.gk_dir_assign(None, kp, 3, op, None, None) == L.GK_E_ARG
    assert lib.gk_dir_size(None) == -1 and lib.gk_dir_capacity(None) == -1
    assert len(d) == 0
    # count == 0 with NULL arrays is valid
    assert lib.gk_dir_assign(d.handle, None, 0, None, None, None) == L.GK_OK
    assert lib.gk_dir_lookup(d.handle, None, 0, None, None) == L.GK_OK
    assert lib.gk_dir_keys(d.handle, None, None) == L.GK_OK
    assert lib.gk_dir_import(d.handle, None, 0, None) == L.GK_OK
    assert d.assign(t64([])).numel() == 0 and d.lookup(t64([])).numel() == 0
    new = ctypes.c_int64(-5)
    assert lib.gk_dir_assign(d.handle, kp, 3, op, ctypes.byref(new), None) == L.GK_OK and new.value == 3
    assert out.cpu().tolist() == [0, 1, 2]
    d.close()


def case_symbols():
    L = _L()
    names = ["gk_dir_create", "gk_dir_destroy", "gk_dir_capacity", "gk_dir_size", "gk_dir_assign", "gk_dir_lookup",
             "gk_dir_keys", "gk_dir_import"]
    for n in names:
        assert n in L.SYMBOLS and n in L.CPU_SYMBOLS, n
    cpu = L.load_cpu()
    for n in names:
        assert hasattr(cpu, n), n


# ------------------------------------------------------------ 9. end to end
QS = [0.0, 0.01, 0.25, 0.5, 0.75, 0.99, 1.0]
XS = [-1.0, 0.0, 0.2, 0.5, 1.0, 2.5, 40.0]


def _oracle_add(oracles, eps, ks, vs):
    for k, v in zip(np.asarray(ks, dtype=np.int64).tolist(), np.asarray(vs, dtype=np.float64).tolist()):
        if k == NONE:
            continue
        o = oracles.get(k)
        if o is None:
            o = oracles[k] = OracleGK(eps)
        o.add(v)


def check_keyed(kss, oracles, what):
    """quantiles, ranks and stats of EVERY key against its oracle (strict)."""
    keys = list(oracles)
    assert len(kss) == len(keys), what
    assert sorted(kss.keys().cpu().tolist()) == sorted(keys), what
    kt = t64(keys)
    got_q = kss.quantiles(kt, QS).cpu().numpy()
    exp_q = np.asarray([oracles[k].quantiles(QS) for k in keys], dtype=np.float64)
    U.assert_same_quantiles(got_q, exp_q, what + " quantiles", None)
    lo, hi = kss.ranks(kt, XS)
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    st = {n: v.cpu().numpy() for n, v in kss.stats(kt).items()}
    for j, k in enumerate(keys):
        o = oracles[k]
        if o.n > 0:
            o.size()
        elo, ehi = expected_ranks(o, XS)
        assert lo[j].tobytes() == elo.tobytes() and hi[j].tobytes() == ehi.tobytes(), (what, k, "ranks")
        assert int(st["n"][j]) == o.n and int(st["size"][j]) == len(o.v) and int(st["pending"][j]) == len(o.pending), \
            (what, k, "counts")
        got = np.asarray([st["min"][j], st["max"][j], st["sum"][j], st["avg"][j]], dtype=np.float64)
        exp = np.asarray([o.min, o.max, o.sum, o.avg], dtype=np.float64)
        assert got.tobytes() == exp.tobytes(), (what, k, "stats", got, exp)


def _batch(rng, lo, hi, n):
    """n samples over the keys spread(lo .. hi), a few of them GK_DIR_NONE."""
    ks = spread(rng.integers(lo, hi, n))
    ks[rng.integers(0, n, 5)] = NONE
    return ks, np.round(rng.lognormal(0, 1, n), 3)


def case_end_to_end(dev, eps, tmp_path):
    P = _pkg()
    L = _L()
    rng = np.random.default_rng(int(1 / eps))
    kss = P.KeyedStreamSet(eps, capacity=4, device=dev)
    oracles = {}
    # about 300 distinct keys over five calls: 4 -> 512 streams, several doublings
    for c, (lo, hi) in enumerate([(0, 3), (0, 40), (20, 130), (100, 300), (0, 300)]):
        ks, vs = _batch(rng, lo, hi, 2500)
        kss.add(t64(ks), torch.from_numpy(vs))
        _oracle_add(oracles, eps, ks, vs)
        assert len(kss) == len(oracles), c
        assert kss.streams.num_streams == kss.directory.capacity
    assert 280 <= len(kss) <= 300 and kss.directory.capacity == 512
    check_keyed(kss, oracles, "after five adds")

    # unknown keys
    stranger = int(spread([100000])[0])
    known = int(kss.keys()[3].item())
    assert known in kss and stranger not in kss
    for call in (lambda k: kss.quantiles(k, QS), lambda k: kss.ranks(k, XS), lambda k: kss.cdf(k, XS), kss.stats,
                 kss.flush, kss.reset):
        with pytest.raises(KeyError) as e:
            call(t64([known, stranger, stranger + 1]))
        assert e.value.args[0] == stranger
    check_keyed(kss, oracles, "after refused queries")

    # a fused query answers for every key, row id for keys()[id]
    ks, vs = _batch(rng, 0, 300, 1500)
    q = kss.add(t64(ks), torch.from_numpy(vs), quantiles=QS).cpu().numpy()
    _oracle_add(oracles, eps, ks, vs)
    order = kss.keys().cpu().tolist()
    U.assert_same_quantiles(q, np.asarray([oracles[k].quantiles(QS) for k in order]), "fused query", None)

    # reset restarts only the listed keys, which keep their binding
    victims = order[5:60:3]
    ids_before = kss.directory.lookup(t64(victims)).cpu().tolist()
    kss.reset(t64(victims))
    for k in victims:
        oracles[k] = OracleGK(eps)
    assert kss.directory.lookup(t64(victims)).cpu().tolist() == ids_before
    check_keyed(kss, oracles, "after reset")
    ks, vs = _batch(rng, 0, 300, 1500)
    kss.add(t64(ks), torch.from_numpy(vs))
    _oracle_add(oracles, eps, ks, vs)
    check_keyed(kss, oracles, "reset keys continue")

    # cdf is (lo + hi) / (2 n) of ranks
    kt = t64(order[:20])
    lo_, hi_ = kss.ranks(kt, XS)
    n = kss.stats(kt)["n"]
    exp_cdf = (lo_ + hi_).to(torch.float64) / (2.0 * n.to(torch.float64)).unsqueeze(1)
    assert kss.cdf(kt, XS).cpu().numpy().tobytes() == exp_cdf.cpu().numpy().tobytes()

    # save / load continues bit for bit (pending values are saved unflushed)
    ks, vs = _batch(rng, 250, 330, 700)  # (some new keys, and pending values in many streams)
    kss.add(t64(ks), torch.from_numpy(vs))
    _oracle_add(oracles, eps, ks, vs)
    path = os.path.join(str(tmp_path), "keyed.gk")
    kss.save(path)
    assert os.path.exists(path) and os.path.exists(path + ".keys.npy")
    back = P.KeyedStreamSet.load(path, device=dev)
    assert back.keys().cpu().tolist() == kss.keys().cpu().tolist()
    assert back.directory.capacity == kss.directory.capacity
    ks, vs = _batch(rng, 200, 340, 1500)
    for x in (kss, back):
        x.add(t64(ks), torch.from_numpy(vs))
    _oracle_add(oracles, eps, ks, vs)
    check_keyed(back, oracles, "loaded copy")
    check_keyed(kss, oracles, "original after save")
    back.close()
    kss.close()

    # max_streams
    small = P.KeyedStreamSet(eps, capacity=4, device=dev, max_streams=10)
    o2 = {}
    ks, vs = spread(np.arange(10).repeat(30)), np.round(rng.random(300), 3)
    small.add(t64(ks), torch.from_numpy(vs))
    _oracle_add(o2, eps, ks, vs)
    assert len(small) == 10 and small.directory.capacity == 10 and small.streams.num_streams == 10
    with pytest.raises(L.GKBackendError) as e:
        small.add(t64(spread([3, 4, 10, 5])), torch.ones(4, dtype=torch.float64))
    assert e.value.code == L.GK_E_OVERFLOW
    assert len(small) == 10 and small.directory.capacity == 10 and small.streams.num_streams == 10
    check_keyed(small, o2, "after a batch max_streams refused")
    small.add(t64(ks[::-1].copy()), torch.from_numpy(vs))
    _oracle_add(o2, eps, ks[::-1], vs)
    check_keyed(small, o2, "known keys at max_streams")
    small.close()


# ---------------------------------------------------------- 10. cross-engine
def case_cross_engine(dev):
    rng = np.random.default_rng(10)
    g, c = new_dir(4096, dev), new_dir(4096, "cpu")
    for j, (pool, n) in enumerate([(50, 3000), (3000, 5000), (6000, 2049), (3000, 70000)]):
        ks = spread(rng.integers(0, pool, n))
        ks[rng.integers(0, n, 3)] = NONE
        try:
            a = g.assign(t64(ks)).cpu().numpy()
        except _L().GKBackendError as e:
            a = e.code
        try:
            b = c.assign(t64(ks)).numpy()
        except _L().GKBackendError as e:
            b = e.code
        assert type(a) is type(b), (j, a, b)
        if isinstance(a, np.ndarray):
            assert a.tobytes() == b.tobytes(), j
            assert g.last_new == c.last_new
        assert g.keys().cpu().numpy().tobytes() == c.keys().numpy().tobytes(), j
        assert g.lookup(t64(ks)).cpu().numpy().tobytes() == c.lookup(t64(ks)).numpy().tobytes(), j
    g.close()
    c.close()
