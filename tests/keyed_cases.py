"""Cases of the keyed ingest (gk_group_by_key / gk_ingest_keyed through
StreamSet.group_by_key / ingest_keyed), shared by tests/test_gpu_keyed.py
(device engine) and tests/test_cpu_keyed.py (host engine); the engine is the
``dev`` parameter.  Every comparison is bit for bit (float64 viewed as int64).
Test infrastructure only."""
import numpy as np
import pytest
import torch

import parity_util as U
from gk_oracle import OracleGK
from rollup_cases import assert_set_matches, snapshot

QS = [0.0, 0.5, 0.99, 1.0]

# -0.0, +inf, -inf, the smallest denormal, two NaNs with different payloads
SPECIAL_BITS = np.array([0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x0000000000000001,
                         0x7ff8000000000001, 0xfff4000000000bed], dtype=np.uint64)


# ------------------------------------------------------------ 1. the grouping
def _uniform(rng, S, N, lo=-1):
    return rng.integers(lo, S, N).astype(np.int32)


def _sparse(rng):
    pick = rng.choice(65537, 300, replace=False)
    pick[:2] = [0, 65536]
    ids = pick[rng.integers(0, 300, 5000)]
    ids[:2] = [65536, 0]
    return ids.astype(np.int32)


def _hot(rng):
    ids = rng.integers(0, 1_000_003, 200_000)
    ids[rng.permutation(200_000)[:100_000]] = 777_777
    return ids.astype(np.int32)


# name -> (S, ids builder).  The scatter tile is 4096 samples: N = 20011 spans
# five tiles, 65 two waves of one tile.
GROUP_CASES = {
    "one_stream": (1, lambda rng: np.zeros(20011, np.int32)),
    "n0": (1000, lambda rng: _uniform(rng, 1000, 0)),
    "n1": (1000, lambda rng: _uniform(rng, 1000, 1, lo=0)),
    "n63": (1000, lambda rng: _uniform(rng, 1000, 63)),
    "n64": (1000, lambda rng: _uniform(rng, 1000, 64)),
    "n65": (1000, lambda rng: _uniform(rng, 1000, 65)),
    "skips_second_digit": (257, lambda rng: _uniform(rng, 257, 20011)),
    "third_digit_sparse": (65537, _sparse),
    "round_robin": (4099, lambda rng: (np.arange(10 * 4099 + 3) % 4099).astype(np.int32)),
    "ascending": (4099, lambda rng: np.sort(_uniform(rng, 4099, 30011, lo=0))),
    "descending": (4099, lambda rng: np.sort(_uniform(rng, 4099, 30011, lo=0))[::-1].copy()),
    "hot_key_20_bits": (1_000_003, _hot),
}


def expected_group(ids, vals, S):
    keep = ids >= 0
    order = np.argsort(ids[keep], kind="stable")
    offs = np.zeros(S + 1, np.int64)
    offs[1:] = np.cumsum(np.bincount(ids[keep], minlength=S))
    return vals[keep][order], offs


def sample_values(N, rng):
    """float(i) for sample i (a wrong order inside a stream shows at once); a
    handful overwritten with the special bit patterns."""
    vals = np.arange(N, dtype=np.float64)
    if N >= len(SPECIAL_BITS):
        at = rng.choice(N, len(SPECIAL_BITS), replace=False)
        vals.view(np.uint64)[at] = SPECIAL_BITS
    return vals


def case_group(dev, name, int64_ids=False):
    S, build = GROUP_CASES[name]
    rng = np.random.default_rng(1234)
    ids = build(rng)
    vals = sample_values(len(ids), rng)
    ss = U._ss(S, 0.01, dev)
    t_ids = torch.from_numpy(ids.astype(np.int64) if int64_ids else ids).to(dev)
    got_v, got_o = ss.group_by_key(t_ids, torch.from_numpy(vals).to(dev))
    exp_v, exp_o = expected_group(ids, vals, S)
    assert np.array_equal(got_o.cpu().numpy(), exp_o), name + ": offsets"
    got_v = got_v.cpu().numpy()
    assert got_v.shape == exp_v.shape, name + ": %d grouped values, expected %d" % (len(got_v), len(exp_v))
    bad = np.flatnonzero(got_v.view(np.int64) != exp_v.view(np.int64))
    assert bad.size == 0, "%s: %d values differ, first at %d" % (name, bad.size, bad[0])
    # the set itself is untouched
    assert int(ss.stats()["n"].sum().item()) == 0


# --------------------------------------- 2. keyed ingest vs the oracle's loop
def skewed_ids(rng, S, N, hot, skip=0.03):
    r = rng.random(N)
    ids = rng.integers(0, S, N)
    ids[r < 0.4] = hot
    ids[r > 1.0 - skip] = -1
    return ids.astype(np.int32)


def pareto(rng, N):
    return (1.0 - rng.random(N)) ** (-1.0 / 1.5)


def oracle_loop(oracles, ids, vals):
    for i, v in zip(ids.tolist(), vals.tolist()):
        if i >= 0:
            oracles[i].add(v)


def case_oracle_loop(dev, eps):
    S, N = 37, 6000
    rng = np.random.default_rng(int(1 / eps) + 5)
    ss = U._ss(S, eps, dev)
    oracles = [OracleGK(eps) for _ in range(S)]
    for call in range(3):
        ids, vals = skewed_ids(rng, S, N, hot=5), pareto(rng, N)
        ss.ingest_keyed(torch.from_numpy(ids).to(dev), torch.from_numpy(vals).to(dev))
        oracle_loop(oracles, ids, vals)
        if call == 0:  # one plain CSR ingest between the keyed calls: pending values carry across
            seqs = [pareto(rng, s % 7) for s in range(S)]
            U.ingest_np(ss, seqs)
            for o, x in zip(oracles, seqs):
                o.add_many(x)
    assert_set_matches(ss, oracles, "keyed ingest eps=%g" % eps)
    got = ss.quantiles(QS).cpu().numpy()
    exp = np.asarray([o.quantiles(QS) for o in oracles], dtype=np.float64).reshape(S, len(QS))
    U.assert_same_quantiles(got, exp, "keyed ingest eps=%g quantiles" % eps, None)


# ---------------------------------------------- 3. keyed == CSR, same engine
def assert_snapshots_equal(a, b, what):
    for k in ("offs", "g", "d", "poffs", "n"):
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)
    for k in ("v", "pv", "min", "max", "sum", "avg"):
        assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), "%s: %s differs" % (what, k)


def case_equals_csr(dev):
    S, N, eps = 20_000, 400_000, 0.01
    rng = np.random.default_rng(99)
    ids = rng.integers(-1, S, N).astype(np.int32)
    ids[rng.random(N) < 0.2] = 123  # one long stream among short ones
    vals = pareto(rng, N)
    a, b = U._ss(S, eps, dev), U._ss(S, eps, dev)
    qa = a.ingest_keyed(torch.from_numpy(ids).to(dev), torch.from_numpy(vals).to(dev), quantiles=[.5, .9, .99])
    gv, go = expected_group(ids, vals, S)
    qb = b.ingest(torch.from_numpy(gv).to(dev), torch.from_numpy(go).to(dev), quantiles=[.5, .9, .99])
    assert np.array_equal(qa.cpu().numpy().view(np.int64), qb.cpu().numpy().view(np.int64)), "fused quantiles"
    assert_snapshots_equal(snapshot(a), snapshot(b), "keyed vs CSR")


# ------------------- 4. deferred re-run from the set's own buffers (GPU only)
def case_deferred(dev, asynchronous):
    """tests/test_gpu_state.py::test_promotion_arena_exhaustion_defers_and_reruns
    fed as shuffled keyed batches (the caller sets GK_POOL_SLOTS=2): streams
    deferred by one call are re-run from the set's grouped buffers, which the
    next keyed call must not regroup into before that."""
    rng = np.random.default_rng(83)
    S = 48
    ss = U._ss(S, 0.01, dev)
    o = U.OracleSet(S, 0.01)
    keep = []
    for part in range(3):
        seqs = [np.sort(rng.random(int(L)))[::-1].copy() if k % 3 else rng.random(int(L))
                for k, L in enumerate(rng.integers(5000, 30000, S))]
        flat, offs = U.csr(seqs)
        ids = np.repeat(np.arange(S, dtype=np.int32), np.diff(offs))
        # a random interleave of the streams that keeps every stream's own order
        slot_ids = rng.permutation(ids)
        vals = np.empty_like(flat)
        for s in range(S):
            vals[np.flatnonzero(slot_ids == s)] = flat[offs[s]:offs[s + 1]]
        ti, tv = torch.from_numpy(slot_ids).to(dev), torch.from_numpy(vals).to(dev)
        keep.append((ti, tv))  # inputs stay valid until the next call (async contract)
        ss.ingest_keyed(ti, tv, sync=not asynchronous)
        o.ingest(flat, offs)
    ss.sync()
    assert ss.num_promoted > 2
    U.assert_same_state(ss, o, "keyed deferred re-run")
    q = ss.quantiles([0.01, 0.5, 0.99]).cpu().numpy()
    U.assert_same_quantiles(q, o.quantiles([0.01, 0.5, 0.99]), "keyed deferred q", None)


# ------------------------------------------------------------------ 5. errors
def case_errors(dev):
    from gkarray_amd import GKBackendError
    from gkarray_amd import _lib as L
    S, eps = 37, 0.01
    rng = np.random.default_rng(3)
    ss, twin = U._ss(S, eps, dev), U._ss(S, eps, dev)
    oracles = [OracleGK(eps) for _ in range(S)]
    ids, vals = skewed_ids(rng, S, 3000, hot=2), pareto(rng, 3000)
    for x in (ss, twin):
        x.ingest_keyed(torch.from_numpy(ids).to(dev), torch.from_numpy(vals).to(dev))
    oracle_loop(oracles, ids, vals)
    before = snapshot(ss)
    # an id equal to S among valid ones: GK_E_ARG (on the GPU at sync() at the latest), nothing added
    bad = skewed_ids(rng, S, 5000, hot=2)
    bad[1234] = S
    bad_t, vals_t = torch.from_numpy(bad).to(dev), torch.from_numpy(pareto(rng, 5000)).to(dev)
    with pytest.raises(GKBackendError) as e:
        ss.ingest_keyed(bad_t, vals_t, sync=False)
        ss.sync()
    assert e.value.code == L.GK_E_ARG
    assert "1234" in str(e.value) or str(S) in str(e.value)
    assert_snapshots_equal(snapshot(ss), before, "state after a bad id")
    with pytest.raises(GKBackendError) as e:
        ss.group_by_key(bad_t, vals_t)
    assert e.value.code == L.GK_E_ARG
    assert_snapshots_equal(snapshot(ss), before, "state after a bad id in group_by_key")
    # a valid keyed call afterwards matches the oracle
    ids, vals = skewed_ids(rng, S, 3000, hot=7), pareto(rng, 3000)
    ss.ingest_keyed(torch.from_numpy(ids).to(dev), torch.from_numpy(vals).to(dev))
    oracle_loop(oracles, ids, vals)
    assert_set_matches(ss, oracles, "keyed call after an error")
    # shapes
    with pytest.raises(ValueError):
        ss.ingest_keyed(torch.zeros(4, dtype=torch.int32), torch.zeros(5, dtype=torch.float64))
    with pytest.raises(ValueError):
        ss.ingest_keyed(torch.zeros((2, 2), dtype=torch.int32), torch.zeros((2, 2), dtype=torch.float64))
    with pytest.raises(ValueError):
        ss.group_by_key(torch.zeros(4, dtype=torch.int32), torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError):
        ss.ingest_keyed(torch.tensor([0, 2 ** 31], dtype=torch.int64), torch.zeros(2, dtype=torch.float64))
    assert_set_matches(ss, oracles, "after refused arguments")
    # with a fused query the voided call answers as quantiles() from the pre-call state
    # (the GPU engine returns the tensor and reports at sync(); the host engine raises in the call)
    twin.ingest_keyed(torch.from_numpy(ids).to(dev), torch.from_numpy(vals).to(dev))
    q_bad = None
    with pytest.raises(GKBackendError) as e:
        q_bad = ss.ingest_keyed(bad_t, vals_t, quantiles=QS, sync=False)
        ss.sync()
    assert e.value.code == L.GK_E_ARG
    if q_bad is not None:
        assert np.array_equal(q_bad.cpu().numpy().view(np.int64), twin.quantiles(QS).cpu().numpy().view(np.int64))
        assert_snapshots_equal(snapshot(ss), snapshot(twin), "state after a voided call with a query")


def case_empty_with_query(dev):
    S, eps = 37, 0.01
    rng = np.random.default_rng(4)
    ss, twin = U._ss(S, eps, dev), U._ss(S, eps, dev)
    ids, vals = skewed_ids(rng, S, 3000, hot=2), pareto(rng, 3000)
    for x in (ss, twin):
        x.ingest_keyed(torch.from_numpy(ids).to(dev), torch.from_numpy(vals).to(dev))
    got = ss.ingest_keyed(torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.float64), quantiles=QS)
    exp = twin.quantiles(QS)
    assert np.array_equal(got.cpu().numpy().view(np.int64), exp.cpu().numpy().view(np.int64))
    assert_snapshots_equal(snapshot(ss), snapshot(twin), "count == 0 with a query")
    assert ss.ingest_keyed(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.float64)) is None
    assert_snapshots_equal(snapshot(ss), snapshot(twin), "count == 0 without a query")
