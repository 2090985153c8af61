"""Random operation sequences (tests/opseq_cases.py) on the host engine
(device="cpu"): every configuration the device test runs, with the same
(eps, seed, nops) and further seeds; the coverage conditions, counted on the
model alone over exactly the seeds the device test runs; and the model faults,
each of which the comparisons must notice."""
import collections

import pytest

import opseq_cases as O

_results = {}


def result(name, eps, seed):
    """One host-engine run per (configuration, eps, seed), shared by the tests below."""
    key = (name, eps, seed)
    if key not in _results:
        cfg = O.CONFIGS[name]
        _results[key] = O.run_sequence("cpu", eps, seed, cfg["nops"], **cfg["kw"])
    return _results[key]


ALL_RUNS = [(name, eps, seed) for name in O.CONFIGS for eps, seed in O.runs(name, "gpu_seeds") + O.runs(name, "cpu_seeds")]


@pytest.mark.parametrize("name,eps,seed", ALL_RUNS)
def test_cpu_opseq(name, eps, seed):
    r = result(name, eps, seed)
    assert sum(r["ran"].values()) == O.CONFIGS[name]["nops"]


def totals(name):
    ran, eff, ev = collections.Counter(), collections.Counter(), collections.Counter()
    top = large = 0
    for eps, seed in O.runs(name, "gpu_seeds"):
        r = result(name, eps, seed)
        ran += r["ran"]
        eff += r["effective"]
        ev += r["events"]
        top, large = max(top, r["max_table"]), max(large, r["max_large"])
    return ran, eff, ev, top, large


@pytest.mark.parametrize("name", list(O.CONFIGS))
def test_opseq_coverage_of_the_device_seeds(name):
    """Conditions, not measurements, over the seeds the device test runs: every
    operation kind effective at least 3 times (a compaction: the model predicts
    a demotion), every event at least once (with ingests left in flight: every
    kind directly after each of the three calls that can be), more
    streams large at once than GK_POOL_SLOTS=2 has slots, and on the short
    ladder a table beyond the last bounded class."""
    ran, eff, ev, top, large = totals(name)
    print(name, "ran/effective", {k: (ran[k], eff[k]) for k in O.KINDS})
    print(name, "folds replaced by a reset (counted apart):", ran[O.REPLACED])
    print(name, "events", dict(sorted(ev.items())), "largest table", top, "large at once", large)
    assert not [k for k in O.KINDS if eff[k] < 3], {k: eff[k] for k in O.KINDS}
    assert not [e for e in O.required_events(name) if ev[e] < 1], dict(ev)
    assert large >= 3
    if "GK_CAPS" in O.CONFIGS[name]["env"]:
        assert top > O.LAST_BOUNDED_CAPACITY
        assert top < 4095  # (the ladder's last class holds one entry less than its capacity)


def test_fit_boundaries():
    """fit(E): the smallest class t with E <= cap[t] - 1, at the table sizes of
    compact_cases.case_fit_boundaries on 128,256,512,4096."""
    caps = O.ladder(0.01, O.SHORT_LADDER)
    assert caps == [128, 256, 512, 4096]
    assert [O.fit(E, caps) for E in (0, 1, 127, 128, 255, 256, 511, 512)] == [0, 0, 0, 1, 1, 2, 2, 3]
    assert O.fit(4095, caps) == 3
    with pytest.raises(ValueError):
        O.fit(4096, caps)
    assert O.ladder(0.01) == [128, 2048, 32768, 1 << 20] and O.ladder(0.001) == [2048, 32768, 1 << 20]


def test_opseq_is_reproducible_and_replayable():
    """The same (eps, seed, nops) gives the same operations; stop_after gives their prefix."""
    a = O.run_sequence("cpu", 0.01, 11, 40)
    b = O.run_sequence("cpu", 0.01, 11, 40)
    c = O.run_sequence("cpu", 0.01, 11, 40, stop_after=17)
    assert repr(a["log"]) == repr(b["log"]) and a["events"] == b["events"]
    assert repr(c["log"]) == repr(a["log"][:17])


@pytest.mark.parametrize("fault", O.FAULTS)
def test_opseq_notices_a_model_fault(fault):
    """A model that is wrong in one small way must not survive the configured seeds."""
    name = "tiny_arenas" if fault.startswith("drop") else "short_ladder"
    cfg = O.CONFIGS[name]
    for eps, seed in O.runs(name, "gpu_seeds"):
        try:
            O.run_sequence("cpu", eps, seed, cfg["nops"], model_fault=fault, **cfg["kw"])
        except AssertionError as e:
            assert "opseq eps=" in str(e) and "operations so far" in str(e)
            # noticed by a comparison, not by the driver tripping over its own model
            assert type(e.__cause__) is AssertionError, repr(e.__cause__)
            return
    pytest.fail("model fault %r went unnoticed over the seeds of %s" % (fault, name))
