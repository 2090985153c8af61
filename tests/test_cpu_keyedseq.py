"""Random operation sequences on a KeyedStreamSet (tests/keyedseq_cases.py) on
the host engine (device="cpu"): every configuration the device test runs, with
the same (eps, seed, nops) and two further seeds; the events, counted on the
model alone over exactly the seeds the device test runs; and the model faults,
each of which the comparisons must notice."""
import collections

import pytest

import keyedseq_cases as S

_results = {}


def result(name, eps, seed):
    """One host-engine run per (configuration, eps, seed), shared by the tests below."""
    key = (name, eps, seed)
    if key not in _results:
        cfg = S.CONFIGS[name]
        _results[key] = S.run_sequence("cpu", eps, seed, cfg["nops"], **cfg["kw"])
    return _results[key]


ALL_RUNS = [(name, eps, seed) for name in S.CONFIGS for eps, seed in S.runs(name, "gpu_seeds") + S.runs(name, "cpu_seeds")]


@pytest.mark.parametrize("name,eps,seed", ALL_RUNS)
def test_cpu_keyedseq(name, eps, seed):
    r = result(name, eps, seed)
    assert sum(r["ran"].values()) == S.CONFIGS[name]["nops"]


@pytest.mark.parametrize("name", list(S.CONFIGS))
def test_keyedseq_coverage_of_the_device_seeds(name):
    """Conditions over the seeds the device test runs: every operation kind at
    least 3 times, every event at least once, the object doubled at least three
    times (8 -> 64) where max_streams does not stop it, and a table beyond class
    0 of the ladder."""
    ran, ev = collections.Counter(), collections.Counter()
    top = cap = 0
    for eps, seed in S.runs(name, "gpu_seeds"):
        r = result(name, eps, seed)
        ran += r["ran"]
        ev += r["events"]
        top, cap = max(top, r["max_table"]), max(cap, r["max_capacity"])
    print(name, "ran", dict(ran), "events", dict(sorted(ev.items())), "largest table", top, "capacity", cap)
    assert not [k for k in S.KINDS if ran[k] < 3], dict(ran)
    assert not [e for e in S.required_events(name) if ev[e] < 1], dict(ev)
    assert top > 128
    assert cap == (48 if "max_streams" in S.CONFIGS[name]["kw"] else 64)


def test_keyedseq_is_reproducible_and_replayable():
    a = S.run_sequence("cpu", 0.01, 11, 40)
    b = S.run_sequence("cpu", 0.01, 11, 40)
    c = S.run_sequence("cpu", 0.01, 11, 40, stop_after=17)
    assert repr(a["log"]) == repr(b["log"]) and a["events"] == b["events"]
    assert repr(c["log"]) == repr(a["log"][:17])


@pytest.mark.parametrize("fault", S.FAULTS)
def test_keyedseq_notices_a_model_fault(fault):
    """A model that is wrong in one small way must not survive the configured seeds."""
    name = "short_ladder"
    cfg = S.CONFIGS[name]
    for eps, seed in S.runs(name, "gpu_seeds"):
        try:
            S.run_sequence("cpu", eps, seed, cfg["nops"], model_fault=fault, **cfg["kw"])
        except AssertionError as e:
            assert "keyedseq eps=" in str(e) and "operations so far" in str(e)
            assert type(e.__cause__) is AssertionError, repr(e.__cause__)
            return
    pytest.fail("model fault %r went unnoticed over the seeds of %s" % (fault, name))
