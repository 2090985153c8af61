"""Keyed rank queries on the MI355X engine (k_rank_keyed through gk_ranks_keyed
and StreamSet.ranks_keyed / cdf_keyed, KeyedStreamSet.ranks_keyed / score):
every case of tests/rankkeyed_cases.py, bit for bit against the contract of
include/gk_capi.h applied to the oracle's tables."""
import pytest

import rankkeyed_cases as Q

pytestmark = pytest.mark.gpu


@pytest.fixture
def setenv(monkeypatch):
    return lambda k, v: monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)


def test_rank_keyed_chunk_and_run_boundaries(gpu_device, setenv):
    """Case 1: runs that start on, straddle and span 64-sample chunks, a chunk of
    one-sample streams; the same bytes at the default chunk."""
    Q.case_boundaries(gpu_device, setenv)


def test_rank_keyed_thresholds(gpu_device):
    """Case 2: +-inf, signed zeros, min, max, entries, midpoints for every stream."""
    Q.case_thresholds(gpu_device)


def test_rank_keyed_equivalence(gpu_device):
    """Case 3: == ranks_select gathered; the state flush_select leaves; idempotent."""
    Q.case_equivalence(gpu_device)


def test_rank_keyed_negative_ids(gpu_device):
    """Case 4: -1, -7, INT32_MIN with NaN; all negative; count 0 and 1."""
    Q.case_negative(gpu_device)


@pytest.mark.parametrize("S", [1, 257, 65537])
def test_rank_keyed_radix_passes(gpu_device, S):
    """Case 5: one, two and three passes of the group-by carrying sample indices."""
    Q.case_radix(gpu_device, S)


def test_rank_keyed_long_table(gpu_device):
    """Case 6: a 2079-entry table, beyond the tile, gets 70 samples."""
    Q.case_long_table(gpu_device)


def test_rank_keyed_promoted_streams(gpu_device, monkeypatch):
    """Case 6: an occurring stream climbs a class inside the call."""
    monkeypatch.setenv("GK_CAPS", "128,256,512,4096")
    Q.case_promoted(gpu_device)


def test_rank_keyed_refusals_leave_state(gpu_device, setenv):
    """Case 7: id == S, NaN on a live row, both, no output, bad counts, NULL ids, a bad chunk."""
    Q.case_refusals(gpu_device, setenv)


def test_rank_keyed_overflow_past_last_class(gpu_device, monkeypatch):
    """Case 8: GK_E_OVERFLOW leaves the outputs and the stream that did not fit untouched."""
    monkeypatch.setenv("GK_CAPS", "128,256")
    Q.case_overflow(gpu_device)


def test_rank_keyed_settles_deferred_keyed_ingest_first(gpu_device, monkeypatch):
    """Case 8: streams an in-flight keyed ingest deferred are re-run before the ranks are read."""
    monkeypatch.setenv("GK_POOL_SLOTS", "2")
    Q.case_deferred(gpu_device)


def test_rank_keyed_python_layer(gpu_device):
    """Case 9: cdf_keyed; KeyedStreamSet.ranks_keyed / score with unknown keys; score-then-add."""
    Q.case_python(gpu_device)
