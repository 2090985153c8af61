"""Keyed score-and-ingest on the MI355X engine (k_rank_ingest_keyed through
gk_rank_ingest_keyed and StreamSet.rank_ingest_keyed / score_ingest_keyed,
KeyedStreamSet.score_add): every case of tests/rankingest_cases.py, bit for bit
against the oracle and against ranks_keyed + ingest_keyed on a twin set."""
import pytest

import rankingest_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture
def setenv(monkeypatch):
    return lambda k, v: monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)


def test_rank_ingest_chunk_and_run_boundaries(gpu_device, setenv):
    """Case 1: runs of 0 .. 200 samples on, across and over 64-sample chunks;
    every value at its own grouped position; the same states at the default chunk."""
    F.case_boundaries(gpu_device, setenv)


def test_rank_ingest_repeated_calls(gpu_device):
    """Case 2: the second call ranks against the first call's values; flush
    points inside a run and exactly at its end."""
    F.case_repeated(gpu_device)


def test_rank_ingest_special_values(gpu_device):
    """Case 3: negative ids, all negative, count 0 and 1, no rank output,
    signed zeros, infinities and denormals bit for bit."""
    F.case_special(gpu_device)


@pytest.mark.parametrize("S", [1, 257, 65537])
def test_rank_ingest_radix_passes(gpu_device, S):
    """Case 4: one, two and three passes of the one group-by."""
    F.case_radix(gpu_device, S)


def test_rank_ingest_long_table(gpu_device):
    """Case 5: a 2079-entry table, streamed tile after tile."""
    F.case_long_table(gpu_device)


def test_rank_ingest_promoted_streams(gpu_device, monkeypatch):
    """Case 5: one stream climbs a class in the rank half's flush, one in the ingest half."""
    monkeypatch.setenv("GK_CAPS", "128,256,512,4096")
    F.case_promoted(gpu_device)


@pytest.mark.parametrize("run", ["sorted", "unsorted", "single"])
def test_rank_ingest_fused_quantiles(gpu_device, run):
    """Case 6: quantiles of every stream after the batch, in the same call."""
    F.case_quantiles(gpu_device, run)


def test_rank_ingest_settles_deferred_keyed_ingest_first(gpu_device, monkeypatch):
    """Case 7a: an in-flight keyed ingest's deferred streams are re-run before the call."""
    monkeypatch.setenv("GK_POOL_SLOTS", "2")
    F.case_deferred_before(gpu_device)


@pytest.mark.parametrize("then", ["ranks_keyed", "ingest_keyed"])
def test_rank_ingest_own_deferred_streams_rerun_from_set_buffers(gpu_device, monkeypatch, then):
    """Case 7b: the fused call's own deferred streams, re-run by the next keyed call."""
    monkeypatch.setenv("GK_POOL_SLOTS", "2")
    F.case_deferred_own(gpu_device, then)


def test_rank_ingest_overflow_in_the_rank_half(gpu_device, monkeypatch):
    """Case 8: GK_E_OVERFLOW of the flush: outputs untouched, nothing ingested."""
    monkeypatch.setenv("GK_CAPS", "128,256")
    F.case_overflow(gpu_device)


def test_rank_ingest_refusals_leave_state(gpu_device, setenv):
    """Case 9: every GK_E_ARG, with sentinel outputs and an unchanged set."""
    F.case_refusals(gpu_device, setenv)


def test_rank_ingest_python_layer(gpu_device):
    """Case 10: score_ingest_keyed; KeyedStreamSet.score_add vs the oracle loop and vs score + add."""
    F.case_python(gpu_device)
