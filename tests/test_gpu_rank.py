"""Rank queries on the MI355X engine (k_rank through gk_ranks / gk_ranks_select
and StreamSet.ranks / ranks_select / cdf, GKArray.rank / cdf): every case of
tests/rank_cases.py, bit for bit against the contract of include/gk_capi.h
applied to the oracle's tables."""
import pytest

import rank_cases as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("run", K.MIXED_RUNS)
def test_rank_mixed_set(gpu_device, run):
    """Case 1: tables of 63..193 entries beside the mixed set; +-inf, signed
    zeros, every stream's min / max / entries / midpoints as thresholds."""
    K.case_mixed(gpu_device, run)


def test_rank_select(gpu_device):
    """Case 2: unsorted ids with a repeat; unlisted neighbours keep their pending values."""
    K.case_select(gpu_device)


def test_rank_equivalences(gpu_device):
    """Case 3: ranks_select == ranks()[ids]; ranks leaves the state flush() leaves; idempotent."""
    K.case_equivalences(gpu_device)


def test_rank_promoted_streams(gpu_device, monkeypatch):
    """Case 4: a listed stream climbs a class inside the call."""
    monkeypatch.setenv("GK_CAPS", "128,256,512,4096")
    K.case_promoted(gpu_device)


def test_rank_long_table(gpu_device):
    """Case 5: a table of 2079 entries, 70 thresholds."""
    K.case_long_table(gpu_device)


def test_rank_bracket_on_ingest_only_streams(gpu_device):
    """Case 6: lo <= #{values <= x} <= hi."""
    K.case_bracket(gpu_device)


def test_rank_merged_histories(gpu_device):
    """Case 7: after merge_from and rollup_from, the formula on the merged table."""
    K.case_merged(gpu_device)


def test_rank_errors_leave_state(gpu_device):
    """Case 8: NaN thresholds, bad ids, nx < 0, no output, count == 0, nx == 0."""
    K.case_errors(gpu_device)


def test_rank_overflow_past_last_class(gpu_device, monkeypatch):
    """Case 9: GK_E_OVERFLOW leaves lo / hi and the stream that did not fit untouched."""
    monkeypatch.setenv("GK_CAPS", "128,256")
    K.case_overflow(gpu_device)


def test_rank_settles_deferred_streams_first(gpu_device, monkeypatch):
    """Case 10: streams an in-flight ingest deferred are re-run before the ranks are read."""
    monkeypatch.setenv("GK_POOL_SLOTS", "2")
    K.case_deferred(gpu_device)


def test_rank_dropin_and_cdf(gpu_device):
    """Case 11: GKArray.rank / cdf and StreamSet.cdf / cdf_select."""
    K.case_dropin(gpu_device)
