"""Per-stream selection on the MI355X engine (k_select_check / k_select_query /
k_select_reset / k_select_stats through gk_*_select and
StreamSet.quantiles_select / flush_select / reset_select / stats_select): every
case of tests/select_cases.py, bit for bit against one oracle per stream on
which only the listed streams are queried, flushed or replaced."""
import pytest

import select_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("run", sorted(C.MIXED_RUNS))
def test_select_mixed_set(gpu_device, run):
    """Case 1: unsorted ids with a repeat and an empty stream; listed and
    unlisted neighbours with pending values; D(190) leaves the 128-entry class
    inside the call."""
    C.case_mixed(gpu_device, run)


def test_select_continuation(gpu_device):
    """Case 2: queried and never-queried streams continue their own histories."""
    C.case_continuation(gpu_device)


def test_select_promoted_streams(gpu_device, monkeypatch):
    """Case 3: on the ladder 128,256,512,4096 a class-1 stream climbs to class 2
    inside the call; a class-2 stream is queried where it stands."""
    monkeypatch.setenv("GK_CAPS", "128,256,512,4096")
    C.case_promoted(gpu_device)


def test_select_reset_keeps_class(gpu_device):
    """Case 4: reset_select of a class-0, a class-1 and an empty stream; new
    values into them; stats_select == stats()[ids]."""
    C.case_reset(gpu_device)


def test_select_flush(gpu_device):
    """Case 5: flush_select == the state quantiles_select leaves; idempotent."""
    C.case_flush(gpu_device)


def test_select_errors_leave_state(gpu_device):
    """Case 6: bad ids, NaN quantiles, bad id tensors, count == 0, nq == 0."""
    C.case_errors(gpu_device)


def test_select_overflow_past_last_class(gpu_device, monkeypatch):
    """Case 7: a listed stream whose flush outgrows the last class keeps its
    state, the other listed streams are flushed, GK_E_OVERFLOW."""
    monkeypatch.setenv("GK_CAPS", "128,256")
    C.case_overflow(gpu_device)


def test_select_settles_deferred_streams_first(gpu_device, monkeypatch):
    """Case 8: with 2-slot arenas, streams an in-flight ingest deferred are
    re-run before the selection reads them."""
    monkeypatch.setenv("GK_POOL_SLOTS", "2")
    C.case_deferred(gpu_device)


def test_select_reset_after_fused_query_in_flight(gpu_device, monkeypatch):
    """Case 9: with 2-slot arenas, reset() directly after an ingest with a
    fused query left in flight: the deferred streams' answers are still written."""
    monkeypatch.setenv("GK_POOL_SLOTS", "2")
    C.case_reset_after_fused_query_in_flight(gpu_device)
