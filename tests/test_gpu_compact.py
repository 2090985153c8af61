"""Compaction on the MI355X engine (k_compact_plan / k_compact_move through
gk_compact / gk_class_usage and StreamSet.compact / class_usage): every case of
tests/compact_cases.py, bit for bit against the oracles and against the state
before the call."""
import pytest

import compact_cases as X

pytestmark = pytest.mark.gpu

LADDER = "128,256,512,4096"


def test_compact_reset_gives_back(gpu_device, monkeypatch):
    """Case 1: streams of classes 2 and 3 are reset; the compaction empties both
    classes, keeps the class-1 stream, and a reset stream is promoted again."""
    monkeypatch.setenv("GK_CAPS", LADDER)
    X.case_reset_gives_back(gpu_device)


def test_compact_fit_boundaries(gpu_device, monkeypatch):
    """Case 2: tables of 0, 1, 127 | 128, 255 | 256, 511 | 512 entries, all in
    class 3, land in classes 0 | 1 | 2 | 3; pending values stay where they are."""
    monkeypatch.setenv("GK_CAPS", LADDER)
    X.case_fit_boundaries(gpu_device)


def test_compact_noop_and_idempotence(gpu_device, monkeypatch):
    """Case 3: nothing promoted, everything still needed, a second call, S == 0."""
    monkeypatch.setenv("GK_CAPS", LADDER)
    X.case_noop(gpu_device)


def test_compact_many_streams(gpu_device):
    """Case 4: 4099 streams on the default ladder -- more than one workgroup, a
    partial last wave; 1367 promoted, 684 of them reset again."""
    X.case_many_streams(gpu_device)


def test_compact_arenas_shrink_and_regrow(gpu_device, monkeypatch):
    """Case 5: a 12-slot arena goes back to the 2 slots a set starts with, the
    next call does not regrow it, and 5 streams come back through deferral."""
    monkeypatch.setenv("GK_CAPS", LADDER)
    monkeypatch.setenv("GK_POOL_SLOTS", "2")
    X.case_arenas(gpu_device)


def test_compact_settles_deferred_streams_first(gpu_device, monkeypatch):
    """Case 6: streams an in-flight ingest deferred are re-run before the compaction."""
    monkeypatch.setenv("GK_CAPS", LADDER)
    monkeypatch.setenv("GK_POOL_SLOTS", "2")
    X.case_deferred(gpu_device)


def test_compact_returns_sticky_error(gpu_device, monkeypatch):
    """Case 6: a pending GK_E_OVERFLOW is returned and nothing is compacted."""
    monkeypatch.setenv("GK_CAPS", "128,256")
    X.case_sticky_error(gpu_device)


@pytest.mark.parametrize("seed", [71, 72, 73])
def test_compact_random_sequences(gpu_device, monkeypatch, seed):
    """Case 7: ingest / reset / flush / put / ranks / compact in random order."""
    monkeypatch.setenv("GK_CAPS", LADDER)
    X.case_random(gpu_device, seed)


def test_compact_keyed_churn(gpu_device, monkeypatch):
    """Case 8: keys with promoted streams leave, new keys inherit ids and
    classes, KeyedStreamSet.compact() brings them home."""
    monkeypatch.setenv("GK_CAPS", LADDER)
    X.case_keyed_churn(gpu_device)


def test_compact_arguments(gpu_device, monkeypatch):
    """Case 9: class index out of range, NULL outputs, a NULL set."""
    monkeypatch.setenv("GK_CAPS", LADDER)
    X.case_arguments(gpu_device)
