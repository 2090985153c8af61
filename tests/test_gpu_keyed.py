"""Keyed ingest on the MI355X engine (the k_group_* radix partition through
gk_group_by_key / gk_ingest_keyed / StreamSet.group_by_key / ingest_keyed):
every case of tests/keyed_cases.py, bit for bit against numpy's stable sort,
the oracle's per-sample loop and the CSR ingest of the same engine."""
import pytest

import keyed_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(C.GROUP_CASES))
def test_group_by_key_matches_stable_sort(gpu_device, name):
    """Case 1: one, two and three radix passes, wave-edge sizes, skipped ids,
    a key's run across many tiles, ordered and reverse-ordered input."""
    C.case_group(gpu_device, name)


def test_group_by_key_int64_ids(gpu_device):
    C.case_group(gpu_device, "skips_second_digit", int64_ids=True)


@pytest.mark.parametrize("eps", [0.1, 0.01])
def test_ingest_keyed_matches_oracle_loop(gpu_device, eps):
    """Case 2: three keyed calls and a CSR ingest == OracleGK.add per sample in
    arrival order."""
    C.case_oracle_loop(gpu_device, eps)


def test_ingest_keyed_equals_csr_ingest(gpu_device):
    """Case 3: S = 20000, N = 400000 with a fused query == ingest of the
    numpy-grouped batch."""
    C.case_equals_csr(gpu_device)


@pytest.mark.parametrize("asynchronous", [False, True])
def test_keyed_deferred_rerun_from_set_buffers(gpu_device, monkeypatch, asynchronous):
    """Case 4: with 2-slot arenas, streams deferred by a keyed call are re-run
    from the set's own grouped buffers before the next call regroups into them."""
    monkeypatch.setenv("GK_POOL_SLOTS", "2")
    C.case_deferred(gpu_device, asynchronous)


def test_keyed_errors_leave_state(gpu_device):
    """Case 5: an id == S voids the call (GK_E_ARG at sync() at the latest)."""
    C.case_errors(gpu_device)


def test_keyed_empty_batch_with_query(gpu_device):
    C.case_empty_with_query(gpu_device)
