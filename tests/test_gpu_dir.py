"""The key directory on the MI355X engine (k_dir_insert / k_dir_flag / k_scan_*
/ k_dir_number / k_dir_lookup through gk_dir_assign, gk_dir_lookup,
gk_dir_keys, gk_dir_import and KeyDirectory / KeyedStreamSet): every case of
tests/dir_cases.py, ids bit for bit against a Python dict that runs the loop
of include/gk_capi.h, streams against one OracleGK per key."""
import pytest

import dir_cases as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("count", D.COUNTS)
def test_dir_sizes(gpu_device, count):
    """Case 1: counts round the wave and the scan tile, capacities 1, 32, 2^17,
    a key pool smaller and one larger than the count."""
    D.case_sizes(gpu_device, count)


def test_dir_ordering(gpu_device):
    """Case 2: one multiset ascending, descending and shuffled twice, in three
    calls each: ids follow first occurrence."""
    D.case_ordering(gpu_device)


@pytest.mark.parametrize("which", ["one", "three", "twice"])
def test_dir_contention(gpu_device, which):
    """Case 3: 200 000 samples of one key, of three keys interleaved, and
    65 536 keys twice with the second copies reversed."""
    D.case_contention(gpu_device, which)


@pytest.mark.parametrize("bits", ["0", "2"])
def test_dir_worst_case_chains(gpu_device, bits, monkeypatch):
    """Case 4: every home slot in the last 2^bits slots: one probe chain that
    wraps round the table end, filled to capacity over three calls."""
    monkeypatch.setenv("GK_DIR_HASH_BITS", bits)
    D.case_chains(gpu_device)


def test_dir_none_and_special_keys(gpu_device):
    """Case 5: GK_DIR_NONE answers -1 and is never stored; negative, zero,
    INT64_MAX and INT64_MIN + 1 are ordinary keys."""
    D.case_none(gpu_device)


def test_dir_overflow_is_void(gpu_device):
    """Case 6: 13 and 1000 new keys into 12 free ids: GK_E_OVERFLOW, and the
    directory answers as before."""
    D.case_overflow(gpu_device)


def test_dir_import_and_resize(gpu_device):
    """Case 7: round trip, the three refusals with the old contents intact, resized."""
    D.case_import(gpu_device)


def test_dir_argument_errors(gpu_device):
    """Case 8: counts, NULL arrays, capacities."""
    D.case_arguments(gpu_device)


@pytest.mark.parametrize("eps", [0.1, 0.01])
def test_keyed_stream_set_end_to_end(gpu_device, eps, tmp_path):
    """Case 9: capacity 4 to 512 over five adds; every key against its oracle;
    KeyError, reset, save / load, max_streams."""
    D.case_end_to_end(gpu_device, eps, tmp_path)


def test_dir_cross_engine(gpu_device):
    """Case 10: the same batches through a GPU and a host directory."""
    D.case_cross_engine(gpu_device)
