"""Key removal and id recycling on the MI355X engine (k_dir_remove_mark /
k_dir_remove_release / k_dir_free_flag / k_dir_free_compact and k_dir_number's
free-id branch, through gk_dir_remove, gk_dir_assign, gk_dir_import_sparse and
KeyDirectory / KeyedStreamSet): every case of tests/dirremove_cases.py, bit for
bit against a Python model that runs the loops of include/gk_capi.h, streams
against one OracleGK per live key."""
import pytest

import dirremove_cases as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("count", R.COUNTS)
def test_dir_remove_sizes(gpu_device, count):
    """Case 1: remove counts round the wave, the workgroup and the scan tile,
    capacities 1, 32, 2^17; known keys, strangers and GK_DIR_NONE; then an
    assign of old, removed and fresh keys, a void one, and a lookup."""
    R.case_sizes(gpu_device, count)


def test_dir_recycling_order(gpu_device):
    """Case 2: ids 3, 17, 4, 30 freed in that order over two calls come back
    as 3, 4, 17, 30, bound, bound + 1 in first-occurrence order, whatever the
    batch order and over one or two assign calls."""
    R.case_recycling(gpu_device)


@pytest.mark.parametrize("which", ["one", "twice", "returns"])
def test_dir_remove_duplicates(gpu_device, which):
    """Case 3: one key 200 000 times; 65 536 keys twice, the second copies
    reversed; one key removed and assigned again across five calls."""
    R.case_duplicates(gpu_device, which)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("bits", ["0", "2"])
def test_dir_tombstone_chains(gpu_device, bits, half, monkeypatch):
    """Case 4: every home slot in the last 2^bits of 64 slots; five whole
    generations of 32 keys, or 16 out and 16 in for 8 rounds: no overflow."""
    monkeypatch.setenv("GK_DIR_HASH_BITS", bits)
    R.case_chains(gpu_device, half)


def test_dir_overflow_is_void_with_holes(gpu_device):
    """Case 5: 6 new keys into 5 free ids of a full id space: GK_E_OVERFLOW and
    keys() byte-identical; then 5 new keys take the 5 freed ids, ascending."""
    R.case_overflow(gpu_device)


def test_dir_sparse_import_and_resize(gpu_device):
    """Case 6: round trip of a directory with holes, resized, the refusals."""
    R.case_sparse_import(gpu_device)


def test_dir_remove_argument_errors(gpu_device):
    """Case 7: counts, NULL arrays, NULL directory."""
    R.case_arguments(gpu_device)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("capacity", [64, 600])
def test_dir_random_sequences(gpu_device, capacity, seed):
    """Case 8: 200 random operations, directory and model compared after each."""
    R.case_sequences(gpu_device, capacity, seed)


def test_dir_remove_cross_engine(gpu_device):
    """Case 9: the same sequence through a GPU and a host directory."""
    R.case_cross_engine(gpu_device)


@pytest.mark.parametrize("eps", [0.1, 0.01])
def test_keyed_stream_set_churn(gpu_device, eps, tmp_path):
    """Case 10: ten generations of about 100 keys through 128 streams; remove,
    discard, pop to the host engine; KeyError; save / load with holes."""
    R.case_end_to_end(gpu_device, eps, tmp_path)


def test_keyed_stream_set_grows_with_holes(gpu_device):
    """Growth by doubling of a KeyedStreamSet whose directory has free ids."""
    R.case_growth(gpu_device)
