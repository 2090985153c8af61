"""Key removal and id recycling on the host engine (device="cpu"): the cases of
tests/dirremove_cases.py bit for bit against a Python model that runs the
loops of include/gk_capi.h, KeyedStreamSet against one OracleGK per live key,
and the ASan + UBSan program tests/cpu_dirremove_selftest.cpp (host engine vs
a std::map and a std::set of free ids)."""
import os
import shutil
import subprocess

import pytest

import dirremove_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("count", R.COUNTS)
def test_cpu_dir_remove_sizes(count):
    R.case_sizes("cpu", count)


def test_cpu_dir_recycling_order():
    R.case_recycling("cpu")


@pytest.mark.parametrize("which", ["one", "twice", "returns"])
def test_cpu_dir_remove_duplicates(which):
    R.case_duplicates("cpu", which)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("bits", ["0", "2"])
def test_cpu_dir_tombstone_chains(bits, half, monkeypatch):
    monkeypatch.setenv("GK_DIR_HASH_BITS", bits)
    R.case_chains("cpu", half)


def test_cpu_dir_overflow_is_void_with_holes():
    R.case_overflow("cpu")


def test_cpu_dir_sparse_import_and_resize():
    R.case_sparse_import("cpu")


def test_cpu_dir_remove_argument_errors():
    R.case_arguments("cpu")


def test_dir_remove_symbols_are_bound():
    R.case_symbols()


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("capacity", [64, 600])
def test_cpu_dir_random_sequences(capacity, seed):
    R.case_sequences("cpu", capacity, seed)


@pytest.mark.parametrize("eps", [0.1, 0.01])
def test_cpu_keyed_stream_set_churn(eps, tmp_path):
    R.case_end_to_end("cpu", eps, tmp_path)


def test_cpu_keyed_stream_set_grows_with_holes():
    R.case_growth("cpu")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cpu_dir_remove_under_asan_ubsan():
    """gk_dir_remove, gk_dir_import_sparse and gk_dir_assign with free ids of
    the host engine under ASan + UBSan, a stand-alone program checked against
    a std::map and a std::set: random sequences, tombstone chains, void calls
    with holes."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "sketches-py_amd", "cpu"), "sanitize-dirremove"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "cpu_dirremove_selftest: ok" in r.stdout
