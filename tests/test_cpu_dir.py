"""The key directory on the host engine (device="cpu"): the cases of
tests/dir_cases.py bit for bit against a Python dict that runs the loop of
include/gk_capi.h, KeyedStreamSet against one OracleGK per key, and the
ASan + UBSan program tests/cpu_dir_selftest.cpp (host engine vs a std::map)."""
import os
import shutil
import subprocess

import pytest

import dir_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("count", D.COUNTS)
def test_cpu_dir_sizes(count):
    D.case_sizes("cpu", count)


def test_cpu_dir_ordering():
    D.case_ordering("cpu")


@pytest.mark.parametrize("which", ["one", "three", "twice"])
def test_cpu_dir_contention(which):
    D.case_contention("cpu", which)


@pytest.mark.parametrize("bits", ["0", "2"])
def test_cpu_dir_worst_case_chains(bits, monkeypatch):
    monkeypatch.setenv("GK_DIR_HASH_BITS", bits)
    D.case_chains("cpu")


def test_cpu_dir_none_and_special_keys():
    D.case_none("cpu")


def test_cpu_dir_overflow_is_void():
    D.case_overflow("cpu")


def test_cpu_dir_import_and_resize():
    D.case_import("cpu")


def test_cpu_dir_argument_errors():
    D.case_arguments("cpu")


def test_cpu_dir_bad_hash_bits(monkeypatch):
    from gkarray_amd import GKBackendError, KeyDirectory, _lib
    monkeypatch.setenv("GK_DIR_HASH_BITS", "many")
    with pytest.raises(GKBackendError) as e:
        KeyDirectory(4, device="cpu")
    assert e.value.code == _lib.GK_E_ARG


def test_dir_symbols_are_bound():
    D.case_symbols()


@pytest.mark.parametrize("eps", [0.1, 0.01])
def test_cpu_keyed_stream_set_end_to_end(eps, tmp_path):
    D.case_end_to_end("cpu", eps, tmp_path)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cpu_dir_under_asan_ubsan():
    """gk_dir_* of the host engine under ASan + UBSan, a stand-alone program
    checked against a std::map: random batches, overflow, import refusals and
    the wrap-around switch."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "sketches-py_amd", "cpu"), "sanitize-dir"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "cpu_dir_selftest: ok" in r.stdout
