"""Per-stream selection on the host engine (device="cpu"): the cases of
tests/select_cases.py bit for bit against the oracle, and the ASan + UBSan
program tests/cpu_select_selftest.cpp (host engine vs the C oracle)."""
import os
import shutil
import subprocess

import pytest

import select_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("run", sorted(C.MIXED_RUNS))
def test_cpu_select_mixed_set(run):
    C.case_mixed("cpu", run)


def test_cpu_select_continuation():
    C.case_continuation("cpu")


def test_cpu_select_long_descending_streams():
    C.case_promoted("cpu")


def test_cpu_select_reset():
    C.case_reset("cpu")


def test_cpu_select_flush():
    C.case_flush("cpu")


def test_cpu_select_errors_leave_state():
    C.case_errors("cpu")


def test_cpu_select_reset_after_fused_query_in_flight():
    C.case_reset_after_fused_query_in_flight("cpu")


def test_select_symbols_are_bound():
    from gkarray_amd import _lib
    for name in ("gk_quantiles_select", "gk_flush_select", "gk_reset_select", "gk_stats_select"):
        assert name in _lib.SYMBOLS and name in _lib.CPU_SYMBOLS, name
        assert hasattr(_lib.load_cpu(), name), name


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cpu_select_under_asan_ubsan():
    """Case 9: the four selection calls of the host engine under ASan + UBSan,
    a stand-alone program checked against the C oracle."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "sketches-py_amd", "cpu"), "sanitize-select"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "cpu_select_selftest: ok" in r.stdout
