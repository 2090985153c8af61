"""Stream transfer on the host engine (device="cpu"): the cases of
tests/transfer_cases.py bit for bit against the oracle, and the ASan + UBSan
program tests/cpu_transfer_selftest.cpp (host engine vs the C oracle)."""
import os
import shutil
import subprocess

import pytest

import transfer_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpu_transfer_take_mixed_set():
    T.case_take("cpu")


def test_cpu_transfer_continuation():
    T.case_continuation("cpu")


def test_cpu_transfer_bytes_equal_pack():
    T.case_bytes_vs_pack("cpu")


def test_cpu_transfer_lane_and_offset_edges():
    T.case_edges("cpu")


@pytest.mark.parametrize("nrows", [2048, 2049, 1024 * 2048 + 1])
def test_cpu_transfer_scan_boundaries(nrows):
    T.case_scan("cpu", nrows)


def test_cpu_transfer_errors_leave_state():
    T.case_errors("cpu")


def test_cpu_transfer_python_surface():
    T.case_python_surface("cpu")


def test_transfer_symbols_are_bound():
    T.case_symbols()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cpu_transfer_under_asan_ubsan():
    """Case 11: gk_pack_select / gk_unpack_select of the host engine under
    ASan + UBSan, a stand-alone program checked against the C oracle."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "sketches-py_amd", "cpu"), "sanitize-transfer"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "cpu_transfer_selftest: ok" in r.stdout
