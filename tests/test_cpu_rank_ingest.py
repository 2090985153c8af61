"""Keyed score-and-ingest on the host engine (device="cpu"): the cases of
tests/rankingest_cases.py -- bit for bit against the oracle and against the
two calls ranks_keyed + ingest_keyed on a twin set -- and the ASan + UBSan
program tests/cpu_rankingest_selftest.cpp."""
import os
import shutil
import subprocess

import pytest

import rankingest_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def setenv(monkeypatch):
    return lambda k, v: monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)


def test_cpu_rank_ingest_boundaries(setenv):
    F.case_boundaries("cpu", setenv)


def test_cpu_rank_ingest_repeated_calls():
    F.case_repeated("cpu")


def test_cpu_rank_ingest_special_values():
    F.case_special("cpu")


@pytest.mark.parametrize("S", [1, 257, 65537])
def test_cpu_rank_ingest_stream_counts(S):
    F.case_radix("cpu", S)


def test_cpu_rank_ingest_long_table():
    F.case_long_table("cpu")


def test_cpu_rank_ingest_long_descending_streams():
    F.case_promoted("cpu")


@pytest.mark.parametrize("run", ["sorted", "unsorted", "single"])
def test_cpu_rank_ingest_fused_quantiles(run):
    F.case_quantiles("cpu", run)


def test_cpu_rank_ingest_refusals_leave_state(setenv):
    F.case_refusals("cpu", setenv)


def test_cpu_rank_ingest_python_layer():
    F.case_python("cpu")


def test_rank_ingest_symbol_is_bound():
    F.case_symbols()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cpu_rank_ingest_under_asan_ubsan():
    """gk_rank_ingest_keyed of the host engine under ASan + UBSan, a stand-alone
    program: the fused call against the two-call composition, and its refusals."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "sketches-py_amd", "cpu"), "sanitize-rankingest"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "cpu_rankingest_selftest: ok" in r.stdout
