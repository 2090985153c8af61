"""Keyed rank queries on the host engine (device="cpu"): the cases of
tests/rankkeyed_cases.py, bit for bit against the contract of
include/gk_capi.h applied to the oracle's tables, and the ASan + UBSan program
tests/cpu_rankkeyed_selftest.cpp (host engine vs the C oracle)."""
import os
import shutil
import subprocess

import pytest

import rankkeyed_cases as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def setenv(monkeypatch):
    return lambda k, v: monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)


def test_cpu_rank_keyed_boundaries(setenv):
    Q.case_boundaries("cpu", setenv)


def test_cpu_rank_keyed_thresholds():
    Q.case_thresholds("cpu")


def test_cpu_rank_keyed_equivalence():
    Q.case_equivalence("cpu")


def test_cpu_rank_keyed_negative_ids():
    Q.case_negative("cpu")


@pytest.mark.parametrize("S", [1, 257, 65537])
def test_cpu_rank_keyed_stream_counts(S):
    Q.case_radix("cpu", S)


def test_cpu_rank_keyed_long_table():
    Q.case_long_table("cpu")


def test_cpu_rank_keyed_long_descending_streams():
    Q.case_promoted("cpu")


def test_cpu_rank_keyed_refusals_leave_state(setenv):
    Q.case_refusals("cpu", setenv)


def test_cpu_rank_keyed_python_layer():
    Q.case_python("cpu")


def test_rank_keyed_symbol_is_bound():
    Q.case_symbols()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cpu_rank_keyed_under_asan_ubsan():
    """gk_ranks_keyed of the host engine under ASan + UBSan, a stand-alone
    program checked against the formula over the C oracle's tables."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "sketches-py_amd", "cpu"), "sanitize-rankkeyed"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "cpu_rankkeyed_selftest: ok" in r.stdout
