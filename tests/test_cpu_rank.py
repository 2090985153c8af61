"""Rank queries on the host engine (device="cpu"): the cases of
tests/rank_cases.py, bit for bit against the contract of include/gk_capi.h
applied to the oracle's tables, and the ASan + UBSan program
tests/cpu_rank_selftest.cpp (host engine vs the C oracle)."""
import os
import shutil
import subprocess

import pytest

import rank_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("run", K.MIXED_RUNS)
def test_cpu_rank_mixed_set(run):
    K.case_mixed("cpu", run)


def test_cpu_rank_select():
    K.case_select("cpu")


def test_cpu_rank_equivalences():
    K.case_equivalences("cpu")


def test_cpu_rank_long_descending_streams():
    K.case_promoted("cpu")


def test_cpu_rank_long_table():
    K.case_long_table("cpu")


def test_cpu_rank_bracket_on_ingest_only_streams():
    K.case_bracket("cpu")


def test_cpu_rank_merged_histories():
    K.case_merged("cpu")


def test_cpu_rank_errors_leave_state():
    K.case_errors("cpu")


def test_cpu_rank_dropin_and_cdf():
    K.case_dropin("cpu")


def test_rank_symbols_are_bound():
    K.case_symbols()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cpu_rank_under_asan_ubsan():
    """The two rank calls of the host engine under ASan + UBSan, a stand-alone
    program checked against the formula over the C oracle's tables."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "sketches-py_amd", "cpu"), "sanitize-rank"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "cpu_rank_selftest: ok" in r.stdout
