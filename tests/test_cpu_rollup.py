"""Group-by roll-up on the host engine (device="cpu"): the cases of
tests/rollup_cases.py bit for bit against the oracle, and the ASan + UBSan
program tests/cpu_rollup_selftest.cpp (host engine vs the C oracle)."""
import os
import shutil
import subprocess

import pytest

import rollup_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("pre", [False, True], ids=["fresh_dst", "preingested_dst"])
def test_cpu_rollup_mixed_groups(pre):
    C.case_mixed("cpu", pre)


def test_cpu_rollup_small_eps():
    C.case_small_eps("cpu")


def test_cpu_merge_and_merge_compress_ladder_case():
    C.case_merge_ladder("cpu")


def test_cpu_merge_of_source_with_records_below_min():
    C.case_merge_source_with_records_below_min("cpu")


def test_cpu_rollup_equals_merge_from():
    C.case_equivalence("cpu")


def test_cpu_rollup_by_key_order():
    C.case_by_key_order("cpu")


def test_cpu_rollup_errors_leave_state():
    C.case_errors("cpu")


def test_cpu_rollup_repeat_call_continues():
    C.case_repeat("cpu")


def test_rollup_engine_mismatch_is_value_error():
    from gkarray_amd import StreamSet

    class Other(StreamSet):
        is_cpu = False  # (stands for a device-engine set; no GPU needed for the check)

    a = StreamSet(2, 0.01, device="cpu")
    b = Other(3, 0.01, device="cpu")
    with pytest.raises(ValueError):
        a.rollup_from(b, [0, 1, 2], [0, 1])


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cpu_rollup_under_asan_ubsan():
    """Case 8: gk_rollup of the host engine under ASan + UBSan, a stand-alone
    program checked against the C oracle."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "sketches-py_amd", "cpu"), "sanitize-rollup"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "cpu_rollup_selftest: ok" in r.stdout
