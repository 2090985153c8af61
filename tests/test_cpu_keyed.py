"""Keyed ingest on the host engine (device="cpu"): the cases of
tests/keyed_cases.py bit for bit against numpy's stable sort and the oracle's
per-sample loop, and the ASan + UBSan program tests/cpu_keyed_selftest.cpp
(host engine vs the C oracle)."""
import os
import re
import shutil
import subprocess

import pytest

import keyed_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(C.GROUP_CASES))
def test_cpu_group_by_key_matches_stable_sort(name):
    C.case_group("cpu", name)


def test_cpu_group_by_key_int64_ids():
    C.case_group("cpu", "skips_second_digit", int64_ids=True)


@pytest.mark.parametrize("eps", [0.1, 0.01])
def test_cpu_ingest_keyed_matches_oracle_loop(eps):
    C.case_oracle_loop("cpu", eps)


def test_cpu_ingest_keyed_equals_csr_ingest():
    C.case_equals_csr("cpu")


def test_cpu_keyed_errors_leave_state():
    C.case_errors("cpu")


def test_cpu_keyed_empty_batch_with_query():
    C.case_empty_with_query("cpu")


def test_group_kernels_do_not_spill(tmp_path):
    """The k_group_* / k_scan_* kernels of gk_keyed.hip compile for gfx950
    without scratch (no register spills), and the scatter's LDS leaves room
    for four workgroups in a CU's 160 KiB."""
    csrc = os.path.join(ROOT, "sketches-py_amd", "csrc")
    r = subprocess.run(
        ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-Rpass-analysis=kernel-resource-usage", "-c",
         os.path.join(csrc, "gk_keyed.hip"), "-o", str(tmp_path / "k.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert any("k_group_scatter" in n for n in names) and any("k_scan_apply" in n for n in names), names
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(scratch) == len(names) and not any(scratch), list(zip(names, scratch))
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert max(lds) <= 40 * 1024, max(lds)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cpu_keyed_under_asan_ubsan():
    """Case 6: gk_group_by_key / gk_ingest_keyed of the host engine under ASan +
    UBSan, a stand-alone program checked against the C oracle."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "sketches-py_amd", "cpu"), "sanitize-keyed"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "cpu_keyed_selftest: ok" in r.stdout
