"""Compaction on the host engine (device="cpu"): one unbounded class, nothing to
demote -- gk_compact returns unused buffer capacity and changes no stream, and
gk_class_usage knows class 0 alone.  The cases of tests/compact_cases.py that
apply, and the ASan + UBSan program tests/cpu_compact_selftest.cpp (host engine
vs the C oracle)."""
import os
import shutil
import subprocess

import pytest

import compact_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpu_compact_noop_and_idempotence():
    X.case_noop("cpu")


@pytest.mark.parametrize("seed", [71, 72, 73])
def test_cpu_compact_random_sequences(seed):
    assert X.case_random("cpu", seed) == 0  # demoted


def test_cpu_compact_keyed_churn():
    X.case_keyed_churn("cpu")


def test_cpu_compact_arguments():
    X.case_arguments("cpu")


def test_cpu_compact_arena_bytes_do_not_grow():
    """class_usage() has one entry; its arena_bytes covers what the streams
    hold and does not grow across compact()."""
    import select_cases as C
    ss, _ = C.make("cpu", C.MIXED)
    ss.reset_select(C.i32([8, 9, 14]))  # 1000, 1500 and 1000 values: cleared buffers keep their capacity
    (before,) = ss.class_usage()
    st = ss.stats()
    held = 24 * int(st["size"].sum()) + 8 * int(st["pending"].sum())
    assert before["arena_bytes"] >= held and before["workspace_bytes"] == 0
    res = ss.compact()
    (after,) = ss.class_usage()
    assert res == {"demoted": 0, "bytes_freed": before["arena_bytes"] - after["arena_bytes"]}
    assert held <= after["arena_bytes"] <= before["arena_bytes"]
    assert {k: after[k] for k in ("streams", "slots_used", "slots_alloc")} == dict.fromkeys(
        ("streams", "slots_used", "slots_alloc"), len(C.MIXED))


def test_compact_symbols_are_bound():
    X.case_symbols()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cpu_compact_under_asan_ubsan():
    """gk_compact / gk_class_usage of the host engine under ASan + UBSan, a
    stand-alone program checked against the C oracle."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "sketches-py_amd", "cpu"), "sanitize-compact"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "cpu_compact_selftest: ok" in r.stdout
