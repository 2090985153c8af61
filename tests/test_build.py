"""Build-level invariants of the HIP kernels (no GPU needed: hipcc
cross-compiles for gfx950 here)."""
import glob
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sketches-py_amd", "csrc")


@pytest.fixture(scope="module")
def units():
    """Every unit of csrc compiled once, with the Makefile's flags, by
    tools/isa_diff.py: {unit: (device assembly, resource remarks)} and the
    module itself."""
    spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(ROOT, "tools", "isa_diff.py"))
    isa_diff = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa_diff)
    return isa_diff, isa_diff.compile_tree(ROOT)


@pytest.fixture(scope="module")
def small_unit(units):
    """(assembly, remarks) of the unit that holds k_ingest_small."""
    small = [u for u in units[1].values() if any(n.startswith("_Z14k_ingest_small") for n in u[1])]
    assert len(small) == 1
    return small[0]


@pytest.fixture(scope="module")
def resource_report(small_unit):
    return {k: {n: int(x) for n, x in v.items() if x.isdigit()} for k, v in small_unit[1].items()}


@pytest.fixture(scope="module")
def small_isa(small_unit):
    text = small_unit[0]
    bodies = {}
    for m in re.finditer(r"^(_Z14k_ingest_small\w+):", text, re.M):
        end = text.index("s_endpgm", m.end())
        bodies[m.group(1)] = text[m.end():end]
    return bodies


def test_fast_class_has_no_scratch(resource_report, small_isa):
    """The small class runs nearly every stream: no scratch traffic in the
    per-flush path.  The allocator folds a few loop-invariant per-lane
    addresses into scratch, stored at kernel entry and reloaded per stream or
    per stats batch (loop depth <= 1 in the ISA's loop annotations); a spill
    inside the flush loop (depth >= 2) costs a memory round trip per flush
    and fails this test.  Since round 6 every (VPL, stats role) instance is
    built twice, for 7 waves per SIMD (72 VGPRs, the product) and for 6 (80
    VGPRs: launches of few streams per wave), 8 instances; the 7-wave
    stats-role instances carry the most (<= 40 scratch instructions, all per
    stream / per batch: profiles/r06/r07_waves_per_simd_ab.txt)."""
    fast = {k: v for k, v in resource_report.items() if k.startswith("_Z14k_ingest_small")}
    assert len(fast) == 8
    for k, v in fast.items():
        assert v.get("ScratchSize [bytes/lane]", 0) <= 96, (k, v)
    for name, body in small_isa.items():
        depth = 0
        inner = []
        total = 0
        for line in body.splitlines():
            if line.startswith(".LBB") or line.startswith("; %bb"):
                m = re.search(r"Loop: Header=\S+ Depth=(\d+)", line)
                depth = int(m.group(1)) if m else 0
            if re.match(r"^\s*scratch_\w+", line):
                total += 1
                if depth >= 2:
                    inner.append(line.strip())
        assert not inner, (name, inner)
        assert total <= 40, (name, total)


def test_no_inline_asm_memory_ops():
    """Inline-asm loads were rejected: the compiler may copy an asm output
    register before the load lands (tools/check_async_loads.py found such
    copies).  Memory operations in the kernels stay compiler-visible: in
    every kernel unit and every header of csrc."""
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert os.path.join(CSRC, "gk_ops.hip") in files and os.path.join(CSRC, "gk_dev.h") in files
    for f in files:
        for m in re.finditer(r'asm\s+volatile\s*\(\s*"([^"]*)"', open(f).read()):
            assert "load" not in m.group(1) and "store" not in m.group(1), (f, m.group(1))


def test_every_kernel_lives_in_one_unit(units):
    """The library is linked without relocatable device code: a kernel or a
    noinline device function that two units define would be two copies.
    Every unit of csrc compiles for gfx950 with the Makefile's flags, and no
    function name comes out of two of them."""
    isa_diff, compiled = units
    assert set(compiled) == {os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "*.hip"))}
    where, remarks = {}, []
    for unit, (text, res) in compiled.items():
        for n in isa_diff.functions(text):
            assert n not in where, (n, where[n], unit)
            where[n] = unit
        remarks += list(res)
    assert len(set(remarks)) == len(remarks) >= 48, len(remarks)
    assert set(remarks) <= set(where)


def test_fast_class_occupancy(resource_report):
    """The 7-wave build reaches 7 waves per SIMD (the persistent grid assumes
    it), the 6-wave build 6; LDS stays small enough for 7 x 4 waves per CU."""
    ks = {n: v for n, v in resource_report.items() if n.startswith("_Z14k_ingest_smallILi2E")}
    assert ks
    for n, k in ks.items():
        want = 7 if "Li7E" in n else 6
        assert k["Occupancy [waves/SIMD]"] >= want, (n, k)
        assert k["LDS Size [bytes/block]"] * 28 <= 160 * 1024, (n, k)
