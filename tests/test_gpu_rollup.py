"""Group-by roll-up on the MI355X engine (k_fold through gk_rollup /
StreamSet.rollup_from / rollup_by_key): every case of tests/rollup_cases.py,
bit for bit against the oracle's loop of GKArray.merge (gk:111-154)."""
import pytest

import rollup_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pre", [False, True], ids=["fresh_dst", "preingested_dst"])
def test_rollup_mixed_groups(gpu_device, pre):
    """Case 1: a 17-member group that crosses the 128-entry class mid-fold
    (promotion and resume), groups of 0, 1, 2 and 5, empty members first, only
    empty members, non-members with pending values."""
    C.case_mixed(gpu_device, pre)


def test_rollup_small_eps_global_workspace(gpu_device):
    """Case 2: eps = 0.001 (flush period 1001: the bitonic order of the pending
    values); the destination passes 2048 entries (the global-workspace class)."""
    C.case_small_eps(gpu_device)


def test_rollup_narrow_ladder_two_levels(gpu_device, monkeypatch):
    """Case 3: on the ladder 128,256,512,4096 the 17-member fold climbs two
    levels in one call."""
    monkeypatch.setenv("GK_CAPS", "128,256,512,4096")
    C.case_narrow_ladder(gpu_device)


def test_merge_and_merge_compress_climb_narrow_ladder(gpu_device, monkeypatch):
    """merge_from and merge_compress(entries) on the ladder 128,256,512,4096: a
    class-0 stream climbs inside each call, beside one that stays in class 0."""
    monkeypatch.setenv("GK_CAPS", "128,256,512,4096")
    C.case_merge_ladder(gpu_device)


def test_merge_of_source_with_records_below_min(gpu_device):
    """merge_from and rollup_from of source streams whose tables start below
    their _min (records from merge_compress): the converted list is sorted (gk:72)."""
    C.case_merge_source_with_records_below_min(gpu_device)


def test_merge_and_merge_compress_overflow_keep_state(gpu_device, monkeypatch):
    """GK_E_OVERFLOW of merge_from and merge_compress(entries) on the ladder
    128,200: the stream that did not fit is bit-identical to before the call
    (min / max included), the other stream complete, the source flushed."""
    monkeypatch.setenv("GK_CAPS", "128,200")
    C.case_merge_overflow(gpu_device)


def test_rollup_equals_merge_from(gpu_device):
    """Case 4: rollup_by_key(s % G) == merge_from of the source's slices."""
    C.case_equivalence(gpu_device)


def test_rollup_by_key_order(gpu_device):
    """Case 5: permuted keys with -1 == rollup_from with hand-built CSR."""
    C.case_by_key_order(gpu_device)


def test_rollup_errors_leave_state(gpu_device):
    """Case 6: every argument error leaves both sets bit-identical; a valid
    roll-up afterwards still matches the oracle."""
    C.case_errors(gpu_device)


def test_rollup_repeat_call_continues(gpu_device):
    """Case 7: a second roll-up into the same destination continues the fold."""
    C.case_repeat(gpu_device)


@pytest.mark.parametrize("caps,member", [("128,264", False), ("128,256", True)], ids=["destination", "member_flush"])
def test_rollup_overflow_past_last_class(gpu_device, monkeypatch, caps, member):
    """GK_E_OVERFLOW and the documented state: a destination that outgrows the
    last class holds the fold before the member that did not fit; a member
    whose own flush does not fit keeps its state and no destination is touched."""
    monkeypatch.setenv("GK_CAPS", caps)
    C.case_overflow(gpu_device, member)
