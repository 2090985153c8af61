"""Stream transfer on the MI355X engine (k_pack_sizes / k_pack_select /
k_unpack_check / k_unpack_select through gk_pack_select / gk_unpack_select and
StreamSet.pack_select / unpack_select / take / put / resized): every case of
tests/transfer_cases.py, bit for bit against oracles moved the same way."""
import pytest

import transfer_cases as T

pytestmark = pytest.mark.gpu


def test_transfer_take_mixed_set(gpu_device):
    """Case 1: unsorted ids with a repeat and an empty stream; rows equal deep
    copies of the listed oracles, pending values unflushed; the source and its
    num_promoted are unchanged."""
    T.case_take(gpu_device)


def test_transfer_continuation(gpu_device):
    """Case 2: streams taken out of one set and put into another continue as
    oracles moved the same way: ingest, ranks, flush, merge, quantiles."""
    T.case_continuation(gpu_device)


def test_transfer_bytes_equal_pack(gpu_device):
    """Case 3: pack_select(arange(S)) is byte for byte pack()."""
    T.case_bytes_vs_pack(gpu_device)


def test_transfer_lane_and_offset_edges(gpu_device):
    """Case 4: table sizes and pending counts around the wave width."""
    T.case_edges(gpu_device)


@pytest.mark.parametrize("nrows", [2048, 2049, 1024 * 2048 + 1])
def test_transfer_scan_boundaries(gpu_device, nrows):
    """Case 5: one row past a scan tile, one past a round of the tile sums."""
    T.case_scan(gpu_device, nrows)


def test_transfer_promotion_on_unpack(gpu_device, monkeypatch):
    """Case 6: tables for classes 1, 2 and 3 into class-0 streams; a small
    table into a class-2 stream, which keeps its class."""
    monkeypatch.setenv("GK_CAPS", "128,256,512,4096")
    T.case_promotion(gpu_device)


def test_transfer_errors_leave_state(gpu_device):
    """Case 7: every refusal leaves the whole set as it was."""
    T.case_errors(gpu_device)


def test_transfer_overflow_past_last_class(gpu_device, monkeypatch):
    """Case 7, GPU only: a table of more than 255 entries on the ladder 128,256."""
    monkeypatch.setenv("GK_CAPS", "128,256")
    T.case_overflow(gpu_device)


def test_transfer_settles_deferred_streams_first(gpu_device, monkeypatch):
    """Case 8: with 2-slot arenas, streams an in-flight ingest deferred are
    re-run before pack_select reads them."""
    monkeypatch.setenv("GK_POOL_SLOTS", "2")
    T.case_deferred(gpu_device)


def test_transfer_across_engines(gpu_device):
    """Case 9: GPU -> host engine -> a second GPU set, continuing bit-exactly."""
    T.case_across_engines(gpu_device)


def test_transfer_python_surface(gpu_device):
    """Case 10: resized up and down, put with a wrong-sized other, take of no ids."""
    T.case_python_surface(gpu_device)
