"""Cases of the stream transfer (gk_pack_select / gk_unpack_select through
StreamSet.pack_select / unpack_select / take / put / resized), shared by
tests/test_gpu_transfer.py (device engine) and tests/test_cpu_transfer.py (host
engine); the engine is the ``dev`` parameter.

The expected state is the oracle's: one ``OracleGK`` per stream, moved between
Python lists with ``copy.deepcopy`` exactly as the streams are moved between
sets.  Every comparison is bit for bit (v, pending values and the float header
words by bit pattern, sign of zero included), pending values unflushed.
Test infrastructure only."""
import copy
import struct

import numpy as np
import pytest
import torch

import parity_util as U
import rank_cases as K
import rollup_cases as R
import select_cases as C
from gk_oracle import OracleGK

EPS = C.EPS
HEADER = 64  # bytes of a packed state's header (csrc/gk_pack.h)


def align256(x):
    return (x + 255) & ~255


def layout(S, E, P):
    """Section offsets of a GKPACK01 buffer (csrc/gk_pack.h), restated."""
    o = align256(HEADER)
    L = {}
    for name, nbytes in (("n", 8 * S), ("min", 8 * S), ("max", 8 * S), ("sum", 8 * S), ("avg", 8 * S),
                         ("eoffs", 8 * (S + 1)), ("poffs", 8 * (S + 1)), ("v", 8 * E), ("g", 4 * E), ("d", 4 * E),
                         ("pv", 8 * P)):
        L[name] = o
        o = align256(o + nbytes)
    L["total"] = o
    return L


def header_of(buf):
    raw = bytes(buf[:HEADER].cpu().numpy())
    magic, version, hbytes, eps, S, E, P, total, _ = struct.unpack("<8sIIdqqqqQ", raw)
    return dict(magic=magic, version=version, header_bytes=hbytes, eps=eps, S=S, E=E, P=P, bytes=total)


def section(buf, L, name, dtype, count):
    a = buf.cpu().numpy()
    return a[L[name]:L[name] + count * np.dtype(dtype).itemsize].view(dtype)


def patched(buf, offset, raw):
    """A copy of the packed buffer with bytes [offset, offset + len(raw)) replaced."""
    b = buf.clone()
    b[offset:offset + len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(b.device)
    return b


def copies(oracles, ids):
    return [copy.deepcopy(oracles[s]) for s in ids]


def same_snapshot(ss, before, what):
    after = R.snapshot(ss)
    for s in range(ss.num_streams):
        R.assert_stream(R.stream_of_snapshot(after, s), R.stream_of_snapshot(before, s),
                        "%s: stream %d vs its state before the call" % (what, s))


def mixed(dev):
    """select_cases.MIXED with D(190) (stream 10) flushed: a 138-entry table, in
    class 1 on the GPU engine."""
    ss, orc = C.make(dev, C.MIXED)
    ss.flush_select(C.i32([10]))
    orc[10].size()
    assert C.sizes(ss, 10) == (138, 0) and len(orc[10].v) == 138
    return ss, orc


# --------------------------------------------------------------- case 1: take
def case_take(dev):
    ss, orc = mixed(dev)
    ids = C.MIXED_IDS  # unsorted, stream 3 twice, stream 0 has n = 0
    assert orc[0].n == 0 and ids.count(3) == 2 and sum(1 for s in ids if orc[s].pending) >= 5
    before = R.snapshot(ss)
    promoted = ss.num_promoted
    if dev != "cpu":
        assert promoted >= 1
    t = ss.take(C.i32(ids))
    assert t.num_streams == len(ids) and t.eps == ss.eps and t.device == ss.device
    R.assert_set_matches(t, copies(orc, ids), "take")
    same_snapshot(ss, before, "take (source)")
    C.assert_all(ss, orc, "take (source vs oracle)")
    assert ss.num_promoted == promoted
    return ss, orc, t


# ------------------------------------------------------- case 2: continuation
B_SPECS = [(1, 150, 971), (2, 640, 972), (0, 57, 973), ("D", 750, 0), (3, 333, 974), (0, 0, 975), (5, 1000, 976),
           (1, 50, 977), (7, 202, 978), (6, 101, 979), (4, 99, 980), (1, 1500, 981)]
MOVE_FROM = [10, 11, 4, 0, 9]   # of A: class 1 table, pending values, flush point, empty, 1500 values
MOVE_TO = [7, 2, 9, 5, 0]       # of B, all with their own history (5 is empty)


def case_continuation(dev):
    """The guarantee: moved streams and their neighbours continue exactly as
    oracles moved the same way."""
    a, oa = mixed(dev)
    b, ob = C.make(dev, B_SPECS)
    t = a.take(C.i32(MOVE_FROM))
    before_b = R.snapshot(b)
    b.put(C.i32(MOVE_TO), t)
    for src, dst in zip(MOVE_FROM, MOVE_TO):
        ob[dst] = copy.deepcopy(oa[src])
    C.assert_all(b, ob, "put", before_b, set(MOVE_TO))
    C.assert_all(a, oa, "take left the source")
    R.assert_set_matches(t, copies(oa, MOVE_FROM), "the taken set after put")
    # more values into every stream of both sets
    for ss, orc, seed in ((a, oa, 0), (b, ob, 100)):
        extra = [C.more_values(seed + s, 253 + 11 * s) for s in range(ss.num_streams)]
        U.ingest_np(ss, extra)
        for o, x in zip(orc, extra):
            o.add_many(x)
        C.assert_all(ss, orc, "continued ingest")
    # ranks of moved and unmoved streams (flushes the covered ones), then a
    # flush of a few others, then quantiles of everything
    xs = [-1.0, 0.5, 1.0, 3.0, 100.0, 3900.0]
    K.check_ranks(b, ob, [7, 3, 2, 11], xs, "ranks after put")
    K.check_ranks(a, oa, [10, 12, 0], xs, "ranks in the source")
    b.flush_select(C.i32([9, 4]))
    for s in (9, 4):
        ob[s].size()
    C.assert_all(b, ob, "flush after put")
    # a moved stream merged with an unmoved one: c[0].merge(b[7]); c[0].merge(b[3])
    c, oc = C.make(dev, [(1, 57, 985), (0, 0, 986)])
    R.check_rollup(c, b, oc, ob, [[7, 3], [0]], "merge of a moved stream", quantiles=False)
    for ss, orc in ((a, oa), (b, ob), (c, oc)):
        R.assert_quantiles(ss, orc, "continuation")
        C.assert_all(ss, orc, "continuation after quantiles()")


# ----------------------------------------- case 3: byte identity with gk_pack
def case_bytes_vs_pack(dev):
    ss, _ = mixed(dev)
    S = ss.num_streams
    n = ss.pack_bytes()
    assert ss.pack_select_bytes(torch.arange(S, dtype=torch.int32)) == n
    whole = ss.pack(torch.zeros(n + 512, dtype=torch.uint8, device=ss.device))
    sel = ss.pack_select(torch.arange(S, dtype=torch.int32), torch.zeros(n + 512, dtype=torch.uint8, device=ss.device))
    assert bytes(whole.cpu().numpy()) == bytes(sel.cpu().numpy())
    # (bytes past the packed size stayed zero in both)
    assert not sel[n:].any().item()


# ------------------------------ case 4: lane and offset edges, without the oracle
EDGE_E = [0, 1, 63, 64, 65, 127]
EDGE_P = [0, 1, 63, 64, 65, 100]


def synthetic_state(rng, sizes, pends, P=101):
    S = len(sizes)
    offs = np.zeros(S + 1, np.int64)
    offs[1:] = np.cumsum(sizes)
    poffs = np.zeros(S + 1, np.int64)
    poffs[1:] = np.cumsum(pends)
    E, Pt = int(offs[-1]), int(poffs[-1])
    v = np.concatenate([np.sort(rng.normal(0, 5, e)) for e in sizes] + [np.zeros(0)])
    if E:
        v[0] = -0.0
    g = rng.integers(1, 9, max(E, 1)).astype(np.int32)[:E]
    d = rng.integers(0, 7, max(E, 1)).astype(np.int32)[:E]
    pv = rng.lognormal(0, 1, Pt)
    if Pt:
        pv[-1] = -0.0
    # n with p <= n mod P (gk_import's rule), and at least the table's g sum
    n = np.asarray([P * (10 + s) + p for s, p in enumerate(pends)], np.int64)
    st = dict(offs=offs, v=v, g=g, d=d, poffs=poffs, pv=pv, n=n, mn=rng.normal(0, 1, S), mx=rng.normal(9, 1, S),
              sm=rng.normal(0, 100, S), av=rng.normal(0, 1, S))
    return st


def import_synthetic(dev, st, eps=EPS):
    S = len(st["n"])
    ss = U._ss(S, eps, dev)
    t = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in st.items()}
    for k in ("v", "g", "d", "pv"):
        if t[k].numel() == 0:
            t[k] = torch.zeros(1, dtype=t[k].dtype, device=t[k].device)
    ss.import_arrays(t["offs"], t["v"], t["g"], t["d"], t["poffs"], t["pv"], t["n"], t["mn"], t["mx"], t["sm"], t["av"])
    ss.sync()
    return ss


def assert_state_arrays(st, rows, exp, what):
    """export_state() arrays `st` against rows `rows` of the synthetic state `exp` (numpy only)."""
    eo, po = exp["offs"], exp["poffs"]
    rows = np.asarray(rows, np.int64)
    es, ps = (eo[1:] - eo[:-1])[rows], (po[1:] - po[:-1])[rows]
    assert np.array_equal(st["offs"], np.concatenate([[0], np.cumsum(es)])), what + " table offsets"
    assert np.array_equal(st["poffs"], np.concatenate([[0], np.cumsum(ps)])), what + " pending offsets"
    gather = np.concatenate([np.arange(eo[r], eo[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    pgather = np.concatenate([np.arange(po[r], po[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    assert st["v"].view(np.int64).tobytes() == exp["v"][gather].view(np.int64).tobytes(), what + " v"
    assert np.array_equal(st["g"], exp["g"][gather]) and np.array_equal(st["d"], exp["d"][gather]), what + " g / d"
    assert st["pv"].view(np.int64).tobytes() == exp["pv"][pgather].view(np.int64).tobytes(), what + " pending"
    assert np.array_equal(st["n"], exp["n"][rows]), what + " n"
    for a, b in (("min", "mn"), ("max", "mx"), ("sum", "sm"), ("avg", "av")):
        assert st[a].view(np.int64).tobytes() == exp[b][rows].view(np.int64).tobytes(), what + " " + a


def case_edges(dev):
    rng = np.random.default_rng(4)
    sizes = [e for e in EDGE_E for _ in EDGE_P]
    pends = [p for _ in EDGE_E for p in EDGE_P]
    exp = synthetic_state(rng, sizes, pends)
    src = import_synthetic(dev, exp)
    S = src.num_streams
    assert_state_arrays(R.snapshot(src), np.arange(S), exp, "imported")
    rows = rng.permutation(S)
    buf = src.pack_select(torch.from_numpy(rows.astype(np.int32)))
    h = header_of(buf)
    assert (h["magic"], h["version"], h["header_bytes"], h["eps"], h["S"]) == (b"GKPACK01", 1, HEADER, EPS, S)
    assert h["bytes"] == buf.numel() == layout(S, h["E"], h["P"])["total"]
    dst = U._ss(S + 3, EPS, dev)
    where = rng.permutation(S + 3)[:S]
    dst.unpack_select(torch.from_numpy(where.astype(np.int32)), buf)
    got = dst.take(torch.from_numpy(where.astype(np.int32)))
    assert_state_arrays(R.snapshot(got), rows, exp, "unpacked")
    # the three unlisted streams of dst are still empty
    rest = sorted(set(range(S + 3)) - set(int(x) for x in where))
    st = dst.stats_select(C.i32(rest))
    assert st["n"].cpu().tolist() == [0, 0, 0] and st["size"].cpu().tolist() == [0, 0, 0]
    assert_state_arrays(R.snapshot(src), np.arange(S), exp, "the source after pack_select")


# ----------------------------------------------------- case 5: scan boundaries
def case_scan(dev, nrows):
    """Rows past each internal boundary of the device scan (2048-entry tiles,
    1024 tile sums per round of the middle kernel): a 64-stream set of streams
    with n <= 3 (empty tables, up to 3 pending values), repeated ids."""
    rng = np.random.default_rng(nrows)
    S = 64
    pends = [int(x) for x in rng.integers(0, 4, S)]
    pends[:4] = [0, 1, 2, 3]
    exp = synthetic_state(rng, [0] * S, pends)
    exp["n"] = np.asarray(pends, np.int64)  # n <= 3, p == n mod 101
    ss = import_synthetic(dev, exp)
    ids = rng.integers(0, S, nrows).astype(np.int32)
    buf = ss.pack_select(torch.from_numpy(ids))
    h = header_of(buf)
    p_of = np.asarray(pends, np.int64)[ids]
    assert (h["S"], h["E"], h["P"]) == (nrows, 0, int(p_of.sum()))
    L = layout(nrows, 0, h["P"])
    assert buf.numel() == h["bytes"] == L["total"]
    assert not section(buf, L, "eoffs", np.int64, nrows + 1).any()
    po = np.concatenate([[0], np.cumsum(p_of)])
    assert np.array_equal(section(buf, L, "poffs", np.int64, nrows + 1), po)
    assert np.array_equal(section(buf, L, "n", np.int64, nrows), exp["n"][ids])
    for name, key in (("min", "mn"), ("max", "mx"), ("sum", "sm"), ("avg", "av")):
        assert np.array_equal(section(buf, L, name, np.int64, nrows), exp[key][ids].view(np.int64)), name
    # pending values: a vectorised gather of the source's
    start = exp["poffs"][:-1][ids]
    idx = np.repeat(start - po[:-1], p_of) + np.arange(int(p_of.sum()))
    assert np.array_equal(section(buf, L, "pv", np.int64, h["P"]), exp["pv"][idx].view(np.int64))


# ------------------------------------------- case 6: promotion on unpack (GPU)
def DL(n):
    """A descending run of n values (select_cases.D stops at 4000)."""
    return np.arange(float(n))[::-1].copy()


def case_promotion(dev):
    """(GK_CAPS=128,256,512,4096 set by the caller) tables sized for classes 1,
    2 and 3 are installed into class-0 streams; a small table into a stream
    already in class 2, which keeps its class."""
    seqs = [C.D(190), C.D(1500), DL(60000), R.seq(1, 150, 991)]
    src_o = []
    for x in seqs:
        o = OracleGK(EPS)
        o.add_many(x)
        o.size()
        src_o.append(o)
    sizes = [len(o.v) for o in src_o]
    assert sizes[0] == 138 and sizes[1] == 285 and 512 <= sizes[2] < 4095 and sizes[3] < 128, sizes
    src = U._ss(4, EPS, dev)
    U.ingest_np(src, seqs)
    src.flush()
    assert src.capacity(1) == 256 and src.capacity(2) == 512 and src.capacity(3) == 4096
    R.assert_set_matches(src, src_o, "promotion source")
    # dst: stream 3 sits in class 2 (D(1500), 275 + 86 pending -> flushed 285), the others in class 0
    dspecs = [(1, 150, 992), (2, 50, 993), (0, 57, 994), ("D", 1500, 0), (1, 150, 995), (0, 0, 996), (3, 99, 997)]
    dst, dst_o = C.make(dev, dspecs)
    dst.flush_select(C.i32([3]))
    dst_o[3].size()
    assert C.sizes(dst, 3) == (285, 0)
    assert dst.num_promoted == 1
    before = R.snapshot(dst)
    where = [4, 0, 5, 3]  # classes 1, 2, 3 into class-0 streams; the small table into the class-2 stream
    dst.put(C.i32(where), src)
    for k, s in enumerate(where):
        dst_o[s] = copy.deepcopy(src_o[k])
    C.assert_all(dst, dst_o, "promotion on unpack", before, set(where))
    assert dst.num_promoted == 4  # streams 4, 0, 5 moved up; 3 stayed where it was
    # all continue ingesting
    extra = [C.more_values(40 + s, 300 + 7 * s) for s in range(len(dspecs))]
    U.ingest_np(dst, extra)
    for o, x in zip(dst_o, extra):
        o.add_many(x)
    C.assert_all(dst, dst_o, "promotion on unpack, continued")
    R.assert_quantiles(dst, dst_o, "promotion on unpack, continued")
    assert dst.num_promoted == 4


# ----------------------------------------------------------------- case 7: errors
def case_errors(dev):
    from gkarray_amd import UnequalEpsilonException
    from gkarray_amd._lib import GK_E_ARG, GK_E_FORMAT, GKBackendError
    ss, orc = mixed(dev)
    S = ss.num_streams
    ids = [11, 3, 8]
    good = ss.pack_select(C.i32(ids))
    h = header_of(good)
    L = layout(3, h["E"], h["P"])
    st0 = R.snapshot(ss)
    other_eps = C.make(dev, [(1, 150, 911), (1, 50, 913), (0, 0, 915)], eps=0.02)[0].pack()
    eo = section(good, L, "eoffs", np.int64, 4).copy()
    assert eo[1] > 0 and eo[3] > eo[2]  # (stream 3, 99 values, has no table yet: eo[2] == eo[1])
    n = section(good, L, "n", np.int64, 3).copy()
    po = section(good, L, "poffs", np.int64, 4).copy()
    assert (po[1] - po[0], n[0] % 101) == (49, 49)  # stream 11: 150 values, 49 pending
    i64 = lambda x: struct.pack("<q", int(x))
    short = torch.zeros(good.numel() - 256, dtype=torch.uint8, device=ss.device)
    bad = [
        ("pack id == S", lambda: ss.pack_select(C.i32([11, 3, S, -5])), GK_E_ARG, "ids[2] = %d" % S),
        ("pack id == -1", lambda: ss.pack_select(C.i32([11, -1])), GK_E_ARG, "ids[1] = -1"),
        ("bytes id == S", lambda: ss.pack_select_bytes(C.i32([S])), GK_E_ARG, "ids[0] = %d" % S),
        ("short pack buffer", lambda: ss.pack_select(C.i32(ids), short), GK_E_ARG, "needs %d bytes" % good.numel()),
        ("unpack id == S", lambda: ss.unpack_select(C.i32([1, S, 2]), good), GK_E_ARG, "ids[1] = %d" % S),
        ("unpack id == -1", lambda: ss.unpack_select(C.i32([-1, 5, 2]), good), GK_E_ARG, "ids[0] = -1"),
        ("unpack duplicate id", lambda: ss.unpack_select(C.i32([4, 7, 4]), good), GK_E_ARG, "more than once"),
        ("header S != count", lambda: ss.unpack_select(C.i32([4, 7]), good), GK_E_ARG, "3 streams"),
        ("flipped magic byte", lambda: ss.unpack_select(C.i32([4, 7, 2]), patched(good, 3, b"\x00")), GK_E_FORMAT,
         "not a packed"),
        ("version 2", lambda: ss.unpack_select(C.i32([4, 7, 2]), patched(good, 8, struct.pack("<I", 2))), GK_E_FORMAT,
         "version"),
        ("byte count", lambda: ss.unpack_select(C.i32([4, 7, 2]), patched(good, 48, i64(h["bytes"] + 256))),
         GK_E_FORMAT, "inconsistent"),
        ("decreasing offset", lambda: ss.unpack_select(C.i32([4, 7, 2]), patched(good, L["eoffs"] + 8, i64(eo[2] + 1))),
         GK_E_FORMAT, "monotone"),
        ("first offset != 0", lambda: ss.unpack_select(C.i32([4, 7, 2]), patched(good, L["poffs"], i64(1))),
         GK_E_FORMAT, "monotone"),
        ("pending beyond n mod P", lambda: ss.unpack_select(C.i32([4, 7, 2]), patched(good, L["n"], i64(n[0] - 1))),
         GK_E_ARG, "pending"),
        ("negative n", lambda: ss.unpack_select(C.i32([4, 7, 2]), patched(good, L["n"] + 8, i64(-5))), GK_E_ARG,
         "pending"),
    ]
    for what, call, code, text in bad:
        with pytest.raises(GKBackendError) as ei:
            call()
        assert ei.value.code == code, (what, ei.value)
        assert text in str(ei.value), (what, ei.value)
        same_snapshot(ss, st0, "after '%s'" % what)
    with pytest.raises(UnequalEpsilonException):
        ss.unpack_select(C.i32([4, 7, 2]), other_eps)
    same_snapshot(ss, st0, "after the eps mismatch")
    # count == 0 on both calls: a packed state of zero streams, validated on the way in
    empty = ss.pack_select(C.i32([]))
    he = header_of(empty)
    assert empty.numel() == layout(0, 0, 0)["total"] == he["bytes"] and (he["S"], he["E"], he["P"]) == (0, 0, 0)
    assert ss.pack_select_bytes(C.i32([])) == empty.numel()
    ss.unpack_select(C.i32([]), empty)
    with pytest.raises(GKBackendError) as ei:
        ss.unpack_select(C.i32([]), good)  # its S must be 0
    assert ei.value.code == GK_E_ARG
    same_snapshot(ss, st0, "after count == 0")
    C.assert_all(ss, orc, "after the refused calls")
    # and a valid call still works
    ss.unpack_select(C.i32([4, 7, 2]), good)
    for k, s in zip(ids, [4, 7, 2]):
        orc[s] = copy.deepcopy(orc[k])
    C.assert_all(ss, orc, "valid call after the errors", st0, {4, 7, 2})


def case_overflow(dev):
    """(GK_CAPS=128,256 set by the caller; GPU only) a table of more than 255
    entries does not fit the last class: GK_E_OVERFLOW, nothing changed."""
    from gkarray_amd import StreamSet
    from gkarray_amd._lib import GK_E_OVERFLOW, GKBackendError
    o = OracleGK(EPS)
    o.add_many(C.D(1500))
    o.size()
    assert len(o.v) == 285
    src = StreamSet(2, EPS, device="cpu")  # (the host engine has no classes)
    U.ingest_np(src, [C.D(1500), R.seq(1, 150, 998)])
    src.flush_select(C.i32([0]))
    ss, orc = C.make(dev, [(1, 150, 951), (2, 50, 953), (0, 57, 954)])
    assert ss.capacity(1) == 256 and ss.capacity(2) == -1
    st0 = R.snapshot(ss)
    with pytest.raises(GKBackendError) as ei:
        ss.put(C.i32([2, 0]), src)
    assert ei.value.code == GK_E_OVERFLOW, ei.value
    same_snapshot(ss, st0, "after GK_E_OVERFLOW")
    assert ss.num_promoted == 0
    # the 150-value stream alone fits
    ss.put(C.i32([1]), src.take(C.i32([1])))
    orc[1] = OracleGK(EPS)
    orc[1].add_many(R.seq(1, 150, 998))
    C.assert_all(ss, orc, "valid put after GK_E_OVERFLOW", st0, {1})


# ------------------------------------------ case 8: deferred work first (GPU only)
def case_deferred(dev):
    """(GK_POOL_SLOTS=2 set by the caller) an ingest left in flight defers most
    of its overflowing streams; pack_select re-runs them before it reads."""
    specs = [("D", 600 + 75 * k, 0) if k % 4 else (k % 8, 150 + 50 * k, 960 + k) for k in range(14)]
    ss = U._ss(len(specs), EPS, dev)
    flat, offs = U.csr([C.seq(sp) for sp in specs])
    tf, to = torch.from_numpy(flat).to(dev), torch.from_numpy(offs).to(dev)
    ss.ingest(tf, to, sync=False)
    orc = [C.oracle_of(EPS, sp) for sp in specs]
    ids = [13, 1, 4, 2, 9, 1]
    t = ss.take(C.i32(ids))
    R.assert_set_matches(t, copies(orc, ids), "deferred take")
    assert ss.num_promoted > 2  # more streams than the 2 slots a class started with: some were deferred
    C.assert_all(ss, orc, "deferred")


# ------------------------------------------------ case 9: across engines (GPU)
def case_across_engines(dev):
    a, oa = mixed(dev)
    ids = [10, 11, 0, 8]
    h = a.take(C.i32(ids), device="cpu")
    assert h.is_cpu and h.num_streams == len(ids)
    oh = copies(oa, ids)
    R.assert_set_matches(h, oh, "take to the host engine")
    # the host set goes on for a while, then comes back into a second GPU set
    extra = [C.more_values(60 + s, 120) for s in range(len(ids))]
    U.ingest_np(h, extra)
    for o, x in zip(oh, extra):
        o.add_many(x)
    R.assert_set_matches(h, oh, "host engine, continued")
    b, ob = C.make(dev, B_SPECS)
    where = [6, 1, 11, 5]
    before = R.snapshot(b)
    b.put(C.i32(where), h)
    for k, s in enumerate(where):
        ob[s] = copy.deepcopy(oh[k])
    C.assert_all(b, ob, "put from the host engine", before, set(where))
    extra = [C.more_values(80 + s, 253) for s in range(b.num_streams)]
    U.ingest_np(b, extra)
    for o, x in zip(ob, extra):
        o.add_many(x)
    C.assert_all(b, ob, "back on the GPU, continued")
    R.assert_quantiles(b, ob, "back on the GPU, continued")


# ------------------------------------------------- case 10: the Python surface
def case_python_surface(dev):
    ss, orc = mixed(dev)
    S = ss.num_streams
    before = R.snapshot(ss)
    up = ss.resized(S + 5)
    assert up.num_streams == S + 5 and up.device == ss.device
    R.assert_set_matches(up, copies(orc, range(S)) + [OracleGK(EPS) for _ in range(5)], "resized up")
    down = ss.resized(7)
    assert down.num_streams == 7
    R.assert_set_matches(down, copies(orc, range(7)), "resized down")
    none = ss.resized(0)
    assert none.num_streams == 0
    same_snapshot(ss, before, "resized (the original)")
    # a grown set takes keyed samples for the new ids
    up.ingest_keyed(torch.tensor([S + 4, 2, S + 4], dtype=torch.int32), torch.tensor([3.0, 1.0, -0.0]))
    grown = copies(orc, range(S)) + [OracleGK(EPS) for _ in range(5)]
    grown[S + 4].add_many([3.0, -0.0])
    grown[2].add_many([1.0])
    R.assert_set_matches(up, grown, "resized up, keyed ingest")
    # put with a wrong-sized other; take of no ids
    with pytest.raises(ValueError):
        ss.put(C.i32([1, 2, 3]), down)
    with pytest.raises(ValueError):
        ss.put(C.i32([1]), "not a set")
    same_snapshot(ss, before, "refused put")
    t = ss.take(C.i32([]))
    assert t.num_streams == 0 and t.eps == ss.eps
    ss.put(torch.zeros(0, dtype=torch.int64), t)
    same_snapshot(ss, before, "take / put of no ids")
    # int64 ids, and a buffer handed in
    buf = torch.empty(ss.pack_select_bytes([3, 1]) + 100, dtype=torch.uint8, device=ss.device)
    assert ss.pack_select(torch.tensor([3, 1], dtype=torch.int64), buf) is buf
    with pytest.raises(ValueError):
        ss.pack_select(C.i32([3]), torch.empty(4096, dtype=torch.float32, device=ss.device))
    with pytest.raises(ValueError):
        ss.unpack_select(C.i32([3]), torch.zeros(8, dtype=torch.uint8))


def case_symbols():
    from gkarray_amd import _lib
    for name in ("gk_pack_select_bytes", "gk_pack_select", "gk_unpack_select"):
        assert name in _lib.SYMBOLS and name in _lib.CPU_SYMBOLS, name
        assert hasattr(_lib.load_cpu(), name), name
