"""A/B of the keyed ingest on one MI355X (run by hand; not a test).

Data: the cfg3 batch (bench.make_input: 10^6 streams x 1000 Pareto values,
eps 0.01) in ARRIVAL ORDER, the round-robin interleave of the streams: sample
t of every stream before sample t+1 (ids = 0, 1, .., S-1, 0, 1, ..).
  A: ss.ingest_keyed(ids, values, quantiles=[.5, .9, .99]) -- the k_group_*
     radix partition, then the CSR ingest path.
  B: the way without it: stable torch.sort of the ids, gather of the values,
     bincount, cumsum, ss.ingest(grouped, offsets, quantiles=...).
  C: the plain CSR step on the already grouped batch (what both end in), and
     G: ss.group_by_key alone (the grouping kernels + one output allocation).
Every run starts from a reset set.  One warm-up run of each side, then --reps
interleaved repetitions, wall time around the synchronising calls; medians and
the peak torch.cuda.max_memory_allocated of each side are printed as one JSON
line (A's scratch is the library's own: device memory taken by A's first call
is reported beside it).  A's, B's and C's quantiles must be bit-equal.  If B
runs out of memory, that is said and both sides are taken at half the
--values, and so on.

The GPU work runs in a child process under its own time limit (--timeout).
--device cpu with small --streams / --values rehearses the logic on the host
engine; that is not a measurement.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = [0.5, 0.9, 0.99]


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=1_000_000)
    ap.add_argument("--values", type=int, default=1000, help="values per stream")
    ap.add_argument("--eps", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--timeout", type=int, default=900, help="seconds for the child that does the GPU work")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def group_bytes_per_sample(S):
    """Algorithmic bytes the grouping kernels move per sample: every radix pass
    reads the ids for the tile counts, reads the pair and writes the pair."""
    bits = max(S - 1, 0).bit_length()
    passes = max(1, -(-bits // 8))
    return passes * (4 + 12 + 12), passes


def measure(a, L):
    import torch
    from bench import make_input
    from gkarray_amd import StreamSet

    on_gpu = not a.device.startswith("cpu")
    dev = torch.device(a.device)
    S = a.streams
    N = S * L

    def sync():
        if on_gpu:
            torch.cuda.synchronize(dev)

    def peak_reset():
        if on_gpu:
            torch.cuda.reset_peak_memory_stats(dev)
            return torch.cuda.memory_allocated(dev)
        return 0

    def peak_over(base):
        return int(torch.cuda.max_memory_allocated(dev) - base) if on_gpu else 0

    x, offs = make_input(S, L, 3, dev)
    vals = x.view(S, L).t().contiguous().view(-1)  # sample t of every stream before sample t + 1
    ids = torch.arange(S, dtype=torch.int32, device=dev).repeat(L)
    sa, sb, sc = (StreamSet(S, a.eps, device=dev) for _ in range(3))

    def timed(ss, fn):
        ss.reset()
        ss.sync()
        sync()
        base = peak_reset()
        t0 = time.perf_counter()
        q = fn()
        sync()
        return time.perf_counter() - t0, q, peak_over(base)

    def side_a():
        return sa.ingest_keyed(ids, vals, quantiles=QS)

    def side_b():
        sk, order = torch.sort(ids, stable=True)
        gv = vals[order]
        del order
        try:
            counts = torch.bincount(sk, minlength=S)
        except (RuntimeError, TypeError):
            counts = torch.bincount(sk.to(torch.int64), minlength=S)
        del sk
        o = torch.zeros(S + 1, dtype=torch.int64, device=dev)
        o[1:] = torch.cumsum(counts, 0)
        return sb.ingest(gv, o, quantiles=QS)

    def side_c():
        return sc.ingest(x, offs, quantiles=QS)

    def side_g():
        return sa.group_by_key(ids, vals)

    free0 = torch.cuda.mem_get_info(dev)[0] if on_gpu else 0
    timed(sa, side_a)  # warm-up: code objects, scratch, workspaces
    a_device_bytes = free0 - torch.cuda.mem_get_info(dev)[0] if on_gpu else 0
    timed(sb, side_b)  # (an out-of-memory error here is the caller's cue to halve --values)
    timed(sc, side_c)
    timed(sa, side_g)
    ta, tb, tc, tg, pa, pb = [], [], [], [], 0, 0
    for _ in range(a.reps):
        t, qa, p = timed(sa, side_a)
        ta.append(t)
        pa = max(pa, p)
        t, qb, p = timed(sb, side_b)
        tb.append(t)
        pb = max(pb, p)
        t, qc, _ = timed(sc, side_c)
        tc.append(t)
        t, grouped, _ = timed(sa, side_g)
        tg.append(t)
    assert torch.equal(qa.view(torch.int64), qb.view(torch.int64)), "A's and B's quantiles differ"
    assert torch.equal(qa.view(torch.int64), qc.view(torch.int64)), "A's and the plain CSR ingest's quantiles differ"
    assert torch.equal(grouped[0].view(torch.int64), x.view(torch.int64)), "group_by_key differs from the CSR batch"
    assert torch.equal(grouped[1], offs)
    ms = lambda ts: round(statistics.median(ts) * 1e3, 2)  # noqa: E731
    bps, passes = group_bytes_per_sample(S)
    g_med = statistics.median(tg)
    return {
        "tool": "keyed_ab", "engine": "MI355X" if on_gpu else "cpu (rehearsal, not a measurement)",
        "streams": S, "values_per_stream": L, "samples": N, "eps": a.eps, "reps": a.reps,
        "arrival_order": "round-robin interleave of the streams",
        "A_ingest_keyed_ms": [round(t * 1e3, 2) for t in ta], "B_sort_gather_ingest_ms": [round(t * 1e3, 2) for t in tb],
        "A_median_ms": ms(ta), "B_median_ms": ms(tb), "C_plain_csr_median_ms": ms(tc),
        "G_group_by_key_median_ms": ms(tg), "radix_passes": passes, "group_bytes_per_sample": bps,
        "group_achieved_TBps": round(bps * N / g_med / 1e12, 3), "hbm_peak_TBps": 8.0,
        "A_peak_torch_bytes": pa, "B_peak_torch_bytes": pb, "A_device_bytes_first_call": int(a_device_bytes),
        "quantiles_bit_equal": True}


def child(a):
    sys.path.insert(0, os.path.join(ROOT, "sketches-py_amd"))
    sys.path.insert(0, ROOT)
    import torch

    on_gpu = not a.device.startswith("cpu")
    if on_gpu and not torch.cuda.is_available():
        raise SystemExit("keyed_ab: no GPU visible")
    L = a.values
    notes = []
    while True:
        try:
            out = measure(a, L)
            break
        except torch.cuda.OutOfMemoryError:
            if L <= 1:
                raise
            notes.append("out of memory at %d values per stream (%d samples): halved" % (L, L * a.streams))
            sys.stderr.write("keyed_ab: %s\n" % notes[-1])
            L //= 2
            import gc
            gc.collect()
            torch.cuda.empty_cache()
    out["notes"] = notes
    print(json.dumps(out), flush=True)


def main():
    a = parse()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        r = subprocess.run(cmd, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        sys.stderr.write("keyed_ab: the GPU step passed its time limit of %d s\n" % a.timeout)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
