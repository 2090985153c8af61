"""A/B of the group-by roll-up on one MI355X (run by hand; not a test).

Source: the cfg3 data (10^6 streams x 1000 Pareto values, eps 0.01), rolled up
with keys = s % 10^4 into 10^4 destination streams.
  A: dst.rollup_by_key(src, keys) into a fresh set (k_fold with groups: one launch per
     capacity level, the destination table on chip across its 100 members).
  B: the way without gk_rollup: the same tables held as 100 sets of 10^4
     streams (contiguous slices, import_arrays), then dst.merge_from(sets)
     (100 one-step k_fold launches, every destination table through HBM each time).
The source state is restored before every run (merges flush their sources).
One warm-up run of each side, then --reps interleaved repetitions, wall time
around the synchronising calls; medians are printed as one JSON line.  A's and
B's destination quantiles must be bit-equal.

The GPU work runs in a child process under its own time limit (--timeout).
--device cpu with small --streams / --groups rehearses the logic on the host
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
QS = [0.0, 0.5, 0.9, 0.99, 1.0]


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=1_000_000)
    ap.add_argument("--groups", type=int, default=10_000)
    ap.add_argument("--values", type=int, default=1000)
    ap.add_argument("--eps", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--timeout", type=int, default=900, help="seconds for the child that does the GPU work")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def child(a):
    sys.path.insert(0, os.path.join(ROOT, "sketches-py_amd"))
    sys.path.insert(0, ROOT)
    import torch
    from bench import make_input
    from gkarray_amd import StreamSet

    on_gpu = not a.device.startswith("cpu")
    if on_gpu and not torch.cuda.is_available():
        raise SystemExit("rollup_ab: no GPU visible")
    dev = torch.device(a.device)
    S, G, L = a.streams, a.groups, a.values
    if S % G:
        raise SystemExit("rollup_ab: --streams must be a multiple of --groups")
    R = S // G

    def sync():
        if on_gpu:
            torch.cuda.synchronize(dev)

    x, offs = make_input(S, L, 3, dev)
    src = StreamSet(S, a.eps, device=dev)
    src.ingest(x, offs)
    del x
    st = src.export_state()  # restored before every run
    pv = st["pv"] if st["pv"].numel() else torch.zeros(1, dtype=torch.float64, device=dev)
    keys = torch.arange(S, dtype=torch.int64, device=dev) % G
    sets = [StreamSet(G, a.eps, device=dev) for _ in range(R)]
    dst_a, dst_b = StreamSet(G, a.eps, device=dev), StreamSet(G, a.eps, device=dev)

    def run_a():
        src.import_state(st)
        dst_a.reset()
        dst_a.sync()
        sync()
        t0 = time.perf_counter()
        dst_a.rollup_by_key(src, keys)
        sync()
        return time.perf_counter() - t0

    def run_b():
        for r, ss in enumerate(sets):
            lo, hi = r * G, (r + 1) * G
            ss.import_arrays(st["offs"][lo:hi + 1].contiguous(), st["v"], st["g"], st["d"],
                             st["poffs"][lo:hi + 1].contiguous(), pv, st["n"][lo:hi].contiguous(),
                             st["min"][lo:hi].contiguous(), st["max"][lo:hi].contiguous(),
                             st["sum"][lo:hi].contiguous(), st["avg"][lo:hi].contiguous())
        dst_b.reset()
        dst_b.sync()
        sync()
        t0 = time.perf_counter()
        dst_b.merge_from(sets)
        sync()
        return time.perf_counter() - t0

    run_a()  # warm-up: code objects, class arenas, workspaces
    run_b()
    ta, tb = [], []
    for _ in range(a.reps):
        ta.append(run_a())
        tb.append(run_b())
    sa, sb = dst_a.export_state(), dst_b.export_state()
    for k in ("offs", "v", "g", "d", "poffs", "pv", "n", "min", "max", "sum", "avg"):
        u, w = sa[k], sb[k]
        if u.dtype == torch.float64:
            u, w = u.view(torch.int64), w.view(torch.int64)
        assert torch.equal(u, w), "A and B differ in %s" % k
    qa, qb = dst_a.quantiles(QS), dst_b.quantiles(QS)
    assert torch.equal(qa.view(torch.int64), qb.view(torch.int64)), "A's and B's quantiles differ"
    promoted = dst_a.num_promoted
    print(json.dumps({
        "tool": "rollup_ab", "engine": "MI355X" if on_gpu else "cpu (rehearsal, not a measurement)",
        "streams": S, "groups": G, "values_per_stream": L, "eps": a.eps, "reps": a.reps,
        "A_rollup_by_key_ms": [round(t * 1e3, 2) for t in ta], "B_merge_from_ms": [round(t * 1e3, 2) for t in tb],
        "A_median_ms": round(statistics.median(ta) * 1e3, 2), "B_median_ms": round(statistics.median(tb) * 1e3, 2),
        "dst_streams_promoted": int(promoted), "state_and_quantiles_bit_equal": True}), flush=True)


def main():
    a = parse()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        r = subprocess.run(cmd, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        sys.stderr.write("rollup_ab: the GPU step passed its time limit of %d s\n" % a.timeout)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
