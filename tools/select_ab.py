"""Cost of a selected query on one MI355X (run by hand; not a test).

State: --streams streams x --values lognormal values, eps 0.01 (150 values:
every stream holds 49 pending values).  From that state, re-ingested (reset +
ingest) before every timed call:
  A: quantiles_select(ids, qs) of --ids random streams (k_select_check, the
     flush of the listed streams through k_fold, k_select_query).
  B: quantiles(qs) of the whole set (one k_ingest_small launch that flushes and
     answers every stream).
  A2: A again on the state A left (nothing pending in the listed streams: the
     check, no flush, the query) -- the call's fixed cost.
One warm-up of each, then --reps interleaved repetitions, wall time around the
synchronising calls; every time and the medians are printed as one JSON line.
A's rows must be bit-equal to B's rows at ids.

The GPU work runs in a child process under its own time limit (--timeout).
--device cpu with a small --streams rehearses the logic on the host engine;
that is not a measurement.
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
    ap.add_argument("--values", type=int, default=150)
    ap.add_argument("--ids", type=int, default=1000)
    ap.add_argument("--eps", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--timeout", type=int, default=600, help="seconds for the child that does the GPU work")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def child(a):
    sys.path.insert(0, os.path.join(ROOT, "sketches-py_amd"))
    import torch
    from gkarray_amd import StreamSet

    on_gpu = not a.device.startswith("cpu")
    if on_gpu and not torch.cuda.is_available():
        raise SystemExit("select_ab: no GPU visible")
    dev = torch.device(a.device)
    S, L, K = a.streams, a.values, a.ids

    def sync():
        if on_gpu:
            torch.cuda.synchronize(dev)

    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    x = torch.exp(torch.randn(S * L, dtype=torch.float64, device=dev, generator=gen))
    offs = torch.arange(S + 1, dtype=torch.int64, device=dev) * L
    ids = torch.randint(0, S, (K,), dtype=torch.int32, device=dev, generator=gen)
    ss = StreamSet(S, a.eps, device=dev)

    def restore():
        ss.reset()
        ss.ingest(x, offs)
        sync()

    def timed(call):
        sync()
        t0 = time.perf_counter()
        out = call()
        sync()
        return time.perf_counter() - t0, out

    def run_a():
        restore()
        ta, qa = timed(lambda: ss.quantiles_select(ids, QS))
        ta2, qa2 = timed(lambda: ss.quantiles_select(ids, QS))
        assert torch.equal(qa.view(torch.int64), qa2.view(torch.int64)), "A and A2 differ"
        return ta, ta2, qa

    def run_b():
        restore()
        return timed(lambda: ss.quantiles(QS))

    run_a()  # warm-up: code objects, the selection scratch, the query list
    run_b()
    ta, ta2, tb = [], [], []
    for _ in range(a.reps):
        t, t2, qa = run_a()
        ta.append(t)
        ta2.append(t2)
        t, qb = run_b()
        tb.append(t)
        assert torch.equal(qa.view(torch.int64), qb[ids.long()].view(torch.int64)), "A's rows differ from B's"
    pend = int(ss.stats()["pending"].sum().item())  # (after B: everything flushed)
    ms = lambda v: [round(t * 1e3, 3) for t in v]  # noqa: E731
    med = lambda v: round(statistics.median(v) * 1e3, 3)  # noqa: E731
    print(json.dumps({
        "tool": "select_ab", "engine": "MI355X" if on_gpu else "cpu (rehearsal, not a measurement)",
        "streams": S, "values_per_stream": L, "ids": K, "nq": len(QS), "eps": a.eps, "reps": a.reps,
        "A_quantiles_select_ms": ms(ta), "A2_quantiles_select_nothing_pending_ms": ms(ta2),
        "B_quantiles_whole_set_ms": ms(tb), "A_median_ms": med(ta), "A2_median_ms": med(ta2), "B_median_ms": med(tb),
        "pending_after_B": pend, "rows_bit_equal": True}), flush=True)


def main():
    a = parse()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        r = subprocess.run(cmd, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        sys.stderr.write("select_ab: the GPU step passed its time limit of %d s\n" % a.timeout)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
