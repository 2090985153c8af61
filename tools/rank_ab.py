"""Cost of a rank query against the quantile query on one MI355X (run by hand;
not a test).

State: --streams streams x --values lognormal values, eps 0.01 (150 values:
every stream holds 49 pending values) -- the state of tools/select_ab.py.  From
that state, re-ingested (reset + ingest) before every timed call:
  R:  ranks(xs) of the whole set, 3 thresholds (gk_sync, gk_flush, gk_sync,
      k_rank over every stream).
  Q:  quantiles(qs) of the whole set, 3 quantiles (one k_ingest_small launch
      that flushes and answers every stream).
  RS: ranks_select(ids, xs) of --ids random streams (k_select_check, the flush
      of the listed streams through k_fold, k_rank).
  QS: quantiles_select(ids, qs) of the same streams (the same check and flush,
      k_select_query).
Each pair reads the same tables after the same flush.  One warm-up of each,
then --reps interleaved repetitions (R, Q, RS, QS), wall time around the
synchronising calls; every time, the medians and the ranges are printed as one
JSON line.  RS's rows must be bit-equal to R's rows at ids.

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
XS = [0.5, 1.0, 3.0]  # lognormal(0, 1): about the 24th, 50th and 86th percentile


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
        raise SystemExit("rank_ab: no GPU visible")
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

    def timed(call):
        ss.reset()
        ss.ingest(x, offs)
        sync()
        t0 = time.perf_counter()
        out = call()
        sync()
        return time.perf_counter() - t0, out

    calls = {
        "R": lambda: ss.ranks(XS),
        "Q": lambda: ss.quantiles(QS),
        "RS": lambda: ss.ranks_select(ids, XS),
        "QS": lambda: ss.quantiles_select(ids, QS),
    }
    for c in calls.values():  # warm-up: code objects, the selection scratch, the query list
        timed(c)
    t = {k: [] for k in calls}
    for _ in range(a.reps):
        out = {}
        for k, c in calls.items():
            dt, out[k] = timed(c)
            t[k].append(dt)
        for j in (0, 1):
            assert torch.equal(out["RS"][j], out["R"][j][ids.long()]), "RS's rows differ from R's"
        assert torch.equal(out["QS"].view(torch.int64), out["Q"][ids.long()].view(torch.int64)), "QS vs Q"
    ms = lambda v: [round(u * 1e3, 3) for u in v]  # noqa: E731
    res = {"tool": "rank_ab", "engine": "MI355X" if on_gpu else "cpu (rehearsal, not a measurement)",
           "streams": S, "values_per_stream": L, "ids": K, "nx": len(XS), "nq": len(QS), "eps": a.eps, "reps": a.reps,
           "rows_bit_equal": True}
    names = {"R": "ranks_whole_set", "Q": "quantiles_whole_set", "RS": "ranks_select", "QS": "quantiles_select"}
    for k, v in t.items():
        res["%s_%s_ms" % (k, names[k])] = ms(v)
        res["%s_median_ms" % k] = round(statistics.median(v) * 1e3, 3)
        res["%s_range_ms" % k] = [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)]
    res["R_over_Q"] = round(statistics.median(t["R"]) / statistics.median(t["Q"]), 3)
    res["RS_over_QS"] = round(statistics.median(t["RS"]) / statistics.median(t["QS"]), 3)
    print(json.dumps(res), flush=True)


def main():
    a = parse()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        r = subprocess.run(cmd, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        sys.stderr.write("rank_ab: the GPU step passed its time limit of %d s\n" % a.timeout)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
