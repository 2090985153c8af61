"""Time of StreamSet.rank_ingest_keyed against ranks_keyed + ingest_keyed on one
MI355X (run by hand; not a test).

--samples (id, value) rows per batch over --keys streams, ids uniform and
Zipf(--zipf) over the streams, eps = --eps, built once from seeded device-side
draws.  Two sets are pre-filled with one keyed ingest of the batch each -- the
history is in place -- and then driven through the same scoring loop, one batch
per round, the same library for both:
  fused      a.rank_ingest_keyed(ids, values, lo, hi)
  two_call   b.ranks_keyed(ids, values, lo, hi); b.ingest_keyed(ids, values)
             (its halves are also timed on their own: ranks / ingest)
Both sets hold the same state at the start of every round, so the two sides
do the same flushes.  Each timed call runs on tensors made before the clock
starts and ends in a synchronise (a host clock around call + synchronise).
One warm-up round, then --reps (>= 3) rounds that alternate the two sides,
fused first in even rounds, two_call first in odd ones.  After the last round
the rank outputs of the two sides are compared.  Reported per distribution:
every time, median / min / max of each side, the spread (the larger max - min
of the two sides), the saving (two_call median - fused median) and whether it
exceeds the spread; beside them one group_by_key of the same batch, the work
the fused call leaves out.  One JSON line, also written to --out.

The GPU work runs in a child process under its own time limit (--timeout).
--device cpu with a small --samples rehearses the logic on the host engine;
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


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=16_000_000)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--eps", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_ingest_time.json"))
    ap.add_argument("--timeout", type=int, default=540, help="seconds for the child that does the GPU work")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def summary(t):
    return {"ms": [round(x * 1e3, 3) for x in t], "median_ms": round(statistics.median(t) * 1e3, 3),
            "min_ms": round(min(t) * 1e3, 3), "max_ms": round(max(t) * 1e3, 3)}


def child(a):
    sys.path.insert(0, os.path.join(ROOT, "sketches-py_amd"))
    import torch
    from gkarray_amd import StreamSet

    on_gpu = not a.device.startswith("cpu")
    if on_gpu and not torch.cuda.is_available():
        raise SystemExit("rank_ingest_time: no GPU visible")
    if a.reps < 3:
        raise SystemExit("rank_ingest_time: at least 3 repetitions per side")
    dev = torch.device(a.device)
    N, K = a.samples, a.keys

    def sync():
        if on_gpu:
            torch.cuda.synchronize(dev)

    def timed(call):
        sync()
        t0 = time.perf_counter()
        call()
        sync()
        return time.perf_counter() - t0

    gen = torch.Generator(device=dev)
    gen.manual_seed(23)

    def draw(dist):
        if dist == "uniform":
            return torch.randint(0, K, (N,), dtype=torch.int32, device=dev, generator=gen)
        w = torch.arange(1, K + 1, dtype=torch.float64, device=dev).pow_(-a.zipf)
        cdf = torch.cumsum(w, 0)
        u = torch.rand(N, dtype=torch.float64, device=dev, generator=gen) * cdf[-1]
        return torch.searchsorted(cdf, u).clamp_(max=K - 1).to(torch.int32)

    values = torch.rand(N, dtype=torch.float64, device=dev, generator=gen)
    lo = [torch.empty(N, dtype=torch.int64, device=dev) for _ in range(2)]
    hi = [torch.empty(N, dtype=torch.int64, device=dev) for _ in range(2)]
    out = {"tool": "rank_ingest_time", "engine": "MI355X" if on_gpu else "cpu (rehearsal, not a measurement)",
           "samples": N, "keys": K, "zipf": a.zipf, "eps": a.eps, "reps": a.reps, "dists": {}}
    os.environ.pop("GK_RANKK_CHUNK", None)
    for dist in ("uniform", "zipf"):
        ids = draw(dist)
        sa, sb = StreamSet(K, a.eps, device=dev), StreamSet(K, a.eps, device=dev)
        for s in (sa, sb):
            s.ingest_keyed(ids, values)  # the history

        def fused():
            return {"fused": timed(lambda: sa.rank_ingest_keyed(ids, values, lo=lo[0], hi=hi[0]))}

        def two_call():
            r = timed(lambda: sb.ranks_keyed(ids, values, lo=lo[1], hi=hi[1]))
            i = timed(lambda: sb.ingest_keyed(ids, values))
            return {"ranks": r, "ingest": i, "two_call": r + i}

        fused(), two_call()  # warm-up: code objects, scratch, allocator
        times = {"fused": [], "two_call": [], "ranks": [], "ingest": []}
        for rep in range(a.reps):
            for side in ((fused, two_call) if rep % 2 == 0 else (two_call, fused)):
                for k, v in side().items():
                    times[k].append(v)
        assert torch.equal(lo[0], lo[1]) and torch.equal(hi[0], hi[1]), "the two sides answer differently"
        na, nb = sa.stats()["n"], sb.stats()["n"]
        assert torch.equal(na, nb) and int(na.sum().item()) == (a.reps + 2) * N, "the two sides hold different counts"
        timed(lambda: sb.group_by_key(ids, values))
        group = [timed(lambda: sb.group_by_key(ids, values)) for _ in range(a.reps)]
        res = {"occurring_streams": int(torch.unique(ids).numel()), "calls": {k: summary(v) for k, v in times.items()}}
        res["calls"]["group_by_key"] = summary(group)
        f, t = res["calls"]["fused"], res["calls"]["two_call"]
        spread = max(f["max_ms"] - f["min_ms"], t["max_ms"] - t["min_ms"])
        saving = t["median_ms"] - f["median_ms"]
        res.update(spread_ms=round(spread, 3), saving_ms=round(saving, 3),
                   fused_over_two_call=round(f["median_ms"] / t["median_ms"], 4),
                   saving_exceeds_spread=bool(saving > spread))
        out["dists"][dist] = res
        sa.close()
        sb.close()
        del ids, sa, sb
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


def main():
    a = parse()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        r = subprocess.run(cmd, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        sys.stderr.write("rank_ingest_time: the GPU step passed its time limit of %d s\n" % a.timeout)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
