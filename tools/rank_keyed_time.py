"""Time of StreamSet.ranks_keyed on one MI355X (run by hand; not a test).

The batch of tools/dir_time.py: --samples (id, x) rows over --keys streams,
ids uniform and Zipf(--zipf) over the streams, eps = --eps, built once from
seeded device-side draws.  The set is pre-filled with one keyed ingest of the
batch.  Calls timed, each on tensors made before the clock starts and ending
in a synchronise (a host clock around the synchronising call):
  ranks_keyed        right after a keyed ingest of the batch: the state of a
                     score-then-add loop, so the call first flushes every
                     occurring stream that holds pending values
  ranks_keyed_again  the same call once more: nothing is pending, the time is
                     the check, the group-by and k_rank_keyed
and four yardsticks on the same samples, same run, code this tool does not
touch:
  group_by_key       StreamSet.group_by_key of the same ids (with values)
  ingest_keyed       StreamSet.ingest_keyed of the same batch
  ranks_one          StreamSet.ranks([x]) of the whole set, one threshold
  flush_select       after one more (untimed) keyed ingest of the batch,
                     StreamSet.flush_select of the occurring streams: the
                     flush that ranks_keyed shares with every selection call
One warm-up of every call, then --reps (>= 20) rounds that run the six calls
one after the other.  Reported per call and distribution: every time, median /
min / max, samples per second at the median, and the ratios of the medians.
Then, nothing pending, ranks_keyed_again at each GK_RANKK_CHUNK of --chunks
(the A/B behind the default), and on a two-stream set --long-samples rows on
ONE stream whose table fits the kernel's LDS tile against the same number on
one whose table (2079 entries at eps = 0.001) is streamed tile after tile.
One JSON line, also written to --out.

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
    ap.add_argument("--samples", type=int, default=100_000_000)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--eps", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunks", default="256,512,1024,2048,4096")
    ap.add_argument("--long-samples", type=int, default=10_000_000)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_keyed_time.json"))
    ap.add_argument("--timeout", type=int, default=540, help="seconds for the child that does the GPU work")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def summary(t, N):
    med = statistics.median(t)
    return {"ms": [round(x * 1e3, 3) for x in t], "median_ms": round(med * 1e3, 3), "min_ms": round(min(t) * 1e3, 3),
            "max_ms": round(max(t) * 1e3, 3), "samples_per_s_median": round(N / med, 1)}


def child(a):
    sys.path.insert(0, os.path.join(ROOT, "sketches-py_amd"))
    import torch
    from gkarray_amd import StreamSet

    on_gpu = not a.device.startswith("cpu")
    if on_gpu and not torch.cuda.is_available():
        raise SystemExit("rank_keyed_time: no GPU visible")
    if a.reps < 20 and on_gpu:
        raise SystemExit("rank_keyed_time: at least 20 repetitions")
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
    gen.manual_seed(17)

    def draw(dist):
        if dist == "uniform":
            return torch.randint(0, K, (N,), dtype=torch.int32, device=dev, generator=gen)
        w = torch.arange(1, K + 1, dtype=torch.float64, device=dev).pow_(-a.zipf)
        cdf = torch.cumsum(w, 0)
        u = torch.rand(N, dtype=torch.float64, device=dev, generator=gen) * cdf[-1]
        return torch.searchsorted(cdf, u).clamp_(max=K - 1).to(torch.int32)

    values = torch.rand(N, dtype=torch.float64, device=dev, generator=gen)
    xs = torch.rand(N, dtype=torch.float64, device=dev, generator=gen)
    lo = torch.empty(N, dtype=torch.int64, device=dev)
    hi = torch.empty(N, dtype=torch.int64, device=dev)
    out = {"tool": "rank_keyed_time", "engine": "MI355X" if on_gpu else "cpu (rehearsal, not a measurement)",
           "samples": N, "keys": K, "zipf": a.zipf, "eps": a.eps, "reps": a.reps, "dists": {}}
    os.environ.pop("GK_RANKK_CHUNK", None)
    for dist in ("uniform", "zipf"):
        ids = draw(dist)
        ss = StreamSet(K, a.eps, device=dev)
        ss.ingest_keyed(ids, values)  # the pre-fill
        calls = [("ingest_keyed", lambda: ss.ingest_keyed(ids, values)),
                 ("ranks_keyed", lambda: ss.ranks_keyed(ids, xs, lo=lo, hi=hi)),
                 ("ranks_keyed_again", lambda: ss.ranks_keyed(ids, xs, lo=lo, hi=hi)),
                 ("group_by_key", lambda: ss.group_by_key(ids, values)),
                 ("ranks_one", lambda: ss.ranks([0.5])),
                 ("flush_select", lambda: ss.flush_select(uniq))]
        uniq = torch.unique(ids)
        for _, run in calls:  # warm-up: code objects, scratch, allocator
            timed(run)
        # the answers: equal to ranks_select of a few streams, gathered
        probe = torch.unique(ids[:1000])[:8]
        rows = torch.isin(ids, probe).nonzero().flatten()[:2000]
        plo, phi, _ = ss.ranks_keyed(ids[rows], xs[rows])
        assert torch.equal(plo, lo[rows]) and torch.equal(phi, hi[rows]), "a sub-batch answers differently"
        times = {name: [] for name, _ in calls}
        for _ in range(a.reps):
            for name, run in calls:
                if name == "flush_select":
                    ss.ingest_keyed(ids, values)
                times[name].append(timed(run))
        res = {"occurring_streams": int(uniq.numel()),
               "calls": {name: summary(times[name], N) for name, _ in calls}}
        med = {name: res["calls"][name]["median_ms"] for name, _ in calls}
        res["ratios_of_medians"] = {
            "%s_over_%s" % (x, y): round(med[x] / med[y], 4)
            for x in ("ranks_keyed", "ranks_keyed_again") for y in ("group_by_key", "ingest_keyed", "ranks_one", "flush_select")}
        # the default chunk's A/B: nothing pending, the same call at each chunk
        ab = {}
        for c in [int(c) for c in a.chunks.split(",") if c]:
            os.environ["GK_RANKK_CHUNK"] = str(c)
            timed(calls[2][1])
            ab[str(c)] = summary([timed(calls[2][1]) for _ in range(a.reps)], N)
            del ab[str(c)]["ms"]
        os.environ.pop("GK_RANKK_CHUNK", None)
        res["chunk_ab_ranks_keyed_again"] = ab
        out["dists"][dist] = res
        ss.close()
        del ids, ss
    # one stream, table within the tile against table beyond it
    M = min(a.long_samples, N)
    desc = torch.arange(4000, 0, -1, dtype=torch.float64, device=dev)
    ss = StreamSet(2, 0.001, device=dev)
    ss.ingest_keyed(torch.cat([torch.zeros(200, dtype=torch.int32, device=dev),
                               torch.ones(4000, dtype=torch.int32, device=dev)]), torch.cat([desc[:200], desc]))
    ss.flush()
    sizes = ss.stats()["size"].cpu().tolist()
    lx = torch.rand(M, dtype=torch.float64, device=dev, generator=gen) * 4000.0
    long_res = {"samples": M, "table_entries": {"tile": sizes[0], "beyond": sizes[1]}}
    for name, s in (("tile", 0), ("beyond", 1)):
        sid = torch.full((M,), s, dtype=torch.int32, device=dev)
        run = lambda: ss.ranks_keyed(sid, lx, lo=lo[:M], hi=hi[:M])  # noqa: E731
        timed(run)
        long_res[name] = summary([timed(run) for _ in range(a.reps)], M)
        del long_res[name]["ms"]
    long_res["beyond_over_tile"] = round(long_res["beyond"]["median_ms"] / long_res["tile"]["median_ms"], 4)
    out["one_stream"] = long_res
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
        sys.stderr.write("rank_keyed_time: the GPU step passed its time limit of %d s\n" % a.timeout)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
