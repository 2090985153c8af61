"""Time of the key-directory calls on one MI355X (run by hand; not a test).

Samples: --samples keys drawn over --keys distinct 64-bit keys (a fixed mixer
of the key's rank, as a series hash would be), uniform and Zipf(--zipf) over
the ranks, built once from seeded device-side draws.  Calls timed, each on
tensors made before the clock starts and ending in a synchronise:
  assign_new    KeyDirectory.assign into an EMPTY directory (every key new;
                the directory is created outside the clock)
  assign_known  the same batch again (every key known)
  lookup        KeyDirectory.lookup of the batch
and two yardsticks on the same samples:
  group_by_key  StreamSet.group_by_key of the samples' ids with S = --keys
                streams: the stage that follows in a keyed step, so the ratio
                is the share the directory adds to it
  torch_unique  torch.unique(keys, return_inverse=True): what a user can write
                today on the device (no persistence, ids in key order instead
                of arrival order)
One warm-up of every call, then --reps (>= 20) rounds that run the five calls
one after the other, a host clock around each.  Reported per call and
distribution: every time, median / min / max, samples per second at each, and
the ratios of the medians.  One JSON line.  The ids of the three directory
calls must agree, and the number of new keys must equal torch.unique's count.

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
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--timeout", type=int, default=540, help="seconds for the child that does the GPU work")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def child(a):
    sys.path.insert(0, os.path.join(ROOT, "sketches-py_amd"))
    import torch
    from gkarray_amd import KeyDirectory, StreamSet

    on_gpu = not a.device.startswith("cpu")
    if on_gpu and not torch.cuda.is_available():
        raise SystemExit("dir_time: no GPU visible")
    if a.reps < 20 and on_gpu:
        raise SystemExit("dir_time: at least 20 repetitions")
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

    def keys_of(ranks):
        # rank -> 64-bit key: an odd multiplier and an offset modulo 2^64 (one to one)
        return ranks * -7046029254386353131 + 2135587861

    def draw(dist):
        if dist == "uniform":
            r = torch.randint(0, K, (N,), dtype=torch.int64, device=dev, generator=gen)
        else:
            w = torch.arange(1, K + 1, dtype=torch.float64, device=dev).pow_(-a.zipf)
            cdf = torch.cumsum(w, 0)
            u = torch.rand(N, dtype=torch.float64, device=dev, generator=gen) * cdf[-1]
            r = torch.searchsorted(cdf, u).clamp_(max=K - 1)
            del w, cdf, u
        return keys_of(r)

    ss = StreamSet(K, a.eps, device=dev)
    values = torch.rand(N, dtype=torch.float64, device=dev, generator=gen)
    out = {"tool": "dir_time", "engine": "MI355X" if on_gpu else "cpu (rehearsal, not a measurement)",
           "samples": N, "keys": K, "zipf": a.zipf, "reps": a.reps, "dists": {}}
    for dist in ("uniform", "zipf"):
        keys = draw(dist)
        state = {}

        def assign_new():
            state["dir"] = None  # (the previous round's directory is freed outside the clock)
            d = KeyDirectory(K, device=dev)
            t = timed(lambda: state.__setitem__("ids_new", d.assign(keys)))
            state["dir"] = d
            state["new"] = d.last_new
            return t

        def assign_known():
            return timed(lambda: state.__setitem__("ids_known", state["dir"].assign(keys)))

        def lookup():
            return timed(lambda: state.__setitem__("ids_lookup", state["dir"].lookup(keys)))

        def group_by_key():
            return timed(lambda: ss.group_by_key(state["ids_new"], values))

        def torch_unique():
            return timed(lambda: state.__setitem__("uniq", torch.unique(keys, return_inverse=True)))

        calls = [("assign_new", assign_new), ("assign_known", assign_known), ("lookup", lookup),
                 ("group_by_key", group_by_key), ("torch_unique", torch_unique)]
        for _, run in calls:  # warm-up: code objects, scratch, allocator
            run()
        assert torch.equal(state["ids_new"], state["ids_known"]), "assign of known keys gives other ids"
        assert torch.equal(state["ids_new"], state["ids_lookup"]), "lookup gives other ids"
        assert state["dir"].last_new == 0 and state["new"] == len(state["dir"]) == state["uniq"][0].numel(), \
            "the directory and torch.unique count different keys"
        # the same grouping: equal ids <=> equal keys
        assert torch.equal(state["dir"].keys()[state["ids_new"].long()], keys), "keys()[ids] is not the batch"
        distinct = state["new"]
        state.pop("uniq")
        times = {name: [] for name, _ in calls}
        for _ in range(a.reps):
            for name, run in calls:
                times[name].append(run())
            state.pop("uniq", None)
        res = {"distinct_keys": distinct, "calls": {}}
        for name, _ in calls:
            t = times[name]
            med = statistics.median(t)
            res["calls"][name] = {"ms": [round(x * 1e3, 3) for x in t], "median_ms": round(med * 1e3, 3),
                                  "min_ms": round(min(t) * 1e3, 3), "max_ms": round(max(t) * 1e3, 3),
                                  "samples_per_s_median": round(N / med, 1),
                                  "samples_per_s_min": round(N / max(t), 1),
                                  "samples_per_s_max": round(N / min(t), 1)}
        med = {name: res["calls"][name]["median_ms"] for name, _ in calls}
        res["ratios_of_medians"] = {
            "%s_over_%s" % (x, y): round(med[x] / med[y], 4)
            for x in ("assign_new", "assign_known", "lookup") for y in ("group_by_key", "torch_unique")}
        out["dists"][dist] = res
        state.clear()
        del keys
    print(json.dumps(out), flush=True)


def main():
    a = parse()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        r = subprocess.run(cmd, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        sys.stderr.write("dir_time: the GPU step passed its time limit of %d s\n" % a.timeout)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
