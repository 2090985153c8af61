"""Time of key removal and id recycling in the key directory on one MI355X
(run by hand; not a test).

A directory of capacity --keys holds --keys distinct 64-bit keys (a fixed mixer
of the key's rank, as tools/dir_time.py).  Per distribution (uniform and
Zipf(--zipf) over the ranks; seeded device-side draws) three comparisons, every
call on tensors made before the clock starts and ending in a synchronise:

  remove / rebuild_today
      remove          KeyDirectory.remove of a batch that holds --removed
                      distinct held keys (uniform: each once; Zipf: the draws
                      that hit them, hot keys many times)
      rebuild_today   what dropping the same keys costs without remove, on the
                      same library: lookup(victims) -> boolean filter of
                      keys() -> import_keys(survivors).  Every survivor gets a
                      new id.
  tombstones
      A directory from which T/4 keys were removed in one call -- the most
      removed keys the rebuild rule leaves in the table -- against a directory
      of the same contents right after a rebuild (a sparse import), on a batch
      of --samples samples over the keys both still hold:
      lookup_dead / lookup_clean, assign_known_dead / assign_known_clean.
  assign_new
      recycled        --removed new keys (10 samples each on average) into a
                      full id space with --removed free ids: every id comes
                      from the free list
      fresh           the same batch into a dense directory of --keys minus
                      --removed keys: every id is bound, bound + 1, ...

One warm-up of every call, then --reps (>= 20) rounds; the state a call
consumes is put back outside the clock.  Reported per call and distribution:
every time, median / min / max, and the ratios of the medians.  One JSON line.

The GPU work runs in a child process under its own time limit (--timeout).
--device cpu with small sizes rehearses the logic on the host engine; that is
not a measurement.
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
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--removed", type=int, default=100_000)
    ap.add_argument("--samples", type=int, default=10_000_000)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--timeout", type=int, default=540, help="seconds for the child that does the GPU work")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def child(a):
    sys.path.insert(0, os.path.join(ROOT, "sketches-py_amd"))
    import torch
    from gkarray_amd import KeyDirectory

    on_gpu = not a.device.startswith("cpu")
    if on_gpu and not torch.cuda.is_available():
        raise SystemExit("dir_churn_time: no GPU visible")
    if a.reps < 20 and on_gpu:
        raise SystemExit("dir_churn_time: at least 20 repetitions")
    dev = torch.device(a.device)
    K, R, N = a.keys, a.removed, a.samples
    T = 64
    while T < 2 * K:
        T *= 2
    dead = min(T // 4, K - 1)  # the rebuild rule: more than T/4 removed keys in place trigger a rebuild

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

    def keys_of(ranks):
        # rank -> 64-bit key: an odd multiplier and an offset modulo 2^64 (one to one)
        return ranks * -7046029254386353131 + 2135587861

    def draw(dist, n, k):
        """n ranks below k."""
        if dist == "uniform":
            return torch.randint(0, k, (n,), dtype=torch.int64, device=dev, generator=gen)
        w = torch.arange(1, k + 1, dtype=torch.float64, device=dev).pow_(-a.zipf)
        cdf = torch.cumsum(w, 0)
        u = torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * cdf[-1]
        return torch.searchsorted(cdf, u).clamp_(max=k - 1)

    def perm(n):
        return torch.randperm(n, device=dev, generator=gen)

    held = keys_of(torch.arange(K, dtype=torch.int64, device=dev))
    strangers = keys_of(torch.arange(K, K + R, dtype=torch.int64, device=dev))

    def full():
        d = KeyDirectory(K, device=dev)
        d.import_keys(held)
        return d

    out = {"tool": "dir_churn_time", "engine": "MI355X" if on_gpu else "cpu (rehearsal, not a measurement)",
           "keys": K, "removed": R, "samples": N, "zipf": a.zipf, "reps": a.reps, "slots": T, "dists": {}}
    for dist in ("uniform", "zipf"):
        res = {"calls": {}}
        # ---- 1. remove against today's rebuild
        if dist == "uniform":
            victims = held[perm(K)[:R]]
            batch = victims
        else:
            s = draw(dist, max(N // 5, 20 * R), K)
            u = torch.unique(s)
            pick = u[perm(u.numel())[:R]]
            batch = keys_of(s[torch.isin(s, pick)])
            victims = keys_of(pick)
            del s, u, pick
        res["remove_batch"] = {"samples": batch.numel(), "distinct": victims.numel()}
        state = {"a": full(), "b": full()}

        def remove():
            d = state["a"]
            t = timed(lambda: d.remove(batch))
            assert d.last_removed == victims.numel() and len(d) == K - victims.numel()
            d.import_keys(held)
            return t

        def rebuild_today():
            d = state["b"]

            def run():
                ids = d.lookup(victims)
                keep = torch.ones(K, dtype=torch.bool, device=dev)
                keep[ids.long()] = False
                d.import_keys(d.keys()[keep])
            t = timed(run)
            assert len(d) == K - victims.numel()
            d.import_keys(held)
            return t

        # ---- 2. the most tombstones the rebuild rule allows, against a rebuilt table
        dd = full()
        gone = held[perm(K)[:dead]]
        dd.remove(gone)
        assert dd.last_removed == dead
        clean = KeyDirectory(K, device=dev)
        clean.import_keys(dd.keys(), sparse=True)
        live = dd.keys()
        live = live[live != -2 ** 63]
        probe = live[draw(dist, N, live.numel())]
        assert torch.equal(dd.lookup(probe), clean.lookup(probe))
        res["tombstones"] = {"removed_in_place": dead, "live": live.numel(), "samples": N}

        def on(d, op):
            def run():
                t = timed(lambda: getattr(d, op)(probe))
                assert op == "lookup" or d.last_new == 0
                return t
            return run

        # ---- 3. new keys from the free list against new keys into fresh ids
        fresh_keys = strangers[draw(dist, 10 * R, R)]
        base = held[: K - R]
        state["rec"] = full()
        state["rec"].remove(held[K - R:])
        state["fresh"] = KeyDirectory(K, device=dev)
        state["fresh"].import_keys(base)

        def recycled():
            d = state["rec"]
            ids = []
            t = timed(lambda: ids.append(d.assign(fresh_keys)))
            assert d.bound == K and int(ids[0].min()) >= K - R
            d.remove(strangers)
            assert d.bound == K and len(d) == K - R
            return t

        def fresh():
            d = state["fresh"]
            ids = []
            t = timed(lambda: ids.append(d.assign(fresh_keys)))
            assert int(ids[0].min()) >= K - R and d.bound == len(d)
            state["new"] = d.last_new
            d.import_keys(base)
            return t

        calls = [("remove", remove), ("rebuild_today", rebuild_today),
                 ("lookup_dead", on(dd, "lookup")), ("lookup_clean", on(clean, "lookup")),
                 ("assign_known_dead", on(dd, "assign")), ("assign_known_clean", on(clean, "assign")),
                 ("assign_new_recycled", recycled), ("assign_new_fresh", fresh)]
        for _, run in calls:  # warm-up: code objects, scratch, allocator
            run()
        res["assign_new_batch"] = {"samples": fresh_keys.numel(), "distinct": state["new"]}
        times = {name: [] for name, _ in calls}
        for _ in range(a.reps):
            for name, run in calls:
                times[name].append(run())
        for name, _ in calls:
            t = times[name]
            res["calls"][name] = {"ms": [round(x * 1e3, 3) for x in t],
                                  "median_ms": round(statistics.median(t) * 1e3, 3),
                                  "min_ms": round(min(t) * 1e3, 3), "max_ms": round(max(t) * 1e3, 3)}
        med = {name: res["calls"][name]["median_ms"] for name, _ in calls}
        res["ratios_of_medians"] = {
            "%s_over_%s" % (x, y): round(med[x] / med[y], 4)
            for x, y in (("remove", "rebuild_today"), ("lookup_dead", "lookup_clean"),
                         ("assign_known_dead", "assign_known_clean"), ("assign_new_recycled", "assign_new_fresh"))}
        out["dists"][dist] = res
        for d in list(state.values()) + [dd, clean]:
            if isinstance(d, KeyDirectory):
                d.close()
        state.clear()
    print(json.dumps(out), flush=True)


def main():
    a = parse()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        r = subprocess.run(cmd, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        sys.stderr.write("dir_churn_time: the GPU step passed its time limit of %d s\n" % a.timeout)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
