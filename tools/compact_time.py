"""What churn costs a step, and what compact() costs, on one MI355X (run by
hand; not a test).

For each fraction f of --fractions a CHURNED set is made the way a long-running
KeyedStreamSet makes one: f * S streams, evenly spread, are promoted into class
1 by a descending run of 190 values (138 entries after the flush, more than the
127 class 0 holds) and then reset (reset_select): empty streams that keep class
and slot -- the parent commit's behaviour for every later call.  Timed:
  step      a cfg3-shaped, reset-free step, ingest(x, offs, quantiles=[.5, .9,
            .99]) of --values Pareto(1.5) values per stream, on three sets fed
            the same batch: (a) "churned", (b) "compacted" = a second churned
            set after compact(), (c) "fresh" = a new set.  The three hold the
            same streams bit for bit (the reset streams are empty); only the
            placement differs.  Their answers must be equal.
  compact   compact() on a churned set whose other streams hold one step's
            values, against resized(S) on the same set -- the only way the
            parent commit has to re-place streams.  The set is churned again
            before every round.
One warm-up round, then --reps rounds that run the sides one after the other
(interleaved), a host clock around calls that end in a synchronise.  Reported
per side: every time, median / min / max.  One JSON line.

The GPU work runs in a child process under its own time limit (--timeout).
--device cpu with a small --streams rehearses the logic on the host engine;
that is not a measurement (the host engine has no classes).
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
    ap.add_argument("--values", type=int, default=1000)
    ap.add_argument("--fractions", default="0.01,0.1")
    ap.add_argument("--eps", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", default="cuda:0")
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
        raise SystemExit("compact_time: no GPU visible")
    if a.reps < 7 and on_gpu:
        raise SystemExit("compact_time: at least 7 repetitions")
    dev = torch.device(a.device)
    S, L = a.streams, a.values

    def sync():
        if on_gpu:
            torch.cuda.synchronize(dev)

    def timed(call):
        sync()
        t0 = time.perf_counter()
        r = call()
        sync()
        return time.perf_counter() - t0, r

    gen = torch.Generator(device=dev)
    gen.manual_seed(17)
    x = torch.empty(S * L, dtype=torch.float64, device=dev)
    piece = max(1, (1 << 26) // max(L, 1)) * L
    for at in range(0, S * L, piece):  # Pareto(1.5) + 1, as numpy's pareto(1.5) + 1
        u = torch.rand(min(piece, S * L - at), dtype=torch.float64, device=dev, generator=gen)
        x[at:at + u.numel()] = (1.0 - u).pow_(-1.0 / 1.5)
        del u
    offs = torch.arange(S + 1, dtype=torch.int64, device=dev) * L
    run190 = torch.arange(3999, 3999 - 190, -1, dtype=torch.float64, device=dev)  # select_cases.D(190)

    def churn(ss, ids):
        """ids (empty streams of class 0) into class 1 and back to empty: churned."""
        k = ids.numel()
        cnt = torch.zeros(S, dtype=torch.int64, device=dev)
        cnt[ids.long()] = 190
        o = torch.zeros(S + 1, dtype=torch.int64, device=dev)
        o[1:] = torch.cumsum(cnt, 0)
        ss.ingest(run190.repeat(k), o)
        ss.flush_select(ids)
        promoted = ss.num_promoted
        ss.reset_select(ids)
        return promoted

    def slots(ss):
        return [(u["streams"], u["slots_used"], u["slots_alloc"]) for u in ss.class_usage()]

    out = {"tool": "compact_time", "engine": "MI355X" if on_gpu else "cpu (rehearsal, not a measurement)",
           "streams": S, "values_per_step": L, "eps": a.eps, "reps": a.reps, "quantiles": QS, "fractions": {}}
    for f in [float(v) for v in a.fractions.split(",")]:
        k = max(1, int(round(f * S)))
        ids = torch.arange(k, dtype=torch.int64, device=dev).mul_(S).div_(k, rounding_mode="floor").to(torch.int32)
        res = {"churned_streams": k}
        sets = {"churned": StreamSet(S, a.eps, device=dev), "compacted": StreamSet(S, a.eps, device=dev),
                "fresh": StreamSet(S, a.eps, device=dev)}
        res["promoted_by_churn"] = churn(sets["churned"], ids)
        churn(sets["compacted"], ids)
        res["classes_churned"] = slots(sets["churned"])
        res["compact"] = sets["compacted"].compact()
        res["classes_compacted"] = slots(sets["compacted"])
        if on_gpu:
            assert res["promoted_by_churn"] == k and res["compact"]["demoted"] == k, res
        times = {name: [] for name in sets}
        answers = {}
        for rep in range(a.reps + 1):  # (round 0: warm-up)
            for name, ss in sets.items():
                t, q = timed(lambda: ss.ingest(x, offs, quantiles=QS))
                if rep:
                    times[name].append(t)
                answers[name] = q
        assert torch.equal(answers["churned"], answers["fresh"]), "the churned set answers differently"
        assert torch.equal(answers["compacted"], answers["fresh"]), "the compacted set answers differently"
        res["step"] = {name: summary(t) for name, t in times.items()}
        res["promoted_after_steps"] = {name: ss.num_promoted for name, ss in sets.items()}
        # compact() against resized(S) on the churned set (its other streams hold the steps' values)
        z = sets["churned"]
        sets["compacted"].close()
        sets["fresh"].close()
        del sets, answers
        tc, tr = [], []
        for rep in range(a.reps + 1):
            z.compact()  # (the ids go home, empty, whatever the round before left)
            z.reset_select(ids)
            churn(z, ids)
            t, other = timed(lambda: z.resized(S))
            other.close()
            del other
            if rep:
                tr.append(t)
            t, r = timed(z.compact)
            if rep:
                tc.append(t)
                if on_gpu:
                    assert r["demoted"] == k, r
        res["compact_call"] = summary(tc)
        res["resized_call"] = summary(tr)
        z.close()
        del z
        out["fractions"]["%g" % f] = res
    print(json.dumps(out), flush=True)


def main():
    a = parse()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [v for v in sys.argv[1:] if v != "--child"]
    try:
        r = subprocess.run(cmd, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        sys.stderr.write("compact_time: the GPU step passed its time limit of %d s\n" % a.timeout)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
