"""Time of the stream-transfer calls on one MI355X (run by hand; not a test).

State: --streams streams x --values Pareto(1.5) values, eps 0.01, flushed (the
state of bench.py's cfg3), built once from seeded device-side draws, ingested
in chunks.  Calls timed, each into buffers / sets made before the clock starts:
  pack             StreamSet.pack(buf)                      (the yardstick: the
                   parent commit's code; its spread is reported)
  pack_select_all  pack_select(arange(S), buf)
  pack_select_10   pack_select of a random 10 % of the ids
  unpack_fresh     unpack_select(arange(S), full buffer) into a reset set
  unpack_same      unpack_select(arange(S), full buffer) into the packing set
One warm-up of every call, then --reps (>= 20) rounds that run the five calls
one after the other, a host clock around calls that end in a synchronise.
Reported per call: every time, median / min / max, and "packed bytes over call
time" (GB/s of the packed buffer's size; NOT a share of any peak).  One JSON
line.  pack_select_all's buffer must equal pack's byte for byte, and the
unpacked sets must pack to the same bytes.

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


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=1_000_000)
    ap.add_argument("--values", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=100, help="values per stream and ingest call while building the state")
    ap.add_argument("--eps", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--timeout", type=int, default=540, help="seconds for the child that does the GPU work")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def child(a):
    sys.path.insert(0, os.path.join(ROOT, "sketches-py_amd"))
    import torch
    from gkarray_amd import StreamSet

    on_gpu = not a.device.startswith("cpu")
    if on_gpu and not torch.cuda.is_available():
        raise SystemExit("transfer_time: no GPU visible")
    if a.reps < 20 and on_gpu:
        raise SystemExit("transfer_time: at least 20 repetitions")
    dev = torch.device(a.device)
    S, L = a.streams, a.values

    def sync():
        if on_gpu:
            torch.cuda.synchronize(dev)

    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    ss = StreamSet(S, a.eps, device=dev)
    done = 0
    while done < L:
        c = min(a.chunk, L - done)
        u = torch.rand(S * c, dtype=torch.float64, device=dev, generator=gen)
        x = (1.0 - u).pow_(-1.0 / 1.5)  # Pareto(1.5) + 1, as numpy's pareto(1.5) + 1
        ss.ingest(x, torch.arange(S + 1, dtype=torch.int64, device=dev) * c)
        done += c
        del u, x
    ss.flush()
    every = torch.arange(S, dtype=torch.int32, device=dev)
    tenth = torch.randperm(S, device=dev, generator=gen)[:max(S // 10, 1)].to(torch.int32)
    nbytes = ss.pack_bytes()
    nbytes10 = ss.pack_select_bytes(tenth)
    buf_pack = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    buf_all = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    buf_10 = torch.zeros(nbytes10, dtype=torch.uint8, device=dev)
    fresh = StreamSet(S, a.eps, device=dev)

    def timed(call):
        sync()
        t0 = time.perf_counter()
        call()
        sync()
        return time.perf_counter() - t0

    def unpack_fresh():
        fresh.reset()
        fresh.sync()
        return timed(lambda: fresh.unpack_select(every, buf_pack))

    calls = [
        ("pack", nbytes, lambda: timed(lambda: ss.pack(buf_pack))),
        ("pack_select_all", nbytes, lambda: timed(lambda: ss.pack_select(every, buf_all))),
        ("pack_select_10", nbytes10, lambda: timed(lambda: ss.pack_select(tenth, buf_10))),
        ("unpack_fresh", nbytes, unpack_fresh),
        ("unpack_same", nbytes, lambda: timed(lambda: ss.unpack_select(every, buf_pack))),
    ]
    for _, _, run in calls:  # warm-up: code objects, scratch, arenas
        run()
    assert torch.equal(buf_pack, buf_all), "pack_select(all ids) differs from pack()"
    times = {name: [] for name, _, _ in calls}
    for _ in range(a.reps):
        for name, _, run in calls:
            times[name].append(run())
    check = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    assert torch.equal(fresh.pack(check), buf_pack), "the unpacked fresh set packs to other bytes"
    assert torch.equal(ss.pack(check), buf_pack), "the set unpacked into itself packs to other bytes"
    out = {"tool": "transfer_time", "engine": "MI355X" if on_gpu else "cpu (rehearsal, not a measurement)",
           "streams": S, "values_per_stream": L, "eps": a.eps, "reps": a.reps, "packed_bytes": nbytes,
           "packed_bytes_10pct": nbytes10, "promoted": ss.num_promoted, "calls": {}}
    for name, nb, _ in calls:
        t = times[name]
        med = statistics.median(t)
        out["calls"][name] = {"ms": [round(x * 1e3, 3) for x in t], "median_ms": round(med * 1e3, 3),
                              "min_ms": round(min(t) * 1e3, 3), "max_ms": round(max(t) * 1e3, 3),
                              "packed_bytes_over_call_time_GBps": round(nb / med / 1e9, 2)}
    print(json.dumps(out), flush=True)


def main():
    a = parse()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        r = subprocess.run(cmd, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        sys.stderr.write("transfer_time: the GPU step passed its time limit of %d s\n" % a.timeout)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
