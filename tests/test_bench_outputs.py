"""bench.py's plain run, --full and --dump-outputs (host engine, --device cpu):
a plain run times exactly --steps steps and reports ms_per_step without the
roofline / CPU-baseline legs; --full brings them back; --dump-outputs writes
the last timed step's quantiles as float64 .npy, the same from run to run and
whatever the number of steps, equal to what the path returns (--dump).  On
the GPU: the plain run's dumped quantiles against the host engine's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
ARGS = ["--device", "cpu", "--gpus", "1", "--streams", "700", "--values", "333"]


def run(extra):
    env = dict(os.environ, OMP_NUM_THREADS="2")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, BENCH] + ARGS + extra, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("plain")
    line = run(["--steps", "3", "--warmup", "1", "--dump-outputs", str(d / "out"), "--dump", str(d / "npz")])
    return line, d


def test_plain_run_is_the_headline_only(plain):
    line, _ = plain
    assert line["steps"] == 3 and line["warmup"] == 1 and line["warmup_run"]["steps"] == 1
    assert line["unit"] == "values/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    # value = the batch's values per second of one step
    assert abs(line["value"] - 700 * 333 / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    assert "cpu_baseline" not in line and "weak" not in line
    assert line["roofline"]["achieved"] is None and "launch_ms" not in line["roofline"]


def test_dump_outputs_are_what_the_step_returned(plain):
    _, d = plain
    files = sorted(os.listdir(str(d / "out")))
    assert files == ["quantiles.npy"]
    q = np.load(str(d / "out" / "quantiles.npy"))
    assert q.dtype == np.float64 and q.shape == (700, 3)
    assert q.nbytes <= 64 * 1000 * 1000
    ret = np.load(str(d / "npz") + ".rank0.npz")["q"]
    assert np.array_equal(q.view(np.int64), ret.view(np.int64))
    assert np.all(q[:, 0] <= q[:, 1]) and np.all(q[:, 1] <= q[:, 2]) and np.all(q >= 1.0)  # Pareto(1.5)+1


def test_full_run_adds_the_roofline_and_same_outputs(plain, tmp_path):
    _, d = plain
    line = run(["--steps", "1", "--warmup", "0", "--full", "--no-cpu", "--dump-outputs", str(tmp_path / "out")])
    assert line["steps"] == 1 and line["ms_per_step"] > 0
    rf = line["roofline"]
    assert rf["bytes_per_launch"] > 8 * 700 * 333 and "launch_ms" in rf and "traffic_source" in rf
    q1 = np.load(str(d / "out" / "quantiles.npy"))
    q2 = np.load(str(tmp_path / "out" / "quantiles.npy"))
    assert np.array_equal(q1.view(np.int64), q2.view(np.int64)), "same arguments, other steps: other outputs"


def test_dump_sample_of_a_large_output(tmp_path):
    """Beyond the 64 MB limit: a fixed sample of the rows, their numbers beside it."""
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    import torch
    q = torch.arange(30, dtype=torch.float64).reshape(10, 3)
    old = bench.DUMP_LIMIT_BYTES
    bench.DUMP_LIMIT_BYTES = 4 * 8 * 4  # room for 4 rows of 3 quantiles + the row number
    try:
        for k in ("a", "b"):
            bench.dump_outputs(str(tmp_path / k), q, None, 0, 1)
    finally:
        bench.DUMP_LIMIT_BYTES = old
    rows = np.load(str(tmp_path / "a" / "quantiles_rows.npy"))
    got = np.load(str(tmp_path / "a" / "quantiles.npy"))
    assert rows.dtype == np.float64 and got.shape == (4, 3) and np.all(np.diff(rows) > 0)
    assert np.array_equal(got, q.numpy()[rows.astype(np.int64)])
    assert got.nbytes + rows.nbytes <= 4 * 8 * 4
    assert np.array_equal(rows, np.load(str(tmp_path / "b" / "quantiles_rows.npy")))


@pytest.mark.gpu
def test_plain_run_on_device(tmp_path, gpu_device):
    """The plain run on the GPU (no untimed step before the warm-up, no launch
    events): its dumped quantiles are, bit for bit, the host engine's on the
    same seeded batch."""
    S, L = 3000, 1000
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GK_BENCH_REHEARSE")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--streams", str(S), "--values", str(L), "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    line = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["n_gpus"] == 1
    assert abs(line["value"] - S * L / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    assert "cpu_baseline" not in line and line["roofline"]["achieved"] is None
    q = np.load(str(tmp_path / "out" / "quantiles.npy"))
    assert q.dtype == np.float64 and q.shape == (S, 3)
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    from gkarray_amd import StreamSet
    x, offs = bench.make_input(S, L, 3, gpu_device, "pareto")  # bench.py's default seed
    hs = StreamSet(S, 0.01, device="cpu")
    exp = hs.ingest(x.cpu(), offs.cpu(), quantiles=[0.5, 0.9, 0.99]).numpy()
    assert np.array_equal(q.view(np.int64), exp.view(np.int64))
