"""Random operation sequences (tests/opseq_cases.py) on the MI355X engine: the
configurations and seeds of opseq_cases.CONFIGS, whose coverage conditions
tests/test_cpu_opseq.py checks on the model for exactly these runs.  Every
stream of every set is compared bit for bit with its oracle after every
operation.  A failure names eps, seed and step; replay it with
``opseq_cases.run_sequence(dev, eps, seed, nops, stop_after=step, ...)``."""
import pytest

import opseq_cases as O

pytestmark = pytest.mark.gpu

# the stats layout of the default configuration, by position of the seed
# (None: the library's own choice)
FUSED_STATS = ["0", "8", None]


def _run(gpu_device, monkeypatch, name, eps, seed):
    cfg = O.CONFIGS[name]
    for k, v in cfg["env"].items():
        monkeypatch.setenv(k, v)
    r = O.run_sequence(gpu_device, eps, seed, cfg["nops"], **cfg["kw"])
    assert sum(r["ran"].values()) == cfg["nops"]


@pytest.mark.parametrize("eps,seed", O.runs("default", "gpu_seeds"))
def test_opseq_default(gpu_device, monkeypatch, eps, seed):
    """k_ingest_small, promotion to 2048, the product's launch paths."""
    fused = FUSED_STATS[O.CONFIGS["default"]["gpu_seeds"].index(seed) % len(FUSED_STATS)]
    if fused is not None:
        monkeypatch.setenv("GK_FUSED_STATS", fused)
    _run(gpu_device, monkeypatch, "default", eps, seed)


@pytest.mark.parametrize("eps,seed", O.runs("short_ladder", "gpu_seeds"))
def test_opseq_short_ladder(gpu_device, monkeypatch, eps, seed):
    """Four classes on small tables, promotion across several classes in one call, the unbounded class."""
    _run(gpu_device, monkeypatch, "short_ladder", eps, seed)


@pytest.mark.parametrize("eps,seed", O.runs("tiny_arenas", "gpu_seeds"))
def test_opseq_tiny_arenas(gpu_device, monkeypatch, eps, seed):
    """Two-slot arenas and ingests left in flight: deferral and replay ahead of every operation kind."""
    _run(gpu_device, monkeypatch, "tiny_arenas", eps, seed)


@pytest.mark.parametrize("eps,seed", O.runs("no_small_class", "gpu_seeds"))
def test_opseq_no_small_class(gpu_device, monkeypatch, eps, seed):
    """P = 1001: class 0 is 2048, presorted batches."""
    _run(gpu_device, monkeypatch, "no_small_class", eps, seed)


@pytest.mark.parametrize("eps,seed", O.runs("via_host", "gpu_seeds"))
def test_opseq_via_host(gpu_device, monkeypatch, eps, seed):
    """Moves through the host engine and back."""
    _run(gpu_device, monkeypatch, "via_host", eps, seed)


@pytest.mark.parametrize("eps,seed", O.runs("keyed_chunks", "gpu_seeds"))
def test_opseq_keyed_chunks(gpu_device, monkeypatch, eps, seed):
    """64-sample chunks of the two keyed rank kernels on the short ladder, the keyed kinds weighted up,
    keyed ingests and score-and-ingests left in flight."""
    _run(gpu_device, monkeypatch, "keyed_chunks", eps, seed)
