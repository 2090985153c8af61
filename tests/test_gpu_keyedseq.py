"""Random operation sequences on a KeyedStreamSet (tests/keyedseq_cases.py) on
the MI355X engine: the configurations and seeds of keyedseq_cases.CONFIGS, whose
events tests/test_cpu_keyedseq.py requires on the model for exactly these runs.
keys(), the sizes and every id of the stream set are compared after every
operation.  A failure names eps, seed and step; replay it with
``keyedseq_cases.run_sequence(dev, eps, seed, nops, stop_after=step, ...)``."""
import pytest

import keyedseq_cases as S

pytestmark = pytest.mark.gpu


def _run(gpu_device, monkeypatch, name, eps, seed):
    cfg = S.CONFIGS[name]
    for k, v in cfg["env"].items():
        monkeypatch.setenv(k, v)
    r = S.run_sequence(gpu_device, eps, seed, cfg["nops"], **cfg["kw"])
    assert sum(r["ran"].values()) == cfg["nops"]


@pytest.mark.parametrize("eps,seed", S.runs("default", "gpu_seeds"))
def test_keyedseq_default(gpu_device, monkeypatch, eps, seed):
    """The default ladder: recycled ids that inherit the 2048 class, growth by doubling with holes."""
    _run(gpu_device, monkeypatch, "default", eps, seed)


@pytest.mark.parametrize("eps,seed", S.runs("short_ladder", "gpu_seeds"))
def test_keyedseq_short_ladder(gpu_device, monkeypatch, eps, seed):
    """Four classes, two-slot arenas and 64-sample chunks of the keyed rank kernels."""
    _run(gpu_device, monkeypatch, "short_ladder", eps, seed)


@pytest.mark.parametrize("eps,seed", S.runs("max_streams", "gpu_seeds"))
def test_keyedseq_max_streams(gpu_device, monkeypatch, eps, seed):
    """max_streams=48: batches that would pass it are refused with nothing changed."""
    _run(gpu_device, monkeypatch, "max_streams", eps, seed)
