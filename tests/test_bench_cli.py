"""bench.py's --full / --dump-outputs switches and the output dump (CPU: no GPU call)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    sys.path.insert(0, ROOT)
    import bench as b
    return b


def test_plain_run_is_the_default(bench):
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(bench, tmp_path, monkeypatch):
    import torch
    rng = np.random.default_rng(3)
    bufs = [torch.from_numpy(rng.random((5, 64), dtype=np.float32)) for _ in range(2)]
    whole = torch.stack(bufs).numpy()
    bench.dump_outputs(str(tmp_path / "a"), bufs)
    got = np.load(tmp_path / "a" / "film_tiles.npy")
    assert got.dtype == np.float32 and np.array_equal(got, whole)
    # over the size limit: the same seeded sample of the elements in every run
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", whole.nbytes - 1)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    bench.dump_outputs(str(tmp_path / "b"), bufs)
    bench.dump_outputs(str(tmp_path / "c"), bufs)
    b, c = np.load(tmp_path / "b" / "film_tiles.npy"), np.load(tmp_path / "c" / "film_tiles.npy")
    assert b.dtype == np.float32 and b.shape == (100,) and np.array_equal(b, c)
    assert np.isin(b, whole).all() and len(np.unique(b)) > 50
