"""bench.py's command line and its --dump-outputs writer, on the host (no GPU): the plain run is the default, --full opts
into the other legs, --steps must time at least one step, and the dump is the output rows in row order -- the whole
output, or above DUMP_MAX_BYTES a fixed seeded sample of rows with their indices beside it."""
import os

import numpy as np
import pytest
import torch

import bench


class _Ctx:
    dist = None
    world = 1
    rank = 0


class _Job:
    def __init__(self, out):
        self.out = out
        self.n_total, self.vd = out.shape
        self.lo, self.hi = 0, out.shape[0]


def test_plain_run_is_the_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "12", "--warmup", "3"])
    assert a.full is False and a.dump_outputs is None and a.steps == 12 and a.warmup == 3
    b = bench.parse_args(["--steps", "4", "--full", "--dump-outputs", "somewhere"])
    assert b.full is True and b.dump_outputs == "somewhere"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_steps_and_warmup_are_checked(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def test_dump_outputs_whole(tmp_path):
    out = torch.randn(1000, 3, generator=torch.Generator().manual_seed(0))
    bench.dump_outputs(_Ctx, _Job(out), str(tmp_path / "d"))
    assert sorted(os.listdir(tmp_path / "d")) == ["out.npy"]
    got = np.load(tmp_path / "d" / "out.npy")
    assert got.dtype == np.float32 and np.array_equal(got, out.numpy())


def test_dump_outputs_sampled(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4000)
    out = torch.randn(5000, 2, generator=torch.Generator().manual_seed(0))
    for name in ("a", "b"):
        bench.dump_outputs(_Ctx, _Job(out), str(tmp_path / name))
    got, rows = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "a" / "out_rows.npy")
    assert rows.dtype == np.float64 and got.dtype == np.float32
    assert len(rows) == 4000 // (4 * 2 + 8) and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 5000
    assert np.array_equal(got, out.numpy()[rows.astype(np.int64)])
    assert got.nbytes + rows.nbytes <= 4000
    # the sample is fixed: the same rows on every run
    assert np.array_equal(rows, np.load(tmp_path / "b" / "out_rows.npy"))
    assert np.array_equal(got, np.load(tmp_path / "b" / "out.npy"))
