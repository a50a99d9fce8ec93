"""CPU: the options of bench.py that decide what a run does, and the writer behind --dump-outputs."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_plain_run_is_the_default():
    """Everything beyond the headline (stage / kernel times, roofline, other conv mode, CPU baseline, parity) needs --full."""
    a = bench.build_parser().parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.build_parser().parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_writes_float32_and_samples_large_outputs(tmp_path):
    g = torch.Generator().manual_seed(1)
    small = torch.rand((3, 5), generator=g, dtype=torch.float64)
    big = torch.rand(bench.DUMP_SAMPLE + 17, generator=g)
    kept = torch.rand(bench.DUMP_SAMPLE + 3, generator=g)
    bench.dump_outputs(str(tmp_path / "a"), {"small": small, "big": big, "kept": kept}, whole=("kept",))
    bench.dump_outputs(str(tmp_path / "b"), {"big": big})
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["big_sample.npy", "kept.npy", "small.npy"], names
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (3, 5) and np.array_equal(s, small.float().numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "kept.npy"), kept.numpy())
    b = np.load(tmp_path / "a" / "big_sample.npy")
    assert b.dtype == np.float32 and b.shape == (bench.DUMP_SAMPLE,)
    assert np.isin(b, big.numpy()).all()
    # the sample positions are fixed: the same output gives the same sample in every run
    assert np.array_equal(b, np.load(tmp_path / "b" / "big_sample.npy"))


def test_dump_outputs_refuses_more_than_64_mb(tmp_path):
    huge = torch.zeros((bench.DUMP_LIMIT_BYTES // 4) + 1)
    with pytest.raises(SystemExit, match="limit"):
        bench.dump_outputs(str(tmp_path / "c"), {"huge": huge}, whole=("huge",))
    assert not os.path.exists(tmp_path / "c")
