"""bench.py's command line on the CPU: the output dump (float64 .npy files, bounded in size) and
the options a plain run and a --full run take."""
import os

import numpy as np
import pytest

import bench


def test_dump_outputs_writes_float64_npy(tmp_path):
    import torch

    arrays = {"scores": torch.arange(6, dtype=torch.float64).reshape(2, 3),
              "best": torch.tensor([4, 1], dtype=torch.int64),
              "costs": np.linspace(0.0, 1.0, 5, dtype=np.float32)}
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), 0, 1, arrays)
    assert sorted(os.listdir(out)) == ["best.npy", "costs.npy", "scores.npy"]
    for name, a in arrays.items():
        got = np.load(out / f"{name}.npy")
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, np.asarray(a, dtype=np.float64))
    # one file per rank when there is more than one
    bench.dump_outputs(str(out), 3, 8, {"best": arrays["best"]})
    assert (out / "best_rank3.npy").exists()


def test_dump_outputs_caps_large_arrays(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1024)
    a = np.arange(4000, dtype=np.float64).reshape(500, 8)
    bench.dump_outputs(str(tmp_path), 0, 1, {"a": a})
    got = np.load(tmp_path / "a.npy")
    assert got.nbytes <= 1024 and got.shape == (16, 8)
    np.testing.assert_array_equal(got, a[:16])  # the leading rows: the same sample every run


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_rejects_empty_timed_region(monkeypatch, argv):
    monkeypatch.setattr("sys.argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2
