"""bench.py --dump-outputs: the writer alone, on CPU tensors (no GPU).

Asserted: every array lands as <name>.npy in float32 or float64; an array
within its share of the budget is written whole and bit for bit; a larger one
is cut to whole rows, the same sorted rows in every run (two dumps of the same
arrays are identical); the files together stay within the budget; rank r > 0
writes <name>.rank<r>.npy.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bench  # noqa: E402


def _arrays():
    g = torch.Generator().manual_seed(5)
    return {"posterior": torch.rand((37, 9, 16), dtype=torch.float64, generator=g),
            "loglik": torch.rand((37,), dtype=torch.float64, generator=g),
            "status": torch.arange(37, dtype=torch.int32),
            "half": torch.rand((5, 3), generator=g).to(torch.float16),
            "params": np.linspace(0.0, 1.0, 11)}


def test_dump_outputs_sample_and_types(tmp_path, monkeypatch):
    budget = 5 * 4096                                    # 4096 B per array: 3 of posterior's 37 rows (1152 B each)
    monkeypatch.setattr(bench, "DUMP_BUDGET", budget)
    arrs = _arrays()
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, arrs, 1, 0)
    bench.dump_outputs(b, arrs, 1, 0)
    assert sorted(os.listdir(a)) == sorted(n + ".npy" for n in arrs)
    got = {n: np.load(os.path.join(a, n + ".npy")) for n in arrs}
    for n in arrs:
        assert got[n].dtype in (np.float32, np.float64)
        assert np.array_equal(got[n], np.load(os.path.join(b, n + ".npy")))
    assert sum(x.nbytes for x in got.values()) <= budget
    assert got["half"].dtype == np.float32 and got["posterior"].dtype == np.float64
    assert np.array_equal(got["loglik"], arrs["loglik"].numpy())
    assert np.array_equal(got["status"], np.arange(37.0))
    assert np.array_equal(got["params"], arrs["params"])
    # whole rows of the source, in ascending row order
    post = arrs["posterior"].numpy()
    assert got["posterior"].shape == (3, 9, 16)
    rows = [int(np.flatnonzero((post == r).all(axis=(1, 2)))[0]) for r in got["posterior"]]
    assert rows == sorted(set(rows))


def test_dump_outputs_rank_suffix_and_share(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 2 * 2 * 1152)   # two ranks, two arrays: one posterior row each
    arrs = {k: v for k, v in _arrays().items() if k in ("posterior", "loglik")}
    bench.dump_outputs(str(tmp_path), arrs, 2, 1)
    assert sorted(os.listdir(tmp_path)) == ["loglik.rank1.npy", "posterior.rank1.npy"]
    assert np.load(tmp_path / "posterior.rank1.npy").shape == (1, 9, 16)
    assert np.load(tmp_path / "loglik.rank1.npy").shape == (37,)
