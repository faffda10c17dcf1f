"""CPU: bench.py's --dump-outputs writer (bench.dump_outputs) and the --full / --dump-outputs options.
Every array lands as DIR/<name>.npy in float32 (float64 stays float64); an array above DUMP_SAMPLE elements is
written as a sample whose indices depend only on the array's name and size, so two runs -- or two builds -- write the
same elements; the whole dump stays under DUMP_LIMIT.  The GPU test (tests/test_gpu_bench_outputs.py) runs bench.py
itself."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_writes_float32_and_samples_large_arrays(tmp_path):
    b = _bench()
    g = torch.Generator().manual_seed(0)
    big = torch.randn(3, b.DUMP_SAMPLE + 5, generator=g)
    arrays = [("loss_total", torch.tensor(2.5)), ("ids", torch.arange(7)), ("f64", torch.ones(4, dtype=torch.float64)),
              ("half", torch.ones(2, 3, dtype=torch.bfloat16)), ("grad.big", big)]
    b.dump_outputs(str(tmp_path / "a"), arrays)
    b.dump_outputs(str(tmp_path / "b"), arrays)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n, _ in arrays}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n, _ in arrays)
    assert got["loss_total"].dtype == np.float32 and got["loss_total"].tolist() == [2.5]
    assert got["ids"].dtype == np.float32 and got["ids"].tolist() == list(range(7))
    assert got["f64"].dtype == np.float64
    assert got["half"].dtype == np.float32 and got["half"].shape == (6,)
    s = got["grad.big"]
    assert s.dtype == np.float32 and s.shape == (b.DUMP_SAMPLE,)
    # the sample: elements of the flattened array in index order, the same ones on every run
    flat = big.reshape(-1).numpy()
    pos = np.searchsorted(np.sort(flat), s)
    assert np.array_equal(np.sort(flat)[pos], s), "every sampled value is an element of the array"
    assert np.array_equal(s, np.load(tmp_path / "b" / "grad.big.npy"))
    # a changed value at a sampled position shows in the dump (the sample is of positions, not of values)
    big2 = big.clone().reshape(-1)
    first = int(np.flatnonzero(flat == s[0])[0])
    big2[first] += 1.0
    b.dump_outputs(str(tmp_path / "c"), [("grad.big", big2.view_as(big))])
    c = np.load(tmp_path / "c" / "grad.big.npy")
    assert c[0] == s[0] + 1.0 and np.array_equal(c[1:], s[1:])


def test_dump_refuses_to_pass_the_size_limit(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "DUMP_LIMIT", 4 * 10)
    with pytest.raises(SystemExit):
        b.dump_outputs(str(tmp_path), [("a", torch.zeros(8)), ("b", torch.zeros(8))])
    assert b.DUMP_SAMPLE * 4 * 2000 <= 64 * 2 ** 20  # 2000 sampled arrays still fit the real limit


def test_full_and_dump_options_default_off(monkeypatch):
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = b.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out_dir"])
    a = b.parse()
    assert a.full is True and a.dump_outputs == "out_dir"
