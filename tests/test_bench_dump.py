"""bench.py --dump-outputs: the files it writes (float32 / float64) and the seeded row sample that keeps them under the cap."""
import numpy as np
import torch

import bench


def test_dump_writes_float32_and_float64(tmp_path):
    bench.dump_outputs(str(tmp_path), {"a": torch.arange(6, dtype=torch.float16).reshape(3, 2),
                                       "b": np.array([0.25, 0.5], dtype=np.float64)}, rows=3)
    a, b = np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy")
    assert a.dtype == np.float32 and np.array_equal(a, np.arange(6, dtype=np.float32).reshape(3, 2))
    assert b.dtype == np.float64 and np.array_equal(b, [0.25, 0.5])


def test_dump_samples_the_same_windows_of_every_per_window_array(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 4 * 1000)
    rows = 500
    preds = np.arange(rows, dtype=np.float32)[:, None]
    recons = np.repeat(preds[:, None, :], 3, axis=1)            # 16 bytes per window in all: 250 windows fit
    loss = np.ones(2)
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), {"preds": preds, "recons": recons, "loss": loss}, rows=rows)
    p, r = np.load(tmp_path / "one" / "preds.npy"), np.load(tmp_path / "one" / "recons.npy")
    assert p.shape == (249, 1) and r.shape == (249, 3, 1)      # (4000 - 16 bytes of `loss`) / 16 bytes per window
    assert np.all(np.diff(p[:, 0]) > 0) and np.array_equal(r[:, 0, :], p) and np.array_equal(np.load(tmp_path / "one" / "loss.npy"), loss)
    assert np.array_equal(p, np.load(tmp_path / "two" / "preds.npy"))
    assert sum(f.stat().st_size for f in (tmp_path / "one").iterdir()) <= 4000 + 3 * 128   # + one .npy header per file
