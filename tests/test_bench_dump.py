"""bench.py --dump-outputs: what a caller of the timed path received, as float32 / float64 .npy files, a fixed sample under the cap."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _items(n):
    rng = np.random.default_rng(5)
    return [{"pt": rng.standard_normal((10 + i, 3)), "its_done": (5, i % 4), "status": 0,
             "obs_outlier": (rng.random(7 + i) < 0.2).astype(np.uint8), "kf_vel": None} for i in range(n)]


def test_everything_written_when_it_fits(tmp_path):
    items = _items(6)
    bench.dump_outputs(str(tmp_path), items)
    assert sorted(os.listdir(tmp_path)) == ["its_done.npy", "obs_outlier.npy", "pt.npy", "sample.npy", "status.npy"]
    assert np.load(tmp_path / "sample.npy").tolist() == list(range(6))
    pt = np.load(tmp_path / "pt.npy")
    assert pt.dtype == np.float64 and np.array_equal(pt, np.concatenate([it["pt"].ravel() for it in items]))
    outl = np.load(tmp_path / "obs_outlier.npy")
    assert outl.dtype == np.float32 and np.array_equal(outl, np.concatenate([it["obs_outlier"] for it in items]))
    assert np.load(tmp_path / "its_done.npy").dtype == np.float64


def test_sample_is_fixed_and_under_the_cap(tmp_path):
    items = _items(200)
    cap = 20000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), items, cap=cap)
    sample = np.load(tmp_path / "a" / "sample.npy")
    assert 0 < len(sample) < 200 and (np.diff(sample) > 0).all()
    total = 0
    for f in os.listdir(tmp_path / "a"):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert np.array_equal(a, b)
        if f != "sample.npy":
            total += a.nbytes
    assert total <= cap
    pt = np.concatenate([items[int(i)]["pt"].ravel() for i in sample])
    assert np.array_equal(np.load(tmp_path / "a" / "pt.npy"), pt)
