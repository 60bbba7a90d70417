"""CPU-only: bench.py's --dump-outputs writer (float64 files, the size cap, the seeded instance sample)."""
import importlib

import numpy as np


def _arrays(B=40):
    rng = np.random.default_rng(1)
    return {"obs": rng.normal(size=(B, 6)), "reward": rng.normal(size=B), "terminated": rng.integers(0, 2, B).astype(np.uint8),
            "iterations": rng.integers(1, 9, B).astype(np.int32), "violations": rng.integers(0, 2, (B, 4)).astype(np.uint8), "skipped": None}


def test_dump_writes_every_array_whole_as_float64(tmp_path):
    bench = importlib.import_module("bench")
    a = _arrays()
    bench.write_outputs(str(tmp_path / "d"), a)
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == sorted(k + ".npy" for k in a if a[k] is not None)
    for k, v in a.items():
        if v is not None:
            got = np.load(tmp_path / "d" / (k + ".npy"))
            assert got.dtype == np.float64 and np.array_equal(got, v)


def test_dump_above_the_cap_is_the_same_seeded_sample_of_instances_in_every_array(tmp_path, monkeypatch):
    bench = importlib.import_module("bench")
    a = _arrays()
    per_instance = 8 * (6 + 1 + 1 + 1 + 4)
    limit = 10 * per_instance + 256 * 6
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
    for d in ("x", "y"):
        bench.write_outputs(str(tmp_path / d), a, ".rank1")
    idx = np.load(tmp_path / "x" / "instance.rank1.npy").astype(np.int64)
    assert 0 < len(idx) < 10 and np.all(np.diff(idx) > 0)
    assert sum(p.stat().st_size for p in (tmp_path / "x").iterdir()) <= limit
    for k, v in a.items():
        if v is not None:
            got = np.load(tmp_path / "x" / (k + ".rank1.npy"))
            assert np.array_equal(got, v[idx]) and np.array_equal(got, np.load(tmp_path / "y" / (k + ".rank1.npy")))
