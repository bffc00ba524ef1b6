"""CPU: bench.py's --dump-outputs writer (float32 files, a fixed seeded sample of rows above the 64 MB budget)."""
import numpy as np
import pytest


@pytest.fixture
def bench(monkeypatch):
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # (bench.py sets it on import; monkeypatch puts the old value back)
    import bench as b
    return b


def test_dump_outputs_writes_float32(tmp_path, bench):
    x = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    bench.dump_outputs(str(tmp_path / "out"), {"samples": x, "loss": np.array([1.5], dtype=np.float64)})
    got = np.load(tmp_path / "out" / "samples.npy")
    assert got.dtype == np.float32 and got.shape == (2, 3, 4)
    np.testing.assert_array_equal(got, x.astype(np.float32))
    assert np.load(tmp_path / "out" / "loss.npy").tolist() == [1.5]
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["loss.npy", "samples.npy"]


def test_dump_outputs_samples_rows_above_the_budget(tmp_path, monkeypatch, bench):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)
    x = np.arange(100 * 20, dtype=np.float32).reshape(100, 20)          # 8000 bytes: 45 rows + their indices fit in 4000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"samples": x})
    got, rows = np.load(tmp_path / "a" / "samples.npy"), np.load(tmp_path / "a" / "samples_rows.npy")
    assert got.nbytes + rows.nbytes <= 4000 and got.shape == (45, 20) and rows.dtype == np.float64
    assert np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(got, x[rows.astype(np.int64)])
    np.testing.assert_array_equal(got, np.load(tmp_path / "b" / "samples.npy"))      # the same rows every time
