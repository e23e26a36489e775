"""bench.py's --dump-outputs writer (bench.dump_outputs) without a GPU: whole arrays below the caps, fixed seeded
samples with their positions above them, the same files on every call, 64 MB at most."""
import os

import numpy as np

import bench


def test_dump_outputs_small_results_are_written_whole(tmp_path):
    ids = np.array([5, 0, 31999, 7], np.uint32)
    offs = np.array([0, 1, 4], np.uint64)
    bench.dump_outputs(str(tmp_path), ids, offs)
    assert sorted(os.listdir(tmp_path)) == ["ids.npy", "offsets.npy"]
    got_ids, got_offs = np.load(tmp_path / "ids.npy"), np.load(tmp_path / "offsets.npy")
    assert got_ids.dtype == np.float32 and got_offs.dtype == np.float64
    np.testing.assert_array_equal(got_ids, ids.astype(np.float32))
    np.testing.assert_array_equal(got_offs, offs.astype(np.float64))


def test_dump_outputs_large_results_are_sampled_with_positions(tmp_path):
    rng = np.random.default_rng(1)
    ids = rng.integers(0, 65536, 20 << 20).astype(np.uint32)
    offs = np.cumsum(rng.integers(0, 40, (3 << 20) + 1)).astype(np.uint64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), ids, offs)
    names = ["ids.npy", "ids_index.npy", "offsets.npy", "offsets_index.npy"]
    assert sorted(os.listdir(tmp_path / "a")) == names
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    for n in names:  # a fixed sample: the same positions and values on every call
        np.testing.assert_array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
    for name, full in (("ids", ids), ("offsets", offs)):
        idx, vals = np.load(tmp_path / "a" / f"{name}_index.npy"), np.load(tmp_path / "a" / f"{name}.npy")
        assert idx.dtype == np.float64 and idx.size == vals.size and 0 < idx.size < full.size
        assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < full.size
        np.testing.assert_array_equal(vals.astype(np.float64), full[idx.astype(np.int64)].astype(np.float64))
