"""bench.py's host side, no GPU: `--steps`, `--full` and what `--dump-outputs` writes (float32, under its size cap, the same sample every run)."""
import os

import numpy as np
import pytest

import bench


def test_steps_sets_the_timed_steps_and_must_be_positive():
    assert bench.parse_args(["--steps", "7", "--warmup", "2"]).steps == 7
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_full_is_off_by_default():
    assert bench.parse_args(["--steps", "3", "--warmup", "1"]).full is False
    assert bench.parse_args(["--steps", "3", "--warmup", "1", "--full"]).full is True


def test_dump_outputs_writes_the_whole_frame_as_float32(tmp_path):
    frame = np.random.default_rng(3).integers(0, 256, (96 * 128, 3), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path), frame)
    assert sorted(os.listdir(tmp_path)) == ["frame.npy"]
    got = np.load(tmp_path / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, frame.astype(np.float32))


def test_dump_outputs_samples_a_frame_above_the_cap_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100_000)
    frame = np.random.default_rng(4).integers(0, 256, (20_000, 3), dtype=np.uint8)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), frame)
    bench.dump_outputs(str(b), frame)
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= 100_000
    ids = np.load(a / "frame_pixel_ids.npy")
    assert ids.dtype == np.float64 and np.all(np.diff(ids) > 0) and 0 < ids.size < frame.shape[0]
    got = np.load(a / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, frame[ids.astype(np.int64)].astype(np.float32))
    assert np.array_equal(ids, np.load(b / "frame_pixel_ids.npy")) and np.array_equal(got, np.load(b / "frame.npy"))
