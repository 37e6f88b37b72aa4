"""bench.py --dump-outputs: what dump_outputs writes for a frame (host logic only, no GPU)."""
import numpy as np

import bench


def test_small_frame_is_written_whole(tmp_path):
    frame = np.random.default_rng(3).random((7, 5, 3))
    bench.dump_outputs(str(tmp_path / "d"), frame)
    got = np.load(tmp_path / "d" / "frame.npy")
    assert got.dtype == np.float64 and np.array_equal(got, frame)


def test_large_frame_is_a_fixed_pixel_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100 * 24)  # 100 f64 RGB pixels
    frame = np.random.default_rng(4).random((20, 30, 3))
    bench.dump_outputs(str(tmp_path / "a"), frame)
    bench.dump_outputs(str(tmp_path / "b"), frame)
    a, b = np.load(tmp_path / "a" / "frame.npy"), np.load(tmp_path / "b" / "frame.npy")
    assert a.dtype == np.float64 and a.shape == (100, 3) and a.nbytes <= bench.DUMP_LIMIT_BYTES
    assert np.array_equal(a, b)  # the same pixels in every run
    # every row is a pixel of the frame, taken in increasing flat index (random values: a row names its pixel)
    px = frame.reshape(-1, 3)
    idx = [int(np.flatnonzero((px == row).all(axis=1))[0]) for row in a]
    assert idx == sorted(set(idx))


def test_whole_c2_frame_fits_the_limit():
    _, W, H, _, _ = bench.WORKLOADS[bench.SINGLE_GPU_WORKLOAD]
    assert W * H * 3 * 8 <= bench.DUMP_LIMIT_BYTES <= 64_000_000
