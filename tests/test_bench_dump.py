"""bench.py --dump-outputs: what it writes of the timed path's frame (CPU only; the GPU run itself is bench.py's)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _written(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}, sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_a_frame_that_fits_is_written_whole(tmp_path):
    img = np.random.default_rng(1).random((1080, 1920, 4), dtype=np.float32)
    bench.dump_outputs(str(tmp_path), {**bench.image_outputs("pixels", img, bench.DUMP_LIMIT_BYTES // 2), "frames": [3072.0]})
    got, size = _written(str(tmp_path))
    assert sorted(got) == ["frames", "pixels"] and size <= bench.DUMP_LIMIT_BYTES
    assert got["pixels"].dtype == np.float32 and got["pixels"].tobytes() == img.tobytes()
    assert got["frames"].dtype == np.float64 and got["frames"].tolist() == [3072.0]


def test_a_larger_frame_is_a_fixed_sample_within_the_budget(tmp_path):
    """configs[2]'s 3840x2160 frame (133 MB): the same seeded pixels every run, their indices beside them, 64 MB in all."""
    img = np.random.default_rng(2).random((2160, 3840, 4), dtype=np.float32)
    a = bench.image_outputs("image", img, bench.DUMP_LIMIT_BYTES // 2)
    b = bench.image_outputs("image", img + 1.0, bench.DUMP_LIMIT_BYTES // 2)
    assert sorted(a) == ["image_sample", "image_sample_index"]
    assert np.array_equal(a["image_sample_index"], b["image_sample_index"])
    idx = a["image_sample_index"]
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 2160 * 3840
    assert np.array_equal(a["image_sample"], img.reshape(-1, 4)[idx.astype(np.int64)])
    bench.dump_outputs(str(tmp_path), {**a, "frames": [1024.0]})
    got, size = _written(str(tmp_path))
    assert sorted(got) == ["frames", "image_sample", "image_sample_index"] and size <= bench.DUMP_LIMIT_BYTES


def test_only_f32_and_f64_within_the_budget(tmp_path):
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path), {"counts": np.zeros(4, np.uint32)})
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path), {"big": np.zeros(bench.DUMP_LIMIT_BYTES // 4 + 1, np.float32)})
