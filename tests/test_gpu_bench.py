"""bench.py on one GPU (needs an MI355X): a plain run measures the headline and nothing else; --full adds the legs that
measure everything else.  Small frames (--small): the control flow, not the numbers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_parity import assert_bit_identical

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data", "config"}


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--small", *args],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "ONE JSON line:\n" + r.stdout[-2000:]
    return json.loads(lines[0])


def test_a_plain_run_prints_the_headline_and_dumps_the_timed_frame(oracle, tmp_path):
    """No --full: the line carries the headline and its config only, and --dump-outputs writes the frame the warm-up and timed
    steps accumulated, bit for bit the oracle's after (warmup + steps) x spp samples."""
    d = _bench("--dump-outputs", str(tmp_path))
    assert set(d) == HEADLINE_KEYS, sorted(set(d) ^ HEADLINE_KEYS)
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    w, h, spp = d["config"]["width"], d["config"]["height"], d["config"]["spp_per_step"]
    frames = np.load(os.path.join(str(tmp_path), "frames.npy"))
    assert frames.tolist() == [3.0 * spp]
    got = np.load(os.path.join(str(tmp_path), "pixels.npy"))
    assert_bit_identical(got, oracle.render(oracle.scene_analytical(), w, h, 3 * spp, seed=1), "bench.py --dump-outputs")


def test_full_adds_the_secondary_legs():
    d = _bench("--full")
    assert HEADLINE_KEYS <= set(d) and d["value"] > 0
    for key in ("roofline", "roofline_hbm", "general_kernels", "six_primitives", "relaxed", "resident_two_streams", "roofline_c4",
                "roofline_c5", "roofline_denoise_1080p", "roofline_denoise_4k", "c3_rank_tiles", "secondary"):
        assert key in d and "error" not in d[key], (key, d.get(key))
    assert d["roofline"]["flops_per_sample"] > 0
