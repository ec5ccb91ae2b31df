"""The product library itself.  The GPU tests run on librpt_hip_test.so — the product's objects linked with the hooks of
include/rpt_test.h (tests/conftest.py) — so this module checks librpt_hip.so in a process of its own: that it is the library a
plain import loads, that it refuses what it does not export, and that its frames are those of the test build and of the oracle,
bit for bit, for every kernel class."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = os.path.join(ROOT, "rust-pathtracer_amd", "librpt_hip.so")

CHILD = r'''
import hashlib, json, os, sys
sys.path.insert(0, os.path.join(%(root)r, "tests"))
os.environ.pop("RPT_LIB", None)                      # a plain import: the product
import importlib.util
spec = importlib.util.spec_from_file_location("rust_pathtracer_amd", os.path.join(%(root)r, "rust-pathtracer_amd", "__init__.py"),
                                              submodule_search_locations=[os.path.join(%(root)r, "rust-pathtracer_amd")])
rpt = importlib.util.module_from_spec(spec); sys.modules["rust_pathtracer_amd"] = rpt; spec.loader.exec_module(rpt)
from rust_pathtracer_amd import scenes
out = {"path": rpt._lib.LIB_PATH, "hooks": int(rpt.lib().rpt_build_has_test_hooks()), "has_probe": hasattr(rpt.lib(), "rpt_probe_fn")}
cases = {"small": (rpt.AnalyticalScene(), 96, 54, 5, 0), "compact": (rpt.AnalyticalScene(), 96, 54, 1, 0),
         "compact sparse": (rpt.AnalyticalScene(), 1040, 768, 1, 0),
         "nested": (rpt.AnalyticalScene(), 96, 54, 3, rpt._abi.RPT_RENDER_NESTED_LOOPS), "sdf": (scenes.sdf_scene(), 80, 45, 3, 0),
         "large": (scenes.random_spheres_scene(300, 5), 80, 45, 3, 0), "media": (scenes.media_scene(), 64, 36, 3, 0)}
FAST = rpt._abi.RPT_RENDER_FAST_MATH
cases.update({"small relaxed": (rpt.AnalyticalScene(), 96, 54, 5, FAST), "compact relaxed": (rpt.AnalyticalScene(), 96, 54, 1, FAST),
              "sdf relaxed": (scenes.sdf_scene(), 80, 45, 3, FAST), "large relaxed": (scenes.random_spheres_scene(300, 5), 80, 45, 3, FAST)})
for name, (scene, w, h, spp, flags) in cases.items():
    t = rpt.Tracer(scene, device=0, seed=4)
    t.flags = flags
    buf = rpt.ColorBuffer(w, h)
    t.render_n(buf, spp)
    out[name] = hashlib.sha1(buf.image().tobytes()).hexdigest()
    t.close()
import numpy as np
def image(w, h, seed):
    img = np.random.default_rng(seed).uniform(0, 3, (h, w, 4)).astype(np.float32)
    img[h // 2, w // 3, 0], img[1, 1, 1], img[h - 1, w - 1, :3] = -1.0, np.nan, 1e30
    buf = rpt.ColorBuffer(w, h)
    buf.pixels[:] = img.reshape(-1)
    return buf
for name, (w, h, it) in {"denoise": (200, 150, 3), "denoise 1": (65, 97, 1), "denoise 2": (65, 97, 2)}.items():
    out[name] = hashlib.sha1(image(w, h, w + it).denoise(it, 2.0).image().tobytes()).hexdigest()
out["u8"] = hashlib.sha1(image(1021, 3, 5).convert_to_u8().tobytes()).hexdigest()
print("RESULT " + json.dumps(out))
'''


@pytest.mark.gpu
def test_the_product_library_renders_what_the_test_build_renders(rpt, oracle):
    import json
    from rust_pathtracer_amd import scenes
    assert rpt.lib().rpt_build_has_test_hooks() == 1 or os.environ.get("RPT_LIB"), "the tests are expected to run on the test build"
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600,
                       env={k: v for k, v in os.environ.items() if k != "RPT_LIB"})
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert os.path.samefile(got["path"], PRODUCT) and got["hooks"] == 0 and not got["has_probe"]
    # ("compact sparse": 3 120 workgroups, beyond the compacting kernel's dense form)
    cases = {"small": (rpt.AnalyticalScene(), 96, 54, 5, 0), "compact": (rpt.AnalyticalScene(), 96, 54, 1, 0),
             "compact sparse": (rpt.AnalyticalScene(), 1040, 768, 1, 0),
             "nested": (rpt.AnalyticalScene(), 96, 54, 3, rpt._abi.RPT_RENDER_NESTED_LOOPS), "sdf": (scenes.sdf_scene(), 80, 45, 3, 0),
             "large": (scenes.random_spheres_scene(300, 5), 80, 45, 3, 0), "media": (scenes.media_scene(), 64, 36, 3, 0)}
    # the relaxed-arithmetic build of each kernel class (RPT_RENDER_FAST_MATH): not the oracle's frame (tests/test_gpu_relaxed.py holds
    # it to the f64 oracle), but the same objects in both libraries, so the same frame
    FAST = rpt._abi.RPT_RENDER_FAST_MATH
    cases.update({"small relaxed": (rpt.AnalyticalScene(), 96, 54, 5, FAST), "compact relaxed": (rpt.AnalyticalScene(), 96, 54, 1, FAST),
                  "sdf relaxed": (scenes.sdf_scene(), 80, 45, 3, FAST), "large relaxed": (scenes.random_spheres_scene(300, 5), 80, 45, 3, FAST)})
    for name, (scene, w, h, spp, flags) in cases.items():
        want = oracle.render(scene.describe(), w, h, spp, seed=4)
        t = rpt.Tracer(scene, device=0, seed=4)
        t.flags = flags
        buf = rpt.ColorBuffer(w, h)
        t.render_n(buf, spp)
        t.close()
        here = buf.image()
        same = (here.view(np.uint32) == want.view(np.uint32)) | (np.isnan(here) & np.isnan(want))
        assert same.all() or flags & FAST, "%s: the test build differs from the oracle" % name
        assert not flags & FAST or np.isfinite(here).all(), "%s: non-finite pixels" % name
        assert got[name] == hashlib.sha1(here.tobytes()).hexdigest(), "%s: the product library's frame differs from the test build's" % name

    def image(w, h, seed):                                           # (the child's inputs: a pole, a NaN, a saturated pixel)
        img = np.random.default_rng(seed).uniform(0, 3, (h, w, 4)).astype(np.float32)
        img[h // 2, w // 3, 0], img[1, 1, 1], img[h - 1, w - 1, :3] = -1.0, np.nan, 1e30
        buf = rpt.ColorBuffer(w, h)
        buf.pixels[:] = img.reshape(-1)
        return buf
    # the denoiser (denoise_fused_kernel<3>, <1>, <2>) and the u8 conversion: the oracle's, and the same in both libraries
    for name, (w, h, it) in {"denoise": (200, 150, 3), "denoise 1": (65, 97, 1), "denoise 2": (65, 97, 2)}.items():
        src = image(w, h, w + it)
        here = src.denoise(it, 2.0).image()
        want = oracle.denoise(src.image(), w, h, it, 2.0)
        assert ((here.view(np.uint32) == want.view(np.uint32)) | (np.isnan(here) & np.isnan(want))).all(), name
        assert got[name] == hashlib.sha1(here.tobytes()).hexdigest(), "%s: the product library's result differs from the test build's" % name
    src = image(1021, 3, 5)
    here = src.convert_to_u8()
    assert np.array_equal(here, oracle.convert_to_u8(src.image(), 1021, 3))
    assert got["u8"] == hashlib.sha1(here.tobytes()).hexdigest(), "u8: the product library's frame differs from the test build's"
