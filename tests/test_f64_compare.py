"""The power of tests/f64_compare.py (CPU only): the comparison the relaxed-arithmetic kernels are held to (tests/test_gpu_relaxed.py)
passes frames that differ from the f64 frame by f32 rounding only — the strict f32 oracle's and the glibc-libm oracle's — and fails
frames of a subtly wrong scene: one light 1 % brighter, one primitive's roughness 0.03 higher, one sphere wearing another sphere's
material (what a kernel that picks the wrong material class renders)."""
import copy

import numpy as np
import pytest

import conftest
import f64_compare as F

W, H, SPP, SEED = 96, 64, 16, 3


@pytest.fixture(scope="module")
def oracle_f64():
    conftest._build_oracle()
    import oracle_lib
    return oracle_lib.Oracle("liboracle_f64.so")


def _scenes(rpt):
    """(name, scene, render flags): material-table scenes of tests/test_gpu_dispatch.py, an SDF scene, a large scene."""
    from rust_pathtracer_amd import scenes
    from test_gpu_dispatch import _table_scene
    out = []
    for which in ("reference", "overlapping patches", "camera inside glass", "three spheres on a floor", "six spheres two planes",
                  "eight spheres four planes", "sdf two planes", 9):
        s, flags = _table_scene(rpt, which)
        out.append((str(which), s, flags & rpt._abi.RPT_RENDER_RUSSIAN_ROULETTE))
    out.append(("sdf", scenes.sdf_scene(), 0))
    out.append(("large", scenes.random_spheres_scene(300, 5), 0))
    return out


def _calibrated(oracle, oracle_f64, scene, flags):
    return F.Calibrated(oracle, oracle_f64, scene.describe(), W, H, SPP, seed=SEED, render_flags=flags)


@pytest.mark.parametrize("index", range(10))
def test_oracle_frames_pass(rpt, oracle, oracle_libm, oracle_f64, index):
    name, scene, flags = _scenes(rpt)[index]
    cal = _calibrated(oracle, oracle_f64, scene, flags)
    assert cal.strict.median < 1e-6, (name, cal.strict)
    glibc = oracle_libm.render(scene.describe(), W, H, SPP, seed=SEED, render_flags=flags)
    cal.check(glibc, "%s: the glibc-libm oracle's frame" % name)


def _brighter_light(rpt, s):
    s = copy.deepcopy(s)
    L = s.lights[0]
    L.emission = tuple(float(np.float32(e) * np.float32(1.01)) for e in L.emission)
    return s


def _rougher_primitive(rpt, s):
    """The floor's material with its roughness 0.03 higher (a copy: other primitives may share the material)."""
    from rust_pathtracer_amd import scenes
    s = copy.deepcopy(s)
    plane = list(s.planes[0])
    mat = copy.deepcopy(s.materials[plane[3]])
    mat.fields["roughness"] = float(mat.fields.get("roughness", scenes._DEFAULTS["roughness"])) + 0.03
    s.materials.append(mat)
    plane[3] = len(s.materials) - 1
    s.planes[0] = tuple(plane)
    return s


def _swapped_material(rpt, s):
    """Sphere 1 wears sphere 0's material."""
    s = copy.deepcopy(s)
    assert s.spheres[0][2] != s.spheres[1][2]
    c, r, _ = s.spheres[1]
    s.spheres[1] = (c, r, s.spheres[0][2])
    return s


PERTURBATIONS = {"light x 1.01": _brighter_light, "roughness + 0.03": _rougher_primitive, "material swapped": _swapped_material}


@pytest.mark.parametrize("perturb", sorted(PERTURBATIONS))
@pytest.mark.parametrize("which", ["reference", "five spheres on a floor", "six spheres two planes", "eight spheres four planes"])
def test_frames_of_a_subtly_wrong_scene_fail(rpt, oracle, oracle_f64, which, perturb):
    """The f32 oracle's frame of the perturbed scene, held to the bounds of the original one: must fail.  (The material swap stands in
    for a wrong material class: it is tried on the 5-12-primitive scenes the by-class table serves.)"""
    from test_gpu_dispatch import _table_scene
    if perturb == "material swapped" and which == "reference":
        pytest.skip("the material swap is for the scenes of five to twelve primitives")
    s, _ = _table_scene(rpt, which)
    cal = _calibrated(oracle, oracle_f64, s, 0)
    wrong = PERTURBATIONS[perturb](rpt, s)
    frame = oracle.render(wrong.describe(), W, H, SPP, seed=SEED)
    dist = cal.distance(frame)
    assert cal.bounds.failures(dist), "%s, %s: the comparison passes a wrong frame: %r within %r" % (which, perturb, dist, cal.bounds)


def test_each_statement_has_teeth():
    """Distance / Bounds one statement at a time, on a synthetic frame: a non-finite pixel, a shifted median, extra flips, one pixel
    many samples off, and a bias far below the flip threshold each fail on their own."""
    rng = np.random.default_rng(4)
    h, w, spp = 64, 64, 16
    ref = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)
    ref[..., 3] = 1.0
    noise = lambda s: (rng.normal(0.0, s, (h, w, 4)) * [1, 1, 1, 0]).astype(np.float64)     # noqa: E731
    good = (ref + noise(1e-7)).astype(np.float32)
    flips = rng.choice(h * w, 10, replace=False)
    good.reshape(-1, 4)[flips, 0] += rng.choice([-1.0, 1.0], 10).astype(np.float32) / spp
    cal = F.calibrated_bounds(F.Distance(good, ref, spp))
    assert not cal.failures(F.Distance(good, ref, spp))

    def fails(frame, word):
        bad = cal.failures(F.Distance(frame, ref, spp))
        assert len(bad) >= 1 and any(word in b for b in bad), (word, bad)

    f = good.copy()
    f[3, 4, 1] = np.nan
    fails(f, "not finite")
    fails((ref + noise(1e-6)).astype(np.float32), "median")
    f = good.copy()
    more = rng.choice(h * w, 40, replace=False)
    f.reshape(-1, 4)[more, 2] += np.float32(0.5 / spp) * rng.choice([-1.0, 1.0], 40).astype(np.float32)
    fails(f, "flipped")
    f = good.copy()
    f[7, 7, 0] += 40.0 / spp
    fails(f, "samples")
    f = ref + noise(1e-7)                                             # 40 % of the pixels 9e-5 high: below the flip threshold
    f[rng.uniform(size=(h, w)) < 0.4, :3] += 9e-5
    assert F.Distance(f, ref, spp).n_flipped == 0
    fails(f.astype(np.float32), "bias")
