"""The eight material-mapped mesh kernel forms held to the float64 restatement of one pixel-sample (tests/mesh_mmap_f64.py:
MmapMeshDescScene, a subclass of the composed restatement that scales roughness and metallic after the base's patch).

Eight cases, one per form 12 .. 19 (rpt_debug_mesh_form): test_gpu_mesh_compose_f64's cases A .. H — its scene, textures, lamp, sky,
mask and bump maps, taken through its inputs() — with the object's material made metallic (mesh_mmap_f64.scene) and
mesh_mmap_f64.material_maps on top: a 16 x 16 BILINEAR noise map on the object (G roughness, B = 255 - G metallic) and a 5 x 3
NEAREST one on the lamp (R roughness, no metallic channel).  400 samples per case (64 x 48, 200 random pixels x 2 seeds, each a
one-sample render into a fresh buffer), compared through test_gpu_path_f64.Tally with test_path_f64's TAU / REL_CLEAN / NEAR_TIE_MAX:
this file has no tolerance of its own.

The planted fault (test_the_restatement_sees_the_wrong_field, CPU): the factors applied to each other's field moves MOVED = 60 clean
samples beyond REL_CLEAN on case A over test_gpu_mesh_compose_f64's grid of 552 pixels at seed 7 — counted again on every run; the
composed file asks more than 10 of its faults, and so does this one.  test_an_all_255_map_is_the_composed_restatement (CPU) closes the
other side: with both factors exactly 1 the subclass gives the composed restatement's samples bit for bit (its margins can only
narrow: the lamp's NEAREST map adds its texel borders).

The first 150 clean samples of every case are also held to their own f32 tolerance (tests/f32_spread.py, through Tally.add's
spreads; 1.8 to 2.3 s of CPU time per case, computed once for both legs).  test_the_spreads_of_the_restatement holds the conditions
on the CPU (at most 2 % of a case's clean samples have a tolerance above 1e-3), test_the_spreads_see_a_factor_two_percent_off the
metallic factor times 1.02: within REL_CLEAN everywhere, beyond their own tolerance on 51 of 73 clean samples on the object.  The
largest z seen on an MI355X, per case: A 1.37, B 1.21, C 0.89, D 1.62, E 1.68, F 1.29, G 1.25, H 1.34, next to Z_MAX = 8.3; the
medians 0.12 to 0.33.  Measurements, not bounds."""
import ctypes as C
import functools

import numpy as np
import pytest

import f32_spread as S
import mesh_mmap_f64 as MM
from mesh_compose_f64 import ComposedMeshDescScene, ComposedPath, sample_pixels
from test_gpu_mesh_compose_f64 import CASES, GRID, H, W, inputs
from test_gpu_path_f64 import Tally
from test_mesh_material_map_host import MAP_FORM_FIRST, TEXTURED_FORMS
from test_path_f64 import NEAR_TIE_MAX, REL_CLEAN, TAU, rel_distance

MOVED = 60                                                           # test_the_restatement_sees_the_wrong_field prints it


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def form_of(case):
    """12 .. 19: the map over the kernel the composed file's case runs."""
    return MAP_FORM_FIRST + TEXTURED_FORMS.index(CASES[case][4])


def _draws(case):
    k = sorted(CASES).index(case)
    rng = np.random.default_rng([41, k])
    return [(310 + 10 * k + seed, list(zip(rng.integers(0, W, 200).tolist(), rng.integers(0, H, 200).tolist()))) for seed in (1, 2)]


@functools.lru_cache(maxsize=None)
def _restated(oracle, case):
    s = MM.scene()
    path = ComposedPath(MM.MmapMeshDescScene(s.describe(), s, material_maps=MM.material_maps(), **inputs(s, case)))
    return [(seed, pixels) + sample_pixels(path, oracle, seed, pixels, W, H) for seed, pixels in _draws(case)]


@functools.lru_cache(maxsize=None)
def _spreads(oracle, case):
    """The f32 spreads (tests/f32_spread.py) of the case's first 150 clean samples, computed once beside _restated for the CPU and
    the GPU leg: ([spreads per seed, NaN where there is none], CPU seconds)."""
    s = MM.scene()
    path = ComposedPath(MM.MmapMeshDescScene(s.describe(), s, material_maps=MM.material_maps(), **inputs(s, case)))
    return S.spreads_of_draws(path, oracle, _restated(oracle, case), W, H)


def set_composed(t, args):
    """The composed file's set calls, in its order."""
    t.set_mesh_textures(args["textures"])
    t.set_mesh_shading({m: "smooth" for m in args["smooth"]})
    t.set_mesh_lights({m: True for m in args["on"]})
    if args["cutouts"]:
        t.set_mesh_cutouts(args["cutouts"])
    if args["normal_maps"]:
        t.set_mesh_normal_maps(args["normal_maps"])
    if args["environment"]:
        t.set_environment(**args["environment"])


def mesh_form(rpt, t):
    form = C.c_uint32(0)
    assert rpt.lib().rpt_debug_mesh_form(t._h, C.byref(form)) == 0
    return form.value


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_material_mapped_renders_against_the_restatement(rpt, oracle, torch_cuda, case):
    s = MM.scene()
    args = inputs(s, case)
    tally = Tally(TAU, NEAR_TIE_MAX)
    spreads, seconds = _spreads(oracle, case)
    print("case %s: the spreads took %.2f s of CPU time" % (case, seconds))
    for (seed, pixels, restated, margins), spread in zip(_restated(oracle, case), spreads):
        t = rpt.Tracer(s, device=0, seed=seed)
        try:
            set_composed(t, args)
            t.set_mesh_material_maps(MM.material_maps())
            buf = rpt.DeviceColorBuffer(W, H)
            t.render_n(buf, 1)
            torch_cuda.cuda.synchronize()
            frame = buf.pixels.cpu().numpy()
            assert mesh_form(rpt, t) == form_of(case), "case %s: form %d, not %d" % (case, mesh_form(rpt, t), form_of(case))
        finally:
            t.close()
        tally.ran.add("form %d" % form_of(case))
        print("case %s (seed %d): %d of %d samples below TAU" % (case, seed, int((margins <= TAU).sum()), len(margins)))
        tally.add("case %s (seed %d, form %d)" % (case, seed, form_of(case)), frame, restated, margins, pixels, spreads=spread)
    tally.check("case %s" % case)
    assert tally.n == 400


def test_the_forms_of_the_cases_are_12_to_19():
    assert [form_of(c) for c in sorted(CASES)] == list(range(12, 20))


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_spreads_of_the_restatement(rpt, oracle, case):
    """The conditions of the comparison with spreads, on the restatement alone: at least 100 clean samples of the case have a spread,
    and at most 5 % of them a tolerance above 1e-3."""
    spreads, seconds = _spreads(oracle, case)
    S.case_conditions("case %s" % case, _restated(oracle, case), spreads, seconds)


def test_the_spreads_see_a_factor_two_percent_off(rpt, oracle):
    """The metallic factor times 1.02, rounded to f32, as a device's samples, over the grid's pixels on the object under case A's
    inputs: no clean sample leaves REL_CLEAN, so the comparison without spreads passes it; at least 10 leave their own tolerance.
    The object's metallic is 0.3 here, so that 1 - metallic, which scales the diffuse lobe, moves by under a percent per bounce (at
    the cases' 0.7 it moves by up to 4.7 %, and two bounces on the object take a sample beyond REL_CLEAN)."""
    from rust_pathtracer_amd import scenes
    from test_gpu_mesh_compose_f64 import object_pixels
    s = MM.scene()
    s.materials[0] = scenes.full_material(rgb=(0.8, 0.3, 0.25), roughness=0.9, metallic=0.3)
    good = ComposedPath(MM.MmapMeshDescScene(s.describe(), s, material_maps=MM.material_maps(), **inputs(s, "A")))
    bad = ComposedPath(MM.MmapMeshDescScene(s.describe(), s, material_maps=MM.material_maps(), factor_scale=(1.0, 1.02), **inputs(s, "A")))
    pixels = object_pixels(good.scene)
    print("%d pixels on the object" % len(pixels))
    S.teeth_on("the metallic factor x 1.02 (case A)", good, bad, oracle, [(7, pixels)], W, H)


def test_the_restatement_sees_the_wrong_field(rpt, oracle):
    """The restatement with each factor applied to the other field moves more than 10 clean samples beyond REL_CLEAN on case A, whose
    noise map's channels disagree everywhere: a device with that fault would fail the comparison above."""
    s = MM.scene()
    args = inputs(s, "A")
    base, marg = sample_pixels(ComposedPath(MM.MmapMeshDescScene(s.describe(), s, material_maps=MM.material_maps(), **args)), oracle, 7, GRID, W, H)
    mutant = ComposedPath(MM.MmapMeshDescScene(s.describe(), s, material_maps=MM.material_maps(), factor_on_wrong_field=True, **args))
    moved, marg2 = sample_pixels(mutant, oracle, 7, GRID, W, H)
    far = (rel_distance(np.nan_to_num(moved), np.nan_to_num(base)) > REL_CLEAN) & (marg > TAU) & (marg2 > TAU)
    print("factor_on_wrong_field (case A): %d clean samples beyond REL_CLEAN" % int(far.sum()))
    assert far.sum() > 10
    assert int(far.sum()) == MOVED


@pytest.mark.parametrize("case", ["A", "H"])
def test_an_all_255_map_is_the_composed_restatement(rpt, oracle, case):
    """Both factors exactly 1: the samples are the composed restatement's, bit for bit (the BILINEAR lookup of a
    constant 1 is exactly 1 in float64 as well, by include/rpt.h's argument: 1 - f is exact)."""
    s = MM.scene()
    args = inputs(s, case)
    pixels = GRID[::6]
    want = sample_pixels(ComposedPath(ComposedMeshDescScene(s.describe(), s, **args)), oracle, 9, pixels, W, H)
    got = sample_pixels(ComposedPath(MM.MmapMeshDescScene(s.describe(), s, material_maps=MM.material_maps(identity=True), **args)), oracle, 9, pixels, W, H)
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.nan_to_num(want[0]).any()
    assert (got[1] <= want[1]).all(), "the map's NEAREST lookup can only add margins"
    near = np.array_equal(got[1], want[1])
    print("case %s: margins %s" % (case, "equal" if near else "narrowed by the lamp's NEAREST map at %d samples" % int((got[1] < want[1]).sum())))
