"""The float64 restatement of mesh media (tests/mesh_media_f64.py) on the CPU: its reductions, the near-tie condition of the draws
tests/test_gpu_mesh_media_f64.py compares on an MI355X, and the planted faults.

Eight cases on scenes.mesh_media_scene — the glass icosphere (mesh 0) and the lamp quad (mesh 1) — at the composed file's four
bounces, under the composed file's inputs for its cases A .. H (textures on both meshes, mesh 0 SMOOTH, mesh 1 ON in every case, so
the lamp is inside the pick throughout; the SAMPLED sky in B, D, F and H; the mask on mesh 0 in C, D, G and H; the normal maps in E
to H).  The medium sits on mesh 0 and rotates over the cases, so that each type appears twice:

  case  form  medium on mesh 0
  A     28    ABSORB    density 3, colour (0.9, 0.45, 0.3)
  B     29    SCATTER   density 2.5, colour (0.85, 0.9, 0.95), g = 0
  C     30    SCATTER   the same, g = 0.6
  D     31    EMISSIVE  density 0.5, colour (0.2, 0.6, 0.9)
  E     32    ABSORB    as A
  F     33    SCATTER   g = 0.6                                   (the sampled sky and the lamp in one pick)
  G     34    EMISSIVE  as D
  H     35    SCATTER   g = 0

The near-tie condition (test_the_near_tie_count_of_the_restatement): the restatement alone over exactly the GPU test's draws — 200
random pixels x 2 seeds per case — samples of 400 at or below TAU / samples with radiance, BELOW_TAU and LIT below, counted again
on every run; the cap is test_path_f64's NEAR_TIE_MAX (48 of 400) and is a condition, not a measurement:
  A 17 / 215    B 18 / 384    C 16 / 248    D 13 / 397    E 30 / 241    F 16 / 377    G 23 / 232    H 19 / 397
(4.25 %, 4.5 %, 4.0 %, 3.25 %, 7.5 %, 4.0 %, 5.75 %, 4.75 %): every case under the cap, every case with far more than a quarter of
its samples lit.  No case's medium had to be changed to stay under it.

Mutations (test_the_restatement_sees_the_join): clean samples moved beyond REL_CLEAN over the composed file's grid of 552 pixels at
seed 7, counted again on every run, each on the case, the medium and the scene that exercise it (MUTATIONS below):
  side_uses_shading_normal      case E   14   ABSORB density 6, the normal maps at strength 4
  env_sample_attenuated         case D   26   SCATTER density 6, the sky the only pickable light
  no_light_attenuation_inside   case C   19   ABSORB density 3
  medium_from_sphere_hit        case A   21   ABSORB density 6, a diffuse sphere of radius 0.4 inside the icosphere
  hole_leaves_medium            case C   30   SCATTER g = 0.6
  scatter_nee_offset_by_eps     case D   21   SCATTER density 6, the sky the only pickable light, the scene's eps 0.05
The last one needs a scene whose eps is a visible fraction of the mesh: a light estimate from a point moved by eps sees the sky
through the mask's holes from somewhere else, and the fault is worth about eps / distance.  At the scene's own eps = 0.005 against
an icosphere of radius 0.6 it moved 0 to 3 clean samples over every case, density 2.5 to 12 and four to twelve bounces; at 0.02 it
moves 11, at 0.05 21 (27 at density 12).  (On the device the question does not arise in this form: path_shade_medium calls
nee_query<false>, whose scatter_pos is the point itself whatever normal it is handed.)

The spreads (tests/f32_spread.py): spreads() computes each case's once, for the CPU conditions here and for the GPU comparison;
two subtle faults — sigma_t x 1.02, the phase function at g + 0.01 — pass REL_CLEAN on every clean sample and fail the samples' own
tolerances (34 of 63 and 15 of 50 clean samples on the icosphere)."""
import functools

import numpy as np
import pytest

import f32_spread as S
import media_sdf_f64 as MS
from mesh_compose_f64 import ComposedMeshDescScene, ComposedPath, sample_pixels
from mesh_media_f64 import MediaMeshDescScene, MediaMeshPath
from test_gpu_mesh_compose_f64 import CASES, GRID, H, W, inputs
from test_path_f64 import NEAR_TIE_MAX, REL_CLEAN, TAU, rel_distance

AMBER = dict(type="absorb", density=3.0, color=(0.9, 0.45, 0.3))
GLOW = dict(type="emissive", density=0.5, color=(0.2, 0.6, 0.9))


def fog(g):
    return dict(type="scatter", density=2.5, color=(0.85, 0.9, 0.95), anisotropy=g)


MEDIA = {"A": AMBER, "B": fog(0.0), "C": fog(0.6), "D": GLOW, "E": AMBER, "F": fog(0.6), "G": GLOW, "H": fog(0.0)}
# Counted on the CPU (test_the_near_tie_count_of_the_restatement prints the figures): of each case's 400 samples, those at or below
# TAU, and those that carry radiance.
BELOW_TAU = {"A": 17, "B": 18, "C": 16, "D": 13, "E": 30, "F": 16, "G": 23, "H": 19}
LIT = {"A": 215, "B": 384, "C": 248, "D": 397, "E": 241, "F": 377, "G": 232, "H": 397}
# fault -> (the case that exercises it, where it is planted, the medium, what else the scene needs, clean samples moved beyond REL_CLEAN)
DENSE_AMBER = dict(AMBER, density=6.0)
MUTATIONS = {
    # a SMOOTH medium mesh under the normal map at strength 4: G and the bent normal disagree about the side of a grazing direction
    "side_uses_shading_normal": ("E", "path", DENSE_AMBER, dict(strength=4.0), 14),
    # the SAMPLED sky as the only pickable light (no rpt_light, the lamp OFF), seen from inside through the mask's holes
    "env_sample_attenuated": ("D", "path", dict(fog(0.0), density=6.0), dict(sky_only=True), 26),
    "no_light_attenuation_inside": ("C", "path", AMBER, {}, 19),     # the lamp and the light through the mask's holes
    "scatter_nee_offset_by_eps": ("D", "path", dict(fog(0.0), density=6.0), dict(sky_only=True, eps=0.05), 21),
    "medium_from_sphere_hit": ("A", "path", DENSE_AMBER, dict(sphere_inside=0.4), 21),      # a diffuse sphere inside the icosphere
    "hole_leaves_medium": ("C", "scene", fog(0.6), {}, 30),
}


def scene(sphere_inside=None):
    from rust_pathtracer_amd import scenes
    s = scenes.mesh_media_scene(None)[0]
    s.max_depth = 4
    if sphere_inside:
        s.materials.append(scenes.full_material(rgb=(0.8, 0.8, 0.2), roughness=0.8))
        s.spheres = [((0.0, 0.0, 0.0), sphere_inside, len(s.materials) - 1)]
    return s


def draws(case):
    """[(seed, pixels)]: 200 random pixels at each of two seeds, the case's own."""
    k = sorted(CASES).index(case)
    rng = np.random.default_rng([52, k])
    return [(510 + 10 * k + seed, list(zip(rng.integers(0, W, 200).tolist(), rng.integers(0, H, 200).tolist()))) for seed in (1, 2)]


@functools.lru_cache(maxsize=None)
def restated(oracle, case):
    """The restatement of the case's draws, computed once for every test that needs it: [(seed, pixels, radiance, margins)]."""
    s = scene()
    path = MediaMeshPath(MediaMeshDescScene(s.describe(), s, media={0: MEDIA[case]}, **inputs(s, case)))
    return [(seed, pixels) + sample_pixels(path, oracle, seed, pixels, W, H) for seed, pixels in draws(case)]


def path_of(case, medium=None):
    s = scene()
    return MediaMeshPath(MediaMeshDescScene(s.describe(), s, media={0: MEDIA[case] if medium is None else medium}, **inputs(s, case)))


@functools.lru_cache(maxsize=None)
def spreads(oracle, case):
    """The f32 spreads (tests/f32_spread.py) of the case's first 150 clean samples, computed once beside restated() for the CPU and
    the GPU leg: ([spreads per seed, NaN where there is none], CPU seconds)."""
    return S.spreads_of_draws(path_of(case), oracle, restated(oracle, case), W, H)


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_spreads_of_the_restatement(rpt, oracle, case):
    """The conditions of the comparison with spreads, on the restatement alone: at least 100 clean samples of the case have a spread,
    and at most 5 % of them a tolerance above 1e-3."""
    spr, seconds = spreads(oracle, case)
    S.case_conditions("case %s" % case, restated(oracle, case), spr, seconds)


THIN_AMBER = dict(AMBER, density=0.75)
DENSE_FOG = dict(fog(0.6), density=6.0)


def test_the_spreads_see_sigma_t_two_percent_off(rpt, oracle):
    """An ABSORB medium whose density is 1.02 times the scene's, rounded to f32, as a device's samples, over the grid's pixels on the icosphere under case A's
    inputs.
    The medium is AMBER at density 0.75: a path crosses the icosphere (radius 0.6) at most three times in four bounces, so the
    fault is worth at most 3 * 1.2 * 0.7 * 0.75 * 0.02 = 3.8 % and no clean sample leaves REL_CLEAN — the comparison without spreads
    passes it; at least 10 leave their own tolerance."""
    from test_gpu_mesh_compose_f64 import object_pixels
    bad = dict(THIN_AMBER, density=THIN_AMBER["density"] * 1.02)
    good = path_of("A", THIN_AMBER)
    S.teeth_on("sigma_t x 1.02 (case A, ABSORB at density 0.75)", good, path_of("A", bad), oracle, [(7, object_pixels(good.scene))], W, H)


def test_the_spreads_see_the_phase_function_s_g_off_by_a_hundredth(rpt, oracle, monkeypatch):
    """phase_hg evaluated at g + 0.01 (the sampler keeps g, so the paths stay where they are), rounded to f32, as a device's samples,
    over the grid's pixels on the icosphere under case D's inputs and SCATTER at density 6, g = 0.6 (dense, so that many paths scatter; the mask's holes and the
    sampled sky, because a light estimate from inside a closed mesh is always shadowed by it and the phase function's value then
    reaches no pixel): within REL_CLEAN everywhere, beyond their own tolerance on at least 10 clean samples."""
    from mesh_compose_f64 import sample_pixels as sp
    from test_gpu_mesh_compose_f64 import object_pixels
    good = path_of("D", DENSE_FOG)
    entries = [(seed, pixels) + sp(good, oracle, seed, pixels, W, H) for seed, pixels in [(7, object_pixels(good.scene))]]
    spr, _ = S.spreads_of_draws(good, oracle, entries, W, H, count=None)
    plain = MS.phase_hg
    monkeypatch.setattr(MS, "phase_hg", lambda c, g: plain(c, g + 0.01))
    S.teeth("HG phase g + 0.01 (case D, density 6)", entries, spr, [sp(good, oracle, seed, pixels, W, H) for seed, pixels, _, _ in entries])


@pytest.mark.parametrize("case", ["A", "D", "H"])
def test_without_a_medium_it_is_the_composed_restatement(rpt, oracle, case):
    """This test fails without the feature: there is no restatement to import.  With no medium on any mesh — none given, or every one
    None — MediaMeshPath gives ComposedPath's samples and margins bit for bit."""
    s = scene()
    rng = np.random.default_rng(53)
    pixels = list(zip(rng.integers(0, W, 64).tolist(), rng.integers(0, H, 64).tolist()))
    want = sample_pixels(ComposedPath(ComposedMeshDescScene(s.describe(), s, **inputs(s, case))), oracle, 5, pixels, W, H)
    for media in (None, {0: None, 1: dict(type=None, density=3.0, color=(0.5, 0.5, 0.5))}):
        got = sample_pixels(MediaMeshPath(MediaMeshDescScene(s.describe(), s, media=media, **inputs(s, case))), oracle, 5, pixels, W, H)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and want[0].any()


@pytest.mark.parametrize("case", ["A", "C", "F"])
def test_a_white_absorb_medium_is_no_medium(rpt, oracle, case):
    """ABSORB of colour (1, 1, 1): exp(-0) = 1 over every segment and every light sample, and no draw.  The same radiance as no
    medium, exactly (the margins may only shrink: the side test's sign is recorded as well)."""
    s = scene()
    rng = np.random.default_rng(54)
    pixels = list(zip(rng.integers(0, W, 64).tolist(), rng.integers(0, H, 64).tolist()))
    want = sample_pixels(MediaMeshPath(MediaMeshDescScene(s.describe(), s, **inputs(s, case))), oracle, 6, pixels, W, H)
    white = {0: dict(type="absorb", density=7.5, color=(1.0, 1.0, 1.0)), 1: dict(type="emissive", density=0.0, color=(0.3, 0.6, 0.9))}
    got = sample_pixels(MediaMeshPath(MediaMeshDescScene(s.describe(), s, media=white, **inputs(s, case))), oracle, 6, pixels, W, H)
    assert np.array_equal(got[0], want[0]) and (got[1] <= want[1]).all() and want[0].any()
    amber = sample_pixels(MediaMeshPath(MediaMeshDescScene(s.describe(), s, media={0: AMBER}, **inputs(s, case))), oracle, 6, pixels, W, H)
    assert not np.array_equal(amber[0], want[0]), "a coloured one is no identity"


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_near_tie_count_of_the_restatement(rpt, oracle, case):
    """The restatement alone, for exactly the draws of the GPU comparison, case by case: no more than the project's 12 % of the
    samples lie at or below TAU, more than a quarter carry radiance, and both counts are the ones in this file."""
    below = total = lit = 0
    for _, _, radiance, margins in restated(oracle, case):
        below += int((margins <= TAU).sum())
        total += len(margins)
        lit += int((radiance.max(axis=1) > 0).sum())
    print("case %s: %d of %d samples below TAU (%.2f %%), %d with radiance" % (case, below, total, 100.0 * below / total, lit))
    assert total == 400 and below <= NEAR_TIE_MAX * total and lit > total // 4
    assert (below, lit) == (BELOW_TAU[case], LIT[case])


@pytest.mark.parametrize("fault", sorted(MUTATIONS))
def test_the_restatement_sees_the_join(rpt, oracle, fault):
    """A restatement with one line of the join wrong moves more than 10 clean samples beyond REL_CLEAN on the case that exercises it: a
    device with that fault would fail the comparison on the GPU."""
    case, where, medium, needs, count = MUTATIONS[fault]
    s = scene(sphere_inside=needs.get("sphere_inside"))
    composed = inputs(s, case)
    if needs.get("sky_only"):
        s.lights, composed["on"] = [], ()
    s.eps = needs.get("eps", s.eps)
    for nm in (composed["normal_maps"] or {}).values():
        nm["strength"] = needs.get("strength", nm["strength"])
    args = dict(media={0: medium}, **composed)
    base, marg = sample_pixels(MediaMeshPath(MediaMeshDescScene(s.describe(), s, **args)), oracle, 7, GRID, W, H)
    if where == "scene":
        mutant = MediaMeshPath(MediaMeshDescScene(s.describe(), s, **args, **{fault: True}))
    else:
        mutant = MediaMeshPath(MediaMeshDescScene(s.describe(), s, **args), **{fault: True})
    moved, marg2 = sample_pixels(mutant, oracle, 7, GRID, W, H)
    far = (rel_distance(np.nan_to_num(moved), np.nan_to_num(base)) > REL_CLEAN) & (marg > TAU) & (marg2 > TAU)
    print("%s (case %s): %d clean samples beyond REL_CLEAN" % (fault, case, int(far.sum())))
    assert far.sum() > 10, fault
    assert int(far.sum()) == count
