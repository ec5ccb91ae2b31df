"""The oracle held to tests/media_sdf_f64.py, the float64 restatement of participating media and of the SDF object written from
include/rpt.h's text (not from oracle/rpt_oracle.hpp), sample by sample.  CPU only.  The bounds are tests/test_path_f64.py's, imported.

  * shared_sets(): the inputs that this file and the GPU leg (tests/test_gpu_media_sdf_f64.py) both use, one case per strict SDF and
    media kernel at least: the ten sized SDF kernels' scenes of tests/test_gpu_strict_kernels.py (varied in what the kernel choice does
    not depend on), the two general ones, the object alone, the object full of fog; media_scene(), three purpose-built scenes (a lamp
    in dense fog whose anisotropy lies beyond the clamp, a lamp and a matt sphere in absorbing amber, media_scene() with isotropic
    fog and spheres without a medium inside the balls) and six fuzzed ones, each through the megakernel and the compacting kernel;
    300 spheres with media.  8 960 samples, every one of frame 0.
  * Coverage, from the restatement alone.  Event counters over the shared sets (each asserted >= 30): scatter 4 553, absorb segments
    1 602, emissive segments 227, lit light samples inside a medium 2 057, entered 3 337, left 2 218, scatter with |g| set beyond 0.9
    3 319, with |g| < 0.001 552, scatter before an emitter and a later surface 116, a surface without a medium inside one 529; SDF hit
    at t = 0 1 326, steps exhausted 644, max_t exit 6 399, accepted as first primitive 84, won over an earlier hit 1 422, lost to one 43,
    any_hit ignoring max_dist 323, under max_dist 801 (beyond it 37), smin with h > 0 80 935, torus evaluations 101 407.
    Near-tie shares per pool (one pool = one GPU test = one Tally; asserted <= 0.09): sdf 0.068 of 3 520, media 0.051 of 5 040.  The
    large class has its own margin and cap (TAU_LARGE, NEAR_TIE_MAX_LARGE = 0.7: every one of 300 miss tests per ray counts): 0.355
    of 400, asserted <= three quarters of its cap.
  * The f64 oracle against the restatement: the shared sets, 24 fuzzed media scenes (every medium type, densities 0 and 10^4, anisotropy
    beyond the clamp, roulette on half) and 24 fuzzed SDF scenes (1-8 primitives, max_steps 1 and 7, both any_hit modes, scenes with no
    sphere and no plane) — 20 480 samples, 0 outside the f32-rounding band (so none needed its margin).
  * Per function, the f64 oracle's entry points against the restatement's at 2 ulp(f32): phase_hg, sample_hg (g in {0, +-0.0005,
    +-0.001, +-0.3, +-0.9}, r2 at 0 and 1 - 2^-24, v on the onb's switch), sdf_eval and sdf_normal (points on, inside and outside each
    primitive and on a torus's axis, 1-8 primitives, k in {0.05, 0.35, 1}), the march (origins inside, max_steps 1 and 7, max_t below
    the first step) and each medium's transmittance (dist = +inf among them).
  * Teeth: each of media_sdf_f64.MUTANTS, over the first 200 items of the shared cases it bears on, puts at least 10 samples outside
    the band on the f64 leg and moves at least 10 clean samples beyond REL_CLEAN on the f32 leg.  Measured (f64 / f32):
    g_not_clamped 586 / 355, emitter_flag_kept 83 / 70, scatter_ray_offset_eps 651 / 73, nee_medium_unattenuated 482 / 390,
    nee_surface_unattenuated 528 / 78, entering_by_ffnormal 381 / 285, phase_cos_sign_in_nee 482 / 293, sample_hg_about_d 852 / 749,
    emissive_without_density 122 / 70, absorb_with_color 600 / 562, scatter_transmittance_per_channel 611 / 395, phase_pdf_not_stored
    137 / 32, in_medium_cleared_by_plain_surface 325 / 259, medium_after_emission 67 / 67, hit_eps_without_t 522 / 80, smin_half
    448 / 197, central_difference_normal 661 / 28, torus_about_z 678 / 469, sdf_unconditional 28 / 28, sdf_any_hit_ignores_max_dist
    26 / 17, sdf_before_planes 156 / 149.  ("max_t tested before the step" is no mutant: it is the same march.)
  * The f32 oracle (the device's twin) on the shared sets at TAU, REL_CLEAN, NEAR_TIE_MAX (TAU_LARGE, NEAR_TIE_MAX_LARGE for the large
    class): clean samples asserted per case, near ties per pool.  Measured: largest clean relative distance 5.9e-3 (sdf two lights;
    4.1e-3 sdf sized<4>, 4.0e-3 five primitives, the other SDF cases <= 1.1e-3), 3.9e-4 over the media cases, 2.1e-4 on the large one;
    near ties per case 0-8.6 % for the SDF cases (the object full of fog 16.2 %: the checker floor seen through glass), 1.0-13.3 % for
    the media cases.  The largest margin at which an f32 sample took another branch (landed beyond REL_CLEAN): 5.2e-5, below TAU.
With the clamp of g, the `* t` of the march's hit test or the attenuation of the scatter point's light sample deleted from
oracle/rpt_oracle.hpp, the f64 and the f32 comparison here both fail (and test_march_per_function for the second)."""
import collections

import numpy as np
import pytest

import conftest
import media_sdf_f64 as MS
import pt_f64 as P
from scene_fuzz import random_small_scene
from test_path_f64 import (F64_TIE, NEAR_TIE_MAX, NEAR_TIE_MAX_LARGE, REL_CLEAN, TAU, TAU_LARGE, close, first_diverging_ray, in_band,
                           rel_distance)

POOL_SHARE_MAX = 0.09        # largest near-tie share of a pool, from the restatement alone: a quarter below NEAR_TIE_MAX
EVENTS_MIN = 30              # every event counter over the shared sets
TEETH_MIN = 10               # samples a mutant must move, on each leg

# name, scene, frame, render flags, seed, items [(col, row, 0)]; then what the GPU leg needs: the kernel a one-sample launch of the case
# takes, its scene class, whether RPT_COMPACT_MAX_SPP=0 (the megakernel instead of the compacting kernel), and the pool (one Tally)
Case = collections.namedtuple("Case", "name scene w h flags seed items kernel klass mega pool")


@pytest.fixture(scope="module")
def oracle_f64():
    conftest._build_oracle()
    import oracle_lib
    return oracle_lib.Oracle("liboracle_f64.so")


def _plain(**fields):
    """A whole material with no medium.  (A sphere inside a ball is tested after the ball, and a patch is applied over what the ball's
    patch left: a partial one would inherit the ball's spec_trans and its medium.)"""
    from rust_pathtracer_amd import scenes
    return scenes.full_material(medium=dict(type="none"), **fields)


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------
def lamp_in_fog(rpt, g=1.1):
    """tests/test_oracle_media.py's ball of fog (density 3, anisotropy beyond the clamp) seen from close, with a lamp of radius 0.4 at
    its centre — a camera ray's segment inside ends on the lamp, scatters before it, and the path goes on to the ball's wall: the emitter
    flag of step 1 —, a small emissive sphere without a medium inside the fog (the medium acts BEFORE its emission; a surface without
    a medium leaves in_medium alone), and a second lamp outside, which the ball's own wall occludes from inside."""
    from test_oracle_media import ball_scene
    medium = dict(type="scatter", density=3.0, color=(0.9, 0.8, 0.7), anisotropy=g)
    s = ball_scene(rpt, medium, bg=(0.3, 0.35, 0.4), depth=9)
    # (roughness 0.2, not the ball's 0: at 0 every near-normal GGX sample is a near tie of pt_f64.sample_ggxvndf's `lensq > 0`)
    s.materials[0] = rpt.Material(rgb=(1.0, 1.0, 1.0), spec_trans=1.0, ior=1.05, roughness=0.2, medium=medium)
    s.camera = rpt.Pinhole((0.15, 0.1, 2.1), (0.1, 0.0, 0.0), 40.0)
    s.materials.append(_plain(rgb=(0.6, 0.6, 0.6), emission=(1.5, 0.8, 0.3), roughness=0.7))
    s.spheres.append(((0.45, 0.1, 0.55), 0.25, 1))
    s.lights = [rpt.AnalyticalLight.spherical((0.0, 0.0, 0.0), 0.4, (5.0, 5.0, 5.0)),
                rpt.AnalyticalLight.spherical((-2.5, 2.0, 1.5), 0.5, (6.0, 6.0, 6.0))]
    s.any_hit_uses_max_dist = True
    return s


def lamp_in_amber(rpt):
    """A ball of absorbing amber seen from close, with a matt sphere without a medium and a lamp inside it: most camera paths cross the
    wall, reach the matt sphere and take their direct light from the lamp THROUGH the amber (step 3 *: attenuated per channel)."""
    from test_oracle_media import ball_scene
    medium = dict(type="absorb", density=2.5, color=(0.9, 0.55, 0.15))
    s = ball_scene(rpt, medium, bg=(0.3, 0.35, 0.4), depth=6)
    s.materials[0] = rpt.Material(rgb=(1.0, 1.0, 1.0), spec_trans=1.0, ior=1.05, roughness=0.2, medium=medium)
    s.materials.append(_plain(rgb=(0.8, 0.8, 0.8), roughness=0.9))
    s.spheres.append(((0.0, -0.15, -0.1), 0.6, 1))
    s.camera = rpt.Pinhole((0.0, 0.3, 2.3), (0.0, 0.0, 0.0), 50.0)
    s.lights = [rpt.AnalyticalLight.spherical((0.25, 0.6, 0.55), 0.12, (8.0, 8.0, 8.0))]
    s.any_hit_uses_max_dist = True
    return s


def three_media(rpt):
    """media_scene() with the fog practically isotropic (|g| < 0.001: sample_hg's other arm), the amber denser, an emissive floor lamp
    (a sphere with surface emission) behind the amber, and a matt sphere without a medium inside the fog and one inside the amber: a bounce
    off them leaves in_medium alone, and their direct light from the lamp inside the fog is attenuated (step 3 *)."""
    from rust_pathtracer_amd import scenes
    s = scenes.media_scene()
    s.materials[0].medium["anisotropy"] = 0.0005
    s.materials[0].medium["density"] = 2.4
    s.materials[1].medium["density"] = 2.0
    s.materials.append(rpt.Material(rgb=(0.5, 0.5, 0.5), emission=(2.0, 1.6, 0.8), roughness=0.8))
    s.spheres.append(((2.3, -0.5, -0.9), 0.5, 4))
    s.materials.append(_plain(rgb=(0.8, 0.8, 0.8), roughness=0.9))           # no medium: inside a ball, in_medium stays
    s.spheres.append(((-1.1, -0.45, 0.35), 0.3, 5))                                      # in the fog, next to the lamp inside it
    s.spheres.append(((1.1, 0.0, 0.3), 0.35, 5))                                         # in the amber, under a lamp inside the amber
    s.lights.append(rpt.AnalyticalLight.spherical((1.1, 0.55, 0.55), 0.12, (9.0, 9.0, 9.0)))
    s.max_depth = 10
    return s


def fuzz_media_scene(rpt, seed):
    """-> (scene, render flags): tests/test_gpu_media.py's random media over scene_fuzz.random_small_scene at scale 1; roulette on odd
    seeds."""
    from test_gpu_media import _add_random_media
    s, _, _, rng = random_small_scene(rpt, seed, log2_scale=0)
    _add_random_media(rpt, s, rng)
    return s, (rpt._abi.RPT_RENDER_RUSSIAN_ROULETTE if seed % 2 else 0)


def fuzz_sdf_scene(rpt, seed):
    from test_gpu_parity import _random_sdf_scene
    return _random_sdf_scene(rpt, seed)[0]


SHARED_FUZZ_MEDIA = (3, 8, 13, 18, 21, 30)


def _sdf_case(rpt, n, table):
    """tests/test_gpu_strict_kernels.py's scene of the sized SDF kernel <n> (table: with one sphere, so that the material table fits),
    with what the kernel choice does not depend on varied case by case, so that the ten sized cases differ in more than the primitive
    count: any_hit's mode and the lamp's place, the step budget, hit_eps, smooth_k, normal_eps, max_t, and a floor whose patch sets a
    field (metallic) that the object's material leaves alone."""
    from test_gpu_strict_kernels import _sdf
    s = _sdf(rpt, n, spheres=1 if table else 2)
    if table:
        s.materials[2] = rpt.Material(roughness=1.0, metallic=0.8, checker_dir=(0.5, 100.0, 0.25, 0.1))
        s.sdf.update(smooth_k=(0.05, 1.0, 0.35, 0.35)[n - 1], normal_eps=(1e-2, 1e-3, 3e-2, 1e-2)[n - 1])
        if n == 2:
            s.sdf.update(max_t=4.5)
        if n == 4:
            s.sdf.update(max_steps=9)
    else:
        s.spheres[1] = ((-1.1, -0.3, 1.3), 0.45, 1)       # in front of the object: it wins against the march
        if n in (2, 4):                                   # a lamp close in front of the object's big sphere: from the floor and the sphere before
            s.any_hit_uses_max_dist = True                # it, shadow rays that pass the lamp reach the object beyond max_dist
            s.lights = [rpt.AnalyticalLight.spherical((-0.9, -0.3 if n == 2 else 0.15, 1.15 if n == 2 else 1.1), 0.2, (14.0, 13.0, 12.0))]
            s.spheres[1] = ((0.5, -0.55, 1.6), 0.45, 1)
            s.camera = rpt.Pinhole((0.0, 2.4, 3.4), (-0.4, -0.6, 0.9), 70.0)            # from above: the floor before the lamp is in view
        if n == 3:
            s.sdf.update(max_steps=12, hit_eps=1e-2)
    return s


def _pixels(rng, w, h, n, rows=None):
    r0, r1 = rows if rows else (0, h)
    return [(int(c), int(r), 0) for c, r in zip(rng.integers(0, w, n), rng.integers(r0, r1, n))]


def shared_sets(rpt):
    """-> [Case]: the inputs of the CPU leg's f32 comparison, coverage and teeth, and of the GPU leg (tests/test_gpu_media_sdf_f64.py).
    One-sample renders into a fresh buffer, so every item is of frame 0."""
    from test_gpu_strict_kernels import _large_media, _media, _sdf, _sdf_fog
    RR = rpt._abi.RPT_RENDER_RUSSIAN_ROULETTE
    rng = np.random.default_rng(20261019)
    out = []
    w, h = 86, 61
    for n in (1, 2, 3, 4):
        out.append(Case("sdf sized<%d>" % n, _sdf_case(rpt, n, False), w, h, 0, 60 + n, _pixels(rng, w, h, 280),
                        "render_sdf_march2_sized_kernel<%d>" % n, "sdf", False, "sdf"))
        out.append(Case("sdf sized table<%d>" % n, _sdf_case(rpt, n, True), w, h, RR if n == 3 else 0, 70 + n, _pixels(rng, w, h, 280),
                        "render_sdf_march2_sized_table_kernel<%d>" % n, "sdf", False, "sdf"))
    out.append(Case("sdf five primitives", _sdf(rpt, 5, spheres=2), w, h, 0, 81, _pixels(rng, w, h, 320), "render_sdf_march2_kernel", "sdf", False,
                    "sdf"))
    out.append(Case("sdf two lights", _sdf(rpt, 3, lights=2), w, h, RR, 82, _pixels(rng, w, h, 320), "render_sdf_march2_table_kernel", "sdf", False,
                    "sdf"))
    alone = _sdf(rpt, 3)
    alone.spheres, alone.planes = [], []                      # the object is the scene's first primitive: accepted whenever it is hit
    out.append(Case("sdf object alone", alone, w, h, 0, 84, _pixels(rng, w, h, 240), "render_sdf_march2_table_kernel", "sdf", False, "sdf"))
    out.append(Case("sdf full of fog", _sdf_fog(rpt), w, h, 0, 83, _pixels(rng, w, h, 400), "render_sdf_march2_media_kernel", "sdf", False,
                    "sdf"))
    w, h = 98, 73
    k = 0
    for name, s, flags in (("media scene", _media(rpt), 0), ("media scene, roulette", _media(rpt), RR), ("lamp in fog", lamp_in_fog(rpt), 0),
                           ("lamp in fog, roulette", lamp_in_fog(rpt), RR), ("three media", three_media(rpt), 0),
                           ("lamp in amber", lamp_in_amber(rpt), 0)):
        for mega in (True, False):
            out.append(Case("%s, %s" % (name, "megakernel" if mega else "compacting"), s, w, h, flags, 90 + k, _pixels(rng, w, h, 300),
                            "render_small_regen_media_kernel" if mega else "render_small_compact_media_kernel", "small", mega,
                            "media"))
            k += 1
    for i, seed in enumerate(SHARED_FUZZ_MEDIA):
        s, flags = fuzz_media_scene(rpt, seed)
        mega = i % 2 == 0
        out.append(Case("media fuzz seed %d" % seed, s, 64, 48, flags, 110 + i, _pixels(rng, 64, 48, 240),
                        "render_small_regen_media_kernel" if mega else "render_small_compact_media_kernel", "small", mega,
                        "media"))
    out.append(Case("300 spheres with media", _large_media(rpt), 74, 43, 0, 120, _pixels(rng, 74, 43, 400), "render_large_regen_media_kernel",
                    "large", False, "large"))
    return out


def restate(case, oracle, mut=(), limit=None):
    """-> (radiance, margins, rays, events) of the case's items (the first `limit`)."""
    items = case.items[:limit] if limit else case.items
    scene = MS.MediaSdfDescScene(case.scene.describe())
    return MS.sample_many(scene, oracle, case.seed, items, case.w, case.h, mut=mut, roulette=bool(case.flags & P.RENDER_RUSSIAN_ROULETTE))


def oracle_samples(oracle, case, limit=None):
    items = case.items[:limit] if limit else case.items
    c, r, f = (np.array([it[k] for it in items]) for k in range(3))
    return oracle.sample_pixels_flags(case.scene.describe(), c, r, f, case.w, case.h, seed=case.seed, render_flags=case.flags)


MEDIA_MUTANTS = ("g_not_clamped", "emitter_flag_kept", "scatter_ray_offset_eps", "nee_medium_unattenuated", "nee_surface_unattenuated",
                 "entering_by_ffnormal", "phase_cos_sign_in_nee", "sample_hg_about_d", "emissive_without_density", "absorb_with_color",
                 "scatter_transmittance_per_channel", "phase_pdf_not_stored", "in_medium_cleared_by_plain_surface", "medium_after_emission")
SDF_MUTANTS = ("hit_eps_without_t", "smin_half", "central_difference_normal", "torus_about_z", "sdf_unconditional",
               "sdf_any_hit_ignores_max_dist", "sdf_before_planes")
TEETH_ITEMS = 200            # of every case a mutant bears on, the first so many items


@pytest.fixture(scope="module")
def shared(rpt, oracle, oracle_f64):
    """-> [(case, restated radiance, margins, rays, events, f64 oracle's samples, f32 oracle's samples)], each computed once."""
    out = []
    for c in shared_sets(rpt):
        got, marg, rays, ev = restate(c, oracle_f64)
        out.append((c, got, marg, rays, ev, oracle_samples(oracle_f64, c), oracle_samples(oracle, c)))
    return out


def _tau(case):
    return TAU_LARGE if case.klass == "large" else TAU


def test_the_guard_of_pt_f64(rpt):
    """pt_f64.DescScene refuses what it does not restate; the scene class here reads it."""
    from rust_pathtracer_amd import scenes
    for s in (scenes.media_scene(), scenes.sdf_scene()):
        with pytest.raises(ValueError):
            P.DescScene(s.describe())
        MS.MediaSdfDescScene(s.describe())
    P.DescScene(rpt.AnalyticalScene().describe())


def test_shared_sets_cover_the_header_and_keep_their_near_ties_low(rpt, shared):
    """From the restatement alone: every event counter at least EVENTS_MIN over the shared sets, each pool's near-tie share at most
    POOL_SHARE_MAX (three quarters of the cap for the large class, whose cap and margin are its own), all 14 kernels aimed at."""
    from kernel_census import render_kernels      # noqa: F401  (the names below are the strict SDF and media kernels of test_gpu_strict_kernels.CASES)
    from test_gpu_strict_kernels import CASES
    events = MS.total([e for _, _, _, _, ev, _, _ in shared for e in ev])
    print("events over the shared sets:", events)
    short = {k: v for k, v in events.items() if v < EVENTS_MIN}
    assert not short, short
    pools = collections.defaultdict(lambda: [0, 0])
    for c, _, marg, _, _, _, _ in shared:
        pools[c.pool][0] += len(marg)
        pools[c.pool][1] += int((marg <= _tau(c)).sum())
    shares = {k: v[1] / v[0] for k, v in pools.items()}
    print("near-tie shares:", shares, "samples:", {k: v[0] for k, v in pools.items()})
    assert set(shares) == {"sdf", "media", "large"}
    assert shares["sdf"] <= POOL_SHARE_MAX and shares["media"] <= POOL_SHARE_MAX
    assert shares["large"] <= 0.75 * NEAR_TIE_MAX_LARGE
    aimed = {c.kernel for c, *_ in shared}
    assert aimed == {k for k in CASES if "sdf" in k or "media" in k} and len(aimed) == 14
    for c, *_ in shared:
        assert c.w <= 98 and c.h <= 73 and 240 <= len(c.items) <= 400 and all(f == 0 for _, _, f in c.items)


# ---- the f64 oracle ---------------------------------------------------------------------------------------------------------------------
FUZZ_MEDIA_SEEDS = tuple(range(24))
FUZZ_SDF_SEEDS = tuple(range(24))
FUZZ_ITEMS = 240


def fuzz_cases(rpt):
    rng = np.random.default_rng(20261020)
    out = []
    for seed in FUZZ_MEDIA_SEEDS:
        s, flags = fuzz_media_scene(rpt, seed)
        out.append(Case("media fuzz seed %d" % seed, s, 64, 48, flags, 200 + seed,
                        [(c, r, int(f)) for (c, r, _), f in zip(_pixels(rng, 64, 48, FUZZ_ITEMS), rng.integers(0, 4, FUZZ_ITEMS))], None, "small", None, None))
    for seed in FUZZ_SDF_SEEDS:
        s = fuzz_sdf_scene(rpt, seed)
        out.append(Case("sdf fuzz seed %d" % seed, s, 64, 48, 0, 300 + seed,
                        [(c, r, int(f)) for (c, r, _), f in zip(_pixels(rng, 64, 48, FUZZ_ITEMS), rng.integers(0, 4, FUZZ_ITEMS))], None, "sdf", None, None))
    return out


def test_fuzz_covers_what_it_should(rpt):
    A = rpt._abi
    media = [fuzz_media_scene(rpt, s) for s in FUZZ_MEDIA_SEEDS]
    assert len(media) >= 24
    mediums = [m.medium for s, _ in media for m in s.materials if m.medium]
    assert {m["type"] for m in mediums} == {"scatter", "absorb", "emissive", "none"}
    assert {0.0, 1e4} <= {m["density"] for m in mediums}
    assert any(m["anisotropy"] > 0.9 for m in mediums) and any(m["anisotropy"] < -0.9 for m in mediums)
    assert sum(1 for _, f in media if f & A.RPT_RENDER_RUSSIAN_ROULETTE) * 2 == len(media)
    sdf = [fuzz_sdf_scene(rpt, s) for s in FUZZ_SDF_SEEDS]
    assert len(sdf) >= 24
    assert {len(s.sdf["prims"]) for s in sdf} == set(range(1, 9))
    assert {1, 7} <= {s.sdf["max_steps"] for s in sdf}
    assert {s.any_hit_uses_max_dist for s in sdf} == {False, True}
    assert any(not s.spheres and not s.planes for s in sdf)


def _bad_f64(case, got, marg, rays, want, oracle_f64):
    bad = np.nonzero(~in_band(got, want) & (marg >= F64_TIE))[0]
    if not bad.size:
        return None
    k = int(bad[0])
    e = (case.name, case.scene.describe(), None, case.w, case.h, case.flags, case.items, case.seed)
    return "%s: %d samples outside the band with margin >= %g; first: item %s, restated %s, oracle %s, margin %.3g; %s" % (
        case.name, bad.size, F64_TIE, case.items[k], got[k].tolist(), want[k].tolist(), marg[k], first_diverging_ray(oracle_f64, e, k, rays))


def test_f64_oracle_follows_the_restatement(rpt, oracle_f64, shared):
    """Every sample agrees to the f32 rounding of the oracle's output, or took a near tie (margin < F64_TIE) on its path: the shared
    sets, 24 fuzzed media scenes and 24 fuzzed SDF scenes."""
    worst = []
    total = outside = 0
    smallest = np.inf
    for c, got, marg, rays, _, want, _ in shared:
        total += len(marg)
        outside += int((~in_band(got, want)).sum())
        smallest = min(smallest, float(marg.min()))
        worst.append(_bad_f64(c, got, marg, rays, want, oracle_f64))
    for c in fuzz_cases(rpt):
        got, marg, rays, _ = restate(c, oracle_f64)
        want = oracle_samples(oracle_f64, c)
        total += len(marg)
        outside += int((~in_band(got, want)).sum())
        smallest = min(smallest, float(marg.min()))
        worst.append(_bad_f64(c, got, marg, rays, want, oracle_f64))
    print("f64 oracle vs restatement: %d samples, %d outside the f32-rounding band, smallest margin %.3g" % (total, outside, smallest))
    assert total >= 20000
    assert not any(worst), "\n".join(w for w in worst if w)


# ---- per function --------------------------------------------------------------------------------------------------------------------
GS = (0.0, 0.0005, -0.0005, 0.001, -0.001, 0.3, -0.3, 0.9, -0.9)


def test_phase_hg_per_function(oracle_f64):
    for g in GS:
        g = P.f32(g)
        for c in np.linspace(-1.0, 1.0, 81):
            c = P.f32(c)
            assert close([MS.phase_hg(c, g)], [oracle_f64.phase_hg(c, g)]), (g, c)


def test_sample_hg_per_function(oracle_f64):
    rng = np.random.default_rng(41)
    z0 = np.float32(0.999)
    vs = []
    for z in (z0, np.nextafter(z0, np.float32(0)), np.nextafter(z0, np.float32(1)), np.float32(1.0), np.float32(-1.0), -z0):      # the onb's switch
        vs.append(np.array([np.sqrt(max(0.0, 1.0 - float(z) ** 2)), 0.0, z], dtype=np.float32))
    for _ in range(40):
        v = rng.normal(size=3)
        vs.append((v / np.linalg.norm(v)).astype(np.float32))
    r2s = [0.0, float(np.float32(1.0) - np.float32(2.0 ** -24))] + [float(np.float32(x)) for x in rng.uniform(size=6)]
    for g in GS:
        g = P.f32(g)
        for v in vs:
            for r2 in r2s:
                r1 = float(np.float32(rng.uniform()))
                mine = MS.sample_hg(tuple(float(x) for x in v), g, r1, r2)
                assert close(mine, oracle_f64.sample_hg(v, g, r1, r2)), (g, v, r1, r2)


def _sdf_alone(rpt, n_prims, k, rng, **over):
    A = rpt._abi
    prims = []
    for i in range(n_prims):
        c = tuple(rng.uniform(-1.2, 1.2, 3) * (1, 0.5, 1))
        if i % 2 == 0:
            prims.append((A.RPT_SDF_TORUS_Y, c, (float(rng.uniform(0.4, 1.3)), float(rng.uniform(0.08, 0.3)))))
        else:
            prims.append((A.RPT_SDF_SPHERE, c, (float(rng.uniform(0.2, 0.9)), 0.0)))
    s = rpt.Scene()
    s.materials = [rpt.Material(rgb=(0.5, 0.5, 0.5))]
    s.sdf = dict(prims=prims, material=0, smooth_k=k, max_steps=64, hit_eps=1e-3, max_t=20.0, normal_eps=1e-3)
    s.sdf.update(over)
    return s


def _sdf_points(sc, rng):
    """On each primitive's surface (to f32 rounding), at its centre (inside a sphere; on a torus's axis), along the axis, and around."""
    pts = []
    for kind, c, (p0, p1) in sc.sdf["prims"]:
        c = np.array(c)
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        if kind == MS.SDF_SPHERE:
            pts += [c + p0 * u, c + 0.5 * p0 * u, c]
        else:
            ring = np.array([u[0], 0.0, u[2]]) / np.hypot(u[0], u[2])
            pts += [c + (p0 + p1) * ring, c + p0 * ring, c, c + np.array([0.0, rng.uniform(-1, 1), 0.0])]
    pts += list(rng.uniform(-3, 3, size=(6, 3)))
    return [np.asarray(p, dtype=np.float32) for p in pts]


def test_sdf_eval_and_normal_per_function(rpt, oracle_f64):
    rng = np.random.default_rng(42)
    n = 0
    for n_prims in range(1, 9):
        for k in (0.05, 0.35, 1.0):
            s = _sdf_alone(rpt, n_prims, k, rng)
            d = s.describe()
            sc = MS.MediaSdfDescScene(d)
            for p in _sdf_points(sc, rng):
                pw = tuple(float(x) for x in p)
                assert close([sc.sdf_eval(pw)], [oracle_f64.sdf_eval(d.sdf, p)]), (n_prims, k, p)
                assert close(sc.sdf_normal(pw), oracle_f64.sdf_normal(d.sdf, p)), (n_prims, k, p)
                n += 1
    assert n > 500


def test_march_per_function(rpt, oracle_f64):
    rng = np.random.default_rng(43)
    hits = at0 = budget = short = 0
    for n_prims in (1, 2, 3, 5, 8):
        for over in (dict(), dict(max_steps=1), dict(max_steps=7), dict(max_t=0.05), dict(hit_eps=1e-2, max_t=6.0)):
            s = _sdf_alone(rpt, n_prims, 0.35, rng, **over)
            d = s.describe()
            sc = MS.MediaSdfDescScene(d)
            origins = [p for p in _sdf_points(sc, rng)] + [np.array([0.0, 0.5, 4.0], dtype=np.float32)] * 8
            for o in origins:
                t = rng.normal(size=3) * 0.6 - o.astype(np.float64)
                dr = (t / np.linalg.norm(t)).astype(np.float32)
                M = MS.Trace()
                mine = sc.march(tuple(float(x) for x in o), tuple(float(x) for x in dr), M=M)
                hit, tt = oracle_f64.sdf_march(d.sdf, o, dr)
                if M.m >= F64_TIE:
                    assert hit == (mine is not None), (n_prims, over, o, dr)
                    assert not hit or close([mine], [tt]), (n_prims, over, o, dr, mine, tt)
                hits += hit
                at0 += M.ev.get("sdf_hit_at_0", 0)
                budget += M.ev.get("sdf_steps_exhausted", 0)
                short += M.ev.get("sdf_max_t_exit", 0)
    assert hits > 50 and at0 > 20 and budget > 20 and short > 20, (hits, at0, budget, short)


def test_medium_transmittance_per_function(oracle_f64):
    rng = np.random.default_rng(44)
    for typ in (MS.MEDIUM_NONE, MS.MEDIUM_ABSORB, MS.MEDIUM_SCATTER, MS.MEDIUM_EMISSIVE):
        for density in (0.0, 0.3, 2.5, 1e4):
            for dist in (0.0, 1e-3, 0.7, 12.0, float("inf")):
                color = rng.uniform(0, 1, 3).astype(np.float32)
                md = MS.Medium(typ, P.f32(density), tuple(float(x) for x in color), 0.0)
                assert close(MS.transmittance(md, P.f32(dist)), oracle_f64.medium_transmittance(typ, density, color, dist)), (typ, density, dist)


def test_material_clamps_the_anisotropy():
    for g, want in ((1.2, P.f32(0.9)), (-2.0, -P.f32(0.9)), (0.4, 0.4), (P.f32(0.9), P.f32(0.9))):
        m = MS.Material()
        m.medium = MS.Medium(MS.MEDIUM_SCATTER, 1.0, P.ONE3, g)
        m.finalize()
        assert m.medium.g == want and m.medium.g_raw == g


# ---- teeth -----------------------------------------------------------------------------------------------------------------------------
def test_the_mutant_table_names_what_the_issue_names():
    assert set(MEDIA_MUTANTS) | set(SDF_MUTANTS) == set(MS.MUTANTS) and len(MS.MUTANTS) >= 20


@pytest.mark.parametrize("mutant", MEDIA_MUTANTS + SDF_MUTANTS)
def test_every_mutant_is_caught_on_both_legs(oracle_f64, shared, mutant):
    """A wrong restatement disagrees with the f64 oracle outside the f32-rounding band (margin >= F64_TIE) on at least TEETH_MIN samples,
    and with the f32 oracle by more than REL_CLEAN on at least TEETH_MIN clean samples — on the shared sets, the GPU leg's inputs: a
    device that computed the mutant would fail there."""
    n64 = n32 = 0
    for c, _, _, _, _, want64, want32 in shared:
        sc = MS.MediaSdfDescScene(c.scene.describe())
        if (sc.sdf is None) if mutant in SDF_MUTANTS else (not sc.media):
            continue
        got, marg, _, _ = restate(c, oracle_f64, (mutant,), TEETH_ITEMS)
        n64 += int((~in_band(got, want64[:TEETH_ITEMS]) & (marg >= F64_TIE)).sum())
        n32 += int(((rel_distance(got, want32[:TEETH_ITEMS]) > REL_CLEAN) & (marg > _tau(c))).sum())
    print("%s: %d outside the band on the f64 leg, %d clean samples beyond REL_CLEAN on the f32 leg" % (mutant, n64, n32))
    assert n64 >= TEETH_MIN and n32 >= TEETH_MIN, (mutant, n64, n32)


# ---- the f32 oracle --------------------------------------------------------------------------------------------------------------------
def test_f32_oracle_on_the_shared_sets(oracle, shared):
    """The device's twin at the device's bounds: per case every clean sample (margin > TAU; TAU_LARGE for the large class) within
    REL_CLEAN; per pool at most NEAR_TIE_MAX near ties (NEAR_TIE_MAX_LARGE).  A sample beyond REL_CLEAN took another branch than the
    restatement: the largest margin of such a sample is printed, and by the first assertion is below TAU."""
    pools = collections.defaultdict(lambda: [0, 0])
    flip = 0.0
    for c, got, marg, rays, _, _, want in shared:
        rel = rel_distance(got, want)
        tie = marg <= _tau(c)
        pools[c.pool][0] += len(rel)
        pools[c.pool][1] += int(tie.sum())
        moved = rel > REL_CLEAN
        if moved.any():
            flip = max(flip, float(marg[moved].max()))
        bad = np.nonzero(moved & ~tie)[0]
        e = (c.name, c.scene.describe(), None, c.w, c.h, c.flags, c.items, c.seed)
        assert not bad.size, "%s: %d clean samples beyond %g, first item %s: restated %s, f32 oracle %s, margin %.3g; %s" % (
            c.name, bad.size, REL_CLEAN, c.items[bad[0]], got[bad[0]].tolist(), want[bad[0]].tolist(), marg[bad[0]],
            first_diverging_ray(oracle, e, int(bad[0]), rays))
        print("%s: %d samples, %.1f %% near-tie, largest clean relative distance %.3g" % (c.name, len(rel), 100 * tie.mean(),
                                                                                          rel[~tie].max() if (~tie).any() else 0.0))
    print("largest margin of a sample that took another branch: %.3g" % flip)
    for pool, (n, near) in pools.items():
        assert near <= (NEAR_TIE_MAX_LARGE if pool == "large" else NEAR_TIE_MAX) * n, (pool, near, n)
