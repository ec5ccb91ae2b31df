"""The composed mesh kernel forms held to ONE float64 restatement of one pixel-sample with every feature active
(tests/mesh_compose_f64.py: ComposedMeshDescScene and ComposedPath, written from include/rpt.h's sections "mesh lights" to "mesh
normal maps" over the same functions the single-feature restatements call).  The single-feature files compare each feature on its
simplest base; the forms below run while their features interact — a lamp next to a sampled sky, holes in front of both, a bent smooth
normal over a flat-normal light sampler — and had only identity cases and self-consistency behind them.

Eight cases on scenes.mesh_light_scene(sphere_light=True) at the reference's four bounces (82 triangles: mesh 0 the icosphere, mesh 1
the lamp quad).  Textures on both meshes throughout, over scenes.spherical_uvs about each mesh's centre: mesh 0 a 5 x 3 BILINEAR /
REPEAT two-colour checker with its UVs stretched to [-1, 2] (so the wrap matters, for the mask and the map as well), mesh 1 a 4 x 4
NEAREST / CLAMP one; mesh 0 SMOOTH, mesh 1 ON.  The sky is scenes.mesh_env_scene(16)'s, SAMPLED; the mask
test_gpu_mesh_cutout_f64's 4 x 2 checker of single texels, on mesh 0 only (a light cannot carry one); the map
scenes.mesh_normal_map_scene()'s 32 x 32 bump map at strength 1, BILINEAR on mesh 0 and NEAREST + FLIP_GREEN on mesh 1.

  case  on top of A                 bits 25-31 (rpt_debug_kernel_choice)      kernel (kernel_census.mesh_kernel_of)
  A     —                           MESH SMOOTH LIGHT TEX                     meshtex_light_regen_kernel
  B     environment                 ... ENV                                   meshenv_regen_kernel, textures bound
  C     cutout on 0                 ... CUT                                   meshcut_regen_kernel, the light tables bound (mesh_args.h)
  D     cutout on 0, environment    ... ENV CUT                               meshcut_env_regen_kernel
  E     maps                        ... NRM                                   meshnrm_regen_kernel, light branch, smooth N
  F     maps, environment           ... ENV NRM                               meshnrm_env_regen_kernel
  G     maps, cutout on 0           ... CUT NRM                               meshnrm_cut_regen_kernel
  H     all three                   every bit 25-31                           meshnrm_cut_env_regen_kernel

Draws: 64 x 48, 200 random pixels x 2 seeds per case, each sample a one-sample render into a fresh DeviceColorBuffer, compared through
test_gpu_path_f64.Tally with test_path_f64's TAU / REL_CLEAN / NEAR_TIE_MAX: this file has no tolerance of its own.  The comparison
needs an MI355X; everything else here runs on the CPU.

The near-tie condition (test_the_near_tie_count_of_the_restatement, per case: the cap keeps the comparison from hiding a failure, so
it is a condition, not a measurement).  The restatement alone, for exactly the GPU test's draws, samples of 400 at or below TAU /
samples with radiance — BELOW_TAU and LIT, counted again on every run:
  A 24 / 223    B 12 / 395    C 17 / 240    D 11 / 398    E 18 / 216    F 15 / 394    G 12 / 236    H 12 / 391
(6.0 %, 3.0 %, 4.25 %, 2.75 %, 4.5 %, 3.75 %, 3.0 %, 3.0 %):
every case under the cap of 48 (12 %), every case with far more than a quarter of its samples lit.  The single-feature counts on this
scene family are 1.4 % (environment) and 9.0 % (lights); the mask's and the NEAREST texels' borders add to them.  No case's inputs
had to be changed to stay under the cap.

Mutations (test_the_restatement_sees_the_interaction): six faults, each of which a device could have in exactly one interaction,
planted in the restatement by a keyword argument; clean samples moved beyond REL_CLEAN on the case that exercises it, over a grid of
552 pixels on the object, the floor and the lamp at seed 7 — MOVED, counted again on every run, each above 10:
  light_uses_shading_normal      case E   89   the mesh-light sampler and the hit weight use the shading normal (smooth, bent)
  no_cut_in_any_hit              case C   37   the cut test is applied in closest_hit but not in any_hit
  bend_from_flat                 case E   48   the bend starts from the flat normal on a SMOOTH mesh
  map_wrap_clamp                 case E   53   the map is looked up with CLAMP instead of the texture's REPEAT
  no_texture_under_env           case B   97   the texture is dropped under the environment form
  n_without_on_meshes_under_env  case B  292   N leaves out the ON mesh while an environment is SAMPLED
The lamp keeps its size: none of the six needed a wider one or other draws.
test_the_composed_restatement_reduces_to_the_single_feature_ones closes the other side: with one branch's features only, the composed
classes give the single-feature restatements' samples and margins bit for bit.

The restatement's time on the CPU, measured: 1.9 ms per sample — 0.75 s for a case's 400 draws, 2 s for a mutation's two passes over
the grid, 18 s for this file's CPU tests together.  On an MI355X each of the eight comparisons takes 2.3 to 2.7 s, the restatement
included; the largest clean relative distance seen was 1.4e-4 (case E), next to REL_CLEAN = 5e-2.

The first 150 clean samples of every case are also held to their own f32 tolerance (tests/f32_spread.py: Tally.add's spreads; the
mesh kernels have no f32 twin, and REL_CLEAN is hundreds of times what they have ever shown), computed once per case beside
_restated (1.7 to 2.9 s of CPU time; the case's two plain passes take 0.75 s).  test_the_spreads_of_the_restatement holds the
conditions on the CPU (at least 100 clean samples with a spread, at most 5 % with a tolerance above 1e-3: 0 % in every case),
test_the_spreads_see_a_subtle_fault three faults that stay within REL_CLEAN on every clean sample and leave their own tolerance on
38 (the mesh light's pdf x 0.98), 119 (the environment's pdf from the neighbouring texel row) and 16 (a BILINEAR lookup 1/32 of a
texel off).  The largest z seen on an MI355X, per case: A 0.94, B 1.34, C 1.58, D 1.46, E 1.47, F 1.37, G 1.84, H 1.68, next to
Z_MAX = 8.3; the medians 0.13 to 0.32, next to Z_MEDIAN = 1.4.  Measurements, not bounds."""
import ctypes as C
import functools

import numpy as np
import pytest

import f32_spread as S
import mesh_compose_f64 as MC
from kernel_census import (CUT_BIT, ENV_BIT, LIGHT_BIT, MESH_BIT, MESH_FORM_BITS, MESH_RENDER_KERNELS, NRM_BIT, SMOOTH_BIT, TEX_BIT,
                           mesh_kernel_of)
from mesh_compose_f64 import ComposedMeshDescScene, ComposedPath, sample_pixels
from test_gpu_mesh_cutout_f64 import scene_masks
from test_gpu_mesh_env_f64 import ENV_SIZE
from test_gpu_mesh_normal_map_f64 import bump_map
from test_gpu_mesh_texture_f64 import GAMMA
from test_gpu_path_f64 import Tally
from test_path_f64 import NEAR_TIE_MAX, REL_CLEAN, TAU, rel_distance

W, H = 64, 48
BASE = MESH_BIT | SMOOTH_BIT | LIGHT_BIT | TEX_BIT
# case -> (environment, cutout on mesh 0, maps, the exact bits 25-31, the kernel)
CASES = {
    "A": (False, False, False, BASE, "meshtex_light_regen_kernel"),
    "B": (True, False, False, BASE | ENV_BIT, "meshenv_regen_kernel"),
    "C": (False, True, False, BASE | CUT_BIT, "meshcut_regen_kernel"),
    "D": (True, True, False, BASE | ENV_BIT | CUT_BIT, "meshcut_env_regen_kernel"),
    "E": (False, False, True, BASE | NRM_BIT, "meshnrm_regen_kernel"),
    "F": (True, False, True, BASE | ENV_BIT | NRM_BIT, "meshnrm_env_regen_kernel"),
    "G": (False, True, True, BASE | CUT_BIT | NRM_BIT, "meshnrm_cut_regen_kernel"),
    "H": (True, True, True, MESH_FORM_BITS, "meshnrm_cut_env_regen_kernel"),
}
# Counted on the CPU (test_the_near_tie_count_of_the_restatement prints the figures): of each case's 400 samples, those at or below
# TAU, and those that carry radiance.
BELOW_TAU = {"A": 24, "B": 12, "C": 17, "D": 11, "E": 18, "F": 15, "G": 12, "H": 12}
LIT = {"A": 223, "B": 395, "C": 240, "D": 398, "E": 216, "F": 394, "G": 236, "H": 391}
# fault -> (the case that exercises it, where it is planted, clean samples moved beyond REL_CLEAN)
MUTATIONS = {
    "light_uses_shading_normal": ("E", "path", 89),
    "no_cut_in_any_hit": ("C", "scene", 37),
    "bend_from_flat": ("E", "scene", 48),
    "map_wrap_clamp": ("E", "scene", 53),
    "no_texture_under_env": ("B", "scene", 97),
    "n_without_on_meshes_under_env": ("B", "path", 292),
}
GRID = [(c, r) for r in range(2, 48, 2) for c in range(8, 56, 2)]  # the lamp, the object and the floor


def object_pixels(sc, mesh=0):
    """The pixels of GRID whose centre sees mesh `mesh` of the restated scene `sc` first: where a fault on that mesh shows."""
    import pt_f64 as P
    out = []
    for c, r in GRID:
        o, d = P.gen_ray(sc.cam, (float(c) / W, 1.0 - (float(H) - float(H - 1 - r)) / H), (0.5, 0.5), float(W), float(H))
        st = P.State()
        st.material = P.Material(1.5)
        if sc.closest_hit(o, d, st, P.LightSampleRec(), frozenset(), P.Margin()) and sc.won is not None and sc.tri_mesh[sc.won] == mesh:
            out.append((c, r))
    return out


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _scene():
    from rust_pathtracer_amd import scenes
    s = scenes.mesh_light_scene(sphere_light=True)
    s.max_depth = 4
    return s


def inputs(scene, case):
    """-> the arguments of the set calls, which are ComposedMeshDescScene's as well: dict(smooth=, on=, textures=, cutouts=,
    normal_maps=, environment=), the last three None where the case leaves them out."""
    from rust_pathtracer_amd import scenes
    environment, cutout, maps = CASES[case][:3]
    uvs = []
    for m, (v, _, _) in enumerate(scene.meshes):
        v = np.asarray(v, np.float32)
        uvs.append(scenes.spherical_uvs(v, 0.5 * (v.min(0).astype(np.float64) + v.max(0))))
    uvs[0] = (uvs[0] * np.float32(3.0) - np.float32(1.0)).astype(np.float32)      # [-1, 2]: the wrap matters
    textures = {0: dict(uvs=uvs[0], texels=scenes.checker_texture(5, 3, (250, 240, 230), (40, 90, 160), cells=5),
                        wrap="repeat", filter="bilinear", gamma=GAMMA),
                1: dict(uvs=uvs[1], texels=scenes.checker_texture(4, 4, (255, 200, 60), (70, 30, 120), cells=4),
                        wrap="clamp", filter="nearest", gamma=GAMMA)}
    return dict(smooth=(0,), on=(1,), textures=textures,
                cutouts={0: scene_masks(scene)[0]} if cutout else None,
                normal_maps={0: dict(texels=bump_map(), filter="bilinear", strength=1.0),
                             1: dict(texels=bump_map(), filter="nearest", flip_green=True, strength=1.0)} if maps else None,
                environment=dict(image=scenes.mesh_env_scene(ENV_SIZE)[1], scale=1.0, sampled=True) if environment else None)


def _draws(case):
    """[(seed, pixels)]: 200 random pixels at each of two seeds, the case's own."""
    k = sorted(CASES).index(case)
    rng = np.random.default_rng([38, k])
    return [(110 + 10 * k + seed, list(zip(rng.integers(0, W, 200).tolist(), rng.integers(0, H, 200).tolist()))) for seed in (1, 2)]


@functools.lru_cache(maxsize=None)
def _restated(oracle, case):
    """The restatement of the case's draws, computed once for every test that needs it: [(seed, pixels, radiance, margins)]."""
    s = _scene()
    path = ComposedPath(ComposedMeshDescScene(s.describe(), s, **inputs(s, case)))
    return [(seed, pixels) + sample_pixels(path, oracle, seed, pixels, W, H) for seed, pixels in _draws(case)]


@functools.lru_cache(maxsize=None)
def _spreads(oracle, case):
    """The f32 spreads (tests/f32_spread.py) of the case's first 150 clean samples, computed once beside _restated for the CPU and
    the GPU leg: ([spreads per seed, NaN where there is none], CPU seconds)."""
    s = _scene()
    path = ComposedPath(ComposedMeshDescScene(s.describe(), s, **inputs(s, case)))
    return S.spreads_of_draws(path, oracle, _restated(oracle, case), W, H)


def _one_composed_sample(rpt, torch, scene, args, seed):
    """A one-sample render under the case's set calls into a fresh buffer -> (frame, kernel choice)."""
    t = rpt.Tracer(scene, device=0, seed=seed)
    try:
        t.set_mesh_textures(args["textures"])
        t.set_mesh_shading({m: "smooth" for m in args["smooth"]})
        t.set_mesh_lights({m: True for m in args["on"]})
        if args["cutouts"]:
            t.set_mesh_cutouts(args["cutouts"])
        if args["normal_maps"]:
            t.set_mesh_normal_maps(args["normal_maps"])
        if args["environment"]:
            t.set_environment(**args["environment"])
        buf = rpt.DeviceColorBuffer(W, H)
        t.render_n(buf, 1)
        torch.cuda.synchronize()
        choice = C.c_uint32()
        assert rpt.lib().rpt_debug_kernel_choice(t._h, C.byref(choice)) == 0
        return buf.pixels.cpu().numpy(), choice.value
    finally:
        t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_composed_mesh_renders_against_the_restatement(rpt, oracle, torch_cuda, case):
    bits, kernel = CASES[case][3:]
    s = _scene()
    args = inputs(s, case)
    t = Tally(TAU, NEAR_TIE_MAX)
    spreads, seconds = _spreads(oracle, case)
    print("case %s: the spreads took %.2f s of CPU time" % (case, seconds))
    for (seed, pixels, restated, margins), spread in zip(_restated(oracle, case), spreads):
        frame, choice = _one_composed_sample(rpt, torch_cuda, s, args, seed)
        assert choice & MESH_FORM_BITS == bits, "case %s: bits 25-31 are 0x%x, not 0x%x" % (case, choice & MESH_FORM_BITS, bits)
        assert mesh_kernel_of(choice) == kernel
        t.ran.add(mesh_kernel_of(choice))
        print("case %s (seed %d): %d of %d samples below TAU" % (case, seed, int((margins <= TAU).sum()), len(margins)))
        t.add("case %s (seed %d, %s)" % (case, seed, kernel), frame, restated, margins, pixels, spreads=spread)
    t.check("case %s" % case)
    assert t.n == 400 and t.ran == {kernel}


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_near_tie_count_of_the_restatement(rpt, oracle, case):
    """The restatement alone, for exactly the draws of the GPU comparison, case by case: no more than the project's 12 % of the
    samples lie at or below TAU, more than a quarter carry radiance, and both counts are the ones in this file's docstring."""
    below = total = lit = 0
    for _, _, restated, margins in _restated(oracle, case):
        below += int((margins <= TAU).sum())
        total += len(margins)
        lit += int((restated.max(axis=1) > 0).sum())
    print("case %s: %d of %d samples below TAU (%.2f %%), %d with radiance" % (case, below, total, 100.0 * below / total, lit))
    assert total == 400 and below <= NEAR_TIE_MAX * total and lit > total // 4
    assert (below, lit) == (BELOW_TAU[case], LIT[case])


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_spreads_of_the_restatement(rpt, oracle, case):
    """The conditions of the comparison with spreads, on the restatement alone: at least 100 clean samples of the case have a spread,
    and at most 5 % of them a tolerance above 1e-3 — for the others the bound is at least 50 times sharper than REL_CLEAN."""
    spreads, seconds = _spreads(oracle, case)
    S.case_conditions("case %s" % case, _restated(oracle, case), spreads, seconds)


def _low_contrast_texture(args):
    """Mesh 0's BILINEAR checker with two colours a tenth apart: a lookup 1/32 of a texel off is wrong by well under a percent."""
    from rust_pathtracer_amd import scenes
    args["textures"][0]["texels"] = scenes.checker_texture(5, 3, (200, 190, 180), (180, 185, 190), cells=5)


def _smooth_sky(args):
    """A sky that brightens by 2 % from one texel row to the next, in place of the sun's few texels: the neighbouring row's pdf
    is wrong by 2 %."""
    rows = (1.0 + 0.02 * np.arange(ENV_SIZE))[:, None, None]
    args["environment"]["image"] = np.ascontiguousarray(rows * np.array([0.5, 0.6, 0.8]) * np.ones((ENV_SIZE, ENV_SIZE, 1)), np.float32)


# fault -> (the case, what changes its inputs or None, the path's keyword arguments, the scene's attributes, mesh_compose_f64's values)
SUBTLE = {
    "mesh light pdf x 0.98": ("A", None, dict(mesh_light_pdf_scale=0.98), {}, {}),
    "environment pdf from the neighbouring texel row": ("B", _smooth_sky, {}, dict(env_pdf_from_next_row=True), {}),
    "bilinear lookup shifted by 1/32 texel": ("A", _low_contrast_texture, {}, {}, dict(BILINEAR_SHIFT=1.0 / 32.0)),
}


@pytest.mark.parametrize("fault", sorted(SUBTLE))
def test_the_spreads_see_a_subtle_fault(rpt, oracle, monkeypatch, fault):
    """A restatement that is wrong in the second or third digit, rounded to f32, stands in for a device: every clean sample stays
    within REL_CLEAN, so the comparison without spreads passes it; held to its samples' own tolerances it fails on at least 10.
    Where the case's own inputs would make the fault a gross one (a checker of high contrast, a sky with a sun) the input is
    replaced by a gentle one, and the restatement and its spreads are computed for it here."""
    case, change, path_args, scene_attrs, module_values = SUBTLE[fault]
    s = _scene()
    args = inputs(s, case)
    if change is not None:
        change(args)
    good = ComposedPath(ComposedMeshDescScene(s.describe(), s, **args))
    sc = ComposedMeshDescScene(s.describe(), s, **args)
    for k, v in scene_attrs.items():
        setattr(sc, k, v)
    faulty = ComposedPath(sc, **path_args)
    if change is not None or module_values:
        draws, entries = _draws(case)[:1], None
        entries = [(seed, pixels) + sample_pixels(good, oracle, seed, pixels, W, H) for seed, pixels in draws]
        spreads, _ = S.spreads_of_draws(good, oracle, entries, W, H, count=None)
    else:
        entries, (spreads, _) = _restated(oracle, case), _spreads(oracle, case)
    for k, v in module_values.items():                                # (from here on: the restatement and its spreads are made)
        monkeypatch.setattr(MC, k, v)
    moved = [sample_pixels(faulty, oracle, seed, pixels, W, H) for seed, pixels, _, _ in entries]
    S.teeth("%s (case %s)" % (fault, case), entries, spreads, moved)


@pytest.mark.parametrize("fault", sorted(MUTATIONS))
def test_the_restatement_sees_the_interaction(rpt, oracle, fault):
    """A restatement with one interaction wrong moves more than 10 clean samples beyond REL_CLEAN on the case that exercises it: a
    device with that fault would fail the comparison above."""
    case, where, count = MUTATIONS[fault]
    s = _scene()
    args = inputs(s, case)
    base, marg = sample_pixels(ComposedPath(ComposedMeshDescScene(s.describe(), s, **args)), oracle, 7, GRID, W, H)
    if where == "scene":
        mutant = ComposedPath(ComposedMeshDescScene(s.describe(), s, **args, **{fault: True}))
    else:
        mutant = ComposedPath(ComposedMeshDescScene(s.describe(), s, **args), **{fault: True})
    moved, marg2 = sample_pixels(mutant, oracle, 7, GRID, W, H)
    far = (rel_distance(np.nan_to_num(moved), np.nan_to_num(base)) > REL_CLEAN) & (marg > TAU) & (marg2 > TAU)
    print("%s (case %s): %d clean samples beyond REL_CLEAN" % (fault, case, int(far.sum())))
    assert far.sum() > 10, fault
    assert int(far.sum()) == count


def test_the_composed_restatement_reduces_to_the_single_feature_ones(rpt, oracle):
    """With one branch's features only, ComposedMeshDescScene and ComposedPath give the single-feature restatements' samples and
    margins exactly: the lamp, the spherical light and the sky as test_gpu_mesh_env_f64 has them, the textured cutout scene of
    test_gpu_mesh_cutout_f64 and the normal-mapped one of test_gpu_mesh_normal_map_f64.  (The other direction — what the
    composition adds — is what the mutations above are for.)"""
    import pt_f64 as P
    import test_gpu_mesh_env_f64 as E
    from test_gpu_mesh_cutout_f64 import CutMeshDescScene
    from test_gpu_mesh_f64 import _scenes as mesh_scenes
    from test_gpu_mesh_normal_map_f64 import NrmMeshDescScene
    from test_gpu_mesh_texture_f64 import MODES, scene_textures
    rng = np.random.default_rng(39)
    pixels = list(zip(rng.integers(0, W, 48).tolist(), rng.integers(0, H, 48).tolist()))
    _, s, smooth, on, image = E._scenes()[1]
    want = E.sample_many(E.EnvMeshDescScene(s.describe(), s, smooth, on, image), oracle, 5, pixels, W, H)
    got = sample_pixels(ComposedPath(ComposedMeshDescScene(s.describe(), s, smooth, on, environment=dict(image=image))), oracle, 5, pixels, W, H)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and want[0].any()
    for k, single, extra in ((0, CutMeshDescScene, lambda s: dict(cutouts=scene_masks(s))),
                             (1, NrmMeshDescScene, lambda s: dict(normal_maps={m: bump_map() for m in range(len(s.meshes))}))):
        s = mesh_scenes()[k][1]
        wrap, filt = MODES[k]
        textures = {m: dict(uvs=uv, texels=img, wrap=("repeat", "clamp")[wrap], filter=("nearest", "bilinear")[filt], gamma=GAMMA)
                    for m, (uv, img) in scene_textures(s).items()}
        want, margins, _ = P.sample_many(single(s.describe(), s, wrap, filt), oracle, 5, [(c, r, 0) for c, r in pixels[:24]], W, H)
        got = sample_pixels(ComposedPath(ComposedMeshDescScene(s.describe(), s, textures=textures, **extra(s))), oracle, 5, pixels[:24], W, H)
        assert np.array_equal(got[0], want, equal_nan=True) and np.array_equal(got[1], margins) and np.nan_to_num(want).any()


def test_every_mesh_kernel_name_is_in_a_code_object():
    """kernel_census.mesh_kernel_of names only kernels that the test_mesh_*_host.py files read from the libraries' code objects, over
    every combination of bits 26-31, and reaches each of the twelve mesh forms (csrc/mesh_args.h, MeshForm)."""
    from test_mesh_cutout_host import CUT_KERNELS
    from test_mesh_env_host import ENV_KERNELS
    from test_mesh_host import MESH_KERNELS
    from test_mesh_light_host import LIGHT_KERNELS
    from test_mesh_normal_map_host import NRM_KERNELS
    from test_mesh_smooth_host import SMOOTH_KERNELS
    from test_mesh_texture_host import TEX_KERNELS
    known = set(MESH_KERNELS + SMOOTH_KERNELS + LIGHT_KERNELS + TEX_KERNELS + ENV_KERNELS + CUT_KERNELS + NRM_KERNELS)
    seen = {mesh_kernel_of(MESH_BIT | (k << 26)) for k in range(64)}
    assert seen <= known, sorted(seen - known)
    assert seen == set(MESH_RENDER_KERNELS) and len(MESH_RENDER_KERNELS) == 12
    assert {mesh_kernel_of(bits) for _, _, _, bits, _ in CASES.values()} == {kernel for *_, kernel in CASES.values()}
    with pytest.raises(AssertionError):
        mesh_kernel_of(SMOOTH_BIT)                                    # not a mesh scene's launch
