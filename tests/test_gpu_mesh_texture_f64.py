"""Textured mesh renders held to tests/pt_f64.py, the float64 restatement of one pixel-sample (include/rpt.h, "mesh textures"):
TexMeshDescScene is test_gpu_mesh_smooth_f64.SmoothMeshDescScene — shading flat, as the scenes here are — with the winning
triangle's rgb restated in float64: the decode by P.powf with the end-point rule, the UV interpolation with the triangle test's u
and v, the wrap and the filter.  One-sample renders are compared sample by sample with test_path_f64's TAU / REL_CLEAN /
NEAR_TIE_MAX over test_gpu_mesh_f64's own draws, 200 pixels x 3 seeds x 2 scenes (needs an MI355X).  Every mesh carries a 5 x 3
two-colour texture over spherical UVs; the first scene is BILINEAR / REPEAT, the second NEAREST / CLAMP.  The statements themselves are
functions of tests/mesh_compose_f64.py, which the composed restatement (tests/test_gpu_mesh_compose_f64.py) calls as well.

Margins.  BILINEAR adds none: the filter is continuous across texels and across the wrap, so floorf's choice moves no value.
NEAREST records the distance of x*W (and y*H) to the next integer through M.of(., 1.0), where the coordinate is not clamped.

The restatement alone, on the CPU, for exactly these draws (test_the_near_tie_count_of_the_restatement counts it again):
128 of 1 200 samples lie below TAU (10.7 %), under the 12 % cap of 144; the flat untextured restatement has 127.
Mutation (test_the_restatement_sees_the_texture, the first scene's first 200 draws): a restatement that ignores the texture moves
69 clean samples beyond REL_CLEAN, one that swaps s and t 57.

The first 150 clean samples of each scene are also held to their own f32 tolerance (tests/f32_spread.py, through Tally.add's
spreads), computed once per scene (CASES) for the CPU and the GPU leg; this file has no tolerance of its own.  The textured rgb,
which the device multiplies in f32, carries noise (patch).  On the CPU (test_the_spreads_of_the_restatement): scene 0 median spread
4.0e-7, largest 1.9e-4, 8.9 s of CPU time; scene 1 median 5.2e-7, largest 2.6e-4, 5.0 s; 0.67 % with a tolerance above 1e-3 in
each.  Teeth (test_the_spreads_see_a_shifted_lookup): a BILINEAR lookup 1/32 of a texel off, under a checker whose colours are a
tenth apart, leaves REL_CLEAN on no clean sample of scene 0's first 200 draws and its own tolerance on 55.  On an MI355X: largest z
2.0 and 1.80 next to Z_MAX = 8.3, median z 0.33 and 0.34 next to Z_MEDIAN = 1.4, 7.2 s of wall time for the GPU
test.  Measurements, not bounds."""
import ctypes as C

import numpy as np
import pytest

import f32_spread as S
import mesh_compose_f64 as MC
import pt_f64 as P
from kernel_census import mesh_kernel_of
from mesh_compose_f64 import BILINEAR, CLAMP, NEAREST, REPEAT
from test_gpu_mesh_f64 import _scenes
from test_gpu_mesh_smooth_f64 import SmoothMeshDescScene, _draws
from test_gpu_path_f64 import Tally
from test_path_f64 import NEAR_TIE_MAX, REL_CLEAN, TAU, rel_distance

TEX_BIT = 1 << 28
GAMMA = 2.2
MODES = ((REPEAT, BILINEAR), (CLAMP, NEAREST))                      # per scene of test_gpu_mesh_f64._scenes()
NEAR_TIE_COUNT = 128                                                # of 1 200, counted on the CPU
MUT_IGNORE, MUT_SWAP = 69, 57                                       # of the 200 draws of the mutation case


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def scene_textures(scene):
    """-> {mesh: (uvs [n, 2] f32, RGBA8 [3, 5, 4])}: spherical UVs about each mesh's centre — the second mesh's stretched to
    [-1, 2], so that the wrap matters — and a two-colour 5 x 3 checker each."""
    from rust_pathtracer_amd import scenes
    out = {}
    for m, (v, _, _) in enumerate(scene.meshes):
        v = np.asarray(v, np.float32)
        uv = scenes.spherical_uvs(v, 0.5 * (v.min(0).astype(np.float64) + v.max(0)))
        if m % 2:
            uv = (uv * np.float32(3.0) - np.float32(1.0)).astype(np.float32)
        colours = ((250, 240, 230), (40, 90, 160)) if m % 2 == 0 else ((255, 200, 60), (70, 30, 120))
        out[m] = (uv, scenes.checker_texture(5, 3, colours[0], colours[1], cells=5))
    return out


decode_f64 = MC.decode_texture_f64                                   # include/rpt.h's decode in float64: [h, w, 3]


class TexMeshDescScene(SmoothMeshDescScene):
    """Every mesh FLAT and textured.  fault: None, "ignore" (the texture is not applied) or "swap" (s and t change places)."""

    def __init__(self, desc, scene, wrap, filt, fault=None):
        super().__init__(desc, scene)
        self.wrap, self.filt, self.fault = wrap, filt, fault
        tex = scene_textures(scene)
        self.uv = np.concatenate([tex[m][0] for m in range(len(scene.meshes))]).astype(np.float64)
        self.texels = [decode_f64(tex[m][1], GAMMA) for m in range(len(scene.meshes))]
        self.tri_mesh = np.concatenate([np.full(len(t), m) for m, (_, t, _) in enumerate(scene.meshes)])
        self._won = None

    def triangle_normal(self, k, o, d, M):
        self._won = (k, np.array(o), np.array(d))
        return MC.flat_normal(self, k)

    def patch(self, m, d, hp, mat, mut, M):
        super().patch(m, d, hp, mat, mut, M)
        won, self._won = self._won, None                             # (set by the triangle that has just won, and by nothing else)
        if won is not None and self.fault != "ignore":
            tex = self.lookup(*won, M)
            mat.rgb = tuple(P.noisy(float(c) * float(x)) for c, x in zip(mat.rgb, tex))

    def lookup(self, k, o, d, M):
        s, t = MC.interp_uv(self, k, *self.barycentrics(k, o, d))
        if self.fault == "swap":
            s, t = t, s
        return MC.tex_lookup(self.texels[int(self.tri_mesh[k])], s, t, self.wrap, self.filt, M)


def _path(k):
    s = _scenes()[k][1]
    return P.Path(TexMeshDescScene(s.describe(), s, *MODES[k]))


# per scene: the restated draws and the f32 spreads of their first 150 clean samples, once for the CPU and the GPU leg
CASES = S.Cases(_path, lambda k: [(seed, pixels) for j, _, _, seed, pixels, _, _ in _draws() if j == k])


def _one_textured_sample(rpt, torch, scene, wrap, filt, w, h, seed):
    """A one-sample render with every mesh textured into a fresh buffer -> (frame, kernel choice)."""
    t = rpt.Tracer(scene, device=0, seed=seed)
    try:
        t.set_mesh_textures({m: dict(uvs=uv, texels=img, wrap=("repeat", "clamp")[wrap], filter=("nearest", "bilinear")[filt], gamma=GAMMA)
                             for m, (uv, img) in scene_textures(scene).items()})
        buf = rpt.DeviceColorBuffer(w, h)
        t.render_n(buf, 1)
        torch.cuda.synchronize()
        choice = C.c_uint32()
        assert rpt.lib().rpt_debug_kernel_choice(t._h, C.byref(choice)) == 0
        return buf.pixels.cpu().numpy(), choice.value
    finally:
        t.close()


@pytest.mark.gpu
def test_textured_mesh_renders_against_the_restatement(rpt, oracle, torch_cuda):
    t = Tally(TAU, NEAR_TIE_MAX)
    per = None
    for n, (k, what, s, seed, pixels, w, h) in enumerate(_draws()):
        wrap, filt = MODES[k]
        if n % 3 == 0:
            print("%s: the spreads took %.2f s of CPU time" % (what, CASES.spreads(oracle, k)[1]))
        frame, choice = _one_textured_sample(rpt, torch_cuda, s, wrap, filt, w, h, seed)
        assert choice & (1 << 25) and choice & TEX_BIT, "the textured mesh kernel ran"
        assert mesh_kernel_of(choice) == "meshtex_regen_kernel"
        t.ran.add(mesh_kernel_of(choice))
        seed2, pixels2, restated, margins = CASES.restated(oracle, k)[n % 3]
        assert (seed2, pixels2) == (seed, pixels)
        print("%s (seed %d): %d of %d samples below TAU" % (what, seed, int((margins <= TAU).sum()), len(margins)))
        t.add("%s, textured (seed %d)" % (what, seed), frame, restated, margins, pixels, spreads=CASES.spreads(oracle, k)[0][n % 3])
        per = per if n % 3 else Tally(TAU, NEAR_TIE_MAX)
        per.add("%s, textured (seed %d)" % (what, seed), frame, restated, margins, pixels, spreads=CASES.spreads(oracle, k)[0][n % 3])
        if n % 3 == 2:
            print("%s: %s" % (what, per.held.line()))
    t.check("textured mesh scenes")
    assert t.n == 2 * 3 * 200


def test_the_near_tie_count_of_the_restatement(rpt, oracle):
    """The restatement alone, for exactly the draws of the GPU comparison: the count in this file's docstring, under the cap."""
    near = n = 0
    refs = {}
    for k, what, s, seed, pixels, w, h in _draws():
        if k not in refs:
            refs[k] = TexMeshDescScene(s.describe(), s, *MODES[k])
        _, margins, _ = P.sample_many(refs[k], oracle, seed, [(c, r, 0) for c, r in pixels], w, h)
        near += int((margins <= TAU).sum())
        n += len(margins)
    print("%d of %d samples below TAU" % (near, n))
    assert n == 1200 and near == NEAR_TIE_COUNT and near <= NEAR_TIE_MAX * n


def test_the_restatement_sees_the_texture(rpt, oracle):
    """Two planted faults, each of which a device could have: the texture ignored, s and t swapped.  Each moves clean samples beyond
    REL_CLEAN, so the comparison above would catch it."""
    k, what, s, seed, pixels, w, h = next(iter(_draws()))
    items = [(c, r, 0) for c, r in pixels]
    base, marg, _ = P.sample_many(TexMeshDescScene(s.describe(), s, *MODES[k]), oracle, seed, items, w, h)
    moved = {}
    for fault in ("ignore", "swap"):
        other, marg2, _ = P.sample_many(TexMeshDescScene(s.describe(), s, *MODES[k], fault=fault), oracle, seed, items, w, h)
        clean = (marg > TAU) & (marg2 > TAU)
        moved[fault] = int((rel_distance(np.nan_to_num(other), np.nan_to_num(base))[clean] > REL_CLEAN).sum())
    print("clean samples moved beyond REL_CLEAN:", moved)
    assert moved == {"ignore": MUT_IGNORE, "swap": MUT_SWAP} and min(moved.values()) > 10


@pytest.mark.parametrize("k", (0, 1))
def test_the_spreads_of_the_restatement(rpt, oracle, k):
    """The conditions of the comparison with spreads, on the restatement alone: at least 100 clean samples of the scene have a
    spread, and at most 5 % of them a tolerance above 1e-3."""
    CASES.conditions(oracle, _scenes()[k][0] + ", textured", k)


def test_the_spreads_see_a_shifted_lookup(rpt, oracle, monkeypatch):
    """A BILINEAR lookup 1/32 of a texel off, rounded to f32, as a device's samples over the first scene's first draws: no clean
    sample leaves REL_CLEAN, at least 10 leave their own tolerance.  The scene's own checker has colours a factor six apart, which
    would make the shift a gross fault; here both meshes carry one whose two colours are a tenth apart, and the restatement and
    its spreads are computed for it."""
    from rust_pathtracer_amd import scenes
    k, what, s, seed, pixels, w, h = next(iter(_draws()))
    assert MODES[k] == (REPEAT, BILINEAR)
    gentle = decode_f64(scenes.checker_texture(5, 3, (200, 190, 180), (180, 185, 190), cells=5), GAMMA)
    good, faulty = (TexMeshDescScene(s.describe(), s, *MODES[k]) for _ in range(2))
    good.texels = faulty.texels = [gentle] * len(s.meshes)
    entries = [(seed, pixels) + MC.sample_pixels(P.Path(good), oracle, seed, pixels, w, h)]
    spreads, _ = S.spreads_of_draws(P.Path(good), oracle, entries, w, h)
    monkeypatch.setattr(MC, "BILINEAR_SHIFT", 1.0 / 32.0)            # (from here on: the restatement and its spreads are made)
    S.teeth("bilinear lookup shifted by 1/32 texel (%s)" % what, entries, spreads, [MC.sample_pixels(P.Path(faulty), oracle, seed, pixels, w, h)])
