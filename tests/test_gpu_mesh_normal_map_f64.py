"""Normal-mapped mesh renders held to tests/pt_f64.py, the float64 restatement of one pixel-sample (include/rpt.h, "mesh normal
maps"): NrmMeshDescScene is test_gpu_mesh_texture_f64.TexMeshDescScene — flat shading, every mesh textured — with the winning
triangle's normal bent in float64: the decode c(k) = max((k - 128) / 127, -1), the UV interpolation with the triangle test's u and
v, the texture's wrap, a BILINEAR lookup and the bend.  One-sample renders are compared sample by sample with test_path_f64's TAU /
REL_CLEAN / NEAR_TIE_MAX over test_gpu_mesh_f64's own draws, 200 pixels x 3 seeds x 2 scenes (needs an MI355X).  Every mesh carries
scenes.mesh_normal_map_scene()'s 32 x 32 bump map (tilts of at most about 15 degrees), BILINEAR, strength 1, over the textures of
test_gpu_mesh_texture_f64: the first scene REPEAT, the second CLAMP.  The statements themselves are
functions of tests/mesh_compose_f64.py, which the composed restatement (tests/test_gpu_mesh_compose_f64.py) calls as well.

Margins.  The BILINEAR lookup adds none: it is continuous across texels and across the wrap.  The bend records the sign of D
through M.of(D, |du1 dv2| + |du2 dv1|), the sign of dot(B, B0) through M.of(., |B0|) (B is a unit vector), and the two `l2 > 0`
guards through M.of(l2, |T0|^2) and M.of(l2, x^2 + y^2 + z^2).  The `x == 0 && y == 0` rule needs none: a zero decodes to a zero in
both, and a BILINEAR mix of texels that is zero in one is a near tie of no consequence — the bend is continuous there.

The restatement alone, on the CPU, for exactly these draws (test_the_near_tie_count_of_the_restatement counts it again):
126 of 1 200 samples lie below TAU (10.5 %), under the 12 % cap of 144; the textured restatement without maps has 128.
Mutation (test_the_restatement_sees_the_map, the first scene's first 200 draws): a restatement that ignores the map moves
56 clean samples beyond REL_CLEAN, one that swaps T and B 55.

The first 150 clean samples of each scene are also held to their own f32 tolerance (tests/f32_spread.py, through Tally.add's
spreads), computed once per scene (CASES) for the CPU and the GPU leg; this file has no tolerance of its own, and its class computes
nothing outside mesh_compose_f64's interp_uv, tex_lookup and bend, which carry the noise.  On the CPU
(test_the_spreads_of_the_restatement): scene 0 median spread 4.0e-7, largest 4.7e-3, 0.67 % with a tolerance above 1e-3, 8.7 s of
CPU time; scene 1 median 5.7e-7, largest 1.9e-4, 1.33 % above, 5.5 s.  Teeth
(test_the_spreads_see_a_strength_a_tenth_of_a_percent_off): the map decoded at strength 1.001 leaves REL_CLEAN on no clean sample
of scene 1 and its own tolerance on 67.  The strength x 1.02 first thought of is no subtle fault under mirror-like and clearcoat
materials: it takes 11 (scene 0) and 13 (scene 1) clean samples beyond REL_CLEAN, x 1.005 still 3 and 1, and on scene 0 even
x 1.001 one.  On an MI355X: largest z 2.0 and 1.31 next to Z_MAX = 8.3, median z 0.29 and 0.32 next to Z_MEDIAN = 1.4,
8.0 s of wall time for the GPU test.  Measurements, not bounds."""
import ctypes as C

import numpy as np
import pytest

import f32_spread as S
import mesh_compose_f64 as MC
import pt_f64 as P
from kernel_census import mesh_kernel_of
from test_gpu_mesh_f64 import _scenes
from test_gpu_mesh_smooth_f64 import _draws
from test_gpu_mesh_texture_f64 import BILINEAR, GAMMA, MODES, TexMeshDescScene, scene_textures
from test_gpu_path_f64 import Tally
from test_path_f64 import NEAR_TIE_MAX, REL_CLEAN, TAU, rel_distance

TEX_BIT, NRM_BIT = 1 << 28, 1 << 31
STRENGTH = 1.001                                                      # the planted fault (1.02 is not subtle here: see the docstring)
NEAR_TIE_COUNT = 126                                                # of 1 200, counted on the CPU
MUT_IGNORE, MUT_SWAP = 56, 55                                       # of the 200 draws of the mutation case


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def bump_map():
    from rust_pathtracer_amd import scenes
    return scenes.mesh_normal_map_scene()[2]


def decode_f64(rgba):
    """include/rpt.h's decode in float64 at strength 1, no flip: [h, w, 3]."""
    return MC.decode_normal_map_f64(rgba)


class NrmMeshDescScene(TexMeshDescScene):
    """Every mesh FLAT, textured and normal-mapped.  fault: None, "ignore" (the map is not applied) or "swap" (T and B change
    places); the texture itself is always applied."""

    def __init__(self, desc, scene, wrap, filt, fault=None):
        super().__init__(desc, scene, wrap, filt)
        self.nrm_fault = fault
        self.nrm = decode_f64(bump_map())

    def triangle_normal(self, k, o, d, M):
        N = super().triangle_normal(k, o, d, M)                       # (flat; remembers the winner for the texture)
        if self.nrm_fault == "ignore":
            return N
        s, t = MC.interp_uv(self, k, *self.barycentrics(k, o, d))
        ua, ub, uc = (self.uv[j] for j in self.corner[k])
        return MC.bend(np.array(N), self.e1[k], self.e2[k], ua, ub, uc, self.bilinear(s, t), M, swap=self.nrm_fault == "swap")

    def bilinear(self, s, t):
        """tex_lookup, BILINEAR, over the decoded map with the TEXTURE's wrap."""
        return MC.tex_lookup(self.nrm, s, t, self.wrap, BILINEAR, None)


def _path(k):
    s = _scenes()[k][1]
    return P.Path(NrmMeshDescScene(s.describe(), s, *MODES[k]))


# per scene: the restated draws and the f32 spreads of their first 150 clean samples, once for the CPU and the GPU leg
CASES = S.Cases(_path, lambda k: [(seed, pixels) for j, _, _, seed, pixels, _, _ in _draws() if j == k])


def _one_mapped_sample(rpt, torch, scene, wrap, filt, w, h, seed):
    """A one-sample render with every mesh textured and normal-mapped into a fresh buffer -> (frame, kernel choice)."""
    t = rpt.Tracer(scene, device=0, seed=seed)
    try:
        t.set_mesh_textures({m: dict(uvs=uv, texels=img, wrap=("repeat", "clamp")[wrap], filter=("nearest", "bilinear")[filt], gamma=GAMMA)
                             for m, (uv, img) in scene_textures(scene).items()})
        t.set_mesh_normal_maps({m: dict(texels=bump_map(), filter="bilinear", strength=1.0) for m in range(len(scene.meshes))})
        buf = rpt.DeviceColorBuffer(w, h)
        t.render_n(buf, 1)
        torch.cuda.synchronize()
        choice = C.c_uint32()
        assert rpt.lib().rpt_debug_kernel_choice(t._h, C.byref(choice)) == 0
        return buf.pixels.cpu().numpy(), choice.value
    finally:
        t.close()


@pytest.mark.gpu
def test_normal_mapped_mesh_renders_against_the_restatement(rpt, oracle, torch_cuda):
    t = Tally(TAU, NEAR_TIE_MAX)
    per = None
    for n, (k, what, s, seed, pixels, w, h) in enumerate(_draws()):
        wrap, filt = MODES[k]
        if n % 3 == 0:
            print("%s: the spreads took %.2f s of CPU time" % (what, CASES.spreads(oracle, k)[1]))
        frame, choice = _one_mapped_sample(rpt, torch_cuda, s, wrap, filt, w, h, seed)
        assert choice & (1 << 25) and choice & TEX_BIT and choice & NRM_BIT, "the normal-mapped mesh kernel ran"
        assert mesh_kernel_of(choice) == "meshnrm_regen_kernel"
        t.ran.add(mesh_kernel_of(choice))
        seed2, pixels2, restated, margins = CASES.restated(oracle, k)[n % 3]
        assert (seed2, pixels2) == (seed, pixels)
        print("%s (seed %d): %d of %d samples below TAU" % (what, seed, int((margins <= TAU).sum()), len(margins)))
        t.add("%s, normal-mapped (seed %d)" % (what, seed), frame, restated, margins, pixels, spreads=CASES.spreads(oracle, k)[0][n % 3])
        per = per if n % 3 else Tally(TAU, NEAR_TIE_MAX)
        per.add("%s, normal-mapped (seed %d)" % (what, seed), frame, restated, margins, pixels, spreads=CASES.spreads(oracle, k)[0][n % 3])
        if n % 3 == 2:
            print("%s: %s" % (what, per.held.line()))
    t.check("normal-mapped mesh scenes")
    assert t.n == 2 * 3 * 200


def test_the_near_tie_count_of_the_restatement(rpt, oracle):
    """The restatement alone, for exactly the draws of the GPU comparison: the count in this file's docstring, under the cap."""
    near = n = 0
    refs = {}
    for k, what, s, seed, pixels, w, h in _draws():
        if k not in refs:
            refs[k] = NrmMeshDescScene(s.describe(), s, *MODES[k])
        _, margins, _ = P.sample_many(refs[k], oracle, seed, [(c, r, 0) for c, r in pixels], w, h)
        near += int((margins <= TAU).sum())
        n += len(margins)
    print("%d of %d samples below TAU" % (near, n))
    assert n == 1200 and near == NEAR_TIE_COUNT and near <= NEAR_TIE_MAX * n


def test_the_map_is_gentle():
    d = decode_f64(bump_map())
    tilt = np.degrees(np.arctan2(np.hypot(d[..., 0], d[..., 1]), d[..., 2]))
    assert d.shape == (32, 32, 3) and 10.0 < tilt.max() <= 16.0 and tilt.min() < 3.0


def test_the_restatement_sees_the_map(rpt, oracle):
    """Two planted faults, each of which a device could have: the map ignored, T and B swapped.  Each moves clean samples beyond
    REL_CLEAN, so the comparison above would catch it."""
    k, what, s, seed, pixels, w, h = next(iter(_draws()))
    items = [(c, r, 0) for c, r in pixels]
    base, marg, _ = P.sample_many(NrmMeshDescScene(s.describe(), s, *MODES[k]), oracle, seed, items, w, h)
    moved = {}
    for fault in ("ignore", "swap"):
        other, marg2, _ = P.sample_many(NrmMeshDescScene(s.describe(), s, *MODES[k], fault=fault), oracle, seed, items, w, h)
        clean = (marg > TAU) & (marg2 > TAU)
        moved[fault] = int((rel_distance(np.nan_to_num(other), np.nan_to_num(base))[clean] > REL_CLEAN).sum())
    print("clean samples moved beyond REL_CLEAN:", moved)
    assert moved == {"ignore": MUT_IGNORE, "swap": MUT_SWAP} and min(moved.values()) > 10


@pytest.mark.parametrize("k", (0, 1))
def test_the_spreads_of_the_restatement(rpt, oracle, k):
    """The conditions of the comparison with spreads, on the restatement alone: at least 100 clean samples of the scene have a
    spread, and at most 5 % of them a tolerance above 1e-3."""
    CASES.conditions(oracle, _scenes()[k][0] + ", normal-mapped", k)


def test_the_spreads_see_a_strength_a_tenth_of_a_percent_off(rpt, oracle):
    """The map decoded at strength 1.001, rounded to f32, as a device's samples over the second scene's draws: no clean sample
    leaves REL_CLEAN, at least 10 leave their own tolerance.  (Under these scenes' mirror-like and clearcoat materials a strength of
    1.02 is no subtle fault: it takes 11 and 13 clean samples of the two scenes beyond REL_CLEAN; 1.005 still 3 and 1.)"""
    s = _scenes()[1][1]
    faulty = NrmMeshDescScene(s.describe(), s, *MODES[1])
    faulty.nrm = MC.decode_normal_map_f64(bump_map(), strength=STRENGTH)
    entries, (spreads, _) = CASES.restated(oracle, 1), CASES.spreads(oracle, 1)
    S.teeth("the map's strength x %g (%s)" % (STRENGTH, _scenes()[1][0]), entries, spreads,
            [MC.sample_pixels(P.Path(faulty), oracle, seed, pixels, 64, 48) for seed, pixels, _, _ in entries])
