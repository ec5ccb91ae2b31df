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
56 clean samples beyond REL_CLEAN, one that swaps T and B 55."""
import ctypes as C

import numpy as np
import pytest

import mesh_compose_f64 as MC
import pt_f64 as P
from kernel_census import mesh_kernel_of
from test_gpu_mesh_smooth_f64 import _draws
from test_gpu_mesh_texture_f64 import BILINEAR, GAMMA, MODES, TexMeshDescScene, scene_textures
from test_gpu_path_f64 import Tally
from test_path_f64 import NEAR_TIE_MAX, REL_CLEAN, TAU, rel_distance

TEX_BIT, NRM_BIT = 1 << 28, 1 << 31
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
    refs = {}
    for k, what, s, seed, pixels, w, h in _draws():
        wrap, filt = MODES[k]
        if k not in refs:
            refs[k] = NrmMeshDescScene(s.describe(), s, wrap, filt)
        frame, choice = _one_mapped_sample(rpt, torch_cuda, s, wrap, filt, w, h, seed)
        assert choice & (1 << 25) and choice & TEX_BIT and choice & NRM_BIT, "the normal-mapped mesh kernel ran"
        assert mesh_kernel_of(choice) == "meshnrm_regen_kernel"
        t.ran.add(mesh_kernel_of(choice))
        restated, margins, _ = P.sample_many(refs[k], oracle, seed, [(c, r, 0) for c, r in pixels], w, h)
        print("%s (seed %d): %d of %d samples below TAU" % (what, seed, int((margins <= TAU).sum()), len(margins)))
        t.add("%s, normal-mapped (seed %d)" % (what, seed), frame, restated, margins, pixels)
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
