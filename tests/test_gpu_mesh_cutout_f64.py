"""Cutout mesh renders held to tests/pt_f64.py, the float64 restatement of one pixel-sample (include/rpt.h, "mesh cutouts"):
CutMeshDescScene is test_gpu_mesh_texture_f64.TexMeshDescScene — by import only — with the cut test restated in float64 as the
last line of its triangle test: u and v of that test, the UV interpolation, the texture's wrap, the NEAREST texel of the mask.  One-
sample renders are compared sample by sample with test_path_f64's TAU / REL_CLEAN / NEAR_TIE_MAX over test_gpu_mesh_f64's own
draws, 200 pixels x 3 seeds x 2 scenes (needs an MI355X).  Every mesh carries test_gpu_mesh_texture_f64's texture (the first scene
BILINEAR / REPEAT, the second NEAREST / CLAMP) and a 4 x 2 checker mask of single texels over the same UVs (not square: swapping
s and t must not map the mask onto itself).  The statements themselves are
functions of tests/mesh_compose_f64.py, which the composed restatement (tests/test_gpu_mesh_compose_f64.py) calls as well.

Margins.  The mask is a step function: for every triangle that passes the rest of the test, the distance of x*W and of y*H to the
next integer is recorded through M.of(., 1.0), where the coordinate is not clamped — as NEAREST does in the textured restatement.

The restatement alone, on the CPU, for exactly these draws (test_the_near_tie_count_of_the_restatement counts it again):
130 of 1 200 samples lie below TAU (10.8 %), under the 12 % cap of 144 (the textured restatement without masks has 128).
Mutation (test_the_restatement_sees_the_mask, the first scene's first 200 draws): a restatement that ignores the mask moves
36 clean samples beyond REL_CLEAN, one that swaps s and t 41."""
import ctypes as C

import numpy as np
import pytest

import mesh_compose_f64 as MC
import pt_f64 as P
from kernel_census import mesh_kernel_of
from test_gpu_mesh_smooth_f64 import _draws
from test_gpu_mesh_texture_f64 import GAMMA, MODES, TexMeshDescScene, scene_textures
from test_gpu_path_f64 import Tally
from test_path_f64 import NEAR_TIE_MAX, REL_CLEAN, TAU, rel_distance

CUT_BIT = 1 << 30
MASK_W, MASK_H = 4, 2
NEAR_TIE_COUNT = 130                                                # of 1 200, counted on the CPU
MUT_IGNORE, MUT_SWAP = 36, 41                                       # of the 200 draws of the mutation case


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def scene_masks(scene):
    """-> {mesh: A8 [MASK_H, MASK_W]}: a checker of single texels, texel (0, 0) opaque on even meshes and a hole on odd ones."""
    j, i = np.meshgrid(np.arange(MASK_H), np.arange(MASK_W), indexing="ij")
    return {m: np.where((i + j + m) % 2 == 0, 255, 0).astype(np.uint8) for m in range(len(scene.meshes))}


class CutMeshDescScene(TexMeshDescScene):
    """Every mesh FLAT, textured and cut out.  cut_fault: None, "ignore" (the mask is not applied) or "swap" (s and t change places
    in the cut test only)."""

    def __init__(self, desc, scene, wrap, filt, cut_fault=None):
        super().__init__(desc, scene, wrap, filt)
        self.cut_fault = cut_fault
        self.opaque = [mask >= 128 for _, mask in sorted(scene_masks(scene).items())]

    def _triangles(self, o, d, M):
        """The triangle test with its last line: a triangle that passes everything else misses where its mesh's mask has a hole."""
        hit, t = super()._triangles(o, d, M)
        if self.cut_fault != "ignore":
            MC.cut_test(self, hit, o, d, M, lambda k: (self.opaque[int(self.tri_mesh[k])], self.wrap), swap=self.cut_fault == "swap")
        return hit, t


def _one_cut_sample(rpt, torch, scene, wrap, filt, w, h, seed):
    """A one-sample render with every mesh textured and cut out into a fresh buffer -> (frame, kernel choice)."""
    t = rpt.Tracer(scene, device=0, seed=seed)
    try:
        t.set_mesh_textures({m: dict(uvs=uv, texels=img, wrap=("repeat", "clamp")[wrap], filter=("nearest", "bilinear")[filt], gamma=GAMMA)
                             for m, (uv, img) in scene_textures(scene).items()})
        t.set_mesh_cutouts(scene_masks(scene))
        buf = rpt.DeviceColorBuffer(w, h)
        t.render_n(buf, 1)
        torch.cuda.synchronize()
        choice = C.c_uint32()
        assert rpt.lib().rpt_debug_kernel_choice(t._h, C.byref(choice)) == 0
        return buf.pixels.cpu().numpy(), choice.value
    finally:
        t.close()


@pytest.mark.gpu
def test_cutout_mesh_renders_against_the_restatement(rpt, oracle, torch_cuda):
    t = Tally(TAU, NEAR_TIE_MAX)
    refs = {}
    for k, what, s, seed, pixels, w, h in _draws():
        wrap, filt = MODES[k]
        if k not in refs:
            refs[k] = CutMeshDescScene(s.describe(), s, wrap, filt)
        frame, choice = _one_cut_sample(rpt, torch_cuda, s, wrap, filt, w, h, seed)
        assert choice & (1 << 25) and choice & CUT_BIT, "the cutout mesh kernel ran"
        assert mesh_kernel_of(choice) == "meshcut_regen_kernel"
        t.ran.add(mesh_kernel_of(choice))
        restated, margins, _ = P.sample_many(refs[k], oracle, seed, [(c, r, 0) for c, r in pixels], w, h)
        print("%s (seed %d): %d of %d samples below TAU" % (what, seed, int((margins <= TAU).sum()), len(margins)))
        t.add("%s, cut out (seed %d)" % (what, seed), frame, restated, margins, pixels)
    t.check("cutout mesh scenes")
    assert t.n == 2 * 3 * 200


def test_the_near_tie_count_of_the_restatement(rpt, oracle):
    """The restatement alone, for exactly the draws of the GPU comparison: the count in this file's docstring, under the cap."""
    near = n = 0
    refs = {}
    for k, what, s, seed, pixels, w, h in _draws():
        if k not in refs:
            refs[k] = CutMeshDescScene(s.describe(), s, *MODES[k])
        _, margins, _ = P.sample_many(refs[k], oracle, seed, [(c, r, 0) for c, r in pixels], w, h)
        near += int((margins <= TAU).sum())
        n += len(margins)
    print("%d of %d samples below TAU" % (near, n))
    assert n == 1200 and near == NEAR_TIE_COUNT and near <= NEAR_TIE_MAX * n


def test_the_restatement_sees_the_mask(rpt, oracle):
    """Two planted faults, each of which a device could have: the mask ignored, s and t swapped in the cut test.  Each moves clean
    samples beyond REL_CLEAN, so the comparison above would catch it."""
    k, what, s, seed, pixels, w, h = next(iter(_draws()))
    items = [(c, r, 0) for c, r in pixels]
    base, marg, _ = P.sample_many(CutMeshDescScene(s.describe(), s, *MODES[k]), oracle, seed, items, w, h)
    moved = {}
    for fault in ("ignore", "swap"):
        other, marg2, _ = P.sample_many(CutMeshDescScene(s.describe(), s, *MODES[k], cut_fault=fault), oracle, seed, items, w, h)
        clean = (marg > TAU) & (marg2 > TAU)
        moved[fault] = int((rel_distance(np.nan_to_num(other), np.nan_to_num(base))[clean] > REL_CLEAN).sum())
    print("clean samples moved beyond REL_CLEAN:", moved)
    assert moved == {"ignore": MUT_IGNORE, "swap": MUT_SWAP} and min(moved.values()) > 10
