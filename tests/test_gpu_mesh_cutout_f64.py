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
36 clean samples beyond REL_CLEAN, one that swaps s and t 41.

The first 150 clean samples of each scene are also held to their own f32 tolerance (tests/f32_spread.py, through Tally.add's
spreads), computed once per scene (CASES) for the CPU and the GPU leg; this file has no tolerance of its own, and its class computes
nothing outside mesh_compose_f64's cut_test.  On the CPU (test_the_spreads_of_the_restatement): scene 0 median spread 3.3e-7,
largest 6.3e-5, none with a tolerance above 1e-3, 7.5 s of CPU time; scene 1 median 5.0e-7, largest 2.2e-4, 0.67 % above, 5.5 s.
No teeth of this file's own: the mask is a step function, and a fault in the UV interpolation that feeds it either changes nothing
or flips whole samples.  Measured with u times 1.02, 1.01 and 1.002 in the cut test's interpolation only, over each scene's 600
draws: scene 0 moves no sample at all under any of the three; scene 1 moves 3, 2 and 0, every one of them beyond REL_CLEAN.  No
fault there is both subtle and visible on these draws, so the feature's subtle faults are left to what the cut test shares with the
textured file (interp_uv, held there by a shifted lookup) and the gross ones to test_the_restatement_sees_the_mask.  On an MI355X:
largest z 1.67 and 1.56 next to Z_MAX = 8.3, median z 0.31 and 0.35 next to Z_MEDIAN = 1.4, 7.2 s of wall time for
the GPU test.  Measurements, not bounds."""
import ctypes as C

import numpy as np
import pytest

import f32_spread as S
import mesh_compose_f64 as MC
import pt_f64 as P
from kernel_census import mesh_kernel_of
from test_gpu_mesh_f64 import _scenes
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


def _path(k):
    s = _scenes()[k][1]
    return P.Path(CutMeshDescScene(s.describe(), s, *MODES[k]))


# per scene: the restated draws and the f32 spreads of their first 150 clean samples, once for the CPU and the GPU leg
CASES = S.Cases(_path, lambda k: [(seed, pixels) for j, _, _, seed, pixels, _, _ in _draws() if j == k])


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
    per = None
    for n, (k, what, s, seed, pixels, w, h) in enumerate(_draws()):
        wrap, filt = MODES[k]
        if n % 3 == 0:
            print("%s: the spreads took %.2f s of CPU time" % (what, CASES.spreads(oracle, k)[1]))
        frame, choice = _one_cut_sample(rpt, torch_cuda, s, wrap, filt, w, h, seed)
        assert choice & (1 << 25) and choice & CUT_BIT, "the cutout mesh kernel ran"
        assert mesh_kernel_of(choice) == "meshcut_regen_kernel"
        t.ran.add(mesh_kernel_of(choice))
        seed2, pixels2, restated, margins = CASES.restated(oracle, k)[n % 3]
        assert (seed2, pixels2) == (seed, pixels)
        print("%s (seed %d): %d of %d samples below TAU" % (what, seed, int((margins <= TAU).sum()), len(margins)))
        t.add("%s, cut out (seed %d)" % (what, seed), frame, restated, margins, pixels, spreads=CASES.spreads(oracle, k)[0][n % 3])
        per = per if n % 3 else Tally(TAU, NEAR_TIE_MAX)
        per.add("%s, cut out (seed %d)" % (what, seed), frame, restated, margins, pixels, spreads=CASES.spreads(oracle, k)[0][n % 3])
        if n % 3 == 2:
            print("%s: %s" % (what, per.held.line()))
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


@pytest.mark.parametrize("k", (0, 1))
def test_the_spreads_of_the_restatement(rpt, oracle, k):
    """The conditions of the comparison with spreads, on the restatement alone: at least 100 clean samples of the scene have a
    spread, and at most 5 % of them a tolerance above 1e-3."""
    CASES.conditions(oracle, _scenes()[k][0] + ", cut out", k)
