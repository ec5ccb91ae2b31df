"""The device held to tests/media_sdf_f64.py, the float64 restatement of participating media and of the SDF object written from
include/rpt.h's text, with no oracle/rpt_oracle.hpp in the loop except the draws (Oracle.rng_f32) (needs an MI355X).  One-sample renders
into a fresh buffer of tests/test_media_sdf_f64.py's shared_sets() — frames of at most 98 x 73, 240-400 pixels per case — through
tests/test_gpu_path_f64.py's _one_sample, Tally and _compare at its bounds (TAU, REL_CLEAN, NEAR_TIE_MAX; TAU_LARGE and
NEAR_TIE_MAX_LARGE for the large class); the kernel that ran is asserted per case (tests/kernel_census.py).  All 14 strict SDF and
media kernels: render_sdf_march2_kernel, _table_kernel, _sized_kernel<1..4>, _sized_table_kernel<1..4> and _media_kernel (the object
full of fog: step 4 reads the tetrahedral normal); render_small_regen_media_kernel (RPT_COMPACT_MAX_SPP=0) and
render_small_compact_media_kernel, nine cases each: media_scene(), the purpose-built scenes, with and without roulette, and three of the
six fuzzed media scenes; render_large_regen_media_kernel (300 spheres, brute-forced with numpy).  The relaxed (_fast) kernels have bounds
of their own (tests/test_gpu_relaxed.py).

One Tally per test; its near-tie share is known from the restatement before any launch (tests/test_media_sdf_f64.py asserts it <= 0.09
for the first two).  Measured on an MI355X: sdf 3 520 samples, 6.79 % near ties, largest clean relative distance 5.89e-3; media
5 040 samples, 5.06 %, 3.85e-4; large 400 samples, 35.5 %, 2.06e-4 — the f32 oracle's figures, as they must be for kernels that match
it bit for bit.  What the inputs can catch is shown on the CPU leg, mutant by mutant, on these same items; on the device, with the
`* t` of the march's hit test or the clamp of g deleted from the device headers the SDF test and the media test fail (sized<1>: 1 clean
sample beyond REL_CLEAN in its first case; lamp in fog: 141), and with the scatter point's light sample left unattenuated both fail
(media scene: 29; the object full of fog: 1)."""
import pytest

import media_sdf_f64 as MS
import pt_f64 as P
from kernel_census import kernel_of
from test_gpu_path_f64 import Tally, _compare
from test_media_sdf_f64 import shared_sets
from test_path_f64 import NEAR_TIE_MAX, NEAR_TIE_MAX_LARGE, TAU, TAU_LARGE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def cases(rpt):
    return shared_sets(rpt)


def _pool(rpt, torch, oracle, monkeypatch, cases, pool, tally):
    """Every case of the pool: a one-sample render, the kernel that ran, the samples against the restatement."""
    ran = {}
    for c in cases:
        if c.pool != pool:
            continue
        scene = MS.MediaSdfDescScene(c.scene.describe())
        roulette = bool(c.flags & P.RENDER_RUSSIAN_ROULETTE)

        def restate(oracle, seed, items, w, h, scene=scene, roulette=roulette):
            return MS.sample_many(scene, oracle, seed, items, w, h, roulette=roulette)
        choice = _compare(rpt, torch, oracle, tally, c.name, c.scene, c.w, c.h, c.seed, bool(c.mega), monkeypatch, [(col, row) for col, row, _ in c.items],
                          klass=c.klass, flags=c.flags, restate=restate)
        assert kernel_of(choice, c.klass) == c.kernel, "%s: aimed at %s, ran %s (choice %#x)" % (c.name, c.kernel, kernel_of(choice, c.klass), choice)
        ran[c.kernel] = ran.get(c.kernel, 0) + 1
    tally.check(pool)
    return ran


def test_sdf_kernels_against_the_restatement(rpt, oracle, torch_cuda, monkeypatch, cases):
    ran = _pool(rpt, torch_cuda, oracle, monkeypatch, cases, "sdf", Tally(TAU, NEAR_TIE_MAX))
    want = {"render_sdf_march2_kernel", "render_sdf_march2_table_kernel", "render_sdf_march2_media_kernel"}
    want |= {"render_sdf_march2_sized%s_kernel<%d>" % (t, n) for t in ("", "_table") for n in (1, 2, 3, 4)}
    assert set(ran) == want


def test_small_media_kernels_against_the_restatement(rpt, oracle, torch_cuda, monkeypatch, cases):
    ran = _pool(rpt, torch_cuda, oracle, monkeypatch, cases, "media", Tally(TAU, NEAR_TIE_MAX))
    assert set(ran) == {"render_small_regen_media_kernel", "render_small_compact_media_kernel"}
    assert min(ran.values()) >= 9                                     # media_scene, the purpose-built scenes and three fuzzed ones through each


def test_large_media_kernel_against_the_restatement(rpt, oracle, torch_cuda, monkeypatch, cases):
    ran = _pool(rpt, torch_cuda, oracle, monkeypatch, cases, "large", Tally(TAU_LARGE, NEAR_TIE_MAX_LARGE))
    assert set(ran) == {"render_large_regen_media_kernel"}
