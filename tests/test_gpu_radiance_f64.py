"""Radiance along rays that no camera sends, held to the float64 restatement (tests/radiance_f64.py over the restatements the render
forms are held to) on an MI355X.

Seventeen cases — the eight media cases (the render's forms 28 .. 35), the eight both-maps cases (20 .. 27) and the flat scene (11)
— each with tests/test_radiance_f64.py's 200 rays: origins uniform in the box of the scene's mesh vertices grown by half its size,
directions uniform on the sphere, handed to both sides as the same float32 words.  One sample per ray, of frame FRAME on the stream
of index FIRST_INDEX + i, launched as one radiance query into a zeroed buffer whose frames_done is FRAME, so that the device's word
is the sample times 1 / (FRAME + 1); compared through test_gpu_path_f64.Tally with test_path_f64's TAU / REL_CLEAN / NEAR_TIE_MAX:
this file has no tolerance of its own.  Clean samples are within REL_CLEAN; near-tie samples are at most NEAR_TIE_MAX of each Tally
line — a condition, not a measurement — and tests/test_radiance_f64.py holds that condition for exactly these rays on the CPU.

The largest clean relative distance seen on an MI355X over all seventeen cases (every run prints each case's, pytest -s):
3.7e-4 (media E and both maps H; the other cases 1.3e-6 to 1.3e-4), next to REL_CLEAN = 5e-2.  It is a measurement, not a bound.
All seventeen comparisons together take 1.5 s.

Every ray is also held to its own f32 tolerance (tests/f32_spread.py: the spread of eight noisy runs of the restatement, cached
beside the restated values by tests/test_radiance_f64.py; min(REL_CLEAN, Z_MAX * max(spread, 2^-22)) per sample, the median and bias
statements per case), since the mesh kernels have no f32 twin.  What the first run on an MI355X found: with relative noise on the
results of the helpers and of the triangle test's t, u and v alone, two of the 3 400 samples lay beyond their tolerance — media G ray
37, 7.4e-6 away at a spread of 7.6e-7 (z = 9.7), and both maps F ray 40, 7.1e-6 away at 5.5e-7 (z = 12.8).  Tracer.trace of the
restatement's own segments (the ray queries answer per ray) placed it: on the first segment the device's u lay 22.8 x 2^-24 and 6.0 x
2^-24 from the float64 one, its t 7.0 and 2.0, where |s||p| / |det| — what a rounding of the terms of u is worth — is 34 and 10: the
honest rounding of a quotient of cancelling sums, a hundred times what relative noise on u itself injects, and the shading normal and
the BILINEAR texel followed it.  No kernel fault.  The injection now perturbs the triangle test term by term
(test_gpu_mesh_f64.MeshDescScene.noisy_tuv); with it those two samples have z = 1.05 and 0.51, the calibration is untouched (the
analytical scenes have no triangle) and every planted subtle fault still fails.
The largest z seen on an MI355X since, per case (every run prints it with the median, pytest -s): media A 0.89, B 1.05, C 1.37,
D 1.45, E 1.81, F 1.67, G 1.13, H 1.96; both maps A 1.74, B 1.00, C 1.28, D 1.34, E 1.57, F 1.22, G 1.61, H 1.62; flat 1.19 — the
largest 1.96, next to Z_MAX = 8.3; the medians 0 to 0.41, next to Z_MEDIAN = 1.4.  Measurements, not bounds.  The spreads add 2 to
2.8 s of CPU time per case, computed once for both legs."""
import numpy as np
import pytest

import test_mesh_frames_f64 as TF
import test_radiance_f64 as TR
from test_gpu_mesh_compose_f64 import inputs
from test_gpu_mesh_frames_f64 import open_tracer
from test_gpu_mesh_material_map_f64 import set_composed
from test_gpu_path_f64 import Tally
from test_mesh_media_f64 import MEDIA
from test_path_f64 import NEAR_TIE_MAX, TAU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def open_case(rpt, stack, case):
    """The Tracer of a case of tests/test_radiance_f64.py, its set calls made."""
    if stack == "media":
        s = TR.scene_of(stack, case)
        t = rpt.Tracer(s, device=0, seed=TR.SEED)
        set_composed(t, inputs(s, case))
        t.set_mesh_media({0: MEDIA[case]})
        return t
    if stack == "both maps":
        return open_tracer(rpt, "both maps", case, TR.SEED)
    return open_tracer(rpt, "single", TF.FLAT + " composed", TR.SEED)


@pytest.mark.parametrize("stack,case", TR.ALL_CASES, ids=TR.CASE_IDS)
def test_radiance_along_any_ray_against_the_restatement(rpt, oracle, torch_cuda, stack, case):
    rays = TR.rays_of(stack, case)
    radiance, margins = TR.restated(oracle, stack, case)
    spreads, seconds = TR.spreads(oracle, stack, case)
    print("%s %s: the spreads took %.2f s of CPU time" % (stack, case, seconds))
    t = open_case(rpt, stack, case)
    try:
        got = t.radiance(torch_cuda.from_numpy(rays).cuda(), spp=1, frames_done=TR.FRAME, first_index=TR.FIRST_INDEX)
        torch_cuda.cuda.synchronize()
        got = got.cpu().numpy()
        host = t.radiance(rays, spp=1, frames_done=TR.FRAME, first_index=TR.FIRST_INDEX)
    finally:
        t.close()
    assert np.array_equal(got.view(np.uint32), host.view(np.uint32)), "the host form"
    v = np.float32(1.0) / np.float32(TR.FRAME + 1)
    assert (got[:, 3] == v).all(), "alpha is (1 - v) * 0 + 1 * v"
    tally = Tally(TAU, NEAR_TIE_MAX)
    tally.ran.add("%s %s" % (stack, case))
    # the device's words are the sample times v: one row of 200 "pixels", scaled back in float64
    frame = got.astype(np.float64).reshape(1, TR.N_RAYS, 4) * float(TR.FRAME + 1)
    tally.add("%s %s" % (stack, case), frame, radiance, margins, [(i, 0) for i in range(TR.N_RAYS)], spreads=spreads)
    tally.check("%s %s" % (stack, case))
    assert tally.n == TR.N_RAYS and tally.near == TR.COUNTS[(stack, case)][0]
