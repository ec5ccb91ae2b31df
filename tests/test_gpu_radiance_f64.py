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
All seventeen comparisons together take 1.5 s."""
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
    tally.add("%s %s" % (stack, case), frame, radiance, margins, [(i, 0) for i in range(TR.N_RAYS)])
    tally.check("%s %s" % (stack, case))
    assert tally.n == TR.N_RAYS and tally.near == TR.COUNTS[(stack, case)][0]
