"""The eight media kernel forms (28 .. 35) held to the float64 restatement of mesh media (tests/mesh_media_f64.py: MediaMeshDescScene
and MediaMeshPath, written from include/rpt.h's section "mesh media" over the composed mesh restatement and the media restatement).

One case per form on scenes.mesh_media_scene at four bounces with the composed file's textures, masks, maps and sky (its cases A
.. H); the medium on the glass icosphere rotates over the cases — ABSORB in A and E, SCATTER with g = 0 in B and H and with g = 0.6
in C and F, EMISSIVE in D and G (tests/test_mesh_media_f64.py, MEDIA) — the lamp mesh is ON inside the pick in every case and the
sky is SAMPLED in B, D, F and H.  Per case 200 random pixels x 2 seeds, each sample a one-sample render into a fresh
DeviceColorBuffer, compared through test_gpu_path_f64.Tally with test_path_f64's TAU / REL_CLEAN / NEAR_TIE_MAX: this file has no
tolerance of its own.  tests/test_mesh_media_f64.py holds the near-tie condition of exactly these draws on the CPU.

The largest clean relative distance seen on an MI355X, per case (every run prints it, pytest -s): A 2.4e-4, B 9.7e-6, C 1.2e-5,
D 1.6e-5, E 3.5e-5, F 1.0e-5, G 2.2e-4, H 7.1e-5, next to REL_CLEAN = 5e-2.  All eight comparisons together take 4.2 s.

The first 150 clean samples of every case are also held to their own f32 tolerance (tests/f32_spread.py, through Tally.add's
spreads; tests/test_mesh_media_f64.py computes them once per case, 1.9 to 2.5 s of CPU time, holds their conditions and shows that a
sigma_t 2 % off and a phase function evaluated at g + 0.01 fail them while passing REL_CLEAN).  The largest z seen on an MI355X,
per case: A 1.13, B 2.27, C 1.26, D 1.23, E 1.42, F 1.16, G 1.27, H 1.86, next to Z_MAX = 8.3; the medians 0.12 to 0.33.
Measurements, not bounds."""
import pytest

from test_gpu_mesh_material_map_f64 import mesh_form, set_composed
from test_gpu_mesh_compose_f64 import CASES, H, W, inputs
from test_gpu_path_f64 import Tally
from test_mesh_media_f64 import MEDIA, restated, scene, spreads
from test_path_f64 import NEAR_TIE_MAX, TAU

MED_FORM_FIRST = 28


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_media_renders_against_the_restatement(rpt, oracle, torch_cuda, case):
    form = MED_FORM_FIRST + sorted(CASES).index(case)
    s = scene()
    args = inputs(s, case)
    tally = Tally(TAU, NEAR_TIE_MAX)
    spr, seconds = spreads(oracle, case)
    print("case %s: the spreads took %.2f s of CPU time" % (case, seconds))
    for (seed, pixels, radiance, margins), spread in zip(restated(oracle, case), spr):
        t = rpt.Tracer(s, device=0, seed=seed)
        try:
            set_composed(t, args)
            t.set_mesh_media({0: MEDIA[case]})
            buf = rpt.DeviceColorBuffer(W, H)
            t.render_n(buf, 1)
            torch_cuda.cuda.synchronize()
            frame = buf.pixels.cpu().numpy()
            assert mesh_form(rpt, t) == form, "case %s: form %d, not %d" % (case, mesh_form(rpt, t), form)
        finally:
            t.close()
        tally.ran.add("form %d" % form)
        print("case %s (seed %d): %d of %d samples below TAU" % (case, seed, int((margins <= TAU).sum()), len(margins)))
        tally.add("case %s (seed %d, form %d, %s)" % (case, seed, form, MEDIA[case]["type"]), frame, radiance, margins, pixels,
                  spreads=spread)
    tally.check("case %s" % case)
    assert tally.n == 400 and tally.ran == {"form %d" % form}
