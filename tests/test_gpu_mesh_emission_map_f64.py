"""The eight emission-mapped mesh kernel forms held to the float64 restatement of one pixel-sample (tests/mesh_emap_f64.py:
EmapMeshDescScene and EmapPath, subclasses of the material-mapped restatement that scale the emission after the base's patch and in
the mesh-light sampler).

Eight cases, one per form 20 .. 27 (rpt_debug_mesh_form): test_gpu_mesh_compose_f64's cases A .. H — its scene, textures, lamp, sky,
mask and bump maps, taken through its inputs() — with mesh_mmap_f64's metallic object made to emit a little (mesh_emap_f64.scene),
mesh_mmap_f64.material_maps and mesh_emap_f64.emission_maps on top: a 5 x 3 NEAREST map at gamma 2.2 on the object and a 16 x 16
BILINEAR one on the lamp, which is ON.  The scene's spherical rpt_light stands in front of the floor and the object for some pixels,
so the emitter exit is among the samples.  400 samples per case (64 x 48, 200 random pixels x 2 seeds, each a one-sample render into a
fresh buffer), compared through test_gpu_path_f64.Tally with test_path_f64's TAU / REL_CLEAN / NEAR_TIE_MAX: this file has no
tolerance of its own.  tests/test_mesh_emission_map_f64.py (CPU) holds the restatement's near-tie counts under the cap, counts what
its three planted faults move, and closes the other side with all-255 maps.

The first 150 clean samples of every case and of the emitter exit are also held to their own f32 tolerance (tests/f32_spread.py,
through Tally.add's spreads; the CPU file computes them once per case, 1.8 to 2.3 s of CPU time, and holds their conditions).  The
largest z seen on an MI355X, per case: A 1.06, B 1.38, C 1.57, D 1.31, E 1.74, F 1.50, G 0.98, H 1.42, the emitter exit 1.14, next
to Z_MAX = 8.3; the medians 0.20 to 0.41.  Measurements, not bounds."""
import functools

import numpy as np
import pytest

import f32_spread as S
import mesh_emap_f64 as ME
import mesh_mmap_f64 as MM
from test_gpu_mesh_compose_f64 import CASES, H, W, inputs
from test_gpu_mesh_emission_map import _panel_scene, _panel_textures, _through_the_light, form_of
from test_gpu_mesh_material_map_f64 import mesh_form, set_composed
from test_gpu_path_f64 import Tally
from mesh_compose_f64 import sample_pixels
from test_mesh_emission_map_f64 import restated, spreads
from test_path_f64 import NEAR_TIE_MAX, TAU


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_emission_mapped_renders_against_the_restatement(rpt, oracle, torch_cuda, case):
    s = ME.scene()
    args = inputs(s, case)
    tally = Tally(TAU, NEAR_TIE_MAX)
    spr, seconds = spreads(oracle, case)
    print("case %s: the spreads took %.2f s of CPU time" % (case, seconds))
    for (seed, pixels, want, margins), spread in zip(restated(oracle, case), spr):
        t = rpt.Tracer(s, device=0, seed=seed)
        try:
            set_composed(t, args)
            t.set_mesh_material_maps(MM.material_maps())
            t.set_mesh_emission_maps(ME.emission_maps())
            buf = rpt.DeviceColorBuffer(W, H)
            t.render_n(buf, 1)
            torch_cuda.cuda.synchronize()
            frame = buf.pixels.cpu().numpy()
            assert mesh_form(rpt, t) == form_of(case), "case %s: form %d, not %d" % (case, mesh_form(rpt, t), form_of(case))
        finally:
            t.close()
        tally.ran.add("form %d" % form_of(case))
        print("case %s (seed %d): %d of %d samples below TAU" % (case, seed, int((margins <= TAU).sum()), len(margins)))
        tally.add("case %s (seed %d, form %d)" % (case, seed, form_of(case)), frame, want, margins, pixels, spreads=spread)
    tally.check("case %s" % case)
    assert tally.n == 400


# ---- the emitter exit ----------------------------------------------------------------------------------------------------------------
def exit_maps():
    """The lamp under a 5 x 3 NEAREST map, the panel under a 16 x 16 BILINEAR one at gamma 2.2."""
    return {1: dict(texels=MM.noise_map(5, 3, 97), filter="nearest", gamma=1.0), 2: dict(texels=MM.noise_map(16, 16, 98), filter="bilinear", gamma=2.2)}


def exit_pixels():
    """The pixels whose rays pass through the spherical light and end on the panel behind it, and as many random ones."""
    through = _through_the_light(W, H)
    rng = np.random.default_rng(49)
    return through + list(zip(rng.integers(0, W, len(through)).tolist(), rng.integers(0, H, len(through)).tolist()))


@functools.lru_cache(maxsize=None)
def exit_restated(oracle, seed):
    s = _panel_scene()
    sc = ME.EmapMeshDescScene(s.describe(), s, emission_maps=exit_maps(), on=(1, 2), textures=_panel_textures(s))
    path = ME.EmapPath(sc)
    want, margins = sample_pixels(path, oracle, seed, exit_pixels(), W, H)
    spr, seconds = S.spreads_of_draws(path, oracle, [(seed, exit_pixels(), want, margins)], W, H)
    return want, margins, spr[0], seconds


@pytest.mark.gpu
def test_the_emitter_exit_against_the_restatement(rpt, oracle, torch_cuda):
    """test_gpu_mesh_emission_map's panel scene: a spherical rpt_light in front of an emission-mapped panel, both meshes ON.  One
    frame, the pixels through the light and as many others."""
    s = _panel_scene()
    seed, pixels = 77, exit_pixels()
    want, margins, spread, seconds = exit_restated(oracle, seed)
    print("the emitter exit: the spreads took %.2f s of CPU time" % seconds)
    t = rpt.Tracer(s, device=0, seed=seed)
    try:
        t.set_mesh_textures(_panel_textures(s))
        t.set_mesh_lights({1: True, 2: True})
        t.set_mesh_emission_maps(exit_maps())
        buf = rpt.DeviceColorBuffer(W, H)
        t.render_n(buf, 1)
        torch_cuda.cuda.synchronize()
        frame = buf.pixels.cpu().numpy()
        assert mesh_form(rpt, t) == 20
    finally:
        t.close()
    tally = Tally(TAU, NEAR_TIE_MAX)
    tally.ran.add("form 20")
    tally.add("the emitter exit (seed %d)" % seed, frame, want, margins, pixels, spreads=spread)
    tally.check("the emitter exit")
    assert tally.n == len(pixels) > 100
