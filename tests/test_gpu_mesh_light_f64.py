"""Renders with a mesh light held to tests/pt_f64.py, the float64 restatement of one pixel-sample (include/rpt.h, "mesh lights").
LightMeshDescScene is test_gpu_mesh_smooth_f64.SmoothMeshDescScene (per mesh FLAT or SMOOTH) that also knows which triangle won and
carries, per ON mesh, the INTEGER table (tests/test_mesh_light_host.py's restatement: the integers are the device's by construction)
and the f32 positions as float64.  LightPath is pt_f64.Path with direct_light over the N = n_lights + ON meshes pickable lights —
the mesh sampler in float64: the pick in integers, the point, direction, turned normal and pdf — and sample with the hit-side weight.
It records the margins of the `c > 0` turn, of the facing test, of the hit side's `c > 0`, and of the CDF pick (the distance of T to
the next step below and above, relative to q_k).  One-sample renders are compared sample by sample with test_path_f64's TAU /
REL_CLEAN / NEAR_TIE_MAX through test_gpu_path_f64.Tally (needs an MI355X); the two other tests need no GPU.  The statements themselves are
functions of tests/mesh_compose_f64.py, which the composed restatement (tests/test_gpu_mesh_compose_f64.py) calls as well.

Draws: 64 x 48, 200 pixels x 3 seeds x 2 scenes — scenes.mesh_light_scene() at the reference's four bounces, with the spherical
light (N = 2) and every mesh FLAT, and without it (N = 1) and every mesh SMOOTH.  The restatement alone, on the CPU, for exactly
these draws: 108 of 1 200 samples lie below TAU (9.0 %, under the 12 % cap; BELOW_TAU, which
test_the_draws_leave_enough_clean_samples counts again on every run), 775 samples carry radiance; a restatement without the hit-side
weight moves 40 clean samples beyond REL_CLEAN and one with n_lights where N belongs 264 (test_the_restatement_sees_the_weight_and_
the_count, on a scene whose lamp is eight times as wide so that paths find it by themselves).

The first 150 clean samples of each scene are also held to their own f32 tolerance (tests/f32_spread.py, through Tally.add's
spreads), computed once per scene (CASES) for the CPU and the GPU leg; this file has no tolerance of its own, and its classes
compute nothing outside pt_f64's helpers and mesh_compose_f64's functions, which carry the noise.  On the CPU
(test_the_spreads_of_the_restatement): scene 0 median spread 5.8e-7, largest 2.3e-5, 1.9 s of CPU time; scene 1 median 9.0e-7,
largest 9.9e-5, 2.5 s; no tolerance above 1e-3 in either.  Teeth (test_the_spreads_see_a_pdf_two_percent_off): the mesh light's
area pdf x 0.98 on this lights-only form leaves REL_CLEAN on no clean sample of scene 0 and its own tolerance on 34.  On an
MI355X: largest z 1.38 and 1.47 next to Z_MAX = 8.3, median z 0.31 and 0.27 next to Z_MEDIAN = 1.4, 2.8 s of
wall time for the GPU test.  Measurements, not bounds."""
import ctypes as C

import numpy as np
import pytest

import f32_spread as S
import mesh_compose_f64 as MC
import pt_f64 as P
from kernel_census import mesh_kernel_of
from test_gpu_mesh_smooth_f64 import SmoothMeshDescScene
from test_gpu_path_f64 import Tally
from test_path_f64 import NEAR_TIE_MAX, REL_CLEAN, TAU, rel_distance

LIGHT_BIT, SMOOTH_BIT, MESH_BIT = 1 << 27, 1 << 26, 1 << 25
# Counted on the CPU (test_the_draws_leave_enough_clean_samples prints the figures): samples of the 1 200 below TAU.
BELOW_TAU = 108


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


class LightMeshDescScene(SmoothMeshDescScene):
    """The scene with the meshes `smooth` SMOOTH and the meshes `on` ON."""

    def __init__(self, desc, scene, smooth=(), on=()):
        super().__init__(desc, scene)
        self.smooth_tri = np.concatenate([np.full(len(t), m in smooth) for m, (_, t, _) in enumerate(scene.meshes)])
        MC.bind_mesh_lights(self, desc, scene, on)                    # tri_ord, mesh_lights, won

    def triangle_normal(self, k, o, d, M):
        self.won = k
        if self.smooth_tri[k]:
            return super().triangle_normal(k, o, d, M)
        return MC.flat_normal(self, k)

    def closest_hit(self, o, d, st, ls, mut, M):
        self.won = None
        return super().closest_hit(o, d, st, ls, mut, M)

    def flat_normal(self, k):
        return MC.flat_normal(self, k)


class LightPath(P.Path):
    """pt_f64.Path for a LightMeshDescScene: mesh_compose_f64's statements over N = n_lights + ON meshes pickable lights.
    `no_hit_weight` and `n_lights_for_n` are the two faults the mutation check plants."""

    def __init__(self, scene, no_hit_weight=False, n_lights_for_n=False, mesh_light_pdf_scale=1.0):
        super().__init__(scene)
        self.no_hit_weight, self.n_lights_for_n = no_hit_weight, n_lights_for_n
        self.mesh_light_pdf_scale = mesh_light_pdf_scale             # (a subtle planted fault: 0.98)

    def picks(self):
        sc = self.scene
        return [("light", light) for light in sc.lights] + ([] if self.n_lights_for_n else [("mesh", j) for j in range(len(sc.mesh_lights))])

    def n_pick(self):
        return len(self.picks())

    def sample_mesh_light(self, ordinal, scatter_pos, draw, M):
        return MC.sample_mesh_light(self.scene, ordinal, float(self.n_pick()), scatter_pos, draw, M, pdf_scale=self.mesh_light_pdf_scale)

    def direct_light(self, d, st, draw, M, rays):                    # tracer.rs:126-170 over N pickable lights
        return MC.direct_light(self, d, st, draw, M, rays)

    def hit_weight(self, bounce, d, st, ss_pdf, M):
        return 1.0 if self.no_hit_weight else MC.hit_weight(self.scene, bounce, d, st, ss_pdf, self.mut, M)

    def miss(self, bounce, d, ss_pdf, M):
        return self.scene.background(d)

    def sample(self, col, row, width, height, draws):
        return MC.trace(self, col, row, width, height, draws)


def sample_many(ref, oracle, seed, pixels, w, h, **faults):
    return MC.sample_pixels(LightPath(ref, **faults), oracle, seed, pixels, w, h)


def _scenes():
    """[(what, scene, SMOOTH meshes, ON meshes)]: the lamp ON next to the spherical light with every mesh FLAT, and the lamp alone
    with every mesh SMOOTH; the reference's four bounces."""
    from rust_pathtracer_amd import scenes
    a = scenes.mesh_light_scene(sphere_light=True)
    b = scenes.mesh_light_scene()
    b.camera.origin = (0.5, 0.9, 2.8)
    a.max_depth = b.max_depth = 4
    return [("lamp and spherical light, flat", a, (), (1,)), ("lamp alone, smooth", b, (0, 1), (1,))]


def _draws():
    w, h = 64, 48
    rng = np.random.default_rng(36)
    for k, (what, s, smooth, on) in enumerate(_scenes()):
        for seed in (1, 2, 3):
            pixels = list(zip(rng.integers(0, w, 200).tolist(), rng.integers(0, h, 200).tolist()))
            yield k, what, s, smooth, on, 70 + 10 * k + seed, pixels, w, h


def _path(k):
    _, s, smooth, on = _scenes()[k]
    return LightPath(LightMeshDescScene(s.describe(), s, smooth, on))


# per scene: the restated draws and the f32 spreads of their first 150 clean samples, once for the CPU and the GPU leg
CASES = S.Cases(_path, lambda k: [(d[5], d[6]) for d in _draws() if d[0] == k])


def _one_light_sample(rpt, torch, scene, smooth, on, w, h, seed):
    t = rpt.Tracer(scene, device=0, seed=seed)
    try:
        if smooth:
            t.set_mesh_shading({m: "smooth" for m in smooth})
        t.set_mesh_lights({m: True for m in on})
        buf = rpt.DeviceColorBuffer(w, h)
        t.render_n(buf, 1)
        torch.cuda.synchronize()
        choice = C.c_uint32()
        assert rpt.lib().rpt_debug_kernel_choice(t._h, C.byref(choice)) == 0
        return buf.pixels.cpu().numpy(), choice.value
    finally:
        t.close()


@pytest.mark.gpu
def test_mesh_light_renders_against_the_restatement(rpt, oracle, torch_cuda):
    t = Tally(TAU, NEAR_TIE_MAX)
    per = None
    for n, (k, what, s, smooth, on, seed, pixels, w, h) in enumerate(_draws()):
        if n % 3 == 0:
            print("%s: the spreads took %.2f s of CPU time" % (what, CASES.spreads(oracle, k)[1]))
        frame, choice = _one_light_sample(rpt, torch_cuda, s, smooth, on, w, h, seed)
        assert choice & MESH_BIT and choice & LIGHT_BIT and bool(choice & SMOOTH_BIT) == bool(smooth), "the mesh light kernel ran"
        assert mesh_kernel_of(choice) == "meshlight_regen_kernel"
        t.ran.add(mesh_kernel_of(choice))
        seed2, pixels2, restated, margins = CASES.restated(oracle, k)[n % 3]
        assert (seed2, pixels2) == (seed, pixels)
        print("%s (seed %d): %d of %d samples below TAU" % (what, seed, int((margins <= TAU).sum()), len(margins)))
        t.add("%s (seed %d)" % (what, seed), frame, restated, margins, pixels, spreads=CASES.spreads(oracle, k)[0][n % 3])
        per = per if n % 3 else Tally(TAU, NEAR_TIE_MAX)
        per.add("%s (seed %d)" % (what, seed), frame, restated, margins, pixels, spreads=CASES.spreads(oracle, k)[0][n % 3])
        if n % 3 == 2:
            print("%s: %s" % (what, per.held.line()))
    t.check("mesh light scenes")
    assert t.n == 2 * 3 * 200


def test_the_draws_leave_enough_clean_samples(rpt, oracle):
    """The restatement alone, on the CPU, over the GPU test's own draws: no more than the project's 12 % of the samples lie below
    TAU, and the lamp matters in them (some sample's radiance comes from it)."""
    below = total = lit = 0
    for k, what, s, smooth, on, seed, pixels, w, h in _draws():
        restated, margins = sample_many(LightMeshDescScene(s.describe(), s, smooth, on), oracle, seed, pixels, w, h)
        below += int((margins <= TAU).sum())
        total += len(margins)
        lit += int((restated.max(axis=1) > 0).sum())
    print("mesh light scenes: %d of %d samples below TAU (%.2f %%), %d with radiance" % (below, total, 100.0 * below / total, lit))
    assert total == 1200 and below <= NEAR_TIE_MAX * total and lit > total // 4
    assert BELOW_TAU is None or below == BELOW_TAU


def test_the_restatement_sees_the_weight_and_the_count(rpt, oracle):
    """A restatement that omits the hit-side weight, and one that keeps n_lights where N belongs, each move more than 10 clean
    samples beyond REL_CLEAN: a device with either fault would fail the comparison above."""
    w, h = 64, 48
    pixels = [(c, r) for r in range(20, 48, 2) for c in range(8, 56, 2)]       # the floor and the object below the lamp
    _, s, smooth, on = _scenes()[0]
    v, idx, mat = s.meshes[1]                                         # a lamp eight times as wide: paths find it by themselves often enough
    centre = np.asarray(v, np.float32).mean(0)
    s.meshes[1] = ((centre + (np.asarray(v, np.float32) - centre) * np.float32(8.0)).astype(np.float32), idx, mat)
    ref = LightMeshDescScene(s.describe(), s, smooth, on)
    base, marg = sample_many(ref, oracle, 7, pixels, w, h)
    clean = marg > TAU
    for fault in ("no_hit_weight", "n_lights_for_n"):
        moved, marg2 = sample_many(ref, oracle, 7, pixels, w, h, **{fault: True})
        far = (rel_distance(np.nan_to_num(moved), np.nan_to_num(base)) > REL_CLEAN) & clean & (marg2 > TAU)
        print("%s: %d clean samples beyond REL_CLEAN" % (fault, int(far.sum())))
        assert far.sum() > 10, fault


@pytest.mark.parametrize("k", (0, 1))
def test_the_spreads_of_the_restatement(rpt, oracle, k):
    """The conditions of the comparison with spreads, on the restatement alone: at least 100 clean samples of the scene have a
    spread, and at most 5 % of them a tolerance above 1e-3."""
    CASES.conditions(oracle, _scenes()[k][0], k)


def test_the_spreads_see_a_pdf_two_percent_off(rpt, oracle):
    """The mesh light's area pdf times 0.98 on the lights-only form, rounded to f32, as a device's samples over the first scene's
    draws: no clean sample leaves REL_CLEAN, at least 10 leave their own tolerance."""
    entries, (spreads, _) = CASES.restated(oracle, 0), CASES.spreads(oracle, 0)
    ref = CASES.path(0).scene
    S.teeth("mesh light pdf x 0.98 (%s)" % _scenes()[0][0], entries, spreads,
            [sample_many(ref, oracle, seed, pixels, 64, 48, mesh_light_pdf_scale=0.98) for seed, pixels, _, _ in entries])
