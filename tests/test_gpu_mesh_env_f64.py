"""Renders under an environment held to tests/pt_f64.py, the float64 restatement of one pixel-sample (include/rpt.h, "environment
lighting").  EnvMeshDescScene is test_gpu_mesh_light_f64.LightMeshDescScene that also carries the environment: the f32 texels as
float64 and the INTEGER table (tests/test_mesh_env_host.py's restatement: the integers are the device's by construction).  EnvPath is
LightPath with the lookup, the sampler, the miss weight and N = n_lights + ON meshes + the sampled environment in float64.  Besides
the inherited margins it records the distance of s * S_f and t * S_f to a texel border, |d.y| / l1 (the lookup's fold) and py (the
sampler's), and the CDF pick's margin (the distance of T to the next step below and above, relative to q_k).  One-sample renders are
compared sample by sample with test_path_f64's TAU / REL_CLEAN / NEAR_TIE_MAX through test_gpu_path_f64.Tally (needs an MI355X);
the two other tests need no GPU.  The statements themselves are
functions of tests/mesh_compose_f64.py, which the composed restatement (tests/test_gpu_mesh_compose_f64.py) calls as well.

Draws: 64 x 48, 200 pixels x 3 seeds x 2 scenes at the reference's four bounces under scenes.mesh_env_scene(16)'s sky (16 x 16
keeps texel borders rare): the sky alone over mesh_env_scene's object with every mesh SMOOTH (N = 1), and the sky over
scenes.mesh_light_scene(sphere_light=True) with the lamp ON and every mesh FLAT (N = 3).  The restatement alone, on the CPU, for
exactly these draws: 17 of 1 200 samples lie below TAU (1.42 %, under the 12 % cap; BELOW_TAU, which
test_the_draws_leave_enough_clean_samples counts again on every run), 1 196 samples carry radiance; a restatement without the
miss-side weight moves 40 clean samples beyond REL_CLEAN and one whose N leaves the environment out 360
(test_the_restatement_sees_the_weight_and_the_count).

The first 150 clean samples of each scene are also held to their own f32 tolerance (tests/f32_spread.py, through Tally.add's
spreads), computed once per scene (CASES) for the CPU and the GPU leg; this file has no tolerance of its own, and its classes
compute nothing outside pt_f64's helpers and mesh_compose_f64's functions, which carry the noise.  On the CPU
(test_the_spreads_of_the_restatement): scene 0 median spread 3.6e-7, largest 4.6e-6, 1.9 s of CPU time; scene 1 median 4.1e-7,
largest 6.6e-6, 3.2 s; no tolerance above 1e-3 in either.  Teeth (test_the_spreads_see_the_neighbouring_row_s_pdf): the pdf of the
neighbouring texel row, under a sky that brightens by 2 % per row, leaves REL_CLEAN on no clean sample of scene 0's first 200
draws and its own tolerance on 89.  On an MI355X: largest z 1.65 and 2.27 next to Z_MAX = 8.3, median z 0.20 and 0.19
next to Z_MEDIAN = 1.4, 2.4 s of wall time for the GPU test.  Measurements, not bounds."""
import ctypes as C

import numpy as np
import pytest

import f32_spread as S
import mesh_compose_f64 as MC
from kernel_census import mesh_kernel_of
from test_gpu_mesh_light_f64 import LightMeshDescScene, LightPath
from test_gpu_path_f64 import Tally
from test_path_f64 import NEAR_TIE_MAX, REL_CLEAN, TAU, rel_distance

ENV_BIT, LIGHT_BIT, SMOOTH_BIT, MESH_BIT = 1 << 29, 1 << 27, 1 << 26, 1 << 25
ENV_SIZE = 16
# Counted on the CPU (test_the_draws_leave_enough_clean_samples prints the figures): samples of the 1 200 below TAU.
BELOW_TAU = 17


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


class EnvMeshDescScene(LightMeshDescScene):
    """The scene with the meshes `smooth` SMOOTH, the meshes `on` ON and the environment `image` times `scale`, SAMPLED or not."""

    def __init__(self, desc, scene, smooth, on, image, scale=1.0, sampled=True):
        super().__init__(desc, scene, smooth, on)
        MC.bind_environment(self, image, scale, sampled)              # env_size, env_rgb, env_cdf, env_q, env_scale, env_sampled

    def env_quantum(self, k):
        return MC.env_quantum(self, k)


class EnvPath(LightPath):
    """pt_f64.Path for an EnvMeshDescScene: mesh_compose_f64's statements with the environment as the last pickable light.
    `no_miss_weight` and `n_without_env` are the two faults the mutation check plants."""

    def __init__(self, scene, no_miss_weight=False, n_without_env=False):
        super().__init__(scene)
        self.no_miss_weight, self.n_without_env = no_miss_weight, n_without_env

    def picks(self):
        return super().picks() + ([("env", None)] if self.scene.env_sampled and not self.n_without_env else [])

    def env_pdf(self, k, p):
        return MC.env_pdf(self.scene, k, p)

    def env_lookup(self, d, M):
        return MC.env_lookup(self.scene, d, M)

    def sample_env(self, draw, M):
        return MC.sample_env(self.scene, float(self.n_pick()), draw, M)

    def miss(self, bounce, d, ss_pdf, M):
        return MC.miss(self.scene, bounce, d, ss_pdf, self.mut, M, no_weight=self.no_miss_weight)


def sample_many(ref, oracle, seed, pixels, w, h, **faults):
    return MC.sample_pixels(EnvPath(ref, **faults), oracle, seed, pixels, w, h)


def _scenes():
    """[(what, scene, SMOOTH meshes, ON meshes, image)]: the sky alone with every mesh SMOOTH (N = 1), and the sky, the spherical
    light and the lamp ON with every mesh FLAT (N = 3); the reference's four bounces."""
    from rust_pathtracer_amd import scenes
    a, image = scenes.mesh_env_scene(ENV_SIZE)
    b = scenes.mesh_light_scene(sphere_light=True)
    a.max_depth = b.max_depth = 4
    return [("the sky alone, smooth", a, (0,), (), image), ("the sky, the spherical light and the lamp, flat", b, (), (1,), image)]


def _draws():
    w, h = 64, 48
    rng = np.random.default_rng(37)
    for k, (what, s, smooth, on, image) in enumerate(_scenes()):
        for seed in (1, 2, 3):
            pixels = list(zip(rng.integers(0, w, 200).tolist(), rng.integers(0, h, 200).tolist()))
            yield k, what, s, smooth, on, image, 90 + 10 * k + seed, pixels, w, h


def _path(k):
    _, s, smooth, on, image = _scenes()[k]
    return EnvPath(EnvMeshDescScene(s.describe(), s, smooth, on, image))


# per scene: the restated draws and the f32 spreads of their first 150 clean samples, once for the CPU and the GPU leg
CASES = S.Cases(_path, lambda k: [(d[6], d[7]) for d in _draws() if d[0] == k])


def _one_env_sample(rpt, torch, scene, smooth, on, image, w, h, seed):
    t = rpt.Tracer(scene, device=0, seed=seed)
    try:
        if smooth:
            t.set_mesh_shading({m: "smooth" for m in smooth})
        if on:
            t.set_mesh_lights({m: True for m in on})
        t.set_environment(image, sampled=True)
        buf = rpt.DeviceColorBuffer(w, h)
        t.render_n(buf, 1)
        torch.cuda.synchronize()
        choice = C.c_uint32()
        assert rpt.lib().rpt_debug_kernel_choice(t._h, C.byref(choice)) == 0
        return buf.pixels.cpu().numpy(), choice.value
    finally:
        t.close()


@pytest.mark.gpu
def test_environment_renders_against_the_restatement(rpt, oracle, torch_cuda):
    t = Tally(TAU, NEAR_TIE_MAX)
    per = None
    for n, (k, what, s, smooth, on, image, seed, pixels, w, h) in enumerate(_draws()):
        if n % 3 == 0:
            print("%s: the spreads took %.2f s of CPU time" % (what, CASES.spreads(oracle, k)[1]))
        frame, choice = _one_env_sample(rpt, torch_cuda, s, smooth, on, image, w, h, seed)
        assert choice & MESH_BIT and choice & ENV_BIT and bool(choice & SMOOTH_BIT) == bool(smooth) and bool(choice & LIGHT_BIT) == bool(on)
        assert mesh_kernel_of(choice) == "meshenv_regen_kernel"
        t.ran.add(mesh_kernel_of(choice))
        seed2, pixels2, restated, margins = CASES.restated(oracle, k)[n % 3]
        assert (seed2, pixels2) == (seed, pixels)
        print("%s (seed %d): %d of %d samples below TAU" % (what, seed, int((margins <= TAU).sum()), len(margins)))
        t.add("%s (seed %d)" % (what, seed), frame, restated, margins, pixels, spreads=CASES.spreads(oracle, k)[0][n % 3])
        per = per if n % 3 else Tally(TAU, NEAR_TIE_MAX)
        per.add("%s (seed %d)" % (what, seed), frame, restated, margins, pixels, spreads=CASES.spreads(oracle, k)[0][n % 3])
        if n % 3 == 2:
            print("%s: %s" % (what, per.held.line()))
    t.check("environment scenes")
    assert t.n == 2 * 3 * 200


def test_the_draws_leave_enough_clean_samples(rpt, oracle):
    """The restatement alone, on the CPU, over the GPU test's own draws: no more than the project's 12 % of the samples lie below
    TAU, and more than a quarter of them carry radiance."""
    below = total = lit = 0
    for k, what, s, smooth, on, image, seed, pixels, w, h in _draws():
        restated, margins = sample_many(EnvMeshDescScene(s.describe(), s, smooth, on, image), oracle, seed, pixels, w, h)
        below += int((margins <= TAU).sum())
        total += len(margins)
        lit += int((restated.max(axis=1) > 0).sum())
    print("environment scenes: %d of %d samples below TAU (%.2f %%), %d with radiance" % (below, total, 100.0 * below / total, lit))
    assert total == 1200 and below <= NEAR_TIE_MAX * total and lit > total // 4
    assert BELOW_TAU is None or below == BELOW_TAU


def test_the_restatement_sees_the_weight_and_the_count(rpt, oracle):
    """A restatement without the miss-side weight, and one whose N leaves the environment out, each move more than 10 clean samples
    beyond REL_CLEAN: a device with either fault would fail the comparison above."""
    w, h = 64, 48
    pixels = [(c, r) for r in range(16, 48, 2) for c in range(8, 56, 2)]
    _, s, smooth, on, image = _scenes()[0]
    ref = EnvMeshDescScene(s.describe(), s, smooth, on, image)
    base, marg = sample_many(ref, oracle, 7, pixels, w, h)
    clean = marg > TAU
    for fault in ("no_miss_weight", "n_without_env"):
        moved, marg2 = sample_many(ref, oracle, 7, pixels, w, h, **{fault: True})
        far = (rel_distance(np.nan_to_num(moved), np.nan_to_num(base)) > REL_CLEAN) & clean & (marg2 > TAU)
        print("%s: %d clean samples beyond REL_CLEAN" % (fault, int(far.sum())))
        assert far.sum() > 10, fault


@pytest.mark.parametrize("k", (0, 1))
def test_the_spreads_of_the_restatement(rpt, oracle, k):
    """The conditions of the comparison with spreads, on the restatement alone: at least 100 clean samples of the scene have a
    spread, and at most 5 % of them a tolerance above 1e-3."""
    CASES.conditions(oracle, _scenes()[k][0], k)


def test_the_spreads_see_the_neighbouring_row_s_pdf(rpt, oracle):
    """The environment's pdf taken from the neighbouring texel row, rounded to f32, as a device's samples over the first scene's
    first draws: no clean sample leaves REL_CLEAN, at least 10 leave their own tolerance.  Under the scene's own sky, whose sun is
    a few texels, the neighbouring row's pdf is wrong by far more than a few percent; here the sky brightens by 2 % from one texel
    row to the next, and the restatement and its spreads are computed for it."""
    k, what, s, smooth, on, _, seed, pixels, w, h = next(iter(_draws()))
    rows = (1.0 + 0.02 * np.arange(ENV_SIZE))[:, None, None]
    image = np.ascontiguousarray(rows * np.array([0.5, 0.6, 0.8]) * np.ones((ENV_SIZE, ENV_SIZE, 1)), np.float32)
    good, faulty = (EnvMeshDescScene(s.describe(), s, smooth, on, image) for _ in range(2))
    faulty.env_pdf_from_next_row = True
    entries = [(seed, pixels) + sample_many(good, oracle, seed, pixels, w, h)]
    spreads, _ = S.spreads_of_draws(EnvPath(good), oracle, entries, w, h)
    S.teeth("environment pdf from the neighbouring texel row (%s)" % what, entries, spreads, [sample_many(faulty, oracle, seed, pixels, w, h)])
