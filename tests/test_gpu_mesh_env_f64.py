"""Renders under an environment held to tests/pt_f64.py, the float64 restatement of one pixel-sample (include/rpt.h, "environment
lighting").  EnvMeshDescScene is test_gpu_mesh_light_f64.LightMeshDescScene that also carries the environment: the f32 texels as
float64 and the INTEGER table (tests/test_mesh_env_host.py's restatement: the integers are the device's by construction).  EnvPath is
LightPath with the lookup, the sampler, the miss weight and N = n_lights + ON meshes + the sampled environment in float64.  Besides
the inherited margins it records the distance of s * S_f and t * S_f to a texel border, |d.y| / l1 (the lookup's fold) and py (the
sampler's), and the CDF pick's margin (the distance of T to the next step below and above, relative to q_k).  One-sample renders are
compared sample by sample with test_path_f64's TAU / REL_CLEAN / NEAR_TIE_MAX through test_gpu_path_f64.Tally (needs an MI355X);
the two other tests need no GPU.

Draws: 64 x 48, 200 pixels x 3 seeds x 2 scenes at the reference's four bounces under scenes.mesh_env_scene(16)'s sky (16 x 16
keeps texel borders rare): the sky alone over mesh_env_scene's object with every mesh SMOOTH (N = 1), and the sky over
scenes.mesh_light_scene(sphere_light=True) with the lamp ON and every mesh FLAT (N = 3).  The restatement alone, on the CPU, for
exactly these draws: 17 of 1 200 samples lie below TAU (1.42 %, under the 12 % cap; BELOW_TAU, which
test_the_draws_leave_enough_clean_samples counts again on every run), 1 196 samples carry radiance; a restatement without the
miss-side weight moves 40 clean samples beyond REL_CLEAN and one whose N leaves the environment out 360
(test_the_restatement_sees_the_weight_and_the_count)."""
import bisect
import ctypes as C
import math

import numpy as np
import pytest

import pt_f64 as P
from test_gpu_mesh_light_f64 import N_DRAWS, LightMeshDescScene, LightPath
from test_gpu_path_f64 import Tally
from test_mesh_env_host import restate_table
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


def _sgn(x):
    return 1.0 if x >= 0.0 else -1.0


class EnvMeshDescScene(LightMeshDescScene):
    """The scene with the meshes `smooth` SMOOTH, the meshes `on` ON and the environment `image` times `scale`, SAMPLED or not."""

    def __init__(self, desc, scene, smooth, on, image, scale=1.0, sampled=True):
        super().__init__(desc, scene, smooth, on)
        texels, cdf, _ = restate_table(image, sampled)
        self.env_size = int(np.asarray(image).shape[0])
        self.env_rgb = [tuple(float(x) for x in c[:3]) for c in texels]
        self.env_cdf = [int(c) for c in cdf]
        self.env_q = self.env_cdf[-1] if sampled else 0
        self.env_scale = float(np.float32(scale))
        self.env_sampled = bool(sampled)

    def env_quantum(self, k):
        return self.env_cdf[k] - (self.env_cdf[k - 1] if k else 0)


class EnvPath(LightPath):
    """pt_f64.Path for an EnvMeshDescScene.  `no_miss_weight` and `n_without_env` are the two faults the mutation check plants."""

    def __init__(self, scene, no_miss_weight=False, n_without_env=False):
        super().__init__(scene)
        self.no_miss_weight, self.n_without_env = no_miss_weight, n_without_env

    def n_pick(self):
        sc = self.scene
        return len(sc.lights) + len(sc.mesh_lights) + (1 if sc.env_sampled and not self.n_without_env else 0)

    def env_pdf(self, k, p):
        sc = self.scene
        s_f = float(sc.env_size)
        l2 = P.dot(p, p)
        ln = P.sqrt(l2)
        sel = P.dv(float(sc.env_quantum(k)), float(sc.env_q))
        return (sel * ((s_f * s_f) * 0.25)) * (l2 * ln), ln

    def env_lookup(self, d, M):
        """include/rpt.h, "lookup of a direction" -> (k or None, radiance, p before the fold)."""
        sc = self.scene
        size, s_f = sc.env_size, float(sc.env_size)
        l1 = (abs(d[0]) + abs(d[1])) + abs(d[2])
        if not (l1 > 0.0 and l1 <= 3.40282347e+38):
            return None, P.ZERO3, P.ZERO3
        px, pz = d[0] / l1, d[2] / l1
        p = (px, d[1] / l1, pz)
        M.of(p[1], 1.0)                                               # the fold: d.y < 0
        if d[1] < 0.0:
            px, pz = (1.0 - abs(pz)) * _sgn(px), (1.0 - abs(px)) * _sgn(pz)
        idx = []
        for x in (px * 0.5 + 0.5, pz * 0.5 + 0.5):
            xs = x * s_f
            border = round(xs)
            if 1 <= border <= size - 1:
                M.of(xs - border, 1.0)                                # a texel border
            idx.append(min(int(math.floor(xs)), size - 1))
        k = idx[1] * size + idx[0]
        return k, P.scale(sc.env_scale, sc.env_rgb[k]), p

    def sample_env(self, draw, M):
        """include/rpt.h, "sampling from scatter_pos" -> (LightSampleRec, light.area)."""
        sc = self.scene
        r0a, r0b, r1, r2 = draw(), draw(), draw(), draw()
        ls = P.LightSampleRec()
        if sc.env_q == 0:
            return ls, 1.0
        size, s_f = sc.env_size, float(sc.env_size)
        j = (int(r0a * 16777216.0) << 24) | int(r0b * 16777216.0)
        t = (j * sc.env_q) >> 48
        k = bisect.bisect_right(sc.env_cdf, t)                        # the first index with C_k > T
        below = sc.env_cdf[k - 1] if k else 0
        M.of(min(t - below + 1, sc.env_cdf[k] - t) / float(sc.env_cdf[k] - below), 1.0)
        s, tt = (float(k % size) + r1) / s_f, (float(k // size) + r2) / s_f
        px, pz = s * 2.0 - 1.0, tt * 2.0 - 1.0
        py = (1.0 - abs(px)) - abs(pz)
        M.of(py, 1.0)                                                 # the sampler's fold
        if py < 0.0:
            px, pz = (1.0 - abs(pz)) * _sgn(px), (1.0 - abs(px)) * _sgn(pz)
        p = (px, py, pz)
        ls.pdf, ln = self.env_pdf(k, p)
        ls.direction = P.div3(p, (ln, ln, ln))
        ls.normal = P.neg(ls.direction)
        ls.dist = P.INF
        ls.emission = P.scale(float(self.n_pick()), P.scale(sc.env_scale, sc.env_rgb[k]))
        return ls, 1.0

    def direct_light(self, d, st, draw, M, rays):                    # LightPath's, with the environment as the last pickable light
        sc, mut = self.scene, self.mut
        ld = P.ZERO3
        scatter_pos = P.add(st.fhp, P.scale(self.eps, st.ffnormal))
        n = self.n_pick()
        if n > 0:
            random = draw() * float(n)
            k = round(random)
            if 1 <= k <= n - 1:
                M.rel(random, float(k))
            index = min(int(random), n - 1)
            n_mesh = len(sc.lights) + len(sc.mesh_lights)
            if index < len(sc.lights):
                light = sc.lights[index]
                ls = P.sample_light(sc, light, scatter_pos, draw, M)
                if light[0] == P.LIGHT_SPHERICAL or sc.flags & P.SCENE_SAMPLE_ALL_LIGHT_TYPES:
                    ls.emission = P.scale(float(n), light[2])
                area = light[6]
            elif index < n_mesh:
                ls, area = self.sample_mesh_light(index - len(sc.lights), scatter_pos, draw, M)
            else:
                ls, area = self.sample_env(draw, M)
            li = ls.emission
            fac = P.dot(ls.direction, ls.normal)
            M.of(fac, 1.0)
            if fac < 0.0:
                max_dist = ls.dist - self.eps
                rays.append(scatter_pos + ls.direction + (max_dist,))
                if not sc.any_hit(scatter_pos, ls.direction, max_dist, mut, M):
                    f, pdf = P.disney_eval(st.material, st.eta, P.neg(d), st.ffnormal, ls.direction, mut, M)
                    mis = 1.0
                    if area > 0.0:
                        mis = P.power_heuristic(ls.pdf, pdf, mut)
                    if pdf > 0.0:
                        ld = P.add(ld, P.scale(mis, P.mul(li, P.div3(f, (ls.pdf, ls.pdf, ls.pdf)))))
        return ld

    def miss(self, bounce, d, ss_pdf, M):
        """include/rpt.h, "miss side": w * radiance(d)."""
        sc = self.scene
        k, rad, p = self.env_lookup(d, M)
        w = 1.0
        if not (self.no_miss_weight or bounce == 0 or k is None or sc.env_q == 0 or sc.env_quantum(k) == 0):
            lp, _ = self.env_pdf(k, p)
            if lp != 0.0:
                w = P.power_heuristic(ss_pdf, lp, self.mut)
        return P.scale(w, rad)

    def sample(self, col, row, width, height, draws):
        """LightPath.sample with the miss side."""
        assert not self.mut and not self.roulette
        sc, mut = self.scene, self.mut
        M = P.Margin()
        rays = []
        it = iter(draws)
        draw = lambda: float(next(it))                                # noqa: E731
        j = height - 1 - row
        x = float(col)
        y = float(height) - float(j)
        a = draw()
        b = draw()
        o, d = P.gen_ray(sc.cam, (x / width, 1.0 - y / height), (a, b), float(width), float(height))
        radiance = P.ZERO3
        throughput = P.ONE3
        st = P.State()
        ls = P.LightSampleRec()
        ss_l, ss_pdf = P.ZERO3, 0.0
        depth = sc.depth
        for bounce in range(depth):
            st.material = P.Material(1.5)
            rays.append(o + d + (-1.0,))
            if not sc.closest_hit(o, d, st, ls, mut, M):
                radiance = P.add(radiance, P.mul(self.miss(bounce, d, ss_pdf, M), throughput))
                break
            st.fhp = P.add(o, P.scale(st.hit_dist, d))
            nd = P.dot(st.normal, d)
            M.of(nd, 1.0)
            st.ffnormal = st.normal if nd <= 0.0 else P.neg(st.normal)
            st.material.finalize()
            st.eta = P.dv(1.0, st.material.ior) if nd < 0.0 else st.material.ior
            w = self.hit_weight(bounce, d, st, ss_pdf, M)
            radiance = P.add(radiance, P.mul(P.scale(w, st.material.emission), throughput))
            if st.is_emitter:
                mis = P.power_heuristic(ss_pdf, ls.pdf, mut) if depth > 0 else 1.0
                radiance = P.add(radiance, P.mul(P.scale(mis, ls.emission), throughput))
                break
            radiance = P.add(radiance, P.mul(self.direct_light(d, st, draw, M, rays), throughput))
            f, ss_l, ss_pdf = P.disney_sample(st.material, st.eta, P.neg(d), st.ffnormal, ss_l, draw, mut, M)
            if ss_pdf > 0.0:
                throughput = P.mul(throughput, P.div3(f, (ss_pdf, ss_pdf, ss_pdf)))
            else:
                break
            d = ss_l
            o = P.add(st.fhp, P.scale(self.eps, d))
        return radiance, rays, M.m


def sample_many(ref, oracle, seed, pixels, w, h, **faults):
    path = EnvPath(ref, **faults)
    out, marg = np.zeros((len(pixels), 3)), np.zeros(len(pixels))
    for k, (c, r) in enumerate(pixels):
        dr = oracle.rng_f32(seed, 0, int(r) * w + int(c), N_DRAWS)
        out[k], _, marg[k] = path.sample(int(c), int(r), w, h, dr)
    return out, marg


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
    refs = {}
    for k, what, s, smooth, on, image, seed, pixels, w, h in _draws():
        if k not in refs:
            refs[k] = EnvMeshDescScene(s.describe(), s, smooth, on, image)
        frame, choice = _one_env_sample(rpt, torch_cuda, s, smooth, on, image, w, h, seed)
        assert choice & MESH_BIT and choice & ENV_BIT and bool(choice & SMOOTH_BIT) == bool(smooth) and bool(choice & LIGHT_BIT) == bool(on)
        t.ran.add("meshenv_regen_kernel")
        restated, margins = sample_many(refs[k], oracle, seed, pixels, w, h)
        print("%s (seed %d): %d of %d samples below TAU" % (what, seed, int((margins <= TAU).sum()), len(margins)))
        t.add("%s (seed %d)" % (what, seed), frame, restated, margins, pixels)
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
