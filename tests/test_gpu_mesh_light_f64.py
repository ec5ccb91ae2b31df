"""Renders with a mesh light held to tests/pt_f64.py, the float64 restatement of one pixel-sample (include/rpt.h, "mesh lights").
LightMeshDescScene is test_gpu_mesh_smooth_f64.SmoothMeshDescScene (per mesh FLAT or SMOOTH) that also knows which triangle won and
carries, per ON mesh, the INTEGER table (tests/test_mesh_light_host.py's restatement: the integers are the device's by construction)
and the f32 positions as float64.  LightPath is pt_f64.Path with direct_light over the N = n_lights + ON meshes pickable lights —
the mesh sampler in float64: the pick in integers, the point, direction, turned normal and pdf — and sample with the hit-side weight.
It records the margins of the `c > 0` turn, of the facing test, of the hit side's `c > 0`, and of the CDF pick (the distance of T to
the next step below and above, relative to q_k).  One-sample renders are compared sample by sample with test_path_f64's TAU /
REL_CLEAN / NEAR_TIE_MAX through test_gpu_path_f64.Tally (needs an MI355X); the two other tests need no GPU.

Draws: 64 x 48, 200 pixels x 3 seeds x 2 scenes — scenes.mesh_light_scene() at the reference's four bounces, with the spherical
light (N = 2) and every mesh FLAT, and without it (N = 1) and every mesh SMOOTH.  The restatement alone, on the CPU, for exactly
these draws: 108 of 1 200 samples lie below TAU (9.0 %, under the 12 % cap; BELOW_TAU, which
test_the_draws_leave_enough_clean_samples counts again on every run), 775 samples carry radiance; a restatement without the hit-side
weight moves 40 clean samples beyond REL_CLEAN and one with n_lights where N belongs 264 (test_the_restatement_sees_the_weight_and_
the_count, on a scene whose lamp is eight times as wide so that paths find it by themselves)."""
import bisect
import ctypes as C

import numpy as np
import pytest

import pt_f64 as P
from test_gpu_mesh_smooth_f64 import SmoothMeshDescScene
from test_gpu_path_f64 import Tally
from test_mesh_light_host import restate_table
from test_path_f64 import NEAR_TIE_MAX, REL_CLEAN, TAU, rel_distance

LIGHT_BIT, SMOOTH_BIT, MESH_BIT = 1 << 27, 1 << 26, 1 << 25
N_DRAWS = 128
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
        self.tri_ord = np.concatenate([np.full(len(t), sorted(on).index(m) if m in on else -1) for m, (_, t, _) in enumerate(scene.meshes)])
        self.mesh_lights = []                                          # ordinal -> (cdf list, Q, A_tot, corners f64 [n, 3, 3], emission)
        for m in sorted(on):
            v, t, mat = scene.meshes[m]
            cdf, _, a_tot = restate_table(v, t)
            tri = np.asarray(v, np.float32)[np.asarray(t, np.int64)].astype(np.float64)
            em = tuple(float(x) for x in desc.materials[mat].emission)
            self.mesh_lights.append(([int(c) for c in cdf], int(cdf[-1]) if len(cdf) else 0, float(a_tot), tri, em))
        self.won = None

    def triangle_normal(self, k, o, d, M):
        self.won = k
        if self.smooth_tri[k]:
            return super().triangle_normal(k, o, d, M)
        return P.normalize(tuple(float(x) for x in np.cross(self.e1[k], self.e2[k])))

    def closest_hit(self, o, d, st, ls, mut, M):
        self.won = None
        return super().closest_hit(o, d, st, ls, mut, M)

    def flat_normal(self, k):
        return P.normalize(tuple(float(x) for x in np.cross(self.e1[k], self.e2[k])))


class LightPath(P.Path):
    """pt_f64.Path for a LightMeshDescScene.  `no_hit_weight` and `n_lights_for_n` are the two faults the mutation check plants."""

    def __init__(self, scene, no_hit_weight=False, n_lights_for_n=False):
        super().__init__(scene)
        self.no_hit_weight, self.n_lights_for_n = no_hit_weight, n_lights_for_n

    def n_pick(self):
        sc = self.scene
        return len(sc.lights) if self.n_lights_for_n else len(sc.lights) + len(sc.mesh_lights)

    def sample_mesh_light(self, ordinal, scatter_pos, draw, M):
        """include/rpt.h, "sampling an ON mesh" -> (LightSampleRec, light.area)."""
        cdf, q_all, a_tot, tri, em = self.scene.mesh_lights[ordinal]
        r0a, r0b, r1, r2 = draw(), draw(), draw(), draw()
        ls = P.LightSampleRec()
        if not a_tot > 0.0:
            return ls, 0.0
        j = (int(r0a * 16777216.0) << 24) | int(r0b * 16777216.0)
        t = (j * q_all) >> 48
        k = bisect.bisect_right(cdf, t)                               # the first index with C_k > T
        below = cdf[k - 1] if k else 0
        M.of(min(t - below + 1, cdf[k] - t) / float(cdf[k] - below), 1.0)     # the pick: integer steps to the neighbours, over q_k
        a, b, c = (tuple(float(x) for x in p) for p in tri[k])
        e1, e2 = P.sub(b, a), P.sub(c, a)
        su = P.sqrt(r1)
        bu = 1.0 - su
        bv = r2 * su
        p = P.add(P.add(a, P.scale(bu, e1)), P.scale(bv, e2))
        direction = P.sub(p, scatter_pos)
        ls.dist = P.length(direction)
        dist_sq = ls.dist * ls.dist
        ls.direction = P.div3(direction, (ls.dist, ls.dist, ls.dist))
        n = P.normalize(P.cross(e1, e2))
        cs = P.dot(n, ls.direction)
        M.of(cs, 1.0)                                                 # the `c > 0` turn
        ls.normal = P.neg(n) if cs > 0.0 else n
        ls.emission = P.scale(float(self.n_pick()), em)
        ls.pdf = P.dv(dist_sq, a_tot * abs(cs))
        return ls, a_tot

    def direct_light(self, d, st, draw, M, rays):                    # tracer.rs:126-170 over N pickable lights
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
            if index < len(sc.lights):
                light = sc.lights[index]
                ls = P.sample_light(sc, light, scatter_pos, draw, M)
                if light[0] == P.LIGHT_SPHERICAL or sc.flags & P.SCENE_SAMPLE_ALL_LIGHT_TYPES:
                    ls.emission = P.scale(float(n), light[2])         # N_f takes the place of n_lights as F
                area = light[6]
            else:
                ls, area = self.sample_mesh_light(index - len(sc.lights), scatter_pos, draw, M)
            li = ls.emission
            fac = P.dot(ls.direction, ls.normal)
            M.of(fac, 1.0)                                            # the facing test
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

    def hit_weight(self, bounce, d, st, ss_pdf, M):
        """include/rpt.h, "hit side": the weight of the hit's emission term."""
        sc = self.scene
        if self.no_hit_weight or bounce == 0 or sc.won is None or sc.tri_ord[sc.won] < 0:
            return 1.0
        a_tot = sc.mesh_lights[int(sc.tri_ord[sc.won])][2]
        if not a_tot > 0.0:
            return 1.0
        cs = abs(P.dot(d, sc.flat_normal(sc.won)))
        M.of(cs, 1.0)
        if not cs > 0.0:
            return 1.0
        lp = P.dv(st.hit_dist * st.hit_dist, a_tot * cs)
        return P.power_heuristic(ss_pdf, lp, self.mut)

    def sample(self, col, row, width, height, draws):
        """pt_f64.Path.sample (its mutants left out) with the hit-side weight on the emission term."""
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
                radiance = P.add(radiance, P.mul(sc.background(d), throughput))
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
    path = LightPath(ref, **faults)
    out, marg = np.zeros((len(pixels), 3)), np.zeros(len(pixels))
    for k, (c, r) in enumerate(pixels):
        dr = oracle.rng_f32(seed, 0, int(r) * w + int(c), N_DRAWS)
        out[k], _, marg[k] = path.sample(int(c), int(r), w, h, dr)
    return out, marg


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
    refs = {}
    for k, what, s, smooth, on, seed, pixels, w, h in _draws():
        if k not in refs:
            refs[k] = LightMeshDescScene(s.describe(), s, smooth, on)
        frame, choice = _one_light_sample(rpt, torch_cuda, s, smooth, on, w, h, seed)
        assert choice & MESH_BIT and choice & LIGHT_BIT and bool(choice & SMOOTH_BIT) == bool(smooth), "the mesh light kernel ran"
        t.ran.add("meshlight_regen_kernel")
        restated, margins = sample_many(refs[k], oracle, seed, pixels, w, h)
        print("%s (seed %d): %d of %d samples below TAU" % (what, seed, int((margins <= TAU).sum()), len(margins)))
        t.add("%s (seed %d)" % (what, seed), frame, restated, margins, pixels)
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
