"""Mesh renders held to tests/pt_f64.py, the float64 restatement of one pixel-sample, extended by the triangles of include/rpt.h
("triangle meshes"): MeshDescScene adds them to pt_f64.DescScene's closest_hit (after the planes, before Scene::sample_lights) and
any_hit, with the normal normalize(cross(e1, e2)) and the triangle's full patch, and records the branch margins of det, u, v, u + v,
t, the point check and t against the running distance.  One-sample renders at several seeds are compared sample by sample with
test_path_f64's TAU / REL_CLEAN / NEAR_TIE_MAX, as tests/test_gpu_path_f64.py does for the other classes (needs an MI355X).  The
oracle only supplies the random draws (rng_f32); it knows nothing of meshes.

The first 150 clean samples of each scene are also held to their own f32 tolerance (tests/f32_spread.py, through Tally.add's
spreads), computed once per scene (CASES) for the CPU and the GPU leg; this file has no tolerance of its own.  The flat normal,
which the device computes at the hit in f32, carries noise term by term (MeshDescScene.flat_normal).  On the CPU
(test_the_spreads_of_the_restatement): scene 0 median spread 3.3e-7, largest 2.8e-5, none with a tolerance above 1e-3, 6.8 s of CPU
time; scene 1 median 4.7e-7, 0.67 % above 1e-3 (one grazing sample of spread 0.99, capped at REL_CLEAN), 4.3 s.  Teeth
(test_the_spreads_see_a_tilted_normal): the flat normal tilted by 0.05 % of e1's direction leaves REL_CLEAN on no clean sample of
scene 0 and its own tolerance on 55; the 1 % first thought of is no subtle fault on a mirror-like icosphere and a clearcoat torus
(27 clean samples beyond REL_CLEAN; 0.2 % still 2).  On an MI355X: largest z 2.0 (scene 0) and 1.66 (scene 1) next to
Z_MAX = 8.3, median z 0.29 and 0.33 next to Z_MEDIAN = 1.4, 7.0 s of wall time for the GPU test.  Measurements, not
bounds."""
import numpy as np
import pytest

import f32_spread as S
import pt_f64 as P
from kernel_census import mesh_kernel_of
from test_gpu_path_f64 import Tally, _one_sample
from test_path_f64 import NEAR_TIE_MAX, TAU

W, H = 64, 48


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _norm(x):
    return np.sqrt((x * x).sum(-1))


class MeshDescScene(P.DescScene):
    """DescScene with the scene's triangles (flattened order: meshes in order, each mesh's triangles in order)."""

    def __init__(self, desc, scene):
        super().__init__(desc)
        tri = np.concatenate([np.asarray(v, np.float32)[np.asarray(t, np.int64)] for v, t, _ in scene.meshes]).astype(np.float64)
        self.tri_mat = np.concatenate([np.full(len(t), m) for _, t, m in scene.meshes])
        self.ta, self.e1, self.e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        lo = self.ta + np.minimum(np.minimum(0.0, self.e1), self.e2)
        hi = self.ta + np.maximum(np.maximum(0.0, self.e1), self.e2)
        self.lo, self.hi = lo, hi
        self.normal_tilt = 0.0                                        # a planted fault: the flat normal tilted by this much of e1's direction

    def flat_normal(self, k):
        """normalize(cross(e1, e2)) of triangle k's row, which the device computes at the hit in f32: under pt_f64's noise mode every
        product and every difference of the cross carries its own noise (the normalisation carries its own through P.normalize)."""
        g = np.cross(self.e1[k], self.e2[k])
        if P._NOISE is not None:
            a, b, N = self.e1[k], self.e2[k], P.noisy
            g = np.array([N(N(a[1] * b[2]) - N(a[2] * b[1])), N(N(a[2] * b[0]) - N(a[0] * b[2])), N(N(a[0] * b[1]) - N(a[1] * b[0]))])
        if self.normal_tilt:
            g = g + self.normal_tilt * np.sqrt((g * g).sum() / (self.e1[k] * self.e1[k]).sum()) * self.e1[k]
        return P.normalize(tuple(float(x) for x in g))

    def _triangles(self, o, d, M):
        """include/rpt.h's triangle test over every triangle in float64 -> (hit mask, t); records each triangle's flip margin: the
        smallest margin of its conditions when all hold, else the largest margin among those that fail."""
        o, d = np.array(o), np.array(d)
        with np.errstate(all="ignore"):
            p = np.cross(d[None, :], self.e2)
            det = (self.e1 * p).sum(-1)
            inv = 1.0 / det
            s = o[None, :] - self.ta
            u = (s * p).sum(-1) * inv
            q = np.cross(s, self.e1)
            v = (d[None, :] * q).sum(-1) * inv
            t = (self.e2 * q).sum(-1) * inv
            su = _norm(s) * _norm(p) / np.abs(det)
            sv = _norm(d)[None] * _norm(q) / np.abs(det)
            st = _norm(self.e2) * _norm(q) / np.abs(det)
            conds = [(det != 0.0, np.abs(det) / (_norm(self.e1) * _norm(p))),
                     (u >= 0.0, np.abs(u) / su), (u <= 1.0, np.abs(u - 1.0) / su),
                     (v >= 0.0, np.abs(v) / sv), (u + v <= 1.0, np.abs(u + v - 1.0) / (su + sv)),
                     (t >= 0.0, np.abs(t) / st)]
            w = (np.maximum(np.abs(self.lo), np.abs(self.hi)) + np.abs(o)[None, :]) * 2.0 ** -16
            pt = o[None, :] + t[:, None] * d[None, :]
            sp = np.abs(o)[None, :] + np.abs(t[:, None] * d[None, :]) + np.maximum(np.abs(self.lo), np.abs(self.hi)) + w
            for i in range(3):
                conds.append((self.lo[:, i] - w[:, i] <= pt[:, i], np.abs(pt[:, i] - (self.lo[:, i] - w[:, i])) / sp[:, i]))
                conds.append((pt[:, i] <= self.hi[:, i] + w[:, i], np.abs(self.hi[:, i] + w[:, i] - pt[:, i]) / sp[:, i]))
            ok = np.stack([c for c, _ in conds])
            m = np.stack([np.nan_to_num(x, nan=0.0) for _, x in conds])
            hit = ok.all(0) & (t < P.F_MAX)
            flip = np.where(hit, m.min(0), np.where(ok, -np.inf, m).max(0))
        if flip.size:
            M.m = min(M.m, float(flip.min()))
        if P._NOISE is not None:                                      # (the conditions above keep their bits; u and v: barycentrics)
            t = self.noisy_tuv(o, d)[0]
        return hit, t

    def noisy_tuv(self, o, d, k=None):
        """The triangle test's t, u and v (of triangle k, or of every triangle) under pt_f64's noise mode, as f32 rounds them: every
        product and every difference of the two crosses, of s = o - a and of the four dot products carries its own relative noise
        before the terms are added, so that a result that cancels (u, v and t are quotients of such sums: their error is relative
        to the terms, |s||p| / |det| and the like, not to the result) moves by what f32 would move it.  Relative noise on the
        results alone left a device sample 12.8 of its spreads away; see tests/test_gpu_radiance_f64.py."""
        N = P.noisy_array
        sel = slice(None) if k is None else k
        ta, e1, e2 = self.ta[sel], self.e1[sel], self.e2[sel]
        o, d = np.array(o), np.array(d)

        def cross(a, b):
            return np.stack([N(a[..., 1] * b[..., 2]) - N(a[..., 2] * b[..., 1]), N(a[..., 2] * b[..., 0]) - N(a[..., 0] * b[..., 2]),
                             N(a[..., 0] * b[..., 1]) - N(a[..., 1] * b[..., 0])], -1)

        def dot(a, b):
            x = N(a * b)
            return N(N(x[..., 0] + x[..., 1]) + x[..., 2])

        with np.errstate(all="ignore"):
            p = N(cross(d, e2))
            inv = N(1.0 / dot(e1, p))
            s = N(o - ta)
            q = N(cross(s, e1))
            return N(dot(e2, q) * inv), N(dot(s, p) * inv), N(dot(d, q) * inv)

    def closest_hit(self, o, d, st, ls, mut, M):
        """DescScene.closest_hit (spheres, then planes) with the triangles after the planes, then Scene::sample_lights."""
        dist = P.F_MAX
        hit = False
        first = True
        for c, r, m in self.spheres:
            t = P.sphere(o, d, c, r, mut, M)
            if t is not None:
                if not first:
                    M.rel(t, dist)
                if first or t < dist:
                    hp = P.add(o, P.scale(t, d))
                    st.hit_dist, st.normal = t, P.normalize(P.sub(hp, c))
                    self.patch(m, d, hp, st.material, mut, M)
                    hit, dist = True, t
            first = False
        for n, p, md, m, mt in self.planes:
            t = P.plane(o, d, n, p, md, mt, M)
            if t is not None:
                if not first:
                    M.rel(t, dist)
                if first or t < dist:
                    st.hit_dist, st.normal = t, n
                    self.patch(m, d, P.add(o, P.scale(t, d)), st.material, mut, M)
                    hit, dist = True, t
            first = False
        th, tt = self._triangles(o, d, M)
        idx = np.nonzero(th)[0]
        if idx.size:
            ts = tt[idx]
            order = np.argsort(ts, kind="stable")
            if hit:
                M.rel(float(ts[order[0]]), dist)
            if idx.size > 1:
                M.rel(float(ts[order[0]]), float(ts[order[1]]))
            k = int(idx[order[0]])                                     # least t, lowest index on ties
            t = float(tt[k])
            if t < dist:
                st.hit_dist, st.normal = t, self.flat_normal(k)
                self.patch(int(self.tri_mat[k]), d, P.add(o, P.scale(t, d)), st.material, mut, M)
                hit, dist = True, t
        if self.sample_lights(o, d, st, ls, mut, M):
            hit = True
        return hit

    def any_hit(self, o, d, max_dist, mut, M):
        if super().any_hit(o, d, max_dist, mut, M):
            return True
        use_max = bool(self.flags & P.SCENE_ANYHIT_USES_MAX_DIST)
        th, tt = self._triangles(o, d, M)
        for t in tt[th]:
            if use_max:
                M.rel(float(t), max_dist)
            if not use_max or t < max_dist:
                return True
        return False


def _scenes():
    """The mesh scene at a test size with two spheres in front of it (spheres, a plane and triangles in one closest_hit), and the
    same without spheres (the plane is then accepted whenever hit: analytical.rs's first-primitive rule) and with any_hit honouring
    max_dist."""
    from rust_pathtracer_amd import scenes
    a = scenes.mesh_scene(subdivisions=3, n_major=32, n_minor=16)
    a.materials.append(scenes.full_material(rgb=(0.2, 0.6, 0.9), roughness=0.3, clearcoat=0.5))
    a.materials.append(scenes.full_material(rgb=(0.9, 0.9, 0.9), emission=(2.0, 1.5, 1.0)))
    a.spheres = [((0.0, -0.6, 0.9), 0.35, 3), ((-0.4, 0.7, 0.6), 0.2, 4)]
    b = scenes.mesh_scene(subdivisions=2, n_major=24, n_minor=12)
    b.any_hit_uses_max_dist = True
    b.camera.origin = (0.4, 0.6, 2.6)
    return [("spheres, plane, meshes", a), ("plane and meshes, any_hit with max_dist", b)]


def _draws():
    """[(k, what, scene, seed, pixels)]: 200 random pixels x 3 seeds x 2 scenes, 64 x 48, from one generator."""
    rng = np.random.default_rng(35)
    out = []
    for k, (what, s) in enumerate(_scenes()):
        for seed in (1, 2, 3):
            out.append((k, what, s, 50 + 10 * k + seed, list(zip(rng.integers(0, W, 200).tolist(), rng.integers(0, H, 200).tolist()))))
    return out


def _path(k):
    s = _scenes()[k][1]
    return P.Path(MeshDescScene(s.describe(), s))


# per scene: the restated draws and the f32 spreads of their first 150 clean samples, once for the CPU and the GPU leg
CASES = S.Cases(_path, lambda k: [(seed, pixels) for j, _, _, seed, pixels in _draws() if j == k], W, H)


@pytest.mark.gpu
def test_mesh_renders_against_the_restatement(rpt, oracle, torch_cuda, monkeypatch):
    t = Tally(TAU, NEAR_TIE_MAX)
    for k, (what, s) in enumerate(_scenes()):
        spreads, seconds = CASES.spreads(oracle, k)
        print("%s: the spreads took %.2f s of CPU time" % (what, seconds))
        per = Tally(TAU, NEAR_TIE_MAX)
        for (seed, pixels, restated, margins), spread in zip(CASES.restated(oracle, k), spreads):
            frame, choice = _one_sample(rpt, torch_cuda, s, W, H, seed, False, monkeypatch)
            assert choice & (1 << 25), "the mesh kernel ran"
            assert mesh_kernel_of(choice) == "mesh_regen_kernel"
            t.ran.add(mesh_kernel_of(choice))
            t.add("%s (seed %d)" % (what, seed), frame, restated, margins, pixels, spreads=spread)
            per.add("%s (seed %d)" % (what, seed), frame, restated, margins, pixels, spreads=spread)
        print("%s: %s" % (what, per.held.line()))
    t.check("mesh scenes")
    assert t.n == 2 * 3 * 200


def test_the_restated_draws_are_sample_many_s(rpt, oracle):
    """The cached restatement (mesh_compose_f64.sample_pixels over pt_f64.Path) gives pt_f64.sample_many's samples and margins bit
    for bit, as this file compared them before, and the generator's draws are the ones it always made."""
    rng = np.random.default_rng(35)
    for k, (what, s) in enumerate(_scenes()):
        for j, (seed, pixels, restated, margins) in enumerate(CASES.restated(oracle, k)):
            assert pixels == list(zip(rng.integers(0, W, 200).tolist(), rng.integers(0, H, 200).tolist())) and seed == 50 + 10 * k + j + 1
            if j == 0:
                want, marg, _ = P.sample_many(CASES.path(k).scene, oracle, seed, [(c, r, 0) for c, r in pixels], W, H)
                assert np.array_equal(want, restated, equal_nan=True) and np.array_equal(marg, margins)


@pytest.mark.parametrize("k", (0, 1))
def test_the_spreads_of_the_restatement(rpt, oracle, k):
    """The conditions of the comparison with spreads, on the restatement alone: at least 100 clean samples of the scene have a
    spread, and at most 5 % of them a tolerance above 1e-3."""
    CASES.conditions(oracle, _scenes()[k][0], k)


def test_the_spreads_see_a_tilted_normal(rpt, oracle):
    """The flat normal tilted by 0.05 % of e1's direction, rounded to f32, as a device's samples over the first scene's draws: no
    clean sample leaves REL_CLEAN, at least 10 leave their own tolerance.  (On this scene's mirror-like icosphere and clearcoat torus
    a tilt of 1 % is no subtle fault: it takes 27 clean samples beyond REL_CLEAN, one of 0.2 % still 2.)"""
    from mesh_compose_f64 import sample_pixels
    s = _scenes()[0][1]
    faulty = MeshDescScene(s.describe(), s)
    faulty.normal_tilt = 0.0005
    entries, (spreads, _) = CASES.restated(oracle, 0), CASES.spreads(oracle, 0)
    S.teeth("the flat normal tilted by 0.05 %% of e1 (%s)" % _scenes()[0][0], entries, spreads,
            [sample_pixels(P.Path(faulty), oracle, seed, pixels, W, H) for seed, pixels, _, _ in entries])


@pytest.mark.gpu
def test_the_restatement_sees_the_triangles(rpt, oracle):
    """A wrong normal or material in the restatement must show: flipping the normal or giving the triangles another material moves
    the restated samples far beyond REL_CLEAN (so the comparison above would catch those faults on the device)."""
    from test_path_f64 import REL_CLEAN, rel_distance
    s = _scenes()[0][1]
    w, h = 64, 48
    pixels = [(c, r) for r in range(12, 40, 4) for c in range(4, 60, 4)]
    items = [(c, r, 0) for c, r in pixels]
    ref = MeshDescScene(s.describe(), s)
    base, marg, _ = P.sample_many(ref, oracle, 7, items, w, h)
    flipped = MeshDescScene(s.describe(), s)
    flipped.e1, flipped.e2 = flipped.e2.copy(), flipped.e1.copy()      # cross(e2, e1): the normal turned over
    moved, _, _ = P.sample_many(flipped, oracle, 7, items, w, h)
    other = MeshDescScene(s.describe(), s)
    other.tri_mat = other.tri_mat[::-1].copy()
    remat, _, _ = P.sample_many(other, oracle, 7, items, w, h)
    clean = marg > TAU
    assert (rel_distance(np.nan_to_num(moved), np.nan_to_num(base))[clean] > REL_CLEAN).sum() > 10
    assert (rel_distance(np.nan_to_num(remat), np.nan_to_num(base))[clean] > REL_CLEAN).sum() > 10
