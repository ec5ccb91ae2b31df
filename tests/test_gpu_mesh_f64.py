"""Mesh renders held to tests/pt_f64.py, the float64 restatement of one pixel-sample, extended by the triangles of include/rpt.h
("triangle meshes"): MeshDescScene adds them to pt_f64.DescScene's closest_hit (after the planes, before Scene::sample_lights) and
any_hit, with the normal normalize(cross(e1, e2)) and the triangle's full patch, and records the branch margins of det, u, v, u + v,
t, the point check and t against the running distance.  One-sample renders at several seeds are compared sample by sample with
test_path_f64's TAU / REL_CLEAN / NEAR_TIE_MAX, as tests/test_gpu_path_f64.py does for the other classes (needs an MI355X).  The
oracle only supplies the random draws (rng_f32); it knows nothing of meshes."""
import numpy as np
import pytest

import pt_f64 as P
from kernel_census import mesh_kernel_of
from test_gpu_path_f64 import Tally, _one_sample
from test_path_f64 import NEAR_TIE_MAX, TAU

pytestmark = pytest.mark.gpu


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
                n = P.normalize(tuple(float(x) for x in np.cross(self.e1[k], self.e2[k])))
                st.hit_dist, st.normal = t, n
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


def test_mesh_renders_against_the_restatement(rpt, oracle, torch_cuda, monkeypatch):
    w, h = 64, 48
    rng = np.random.default_rng(35)
    t = Tally(TAU, NEAR_TIE_MAX)
    for k, (what, s) in enumerate(_scenes()):
        ref = MeshDescScene(s.describe(), s)
        for seed in (1, 2, 3):
            pixels = list(zip(rng.integers(0, w, 200).tolist(), rng.integers(0, h, 200).tolist()))
            frame, choice = _one_sample(rpt, torch_cuda, s, w, h, 50 + 10 * k + seed, False, monkeypatch)
            assert choice & (1 << 25), "the mesh kernel ran"
            assert mesh_kernel_of(choice) == "mesh_regen_kernel"
            t.ran.add(mesh_kernel_of(choice))
            restated, margins, _ = P.sample_many(ref, oracle, 50 + 10 * k + seed, [(c, r, 0) for c, r in pixels], w, h)
            t.add("%s (seed %d)" % (what, 50 + 10 * k + seed), frame, restated, margins, pixels)
    t.check("mesh scenes")
    assert t.n == 2 * 3 * 200


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
