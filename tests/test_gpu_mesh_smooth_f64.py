"""Smooth-shaded mesh renders held to tests/pt_f64.py, the float64 restatement of one pixel-sample (include/rpt.h, "smooth mesh
shading"): SmoothMeshDescScene is test_gpu_mesh_f64.MeshDescScene with a winning triangle's normal restated — float64 vertex normals
from the f32 positions (area-weighted face vectors, summed, normalised), interpolated with the triangle test's u and v, falling back
to the flat normal — and records the margin of the `l2 > 0` branch.  One-sample renders with every mesh SMOOTH are compared sample by
sample with test_path_f64's TAU / REL_CLEAN / NEAR_TIE_MAX over test_gpu_mesh_f64's own draws (needs an MI355X).

The restatement alone, on the CPU, for exactly these draws: 131 of 1 200 samples lie below TAU (10.9 %, under the 12 % cap; the flat
restatement has 127), no vertex normal is zero, the smallest interpolated l2 is 0.92, and f32 and f64 vertex normals differ by at
most 1.3e-7.  271 clean samples differ between the flat and the smooth restatement by more than REL_CLEAN: a device that ignored the
vertex normals would fail.

The first 150 clean samples of each scene are also held to their own f32 tolerance (tests/f32_spread.py, through Tally.add's
spreads), computed once per scene (CASES) for the CPU and the GPU leg; this file has no tolerance of its own.  Under pt_f64's noise
mode the interpolation carries what the device rounds in f32: each corner's product, both sums, and the vertex normals themselves
(vertex_normal: the device's table is built in f32); with the mode off interpolated_normal keeps its bits
(test_the_noise_mode_off_keeps_the_bits).  On the CPU (test_the_spreads_of_the_restatement): scene 0 median spread 4.3e-7, largest
2.9e-4, 0.67 % with a tolerance above 1e-3, 7.3 s of CPU time; scene 1 median 6.2e-7, largest 6.6e-5, none above, 4.1 s.  Teeth
(test_the_spreads_see_a_weight_a_fifth_of_a_percent_off): u x 1.002 in the interpolation only leaves REL_CLEAN on no clean sample
of scene 0 and its own tolerance on 50; u x 1.01 takes one clean sample beyond REL_CLEAN, so it is no subtle fault here.  On an
MI355X: largest z 2.0 and 1.47 next to Z_MAX = 8.3, median z 0.29 and 0.32 next to Z_MEDIAN = 1.4, 7.5 s
of wall time for the GPU test (the flat restatement of its teeth is test_gpu_mesh_f64's cached one).  Measurements, not bounds."""
import ctypes as C

import numpy as np
import pytest

import f32_spread as S
import pt_f64 as P
from kernel_census import mesh_kernel_of
from test_gpu_mesh_f64 import MeshDescScene, _scenes
from test_gpu_path_f64 import Tally
from test_path_f64 import NEAR_TIE_MAX, REL_CLEAN, TAU, rel_distance

SMOOTH_BIT = 1 << 26
U_SCALE = 1.002                                                       # (1.01 takes one clean sample beyond REL_CLEAN: not subtle)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def vertex_normals_f64(v, idx):
    """include/rpt.h's vertex normals of one mesh in float64, from its f32 positions: [n, 3]; (0, 0, 0) where !(l2 > 0)."""
    v = np.asarray(v, np.float32).astype(np.float64)
    idx = np.asarray(idx, np.int64)
    g = np.cross(v[idx[:, 1]] - v[idx[:, 0]], v[idx[:, 2]] - v[idx[:, 0]])
    s = np.zeros_like(v)
    for k, (a, b, c) in enumerate(idx):
        for j in {int(a), int(b), int(c)}:                            # each triangle once per vertex it names
            s[j] += g[k]
    l2 = (s * s).sum(1)
    with np.errstate(all="ignore"):
        return np.where((l2 > 0.0)[:, None], s / np.sqrt(l2)[:, None], 0.0)


class SmoothMeshDescScene(MeshDescScene):
    """MeshDescScene with every mesh SMOOTH: closest_hit's triangle normal is the interpolated one."""

    def __init__(self, desc, scene):
        super().__init__(desc, scene)
        normals, corners, first = [], [], 0
        for v, t, _ in scene.meshes:
            normals.append(vertex_normals_f64(v, t))
            corners.append(np.asarray(t, np.int64) + first)
            first += len(v)
        self.vn = np.concatenate(normals)
        self.corner = np.concatenate(corners)
        self.l2_min = np.inf
        self.u_scale = 1.0                                            # a planted fault: the weight u times this in the interpolation only

    def barycentrics(self, k, o, d):
        """The triangle test's own u and v for this ray and triangle k, recomputed."""
        o, d = np.array(o), np.array(d)
        p = np.cross(d, self.e2[k])
        inv = 1.0 / float((self.e1[k] * p).sum())
        s = o - self.ta[k]
        u = float((s * p).sum()) * inv
        v = float((d * np.cross(s, self.e1[k])).sum()) * inv
        if P._NOISE is not None:
            _, u, v = (float(x) for x in self.noisy_tuv(o, d, k))
        return u, v

    def triangle_normal(self, k, o, d, M):
        return self.interpolated_normal(k, *self.barycentrics(k, o, d), M)

    def interpolated_normal(self, k, u, v, M):
        """include/rpt.h, "normal of a winning triangle of a SMOOTH mesh", at the barycentrics u, v of triangle k."""
        na, nb, nc = (self.vertex_normal(j) for j in self.corner[k])
        u = u * self.u_scale
        m = P.noisy_array(P.noisy_array(P.noisy_array(((1.0 - u) - v) * na) + P.noisy_array(u * nb)) + P.noisy_array(v * nc))
        l2 = float((m * m).sum())
        M.of(l2, 1.0)                                                 # the `l2 > 0` branch: the corners' normals are unit vectors
        self.l2_min = min(self.l2_min, l2)
        if l2 > 0.0 and l2 <= P.F_MAX:
            return P.normalize(tuple(float(x) for x in m))
        return self.flat_normal(k)

    def vertex_normal(self, j):
        """Vertex j's normal.  The device builds it in f32 — the faces' crosses, their sum, the normalisation — so under pt_f64's
        noise mode it carries one relative noise for each of the three (the table's own error, drawn again per sample: what is
        measured is the sample's sensitivity to it)."""
        return P.noisy_array(P.noisy_array(P.noisy_array(self.vn[j])))

    def closest_hit(self, o, d, st, ls, mut, M):
        """MeshDescScene.closest_hit with the winning triangle's normal replaced."""
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
                st.hit_dist, st.normal = t, self.triangle_normal(k, o, d, M)
                self.patch(int(self.tri_mat[k]), d, P.add(o, P.scale(t, d)), st.material, mut, M)
                hit, dist = True, t
        if self.sample_lights(o, d, st, ls, mut, M):
            hit = True
        return hit


def _one_smooth_sample(rpt, torch, scene, w, h, seed):
    """A one-sample render with every mesh SMOOTH into a fresh buffer -> (frame, kernel choice)."""
    t = rpt.Tracer(scene, device=0, seed=seed)
    try:
        t.set_mesh_shading({m: "smooth" for m in range(len(scene.meshes))})
        buf = rpt.DeviceColorBuffer(w, h)
        t.render_n(buf, 1)
        torch.cuda.synchronize()
        choice = C.c_uint32()
        assert rpt.lib().rpt_debug_kernel_choice(t._h, C.byref(choice)) == 0
        return buf.pixels.cpu().numpy(), choice.value
    finally:
        t.close()


def _draws():
    """test_gpu_mesh_f64's own draws: default_rng(35), seeds 50 + 10k + seed, 200 pixels each, 64 x 48."""
    w, h = 64, 48
    rng = np.random.default_rng(35)
    for k, (what, s) in enumerate(_scenes()):
        for seed in (1, 2, 3):
            pixels = list(zip(rng.integers(0, w, 200).tolist(), rng.integers(0, h, 200).tolist()))
            yield k, what, s, 50 + 10 * k + seed, pixels, w, h


def _path(k):
    s = _scenes()[k][1]
    return P.Path(SmoothMeshDescScene(s.describe(), s))


# per scene: the restated draws and the f32 spreads of their first 150 clean samples, once for the CPU and the GPU leg
CASES = S.Cases(_path, lambda k: [(seed, pixels) for j, _, _, seed, pixels, _, _ in _draws() if j == k])


@pytest.mark.gpu
def test_smooth_mesh_renders_against_the_restatement(rpt, oracle, torch_cuda):
    from test_gpu_mesh_f64 import CASES as FLAT_CASES                 # the flat restatement of the same draws, shared with that file
    t = Tally(TAU, NEAR_TIE_MAX)
    differ = 0
    refs, per = {}, None
    for n, (k, what, s, seed, pixels, w, h) in enumerate(_draws()):
        if k not in refs:
            refs[k] = CASES.path(k).scene
            assert refs[k].vn.any(axis=1).all(), "no vertex normal is zero"
            print("%s: the spreads took %.2f s of CPU time" % (what, CASES.spreads(oracle, k)[1]))
        frame, choice = _one_smooth_sample(rpt, torch_cuda, s, w, h, seed)
        assert choice & (1 << 25) and choice & SMOOTH_BIT, "the smooth mesh kernel ran"
        assert mesh_kernel_of(choice) == "meshsmooth_regen_kernel"
        t.ran.add(mesh_kernel_of(choice))
        seed2, pixels2, restated, margins = CASES.restated(oracle, k)[n % 3]
        assert (seed2, pixels2) == (seed, pixels)
        print("%s (seed %d): %d of %d samples below TAU" % (what, seed, int((margins <= TAU).sum()), len(margins)))
        t.add("%s, smooth (seed %d)" % (what, seed), frame, restated, margins, pixels, spreads=CASES.spreads(oracle, k)[0][n % 3])
        per = per if n % 3 else Tally(TAU, NEAR_TIE_MAX)
        per.add("%s, smooth (seed %d)" % (what, seed), frame, restated, margins, pixels, spreads=CASES.spreads(oracle, k)[0][n % 3])
        if n % 3 == 2:
            print("%s: %s" % (what, per.held.line()))
        # teeth: where the flat restatement lands elsewhere, a device that ignored the vertex normals would have failed above
        seed3, pixels3, flat_restated, flat_margins = FLAT_CASES.restated(oracle, k)[n % 3]
        assert (seed3, pixels3) == (seed, pixels)
        clean = (margins > TAU) & (flat_margins > TAU)
        differ += int((rel_distance(np.nan_to_num(flat_restated), np.nan_to_num(restated))[clean] > REL_CLEAN).sum())
    t.check("smooth mesh scenes")
    print("smallest interpolated l2 %.3g; %d clean samples differ between the flat and the smooth restatement" % (
        min(r.l2_min for r in refs.values()), differ))
    assert t.n == 2 * 3 * 200
    assert min(r.l2_min for r in refs.values()) > 0.5
    assert differ > 50


@pytest.mark.parametrize("k", (0, 1))
def test_the_spreads_of_the_restatement(rpt, oracle, k):
    """The conditions of the comparison with spreads, on the restatement alone: at least 100 clean samples of the scene have a
    spread, and at most 5 % of them a tolerance above 1e-3."""
    CASES.conditions(oracle, _scenes()[k][0] + ", smooth", k)


def test_the_spreads_see_a_weight_a_fifth_of_a_percent_off(rpt, oracle):
    """The barycentric weight u times 1.002 in the normal interpolation only, rounded to f32, as a device's samples over the first
    scene's draws: no clean sample leaves REL_CLEAN, at least 10 leave their own tolerance."""
    from mesh_compose_f64 import sample_pixels
    s = _scenes()[0][1]
    faulty = SmoothMeshDescScene(s.describe(), s)
    faulty.u_scale = U_SCALE
    entries, (spreads, _) = CASES.restated(oracle, 0), CASES.spreads(oracle, 0)
    S.teeth("u x %g in the normal interpolation (%s)" % (U_SCALE, _scenes()[0][0]), entries, spreads,
            [sample_pixels(P.Path(faulty), oracle, seed, pixels, 64, 48) for seed, pixels, _, _ in entries])


def test_the_noise_mode_off_keeps_the_bits(rpt, oracle):
    """With the noise mode off the interpolated normal is the plain float64 expression's, bit for bit."""
    s = _scenes()[1][1]
    sc = CASES.path(1).scene
    rng = np.random.default_rng(3)
    for k in rng.integers(0, len(sc.corner), 50):
        u, v = rng.uniform(0, 0.5, 2)
        na, nb, nc = (sc.vn[j] for j in sc.corner[k])
        m = ((1.0 - u) - v) * na + u * nb + v * nc
        assert sc.interpolated_normal(int(k), float(u), float(v), P.Margin()) == P.normalize(tuple(float(x) for x in m))
