"""Triangle meshes on the GPU (include/rpt.h, "triangle meshes").

* The hierarchy's walks (rpt_debug_mesh_query, the device functions the mesh kernel calls) return exactly what include/rpt.h's
  ordered loop returns — t bits, triangle index, any_hit — held to a numpy float32 restatement of that loop, bit for bit, on random
  rays, rays through shared edges and vertices, axis-parallel rays, origins inside boxes and on triangles, degenerate and duplicated
  triangles (ties), rays in a triangle's plane, NaN rays, and meshes at scales 2^-20 and 2^20.
* Frames do not depend on how they are dispatched: dispatch settings, chunked launches, one-shot against resident, one context
  against a multi context with the device listed twice; Russian roulette is deterministic.
* Every error and unsupported case returns its code and leaves the previous scene rendering as before; mesh -> analytical -> mesh on
  one context gives the oracle's analytical frame.
The oracle knows nothing of meshes and is only asked about the analytical scene."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32_MAX = np.float32(3.40282347e38)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


# ---- the ordered loop of include/rpt.h in numpy float32 -----------------------------------------------------------------------
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def brute_force(tris, rays, use_max):
    """tris [T, 3, 3] f32 (flattened order), rays [N, 7] f32 -> (t bits, index or -1, any) by include/rpt.h's statements."""
    tris = tris.astype(np.float32)
    a = tris[None, :, 0]
    e1 = tris[None, :, 1] - tris[None, :, 0]
    e2 = tris[None, :, 2] - tris[None, :, 0]
    out_t = np.full(len(rays), 0x7F800000, np.uint32)
    out_i = np.full(len(rays), -1, np.int64)
    out_any = np.zeros(len(rays), np.uint32)
    with np.errstate(all="ignore"):
        for s in range(0, len(rays), 1024):
            r = rays[s:s + 1024].astype(np.float32)
            o, d, md = r[:, None, 0:3], r[:, None, 3:6], r[:, 6:7]
            d = np.broadcast_to(d, (len(r),) + e2.shape[1:])
            p = _cross(d, np.broadcast_to(e2, d.shape))
            det = _dot(np.broadcast_to(e1, d.shape), p)
            hit = (det < 0) | (det > 0)
            inv = np.float32(1.0) / det
            sv = o - a
            u = _dot(sv, p) * inv
            hit &= (u >= 0) & (u <= 1)
            q = _cross(sv, np.broadcast_to(e1, sv.shape))
            v = _dot(d, q) * inv
            hit &= (v >= 0) & (u + v <= 1)
            t = _dot(np.broadcast_to(e2, q.shape), q) * inv
            hit &= (t >= 0) & (t < F32_MAX)
            # the point check, per axis (f32; e1, e2 as the device has them)
            for i in range(3):
                ai, e1i, e2i = a[..., i], e1[..., i], e2[..., i]
                lo = ai + np.minimum(np.minimum(np.float32(0), e1i), e2i)
                hi = ai + np.maximum(np.maximum(np.float32(0), e1i), e2i)
                w = (np.maximum(np.abs(lo), np.abs(hi)) + np.abs(o[..., i])) * np.float32(2.0 ** -16)
                pi = o[..., i] + t * d[..., i]
                hit &= (lo - w <= pi) & (pi <= hi + w)
            tt = np.where(hit, t, np.float32(np.inf))
            k = np.argmin(tt, axis=1)                                  # the first of equal minima: the lowest index
            best = tt[np.arange(len(r)), k]
            got = np.isfinite(best)
            out_t[s:s + len(r)] = np.where(got, best.view(np.uint32), np.uint32(0x7F800000))
            out_i[s:s + len(r)] = np.where(got, k, -1)
            occ = hit & (t < md) if use_max else hit
            out_any[s:s + len(r)] = occ.any(axis=1)
    return out_t, out_i, out_any


def _mesh_tris(scene):
    return np.concatenate([np.asarray(v, np.float32)[np.asarray(t, np.int64)] for v, t, _ in scene.meshes])


def _query(rpt, torch, tracer, rays, flags):
    n = len(rays)
    dev = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float32)).cuda()
    out = torch.zeros(n, 3, dtype=torch.int32, device="cuda")
    rpt._lib.check(rpt.lib().rpt_debug_mesh_query(tracer._h, dev.data_ptr(), n, out.data_ptr(), flags, None), tracer._h)
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    return o[:, 0], o[:, 1].astype(np.int64) - (o[:, 1] == 0xFFFFFFFF) * (1 << 32), o[:, 2]


def _test_scene(scale=1.0):
    """Two small meshes plus degenerate and duplicated triangles: a sliver, a zero-area triangle, a triangle repeated (a tie on every
    ray that hits it), an axis-aligned quad (flat boxes)."""
    from rust_pathtracer_amd import scenes
    s = scenes.mesh_scene(subdivisions=3, n_major=24, n_minor=12)
    s.planes = []
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 0], [2, 0.001, 0]], np.float32) + np.float32([-0.5, -0.5, 0.5])
    t = np.array([[0, 1, 2], [1, 3, 2], [0, 1, 2], [0, 4, 3], [0, 1, 5], [1, 2, 0]], np.uint32)
    s.meshes.append((v, t, 1))
    s.meshes = [(np.asarray(vv, np.float32) * np.float32(scale), tt, m) for vv, tt, m in s.meshes]
    return s


def _rays(tris, n, rng, scale=1.0):
    """Random rays and the hard cases, [n, 7] f32 {o, d, max_dist}."""
    verts = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = verts.min(0), verts.max(0)
    centre, ext = 0.5 * (lo + hi), (hi - lo).max()
    parts = []
    k = n // 8
    # 1 random: origins around the scene, directions anywhere
    o = centre + rng.uniform(-2, 2, (k, 3)) * ext
    parts.append((o, rng.normal(size=(k, 3))))
    # 2 aimed at vertices (shared by up to six triangles)
    tgt = verts[rng.integers(0, len(verts), k)]
    o = centre + rng.normal(size=(k, 3)) * ext
    parts.append((o, tgt - o))
    # 3 aimed at edge midpoints (shared edges)
    tri = tris[rng.integers(0, len(tris), k)].astype(np.float64)
    j = rng.integers(0, 3, k)
    tgt = 0.5 * (tri[np.arange(k), j] + tri[np.arange(k), (j + 1) % 3])
    o = centre + rng.normal(size=(k, 3)) * ext
    parts.append((o, tgt - o))
    # 4 axis-parallel (zero direction components)
    o = centre + rng.uniform(-1, 1, (k, 3)) * ext
    d = np.zeros((k, 3))
    ax = rng.integers(0, 3, k)
    d[np.arange(k), ax] = rng.choice([-1.0, 1.0], k)
    parts.append((o, d))
    # 5 origins inside the meshes' boxes
    o = lo + rng.uniform(0, 1, (k, 3)) * (hi - lo)
    parts.append((o, rng.normal(size=(k, 3))))
    # 6 origins ON triangles (barycentric points), directions anywhere
    tri = tris[rng.integers(0, len(tris), k)].astype(np.float64)
    w = rng.dirichlet([1, 1, 1], k)
    o = (w[:, :, None] * tri).sum(1)
    parts.append((o, rng.normal(size=(k, 3))))
    # 7 grazing: along a triangle's plane through its centroid — in the plane to f32 precision (det is rounding noise: the point
    #   check decides), and 1e-6 or 1e-3 (relative) off it
    tri = tris[rng.integers(0, len(tris), k)].astype(np.float64)
    c = tri.mean(1)
    e = tri[:, 1] - tri[:, 0]
    o = c - e * rng.uniform(1, 4, (k, 1))
    off = rng.choice([0.0, 1e-6, 1e-3], (k, 1)) * np.linalg.norm(e, axis=1, keepdims=True)
    parts.append((o, e + rng.normal(size=(k, 3)) * off))
    # 8 NaN and infinite components, and huge / tiny directions
    m = n - 7 * k
    o = centre + rng.uniform(-2, 2, (m, 3)) * ext
    d = rng.normal(size=(m, 3))
    sel = rng.integers(0, 6, m)
    o[sel == 0, 0] = np.nan
    d[sel == 1, 1] = np.nan
    d[sel == 2, 2] = np.inf
    d[sel == 3] *= 1e-30
    d[sel == 4] *= 1e30
    parts.append((o, d))
    o = np.concatenate([p[0] for p in parts])
    d = np.concatenate([p[1] for p in parts])
    md = rng.uniform(0.0, 3.0, (len(o), 1)) * ext
    return np.concatenate([o, d, md], 1).astype(np.float32)


@pytest.mark.parametrize("scale_exp", [0, -20, 20])
def test_walks_equal_the_ordered_loop(rpt, torch_cuda, scale_exp):
    scale = 2.0 ** scale_exp
    s = _test_scene(scale)
    tris = _mesh_tris(s)
    rng = np.random.default_rng(1000 + scale_exp)
    rays = _rays(tris, 120_000 if scale_exp == 0 else 40_000, rng, scale)
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        for use_max in (False, True):
            want = brute_force(tris, rays, use_max)
            flags = rpt._abi.RPT_MESH_QUERY_USE_MAX if use_max else 0
            for brute in (False, True):
                got = _query(rpt, torch_cuda, t, rays, flags | (rpt._abi.RPT_MESH_QUERY_BRUTE if brute else 0))
                for name, g, w in zip(("t bits", "index", "any_hit"), got, want):
                    bad = np.nonzero(g != w)[0]
                    assert len(bad) == 0, "%s (brute %s, use_max %s): %d rays differ, first %s: got %s want %s" % (
                        name, brute, use_max, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])
        hits = want[1] >= 0
        assert hits.mean() > 0.2 and want[2].mean() > 0.05               # the sample does hit things (want: the use_max pass)
    finally:
        t.close()


def _render(rpt, torch, t, w, h, spp):
    buf = rpt.DeviceColorBuffer(w, h)
    t.render_n(buf, spp)
    torch.cuda.synchronize()
    return buf.pixels.cpu().numpy()


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _small_mesh_scene():
    from rust_pathtracer_amd import scenes
    return scenes.mesh_scene(subdivisions=4, n_major=48, n_minor=24)


def test_mesh_frames_do_not_depend_on_the_dispatch(rpt, torch_cuda):
    w, h, spp = 80, 48, 6
    s = _small_mesh_scene()
    t = rpt.Tracer(s, device=0, seed=3)
    ref = _render(rpt, torch_cuda, t, w, h, spp)
    choice = C.c_uint32(0)
    rpt._lib.check(rpt.lib().rpt_debug_kernel_choice(t._h, C.byref(choice)), t._h)
    assert choice.value & (1 << 25)
    assert np.isfinite(ref).all() and ref[..., :3].mean() > 0.01
    for disp in ((0, 12, 64, 0), (1, 0, 64, 0), (1, 1000, 1, 0), (2, 1000, 2, 7)):      # incl. chunked launches (unit_rounds 1000)
        t.set_dispatch(*disp)
        assert _same(_render(rpt, torch_cuda, t, w, h, spp), ref), disp
    t.set_dispatch(1, 12, 64, 0)
    t.render_resident(w, h, spp)
    res = t.resident_to_host(w, h).pixels.reshape(h, w, 4)
    assert _same(res, ref.reshape(h, w, 4)), "resident"
    t.close()
    m = rpt.Tracer(s, devices=[0, 0], seed=3)
    m.render_resident(w, h, spp)
    assert _same(m.resident_to_host(w, h).pixels.reshape(h, w, 4), ref.reshape(h, w, 4)), "device listed twice"
    m.close()


def test_mesh_roulette_is_deterministic(rpt, torch_cuda):
    s = _small_mesh_scene()
    s.max_depth = 8
    frames = []
    for flags in (0, rpt._abi.RPT_RENDER_RUSSIAN_ROULETTE):
        for _ in range(2):
            t = rpt.Tracer(s, device=0, seed=11)
            t.flags = flags
            frames.append(_render(rpt, torch_cuda, t, 64, 40, 4))
            t.close()
    assert _same(frames[0], frames[1]) and _same(frames[2], frames[3]) and not _same(frames[0], frames[2])


def test_mesh_analytical_mesh_on_one_context(rpt, torch_cuda, oracle):
    w, h, spp = 64, 48, 2
    s = _small_mesh_scene()
    t = rpt.Tracer(s, device=0, seed=1)
    first = _render(rpt, torch_cuda, t, w, h, spp)
    a = rpt.AnalyticalScene()
    t._scene = a
    t.upload_scene()
    got = _render(rpt, torch_cuda, t, w, h, spp)
    want = oracle.render(oracle.scene_analytical(), w, h, spp, seed=1)
    assert _same(got, want)
    t._scene = s
    t.upload_scene()
    assert _same(_render(rpt, torch_cuda, t, w, h, spp), first)
    t.close()


def test_mesh_errors_leave_the_previous_scene(rpt, torch_cuda):
    from rust_pathtracer_amd import scenes
    A = rpt._abi
    w, h, spp = 48, 32, 2
    good = _small_mesh_scene()
    t = rpt.Tracer(good, device=0, seed=2)
    ref = _render(rpt, torch_cuda, t, w, h, spp)
    v, tri = scenes.icosphere(1)

    def upload(mod):
        s = _small_mesh_scene()
        s.meshes = [(v.copy(), tri.copy(), 0)]
        mod(s)
        d = s.describe()
        return rpt.lib().rpt_upload_scene(t._h, C.byref(d))

    def bad_index(s): s.meshes[0][1][3, 1] = len(v)
    def nan_vertex(s): s.meshes[0][0][2, 0] = np.nan
    def inf_vertex(s): s.meshes[0][0][0, 2] = np.inf
    def bad_material(s): s.meshes[0] = (v, tri, len(s.materials))
    def media(s): s.media = True
    def sdf(s): s.sdf = dict(prims=[(A.RPT_SDF_SPHERE, (0.0, 0.0, 0.0), (0.5, 0.0))], material=0)
    def patch_material(s): s.meshes[0] = (v, tri, 2)                   # the checker floor's patch
    def patch_sphere(s): s.spheres.append(((0.0, 3.0, 0.0), 0.5, 2))
    cases = [(bad_index, A.RPT_ERR_INVALID_ARG), (nan_vertex, A.RPT_ERR_INVALID_ARG), (inf_vertex, A.RPT_ERR_INVALID_ARG),
             (bad_material, A.RPT_ERR_INVALID_ARG), (media, A.RPT_ERR_UNSUPPORTED), (sdf, A.RPT_ERR_UNSUPPORTED),
             (patch_material, A.RPT_ERR_UNSUPPORTED), (patch_sphere, A.RPT_ERR_UNSUPPORTED)]
    for mod, code in cases:
        assert upload(mod) == code, mod.__name__
        assert _same(_render(rpt, torch_cuda, t, w, h, spp), ref), mod.__name__
    # NULL arrays with non-zero counts
    s = _small_mesh_scene()
    d = s.describe()
    for field in ("vertices", "indices"):
        d2 = s.describe()
        me = (A.rpt_mesh * 1)(d2.meshes[0])
        setattr(me[0], field, None)
        d2.n_meshes = 1
        d2.meshes = C.cast(me, C.POINTER(A.rpt_mesh))
        assert rpt.lib().rpt_upload_scene(t._h, C.byref(d2)) == A.RPT_ERR_INVALID_ARG, field
    d.meshes = None
    assert rpt.lib().rpt_upload_scene(t._h, C.byref(d)) == A.RPT_ERR_INVALID_ARG
    assert _same(_render(rpt, torch_cuda, t, w, h, spp), ref)
    # the kernel forms a mesh scene does not have
    for flag in (A.RPT_RENDER_FAST_MATH, A.RPT_RENDER_NESTED_LOOPS, A.RPT_RENDER_SMALL_COMPACT):
        px = np.zeros(w * h * 4, np.float32)
        assert rpt.lib().rpt_render(t._h, px.ctypes.data, w, h, 0, 1, 1, flag) == A.RPT_ERR_UNSUPPORTED, flag
    assert _same(_render(rpt, torch_cuda, t, w, h, spp), ref)
    t.close()
