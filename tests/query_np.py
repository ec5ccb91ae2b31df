"""Ray queries restated in numpy float32 (include/rpt.h, "ray queries"): the ordered loop of "triangle meshes" over spheres, planes
and the flattened triangles, carrying u, v and the winner rule, and its any-hit with a per-ray max_dist.  Sphere and plane distances
follow oracle/rpt_oracle.hpp's operation order (hit_sphere, hit_plane): every product, sum, divide and root is one float32 operation
of numpy, in that order.  mesh_test_scene and mesh_rays are tests/test_gpu_mesh.py's _test_scene and _rays, copied.

A NaN distance.  A ray with a NaN or infinite component can make the FIRST sphere's test return a NaN that the "first primitive"
rule accepts.  IEEE 754 leaves a NaN's sign and payload to the implementation, so compare_words treats two NaN distances as equal
and every other word bit for bit."""
import ctypes as C

import numpy as np

F = np.float32
F32_MAX = F(3.40282347e38)
INF_BITS, NONE = 0x7F800000, 0xFFFFFFFF
HIT_NONE, HIT_SPHERE, HIT_PLANE, HIT_TRIANGLE = range(4)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def mesh_tris(scene):
    return np.concatenate([np.asarray(v, F)[np.asarray(t, np.int64)] for v, t, _ in scene.meshes])


def mesh_test_scene(scale=1.0):
    """Two small meshes plus degenerate and duplicated triangles: a sliver, a zero-area triangle, a triangle repeated (a tie on every
    ray that hits it), an axis-aligned quad (flat boxes)."""
    from rust_pathtracer_amd import scenes
    s = scenes.mesh_scene(subdivisions=3, n_major=24, n_minor=12)
    s.planes = []
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 0], [2, 0.001, 0]], F) + F([-0.5, -0.5, 0.5])
    t = np.array([[0, 1, 2], [1, 3, 2], [0, 1, 2], [0, 4, 3], [0, 1, 5], [1, 2, 0]], np.uint32)
    s.meshes.append((v, t, 1))
    s.meshes = [(np.asarray(vv, F) * F(scale), tt, m) for vv, tt, m in s.meshes]
    return s


def query_scene(scale=1.0):
    """mesh_test_scene plus two spheres and one plane with max_t > 0 that cut through the meshes, all scaled by `scale` (a power of two:
    the products are exact).  Spheres take full materials (0 and 1), the plane the checker floor's patch (2)."""
    s = mesh_test_scene(scale)
    k = F(scale)
    s.spheres = [(tuple(F([0.1, 0.95, 0.3]) * k), float(F(0.75) * k), 1), (tuple(F([-0.4, -1.0, -0.5]) * k), float(F(0.85) * k), 0)]
    s.planes = [((0.0, 1.0, 0.0), tuple(F([0.0, -0.35, 0.0]) * k), 0.0001, 2, float(F(5.0) * k))]
    return s


def mesh_rays(tris, n, rng, scale=1.0):
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
    return np.concatenate([o, d, md], 1).astype(F)


def unit_directions(r7):
    """The rays with their directions normalised (in float64, rounded once) where the length is finite and neither tiny nor huge: the
    sphere test assumes a unit direction, as the integrator's rays have; the NaN, infinite, 1e-30 and 1e30 kinds stay as they are."""
    r7 = np.array(r7, F, copy=True)
    d = r7[:, 3:6].astype(np.float64)
    with np.errstate(all="ignore"):
        length = np.sqrt((d * d).sum(1))
        ok = np.isfinite(length) & (length > 1e-20) & (length < 1e20)
        r7[ok, 3:6] = (d[ok] / length[ok, None]).astype(F)
    return r7


def big_case(scale_exp, n=40_000):
    """-> (scene, rays [n, 7], which rays were normalised): query_scene at 2^scale_exp and `n` rays of every kind of mesh_rays.  Three
    rays in four get a unit direction, as the integrator's rays have — the sphere test assumes one, so only there do spheres answer
    for the geometry —; every fourth keeps the direction mesh_rays gave it (lengths from 1e-30 to 1e30: rpt_ray's direction is taken
    as it comes), and so do the NaN, infinite, tiny and huge kinds."""
    scale = 2.0 ** scale_exp
    s = query_scene(scale)
    raw = mesh_rays(mesh_tris(s), n, np.random.default_rng(7000 + scale_exp), scale)
    r7 = unit_directions(raw)
    keep = np.arange(n) % 4 == 3
    r7[keep] = raw[keep]
    with np.errstate(all="ignore"):
        length = np.sqrt((r7[:, 3:6].astype(np.float64) ** 2).sum(1))
    return s, r7, ~keep & (np.abs(length - 1.0) < 1e-3)


def to_rpt_rays(r7):
    """[n, 7] {o, d, max_dist} -> [n, 8] rpt_ray words {origin, max_dist, direction, reserved}."""
    r7 = np.asarray(r7, F)
    out = np.zeros((len(r7), 8), F)
    out[:, 0:3], out[:, 3], out[:, 4:7] = r7[:, 0:3], r7[:, 6], r7[:, 3:6]
    return out


def hit_sphere(o, d, centre, radius):
    """rpt_oracle.hpp's hit_sphere, per ray -> (hit, t)."""
    l = F(centre)[None, :] - o
    tca = dot(l, d)
    d2 = dot(l, l) - tca * tca
    radius2 = F(radius) * F(radius)
    miss = d2 > radius2
    thc = np.sqrt(radius2 - d2)
    t0, t1 = tca - thc, tca + thc
    swap = t0 > t1
    t0, t1 = np.where(swap, t1, t0), np.where(swap, t0, t1)
    neg = t0 < 0
    t0 = np.where(neg, t1, t0)
    miss = miss | (neg & (t0 < 0))
    return ~miss, t0.astype(F)


def hit_plane(o, d, normal, point, min_denom, max_t):
    """rpt_oracle.hpp's hit_plane with the project's max_t, per ray -> (hit, t)."""
    n = F(normal)[None, :]
    denom = dot(np.broadcast_to(n, d.shape), d)
    tt = dot(F(point)[None, :] - o, np.broadcast_to(n, d.shape)) / denom
    hit = (np.abs(denom) > F(min_denom)) & (tt >= 0)
    if F(max_t) > 0:
        hit = hit & (tt <= F(max_t))
    return hit, tt.astype(F)


def triangles(tris, o, d):
    """include/rpt.h's triangle test of every ray against every triangle -> (hit, t, u, v), each [n, T]."""
    a = tris[None, :, 0]
    e1 = tris[None, :, 1] - tris[None, :, 0]
    e2 = tris[None, :, 2] - tris[None, :, 0]
    o, d = o[:, None, :], d[:, None, :]
    d = np.broadcast_to(d, (d.shape[0],) + e2.shape[1:])
    p = cross(d, np.broadcast_to(e2, d.shape))
    det = dot(np.broadcast_to(e1, d.shape), p)
    hit = (det < 0) | (det > 0)
    inv = F(1.0) / det
    sv = o - a
    u = dot(sv, p) * inv
    hit &= (u >= 0) & (u <= 1)
    q = cross(sv, np.broadcast_to(e1, sv.shape))
    v = dot(d, q) * inv
    hit &= (v >= 0) & (u + v <= 1)
    t = dot(np.broadcast_to(e2, q.shape), q) * inv
    hit &= (t >= 0) & (t < F32_MAX)
    for i in range(3):                                               # the point check, per axis
        ai, e1i, e2i = a[..., i], e1[..., i], e2[..., i]
        lo = ai + np.minimum(np.minimum(F(0), e1i), e2i)
        hi = ai + np.maximum(np.maximum(F(0), e1i), e2i)
        w = (np.maximum(np.abs(lo), np.abs(hi)) + np.abs(o[..., i])) * F(2.0 ** -16)
        pi = o[..., i] + t * d[..., i]
        hit &= (lo - w <= pi) & (pi <= hi + w)
    return hit, t, u, v


def restate(scene, r7):
    """-> (hits [n, 8] uint32: the words of rpt_hit, occluded [n] uint8) for rays [n, 7] {o, d, max_dist}."""
    tris = mesh_tris(scene).astype(F)
    first = np.cumsum([0] + [len(t) for _, t, _ in scene.meshes])
    mesh_of = np.concatenate([np.full(len(t), m) for m, (_, t, _) in enumerate(scene.meshes)])
    n = len(r7)
    hits = np.zeros((n, 8), np.uint32)
    occluded = np.zeros(n, np.uint8)
    with np.errstate(all="ignore"):
        for s0 in range(0, n, 1024):
            r = np.asarray(r7[s0:s0 + 1024], F)
            o, d, md = r[:, 0:3], r[:, 3:6], r[:, 6]
            m = len(r)
            dist = np.full(m, F32_MAX, F)
            hit = np.zeros(m, bool)
            sphere = np.full(m, -1)
            plane = np.full(m, -1)
            occ = np.zeros(m, bool)
            for i, sp in enumerate(scene.spheres):
                h, t = hit_sphere(o, d, sp[0], sp[1])
                acc = h & (np.full(m, i == 0) | (t < dist))
                dist, sphere, hit = np.where(acc, t, dist), np.where(acc, i, sphere), hit | acc
                occ |= h & (t < md)
            for k, pl in enumerate(scene.planes):
                h, t = hit_plane(o, d, pl[0], pl[1], pl[2], pl[4] if len(pl) > 4 else 0.0)
                acc = h & (np.full(m, len(scene.spheres) == 0 and k == 0) | (t < dist))
                dist, plane, hit = np.where(acc, t, dist), np.where(acc, k, plane), hit | acc
                occ |= h & (t < md)
            th, tt, tu, tv = triangles(tris, o, d)
            occ |= (th & (tt < md[:, None])).any(axis=1)
            cand = np.where(th & (tt < dist[:, None]), tt, F(np.inf))
            k = np.argmin(cand, axis=1)                              # the first of equal minima: the lowest index
            rows = np.arange(m)
            tri = np.isfinite(cand[rows, k])
            dist = np.where(tri, cand[rows, k], dist).astype(F)
            hit |= tri
            kind = np.where(tri, HIT_TRIANGLE, np.where(plane >= 0, HIT_PLANE, np.where(sphere >= 0, HIT_SPHERE, HIT_NONE)))
            kind = np.where(hit, kind, HIT_NONE)
            prim = np.where(tri, k, np.where(plane >= 0, plane, sphere))
            out = hits[s0:s0 + m]
            out[:, 0] = np.where(hit, dist.view(np.uint32), np.uint32(INF_BITS))
            out[:, 1] = kind
            out[:, 2] = np.where(hit, prim, NONE).astype(np.uint32)
            out[:, 3] = np.where(tri, mesh_of[k], NONE).astype(np.uint32)
            out[:, 4] = np.where(tri, k - first[mesh_of[k]], NONE).astype(np.uint32)
            out[:, 5] = np.where(tri, tu[rows, k], F(0)).astype(F).view(np.uint32)
            out[:, 6] = np.where(tri, tv[rows, k], F(0)).astype(F).view(np.uint32)
            occluded[s0:s0 + m] = occ
    return hits, occluded


def flat_normals(tris, index):
    """normalize(cross(e1, e2)) of triangles `index`, as hit_normal computes it: the length's root, then three divides."""
    t = tris[index].astype(F)
    c = cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    with np.errstate(all="ignore"):
        length = np.sqrt(dot(c, c))
        return (c / length[:, None]).astype(F)


def compare_words(got, want):
    """-> the rays where the rpt_hit words differ; a NaN t on both sides counts as equal (see the head of this file)."""
    got, want = np.asarray(got).view(np.uint32).reshape(-1, 8), np.asarray(want).view(np.uint32).reshape(-1, 8)
    same = got == want
    same[:, 0] |= np.isnan(got[:, 0].view(F)) & np.isnan(want[:, 0].view(F))
    return np.nonzero(~same.all(axis=1))[0]


def sphere_normals(o, d, t, centre):
    """The integrator's normal of a sphere hit at distance t: normalize((o + t * d) - centre), the length's root, then three divides."""
    with np.errstate(all="ignore"):
        v = (o + t[:, None] * d) - F(centre)[None, :]
        return (v / np.sqrt(dot(v, v))[:, None]).astype(F)


# ---- small helpers of other test files, copied (a test file is not imported from) -------------------------------------------------
REPEAT, CLAMP, NEAREST, BILINEAR = 0, 1, 0, 1                       # tests/test_mesh_texture_host.py
WRAPS, FILTERS = {REPEAT: "repeat", CLAMP: "clamp"}, {NEAREST: "nearest", BILINEAR: "bilinear"}
# tests/test_gpu_mesh_normal_map.py: a rotation about z with a stretch along z and a small shift
MATRIX = np.array([[0.96, -0.28, 0.0, 0.05], [0.28, 0.96, 0.0, -0.02], [0.0, 0.0, 1.25, 0.01]], F)


def random_texels(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def tex(uvs, texels, wrap=REPEAT, filt=BILINEAR, gamma=1.0):
    """One item of Tracer.set_mesh_textures (tests/test_gpu_mesh_texture.py, _tex)."""
    return dict(uvs=uvs, texels=texels, wrap=WRAPS[wrap], filter=FILTERS[filt], gamma=gamma)


def checker(w, h, cells):
    from rust_pathtracer_amd import scenes
    return scenes.checker_mask(w, h, cells)


def probe_scene():
    """tests/test_gpu_mesh_normal_map.py's _probe_scene: mesh_texture_scene() with the quad's UVs mirrored in s and, as mesh 2, one
    triangle whose first two corners share a UV."""
    from rust_pathtracer_amd import scenes
    s, uvs = scenes.mesh_texture_scene()
    quad_uv = uvs[1].copy()
    quad_uv[:, 0] = F(1.0) - quad_uv[:, 0]
    tri = np.array([[-1.6, -0.4, 0.2], [-0.9, -0.45, 0.4], [-1.3, 0.5, 0.3]], F)
    s.meshes.append((tri, np.array([[0, 1, 2]], np.uint32), 1))
    return s, [uvs[0], quad_uv, np.array([[0.3, 0.3], [0.3, 0.3], [0.7, 0.9]], F)]


def texture_rays(scene, uvs, w, n, rng):
    """tests/test_gpu_mesh_texture.py's _query_rays: rays aimed at random points of the meshes and, on the quad (whose s is linear along
    its first edge, from -1.5 to 2.5), at points whose s is a texel centre or a texel border of a texture `w` wide.  [n, 7] f32."""
    tris = mesh_tris(scene).astype(np.float64)
    half = n // 2
    tri = tris[rng.integers(0, len(tris), half)]
    bary = rng.dirichlet([1, 1, 1], half)
    tgt = [(bary[:, :, None] * tri).sum(1)]
    q = np.asarray(scene.meshes[1][0], np.float64)
    k = rng.integers(-2 * w, 3 * w, n - half)
    s = np.where(rng.integers(0, 2, n - half) == 0, (k + 0.5) / w, k / w)
    a, b = np.clip((s + 1.5) / 4.0, 0.0, 1.0), rng.uniform(0.02, 0.98, n - half)
    tgt.append(q[0] + a[:, None] * (q[1] - q[0]) + b[:, None] * (q[3] - q[0]))
    tgt = np.concatenate(tgt)
    o = np.array([0.3, 0.4, 3.0]) + rng.normal(size=(n, 3)) * 0.8
    return np.concatenate([o, tgt - o, np.full((n, 1), 3.0e38)], 1).astype(F)


def small_scene():
    from rust_pathtracer_amd import scenes
    return scenes.mesh_scene(subdivisions=2, n_major=16, n_minor=8)


def with_vertices(make, arrays):
    """A new scene from `make()` with its meshes' vertex arrays replaced by copies of `arrays`."""
    s = make()
    s.meshes = [(np.array(v, F, copy=True), t, m) for v, (_, t, m) in zip(arrays, s.meshes)]
    return s


def mesh_form(rpt, t):
    form = C.c_uint32(0)
    assert rpt.lib().rpt_debug_mesh_form(t._h, C.byref(form)) == 0
    return form.value


def gen_ray_probe(rpt, torch, tracer, px, py, width, height):
    """rpt_probe_fn's GEN_RAY records for pixel coordinates (px, py) with both offsets 0.5 -> [n, 6] f32 {origin, direction}."""
    A = rpt._abi
    rec = np.zeros((len(px), A.RPT_PROBE_IN_STRIDE), F)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = px, py, 0.5, 0.5
    dev = torch.from_numpy(rec).cuda()
    out = torch.empty(len(px), A.RPT_PROBE_OUT_STRIDE, dtype=torch.float32, device="cuda")
    params = np.array([width, height], F)
    rpt._lib.check(rpt.lib().rpt_probe_fn(tracer._h, A.RPT_PROBE_FN_GEN_RAY, dev.data_ptr(), out.data_ptr(), len(px), params.ctypes.data, None), tracer._h)
    torch.cuda.synchronize()
    return out.cpu().numpy()[:, 0:6]
