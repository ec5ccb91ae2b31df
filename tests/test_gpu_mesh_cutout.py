"""Mesh cutouts on the GPU (include/rpt.h, "mesh cutouts"): an A8 mask per mesh, tested inside both hierarchy walks.

Everything is bit for bit, and nothing takes the device's own output as truth:
* the mask bits (rpt_download_mesh_cutout) equal tests/test_mesh_cutout_host.py's packed-bits restatement, up to 257 x 129;
* the walks (rpt_debug_mesh_cutout_query) equal the numpy float32 ordered loop with the cut test as its last line — index, t and
  any-hit, through the hierarchy and the ordered loop, with and without max_dist, one mesh REPEAT and one CLAMP;
* an all-opaque mask gives the frames of the same context without cutouts, in the flat, smooth, textured and environment forms;
* THE INDEPENDENT YARDSTICK: a triangle soup whose triangles are each wholly opaque or wholly transparent renders the frames of a
  fresh upload of the scene with exactly the transparent triangles removed — seen by the camera and standing between the light and
  the floor — and an all-transparent mesh renders the scene without that mesh;
* a checker changes the frame and rays through its holes return the triangle behind; after every kind of move the frames are those
  of a fresh upload of the moved scene followed by the same calls;
* bit 30 of rpt_debug_kernel_choice is set exactly while a cutout is ON, and OFF is the way back; every stated answer, both
  directions of the mesh-light exclusion and the texture-removal rule; a device listed twice renders the one-device frame."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_mesh import F32_MAX, _cross, _dot, _mesh_tris, _query
from test_gpu_mesh_texture import _move_textures, _query_rays, _tex, _white
from test_gpu_mesh_update import _assert_frames, _choice, _frames, _same, _small_scene, _with_vertices
from test_mesh_cutout_host import MASK_SIZES, THRESHOLDS, random_alpha, restate_cut_texel, restate_mask_bits, restate_mask_words
from test_mesh_texture_host import BILINEAR, CLAMP, NEAREST, REPEAT, random_texels

pytestmark = pytest.mark.gpu

F = np.float32
MESH_BIT, SMOOTH_BIT, LIGHT_BIT, TEX_BIT, ENV_BIT, CUT_BIT = 1 << 25, 1 << 26, 1 << 27, 1 << 28, 1 << 29, 1 << 30
SMALL = dict(sizes=((32, 24, 4),), resident=None)
MATRIX = np.array([[0.96, -0.28, 0.0, 0.05], [0.28, 0.96, 0.0, -0.02], [0.0, 0.0, 1.25, 0.01]], F)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _checker(w, h, cells):
    from rust_pathtracer_amd import scenes
    return scenes.checker_mask(w, h, cells)


def _opaque(w=3, h=2):
    return np.full((h, w), 255, np.uint8)


# ---- 1. the mask bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", MASK_SIZES + ((257, 129),), ids=lambda wh: "%dx%d" % wh)
def test_mask_bits_equal_the_restatement(rpt, torch_cuda, size):
    from rust_pathtracer_amd import scenes
    w, h = size
    s, uvs, _ = scenes.mesh_cutout_scene()
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        t.set_mesh_textures({m: _tex(uvs[m], _white()) for m in (0, 1, 2)})
        other = random_alpha(7, 9, 5)
        for threshold in THRESHOLDS:
            alpha = random_alpha(w, h, 1000 * w + h + threshold)
            t.set_mesh_cutouts({0: dict(alpha=other, threshold=77), 2: dict(alpha=alpha, threshold=threshold)})
            got = t.mesh_cutout(2)
            assert got.shape == (h, w) and np.array_equal(got.reshape(-1), restate_mask_bits(alpha, threshold)), (size, threshold)
            words = np.zeros((w * h + 31) // 32, np.uint32)
            rpt._lib.check(rpt.lib().rpt_download_mesh_cutout(t._h, 2, words.ctypes.data, words.size), t._h)
            assert np.array_equal(words, restate_mask_words(alpha, threshold)), "the words, their ragged last one's padding zero"
            assert np.array_equal(t.mesh_cutout(0).reshape(-1), restate_mask_bits(other, 77)), "the first mask of the call"
        # a mesh not named keeps its bits though the table is made anew; OFF removes
        t.set_mesh_cutouts({0: None, 1: dict(alpha=other, threshold=200)})
        assert np.array_equal(t.mesh_cutout(2).reshape(-1), restate_mask_bits(alpha, THRESHOLDS[-1]))
        assert np.array_equal(t.mesh_cutout(1).reshape(-1), restate_mask_bits(other, 200))
        words = np.zeros(2, np.uint32)
        assert rpt.lib().rpt_download_mesh_cutout(t._h, 0, words.ctypes.data, 2) == rpt._abi.RPT_ERR_INVALID_ARG
        assert b"mesh 0 has no cutout" in rpt.lib().rpt_last_error(t._h)
        assert rpt.lib().rpt_download_mesh_cutout(t._h, 1, words.ctypes.data, 3) == rpt._abi.RPT_ERR_INVALID_ARG
        assert b"n_words 3 != 2" in rpt.lib().rpt_last_error(t._h)
        assert rpt.lib().rpt_download_mesh_cutout(t._h, 1, None, 2) == rpt._abi.RPT_ERR_INVALID_ARG
        assert rpt.lib().rpt_download_mesh_cutout(t._h, 3, words.ctypes.data, 2) == rpt._abi.RPT_ERR_INVALID_ARG
    finally:
        t.close()


# ---- 2. the walks -----------------------------------------------------------------------------------------------------------------
def brute_force_cut(scene, cutouts, rays, use_max):
    """The ordered loop of include/rpt.h in numpy float32 (tests/test_gpu_mesh.py, brute_force) with the cut test as the triangle
    test's last line.  `cutouts`: mesh -> (uvs [n_vertices, 2], opaque bits [h, w] bool, wrap).  -> (t bits, index or -1, any)."""
    tris = _mesh_tris(scene).astype(F)
    a = tris[None, :, 0]
    e1 = tris[None, :, 1] - tris[None, :, 0]
    e2 = tris[None, :, 2] - tris[None, :, 0]
    cols, first = {}, 0
    for m, (v, idx, _) in enumerate(scene.meshes):
        n = len(np.asarray(idx).reshape(-1, 3))
        if m in cutouts:
            uv = np.asarray(cutouts[m][0], F)[np.asarray(idx, np.int64).reshape(-1, 3)]          # [n, 3, 2]
            cols[m] = (first, first + n, uv)
        first += n
    out_t = np.full(len(rays), 0x7F800000, np.uint32)
    out_i = np.full(len(rays), -1, np.int64)
    out_any = np.zeros(len(rays), np.uint32)
    with np.errstate(all="ignore"):
        for s in range(0, len(rays), 1024):
            r = rays[s:s + 1024].astype(F)
            o, d, md = r[:, None, 0:3], r[:, None, 3:6], r[:, 6:7]
            d = np.broadcast_to(d, (len(r),) + e2.shape[1:])
            p = _cross(d, np.broadcast_to(e2, d.shape))
            det = _dot(np.broadcast_to(e1, d.shape), p)
            hit = (det < 0) | (det > 0)
            inv = F(1.0) / det
            sv = o - a
            u = _dot(sv, p) * inv
            hit &= (u >= 0) & (u <= 1)
            q = _cross(sv, np.broadcast_to(e1, sv.shape))
            v = _dot(d, q) * inv
            hit &= (v >= 0) & (u + v <= 1)
            t = _dot(np.broadcast_to(e2, q.shape), q) * inv
            hit &= (t >= 0) & (t < F32_MAX)
            for i in range(3):
                ai, e1i, e2i = a[..., i], e1[..., i], e2[..., i]
                lo = ai + np.minimum(np.minimum(F(0), e1i), e2i)
                hi = ai + np.maximum(np.maximum(F(0), e1i), e2i)
                w = (np.maximum(np.abs(lo), np.abs(hi)) + np.abs(o[..., i])) * F(2.0 ** -16)
                pi = o[..., i] + t * d[..., i]
                hit &= (lo - w <= pi) & (pi <= hi + w)
            for m, (c0, c1, uv) in cols.items():                     # the cut test: the last line, with the test's own u and v
                _, bits, wrap = cutouts[m]
                h_, w_ = bits.shape
                n = c1 - c0
                uu, vv = np.where(hit[:, c0:c1], u[:, c0:c1], F(0)).reshape(-1), np.where(hit[:, c0:c1], v[:, c0:c1], F(0)).reshape(-1)
                corner = lambda k: np.broadcast_to(uv[None, :, k], (len(r), n, 2)).reshape(-1, 2)      # noqa: E731
                k = restate_cut_texel(uu, vv, corner(0), corner(1), corner(2), w_, h_, wrap)
                hit[:, c0:c1] &= bits.reshape(-1)[k].reshape(len(r), n)
            tt = np.where(hit, t, F(np.inf))
            k = np.argmin(tt, axis=1)                                  # the first of equal minima: the lowest index
            best = tt[np.arange(len(r)), k]
            got = np.isfinite(best)
            out_t[s:s + len(r)] = np.where(got, best.view(np.uint32), np.uint32(0x7F800000))
            out_i[s:s + len(r)] = np.where(got, k, -1)
            occ = hit & (t < md) if use_max else hit
            out_any[s:s + len(r)] = occ.any(axis=1)
    return out_t, out_i, out_any


def _cut_query(rpt, torch, tracer, rays, flags):
    n = len(rays)
    dev = torch.from_numpy(np.ascontiguousarray(rays, dtype=F)).cuda()
    out = torch.zeros(n, 3, dtype=torch.int32, device="cuda")
    rpt._lib.check(rpt.lib().rpt_debug_mesh_cutout_query(tracer._h, dev.data_ptr(), n, out.data_ptr(), flags, None), tracer._h)
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    return o[:, 0], o[:, 1].astype(np.int64) - (o[:, 1] == 0xFFFFFFFF) * (1 << 32), o[:, 2]


def _query_scene():
    """mesh_texture_scene() with its icosphere subdivided once more (320 triangles: interior nodes and leaves of several triangles)."""
    from rust_pathtracer_amd import scenes
    s, uvs = scenes.mesh_texture_scene()
    v, idx = scenes.icosphere(2, (0.0, 0.0, 0.0), 0.6)
    s.meshes[0] = (v, idx, s.meshes[0][2])
    return s, [scenes.spherical_uvs(v, (0.0, 0.0, 0.0)), uvs[1]]


@pytest.mark.parametrize("wraps", [(REPEAT, CLAMP), (CLAMP, REPEAT)], ids=["sphere-repeat", "sphere-clamp"])
def test_walks_equal_the_ordered_loop_with_the_cut_test(rpt, torch_cuda, wraps):
    """4096 rays at the meshes and at the quad's texel borders; 4 x 4 on the sphere and 5 x 3 on the quad, whose UVs run over
    [-1.5, 2.5]: REPEAT tiles the checker four times, CLAMP stretches its edge texels."""
    A = rpt._abi
    s, uvs = _query_scene()
    rng = np.random.default_rng(4100 + wraps[0])
    rays = _query_rays(s, uvs, 5, 4096, rng)
    rays[:, 6] = rng.uniform(0.5, 1.5, len(rays)).astype(F)           # the targets lie at t = 1
    masks = [_checker(4, 4, 4), _checker(5, 3, 5)]
    masks[1][2, :] = masks[1][0, ::-1]                                 # (five cells over three rows repeat the second row: alternate instead)
    t = rpt.Tracer(s, device=0, seed=2)
    try:
        t.set_mesh_textures({m: _tex(uvs[m], random_texels(2, 2, 8 + m), wraps[m], BILINEAR) for m in (0, 1)})
        t.set_mesh_cutouts({m: dict(alpha=masks[m], threshold=128) for m in (0, 1)})
        cut = {m: (uvs[m], masks[m] >= 128, wraps[m]) for m in (0, 1)}
        plain_t, plain_i, _ = brute_force_cut(s, {}, rays, False)
        for use_max in (False, True):
            want_t, want_i, want_any = brute_force_cut(s, cut, rays, use_max)
            for brute in (False, True):
                flags = (A.RPT_MESH_QUERY_USE_MAX if use_max else 0) | (A.RPT_MESH_QUERY_BRUTE if brute else 0)
                got_t, got_i, got_any = _cut_query(rpt, torch_cuda, t, rays, flags)
                what = "use_max %s brute %s" % (use_max, brute)
                assert np.array_equal(got_i, want_i), "%s: index of %d rays differs" % (what, int((got_i != want_i).sum()))
                assert np.array_equal(got_t, want_t), "%s: t of %d rays differs" % (what, int((got_t != want_t).sum()))
                assert np.array_equal(got_any, want_any), "%s: any-hit of %d rays differs" % (what, int((got_any != want_any).sum()))
        n_sphere = len(s.meshes[0][1])
        assert (want_i >= n_sphere).mean() > 0.1 and ((want_i >= 0) & (want_i < n_sphere)).mean() > 0.1, "both meshes are hit"
        changed = want_i != plain_i
        assert changed.mean() > 0.2 and (changed & (want_i >= 0)).sum() > 100, "holes matter, and rays go on to what lies behind"
        assert ((want_any == 1) & (want_i >= 0)).sum() > 100 and ((want_any == 0) & (want_i >= 0)).sum() > 100, "max_dist decides some"
    finally:
        t.close()


def test_the_hook_needs_a_cutout(rpt, torch_cuda):
    s, uvs = _query_scene()
    t = rpt.Tracer(s, device=0, seed=2)
    try:
        t.set_mesh_textures({0: _tex(uvs[0], _white())})
        rays = torch_cuda.zeros(7, device="cuda")
        out = torch_cuda.zeros(3, dtype=torch_cuda.int32, device="cuda")
        assert rpt.lib().rpt_debug_mesh_cutout_query(t._h, rays.data_ptr(), 1, out.data_ptr(), 0, None) == rpt._abi.RPT_ERR_INVALID_ARG
        assert b"no mesh has a cutout" in rpt.lib().rpt_last_error(t._h)
        t.set_mesh_cutouts({0: _opaque()})
        assert rpt.lib().rpt_debug_mesh_cutout_query(t._h, rays.data_ptr(), 1, out.data_ptr(), 4, None) == rpt._abi.RPT_ERR_INVALID_ARG
        assert rpt.lib().rpt_debug_mesh_cutout_query(t._h, rays.data_ptr(), 1, out.data_ptr(), 0, None) == rpt._abi.RPT_OK
    finally:
        t.close()


# ---- 3. an all-opaque mask is no mask ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["flat", "smooth", "textured", "environment"])
def test_an_all_opaque_mask_is_the_frame_without_cutouts(rpt, torch_cuda, form):
    from rust_pathtracer_amd import scenes
    s, uvs = scenes.mesh_texture_scene()
    t = rpt.Tracer(s, device=0, seed=4)
    try:
        if form == "textured":
            t.set_mesh_textures({0: _tex(uvs[0], random_texels(5, 3, 21), REPEAT, BILINEAR, 2.2), 1: _tex(uvs[1], random_texels(4, 4, 22), CLAMP, NEAREST)})
        else:
            t.set_mesh_textures({m: _tex(uvs[m], _white()) for m in (0, 1)})
        if form == "smooth":
            t.set_mesh_shading({0: "smooth"})
        if form == "environment":
            t.set_environment(scenes.mesh_env_scene(16)[1], 1.0, sampled=True)
        base = MESH_BIT | TEX_BIT | (SMOOTH_BIT if form == "smooth" else 0) | (ENV_BIT if form == "environment" else 0)
        every = MESH_BIT | SMOOTH_BIT | LIGHT_BIT | TEX_BIT | ENV_BIT | CUT_BIT
        plain = _frames(rpt, t, **SMALL)
        assert _choice(rpt, t) & every == base
        t.set_mesh_cutouts({0: _opaque(3, 2), 1: dict(alpha=_opaque(1, 1), threshold=255)})
        _assert_frames(_frames(rpt, t, **SMALL), plain, "%s: an all-opaque mask" % form)
        assert _choice(rpt, t) & every == base | CUT_BIT
        assert np.isfinite(plain[0]).all() and plain[0][..., :3].mean() > 0.005
    finally:
        t.close()


# ---- 4. deleted triangles: the independent yardstick ---------------------------------------------------------------------------------
def _soup(center, radius):
    """An icosphere of 80 triangles with no shared vertices, one UV per TRIANGLE: the centre of texel k * 5 % 64 of an 8 x 8 mask."""
    from rust_pathtracer_amd import scenes
    v, idx = scenes.icosphere(1, center, radius)
    verts = np.ascontiguousarray(np.asarray(v, F)[np.asarray(idx, np.int64).reshape(-1)])
    index = np.arange(len(verts), dtype=np.uint32).reshape(-1, 3)
    texel = (np.arange(len(index)) * 5) % 64
    uv = np.stack([(texel % 8 + 0.5) / 8.0, (texel // 8 + 0.5) / 8.0], 1).astype(F)
    return verts, index, np.repeat(uv, 3, axis=0), texel


def _soup_scene(center, radius, keep=None):
    """mesh_texture_scene() with the soup for its icosphere; `keep` (bool per triangle): only those triangles."""
    from rust_pathtracer_amd import scenes
    s, uvs = scenes.mesh_texture_scene()
    verts, index, uv, texel = _soup(center, radius)
    if keep is not None:
        sel = np.repeat(np.asarray(keep, bool), 3)
        verts, uv = np.ascontiguousarray(verts[sel]), np.ascontiguousarray(uv[sel])
        index = np.arange(len(verts), dtype=np.uint32).reshape(-1, 3)
    s.meshes[0] = (verts, index, s.meshes[0][2])
    return s, [uv, uvs[1]], texel


@pytest.mark.parametrize("where", ["seen", "shadow"])
def test_transparent_triangles_are_deleted_triangles(rpt, torch_cuda, where):
    """Every triangle's three UVs are one texel centre, so the mask deletes whole triangles: the frames equal those of a fresh upload
    without them.  "shadow": the soup hangs between the light (-2.5, 1.5, 1) and the floor the camera sees, so its shadow rays decide
    pixels."""
    center, radius = ((0.0, 0.0, 0.0), 0.6) if where == "seen" else ((-1.0, 0.45, 0.6), 0.45)
    alpha = np.where(np.random.default_rng(77).integers(0, 2, (8, 8)) == 1, 255, 0).astype(np.uint8)
    s, uvs, texel = _soup_scene(center, radius)
    keep = alpha.reshape(-1)[texel] >= 128
    assert 20 < keep.sum() < 60
    tex = lambda u: {0: _tex(u[0], random_texels(8, 8, 31), REPEAT, NEAREST), 1: _tex(u[1], random_texels(3, 3, 32), CLAMP, BILINEAR)}      # noqa: E731
    t = rpt.Tracer(s, device=0, seed=12)
    try:
        t.set_mesh_textures(tex(uvs))
        whole = _frames(rpt, t, **SMALL)
        t.set_mesh_cutouts({0: alpha})
        got = _frames(rpt, t, **SMALL)
        assert _choice(rpt, t) & CUT_BIT
    finally:
        t.close()
    s2, uvs2, _ = _soup_scene(center, radius, keep)
    b = rpt.Tracer(s2, device=0, seed=12)
    try:
        b.set_mesh_textures(tex(uvs2))
        want = _frames(rpt, b, **SMALL)
        assert not _choice(rpt, b) & CUT_BIT
    finally:
        b.close()
    _assert_frames(got, want, "%s: the soup with its transparent triangles removed" % where)
    assert not _same(got[0], whole[0]), "the holes show"


def test_an_all_transparent_mesh_is_no_mesh(rpt, torch_cuda):
    from rust_pathtracer_amd import scenes
    s, uvs = scenes.mesh_texture_scene()
    t = rpt.Tracer(s, device=0, seed=13)
    try:
        t.set_mesh_textures({m: _tex(uvs[m], random_texels(3, 3, 40 + m), REPEAT, BILINEAR) for m in (0, 1)})
        t.set_mesh_cutouts({0: np.zeros((4, 4), np.uint8)})
        got = _frames(rpt, t, **SMALL)
    finally:
        t.close()
    s2, _ = scenes.mesh_texture_scene()
    s2.meshes = s2.meshes[1:]
    b = rpt.Tracer(s2, device=0, seed=13)
    try:
        b.set_mesh_textures({0: _tex(uvs[1], random_texels(3, 3, 41), REPEAT, BILINEAR)})
        _assert_frames(got, _frames(rpt, b, **SMALL), "an all-transparent icosphere")
    finally:
        b.close()


# ---- 5. a checker ------------------------------------------------------------------------------------------------------------------
def test_a_checker_changes_the_frame_and_rays_go_through_its_holes(rpt, torch_cuda):
    from rust_pathtracer_amd import scenes
    s, uvs, mask = scenes.mesh_cutout_scene(cells=6, size=48)
    t = rpt.Tracer(s, device=0, seed=6)
    try:
        t.set_mesh_textures({m: _tex(uvs[m], _white()) for m in (0, 1, 2)})
        plain = _frames(rpt, t, **SMALL)
        t.set_mesh_cutouts({2: mask})
        assert not _same(_frames(rpt, t, **SMALL)[0], plain[0])
        # rays through the screen's 6 x 6 fields at the icosphere's centre: each crosses the screen once, inside its field, and
        # then meets the icosphere (80 triangles, radius 0.6 about the origin) before anything else
        q = np.asarray(s.meshes[2][0], np.float64)
        a, b = np.meshgrid((np.arange(6) + 0.5) / 6.0, (np.arange(6) + 0.4) / 6.0, indexing="xy")      # s = a, t = b: never on the diagonal
        # the screen is not planar: aim inside triangle (0, 1, 2), where s >= t, or inside (0, 2, 3)
        through = np.where((a >= b)[..., None], q[0] + (a - b)[..., None] * (q[1] - q[0]) + b[..., None] * (q[2] - q[0]),
                           q[0] + a[..., None] * (q[2] - q[0]) + (b - a)[..., None] * (q[3] - q[0])).reshape(-1, 3)
        o = 2.0 * through                                            # as far in front of the screen as the screen is from the centre
        rays = np.concatenate([o, -o, np.full((len(o), 1), 3.0e38)], 1).astype(F)
        _, uncut, _ = _query(rpt, torch_cuda, t, rays, 0)            # the walk without the cut test: the screen stops every ray
        assert (uncut >= 82).all()
        _, index, _ = _cut_query(rpt, torch_cuda, t, rays, 0)
        _, index_brute, _ = _cut_query(rpt, torch_cuda, t, rays, rpt._abi.RPT_MESH_QUERY_BRUTE)
        assert np.array_equal(index, index_brute)
        hole = (mask[(b * 48).astype(int), (a * 48).astype(int)] == 0).reshape(-1)
        assert hole.sum() == 18
        assert (index[~hole] >= 82).all(), "an opaque field stops the ray"
        assert ((index[hole] >= 0) & (index[hole] < 80)).all(), "through a hole: the icosphere behind"
    finally:
        t.close()


# ---- 6. moves ---------------------------------------------------------------------------------------------------------------------
def _move_cutouts():
    return {0: dict(alpha=_checker(12, 6, 6), threshold=128), 1: dict(alpha=_checker(9, 9, 3), threshold=1)}


def _fresh(rpt, arrays):
    """The yardstick: a fresh context that uploads the scene with these positions and then makes the same set calls."""
    b = rpt.Tracer(_with_vertices(_small_scene, arrays), device=0, seed=8)
    try:
        b.set_mesh_textures(_move_textures(_small_scene()))
        b.set_mesh_cutouts(_move_cutouts())
        return _frames(rpt, b, **SMALL)
    finally:
        b.close()


@pytest.mark.parametrize("form", ["update", "rebuild", "update_device", "rebuild_device"])
def test_cutout_frames_follow_every_kind_of_move(rpt, torch_cuda, form):
    from rust_pathtracer_amd import scenes
    s = _small_scene()
    rest = [np.array(v, F, copy=True) for v, _, _ in s.meshes]
    t = rpt.Tracer(s, device=0, seed=8)
    try:
        t.set_mesh_textures(_move_textures(s))
        uncut = _frames(rpt, t, **SMALL)
        t.set_mesh_cutouts(_move_cutouts())
        still = _frames(rpt, t, **SMALL)
        _assert_frames(still, _fresh(rpt, rest), "before any move")
        assert not _same(still[0], uncut[0])
        masks = [t.mesh_cutout(m).copy() for m in (0, 1)]
        moved = scenes.mesh_scene_moved(s, 0.7)
        if form == "update":
            t.update_meshes(dict(enumerate(moved)))
        elif form == "rebuild":
            t.rebuild_meshes(dict(enumerate(moved)))
        else:                                                         # the device forms: mesh 0 as it is, mesh 1 through a 3x4 matrix
            src = {0: torch_cuda.from_numpy(moved[0]).to("cuda:0"), 1: (torch_cuda.from_numpy(rest[1]).to("cuda:0"), MATRIX)}
            (t.update_meshes_device if form == "update_device" else t.rebuild_meshes_device)(src)
        held = [t.mesh_vertices(m) for m in (0, 1)]
        got = _frames(rpt, t, **SMALL)
        assert _choice(rpt, t) & CUT_BIT
        _assert_frames(got, _fresh(rpt, held), "%s: against a fresh upload" % form)
        assert not _same(got[0], still[0])
        assert all(np.array_equal(t.mesh_cutout(m), masks[m]) for m in (0, 1)), "a move leaves the masks alone"
    finally:
        t.close()


# ---- 7. lifetime ------------------------------------------------------------------------------------------------------------------
def test_bit_30_and_the_way_back(rpt, torch_cuda):
    from rust_pathtracer_amd import scenes
    s, uvs, mask = scenes.mesh_cutout_scene()
    every = MESH_BIT | SMOOTH_BIT | LIGHT_BIT | TEX_BIT | ENV_BIT | CUT_BIT
    t = rpt.Tracer(s, device=0, seed=9)
    try:
        t.set_mesh_textures({m: _tex(uvs[m], random_texels(3, 5, 60 + m)) for m in (0, 1, 2)})
        never = _frames(rpt, t, **SMALL)
        before = _choice(rpt, t)
        assert before & every == MESH_BIT | TEX_BIT
        t.set_mesh_cutouts({2: mask, 0: _checker(8, 8, 4)})
        both = _frames(rpt, t, **SMALL)
        assert _choice(rpt, t) == before | CUT_BIT and not _same(both[0], never[0])
        t.set_mesh_cutouts({0: None})
        one = _frames(rpt, t, **SMALL)
        assert _choice(rpt, t) & CUT_BIT and not _same(one[0], never[0]) and not _same(one[0], both[0])
        # replacing a texture keeps the cutout; a texture for another wrap is read by the cut test at once
        t.set_mesh_textures({2: _tex(uvs[2], random_texels(3, 5, 62))})
        _assert_frames(_frames(rpt, t, **SMALL), one, "the same texture again")
        t.set_mesh_textures({0: None})                               # the ordinals move: the screen's descriptor follows
        assert np.array_equal(t.mesh_cutout(2), mask >= 128)
        t.set_mesh_textures({0: _tex(uvs[0], random_texels(3, 5, 60))})
        _assert_frames(_frames(rpt, t, **SMALL), one, "the ordinals moved and moved back")
        t.set_mesh_cutouts({2: None})
        _assert_frames(_frames(rpt, t, **SMALL), never, "the last cutout OFF")
        assert _choice(rpt, t) == before
        t.set_mesh_cutouts({0: None, 1: None, 2: None})              # removing what is not there is no error
        t.set_mesh_cutouts({2: mask, 0: _checker(8, 8, 4)})
        _assert_frames(_frames(rpt, t, **SMALL), both, "the same cutouts again")
        t.upload_scene()                                             # an upload drops cutouts (and textures)
        _frames(rpt, t, **SMALL)
        assert _choice(rpt, t) & every == MESH_BIT
        words = np.zeros(72, np.uint32)
        assert rpt.lib().rpt_download_mesh_cutout(t._h, 2, words.ctypes.data, 72) == rpt._abi.RPT_ERR_INVALID_ARG
        assert rpt.lib().rpt_set_mesh_cutouts(t._h, None, 0) == rpt._abi.RPT_OK
    finally:
        t.close()


def test_the_ordinals_move_under_a_cutout(rpt, torch_cuda):
    """Textures set and removed on OTHER meshes renumber the texture ordinals the descriptors are indexed by: the frames are those of
    a context that made the calls in the plain order."""
    from rust_pathtracer_amd import scenes
    s, uvs, mask = scenes.mesh_cutout_scene()
    texs = {m: _tex(uvs[m], random_texels(3, 5, 90 + m), CLAMP if m == 2 else REPEAT) for m in (0, 1, 2)}
    a = rpt.Tracer(s, device=0, seed=14)
    try:
        a.set_mesh_textures(texs)
        a.set_mesh_cutouts({2: mask, 1: _checker(10, 10, 5)})
        want = _frames(rpt, a, **SMALL)
    finally:
        a.close()
    b = rpt.Tracer(scenes.mesh_cutout_scene()[0], device=0, seed=14)
    try:
        b.set_mesh_textures({2: dict(texs[2], wrap="repeat")})       # ordinal 0, another wrap
        b.set_mesh_cutouts({2: mask})
        b.set_mesh_textures({1: texs[1]})                            # the screen becomes ordinal 1
        b.set_mesh_cutouts({1: _checker(10, 10, 5)})
        b.set_mesh_textures({0: texs[0], 2: texs[2]})                # ordinal 2, and its wrap is CLAMP from now on
        _assert_frames(_frames(rpt, b, **SMALL), want, "the calls in another order")
    finally:
        b.close()


# ---- 8. answers -------------------------------------------------------------------------------------------------------------------
def test_every_answer_and_a_rejected_call_changes_nothing(rpt, torch_cuda):
    A, lib = rpt._abi, rpt.lib()
    from rust_pathtracer_amd import scenes
    s = scenes.mesh_light_scene(sphere_light=True)                  # mesh 0 the object, mesh 1 the lamp
    uvs = [scenes.spherical_uvs(v, (0.0, 0.0, 0.0)) for v, _, _ in s.meshes]
    t = rpt.Tracer(s, device=0, seed=10)
    try:
        t.set_mesh_textures({0: _tex(uvs[0], random_texels(3, 5, 61), CLAMP, BILINEAR, 2.2)})
        t.set_mesh_cutouts({0: dict(alpha=_checker(6, 6, 3), threshold=9)})
        ref = _frames(rpt, t, **SMALL)
        held = t.mesh_cutout(0).copy()
        alpha = np.ascontiguousarray(random_alpha(2, 2, 62))
        bptr = alpha.ctypes.data_as(C.POINTER(C.c_uint8))

        def items(*rows):
            arr = (A.rpt_mesh_cutout * len(rows))()
            for it, r in zip(arr, rows):
                r = dict(dict(mesh=0, mode=A.RPT_MESH_CUTOUT_ON, width=2, height=2, alpha=bptr, threshold=128), **r)
                for key, val in r.items():
                    setattr(it, key, val)
            return arr

        off = dict(mode=A.RPT_MESH_CUTOUT_OFF, width=0, height=0, alpha=None, threshold=0)
        cases = [("NULL items", None, 1, "items is NULL"),
                 ("mesh out of range", items(dict(mesh=2)), 1, "mesh 2 out of range"),
                 ("named twice", items(dict(), dict()), 2, "item 1: mesh 0 is named twice"),
                 ("mode", items(dict(mode=2)), 1, "mode 2"),
                 ("width 0", items(dict(width=0)), 1, "a mask of 0 x 2"),
                 ("height above 16384", items(dict(height=16385)), 1, "a mask of 2 x 16385"),
                 ("NULL alpha", items(dict(alpha=None)), 1, "alpha is NULL"),
                 ("threshold 0", items(dict(threshold=0)), 1, "threshold 0"),
                 ("threshold 256", items(dict(threshold=256)), 1, "threshold 256"),
                 ("OFF with a size", items(dict(off, width=2)), 1, "RPT_MESH_CUTOUT_OFF takes"),
                 ("OFF with a pointer", items(dict(off, alpha=bptr)), 1, "RPT_MESH_CUTOUT_OFF takes"),
                 ("untextured", items(dict(mesh=1)), 1, "mesh 1 is untextured")]
        for what, arr, n, says in cases:
            assert lib.rpt_set_mesh_cutouts(t._h, arr, n) == A.RPT_ERR_INVALID_ARG, what
            err = lib.rpt_last_error(t._h).decode()
            assert err.startswith("rpt_set_mesh_cutouts: ") and says in err, (what, err)
            assert np.array_equal(t.mesh_cutout(0), held), what
        assert "1 x 1 white texture" in lib.rpt_last_error(t._h).decode()
        # sizes whose sum passes 2^26 texels: refused on the host from the sizes alone (alpha is never read)
        big = items(dict(width=8192, height=8193))
        assert lib.rpt_set_mesh_cutouts(t._h, big, 1) == A.RPT_ERR_UNSUPPORTED and "2^26" in lib.rpt_last_error(t._h).decode()
        # a cutout mesh cannot become a mesh light ...
        light = (A.rpt_mesh_light * 1)()
        light[0].mesh, light[0].mode = 0, A.RPT_MESH_LIGHT_ON
        assert lib.rpt_set_mesh_lights(t._h, light, 1) == A.RPT_ERR_UNSUPPORTED
        err = lib.rpt_last_error(t._h).decode()
        assert err.startswith("rpt_set_mesh_lights: ") and "mesh 0 has a cutout" in err
        # ... nor a mesh light a cutout mesh (another mesh of the scene may be ON)
        t.set_mesh_lights({1: True})
        lit = _frames(rpt, t, **SMALL)
        assert _choice(rpt, t) & (LIGHT_BIT | CUT_BIT) == LIGHT_BIT | CUT_BIT and not _same(lit[0], ref[0])
        t.set_mesh_textures({1: _tex(uvs[1], _white())})
        assert lib.rpt_set_mesh_cutouts(t._h, items(dict(mesh=1)), 1) == A.RPT_ERR_UNSUPPORTED
        err = lib.rpt_last_error(t._h).decode()
        assert err.startswith("rpt_set_mesh_cutouts: ") and "mesh 1 is a mesh light" in err
        t.set_mesh_lights({1: False})
        t.set_mesh_textures({1: None})
        # the texture of a cutout mesh cannot be removed, alone or among others; replacing it is fine
        for gone in ({0: None}, {0: None, 1: _tex(uvs[1], _white())}):
            with pytest.raises(Exception) as e:
                t.set_mesh_textures(gone)
            assert "remove the cutout first" in str(e.value) and lib.rpt_last_error(t._h).decode().startswith("rpt_set_mesh_textures: ")
        tex = (A.rpt_mesh_texture * 1)()
        tex[0].mesh = 0
        assert lib.rpt_set_mesh_textures(t._h, tex, 1) == A.RPT_ERR_INVALID_ARG
        _assert_frames(_frames(rpt, t, **SMALL), ref, "after every rejected call")
        assert np.array_equal(t.mesh_cutout(0), held) and _choice(rpt, t) & CUT_BIT
        assert lib.rpt_set_mesh_cutouts(t._h, None, 0) == A.RPT_OK
        t.set_mesh_cutouts({0: None})
        t.set_mesh_textures({0: None})                               # the cutout removed first: now it goes
        assert _choice(rpt, t) & CUT_BIT                              # (last_choice is the last launch's)
        _frames(rpt, t, **SMALL)
        assert not _choice(rpt, t) & (CUT_BIT | TEX_BIT)
        # no scene with meshes
        b = rpt.Tracer(scenes.six_primitive_scene(), device=0, seed=1)
        try:
            assert lib.rpt_set_mesh_cutouts(b._h, items(dict()), 1) == A.RPT_ERR_NO_SCENE
            assert lib.rpt_set_mesh_cutouts(b._h, None, 0) == A.RPT_ERR_NO_SCENE
            words = np.zeros(4, np.uint32)
            assert lib.rpt_download_mesh_cutout(b._h, 0, words.ctypes.data, 1) == A.RPT_ERR_NO_SCENE
        finally:
            b.close()
    finally:
        t.close()


# ---- 9. several devices -------------------------------------------------------------------------------------------------------------
def test_a_device_listed_twice_renders_the_one_context_frame(rpt, torch_cuda):
    from rust_pathtracer_amd import scenes
    s, uvs, mask = scenes.mesh_cutout_scene()
    tex = {m: _tex(uvs[m], random_texels(3, 5, 80 + m), REPEAT, BILINEAR, 2.2) for m in (0, 1, 2)}
    w, h, spp = 32, 24, 4
    t = rpt.Tracer(s, device=0, seed=11)
    try:
        t.set_mesh_textures(tex)
        t.set_mesh_cutouts({2: mask})
        t.render_resident(w, h, spp)
        one = t.resident_to_host(w, h).pixels.reshape(h, w, 4).copy()
    finally:
        t.close()
    m = rpt.Tracer(scenes.mesh_cutout_scene()[0], devices=[0, 0], seed=11)
    try:
        m.set_mesh_textures(tex)
        m.set_mesh_cutouts({2: mask})
        m.render_resident(w, h, spp)
        assert _choice(rpt, m) & CUT_BIT
        assert _same(m.resident_to_host(w, h).pixels.reshape(h, w, 4), one)
        assert np.array_equal(m.mesh_cutout(2), mask >= 128)
        m.set_mesh_cutouts({2: None})
        m.resident_reset()
        m.render_resident(w, h, spp)
        assert not _choice(rpt, m) & CUT_BIT
    finally:
        m.close()
