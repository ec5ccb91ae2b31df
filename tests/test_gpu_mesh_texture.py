"""Mesh textures on the GPU (include/rpt.h, "mesh textures"): a UV-mapped RGBA8 base colour per mesh, decoded on the device and
filtered at the hit.

Everything is bit for bit, and nothing takes the device's own output as truth:
* the decoded texels (rpt_download_mesh_texture) equal tests/test_mesh_texture_host.py's restatement — the oracle's strict pow and the
  end-point rule — for every byte value at gamma 1, 2.2 and 0.4545;
* the base colour a hit is shaded with (rpt_debug_mesh_texture_query) equals the numpy float32 restatement of u, v, the
  interpolation, the wrap, the filter and the product, for the walk and the ordered loop, both wraps, both filters, four sizes;
* a 1x1 white texture gives the untextured frame in all four base forms, and a 1x1 texture of any colour gives the frame of the
  untextured scene whose material holds the products: the new kernels are tied to the path the oracle pins;
* a checker changes the frame; after every kind of move the textured frames are those of a fresh upload of the moved scene followed
  by the same call, and a rebuild leaves the hook's answers word for word;
* removing the last texture, an upload and a rejected call behave as include/rpt.h says; a device listed twice renders the
  one-device frame.  rpt_debug_kernel_choice's bit 28 is set exactly while a mesh is textured."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_mesh import _mesh_tris, brute_force
from test_gpu_mesh_update import _assert_frames, _choice, _frames, _same, _small_scene, _with_vertices
from test_mesh_texture_host import (BILINEAR, CLAMP, GAMMAS, NEAREST, REPEAT, SIZES, random_texels, restate_decode, restate_decode_table,
                                    restate_hit_st, restate_lookup)

pytestmark = pytest.mark.gpu

F = np.float32
MESH_BIT, SMOOTH_BIT, LIGHT_BIT, TEX_BIT = 1 << 25, 1 << 26, 1 << 27, 1 << 28
WRAPS, FILTERS = {REPEAT: "repeat", CLAMP: "clamp"}, {NEAREST: "nearest", BILINEAR: "bilinear"}
SMALL = dict(sizes=((64, 48, 4),), resident=None)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _tex(uvs, texels, wrap=REPEAT, filt=BILINEAR, gamma=1.0):
    return dict(uvs=uvs, texels=texels, wrap=WRAPS[wrap], filter=FILTERS[filt], gamma=gamma)


def _white():
    return np.full((1, 1, 4), 255, np.uint8)


def _scene():
    from rust_pathtracer_amd import scenes
    return scenes.mesh_texture_scene()


# ---- 1. decode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", GAMMAS)
def test_decoded_texels_equal_the_restatement(rpt, torch_cuda, oracle, gamma):
    s, uvs = _scene()
    every = np.zeros((1, 256, 4), np.uint8)                          # 256 x 1: every byte value, in every channel at another place
    every[0, :, 0], every[0, :, 1], every[0, :, 2], every[0, :, 3] = np.arange(256), np.arange(256)[::-1], np.roll(np.arange(256), 77), 9
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        for img in (np.array([[[0, 255, 128, 3]]], np.uint8), random_texels(3, 5, 11), every):
            h, w = img.shape[:2]
            t.set_mesh_textures({0: _tex(uvs[0], img, gamma=gamma), 1: _tex(uvs[1], random_texels(2, 2, 12), gamma=gamma)})
            got, want = t.mesh_texture(0), restate_decode(oracle, img, gamma)
            assert got.shape == want.shape == (h, w, 4)
            assert np.array_equal(_bits(got), _bits(want)), "%dx%d at gamma %g: %d words differ" % (w, h, gamma, int((_bits(got) != _bits(want)).sum()))
            assert np.array_equal(_bits(t.mesh_texture(1)), _bits(restate_decode(oracle, random_texels(2, 2, 12), gamma))), "the second image of the call"
        # a mesh not named keeps its texels, bit for bit, though the table is made anew
        t.set_mesh_textures({1: _tex(uvs[1], random_texels(4, 4, 13), gamma=gamma)})
        assert np.array_equal(_bits(t.mesh_texture(0)), _bits(restate_decode(oracle, every, gamma)))
        assert np.array_equal(_bits(t.mesh_texture(1)), _bits(restate_decode(oracle, random_texels(4, 4, 13), gamma)))
        out = np.zeros((2, 2, 4), F)
        t.set_mesh_textures({1: None})
        assert rpt.lib().rpt_download_mesh_texture(t._h, 1, out.ctypes.data, 2, 2) == rpt._abi.RPT_ERR_INVALID_ARG
        assert b"mesh 1 is untextured" in rpt.lib().rpt_last_error(t._h)
        assert rpt.lib().rpt_download_mesh_texture(t._h, 0, out.ctypes.data, 2, 2) == rpt._abi.RPT_ERR_INVALID_ARG
        assert b"not its texture's 256 x 1" in rpt.lib().rpt_last_error(t._h)
    finally:
        t.close()


# ---- 2. the lookup at a hit -------------------------------------------------------------------------------------------------------
def _texture_query(rpt, torch, tracer, rays, flags):
    n = len(rays)
    dev = torch.from_numpy(np.ascontiguousarray(rays, dtype=F)).cuda()
    out = torch.zeros(n, 4, dtype=torch.int32, device="cuda")
    rpt._lib.check(rpt.lib().rpt_debug_mesh_texture_query(tracer._h, dev.data_ptr(), n, out.data_ptr(), flags, None), tracer._h)
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    return o[:, 0].astype(np.int64) - (o[:, 0] == 0xFFFFFFFF) * (1 << 32), o[:, 1:4].copy().view(F)


def _query_rays(scene, uvs, w, n, rng):
    """Rays aimed at random points of the meshes and, on the quad (whose s is linear along its first edge, from -1.5 to 2.5), at
    points whose s is a texel centre or a texel border of a texture `w` wide.  [n, 7] f32."""
    tris = _mesh_tris(scene).astype(np.float64)
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


def _restate_query(scene, textures, rays):
    """-> (index or -1, rgb [n, 3] f32) by the ordered loop and include/rpt.h's lookup.  `textures`: mesh -> (uvs, decoded texels
    [h, w, 4] f32, wrap, filter) or None."""
    tris = _mesh_tris(scene)
    _, index, _ = brute_force(tris, rays, False)
    corner, mesh_of, uv, first = [], [], [], 0
    for m, (v, t, _) in enumerate(scene.meshes):
        corner.append(np.asarray(t, np.int64) + first)
        mesh_of.append(np.full(len(t), m))
        uv.append(np.asarray(textures[m][0], F) if textures.get(m) else np.zeros((len(v), 2), F))
        first += len(v)
    corner, mesh_of, uv = np.concatenate(corner), np.concatenate(mesh_of), np.concatenate(uv)
    rgb = np.zeros((len(rays), 3), F)
    for m, (_, _, mat) in enumerate(scene.meshes):
        sel = np.nonzero((index >= 0) & (mesh_of[np.maximum(index, 0)] == m))[0]
        base = np.array(scene.materials[mat].fields["rgb"], F)
        rgb[sel] = base
        if not textures.get(m) or not len(sel):
            continue
        k = index[sel]
        _, texels, wrap, filt = textures[m]
        s, t = restate_hit_st(rays[sel, 0:3], rays[sel, 3:6], tris[k, 0], tris[k, 1] - tris[k, 0], tris[k, 2] - tris[k, 0],
                              uv[corner[k, 0]], uv[corner[k, 1]], uv[corner[k, 2]])
        rgb[sel] = base * restate_lookup(texels, wrap, filt, s, t)
        assert rgb.dtype == F
    return index, rgb


@pytest.mark.parametrize("size", SIZES, ids=lambda wh: "%dx%d" % wh)
def test_hit_colours_equal_the_numpy_restatement(rpt, torch_cuda, oracle, size):
    """4096 rays, through the walk and the ordered loop, for the four wrap x filter pairs: mesh 0 takes one pair and mesh 1 the
    opposite one, then the other way round."""
    w, h = size
    s, uvs = _scene()
    rng = np.random.default_rng(7000 + 16 * w + h)
    rays = _query_rays(s, uvs, w, 4096, rng)
    imgs = [random_texels(w, h, 70 + w), random_texels(w, h, 90 + h)]
    t = rpt.Tracer(s, device=0, seed=2)
    try:
        seen = set()
        for wrap0, filt0 in ((REPEAT, BILINEAR), (CLAMP, BILINEAR), (REPEAT, NEAREST), (CLAMP, NEAREST)):
            pairs = [(wrap0, filt0), (1 - wrap0, 1 - filt0)]
            t.set_mesh_textures({m: _tex(uvs[m], imgs[m], pairs[m][0], pairs[m][1], 2.2) for m in (0, 1)})
            textures = {m: (uvs[m], restate_decode(oracle, imgs[m], 2.2), pairs[m][0], pairs[m][1]) for m in (0, 1)}
            index, want = _restate_query(s, textures, rays)
            for brute in (False, True):
                got_i, got = _texture_query(rpt, torch_cuda, t, rays, rpt._abi.RPT_MESH_QUERY_BRUTE if brute else 0)
                assert np.array_equal(got_i, index), "index (brute %s): %d rays differ" % (brute, int((got_i != index).sum()))
                bad = np.nonzero((_bits(got) != _bits(want)).any(axis=1))[0]
                assert len(bad) == 0, "%s (brute %s): %d rays differ, first %s: got %s want %s" % (pairs, brute, len(bad), bad[:3], got[bad[:3]], want[bad[:3]])
            seen.update(pairs)
            assert (index >= 80).mean() > 0.2 and ((index >= 0) & (index < 80)).mean() > 0.1, "both meshes are hit"
        assert len(seen) == 4
    finally:
        t.close()


def test_the_hook_needs_a_texture(rpt, torch_cuda):
    s, uvs = _scene()
    t = rpt.Tracer(s, device=0, seed=2)
    try:
        rays = torch_cuda.zeros(7, device="cuda")
        out = torch_cuda.zeros(4, dtype=torch_cuda.int32, device="cuda")
        assert rpt.lib().rpt_debug_mesh_texture_query(t._h, rays.data_ptr(), 1, out.data_ptr(), 0, None) == rpt._abi.RPT_ERR_INVALID_ARG
        assert b"no mesh is textured" in rpt.lib().rpt_last_error(t._h)
    finally:
        t.close()


# ---- 3. identity and constant colour: the textured kernels against the ones the oracle pins ------------------------------------------
def _light_scene():
    from rust_pathtracer_amd import scenes
    s = scenes.mesh_light_scene(sphere_light=True)
    uvs = [scenes.spherical_uvs(v, (0.0, 0.0, 0.0)) for v, _, _ in s.meshes]
    return s, uvs


@pytest.mark.parametrize("form", ["flat", "smooth", "on", "smooth+on"])
def test_a_white_texture_is_the_untextured_frame(rpt, torch_cuda, form):
    s, uvs = _light_scene()
    t = rpt.Tracer(s, device=0, seed=4)
    try:
        if "smooth" in form:
            t.set_mesh_shading({0: "smooth"})
        if "on" in form:
            t.set_mesh_lights({1: True})
        base = (SMOOTH_BIT if "smooth" in form else 0) | (LIGHT_BIT if "on" in form else 0) | MESH_BIT
        plain = _frames(rpt, t, **SMALL)
        assert _choice(rpt, t) & (MESH_BIT | SMOOTH_BIT | LIGHT_BIT | TEX_BIT) == base
        t.set_mesh_textures({m: _tex(uvs[m], _white(), REPEAT, NEAREST, 2.2) for m in (0, 1)})
        white = _frames(rpt, t, **SMALL)
        assert _choice(rpt, t) & (MESH_BIT | SMOOTH_BIT | LIGHT_BIT | TEX_BIT) == base | TEX_BIT
        _assert_frames(white, plain, "%s: a 1x1 white texture" % form)
        assert np.isfinite(plain[0]).all() and plain[0][..., :3].mean() > 0.005
    finally:
        t.close()


@pytest.mark.parametrize("mesh", [0, 1])
def test_a_one_texel_texture_is_the_material_with_the_products(rpt, torch_cuda, oracle, mesh):
    s, uvs = _scene()
    k = (200, 90, 33)
    L = restate_decode_table(oracle, 2.2)
    t = rpt.Tracer(s, device=0, seed=5)
    try:
        img = np.array([[[k[0], k[1], k[2], 0]]], np.uint8)
        t.set_mesh_textures({mesh: _tex(uvs[mesh], img, CLAMP, NEAREST, 2.2)})
        got = _frames(rpt, t, **SMALL)
        assert _choice(rpt, t) & TEX_BIT
    finally:
        t.close()
    s2, _ = _scene()
    fields = s2.materials[s2.meshes[mesh][2]].fields
    fields["rgb"] = tuple(float(F(c) * L[kc]) for c, kc in zip(fields["rgb"], k))
    b = rpt.Tracer(s2, device=0, seed=5)
    try:
        want = _frames(rpt, b, **SMALL)
        assert not _choice(rpt, b) & TEX_BIT
    finally:
        b.close()
    _assert_frames(got, want, "a 1x1 texture of %s on mesh %d" % (k, mesh))


def test_a_checker_changes_the_frame_and_both_colours_occur(rpt, torch_cuda):
    from rust_pathtracer_amd import scenes
    s, uvs = _scene()
    t = rpt.Tracer(s, device=0, seed=6)
    try:
        plain = _frames(rpt, t, **SMALL)
        t.set_mesh_textures({0: _tex(uvs[0], scenes.checker_texture(16, 16, (255, 255, 255), (0, 0, 0), cells=4), REPEAT, NEAREST, 1.0)})
        assert not _same(_frames(rpt, t, **SMALL)[0], plain[0])
        rays = _query_rays(s, uvs, 16, 2048, np.random.default_rng(5))
        index, rgb = _texture_query(rpt, torch_cuda, t, rays, 0)
        on0 = rgb[(index >= 0) & (index < 80)]
        base = np.array(s.materials[0].fields["rgb"], F)
        is_a, is_b = (on0 == base).all(axis=1), (on0 == 0).all(axis=1)
        assert (is_a | is_b).all() and is_a.sum() > 50 and is_b.sum() > 50
        assert (rgb[index >= 80] == np.array(s.materials[1].fields["rgb"], F)).all(), "the untextured mesh keeps its colour"
    finally:
        t.close()


# ---- 4. moves ---------------------------------------------------------------------------------------------------------------------
MATRIX = np.array([[0.96, -0.28, 0.0, 0.05], [0.28, 0.96, 0.0, -0.02], [0.0, 0.0, 1.25, 0.01]], F)


def _move_textures(scene):
    from rust_pathtracer_amd import scenes
    uvs = [scenes.spherical_uvs(v, 0.5 * (np.asarray(v).min(0) + np.asarray(v).max(0))) for v, _, _ in scene.meshes]
    return {0: _tex(uvs[0], random_texels(5, 3, 31), REPEAT, BILINEAR, 2.2), 1: _tex(uvs[1] * F(3), random_texels(4, 7, 32), CLAMP, NEAREST, 1.0)}


def _fresh(rpt, arrays):
    """The yardstick: a fresh context that uploads the scene with these positions and then sets the same textures."""
    b = rpt.Tracer(_with_vertices(_small_scene, arrays), device=0, seed=8)
    try:
        b.set_mesh_textures(_move_textures(_small_scene()))
        return _frames(rpt, b, **SMALL)
    finally:
        b.close()


@pytest.mark.parametrize("form", ["update", "rebuild", "update_device", "rebuild_device"])
def test_textured_frames_follow_every_kind_of_move(rpt, torch_cuda, form):
    from rust_pathtracer_amd import scenes
    s = _small_scene()
    rest = [np.array(v, F, copy=True) for v, _, _ in s.meshes]
    t = rpt.Tracer(s, device=0, seed=8)
    try:
        t.set_mesh_textures(_move_textures(s))
        still = _frames(rpt, t, **SMALL)
        _assert_frames(still, _fresh(rpt, rest), "before any move")
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
        assert _choice(rpt, t) & TEX_BIT
        _assert_frames(got, _fresh(rpt, held), "%s: against a fresh upload" % form)
        assert not _same(got[0], still[0])
        # a rebuild with unchanged positions reorders slots and leaves the hook's answers word for word
        tris = np.concatenate([v[np.asarray(i, np.int64)] for v, (_, i, _) in zip(held, s.meshes)]).astype(np.float64)
        rng = np.random.default_rng(9)
        tri = tris[rng.integers(0, len(tris), 2048)]
        tgt = (rng.dirichlet([1, 1, 1], 2048)[:, :, None] * tri).sum(1)
        o = np.array([0.0, 0.3, 3.0]) + rng.normal(size=(2048, 3)) * 0.5
        rays = np.concatenate([o, tgt - o, np.full((2048, 1), 3.0e38)], 1).astype(F)
        before = _texture_query(rpt, torch_cuda, t, rays, 0)
        assert rpt.lib().rpt_rebuild_meshes(t._h, None, 0) == rpt._abi.RPT_OK
        after = _texture_query(rpt, torch_cuda, t, rays, 0)
        assert np.array_equal(before[0], after[0]) and np.array_equal(_bits(before[1]), _bits(after[1])) and (before[0] >= 0).mean() > 0.5
        _assert_frames(_frames(rpt, t, **SMALL), got, "after rpt_rebuild_meshes(ctx, NULL, 0)")
    finally:
        t.close()


# ---- 5. lifetime ------------------------------------------------------------------------------------------------------------------
def test_bit_28_and_the_way_back(rpt, torch_cuda):
    s, uvs = _scene()
    t = rpt.Tracer(s, device=0, seed=9)
    try:
        never = _frames(rpt, t, **SMALL)
        assert not _choice(rpt, t) & TEX_BIT
        t.set_mesh_textures({m: _tex(uvs[m], random_texels(3, 5, 60 + m)) for m in (0, 1)})
        both = _frames(rpt, t, **SMALL)
        assert _choice(rpt, t) & TEX_BIT and not _same(both[0], never[0])
        t.set_mesh_textures({0: None})
        one = _frames(rpt, t, **SMALL)
        assert _choice(rpt, t) & TEX_BIT and not _same(one[0], never[0]) and not _same(one[0], both[0])
        t.set_mesh_textures({1: None})
        _assert_frames(_frames(rpt, t, **SMALL), never, "the last texture removed")
        assert _choice(rpt, t) & (MESH_BIT | SMOOTH_BIT | LIGHT_BIT | TEX_BIT) == MESH_BIT
        t.set_mesh_textures({0: None, 1: None})                      # removing what is not there is no error
        t.set_mesh_textures({m: _tex(uvs[m], random_texels(3, 5, 60 + m)) for m in (0, 1)})
        _assert_frames(_frames(rpt, t, **SMALL), both, "the same textures again")
        t.upload_scene()                                             # an upload drops the textures
        _assert_frames(_frames(rpt, t, **SMALL), never, "after rpt_upload_scene")
        assert not _choice(rpt, t) & TEX_BIT
        out = np.zeros((5, 3, 4), F)
        assert rpt.lib().rpt_download_mesh_texture(t._h, 0, out.ctypes.data, 3, 5) == rpt._abi.RPT_ERR_INVALID_ARG
        assert rpt.lib().rpt_set_mesh_textures(t._h, None, 0) == rpt._abi.RPT_OK
    finally:
        t.close()


def test_every_answer_and_a_rejected_call_changes_nothing(rpt, torch_cuda):
    A, lib = rpt._abi, rpt.lib()
    s, uvs = _scene()
    t = rpt.Tracer(s, device=0, seed=10)
    try:
        t.set_mesh_textures({0: _tex(uvs[0], random_texels(3, 5, 61), CLAMP, BILINEAR, 2.2)})
        ref = _frames(rpt, t, **SMALL)
        held = t.mesh_texture(0).copy()
        img = np.ascontiguousarray(random_texels(2, 2, 62))
        fptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))       # noqa: E731
        bptr = img.ctypes.data_as(C.POINTER(C.c_uint8))

        def items(*rows):
            arr = (A.rpt_mesh_texture * len(rows))()
            for it, r in zip(arr, rows):
                r = dict(dict(mesh=1, n_vertices=4, uvs=fptr(uvs[1]), width=2, height=2, texels=bptr, wrap=0, filter=0, gamma=1.0), **r)
                for key, val in r.items():
                    setattr(it, key, val)
            return arr

        nan, far = uvs[1].copy(), uvs[1].copy()
        nan[2, 1], far[3, 0] = np.nan, F(2.0 ** 20 + 1)
        cases = [("NULL items", None, 1, "items is NULL"),
                 ("mesh out of range", items(dict(mesh=2)), 1, "mesh 2 out of range"),
                 ("named twice", items(dict(), dict()), 2, "item 1: mesh 1 is named twice"),
                 ("n_vertices", items(dict(n_vertices=3)), 1, "mesh 1: n_vertices 3"),
                 ("NULL uvs", items(dict(uvs=None)), 1, "uvs is NULL"),
                 ("width 0", items(dict(width=0)), 1, "a texture of 0 x 2"),
                 ("height above 16384", items(dict(height=16385)), 1, "a texture of 2 x 16385"),
                 ("NULL texels", items(dict(texels=None)), 1, "texels is NULL"),
                 ("wrap", items(dict(wrap=2)), 1, "wrap 2"),
                 ("filter", items(dict(filter=5)), 1, "filter 5"),
                 ("gamma 0", items(dict(gamma=0.0)), 1, "gamma"),
                 ("gamma NaN", items(dict(gamma=float("nan"))), 1, "gamma"),
                 ("gamma above 16", items(dict(gamma=16.5)), 1, "gamma"),
                 ("a NaN UV", items(dict(uvs=fptr(nan))), 1, "mesh 1: vertex 2"),
                 ("a UV beyond 2^20", items(dict(uvs=fptr(far))), 1, "mesh 1: vertex 3")]
        for what, arr, n, says in cases:
            assert lib.rpt_set_mesh_textures(t._h, arr, n) == A.RPT_ERR_INVALID_ARG, what
            err = lib.rpt_last_error(t._h).decode()
            assert err.startswith("rpt_set_mesh_textures: ") and says in err, (what, err)
            assert np.array_equal(_bits(t.mesh_texture(0)), _bits(held)), what
        # sizes whose sum passes 2^26 texels: refused on the host from the sizes alone (the texels are never read)
        big = items(dict(width=8192, height=8192))
        assert lib.rpt_set_mesh_textures(t._h, big, 1) == A.RPT_ERR_UNSUPPORTED and "2^26" in lib.rpt_last_error(t._h).decode()
        _assert_frames(_frames(rpt, t, **SMALL), ref, "after every rejected call")
        assert _choice(rpt, t) & TEX_BIT
        assert lib.rpt_set_mesh_textures(t._h, None, 0) == A.RPT_OK
        # no scene with meshes
        from rust_pathtracer_amd import scenes
        b = rpt.Tracer(scenes.six_primitive_scene(), device=0, seed=1)
        try:
            assert lib.rpt_set_mesh_textures(b._h, items(dict()), 1) == A.RPT_ERR_NO_SCENE
            assert lib.rpt_set_mesh_textures(b._h, None, 0) == A.RPT_ERR_NO_SCENE
            out = np.zeros(16, F)
            assert lib.rpt_download_mesh_texture(b._h, 0, out.ctypes.data, 2, 2) == A.RPT_ERR_NO_SCENE
        finally:
            b.close()
    finally:
        t.close()


def test_a_device_listed_twice_renders_the_one_context_frame(rpt, torch_cuda):
    s, uvs = _scene()
    tex = {m: _tex(uvs[m], random_texels(3, 5, 80 + m), REPEAT, BILINEAR, 2.2) for m in (0, 1)}
    w, h, spp = 64, 48, 4
    t = rpt.Tracer(s, device=0, seed=11)
    try:
        t.set_mesh_textures(tex)
        t.render_resident(w, h, spp)
        one = t.resident_to_host(w, h).pixels.reshape(h, w, 4).copy()
    finally:
        t.close()
    m = rpt.Tracer(_scene()[0], devices=[0, 0], seed=11)
    try:
        m.set_mesh_textures(tex)
        m.render_resident(w, h, spp)
        assert _choice(rpt, m) & TEX_BIT
        assert _same(m.resident_to_host(w, h).pixels.reshape(h, w, 4), one)
        m.set_mesh_textures({0: None, 1: None})
        m.resident_reset()
        m.render_resident(w, h, spp)
        assert not _choice(rpt, m) & TEX_BIT
    finally:
        m.close()
