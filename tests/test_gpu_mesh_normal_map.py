"""Mesh normal maps on the device (include/rpt.h, "mesh normal maps"): decoded texels and probed hit normals equal the numpy float32
restatement bit for bit; a flat map, and any map at strength 0, is the frame without a map in each of the kernel forms — with bit 31
of the kernel choice set, so the new kernels ran; a bump map changes the frame, and where it does depends on the mesh that carries
it; every kind of move gives the frames of a fresh upload; removal restores the kernel choice and the frames; every rejected call
says why and changes nothing.  Frames are 32 x 24, meshes tens to a few hundred triangles."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_mesh import _mesh_tris
from test_gpu_mesh_smooth import _restate_query as _restate_normals
from test_gpu_mesh_texture import _move_textures, _query_rays, _tex, _white
from test_gpu_mesh_update import _assert_frames, _choice, _frames, _same, _small_scene, _with_vertices
from test_mesh_normal_map_host import restate_decode, restate_shade
from test_mesh_smooth_host import _cross, _dot
from test_mesh_texture_host import BILINEAR, CLAMP, NEAREST, REPEAT, random_texels

pytestmark = pytest.mark.gpu
F = np.float32
MESH_BIT, SMOOTH_BIT, LIGHT_BIT, TEX_BIT, ENV_BIT, CUT_BIT, NRM_BIT = 1 << 25, 1 << 26, 1 << 27, 1 << 28, 1 << 29, 1 << 30, 1 << 31
EVERY = MESH_BIT | SMOOTH_BIT | LIGHT_BIT | TEX_BIT | ENV_BIT | CUT_BIT | NRM_BIT
SMALL = dict(sizes=((32, 24, 4),), resident=None)
MATRIX = np.array([[0.96, -0.28, 0.0, 0.05], [0.28, 0.96, 0.0, -0.02], [0.0, 0.0, 1.25, 0.01]], F)
FILTERS = {NEAREST: "nearest", BILINEAR: "bilinear"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _flat_map(w=3, h=2):
    m = np.zeros((h, w, 4), np.uint8)
    m[...] = (128, 128, 255, 7)
    return m


def _blue_map(w, h, seed):
    """Random red and green, blue 255: bent at any strength but 0."""
    m = random_texels(w, h, seed)
    m[..., 2] = 255
    return m


def _nmap(texels, filt=BILINEAR, flip=False, strength=1.0):
    return dict(texels=texels, filter=FILTERS[filt], flip_green=flip, strength=strength)


def _bump():
    from rust_pathtracer_amd import scenes
    return scenes.mesh_normal_map_scene()[2]


# ---- 1. decode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip-green"])
def test_decoded_texels_equal_the_restatement(rpt, torch_cuda, flip):
    from rust_pathtracer_amd import scenes
    s, uvs = scenes.mesh_texture_scene()
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        t.set_mesh_textures({m: _tex(uvs[m], _white()) for m in (0, 1)})
        every = random_texels(64, 64, 13)
        every.reshape(-1, 4)[:256, 0], every.reshape(-1, 4)[:256, 1], every.reshape(-1, 4)[:256, 2] = np.arange(256), np.arange(256)[::-1], np.roll(np.arange(256), 77)
        for img, strength in ((np.array([[[0, 255, 128, 3]]], np.uint8), 1.0), (random_texels(5, 3, 11), 2.5), (every, 0.75), (every, 0.0)):
            h, w = img.shape[:2]
            other = random_texels(2, 2, 12)
            t.set_mesh_normal_maps({0: _nmap(img, NEAREST, flip, strength), 1: _nmap(other, BILINEAR, not flip, 16.0)})
            got, want = t.mesh_normal_map(0), restate_decode(img, strength, flip)
            assert got.shape == want.shape == (h, w, 4)
            assert np.array_equal(_bits(got), _bits(want)), "%dx%d at strength %g: %d words differ" % (w, h, strength, int((_bits(got) != _bits(want)).sum()))
            assert np.array_equal(_bits(t.mesh_normal_map(1)), _bits(restate_decode(other, 16.0, not flip))), "the second map of the call"
        # a mesh not named keeps its texels, bit for bit, though the table is made anew
        t.set_mesh_normal_maps({1: _nmap(random_texels(4, 4, 14), NEAREST, flip, 1.0)})
        assert np.array_equal(_bits(t.mesh_normal_map(0)), _bits(restate_decode(every, 0.0, flip)))
        assert np.array_equal(_bits(t.mesh_normal_map(1)), _bits(restate_decode(random_texels(4, 4, 14), 1.0, flip)))
        out = np.zeros((2, 2, 4), F)
        t.set_mesh_normal_maps({1: None})
        assert rpt.lib().rpt_download_mesh_normal_map(t._h, 1, out.ctypes.data, 2, 2) == rpt._abi.RPT_ERR_INVALID_ARG
        assert b"mesh 1 has no normal map" in rpt.lib().rpt_last_error(t._h)
        assert rpt.lib().rpt_download_mesh_normal_map(t._h, 0, out.ctypes.data, 2, 2) == rpt._abi.RPT_ERR_INVALID_ARG
        assert b"not its map's 64 x 64" in rpt.lib().rpt_last_error(t._h)
        assert rpt.lib().rpt_download_mesh_normal_map(t._h, 0, None, 64, 64) == rpt._abi.RPT_ERR_INVALID_ARG
        assert rpt.lib().rpt_download_mesh_normal_map(t._h, 2, out.ctypes.data, 2, 2) == rpt._abi.RPT_ERR_INVALID_ARG
    finally:
        t.close()


# ---- 2. the normal at a hit -------------------------------------------------------------------------------------------------------
def _probe_scene():
    """mesh_texture_scene() with the quad's UVs mirrored in s (D < 0 on both of its triangles) and, as mesh 2, one triangle whose
    first two corners share a UV (D == 0: its hits keep their normal)."""
    from rust_pathtracer_amd import scenes
    s, uvs = scenes.mesh_texture_scene()
    quad_uv = uvs[1].copy()
    quad_uv[:, 0] = F(1.0) - quad_uv[:, 0]
    tri = np.array([[-1.6, -0.4, 0.2], [-0.9, -0.45, 0.4], [-1.3, 0.5, 0.3]], F)
    s.meshes.append((tri, np.array([[0, 1, 2]], np.uint32), 1))
    return s, [uvs[0], quad_uv, np.array([[0.3, 0.3], [0.3, 0.3], [0.7, 0.9]], F)]


def _normal_map_query(rpt, torch, tracer, rays, flags):
    n = len(rays)
    dev = torch.from_numpy(np.ascontiguousarray(rays, dtype=F)).cuda()
    out = torch.zeros(n, 4, dtype=torch.int32, device="cuda")
    rpt._lib.check(rpt.lib().rpt_debug_mesh_normal_map_query(tracer._h, dev.data_ptr(), n, out.data_ptr(), flags, None), tracer._h)
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    return o[:, 0].astype(np.int64) - (o[:, 0] == 0xFFFFFFFF) * (1 << 32), o[:, 1:4].copy().view(F)


def _restate_probe(scene, smooth, uvs, wraps, maps, rays):
    """-> (index or -1, normal [n, 3] f32, D per ray (NaN: no map), which mapped hits fell back) by the ordered loop, "smooth mesh
    shading"'s normal and include/rpt.h's lookup and bend.  `maps`: mesh -> (decoded texels [h, w, 4] f32, filter) or absent."""
    tris = _mesh_tris(scene)
    index, want, _ = _restate_normals(scene, smooth, rays)
    corner, mesh_of, uv, first = [], [], [], 0
    for m, (v, t, _) in enumerate(scene.meshes):
        corner.append(np.asarray(t, np.int64).reshape(-1, 3) + first)
        mesh_of.append(np.full(len(corner[-1]), m))
        uv.append(np.asarray(uvs[m], F))
        first += len(v)
    corner, mesh_of, uv = np.concatenate(corner), np.concatenate(mesh_of), np.concatenate(uv)
    det, fell = np.full(len(rays), np.nan), np.zeros(len(rays), bool)
    for m in maps:
        sel = np.nonzero((index >= 0) & (mesh_of[np.maximum(index, 0)] == m))[0]
        if not len(sel):
            continue
        k = index[sel]
        o, d, a, e1, e2 = rays[sel, 0:3], rays[sel, 3:6], tris[k, 0], tris[k, 1] - tris[k, 0], tris[k, 2] - tris[k, 0]
        with np.errstate(all="ignore"):                             # u and v of the triangle test, as "smooth mesh shading" restates them
            p = _cross(d, e2)
            inv = F(1.0) / _dot(e1, p)
            sv = o - a
            u = _dot(sv, p) * inv
            v = _dot(d, _cross(sv, e1)) * inv
        texels, filt = maps[m]
        want[sel], fell[sel], det[sel], _ = restate_shade(want[sel], e1, e2, u, v, uv[corner[k, 0]], uv[corner[k, 1]], uv[corner[k, 2]], texels, wraps[m], filt)
    assert want.dtype == F
    return index, want, det, fell


@pytest.mark.parametrize("smooth", [(), (0, 1)], ids=["flat", "smooth"])
def test_probed_normals_equal_the_numpy_restatement(rpt, torch_cuda, smooth):
    """2048 rays, through the walk and the ordered loop, for the four wrap x filter pairs: mesh 0 takes one pair and mesh 1 the opposite
    one; mesh 1's UVs are mirrored, mesh 2's triangle has degenerate UVs, the icosphere's seam triangles have long UV edges."""
    s, uvs = _probe_scene()
    rng = np.random.default_rng(8100 + len(smooth))
    rays = _query_rays(s, uvs, 5, 2048, rng)
    imgs = {0: random_texels(5, 3, 71), 1: random_texels(16, 16, 72), 2: random_texels(2, 2, 73)}
    t = rpt.Tracer(s, device=0, seed=2)
    try:
        if smooth:
            t.set_mesh_shading({m: "smooth" for m in smooth})
        for wrap0, filt0 in ((REPEAT, BILINEAR), (CLAMP, BILINEAR), (REPEAT, NEAREST), (CLAMP, NEAREST)):
            wraps, filts = {0: wrap0, 1: 1 - wrap0, 2: wrap0}, {0: filt0, 1: 1 - filt0, 2: filt0}
            t.set_mesh_textures({m: _tex(uvs[m], _white(), wraps[m], NEAREST) for m in (0, 1, 2)})     # (the colour filter is not the map's)
            t.set_mesh_normal_maps({0: _nmap(imgs[0], filts[0], False, 2.5), 1: _nmap(imgs[1], filts[1], True, 1.0), 2: _nmap(imgs[2], filts[2], False, 1.0)})
            maps = {0: (restate_decode(imgs[0], 2.5, False), filts[0]), 1: (restate_decode(imgs[1], 1.0, True), filts[1]),
                    2: (restate_decode(imgs[2], 1.0, False), filts[2])}
            index, want, det, fell = _restate_probe(s, smooth, uvs, wraps, maps, rays)
            for brute in (False, True):
                got_i, got = _normal_map_query(rpt, torch_cuda, t, rays, rpt._abi.RPT_MESH_QUERY_BRUTE if brute else 0)
                assert np.array_equal(got_i, index), "index (brute %s): %d rays differ" % (brute, int((got_i != index).sum()))
                bad = np.nonzero((_bits(got) != _bits(want)).any(axis=1))[0]
                assert len(bad) == 0, "wrap %s filter %s (brute %s): %d rays differ, first %s: got %s want %s" % (
                    wraps, filts, brute, len(bad), bad[:3], got[bad[:3]], want[bad[:3]])
            hit = index >= 0
            assert (index[hit] < 80).mean() > 0.1 and ((index >= 80) & (index < 82)).mean() > 0.2 and (index == 82).sum() >= 3, "all three meshes are hit"
            assert (det[(index >= 80) & (index < 82)] < 0).all() and (det[hit] > 0).any(), "mirrored and unmirrored UVs"
            assert (det[index == 82] == 0).all() and fell[index == 82].all(), "the degenerate triangle keeps its normal"
            bent = hit & ~fell
            base = _restate_normals(s, smooth, rays)[1]
            assert bent.mean() > 0.3 and (np.abs(want[bent] - base[bent]).max(axis=1) > 1e-3).mean() > 0.9, "the map bends"
        # one mesh only, the others untouched
        t.set_mesh_normal_maps({0: None, 2: None})
        index, want, _, _ = _restate_probe(s, smooth, uvs, wraps, {1: maps[1]}, rays)
        got_i, got = _normal_map_query(rpt, torch_cuda, t, rays, 0)
        assert np.array_equal(got_i, index) and np.array_equal(_bits(got), _bits(want))
    finally:
        t.close()


def test_the_hook_needs_a_normal_map(rpt, torch_cuda):
    s, uvs = _probe_scene()
    t = rpt.Tracer(s, device=0, seed=2)
    try:
        t.set_mesh_textures({0: _tex(uvs[0], _white())})
        rays = torch_cuda.zeros(7, device="cuda")
        out = torch_cuda.zeros(4, dtype=torch_cuda.int32, device="cuda")
        assert rpt.lib().rpt_debug_mesh_normal_map_query(t._h, rays.data_ptr(), 1, out.data_ptr(), 0, None) == rpt._abi.RPT_ERR_INVALID_ARG
        assert b"no mesh has a normal map" in rpt.lib().rpt_last_error(t._h)
        t.set_mesh_normal_maps({0: _flat_map()})
        assert rpt.lib().rpt_debug_mesh_normal_map_query(t._h, rays.data_ptr(), 1, out.data_ptr(), 4, None) == rpt._abi.RPT_ERR_INVALID_ARG
        assert rpt.lib().rpt_debug_mesh_normal_map_query(t._h, rays.data_ptr(), 1, out.data_ptr(), 0, None) == rpt._abi.RPT_OK
    finally:
        t.close()


# ---- 3. identity: a flat map, or strength 0, is no map -------------------------------------------------------------------------------
def _form_context(rpt, form, seed=4):
    """A context in one of the kernel forms a normal map renders over, both meshes textured; -> (tracer, the bits it must show)."""
    from rust_pathtracer_amd import scenes
    if form == "light":
        s = scenes.mesh_light_scene(sphere_light=True)                # mesh 0 the object, mesh 1 the lamp
        uvs = [scenes.spherical_uvs(v, (0.0, 0.0, 0.0)) for v, _, _ in s.meshes]
    else:
        s, uvs = scenes.mesh_texture_scene()
    t = rpt.Tracer(s, device=0, seed=seed)
    t.set_mesh_textures({0: _tex(uvs[0], random_texels(5, 3, 21), REPEAT, BILINEAR, 2.2), 1: _tex(uvs[1], random_texels(4, 4, 22), CLAMP, NEAREST)})
    t.set_mesh_shading({0: "smooth"})
    bits = MESH_BIT | TEX_BIT | SMOOTH_BIT
    if form == "light":
        t.set_mesh_lights({1: True})
        bits |= LIGHT_BIT
    if "environment" in form:
        t.set_environment(scenes.mesh_env_scene(16)[1], 1.0, sampled=True)
        bits |= ENV_BIT
    if "cutout" in form:
        t.set_mesh_cutouts({1: scenes.checker_mask(8, 8, 4)})
        bits |= CUT_BIT
    return t, bits


FORMS = ["plain", "light", "environment", "cutout", "cutout+environment"]


@pytest.mark.parametrize("form", FORMS)
def test_a_flat_map_and_strength_zero_are_the_frame_without_a_map(rpt, torch_cuda, form):
    """This test fails without the feature: bit 31 says that k_nrm.hip's kernel of the form ran."""
    t, bits = _form_context(rpt, form)
    try:
        plain = _frames(rpt, t, **SMALL)
        assert _choice(rpt, t) & EVERY == bits
        assert np.isfinite(plain[0]).all() and plain[0][..., :3].mean() > 0.005
        t.set_mesh_normal_maps({0: _nmap(_flat_map(3, 2), BILINEAR), 1: _nmap(_flat_map(1, 1), NEAREST, True, 16.0)})
        _assert_frames(_frames(rpt, t, **SMALL), plain, "%s: an all-(128, 128, 255) map" % form)
        assert _choice(rpt, t) & EVERY == bits | NRM_BIT, "the normal-mapped kernel ran"
        t.set_mesh_normal_maps({0: _nmap(_blue_map(7, 5, 23), BILINEAR, False, 0.0), 1: _nmap(_blue_map(4, 4, 24), NEAREST, True, 0.0)})
        _assert_frames(_frames(rpt, t, **SMALL), plain, "%s: strength 0" % form)
        assert _choice(rpt, t) & EVERY == bits | NRM_BIT
        t.set_mesh_normal_maps({0: _nmap(_blue_map(7, 5, 23), BILINEAR, False, 1.0)})     # the same map at strength 1 is no identity
        assert not _same(_frames(rpt, t, **SMALL)[0], plain[0]), "%s: the map bends at strength 1" % form
    finally:
        t.close()


# ---- 4. a bump map changes the frame, where its mesh is ------------------------------------------------------------------------------
def test_a_bump_map_changes_the_frame_and_the_mesh_that_carries_it(rpt, torch_cuda):
    t, bits = _form_context(rpt, "plain", seed=5)
    try:
        plain = _frames(rpt, t, **SMALL)[0]
        bump = _bump()
        t.set_mesh_normal_maps({0: _nmap(bump, BILINEAR, False, 2.0)})
        on0 = _frames(rpt, t, **SMALL)[0]
        t.set_mesh_normal_maps({0: None, 1: _nmap(bump, BILINEAR, False, 2.0)})
        on1 = _frames(rpt, t, **SMALL)[0]
        d0, d1 = (_bits(on0) != _bits(plain)).any(axis=2), (_bits(on1) != _bits(plain)).any(axis=2)
        assert d0.sum() >= 10 and d1.sum() >= 10, "either mesh's map changes pixels"
        assert (d0 & ~d1).sum() >= 5 and (d1 & ~d0).sum() >= 5, "and they are other pixels"
        assert np.isfinite(on0).all() and np.isfinite(on1).all()
        t.set_mesh_normal_maps({1: _nmap(bump, BILINEAR, True, 2.0)})
        assert not _same(_frames(rpt, t, **SMALL)[0], on1), "FLIP_GREEN is another map"
    finally:
        t.close()


# ---- 5. moves ---------------------------------------------------------------------------------------------------------------------
def _move_maps():
    return {0: _nmap(_blue_map(12, 6, 41), BILINEAR, False, 2.0), 1: _nmap(_blue_map(9, 9, 42), NEAREST, True, 1.0)}


def _fresh(rpt, arrays):
    """The yardstick: a fresh context that uploads the scene with these positions and then makes the same set calls."""
    b = rpt.Tracer(_with_vertices(_small_scene, arrays), device=0, seed=8)
    try:
        b.set_mesh_textures(_move_textures(_small_scene()))
        b.set_mesh_shading({1: "smooth"})
        b.set_mesh_normal_maps(_move_maps())
        return _frames(rpt, b, **SMALL)
    finally:
        b.close()


@pytest.mark.parametrize("form", ["update", "rebuild", "update_device", "rebuild_device"])
def test_normal_mapped_frames_follow_every_kind_of_move(rpt, torch_cuda, form):
    from rust_pathtracer_amd import scenes
    s = _small_scene()
    rest = [np.array(v, F, copy=True) for v, _, _ in s.meshes]
    t = rpt.Tracer(s, device=0, seed=8)
    try:
        t.set_mesh_textures(_move_textures(s))
        t.set_mesh_shading({1: "smooth"})
        unmapped = _frames(rpt, t, **SMALL)
        t.set_mesh_normal_maps(_move_maps())
        still = _frames(rpt, t, **SMALL)
        _assert_frames(still, _fresh(rpt, rest), "before any move")
        assert not _same(still[0], unmapped[0])
        held_maps = [t.mesh_normal_map(m).copy() for m in (0, 1)]
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
        assert _choice(rpt, t) & NRM_BIT
        _assert_frames(got, _fresh(rpt, held), "%s: against a fresh upload" % form)
        assert not _same(got[0], still[0])
        assert all(np.array_equal(_bits(t.mesh_normal_map(m)), _bits(held_maps[m])) for m in (0, 1)), "a move leaves the maps alone"
    finally:
        t.close()


# ---- 6. lifetime ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "cutout+environment"])
def test_bit_31_and_the_way_back(rpt, torch_cuda, form):
    t, bits = _form_context(rpt, form, seed=9)
    try:
        never = _frames(rpt, t, **SMALL)
        before = _choice(rpt, t)
        assert before & EVERY == bits
        bump = _bump()
        t.set_mesh_normal_maps({0: _nmap(bump, BILINEAR, False, 2.0), 1: _nmap(_blue_map(4, 4, 51), NEAREST)})
        both = _frames(rpt, t, **SMALL)
        assert _choice(rpt, t) == before | NRM_BIT and not _same(both[0], never[0])
        t.set_mesh_normal_maps({1: None})
        one = _frames(rpt, t, **SMALL)
        assert _choice(rpt, t) & NRM_BIT and not _same(one[0], never[0]) and not _same(one[0], both[0])
        if form == "plain":                                          # replacing a texture keeps the map; the ordinals move and move back
            from rust_pathtracer_amd import scenes
            uvs = scenes.mesh_texture_scene()[1]
            t.set_mesh_textures({0: _tex(uvs[0], random_texels(5, 3, 21), REPEAT, BILINEAR, 2.2)})
            _assert_frames(_frames(rpt, t, **SMALL), one, "the same texture again")
            t.set_mesh_textures({1: None})                           # mesh 0 stays ordinal 0; mesh 1 loses its colour
            assert np.array_equal(_bits(t.mesh_normal_map(0)), _bits(restate_decode(bump, 2.0, False)))
            t.set_mesh_textures({1: _tex(uvs[1], random_texels(4, 4, 22), CLAMP, NEAREST)})
            _assert_frames(_frames(rpt, t, **SMALL), one, "a texture removed and set again")
        t.set_mesh_normal_maps({0: None})
        _assert_frames(_frames(rpt, t, **SMALL), never, "the last map OFF")
        assert _choice(rpt, t) == before, "the kernel choice word is what it was"
        t.set_mesh_normal_maps({0: None, 1: None})                   # removing what is not there is no error
        t.set_mesh_normal_maps({0: _nmap(bump, BILINEAR, False, 2.0), 1: _nmap(_blue_map(4, 4, 51), NEAREST)})
        _assert_frames(_frames(rpt, t, **SMALL), both, "the same maps again")
        t.upload_scene()                                             # an upload drops maps (and everything else that was set)
        _frames(rpt, t, **SMALL)
        assert _choice(rpt, t) & EVERY == MESH_BIT
        out = np.zeros((4, 4, 4), F)
        assert rpt.lib().rpt_download_mesh_normal_map(t._h, 1, out.ctypes.data, 4, 4) == rpt._abi.RPT_ERR_INVALID_ARG
        assert rpt.lib().rpt_set_mesh_normal_maps(t._h, None, 0) == rpt._abi.RPT_OK
    finally:
        t.close()


def test_the_ordinals_move_under_a_normal_map(rpt, torch_cuda):
    """Textures set on OTHER meshes renumber the texture ordinals the descriptors are indexed by, and a new wrap is read at once: the
    frames are those of a context that made the calls in the plain order."""
    s, uvs = _probe_scene()
    texs = {m: _tex(uvs[m], random_texels(3, 5, 90 + m), CLAMP if m == 2 else REPEAT) for m in (0, 1, 2)}
    maps = {1: _nmap(_blue_map(6, 6, 95), BILINEAR, False, 2.0), 2: _nmap(_blue_map(3, 3, 96), NEAREST, True, 1.0)}
    a = rpt.Tracer(s, device=0, seed=14)
    try:
        a.set_mesh_textures(texs)
        a.set_mesh_normal_maps(maps)
        want = _frames(rpt, a, **SMALL)
    finally:
        a.close()
    b = rpt.Tracer(_probe_scene()[0], device=0, seed=14)
    try:
        b.set_mesh_textures({2: dict(texs[2], wrap="repeat")})       # ordinal 0, another wrap
        b.set_mesh_normal_maps({2: maps[2]})
        b.set_mesh_textures({1: texs[1]})                            # mesh 2 becomes ordinal 1
        b.set_mesh_normal_maps({1: maps[1]})
        b.set_mesh_textures({0: texs[0], 2: texs[2]})                # ordinal 2, and its wrap is CLAMP from now on
        _assert_frames(_frames(rpt, b, **SMALL), want, "the calls in another order")
    finally:
        b.close()


# ---- 7. answers -------------------------------------------------------------------------------------------------------------------
def test_every_answer_and_a_rejected_call_changes_nothing(rpt, torch_cuda):
    A, lib = rpt._abi, rpt.lib()
    from rust_pathtracer_amd import scenes
    s, uvs = scenes.mesh_texture_scene()
    t = rpt.Tracer(s, device=0, seed=10)
    try:
        t.set_mesh_textures({0: _tex(uvs[0], random_texels(3, 5, 61), CLAMP, BILINEAR, 2.2)})
        t.set_mesh_normal_maps({0: _nmap(_blue_map(6, 6, 62), BILINEAR, True, 2.0)})
        ref = _frames(rpt, t, **SMALL)
        held = t.mesh_normal_map(0).copy()
        texels = np.ascontiguousarray(random_texels(2, 2, 63))
        bptr = texels.ctypes.data_as(C.POINTER(C.c_uint8))

        def items(*rows):
            arr = (A.rpt_mesh_normal_map * len(rows))()
            for it, r in zip(arr, rows):
                r = dict(dict(mesh=0, mode=A.RPT_MESH_NORMAL_MAP_ON, width=2, height=2, texels=bptr, filter=A.RPT_TEX_FILTER_BILINEAR, flags=0, strength=1.0), **r)
                for key, val in r.items():
                    setattr(it, key, val)
            return arr

        off = dict(mode=A.RPT_MESH_NORMAL_MAP_OFF, width=0, height=0, texels=None, filter=0, flags=0, strength=0.0)
        # in the stated order; each case but the last carries the NEXT check's fault as well, so the order itself is held
        cases = [("NULL items", None, 1, "items is NULL"),
                 ("mesh out of range", items(dict(mesh=2, mode=7)), 1, "mesh 2 out of range"),
                 ("named twice", items(dict(), dict(mode=7)), 2, "item 1: mesh 0 is named twice"),
                 ("mode", items(dict(mode=2, width=0)), 1, "mode 2"),
                 ("width 0", items(dict(width=0, texels=None)), 1, "a map of 0 x 2"),
                 ("height above 16384", items(dict(height=16385, texels=None)), 1, "a map of 2 x 16385"),
                 ("NULL texels", items(dict(texels=None, filter=2)), 1, "texels is NULL"),
                 ("filter", items(dict(filter=2, flags=2)), 1, "filter 2"),
                 ("flags", items(dict(flags=6, strength=-1.0)), 1, "unknown flag bits 0x6"),
                 ("strength negative", items(dict(mesh=1, strength=-0.5)), 1, "strength"),
                 ("strength above 16", items(dict(mesh=1, strength=16.5)), 1, "strength"),
                 ("strength infinite", items(dict(mesh=1, strength=float("inf"))), 1, "strength"),
                 ("strength NaN", items(dict(mesh=1, strength=float("nan"))), 1, "strength"),
                 ("OFF with a size", items(dict(off, width=2)), 1, "RPT_MESH_NORMAL_MAP_OFF takes"),
                 ("OFF with a pointer", items(dict(off, texels=bptr)), 1, "RPT_MESH_NORMAL_MAP_OFF takes"),
                 ("untextured", items(dict(mesh=1, width=16384, height=16384)), 1, "mesh 1 is untextured")]
        for what, arr, n, says in cases:
            assert lib.rpt_set_mesh_normal_maps(t._h, arr, n) == A.RPT_ERR_INVALID_ARG, what
            err = lib.rpt_last_error(t._h).decode()
            assert err.startswith("rpt_set_mesh_normal_maps: ") and says in err, (what, err)
            assert np.array_equal(_bits(t.mesh_normal_map(0)), _bits(held)), what
        assert "1 x 1 white texture" in lib.rpt_last_error(t._h).decode()
        assert "item 0" in lib.rpt_last_error(t._h).decode()
        # sizes whose sum passes 2^26 texels: refused on the host from the sizes alone (texels is never read)
        big = items(dict(width=8192, height=8193))
        assert lib.rpt_set_mesh_normal_maps(t._h, big, 1) == A.RPT_ERR_UNSUPPORTED and "2^26" in lib.rpt_last_error(t._h).decode()
        # the texture of a normal-mapped mesh cannot be removed, alone or among others; replacing it is fine
        for gone in ({0: None}, {0: None, 1: _tex(uvs[1], _white())}):
            with pytest.raises(Exception) as e:
                t.set_mesh_textures(gone)
            assert "remove the normal map first" in str(e.value) and lib.rpt_last_error(t._h).decode().startswith("rpt_set_mesh_textures: ")
        tex = (A.rpt_mesh_texture * 1)()
        tex[0].mesh = 0
        assert lib.rpt_set_mesh_textures(t._h, tex, 1) == A.RPT_ERR_INVALID_ARG
        _assert_frames(_frames(rpt, t, **SMALL), ref, "after every rejected call")
        assert np.array_equal(_bits(t.mesh_normal_map(0)), _bits(held)) and _choice(rpt, t) & NRM_BIT
        assert lib.rpt_set_mesh_normal_maps(t._h, None, 0) == A.RPT_OK
        _assert_frames(_frames(rpt, t, **SMALL), ref, "n_items == 0 does nothing")
        t.set_mesh_normal_maps({0: None})
        t.set_mesh_textures({0: None})                               # the map removed first: now the texture goes
        assert _choice(rpt, t) & NRM_BIT                              # (last_choice is the last launch's)
        _frames(rpt, t, **SMALL)
        assert not _choice(rpt, t) & (NRM_BIT | TEX_BIT)
        # no scene with meshes
        b = rpt.Tracer(scenes.six_primitive_scene(), device=0, seed=1)
        try:
            assert lib.rpt_set_mesh_normal_maps(b._h, items(dict()), 1) == A.RPT_ERR_NO_SCENE
            assert lib.rpt_set_mesh_normal_maps(b._h, None, 0) == A.RPT_ERR_NO_SCENE
            assert lib.rpt_set_mesh_normal_maps(b._h, None, 1) == A.RPT_ERR_NO_SCENE         # no scene comes before NULL items
            out = np.zeros(4, F)
            assert lib.rpt_download_mesh_normal_map(b._h, 0, out.ctypes.data, 1, 1) == A.RPT_ERR_NO_SCENE
        finally:
            b.close()
    finally:
        t.close()
