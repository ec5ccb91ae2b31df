"""Mesh material maps on the device (include/rpt.h, "mesh material maps"): decoded texels and probed roughness / metallic equal the
numpy float32 restatement bit for bit; an all-255 map is the frame without a map in each of the eight forms — with
rpt_debug_mesh_form saying 12 .. 19, so the new kernels ran; a constant map is the frame of a scene whose material holds the float32
products; every kind of move gives the frames of a fresh upload; removal restores the form and the frames; replacing a texture keeps
the map and removing it is refused; a device listed twice renders the one-device frame; every rejected call says why and changes
nothing.  Frames are 32 x 24 at 4 spp, meshes tens to a few hundred triangles."""
import ctypes as C

import numpy as np
import pytest

import mesh_mmap_f64 as MM
from kernel_census import MESH_RENDER_KERNELS
from test_gpu_mesh_compose_f64 import CASES, inputs
from test_gpu_mesh_material_map_f64 import form_of, mesh_form, set_composed
from test_gpu_mesh_normal_map import MATRIX, _probe_scene
from test_gpu_mesh_texture import _move_textures, _query_rays, _restate_query, _tex, _texture_query, _white
from test_gpu_mesh_update import _assert_frames, _frames, _same, _small_scene, _with_vertices
from test_mesh_material_map_host import BILINEAR_CONSTANT_EXACT_BYTES, restate_apply, restate_decode, restate_value
from test_mesh_texture_host import BILINEAR, CLAMP, NEAREST, REPEAT, random_texels, restate_hit_st
from test_gpu_mesh import _mesh_tris

pytestmark = pytest.mark.gpu
F = np.float32
SMALL = dict(sizes=((32, 24, 4),), resident=None)
FILTERS = {NEAREST: "nearest", BILINEAR: "bilinear"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _mmap(texels, filt=BILINEAR, rc=1, mc=2):
    return dict(texels=texels, filter=FILTERS[filt], roughness_channel=rc, metallic_channel=mc)


def _constant(k, w=3, h=2):
    return np.full((h, w, 4), k, np.uint8)


# ---- 1. decode --------------------------------------------------------------------------------------------------------------------
def test_decoded_texels_equal_the_restatement(rpt, torch_cuda):
    """1 x 1, 2 x 2, 3 x 5 and 257 x 1 (a byte ramp in every channel, at another place in each: all 256 values pass the device's
    divide), under five channel choices; a mesh not named keeps its texels; the download's answers."""
    from rust_pathtracer_amd import scenes
    s, uvs = scenes.mesh_texture_scene()
    ramp = np.zeros((1, 257, 4), np.uint8)
    k = np.arange(257) % 256
    ramp[0, :, 0], ramp[0, :, 1], ramp[0, :, 2], ramp[0, :, 3] = k, 255 - k, np.roll(k, 77), (7 * k) % 256
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        t.set_mesh_textures({m: _tex(uvs[m], _white()) for m in (0, 1)})
        other = random_texels(2, 2, 12)
        for img in (np.array([[[0, 255, 128, 3]]], np.uint8), random_texels(2, 2, 10), random_texels(3, 5, 11), ramp):
            h, w = img.shape[:2]
            for rc, mc in ((1, 2), (0, 3), (3, None), (None, 0), (2, 2)):
                t.set_mesh_material_maps({0: _mmap(img, NEAREST, rc, mc), 1: _mmap(other, BILINEAR, 0, None)})
                got, want = t.mesh_material_map(0), restate_decode(img, rc, mc)
                assert got.shape == want.shape == (h, w, 4)
                assert np.array_equal(_bits(got), _bits(want)), "%dx%d channels %s, %s: %d words differ" % (w, h, rc, mc, int((_bits(got) != _bits(want)).sum()))
                assert np.array_equal(_bits(t.mesh_material_map(1)), _bits(restate_decode(other, 0, None))), "the second map of the call"
        assert set(np.unique(t.mesh_material_map(0)[..., 0])) == set(restate_value(np.arange(256)).tolist())
        # a mesh not named keeps its texels, bit for bit, though the table is made anew
        t.set_mesh_material_maps({1: _mmap(random_texels(4, 4, 14), NEAREST)})
        assert np.array_equal(_bits(t.mesh_material_map(0)), _bits(restate_decode(ramp, 2, 2)))
        assert np.array_equal(_bits(t.mesh_material_map(1)), _bits(restate_decode(random_texels(4, 4, 14), 1, 2)))
        out = np.zeros((2, 2, 4), F)
        t.set_mesh_material_maps({1: None})
        lib, bad = rpt.lib(), rpt._abi.RPT_ERR_INVALID_ARG
        assert lib.rpt_download_mesh_material_map(t._h, 1, out.ctypes.data, 2, 2) == bad and b"mesh 1 has no material map" in lib.rpt_last_error(t._h)
        assert lib.rpt_download_mesh_material_map(t._h, 0, out.ctypes.data, 2, 2) == bad and b"not its map's 257 x 1" in lib.rpt_last_error(t._h)
        assert lib.rpt_download_mesh_material_map(t._h, 0, None, 257, 1) == bad
        assert lib.rpt_download_mesh_material_map(t._h, 2, out.ctypes.data, 2, 2) == bad
    finally:
        t.close()


# ---- 2. roughness and metallic at a hit ---------------------------------------------------------------------------------------------
def _material_map_query(rpt, torch, tracer, rays, flags):
    n = len(rays)
    dev = torch.from_numpy(np.ascontiguousarray(rays, dtype=F)).cuda()
    out = torch.full((n, 4), 0x55, dtype=torch.int32, device="cuda")
    rpt._lib.check(rpt.lib().rpt_debug_mesh_material_map_query(tracer._h, dev.data_ptr(), n, out.data_ptr(), flags, None), tracer._h)
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    assert (o[:, 3] == 0).all()
    return o[:, 0].astype(np.int64) - (o[:, 0] == 0xFFFFFFFF) * (1 << 32), o[:, 1:3].copy().view(F)


def _restate_probe(scene, uvs, wraps, maps, rays):
    """-> (index or -1, {roughness, metallic} [n, 2] f32) by the texture test's ordered loop (its restatement gives the index) and
    include/rpt.h's lookup and apply.  `maps`: mesh -> (decoded texels [h, w, 4] f32, filter) or absent."""
    tris = _mesh_tris(scene)
    index, _ = _restate_query(scene, {}, rays)
    corner, mesh_of, uv, first = [], [], [], 0
    for m, (v, t, _) in enumerate(scene.meshes):
        corner.append(np.asarray(t, np.int64).reshape(-1, 3) + first)
        mesh_of.append(np.full(len(corner[-1]), m))
        uv.append(np.asarray(uvs[m], F))
        first += len(v)
    corner, mesh_of, uv = np.concatenate(corner), np.concatenate(mesh_of), np.concatenate(uv)
    want = np.zeros((len(rays), 2), F)
    for m, (_, _, mat) in enumerate(scene.meshes):
        sel = np.nonzero((index >= 0) & (mesh_of[np.maximum(index, 0)] == m))[0]
        fields = scene.materials[mat].fields
        want[sel] = (F(fields["roughness"]), F(fields["metallic"]))
        if m not in maps or not len(sel):
            continue
        k = index[sel]
        s, t = restate_hit_st(rays[sel, 0:3], rays[sel, 3:6], tris[k, 0], tris[k, 1] - tris[k, 0], tris[k, 2] - tris[k, 0],
                              uv[corner[k, 0]], uv[corner[k, 1]], uv[corner[k, 2]])
        texels, filt = maps[m]
        want[sel, 0], want[sel, 1] = restate_apply(fields["roughness"], fields["metallic"], texels, wraps[m], filt, s, t)
    return index, want


def test_probed_materials_equal_the_numpy_restatement(rpt, torch_cuda):
    """4096 rays, through the walk and the ordered loop, for the four wrap x filter pairs over a 3 x 5 map on mesh 0 and a 16 x 16
    one on mesh 1 (the opposite pair); mesh 2 is textured and unmapped, and a twelfth of the rays point away from everything."""
    from rust_pathtracer_amd import scenes
    s, uvs = _probe_scene()
    s.materials[0] = scenes.full_material(rgb=(0.8, 0.7, 0.6), roughness=0.9, metallic=0.65)
    s.materials[1] = scenes.full_material(rgb=(0.9, 0.9, 0.9), roughness=0.7, metallic=1.0)
    rng = np.random.default_rng(8200)
    rays = _query_rays(s, uvs, 3, 4096, rng)
    rays[::12, 3:6] = (rng.normal(size=(len(rays[::12]), 3)) * 0.2 + (0.0, 1.0, 0.3)).astype(F)      # upward: nothing is there
    imgs = {0: random_texels(3, 5, 71), 1: random_texels(16, 16, 72)}
    t = rpt.Tracer(s, device=0, seed=2)
    try:
        for wrap0, filt0 in ((REPEAT, BILINEAR), (CLAMP, BILINEAR), (REPEAT, NEAREST), (CLAMP, NEAREST)):
            wraps, filts = {0: wrap0, 1: 1 - wrap0, 2: wrap0}, {0: filt0, 1: 1 - filt0}
            t.set_mesh_textures({m: _tex(uvs[m], _white(), wraps[m], NEAREST) for m in (0, 1, 2)})      # (the colour filter is not the map's)
            t.set_mesh_material_maps({0: _mmap(imgs[0], filts[0], 1, 2), 1: _mmap(imgs[1], filts[1], 3, 0)})
            maps = {0: (restate_decode(imgs[0], 1, 2), filts[0]), 1: (restate_decode(imgs[1], 3, 0), filts[1])}
            index, want = _restate_probe(s, uvs, wraps, maps, rays)
            tex_index, _ = _texture_query(rpt, torch_cuda, t, rays, 0)
            for brute in (False, True):
                got_i, got = _material_map_query(rpt, torch_cuda, t, rays, rpt._abi.RPT_MESH_QUERY_BRUTE if brute else 0)
                assert np.array_equal(got_i, tex_index) and np.array_equal(got_i, index), "index (brute %s): %d rays differ" % (brute, int((got_i != index).sum()))
                bad = np.nonzero((_bits(got) != _bits(want)).any(axis=1))[0]
                assert len(bad) == 0, "wrap %s filter %s (brute %s): %d rays differ, first %s: got %s want %s" % (
                    wraps, filts, brute, len(bad), bad[:3], got[bad[:3]], want[bad[:3]])
            hit = index >= 0
            assert (index[hit] < 80).mean() > 0.1 and ((index >= 80) & (index < 82)).mean() > 0.2 and (index == 82).sum() >= 3, "all three meshes are hit"
            assert (~hit).sum() >= 100 and not want[~hit].any(), "misses answer zeros"
            assert (_bits(want[index == 82]) == _bits(np.array([0.7, 1.0], F))).all(), "the unmapped mesh keeps its material"
            assert len(np.unique(want[hit & (index < 80), 0])) > 10 and len(np.unique(want[(index >= 80) & (index < 82), 1])) > 10, "the maps vary"
        # one mesh only, the other untouched
        t.set_mesh_material_maps({0: None})
        index, want = _restate_probe(s, uvs, wraps, {1: maps[1]}, rays)
        got_i, got = _material_map_query(rpt, torch_cuda, t, rays, 0)
        assert np.array_equal(got_i, index) and np.array_equal(_bits(got), _bits(want))
        # the hook needs a map
        t.set_mesh_material_maps({1: None})
        r1 = torch_cuda.zeros(7, device="cuda")
        o1 = torch_cuda.zeros(4, dtype=torch_cuda.int32, device="cuda")
        assert rpt.lib().rpt_debug_mesh_material_map_query(t._h, r1.data_ptr(), 1, o1.data_ptr(), 0, None) == rpt._abi.RPT_ERR_INVALID_ARG
        assert b"no mesh has a material map" in rpt.lib().rpt_last_error(t._h)
    finally:
        t.close()


# ---- 3. identity: an all-255 map is no map, in each of the eight forms ------------------------------------------------------------------
def _case_tracer(rpt, case, seed, scene=None):
    """A context in the composed file's case (A .. H: the eight textured forms), over mesh_mmap_f64.scene() -> (tracer, its base form)."""
    s = scene if scene is not None else MM.scene()
    t = rpt.Tracer(s, device=0, seed=seed)
    set_composed(t, inputs(s, case))
    return t, MESH_RENDER_KERNELS.index(CASES[case][4])


@pytest.mark.parametrize("case", sorted(CASES))
def test_an_all_255_map_is_the_frame_without_a_map(rpt, torch_cuda, case):
    """This test fails without the feature: rpt_debug_mesh_form says that k_mmap.hip's kernel of the form ran.  Both filters: an
    all-255 map looks up exactly 1 under BILINEAR too (tests/test_mesh_material_map_host.py)."""
    assert BILINEAR_CONSTANT_EXACT_BYTES == (0, 255)
    t, base = _case_tracer(rpt, case, 4)
    try:
        plain = _frames(rpt, t, **SMALL)
        assert mesh_form(rpt, t) == base
        assert np.isfinite(plain[0]).all() and plain[0][..., :3].mean() > 0.005
        t.set_mesh_material_maps({0: _mmap(_constant(255, 3, 5), BILINEAR), 1: _mmap(_constant(255, 1, 1), NEAREST, 3, None)})
        _assert_frames(_frames(rpt, t, **SMALL), plain, "case %s: all-255 maps" % case)
        assert mesh_form(rpt, t) == form_of(case), "the material-mapped kernel ran"
        t.set_mesh_material_maps({0: _mmap(MM.noise_map(), BILINEAR)})     # a noise map on the object is no identity
        assert not _same(_frames(rpt, t, **SMALL)[0], plain[0]), "case %s: the noise map changes the frame" % case
        assert mesh_form(rpt, t) == form_of(case)
    finally:
        t.close()


# ---- 4. a constant map is a material edit -------------------------------------------------------------------------------------------------
def _edited(rc, mc, k):
    """mesh_mmap_f64.scene() with the materials of both meshes edited as a constant map of byte k on these channels would: the
    numpy-float32 products, of the channels that are not None."""
    from rust_pathtracer_amd import scenes
    s = MM.scene()
    c = restate_value(k)
    for mat in (0, 1):
        fields = dict(s.materials[mat].fields)
        if rc is not None:
            fields["roughness"] = float(F(fields["roughness"]) * c)
        if mc is not None:
            fields["metallic"] = float(F(fields["metallic"]) * c)
        s.materials[mat] = scenes.Material(**fields)
    return s


@pytest.mark.parametrize("case", ["A", "B", "E", "H"])
def test_a_constant_map_is_a_material_edit(rpt, torch_cuda, case):
    """Forms 12, 13, 16 and 19.  NEAREST for k in {0, 1, 128, 254}; BILINEAR for k = 0 only — the host test shows that BILINEAR
    returns no other constant exactly (but 255, the identity above); one channel None against editing the other field alone."""
    assert form_of(case) in (12, 13, 16, 19)
    trials = [(NEAREST, 1, 2, k) for k in (0, 1, 128, 254)] + [(BILINEAR, 1, 2, 0), (NEAREST, 0, None, 128), (NEAREST, None, 3, 128)]
    t, _ = _case_tracer(rpt, case, 6)
    seen = []
    try:
        for filt, rc, mc, k in trials:
            t.set_mesh_material_maps({m: _mmap(_constant(k, 3 + m, 2), filt, rc, mc) for m in (0, 1)})
            got = _frames(rpt, t, **SMALL)
            assert mesh_form(rpt, t) == form_of(case)
            b, base = _case_tracer(rpt, case, 6, _edited(rc, mc, k))
            try:
                want = _frames(rpt, b, **SMALL)
                assert mesh_form(rpt, b) == base
            finally:
                b.close()
            _assert_frames(got, want, "case %s, %s, channels %s / %s, byte %d" % (case, FILTERS[filt], rc, mc, k))
            seen.append(got[0])
        assert not _same(seen[0], seen[2]) and not _same(seen[2], seen[5]) and not _same(seen[5], seen[6]), "the edits are different edits"
    finally:
        t.close()


# ---- 5. moves ---------------------------------------------------------------------------------------------------------------------
def _move_maps():
    return {0: _mmap(MM.noise_map(12, 6, 41), BILINEAR), 1: _mmap(MM.noise_map(9, 9, 42), NEAREST, 0, 3)}


def _fresh(rpt, arrays):
    """The yardstick: a fresh context that uploads the scene with these positions and then makes the same set calls."""
    b = rpt.Tracer(_with_vertices(_small_scene, arrays), device=0, seed=8)
    try:
        b.set_mesh_textures(_move_textures(_small_scene()))
        b.set_mesh_shading({1: "smooth"})
        b.set_mesh_material_maps(_move_maps())
        return _frames(rpt, b, **SMALL)
    finally:
        b.close()


@pytest.mark.parametrize("form", ["update", "rebuild", "update_device", "rebuild_device"])
def test_material_mapped_frames_follow_every_kind_of_move(rpt, torch_cuda, form):
    from rust_pathtracer_amd import scenes
    s = _small_scene()
    rest = [np.array(v, F, copy=True) for v, _, _ in s.meshes]
    t = rpt.Tracer(s, device=0, seed=8)
    try:
        t.set_mesh_textures(_move_textures(s))
        t.set_mesh_shading({1: "smooth"})
        unmapped = _frames(rpt, t, **SMALL)
        t.set_mesh_material_maps(_move_maps())
        still = _frames(rpt, t, **SMALL)
        _assert_frames(still, _fresh(rpt, rest), "before any move")
        assert not _same(still[0], unmapped[0])
        held_maps = [t.mesh_material_map(m).copy() for m in (0, 1)]
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
        assert mesh_form(rpt, t) == 12                                # no mesh ON: the form over the textured mesh-light tables, empty
        _assert_frames(got, _fresh(rpt, held), "%s: against a fresh upload" % form)
        assert not _same(got[0], still[0])
        assert all(np.array_equal(_bits(t.mesh_material_map(m)), _bits(held_maps[m])) for m in (0, 1)), "a move leaves the maps alone"
    finally:
        t.close()


# ---- 6. lifetime ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A", "H"])
def test_the_form_and_the_way_back(rpt, torch_cuda, case):
    t, base = _case_tracer(rpt, case, 9)
    args = inputs(MM.scene(), case)
    try:
        never = _frames(rpt, t, **SMALL)
        assert mesh_form(rpt, t) == base
        maps = MM.material_maps()
        t.set_mesh_material_maps(maps)
        both = _frames(rpt, t, **SMALL)
        assert mesh_form(rpt, t) == form_of(case) and not _same(both[0], never[0])
        t.set_mesh_material_maps({1: None})
        one = _frames(rpt, t, **SMALL)
        assert mesh_form(rpt, t) == form_of(case) and not _same(one[0], never[0]) and not _same(one[0], both[0])
        # replacing the texture keeps the map: the same texture again gives the same frames, another one another frame with the map in it
        t.set_mesh_textures({0: args["textures"][0]})
        _assert_frames(_frames(rpt, t, **SMALL), one, "the same texture again")
        t.set_mesh_textures({0: dict(args["textures"][0], texels=random_texels(4, 4, 55))})
        assert np.array_equal(_bits(t.mesh_material_map(0)), _bits(restate_decode(maps[0]["texels"], 1, 2)))
        assert mesh_form(rpt, t) == form_of(case) and not _same(_frames(rpt, t, **SMALL)[0], one[0])
        t.set_mesh_textures({0: args["textures"][0]})
        # removing the texture of a mapped mesh is refused and changes nothing
        with pytest.raises(Exception) as e:
            t.set_mesh_textures({0: None})
        first = "material map" if case == "A" else "cutout"           # (case H: the cutout's rule comes first in rpt_set_mesh_textures)
        assert "remove the %s first" % first in str(e.value) and rpt.lib().rpt_last_error(t._h).decode().startswith("rpt_set_mesh_textures: ")
        if case == "H":                                              # with the cutout and the normal map gone, the material map's rule answers
            t.set_mesh_cutouts({0: None})
            t.set_mesh_normal_maps({0: None})
            with pytest.raises(Exception) as e:
                t.set_mesh_textures({0: None})
            assert "remove the material map first" in str(e.value)
            t.set_mesh_cutouts(args["cutouts"])
            t.set_mesh_normal_maps({0: args["normal_maps"][0]})
        _assert_frames(_frames(rpt, t, **SMALL), one, "after the refused removal")
        # every map OFF: the previous form and frames
        t.set_mesh_material_maps({0: None})
        _assert_frames(_frames(rpt, t, **SMALL), never, "the last map OFF")
        assert mesh_form(rpt, t) == base, "the form is what it was"
        t.set_mesh_material_maps({0: None, 1: None})                 # removing what is not there is no error
        t.set_mesh_material_maps(maps)
        _assert_frames(_frames(rpt, t, **SMALL), both, "the same maps again")
        t.upload_scene()                                             # an upload drops maps (and everything else that was set)
        _frames(rpt, t, **SMALL)
        assert mesh_form(rpt, t) == MESH_RENDER_KERNELS.index("mesh_regen_kernel")
        out = np.zeros((3, 5, 4), F)
        assert rpt.lib().rpt_download_mesh_material_map(t._h, 1, out.ctypes.data, 5, 3) == rpt._abi.RPT_ERR_INVALID_ARG
        assert rpt.lib().rpt_set_mesh_material_maps(t._h, None, 0) == rpt._abi.RPT_OK
    finally:
        t.close()


def test_a_device_listed_twice_renders_the_one_context_frame(rpt, torch_cuda):
    w, h, spp = 32, 24, 4
    frames = []
    for devices in (dict(device=0), dict(devices=[0, 0])):
        s = MM.scene()
        t = rpt.Tracer(s, seed=11, **devices)
        try:
            set_composed(t, inputs(s, "F"))
            t.set_mesh_material_maps(MM.material_maps())
            t.render_resident(w, h, spp)
            assert mesh_form(rpt, t) == form_of("F") == 17
            frames.append(t.resident_to_host(w, h).pixels.reshape(h, w, 4).copy())
            if "devices" in devices:
                t.set_mesh_material_maps({0: None, 1: None})
                t.resident_reset()
                t.render_resident(w, h, spp)
                assert mesh_form(rpt, t) == MESH_RENDER_KERNELS.index("meshnrm_env_regen_kernel")
        finally:
            t.close()
    assert _same(frames[0], frames[1]) and np.isfinite(frames[0]).all()


# ---- 7. answers -------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_say_why_and_change_nothing(rpt, torch_cuda):
    A, lib = rpt._abi, rpt.lib()
    from rust_pathtracer_amd import scenes
    s, uvs = scenes.mesh_texture_scene()
    t = rpt.Tracer(s, device=0, seed=10)
    try:
        t.set_mesh_textures({0: _tex(uvs[0], random_texels(3, 5, 61), CLAMP, BILINEAR, 2.2)})
        t.set_mesh_material_maps({0: _mmap(MM.noise_map(6, 6, 62), BILINEAR)})
        ref = _frames(rpt, t, **SMALL)
        held = t.mesh_material_map(0).copy()
        texels = np.ascontiguousarray(random_texels(2, 2, 63))
        bptr = texels.ctypes.data_as(C.POINTER(C.c_uint8))
        NONE = A.RPT_MATERIAL_MAP_CHANNEL_NONE

        def items(*rows):
            arr = (A.rpt_mesh_material_map * len(rows))()
            for it, r in zip(arr, rows):
                r = dict(dict(mesh=0, mode=A.RPT_MESH_MATERIAL_MAP_ON, width=2, height=2, texels=bptr, filter=A.RPT_TEX_FILTER_BILINEAR,
                              roughness_channel=1, metallic_channel=2), **r)
                for key, val in r.items():
                    setattr(it, key, val)
            return arr

        off = dict(mode=A.RPT_MESH_MATERIAL_MAP_OFF, width=0, height=0, texels=None, filter=0, roughness_channel=NONE, metallic_channel=NONE)
        # in the stated order; each case but the last carries the NEXT check's fault as well, so the order itself is held
        cases = [("NULL items", None, 1, "items is NULL"),
                 ("mesh out of range", items(dict(mesh=2, mode=7)), 1, "mesh 2 out of range"),
                 ("named twice", items(dict(), dict(mode=7)), 2, "item 1: mesh 0 is named twice"),
                 ("mode", items(dict(mode=2, width=0)), 1, "mode 2"),
                 ("width 0", items(dict(width=0, texels=None)), 1, "a map of 0 x 2"),
                 ("NULL texels", items(dict(texels=None, filter=2)), 1, "texels is NULL"),
                 ("filter", items(dict(filter=2, roughness_channel=4)), 1, "filter 2"),
                 ("channel", items(dict(mesh=1, roughness_channel=4, metallic_channel=NONE)), 1, "channels 4 and"),
                 ("both NONE", items(dict(mesh=1, roughness_channel=NONE, metallic_channel=NONE)), 1, "both channels are RPT_MATERIAL_MAP_CHANNEL_NONE"),
                 ("OFF with a size", items(dict(off, width=2)), 1, "RPT_MESH_MATERIAL_MAP_OFF takes"),
                 ("untextured", items(dict(mesh=1, width=16384, height=16384)), 1, "mesh 1 is untextured")]
        for what, arr, n, says in cases:
            assert lib.rpt_set_mesh_material_maps(t._h, arr, n) == A.RPT_ERR_INVALID_ARG, what
            err = lib.rpt_last_error(t._h).decode()
            assert err.startswith("rpt_set_mesh_material_maps: ") and says in err, (what, err)
        assert "item 0" in lib.rpt_last_error(t._h).decode()
        big = items(dict(width=8192, height=8193))                  # refused on the host from the sizes alone (texels is never read)
        assert lib.rpt_set_mesh_material_maps(t._h, big, 1) == A.RPT_ERR_UNSUPPORTED and "2^26" in lib.rpt_last_error(t._h).decode()
        assert np.array_equal(_bits(t.mesh_material_map(0)), _bits(held))
        _assert_frames(_frames(rpt, t, **SMALL), ref, "after every rejected call")
        assert mesh_form(rpt, t) == 12
        assert lib.rpt_set_mesh_material_maps(t._h, None, 0) == A.RPT_OK
        _assert_frames(_frames(rpt, t, **SMALL), ref, "n_items == 0 does nothing")
        # no scene with meshes
        b = rpt.Tracer(scenes.six_primitive_scene(), device=0, seed=1)
        try:
            assert lib.rpt_set_mesh_material_maps(b._h, items(dict()), 1) == A.RPT_ERR_NO_SCENE
            assert lib.rpt_set_mesh_material_maps(b._h, None, 1) == A.RPT_ERR_NO_SCENE         # no scene comes before NULL items
            out = np.zeros(4, F)
            assert lib.rpt_download_mesh_material_map(b._h, 0, out.ctypes.data, 1, 1) == A.RPT_ERR_NO_SCENE
        finally:
            b.close()
    finally:
        t.close()
