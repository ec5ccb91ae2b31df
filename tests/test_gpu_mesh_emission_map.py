"""Mesh emission maps on the device (include/rpt.h, "mesh emission maps"), bit for bit: decoded texels equal numpy float32 with the
oracle's pow; the probed emission of a hit — the hit side's and the emitter exit's — equals the numpy restatement through the walk
and the ordered loop, under both wraps; the probed sampler leaves k, direction and pdf what the unmapped sampler gives and hands out
the restated emission on meshes of 1, 2 and 300 triangles; an all-255 map is the frame without a map in each of the eight forms —
with rpt_debug_mesh_form saying 20 .. 27, so the new kernels ran; a constant NEAREST map is the frame of a fresh upload whose
material emission holds the float32 products, lamp ON and OFF, with an rpt_light in front of the panel; a mesh without emission
renders as without the map; every kind of move gives the frames of a fresh upload; material maps compose; the texture guard; every
rejected call says why and changes nothing; and the lamp ON and OFF estimate the same integral.  Maps are 1 x 1, 5 x 3 NEAREST and
16 x 16 BILINEAR; frames 64 x 48 x 1 spp; probes take 4096 rays or draws."""
import ctypes as C

import numpy as np
import pytest

import mesh_mmap_f64 as MM
from kernel_census import MESH_RENDER_KERNELS
from test_gpu_mesh import _mesh_tris
from test_gpu_mesh_compose_f64 import CASES, inputs
from test_gpu_mesh_light import _lit_small_scene, _sample
from test_gpu_mesh_material_map_f64 import form_of as map_form_of
from test_gpu_mesh_material_map_f64 import mesh_form, set_composed
from test_gpu_mesh_normal_map import MATRIX, _probe_scene
from test_gpu_mesh_texture import _move_textures, _query_rays, _restate_query, _tex, _white
from test_gpu_mesh_update import _assert_frames, _frames, _same, _with_vertices
from test_mesh_emission_map_host import restate_apply, restate_sample_emission, restate_sample_uv, restate_st
from test_mesh_light_host import strip
from test_mesh_texture_host import BILINEAR, CLAMP, NEAREST, REPEAT, random_texels, restate_decode, restate_hit_st

pytestmark = pytest.mark.gpu
F = np.float32
ONE = dict(sizes=((64, 48, 1),), resident=None)
FILTERS = {NEAREST: "nearest", BILINEAR: "bilinear"}
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _emap(texels, filt=BILINEAR, gamma=1.0):
    return dict(texels=texels, filter=FILTERS[filt], gamma=gamma)


def _constant(k, w=5, h=3):
    return np.full((h, w, 4), k, np.uint8)


def form_of(case):
    """20 .. 27: the emission map over the material-mapped form over the kernel the composed file's case runs."""
    return map_form_of(case) + 8


# ---- 1. decode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", (1.0, 2.2))
def test_decoded_texels_equal_the_restatement(rpt, torch_cuda, oracle, gamma):
    """This test fails without the feature, at its first set_mesh_emission_maps.  1 x 1, 5 x 3, 16 x 16 and a 256 x 1 byte ramp; a
    mesh not named keeps its texels; the download's answers."""
    from rust_pathtracer_amd import scenes
    s, uvs = scenes.mesh_texture_scene()
    ramp = np.zeros((1, 256, 4), np.uint8)
    k = np.arange(256)
    ramp[0, :, 0], ramp[0, :, 1], ramp[0, :, 2], ramp[0, :, 3] = k, 255 - k, np.roll(k, 77), 9
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        t.set_mesh_textures({m: _tex(uvs[m], _white()) for m in (0, 1)})
        other = random_texels(2, 2, 12)
        for img in (np.array([[[0, 255, 128, 3]]], np.uint8), random_texels(5, 3, 10), random_texels(16, 16, 11), ramp):
            h, w = img.shape[:2]
            t.set_mesh_emission_maps({0: _emap(img, NEAREST, gamma), 1: _emap(other, BILINEAR, 1.0)})
            got, want = t.download_mesh_emission_map(0), restate_decode(oracle, img, gamma)
            assert got.shape == want.shape == (h, w, 4)
            assert np.array_equal(_bits(got), _bits(want)), "%dx%d at gamma %g: %d words differ" % (w, h, gamma, int((_bits(got) != _bits(want)).sum()))
            assert np.array_equal(_bits(t.download_mesh_emission_map(1)), _bits(restate_decode(oracle, other, 1.0))), "the second map of the call"
        t.set_mesh_emission_maps({1: _emap(random_texels(4, 4, 14), NEAREST, 2.2)})      # a mesh not named keeps its texels
        assert np.array_equal(_bits(t.download_mesh_emission_map(0)), _bits(restate_decode(oracle, ramp, gamma)))
        assert np.array_equal(_bits(t.download_mesh_emission_map(1)), _bits(restate_decode(oracle, random_texels(4, 4, 14), 2.2)))
        out = np.zeros((2, 2, 4), F)
        t.set_mesh_emission_maps({1: None})
        lib, bad = rpt.lib(), rpt._abi.RPT_ERR_INVALID_ARG
        assert lib.rpt_download_mesh_emission_map(t._h, 1, out.ctypes.data, 2, 2) == bad and b"mesh 1 has no emission map" in lib.rpt_last_error(t._h)
        assert lib.rpt_download_mesh_emission_map(t._h, 0, out.ctypes.data, 2, 2) == bad and b"not its map's 256 x 1" in lib.rpt_last_error(t._h)
        assert lib.rpt_download_mesh_emission_map(t._h, 0, None, 256, 1) == bad
        assert lib.rpt_download_mesh_emission_map(t._h, 2, out.ctypes.data, 2, 2) == bad
    finally:
        t.close()


# ---- 2. the emission at a hit -------------------------------------------------------------------------------------------------------
def _emission_map_query(rpt, torch, tracer, rays, flags):
    n = len(rays)
    dev = torch.from_numpy(np.ascontiguousarray(rays, dtype=F)).cuda()
    out = torch.full((n, 7), 0x55, dtype=torch.int32, device="cuda")
    rpt._lib.check(rpt.lib().rpt_debug_mesh_emission_map_query(tracer._h, dev.data_ptr(), n, out.data_ptr(), flags, None), tracer._h)
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    return o[:, 0].astype(np.int64) - (o[:, 0] == 0xFFFFFFFF) * (1 << 32), o[:, 1:4].copy().view(F), o[:, 4:7].copy().view(F)


def _restate_probe(scene, uvs, wraps, maps, rays):
    """-> (index or -1, emission [n, 3] f32) by the texture test's ordered loop (its restatement gives the index) and include/rpt.h's
    lookup and apply.  `maps`: mesh -> (decoded texels [h, w, 4] f32, filter) or absent."""
    tris = _mesh_tris(scene)
    index, _ = _restate_query(scene, {}, rays)
    corner, mesh_of, uv, first = [], [], [], 0
    for m, (v, t, _) in enumerate(scene.meshes):
        corner.append(np.asarray(t, np.int64).reshape(-1, 3) + first)
        mesh_of.append(np.full(len(corner[-1]), m))
        uv.append(np.asarray(uvs[m], F))
        first += len(v)
    corner, mesh_of, uv = np.concatenate(corner), np.concatenate(mesh_of), np.concatenate(uv)
    want = np.zeros((len(rays), 3), F)
    for m, (_, _, mat) in enumerate(scene.meshes):
        sel = np.nonzero((index >= 0) & (mesh_of[np.maximum(index, 0)] == m))[0]
        emission = np.array(scene.materials[mat].fields["emission"], F)
        want[sel] = emission
        if m not in maps or not len(sel):
            continue
        k = index[sel]
        s, t = restate_hit_st(rays[sel, 0:3], rays[sel, 3:6], tris[k, 0], tris[k, 1] - tris[k, 0], tris[k, 2] - tris[k, 0],
                              uv[corner[k, 0]], uv[corner[k, 1]], uv[corner[k, 2]])
        texels, filt = maps[m]
        want[sel] = restate_apply(emission, texels, wraps[m], filt, s, t)
    return index, want


def test_probed_emission_equals_the_numpy_restatement(rpt, torch_cuda, oracle):
    """4096 rays, through the walk and the ordered loop, REPEAT and CLAMP, over a 5 x 3 NEAREST map on mesh 0 and a 16 x 16 BILINEAR
    one on mesh 1; mesh 2 is textured, emissive and unmapped, and a twelfth of the rays point away from everything.  The hit side's
    emission and the emitter exit's are the same words."""
    from rust_pathtracer_amd import scenes
    s, uvs = _probe_scene()
    s.materials[0] = scenes.full_material(rgb=(0.8, 0.7, 0.6), roughness=0.9, emission=(3.0, 2.0, 0.7))
    s.materials[1] = scenes.full_material(rgb=(0.9, 0.9, 0.9), roughness=0.7, emission=(11.0, 0.3, 5.5))
    rng = np.random.default_rng(8300)
    rays = _query_rays(s, uvs, 5, 4096, rng)
    rays[::12, 3:6] = (rng.normal(size=(len(rays[::12]), 3)) * 0.2 + (0.0, 1.0, 0.3)).astype(F)      # upward: nothing is there
    imgs = {0: random_texels(5, 3, 81), 1: random_texels(16, 16, 82)}
    gammas = {0: 2.2, 1: 1.0}
    t = rpt.Tracer(s, device=0, seed=2)
    try:
        for wrap0 in (REPEAT, CLAMP):
            wraps, filts = {0: wrap0, 1: 1 - wrap0, 2: wrap0}, {0: NEAREST, 1: BILINEAR}
            t.set_mesh_textures({m: _tex(uvs[m], _white(), wraps[m], NEAREST) for m in (0, 1, 2)})      # (the colour filter is not the map's)
            t.set_mesh_emission_maps({m: _emap(imgs[m], filts[m], gammas[m]) for m in (0, 1)})
            maps = {m: (restate_decode(oracle, imgs[m], gammas[m]), filts[m]) for m in (0, 1)}
            index, want = _restate_probe(s, uvs, wraps, maps, rays)
            for brute in (False, True):
                got_i, got, got_exit = _emission_map_query(rpt, torch_cuda, t, rays, rpt._abi.RPT_MESH_QUERY_BRUTE if brute else 0)
                assert np.array_equal(got_i, index), "index (brute %s): %d rays differ" % (brute, int((got_i != index).sum()))
                bad = np.nonzero((_bits(got) != _bits(want)).any(axis=1))[0]
                assert len(bad) == 0, "wrap %s (brute %s): %d rays differ, first %s: got %s want %s" % (wraps, brute, len(bad), bad[:3], got[bad[:3]], want[bad[:3]])
                assert np.array_equal(_bits(got_exit), _bits(want)), "the emitter exit's emission"
            hit = index >= 0
            assert (index[hit] < 80).mean() > 0.1 and ((index >= 80) & (index < 82)).mean() > 0.2 and (index == 82).sum() >= 3, "all three meshes are hit"
            assert (~hit).sum() >= 100 and not want[~hit].any(), "misses answer zeros"
            assert (_bits(want[index == 82]) == _bits(np.array([11.0, 0.3, 5.5], F))).all(), "the unmapped mesh keeps its emission"
            assert len(np.unique(want[hit & (index < 80), 0])) > 5 and len(np.unique(want[(index >= 80) & (index < 82), 1])) > 10, "the maps vary"
        t.set_mesh_emission_maps({0: None})                            # one mesh only, the other untouched
        index, want = _restate_probe(s, uvs, wraps, {1: maps[1]}, rays)
        got_i, got, got_exit = _emission_map_query(rpt, torch_cuda, t, rays, 0)
        assert np.array_equal(got_i, index) and np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(got_exit), _bits(want))
        t.set_mesh_emission_maps({1: None})                            # the hooks need a map
        r1 = torch_cuda.zeros(8, device="cuda")
        o1 = torch_cuda.zeros(8, dtype=torch_cuda.int32, device="cuda")
        assert rpt.lib().rpt_debug_mesh_emission_map_query(t._h, r1.data_ptr(), 1, o1.data_ptr(), 0, None) == rpt._abi.RPT_ERR_INVALID_ARG
        assert b"no mesh has an emission map" in rpt.lib().rpt_last_error(t._h)
        assert rpt.lib().rpt_debug_mesh_emission_map_sample(t._h, r1.data_ptr(), 1, o1.data_ptr(), None) == rpt._abi.RPT_ERR_INVALID_ARG
    finally:
        t.close()


# ---- 3. the sampler -----------------------------------------------------------------------------------------------------------------
def _emission_sample(rpt, torch, t, rec):
    n = len(rec)
    dev = torch.from_numpy(np.ascontiguousarray(rec, F)).cuda()
    out = torch.full((n, 8), 0x55, dtype=torch.int32, device="cuda")
    rpt._lib.check(rpt.lib().rpt_debug_mesh_emission_map_sample(t._h, dev.data_ptr(), n, out.data_ptr(), None), t._h)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def test_the_sampler_keeps_its_pick_and_pdf_and_hands_out_the_mapped_emission(rpt, torch_cuda, oracle):
    """4096 draws over ON meshes of 1, 2 and 300 triangles with maps (1 x 1, 5 x 3 NEAREST, 16 x 16 BILINEAR) and one ON mesh
    without: k, direction and pdf are the words rpt_debug_mesh_light_sample gives on the same context; the emission is
    N_f * (m.emission * E(bu, bv)) restated in numpy, N_f * m.emission on the unmapped mesh."""
    from rust_pathtracer_amd import scenes
    rng = np.random.default_rng(8400)
    s = scenes.mesh_light_scene()
    emission = np.array(s.materials[1].fields["emission"], F)
    one = (np.array([[-1.2, 0.9, 0.1], [-0.8, 1.0, 0.2], [-1.0, 1.3, -0.1]], F), np.array([[0, 1, 2]], np.uint32))
    strip_v, strip_t = strip(300, 400)
    extra = [one, (np.ascontiguousarray(strip_v, F), np.ascontiguousarray(strip_t, np.uint32)),
             (np.array([[0.9, 1.0, 0.0], [1.3, 1.0, 0.1], [1.1, 1.4, 0.0]], F), np.array([[0, 1, 2]], np.uint32))]
    for v, t_ in extra:
        s.meshes.append((v, t_, 1))
    on = (1, 2, 3, 4)                                                 # the lamp (2 triangles), one triangle, the strip, one triangle unmapped
    uvs = {m: rng.uniform(-1.5, 2.5, (len(s.meshes[m][0]), 2)).astype(F) for m in on}
    wraps = {1: REPEAT, 2: CLAMP, 3: CLAMP, 4: REPEAT}
    imgs = {1: (random_texels(5, 3, 91), NEAREST, 2.2), 2: (random_texels(1, 1, 92), BILINEAR, 1.0), 3: (random_texels(16, 16, 93), BILINEAR, 1.0)}
    t = rpt.Tracer(s, device=0, seed=3)
    try:
        t.set_mesh_textures({m: _tex(uvs[m], _white(), wraps[m], NEAREST) for m in on})
        t.set_mesh_lights({m: True for m in on})
        t.set_mesh_emission_maps({m: _emap(*imgs[m]) for m in imgs})
        n_f = F(len(s.lights) + len(on))
        total = 0
        for ordinal, m in enumerate(on):
            v, idx, _ = s.meshes[m]
            v, idx = np.asarray(v, F).reshape(-1, 3), np.asarray(idx, np.int64).reshape(-1, 3)
            n = 1024
            scatter = rng.uniform(v.min(0).astype(np.float64) - 1.5, v.max(0).astype(np.float64) + 1.5, (n, 3)).astype(F)
            draws = (rng.integers(0, 1 << 24, (n, 4)).astype(F) / F(16777216.0)).astype(F)
            draws[0, :2], draws[1, :2] = 0.0, F((1 << 24) - 1) / F(16777216.0)
            draws[2:8, 2] = 0.0                                       # r1 = 0: the point is corner b
            draws[8:12, 3] = 0.0                                      # r2 = 0: the point lies on edge a - b
            rec = np.concatenate([scatter, draws, np.full((n, 1), ordinal, np.uint32).view(F)], 1)
            base = _sample(rpt, torch_cuda, t, rec)                   # {k, direction, normal, dist, pdf}: the unmapped sampler's probe
            got = _emission_sample(rpt, torch_cuda, t, rec)           # {k, emission, direction, pdf}
            assert np.array_equal(got[:, 0], base[:, 0]) and (got[:, 0] != NONE).all(), "mesh %d: k" % m
            assert np.array_equal(got[:, 4:7], base[:, 1:4]), "mesh %d: direction" % m
            assert np.array_equal(got[:, 7], base[:, 8]), "mesh %d: pdf" % m
            k = got[:, 0].astype(np.int64)
            assert k.max() < len(idx) and len(np.unique(k)) >= min(len(idx), 100)
            if m in imgs:
                img, filt, gamma = imgs[m]
                bu, bv = restate_sample_uv(draws[:, 2], draws[:, 3])
                st = restate_st(bu, bv, uvs[m][idx[k, 0]], uvs[m][idx[k, 1]], uvs[m][idx[k, 2]])
                want = restate_sample_emission(emission, n_f, restate_decode(oracle, img, gamma), wraps[m], filt, *st)
                if m != 2:
                    assert len(np.unique(want[:, 0])) > 5, "the map varies"
            else:
                want = np.broadcast_to(n_f * emission, (n, 3))
            bad = np.nonzero((got[:, 1:4] != _bits(want)).any(axis=1))[0]
            assert len(bad) == 0, "mesh %d: %d emissions differ, first %s: got %s want %s" % (m, len(bad), bad[:3], got[bad[:3], 1:4].view(F), want[bad[:3]])
            total += n
        assert total == 4096
        rec = np.zeros((2, 8), F)                                     # an ordinal past the ON meshes: zeros
        rec[:, 7] = np.array([4, NONE], np.uint32).view(F)
        got = _emission_sample(rpt, torch_cuda, t, rec)
        assert (got[:, 0] == NONE).all() and not got[:, 1:].any()
        # the light ordinals change under the maps: with the lamp OFF, mesh 2 is ordinal 0 and takes its own 1 x 1 map
        t.set_mesh_lights({1: False})
        rec = np.concatenate([np.zeros((4, 3), F), np.full((4, 4), 0.25, F), np.zeros((4, 1), F)], 1)
        got = _emission_sample(rpt, torch_cuda, t, rec)
        E = restate_decode(oracle, imgs[2][0], 1.0)[0, 0, :3]
        assert np.array_equal(got[:, 1:4], np.broadcast_to(_bits(F(len(on) - 1) * (emission * E)), (4, 3)))
    finally:
        t.close()


# ---- 4. identity: an all-255 map is no map, in each of the eight forms ---------------------------------------------------------------
def _case_tracer(rpt, case, seed, scene=None):
    """A context in the composed file's case (A .. H: the eight textured forms), over mesh_mmap_f64.scene() -> (tracer, its base form)."""
    s = scene if scene is not None else MM.scene()
    t = rpt.Tracer(s, device=0, seed=seed)
    set_composed(t, inputs(s, case))
    return t, MESH_RENDER_KERNELS.index(CASES[case][4])


@pytest.mark.parametrize("case", sorted(CASES))
def test_an_all_255_map_is_the_frame_without_a_map(rpt, torch_cuda, case):
    """rpt_debug_mesh_form says that k_emap.hip's kernel of the form ran.  Any gamma, both filters: an all-255 map looks up exactly 1."""
    t, base = _case_tracer(rpt, case, 4)
    try:
        plain = _frames(rpt, t, **ONE)
        assert mesh_form(rpt, t) == base
        assert np.isfinite(plain[0]).all() and plain[0][..., :3].mean() > 0.005
        t.set_mesh_emission_maps({0: _emap(_constant(255, 1, 1), NEAREST, 0.7), 1: _emap(_constant(255, 16, 16), BILINEAR, 2.2)})
        _assert_frames(_frames(rpt, t, **ONE), plain, "case %s: all-255 maps" % case)
        assert mesh_form(rpt, t) == form_of(case), "the emission-mapped kernel ran"
        t.set_mesh_emission_maps({1: _emap(MM.noise_map(16, 16, 5), BILINEAR)})      # a noise map on the lamp is no identity
        assert not _same(_frames(rpt, t, **ONE)[0], plain[0]), "case %s: the noise map changes the frame" % case
        assert mesh_form(rpt, t) == form_of(case)
        t.set_mesh_emission_maps({0: None, 1: None})                  # every map OFF: the form and the frames of before
        _assert_frames(_frames(rpt, t, **ONE), plain, "case %s: every map OFF" % case)
        assert mesh_form(rpt, t) == base
    finally:
        t.close()


def test_the_forms_of_the_cases_are_20_to_27():
    assert [form_of(c) for c in sorted(CASES)] == list(range(20, 28))


# ---- 5. a constant map is an emission edit; the emitter exit -----------------------------------------------------------------------
PANEL = (np.array([[-1.2, -0.5, -1.4], [1.4, -0.5, -1.3], [1.4, 1.3, -1.35], [-1.2, 1.3, -1.45]], F), np.array([[0, 1, 2], [0, 2, 3]], np.uint32))
PANEL_EMISSION = (1.5, 0.9, 2.25)
LIGHT_AT = (0.4, 0.6, 1.2)


def _panel_scene(lamp_emission=(40.0, 36.0, 30.0), panel_emission=PANEL_EMISSION):
    """scenes.mesh_light_scene() with, as mesh 2, an emissive panel behind the object and a spherical rpt_light between the camera
    and the panel: the rays of some hundred pixels pass through the light and end on the panel — the emitter exit."""
    from rust_pathtracer_amd import scenes
    s = scenes.mesh_light_scene(lamp_emission=lamp_emission)
    s.max_depth = 4
    s.lights = [scenes.AnalyticalLight.spherical(LIGHT_AT, 0.3, (3.0, 3.0, 3.0))]
    s.materials.append(scenes.full_material(rgb=(0.5, 0.5, 0.5), roughness=1.0, emission=tuple(panel_emission)))
    s.meshes.append((PANEL[0].copy(), PANEL[1].copy(), 3))
    return s


def _panel_textures(s):
    from rust_pathtracer_amd import scenes
    uv = [scenes.spherical_uvs(v, 0.5 * (np.asarray(v).min(0) + np.asarray(v).max(0))) for v, _, _ in s.meshes]
    return {1: _tex(uv[1] * F(2), _white(), REPEAT, NEAREST), 2: _tex(uv[2], random_texels(4, 4, 33), CLAMP, BILINEAR, 2.2)}


def _through_the_light(w=64, h=48):
    """The pixels [(col, row)] whose centre's ray meets the spherical light (scenes.mesh_light_scene()'s camera: at (0, 0.5, 3.2),
    looking at the origin, 60 degrees upright); behind it lies the panel."""
    import math
    o = np.array((0.0, 0.5, 3.2))
    c, r = np.array(LIGHT_AT), 0.3
    fwd = -o / np.linalg.norm(o)
    right = np.cross(fwd, (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    tan = math.tan(math.radians(60.0) / 2)
    out = []
    for j in range(h):
        for i in range(w):
            d = fwd + right * ((i + 0.5) / w * 2 - 1) * tan * w / h + up * (1 - (j + 0.5) / h * 2) * tan
            d /= np.linalg.norm(d)
            oc = o - c
            b = oc @ d
            if (b * b - (oc @ oc - r * r)) > 0 and -b > 0:
                out.append((i, j))
    return out


@pytest.mark.parametrize("lamp_on", (True, False))
def test_a_constant_map_is_an_emission_edit(rpt, torch_cuda, oracle, lamp_on):
    """A constant-byte NEAREST map on the lamp and on the panel gives the frames of a fresh upload whose material emission holds the
    float32 products m.emission[c] * L[k] — at the hits, in the sampler (lamp ON) and at the emitter exit, where the rays through the
    spherical light end on the mapped panel.  k in {0, 1, 128, 254} at gamma 1 and 2.2; BILINEAR for k = 0 (exact, as 255 is)."""
    trials = [(NEAREST, 1.0, k) for k in (0, 1, 128, 254)] + [(NEAREST, 2.2, 128), (BILINEAR, 1.0, 0)]
    s = _panel_scene()
    assert len(_through_the_light()) > 50, "the emitter exit is exercised"
    t = rpt.Tracer(s, device=0, seed=6)
    seen = []
    try:
        t.set_mesh_textures(_panel_textures(s))
        if lamp_on:
            t.set_mesh_lights({1: True, 2: True})
        plain = _frames(rpt, t, **ONE)
        assert mesh_form(rpt, t) == MESH_RENDER_KERNELS.index("meshtex_light_regen_kernel" if lamp_on else "meshtex_regen_kernel")
        for filt, gamma, k in trials:
            t.set_mesh_emission_maps({1: _emap(_constant(k, 5, 3), filt, gamma), 2: _emap(_constant(k, 1, 1), filt, gamma)})
            got = _frames(rpt, t, **ONE)
            assert mesh_form(rpt, t) == 20
            c = restate_decode(oracle, _constant(k, 1, 1), gamma)[0, 0, 0]
            edited = _panel_scene(tuple(float(x) for x in np.array((40.0, 36.0, 30.0), F) * c), tuple(float(x) for x in np.array(PANEL_EMISSION, F) * c))
            b = rpt.Tracer(edited, device=0, seed=6)
            try:
                b.set_mesh_textures(_panel_textures(edited))
                if lamp_on:
                    b.set_mesh_lights({1: True, 2: True})
                want = _frames(rpt, b, **ONE)
                assert mesh_form(rpt, b) < 12
            finally:
                b.close()
            _assert_frames(got, want, "lamp %s, %s, gamma %g, byte %d" % ("ON" if lamp_on else "OFF", FILTERS[filt], gamma, k))
            seen.append(got[0])
        assert not _same(seen[0], seen[2]) and not _same(seen[2], seen[3]) and not _same(seen[2], seen[4]), "the edits are different edits"
        assert not _same(seen[2], plain[0])
    finally:
        t.close()


def test_a_mesh_without_emission_renders_as_without_the_map(rpt, torch_cuda):
    """The object of the composed scene emits nothing: 0 * E is 0 whatever the map holds (case A, lamp ON)."""
    t, base = _case_tracer(rpt, "A", 7)
    try:
        plain = _frames(rpt, t, **ONE)
        t.set_mesh_emission_maps({0: _emap(MM.noise_map(16, 16, 6), BILINEAR, 2.2)})
        _assert_frames(_frames(rpt, t, **ONE), plain, "a map on a mesh that emits nothing")
        assert mesh_form(rpt, t) == 20
    finally:
        t.close()


# ---- 6. moves ---------------------------------------------------------------------------------------------------------------------
def _move_maps():
    return {0: _emap(MM.noise_map(5, 3, 41), NEAREST, 2.2), 1: _emap(MM.noise_map(16, 16, 42), BILINEAR)}


def _moving_scene():
    s = _lit_small_scene()
    s.materials[0].fields["emission"] = (0.2, 0.5, 0.9)
    return s


def _set_up_moving(t):
    t.set_mesh_textures(_move_textures(_moving_scene()))
    t.set_mesh_lights({1: True})
    t.set_mesh_emission_maps(_move_maps())


def _fresh(rpt, arrays):
    """The yardstick: a fresh context that uploads the scene with these positions and then makes the same set calls."""
    b = rpt.Tracer(_with_vertices(_moving_scene, arrays), device=0, seed=8)
    try:
        _set_up_moving(b)
        return _frames(rpt, b, **ONE)
    finally:
        b.close()


@pytest.mark.parametrize("form", ["update", "rebuild", "update_device", "rebuild_device"])
def test_emission_mapped_frames_follow_every_kind_of_move(rpt, torch_cuda, form):
    from rust_pathtracer_amd import scenes
    s = _moving_scene()
    rest = [np.array(v, F, copy=True) for v, _, _ in s.meshes]
    t = rpt.Tracer(s, device=0, seed=8)
    try:
        _set_up_moving(t)
        still = _frames(rpt, t, **ONE)
        _assert_frames(still, _fresh(rpt, rest), "before any move")
        held_maps = [t.download_mesh_emission_map(m).copy() for m in (0, 1)]
        moved = scenes.mesh_scene_moved(s, 0.7)
        if form == "update":
            t.update_meshes(dict(enumerate(moved)))
        elif form == "rebuild":
            t.rebuild_meshes(dict(enumerate(moved)))
        else:                                                         # the device forms: mesh 0 as it is, mesh 1 through a 3x4 matrix
            src = {0: torch_cuda.from_numpy(moved[0]).to("cuda:0"), 1: (torch_cuda.from_numpy(rest[1]).to("cuda:0"), MATRIX)}
            (t.update_meshes_device if form == "update_device" else t.rebuild_meshes_device)(src)
        held = [t.mesh_vertices(m) for m in (0, 1)]
        got = _frames(rpt, t, **ONE)
        assert mesh_form(rpt, t) == 20
        _assert_frames(got, _fresh(rpt, held), "%s: against a fresh upload" % form)
        assert not _same(got[0], still[0])
        assert all(np.array_equal(_bits(t.download_mesh_emission_map(m)), _bits(held_maps[m])) for m in (0, 1)), "a move leaves the maps alone"
    finally:
        t.close()


# ---- 7. composition with material maps; the texture guard --------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A", "H"])
def test_material_maps_compose_and_the_texture_guard(rpt, torch_cuda, case):
    t, base = _case_tracer(rpt, case, 9)
    args = inputs(MM.scene(), case)
    try:
        t.set_mesh_material_maps(MM.material_maps())
        mapped = _frames(rpt, t, **ONE)
        assert mesh_form(rpt, t) == map_form_of(case)
        # both kinds ON: the form emission maps alone take; an all-255 emission map leaves the material-mapped frames
        t.set_mesh_emission_maps({1: _emap(_constant(255, 5, 3), NEAREST, 2.2)})
        _assert_frames(_frames(rpt, t, **ONE), mapped, "case %s: an all-255 emission map over material maps" % case)
        assert mesh_form(rpt, t) == form_of(case)
        t.set_mesh_emission_maps({1: _emap(MM.noise_map(5, 3, 43), NEAREST)})
        both = _frames(rpt, t, **ONE)
        assert mesh_form(rpt, t) == form_of(case) and not _same(both[0], mapped[0])
        t.set_mesh_material_maps({0: None, 1: None})                  # emission maps alone: the same form, through the zero table
        alone = _frames(rpt, t, **ONE)
        assert mesh_form(rpt, t) == form_of(case) and not _same(alone[0], both[0])
        t.set_mesh_material_maps(MM.material_maps())
        _assert_frames(_frames(rpt, t, **ONE), both, "the material maps again")
        # replacing the texture keeps the map; removing it is refused and changes nothing
        t.set_mesh_textures({1: args["textures"][1]})
        _assert_frames(_frames(rpt, t, **ONE), both, "the same texture again")
        held = t.download_mesh_emission_map(1).copy()
        t.set_mesh_textures({1: dict(args["textures"][1], texels=random_texels(4, 4, 55), wrap="repeat")})
        assert np.array_equal(_bits(t.download_mesh_emission_map(1)), _bits(held))
        assert mesh_form(rpt, t) == form_of(case) and not _same(_frames(rpt, t, **ONE)[0], both[0])
        t.set_mesh_textures({1: args["textures"][1]})
        t.set_mesh_material_maps({1: None})
        if case == "H":
            t.set_mesh_normal_maps({1: None})
        one = _frames(rpt, t, **ONE)
        with pytest.raises(Exception) as e:
            t.set_mesh_textures({1: None})
        assert "remove the emission map first" in str(e.value) and rpt.lib().rpt_last_error(t._h).decode().startswith("rpt_set_mesh_textures: ")
        _assert_frames(_frames(rpt, t, **ONE), one, "after the refused removal")
        assert np.array_equal(_bits(t.download_mesh_emission_map(1)), _bits(held))
        t.upload_scene()                                             # an upload drops maps (and everything else that was set)
        _frames(rpt, t, **ONE)
        assert mesh_form(rpt, t) == MESH_RENDER_KERNELS.index("mesh_regen_kernel")
        out = np.zeros((3, 5, 4), F)
        assert rpt.lib().rpt_download_mesh_emission_map(t._h, 1, out.ctypes.data, 5, 3) == rpt._abi.RPT_ERR_INVALID_ARG
        assert rpt.lib().rpt_set_mesh_emission_maps(t._h, None, 0) == rpt._abi.RPT_OK
    finally:
        t.close()


# ---- 8. answers -------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_say_why_and_change_nothing(rpt, torch_cuda):
    A, lib = rpt._abi, rpt.lib()
    from rust_pathtracer_amd import scenes
    s, uvs = scenes.mesh_texture_scene()
    s.materials[0] = scenes.full_material(rgb=(0.8, 0.7, 0.6), roughness=0.9, emission=(1.0, 2.0, 3.0))
    t = rpt.Tracer(s, device=0, seed=10)
    try:
        t.set_mesh_textures({0: _tex(uvs[0], random_texels(3, 5, 61), CLAMP, BILINEAR, 2.2)})
        t.set_mesh_emission_maps({0: _emap(MM.noise_map(16, 16, 62), BILINEAR)})
        ref = _frames(rpt, t, **ONE)
        held = t.download_mesh_emission_map(0).copy()
        texels = np.ascontiguousarray(random_texels(2, 2, 63))
        bptr = texels.ctypes.data_as(C.POINTER(C.c_uint8))

        def items(*rows):
            arr = (A.rpt_mesh_emission_map * len(rows))()
            for it, r in zip(arr, rows):
                r = dict(dict(mesh=0, mode=A.RPT_MESH_EMISSION_MAP_ON, width=2, height=2, texels=bptr, filter=A.RPT_TEX_FILTER_BILINEAR, gamma=1.0), **r)
                for key, val in r.items():
                    setattr(it, key, val)
            return arr

        off = dict(mode=A.RPT_MESH_EMISSION_MAP_OFF, width=0, height=0, texels=None, filter=0, gamma=0.0)
        # in the stated order; each case but the last carries the NEXT check's fault as well, so the order itself is held
        cases = [("NULL items", None, 1, "items is NULL"),
                 ("mesh out of range", items(dict(mesh=2, mode=7)), 1, "mesh 2 out of range"),
                 ("named twice", items(dict(), dict(mode=7)), 2, "item 1: mesh 0 is named twice"),
                 ("mode", items(dict(mode=2, width=0)), 1, "mode 2"),
                 ("width 0", items(dict(width=0, texels=None)), 1, "a map of 0 x 2"),
                 ("NULL texels", items(dict(texels=None, filter=2)), 1, "texels is NULL"),
                 ("filter", items(dict(filter=2, gamma=0.0)), 1, "filter 2"),
                 ("gamma 0", items(dict(mesh=1, gamma=0.0)), 1, "gamma 0"),
                 ("gamma 17", items(dict(mesh=1, gamma=17.0)), 1, "gamma 17"),
                 ("gamma nan", items(dict(mesh=1, gamma=float("nan"))), 1, "gamma"),
                 ("OFF with a size", items(dict(off, width=2)), 1, "RPT_MESH_EMISSION_MAP_OFF takes"),
                 ("untextured", items(dict(mesh=1, width=16384, height=16384)), 1, "mesh 1 is untextured")]
        for what, arr, n, says in cases:
            assert lib.rpt_set_mesh_emission_maps(t._h, arr, n) == A.RPT_ERR_INVALID_ARG, what
            err = lib.rpt_last_error(t._h).decode()
            assert err.startswith("rpt_set_mesh_emission_maps: ") and says in err, (what, err)
        assert "item 0" in lib.rpt_last_error(t._h).decode()
        big = items(dict(width=8192, height=8193))                  # refused on the host from the sizes alone (texels is never read)
        assert lib.rpt_set_mesh_emission_maps(t._h, big, 1) == A.RPT_ERR_UNSUPPORTED and "2^26" in lib.rpt_last_error(t._h).decode()
        assert np.array_equal(_bits(t.download_mesh_emission_map(0)), _bits(held))
        _assert_frames(_frames(rpt, t, **ONE), ref, "after every rejected call")
        assert mesh_form(rpt, t) == 20
        assert lib.rpt_set_mesh_emission_maps(t._h, None, 0) == A.RPT_OK
        _assert_frames(_frames(rpt, t, **ONE), ref, "n_items == 0 does nothing")
        b = rpt.Tracer(scenes.six_primitive_scene(), device=0, seed=1)      # no scene with meshes
        try:
            assert lib.rpt_set_mesh_emission_maps(b._h, items(dict()), 1) == A.RPT_ERR_NO_SCENE
            assert lib.rpt_set_mesh_emission_maps(b._h, None, 1) == A.RPT_ERR_NO_SCENE         # no scene comes before NULL items
            out = np.zeros(4, F)
            assert lib.rpt_download_mesh_emission_map(b._h, 0, out.ctypes.data, 1, 1) == A.RPT_ERR_NO_SCENE
        finally:
            b.close()
    finally:
        t.close()


# ---- 9. unbiased ------------------------------------------------------------------------------------------------------------------
K_FRAMES = 256


def test_on_and_off_estimate_the_same_integral_under_a_map(rpt, torch_cuda):
    """scenes.mesh_emission_scene() at 32 x 24, K = 256 one-sample frames with seeds 2000 .. 2255, the striped lamp OFF and then ON;
    per frame the mean over all pixels and the three colour channels.  The existing mesh-light test's criterion: the means of the
    two runs differ by at most 5 standard errors of their difference, and the ON run's per-frame means have the lower variance.  A
    sampler that ignored the map, or looked it up elsewhere than the hit side does, would shift the ON mean alone.  The test prints
    its figures (pytest -s); DESIGN.md records them."""
    from rust_pathtracer_amd import scenes
    w, h = 32, 24
    s, textures, maps = scenes.mesh_emission_scene()
    t = rpt.Tracer(s, device=0, seed=2000)

    def run():
        means = []
        for k in range(K_FRAMES):
            t.seed = 2000 + k
            buf = rpt.ColorBuffer(w, h)
            t.render_n(buf, 1)
            means.append(float(np.asarray(buf.image(), np.float64)[..., :3].mean()))
        return np.array(means)

    try:
        t.set_mesh_textures(textures)
        t.set_mesh_emission_maps(maps)
        off = run()
        assert mesh_form(rpt, t) == 20
        t.set_mesh_lights({1: True})
        on = run()
        assert mesh_form(rpt, t) == 20
    finally:
        t.close()
    se_off, se_on = off.std(ddof=1) / np.sqrt(K_FRAMES), on.std(ddof=1) / np.sqrt(K_FRAMES)
    ratio = on.var(ddof=1) / off.var(ddof=1)
    print("mesh emission maps, K = %d: OFF mean %.6f se %.6f, ON mean %.6f se %.6f, variance ratio ON / OFF %.4f, difference %.2f se"
          % (K_FRAMES, off.mean(), se_off, on.mean(), se_on, ratio, abs(on.mean() - off.mean()) / np.hypot(se_off, se_on)))
    assert off.mean() > 0 and on.mean() > 0
    assert abs(on.mean() - off.mean()) <= 5.0 * np.hypot(se_off, se_on)
    assert ratio < 1.0
