"""Ray queries on the GPU (include/rpt.h, "ray queries").

1. Geometry: all eight words of rpt_hit and the occlusion byte equal tests/query_np.py's numpy float32 restatement of the ordered
   loop over spheres, planes and triangles, for 40 000 rays of every kind (NaN and infinite components included) at scales 2^0 and
   2^20.  Two NaN distances count as equal (query_np.py says why); every other word is compared bit for bit.
2. Ragged and empty batches write exactly n records; the host forms equal the device forms.
3. rpt_surface equals the words of the pinned test hooks, feature by feature and composed; with no feature ON it is the flat normal
   and the Python scene's material values, and a plane over a sphere reports the layered material.
4. The camera's rays equal rpt_probe_fn's GEN_RAY records for the same pixels with offsets 0.5.
5. Queries see every move and setter, on any stream; a rejected call returns its status and writes nothing.
6. Queries change no frame and no render form."""
import ctypes as C

import numpy as np
import pytest

import query_np as Q
from query_np import BILINEAR, CLAMP, MATRIX, NEAREST, REPEAT, random_texels

pytestmark = pytest.mark.gpu
F = np.float32
NONE = 0xFFFFFFFF
PATTERN = 0x5A5A5A5A


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _words(x):
    """A tensor or array of records as uint32 words on the host."""
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return np.atleast_1d(np.ascontiguousarray(x)).view(np.uint32)


def _trace(rpt, torch, t, r8, n=None, surfaces=False, stream=None):
    """rpt_trace_rays_device on the first `n` of `r8` [*, 8] into arrays one record longer than n, pre-filled with PATTERN:
    -> (hits [n + 1, 8], surfaces [n + 1, 16] or None) as uint32 words."""
    n = len(r8) if n is None else n
    dev = torch.from_numpy(np.ascontiguousarray(r8, F)).cuda()
    hits = torch.full((n + 1, 8), PATTERN, dtype=torch.int32, device="cuda")
    surf = torch.full((n + 1, 16), PATTERN, dtype=torch.int32, device="cuda") if surfaces else None
    torch.cuda.synchronize()
    rpt._lib.check(rpt.lib().rpt_trace_rays_device(t._h, dev.data_ptr(), n, hits.data_ptr(), surf.data_ptr() if surfaces else None, 0, stream), t._h)
    torch.cuda.synchronize()
    return _words(hits), (_words(surf) if surfaces else None)


def _occluded(rpt, torch, t, r8, n=None):
    n = len(r8) if n is None else n
    dev = torch.from_numpy(np.ascontiguousarray(r8, F)).cuda()
    out = torch.full((n + 1,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rpt._lib.check(rpt.lib().rpt_occluded_device(t._h, dev.data_ptr(), n, out.data_ptr(), 0, None), t._h)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _hook(rpt, torch, t, name, r7, words, flags=0):
    """One of the rpt_debug_mesh_*_query hooks on rays [n, 7] -> [n, words] uint32."""
    dev = torch.from_numpy(np.ascontiguousarray(r7, F)).cuda()
    out = torch.zeros(len(r7), words, dtype=torch.int32, device="cuda")
    rpt._lib.check(getattr(rpt.lib(), name)(t._h, dev.data_ptr(), len(r7), out.data_ptr(), flags, None), t._h)
    torch.cuda.synchronize()
    return _words(out)


_BIG = {}


def _big(rpt, torch, scale_exp):
    """The big run of test 1, made once per scale: scene, rays, the restatement's and the device's answers."""
    if scale_exp not in _BIG:
        s, r7, unit = Q.big_case(scale_exp)
        want_hits, want_occ = Q.restate(s, r7)
        r8 = Q.to_rpt_rays(r7)
        t = rpt.Tracer(s, device=0, seed=1)
        try:
            got_hits, _ = _trace(rpt, torch, t, r8)
            got_occ = _occluded(rpt, torch, t, r8)
        finally:
            t.close()
        _BIG[scale_exp] = dict(scene=s, r7=r7, r8=r8, unit=unit, want_hits=want_hits, want_occ=want_occ, got_hits=got_hits, got_occ=got_occ)
    return _BIG[scale_exp]


# ---- 1. geometry ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_exp", [0, 20])
def test_hits_and_occlusion_equal_the_ordered_loop(rpt, torch_cuda, scale_exp):
    """This test fails without the feature, at the missing symbol."""
    b = _big(rpt, torch_cuda, scale_exp)
    n = len(b["r7"])
    assert n == 40_000
    got, want = b["got_hits"], b["want_hits"]
    assert (got[n] == PATTERN).all(), "the guard record"
    bad = Q.compare_words(got[:n], want)
    names = ("t", "kind", "primitive", "mesh", "triangle", "u", "v", "reserved")
    per_word = {nm: int((got[:n, k] != want[:, k]).sum()) for k, nm in enumerate(names)}
    print("scale 2^%d: %d of %d rays differ; per word (NaN t counted) %s" % (scale_exp, len(bad), n, per_word))
    assert len(bad) == 0, "%d rays differ, first %s: got %s want %s" % (len(bad), bad[:3], got[bad[:3]], want[bad[:3]])
    occ_bad = np.nonzero(b["got_occ"][:n] != b["want_occ"])[0]
    assert len(occ_bad) == 0 and b["got_occ"][n] == 0x5A, "occluded: %d rays differ, first %s" % (len(occ_bad), occ_bad[:5])
    # the caps, on the rays with a unit direction (three in four; the sphere test assumes one) and, for spheres, a finite distance
    unit = b["unit"]
    kind, finite = want[unit, 1], np.isfinite(want[unit, 0].view(F))
    assert unit.mean() > 0.6 and (~unit).sum() > 10_000
    assert (kind == Q.HIT_TRIANGLE).mean() > 0.2 and ((kind == Q.HIT_SPHERE) & finite).mean() > 0.02 and (kind == Q.HIT_PLANE).mean() > 0.02
    assert b["want_occ"][unit].mean() > 0.05
    # (a property of the restatement's sample, not of the kernels: with a direction of any length the first sphere's test accepts
    #  most rays, so triangles win less often there; 5 % of 12 500 rays is still hundreds of them)
    assert (want[~unit, 1] == Q.HIT_TRIANGLE).mean() > 0.05 and (want[~unit, 1] == Q.HIT_SPHERE).mean() > 0.05, "the rays that keep their lengths hit things too"
    # a NaN max_dist gives 0, +inf "anything along the ray"
    r8 = b["r8"][:4096].copy()
    r8[:, 3] = np.nan
    t = rpt.Tracer(b["scene"], device=0, seed=1)
    try:
        assert not _occluded(rpt, torch_cuda, t, r8)[:4096].any()
        r8[:, 3] = np.inf
        r7 = b["r7"][:4096].copy()
        r7[:, 6] = np.inf
        assert np.array_equal(_occluded(rpt, torch_cuda, t, r8)[:4096], Q.restate(b["scene"], r7)[1])
    finally:
        t.close()


# ---- 2. ragged and empty ----------------------------------------------------------------------------------------------------------------
def test_ragged_batches_and_the_host_forms(rpt, torch_cuda):
    b = _big(rpt, torch_cuda, 0)
    t = rpt.Tracer(b["scene"], device=0, seed=1)
    try:
        for n in (0, 1, 255, 257):
            hits, surf = _trace(rpt, torch_cuda, t, b["r8"], n, surfaces=True)
            assert np.array_equal(hits[:n], b["got_hits"][:n]), n
            assert (hits[n] == PATTERN).all() and (surf[n] == PATTERN).all(), "the guard records at n = %d" % n
            plain, _ = _trace(rpt, torch_cuda, t, b["r8"], n)
            assert np.array_equal(plain, hits), "with and without surfaces, n = %d" % n
            occ = _occluded(rpt, torch_cuda, t, b["r8"], n)
            assert np.array_equal(occ[:n], b["got_occ"][:n]) and occ[n] == 0x5A, n
            # the host forms
            h_hits = np.full((n + 1, 8), PATTERN, np.uint32)
            h_surf = np.full((n + 1, 16), PATTERN, np.uint32)
            h_occ = np.full(n + 1, 0x5A, np.uint8)
            rays = np.ascontiguousarray(b["r8"][:max(n, 1)])
            rpt._lib.check(rpt.lib().rpt_trace_rays(t._h, rays.ctypes.data, n, h_hits.ctypes.data, h_surf.ctypes.data, 0), t._h)
            rpt._lib.check(rpt.lib().rpt_occluded(t._h, rays.ctypes.data, n, h_occ.ctypes.data, 0), t._h)
            assert np.array_equal(h_hits, hits) and np.array_equal(h_surf, surf) and np.array_equal(h_occ, occ), "host forms, n = %d" % n
        # the Python wrappers: tensors in, tensors out; numpy in, numpy out; the same words
        r8 = b["r8"][:257]
        dev = t.trace(torch_cuda.from_numpy(r8).cuda(), surfaces=True)
        host = t.trace(r8, surfaces=True)
        torch_cuda.cuda.synchronize()
        assert sorted(dev) == sorted(host) == sorted(["t", "kind", "primitive", "mesh", "triangle", "u", "v", "ng", "ns", "rgb", "emission", "roughness",
                                                      "metallic", "material"])
        for key in host:
            assert isinstance(host[key], np.ndarray) and torch_cuda.is_tensor(dev[key]) and dev[key].is_cuda, key
            assert np.array_equal(_words(dev[key].contiguous()), _words(host[key])), key
        assert np.array_equal(_words(host["t"]), b["got_hits"][:257, 0]) and np.array_equal(host["primitive"], b["got_hits"][:257, 2])
        assert "ng" not in t.trace(r8)
        assert np.array_equal(t.occluded(r8), b["got_occ"][:257])
        assert np.array_equal(t.occluded(torch_cuda.from_numpy(r8).cuda()).cpu().numpy(), b["got_occ"][:257])
        assert len(t.trace(r8[:0])["t"]) == 0 and len(t.occluded(r8[:0])) == 0
    finally:
        t.close()


# ---- 3. surfaces ----------------------------------------------------------------------------------------------------------------------
def _probe_setup():
    """test_gpu_mesh_normal_map.py's probe scene without its floor (the hooks see triangles only), emissive, and its rays."""
    from rust_pathtracer_amd import scenes
    s, uvs = Q.probe_scene()
    s.planes = []
    s.materials[0] = scenes.full_material(rgb=(0.8, 0.7, 0.6), roughness=0.9, metallic=0.35, emission=(3.0, 2.0, 0.7))
    s.materials[1] = scenes.full_material(rgb=(0.9, 0.9, 0.9), roughness=0.7, metallic=0.8, emission=(11.0, 0.3, 5.5))
    rng = np.random.default_rng(9100)
    r7 = Q.texture_rays(s, uvs, 5, 4096, rng)
    r7[::12, 3:6] = (rng.normal(size=(len(r7[::12]), 3)) * 0.2 + (0.0, 1.0, 0.3)).astype(F)      # upward: nothing is there
    return s, uvs, r7


def _assert_hook(hits, hook, what):
    """The hook's first word is the winning triangle's flattened index: rpt_hit.primitive; a miss is NONE on both sides."""
    tri = hits[:, 1] == Q.HIT_TRIANGLE
    assert np.array_equal(np.where(tri, hits[:, 2], NONE), hook[:, 0]), "%s: primitive and the hook's index" % what
    assert (hits[~tri, 1] == Q.HIT_NONE).all(), "a triangles-only scene"
    assert tri.mean() > 0.3 and (~tri).sum() >= 50, what
    return tri


def test_surfaces_equal_the_smooth_hook(rpt, torch_cuda):
    s = Q.mesh_test_scene()
    r7 = Q.mesh_rays(Q.mesh_tris(s), 4096, np.random.default_rng(9000))
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        t.set_mesh_shading({0: "smooth", 2: "smooth"})
        hook = _hook(rpt, torch_cuda, t, "rpt_debug_mesh_normal_query", r7, 4)
        hits, surf = _trace(rpt, torch_cuda, t, Q.to_rpt_rays(r7), surfaces=True)
        tri = _assert_hook(hits[:-1], hook, "smooth")
        assert np.array_equal(surf[:-1, 3:6], hook[:, 1:4]), "ns: %d rays differ" % int((surf[:-1, 3:6] != hook[:, 1:4]).any(axis=1).sum())
        ng = Q.flat_normals(Q.mesh_tris(s), hits[:-1][tri, 2])
        same = (surf[:-1][tri, 0:3] == _words(ng)) | (np.isnan(surf[:-1][tri, 0:3].view(F)) & np.isnan(ng))
        assert same.all(), "ng is the flat normal"
        assert (surf[:-1][tri, 0:3] != surf[:-1][tri, 3:6]).any(axis=1).mean() > 0.1, "smooth normals differ from flat ones"
        assert not surf[:-1][~tri].any(), "a miss is all zeros"
    finally:
        t.close()


@pytest.mark.parametrize("feature", ["texture", "normal_map", "material_map", "emission_map"])
def test_surfaces_equal_the_map_hooks(rpt, torch_cuda, feature):
    s, uvs, r7 = _probe_setup()
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        t.set_mesh_textures({m: Q.tex(uvs[m], random_texels(5, 3, 20 + m), (REPEAT, CLAMP, REPEAT)[m], (BILINEAR, NEAREST, BILINEAR)[m]) for m in (0, 1, 2)})
        if feature == "texture":
            hook, cols = _hook(rpt, torch_cuda, t, "rpt_debug_mesh_texture_query", r7, 4), slice(6, 9)
        elif feature == "normal_map":
            t.set_mesh_normal_maps({0: dict(texels=random_texels(5, 3, 31), filter="nearest", strength=2.0), 1: dict(texels=random_texels(16, 16, 32), filter="bilinear")})
            hook, cols = _hook(rpt, torch_cuda, t, "rpt_debug_mesh_normal_map_query", r7, 4), slice(3, 6)
        elif feature == "material_map":
            t.set_mesh_material_maps({0: dict(texels=random_texels(5, 3, 41), filter="nearest"), 1: dict(texels=random_texels(16, 16, 42), filter="bilinear")})
            hook, cols = _hook(rpt, torch_cuda, t, "rpt_debug_mesh_material_map_query", r7, 4)[:, :3], slice(12, 14)
        else:
            t.set_mesh_emission_maps({0: dict(texels=random_texels(5, 3, 51), filter="nearest", gamma=2.2), 1: dict(texels=random_texels(16, 16, 52), filter="bilinear")})
            hook, cols = _hook(rpt, torch_cuda, t, "rpt_debug_mesh_emission_map_query", r7, 7)[:, :4], slice(9, 12)
        hits, surf = _trace(rpt, torch_cuda, t, Q.to_rpt_rays(r7), surfaces=True)
        tri = _assert_hook(hits[:-1], hook, feature)
        diff = (surf[:-1, cols] != hook[:, 1:]).any(axis=1)
        assert not diff.any(), "%s: %d rays differ, first %s" % (feature, int(diff.sum()), np.nonzero(diff)[0][:3])
        assert len(np.unique(surf[:-1][tri][:, cols], axis=0)) > 50, "the map varies"
        assert not surf[:-1][~tri].any(), "a miss is all zeros"
        mat_of_mesh = np.array([m for _, _, m in s.meshes], np.uint32)
        assert np.array_equal(surf[:-1][tri, 14], mat_of_mesh[hits[:-1][tri, 3]]), "material is the mesh's"
        if feature != "normal_map":
            assert np.array_equal(surf[:-1][tri, 0:3], surf[:-1][tri, 3:6]), "no normal feature ON: ns is ng"
    finally:
        t.close()


def test_surfaces_of_a_composed_scene_equal_every_hook_that_applies(rpt, torch_cuda):
    """SMOOTH, texture, normal map, material map, emission map and cutout ON at once.  The cutout hook walks with the cut test, as the
    query does: (t, index) and, with per-ray max_dist, any_hit.  The other hooks walk without it, so they answer for the same
    triangle only where no hole lies in front: there — most rays — every surface word is theirs."""
    s, uvs, r7 = _probe_setup()
    r7[:, 6] = np.random.default_rng(9200).uniform(0.5, 1.5, len(r7)).astype(F)           # the targets lie at t = 1
    A = rpt._abi
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        t.set_mesh_textures({m: Q.tex(uvs[m], random_texels(5, 3, 20 + m), (REPEAT, CLAMP, REPEAT)[m], BILINEAR) for m in (0, 1, 2)})
        t.set_mesh_shading({0: "smooth"})
        t.set_mesh_normal_maps({0: dict(texels=random_texels(5, 3, 31), filter="nearest", strength=2.0), 1: dict(texels=random_texels(16, 16, 32), filter="bilinear")})
        t.set_mesh_material_maps({0: dict(texels=random_texels(5, 3, 41), filter="nearest"), 1: dict(texels=random_texels(16, 16, 42), filter="bilinear")})
        t.set_mesh_emission_maps({0: dict(texels=random_texels(5, 3, 51), filter="nearest", gamma=2.2), 1: dict(texels=random_texels(16, 16, 52), filter="bilinear")})
        t.set_mesh_cutouts({0: dict(alpha=Q.checker(4, 4, 4), threshold=128), 1: dict(alpha=Q.checker(5, 3, 5), threshold=128)})
        r8 = Q.to_rpt_rays(r7)
        hits, surf = _trace(rpt, torch_cuda, t, r8, surfaces=True)
        hits, surf = hits[:-1], surf[:-1]
        plain, _ = _trace(rpt, torch_cuda, t, r8)
        assert np.array_equal(plain[:-1], hits), "the closest kernel and the surface kernel agree"
        cut = _hook(rpt, torch_cuda, t, "rpt_debug_mesh_cutout_query", r7, 3, A.RPT_MESH_QUERY_USE_MAX)
        tri = hits[:, 1] == Q.HIT_TRIANGLE
        assert np.array_equal(hits[:, 0], cut[:, 0]) and np.array_equal(np.where(tri, hits[:, 2], NONE), cut[:, 1]), "(t, index) of the cut walk"
        assert np.array_equal(_occluded(rpt, torch_cuda, t, r8)[:-1], cut[:, 2].astype(np.uint8)), "any_hit of the cut walk"
        assert ((cut[:, 2] == 1) & tri).sum() > 100 and ((cut[:, 2] == 0) & tri).sum() > 100, "max_dist decides some"
        nrm = _hook(rpt, torch_cuda, t, "rpt_debug_mesh_normal_map_query", r7, 4)
        tex = _hook(rpt, torch_cuda, t, "rpt_debug_mesh_texture_query", r7, 4)
        mmap = _hook(rpt, torch_cuda, t, "rpt_debug_mesh_material_map_query", r7, 4)
        emap = _hook(rpt, torch_cuda, t, "rpt_debug_mesh_emission_map_query", r7, 7)
        assert np.array_equal(nrm[:, 0], tex[:, 0]) and np.array_equal(nrm[:, 0], mmap[:, 0]) and np.array_equal(nrm[:, 0], emap[:, 0])
        same = tri & (nrm[:, 0] == hits[:, 2])
        holes = tri & ~same
        assert same.mean() > 0.3 and holes.sum() > 100, "most rays meet no hole, many do: %g, %d" % (same.mean(), int(holes.sum()))
        for what, cols, want in (("ns", slice(3, 6), nrm[:, 1:4]), ("rgb", slice(6, 9), tex[:, 1:4]), ("roughness, metallic", slice(12, 14), mmap[:, 1:3]),
                                 ("emission", slice(9, 12), emap[:, 1:4])):
            diff = (surf[same][:, cols] != want[same]).any(axis=1)
            assert not diff.any(), "%s: %d rays differ" % (what, int(diff.sum()))
        assert (surf[same, 0:3] != surf[same, 3:6]).any(axis=1).mean() > 0.3, "the normals are bent"
        assert not surf[~tri].any()
    finally:
        t.close()


def _checker_rgb(params, d):
    """The checker floor's patch colour along direction d (include/rpt.h; analytical.rs:107-115), float32 operation by operation."""
    scale, offset, colour_a, colour_b = (F(p) for p in params)
    rem2 = lambda a: a - F(2.0) * np.trunc(a * F(0.5))                # noqa: E731
    with np.errstate(all="ignore"):
        x = (d[:, 0] / d[:, 1]) * scale + offset
        y = (d[:, 2] / d[:, 1]) * scale + offset
        second = ~(rem2(rem2(np.floor(x)) + rem2(np.floor(y))) < F(1.0))
    return np.where(second, colour_b, colour_a).astype(F)


def test_surfaces_with_no_feature_on(rpt, torch_cuda):
    """The geometry test's scene: flat normals, the Python scene's material values, and the plane's patch layered over the sphere's
    full material where a ray met the sphere first and the plane nearer."""
    b = _big(rpt, torch_cuda, 0)
    s, n = b["scene"], 4096
    pick = np.arange(0, len(b["r7"]), 9)[:n]                          # every kind of ray
    r7, r8 = b["r7"][pick], b["r8"][pick]
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        hits, surf = _trace(rpt, torch_cuda, t, r8, surfaces=True)
    finally:
        t.close()
    hits, surf = hits[:-1], surf[:-1]
    assert np.array_equal(hits, b["got_hits"][pick])
    kind = hits[:, 1]
    finite = np.isfinite(hits[:, 0].view(F))                          # (a NaN distance gives NaN normals: query_np.py)
    ok = (surf[:, 0:3] == surf[:, 3:6]) | (np.isnan(surf[:, 0:3].view(F)) & np.isnan(surf[:, 3:6].view(F)))
    assert ok.all(), "ns equals ng"
    assert not surf[kind == Q.HIT_NONE].any(), "a miss is all zeros"
    assert not surf[:, 15].any(), "reserved"
    mats = [m.fields for m in s.materials]
    # triangles: the flat normal and the mesh material's fields
    tri = kind == Q.HIT_TRIANGLE
    assert np.array_equal(surf[tri, 0:3], _words(Q.flat_normals(Q.mesh_tris(s), hits[tri, 2]))), "ng is normalize(cross(e1, e2))"
    mat_of_mesh = np.array([m for _, _, m in s.meshes], np.uint32)
    assert np.array_equal(surf[tri, 14], mat_of_mesh[hits[tri, 3]])
    for m in (0, 1):
        sel = tri & (surf[:, 14] == m)
        assert sel.sum() > 50
        want = np.array(list(mats[m]["rgb"]) + list(mats[m]["emission"]) + [mats[m]["roughness"], mats[m]["metallic"]], F)
        assert (surf[sel, 6:14] == _words(want)).all(), "mesh material %d" % m
    # spheres: the outward normal, the sphere material's fields
    unit = np.abs(np.linalg.norm(r7[:, 3:6].astype(np.float64), axis=1) - 1.0) < 1e-3      # (the sphere test assumes a unit direction)
    sph = (kind == Q.HIT_SPHERE) & finite & unit
    assert sph.sum() > 100
    sphere_mat = np.array([sp[2] for sp in s.spheres], np.uint32)
    assert np.array_equal(surf[sph, 14], sphere_mat[hits[sph, 2]])
    for i, sp in enumerate(s.spheres):
        sel = sph & (hits[:, 2] == i)
        m = mats[sp[2]]
        want = np.array(list(m["rgb"]) + list(m["emission"]) + [m["roughness"], m["metallic"]], F)
        assert sel.sum() > 20 and (surf[sel, 6:14] == _words(want)).all(), "sphere %d" % i
        want_n = Q.sphere_normals(r7[sel, 0:3], r7[sel, 3:6], hits[sel, 0].view(F), sp[0])
        assert np.array_equal(surf[sel, 0:3], _words(want_n)), "sphere %d: ng is normalize((o + t d) - centre), %d rays differ" % (i, int((surf[sel, 0:3] != _words(want_n)).any(axis=1).sum()))
    # the plane: its normal, its material's index, the checker's rgb and roughness over what lies beneath
    pl = kind == Q.HIT_PLANE
    assert pl.sum() > 100 and (surf[pl, 14] == s.planes[0][3]).all()
    assert (surf[pl, 0:3] == _words(np.array(s.planes[0][0], F))).all()
    floor = s.materials[s.planes[0][3]]
    assert sorted(floor.fields) == ["roughness"] and floor.checker_dir is not None
    rgb = _checker_rgb(floor.checker_dir, r7[pl, 3:6])
    assert (surf[pl, 6:9] == _words(np.stack([rgb, rgb, rgb], 1))).all(), "the patch's rgb"
    assert len(np.unique(rgb)) == 2
    assert (surf[pl, 12] == _words(F(floor.fields["roughness"]))).all(), "the patch's roughness"
    # ... layered: the sphere accepted before the plane wrote every field, the patch overwrote two
    with np.errstate(all="ignore"):
        under = np.full(n, -1)
        dist = np.full(n, Q.F32_MAX, F)
        for i, sp in enumerate(s.spheres):
            h, tt = Q.hit_sphere(r7[:, 0:3], r7[:, 3:6], sp[0], sp[1])
            acc = h & (np.full(n, i == 0) | (tt < dist))
            dist, under = np.where(acc, tt, dist), np.where(acc, i, under)
    layered = pl & (under >= 0)
    bare = pl & (under < 0)
    assert layered.sum() > 20 and bare.sum() > 20, "planes over a sphere and planes alone: %d, %d" % (int(layered.sum()), int(bare.sum()))
    metallic_under = np.array([mats[sp[2]]["metallic"] for sp in s.spheres], F)
    assert np.array_equal(surf[layered, 13], _words(metallic_under[under[layered]])), "the sphere's metallic shows through the patch"
    assert len(np.unique(surf[layered, 13])) == 2, "both spheres lie under the plane somewhere"
    from rust_pathtracer_amd import scenes
    assert (surf[bare, 13] == _words(F(scenes._DEFAULTS["metallic"]))).all() and not surf[pl, 9:12].any(), "Material::new() beneath a bare plane"


# ---- 4. camera rays -------------------------------------------------------------------------------------------------------------------
def test_camera_rays_equal_the_gen_ray_probe(rpt, torch_cuda):
    w, h = 37, 23
    s = Q.small_scene()
    s.camera = rpt.Pinhole((2.0, 1.0, -3.0), (0.5, 0.0, 1.0), 35.0)
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        rays = t.camera_rays(w, h)
        torch_cuda.cuda.synchronize()
        got = rays.cpu().numpy()
        assert got.shape == (w * h, 8)
        # what a render launch computes for pixel (x, y), row 0 on top (csrc/kernel_common.h, pixel_coords), in float32
        y, x = np.divmod(np.arange(w * h), w)
        j = (h - 1 - y).astype(F)
        px = x.astype(F) / F(w)
        py = F(1.0) - (F(h) - j) / F(h)
        want = Q.gen_ray_probe(rpt, torch_cuda, t, px, py, w, h)
        assert np.array_equal(_words(got[:, 0:3]), _words(want[:, 0:3])), "origins"
        assert np.array_equal(_words(got[:, 4:7]), _words(want[:, 3:6])), "directions: %d differ" % int((_words(got[:, 4:7]) != _words(want[:, 3:6])).any(axis=1).sum())
        assert (_words(got[:, 3]) == Q.INF_BITS).all() and not _words(got[:, 7]).any(), "max_dist is +inf, reserved 0"
        d = got[:, 4:7].reshape(h, w, 3)
        assert d[0, :, 1].mean() > d[-1, :, 1].mean(), "row 0 is the top row"
        assert len(np.unique(_words(got[:, 4:7]), axis=0)) == w * h
        # first-hit buffers: one camera_rays plus one trace
        out = t.trace(rays, surfaces=True)
        torch_cuda.cuda.synchronize()
        kinds = out["kind"].cpu().numpy()
        assert (kinds == Q.HIT_TRIANGLE).sum() > 20 and np.isfinite(out["t"].cpu().numpy()[kinds == Q.HIT_TRIANGLE]).all()
    finally:
        t.close()


# ---- 5. state -------------------------------------------------------------------------------------------------------------------------
def _state_rays(scene):
    return Q.to_rpt_rays(Q.unit_directions(Q.mesh_rays(Q.mesh_tris(scene), 4096, np.random.default_rng(9500))))


def _records(rpt, torch, t, r8, stream=None):
    hits, surf = _trace(rpt, torch, t, r8, surfaces=True, stream=stream)
    return np.concatenate([hits[:-1], surf[:-1], _occluded(rpt, torch, t, r8)[:-1, None].astype(np.uint32)], 1)


def _fresh_records(rpt, torch, arrays, r8):
    f = rpt.Tracer(Q.with_vertices(Q.small_scene, arrays), device=0, seed=1)
    try:
        f.set_mesh_shading({0: "smooth"})
        return _records(rpt, torch, f, r8)
    finally:
        f.close()


@pytest.mark.parametrize("move", ["update_meshes", "rebuild_meshes", "update_meshes_device", "rebuild_meshes_device"])
def test_queries_see_every_move(rpt, torch_cuda, move):
    from rust_pathtracer_amd import scenes
    s = Q.small_scene()
    r8 = _state_rays(s)
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        t.set_mesh_shading({0: "smooth"})
        before = _records(rpt, torch_cuda, t, r8)
        moved = scenes.mesh_scene_moved(s, 0.5)
        if move.endswith("_device"):
            getattr(t, move)({m: (torch_cuda.from_numpy(v).cuda(), MATRIX) for m, v in enumerate(moved)})
            held = [t.mesh_vertices(m) for m in range(len(moved))]
        else:
            getattr(t, move)(dict(enumerate(moved)))
            held = moved
        # a query on a second stream right after the move sees the move
        side = torch_cuda.cuda.Stream()
        hits, surf = _trace(rpt, torch_cuda, t, r8, surfaces=True, stream=C.c_void_p(side.cuda_stream))
        after = _records(rpt, torch_cuda, t, r8)
        assert np.array_equal(hits[:-1], after[:, 0:8]) and np.array_equal(surf[:-1], after[:, 8:24]), "the second stream"
        want = _fresh_records(rpt, torch_cuda, held, r8)
        diff = (after != want).any(axis=1)
        assert not diff.any(), "%s: %d rays differ from a fresh upload, first %s" % (move, int(diff.sum()), np.nonzero(diff)[0][:3])
        assert (after != before).any(axis=1).mean() > 0.2, "the move matters"
        assert (after[:, 1] == Q.HIT_TRIANGLE).mean() > 0.2
    finally:
        t.close()


def test_cutouts_on_and_off_again(rpt, torch_cuda):
    s, uvs, r7 = _probe_setup()
    r8 = Q.to_rpt_rays(r7)
    textures = {m: Q.tex(uvs[m], random_texels(5, 3, 20 + m), REPEAT, BILINEAR) for m in (0, 1, 2)}
    never = rpt.Tracer(s, device=0, seed=1)
    try:
        never.set_mesh_textures(textures)
        want = _records(rpt, torch_cuda, never, r8)
    finally:
        never.close()
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        t.set_mesh_textures(textures)
        t.set_mesh_cutouts({0: dict(alpha=Q.checker(4, 4, 4), threshold=128)})
        on = _records(rpt, torch_cuda, t, r8)
        assert (on != want).any(axis=1).mean() > 0.05, "holes matter"
        t.set_mesh_cutouts({0: None})
        assert np.array_equal(_records(rpt, torch_cuda, t, r8), want), "OFF again: a context that never had a cutout"
    finally:
        t.close()


def test_rejected_calls_return_their_status_and_write_nothing(rpt, torch_cuda):
    A, lib = rpt._abi, rpt.lib()
    s = Q.small_scene()
    r8 = _state_rays(s)[:256]
    dev = torch_cuda.from_numpy(r8).cuda()
    hits = torch_cuda.full((257, 8), PATTERN, dtype=torch_cuda.int32, device="cuda")
    surf = torch_cuda.full((257, 16), PATTERN, dtype=torch_cuda.int32, device="cuda")
    occ = torch_cuda.full((272,), 0x5A, dtype=torch_cuda.uint8, device="cuda")
    cam = torch_cuda.full((4 * 4 + 1, 8), PATTERN, dtype=torch_cuda.int32, device="cuda")
    p_r, p_h, p_s, p_o, p_c = dev.data_ptr(), hits.data_ptr(), surf.data_ptr(), occ.data_ptr(), cam.data_ptr()

    def untouched():
        torch_cuda.cuda.synchronize()
        return bool((hits == PATTERN).all() and (surf == PATTERN).all() and (occ == 0x5A).all() and (cam == PATTERN).all())

    def every_call(t, status, what):
        assert lib.rpt_trace_rays_device(t._h, p_r, 256, p_h, p_s, 0, None) == status, what
        assert lib.rpt_occluded_device(t._h, p_r, 256, p_o, 0, None) == status, what
        assert lib.rpt_camera_rays_device(t._h, 4, 4, p_c, None) == status, what
        h = np.full((256, 8), PATTERN, np.uint32)
        o = np.full(256, 0x5A, np.uint8)
        assert lib.rpt_trace_rays(t._h, r8.ctypes.data, 256, h.ctypes.data, None, 0) == status, what
        assert lib.rpt_occluded(t._h, r8.ctypes.data, 256, o.ctypes.data, 0) == status, what
        assert (h == PATTERN).all() and (o == 0x5A).all() and untouched(), what

    t = rpt.Tracer(s, device=0, seed=1)
    try:
        bad = A.RPT_ERR_INVALID_ARG
        assert lib.rpt_trace_rays_device(t._h, p_r + 4, 255, p_h, None, 0, None) == bad and b"16-byte aligned" in lib.rpt_last_error(t._h)
        assert lib.rpt_trace_rays_device(t._h, p_r, 256, p_h + 8, None, 0, None) == bad
        assert lib.rpt_trace_rays_device(t._h, p_r, 256, p_h, p_s + 4, 0, None) == bad
        assert lib.rpt_occluded_device(t._h, p_r + 4, 255, p_o, 0, None) == bad
        assert lib.rpt_camera_rays_device(t._h, 4, 4, p_c + 8, None) == bad
        assert lib.rpt_trace_rays_device(t._h, p_r, 256, p_h, p_s, 1, None) == bad and b"reserved" in lib.rpt_last_error(t._h)
        assert lib.rpt_occluded_device(t._h, p_r, 256, p_o, 1, None) == bad
        assert lib.rpt_trace_rays(t._h, r8.ctypes.data, 256, r8.ctypes.data, None, 0x80000000) == bad
        assert lib.rpt_occluded(t._h, r8.ctypes.data, 256, r8.ctypes.data, 2) == bad
        assert lib.rpt_trace_rays_device(t._h, None, 256, p_h, None, 0, None) == bad and b"NULL array" in lib.rpt_last_error(t._h)
        assert lib.rpt_trace_rays_device(t._h, p_r, 256, None, None, 0, None) == bad
        assert lib.rpt_occluded_device(t._h, p_r, 256, None, 0, None) == bad
        assert lib.rpt_camera_rays_device(t._h, 4, 4, None, None) == bad
        assert lib.rpt_camera_rays_device(t._h, 0, 4, p_c, None) == bad and lib.rpt_camera_rays_device(t._h, 4, 0, p_c, None) == bad
        assert lib.rpt_trace_rays_device(t._h, p_r, 0x7FFFFFFF * 256 + 1, p_h, None, 0, None) == bad and b"workgroups" in lib.rpt_last_error(t._h)
        assert lib.rpt_occluded_device(t._h, p_r, 2 ** 64 - 1, p_o, 0, None) == bad and lib.rpt_trace_rays(t._h, r8.ctypes.data, 2 ** 64 - 200, r8.ctypes.data, None, 0) == bad
        assert lib.rpt_occluded(t._h, None, 3, None, 0) == bad
        assert untouched()
        # n == 0 is RPT_OK and launches nothing, NULL arrays or not
        assert lib.rpt_trace_rays_device(t._h, None, 0, None, None, 0, None) == A.RPT_OK and lib.rpt_occluded_device(t._h, None, 0, None, 0, None) == A.RPT_OK
        assert lib.rpt_trace_rays(t._h, None, 0, None, None, 0) == A.RPT_OK and lib.rpt_occluded(t._h, None, 0, None, 0) == A.RPT_OK
        assert untouched()
        # a misaligned pointer is rejected whatever n is; the occlusion bytes need no alignment
        assert lib.rpt_trace_rays_device(t._h, None, 0, None, p_s + 4, 0, None) == bad and lib.rpt_trace_rays_device(t._h, p_r + 4, 0, None, None, 0, None) == bad
        assert untouched()
        odd = torch_cuda.full((258,), 0x5A, dtype=torch_cuda.uint8, device="cuda")
        assert lib.rpt_occluded_device(t._h, p_r, 256, odd.data_ptr() + 1, 0, None) == A.RPT_OK
        torch_cuda.cuda.synchronize()
        got = odd.cpu().numpy()
        assert got[0] == 0x5A and got[257] == 0x5A and (got[1:257] <= 1).all()
        # a scene that is not a mesh scene
        t._scene = rpt.AnalyticalScene()
        t.upload_scene()
        every_call(t, A.RPT_ERR_UNSUPPORTED, "an analytical scene")
        assert b"not yet" in lib.rpt_last_error(t._h)
    finally:
        t.close()
    # no scene at all
    h = C.c_void_p()
    assert lib.rpt_create(C.byref(h), 0) == A.RPT_OK
    try:
        assert lib.rpt_trace_rays_device(h, p_r, 256, p_h, p_s, 0, None) == A.RPT_ERR_NO_SCENE
        assert lib.rpt_occluded_device(h, p_r, 256, p_o, 0, None) == A.RPT_ERR_NO_SCENE
        assert lib.rpt_camera_rays_device(h, 4, 4, p_c, None) == A.RPT_ERR_NO_SCENE
        assert untouched()
    finally:
        lib.rpt_destroy(h)
    # a context with more than one local device (here: the device listed twice)
    m = rpt.Tracer(s, devices=[0, 0], seed=1)
    try:
        every_call(m, A.RPT_ERR_UNSUPPORTED, "two local devices")
        assert b"one local device" in lib.rpt_last_error(m._h)
    finally:
        m.close()


# ---- 6. nothing else moved --------------------------------------------------------------------------------------------------------------
def test_queries_change_no_frame_and_no_form(rpt, torch_cuda):
    s = Q.small_scene()
    r8 = _state_rays(s)
    t = rpt.Tracer(s, device=0, seed=4)
    try:
        t.set_mesh_shading({0: "smooth"})

        def frame():
            buf = rpt.DeviceColorBuffer(64, 48)
            t.render_n(buf, 2)
            torch_cuda.cuda.synchronize()
            return buf.pixels.cpu().numpy().view(np.uint32), Q.mesh_form(rpt, t)

        before, form = frame()
        dev = torch_cuda.from_numpy(r8).cuda()
        for k in range(6):
            t.trace(dev, surfaces=bool(k & 1))
            t.occluded(dev)
            t.trace(r8[:300], surfaces=True)
            assert Q.mesh_form(rpt, t) == form, "rpt_debug_mesh_form is the last RENDER's"
        t.trace(t.camera_rays(64, 48))
        after, form_after = frame()
        assert np.array_equal(before, after) and form_after == form
    finally:
        t.close()
