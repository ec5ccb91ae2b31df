"""Smooth mesh shading on the GPU (include/rpt.h, "smooth mesh shading"): vertex normals the library computes on the device and keeps
current through every call that moves a mesh, interpolated at the hit.

Everything is bit for bit, and nothing takes the device's own output as truth:
* the normals table (rpt_download_mesh_normals) equals tests/test_mesh_smooth_host.py's numpy float32 restatement, on closed meshes,
  degenerate triangles, a hub of valence 300, unnamed vertices, exact cancellation, meshes of 256 and 257 vertices, at scales where the
  normals live and where every one is (0, 0, 0);
* the normal a hit is shaded with (rpt_debug_mesh_normal_query) equals the restatement of u, v, the interpolation and the fall-back,
  for the walk and the ordered loop, on a scene with smooth and flat meshes;
* smooth frames differ from flat ones, do not depend on how they are dispatched, and going back to FLAT gives the frames of a context
  that never heard of smooth shading; rpt_debug_kernel_choice's bit 26 is set exactly while a mesh is SMOOTH;
* after every kind of move the normals equal the restatement on the new positions and the frames those of a fresh upload of the moved
  scene followed by rpt_set_mesh_shading;
* a rejected call leaves modes, normals and frames as they were; an upload leaves every mesh FLAT; the product library renders the
  test build's smooth frame."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_mesh import _mesh_tris, _rays, _test_scene, brute_force
from test_gpu_mesh_update import _assert_frames, _choice, _frames, _same, _small_scene, _with_vertices
from test_mesh_smooth_host import edge_meshes, restate_hit_normals, restate_vertex_normals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MESH_BIT, SMOOTH_BIT = 1 << 25, 1 << 26


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _bits_equal(got, want):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


def _all_smooth(t):
    t.set_mesh_shading({m: "smooth" for m in range(len(t.scene().meshes))})


def _assert_normals(t, meshes, what):
    """The context's normals of `meshes` (indices) equal the restatement on the positions the context holds."""
    for m in meshes:
        v, idx, _ = t.scene().meshes[m]
        held = t.mesh_vertices(m)
        got, want = t.mesh_normals(m), restate_vertex_normals(held, idx)
        assert got.shape == want.shape == (len(np.asarray(v).reshape(-1, 3)), 3)
        bad = ~_bits_equal(got, want)
        assert not bad.any(), "%s, mesh %d: %d words differ, first vertex %d: got %s want %s" % (
            what, m, int(bad.sum()), int(np.nonzero(bad.any(axis=1))[0][0]), got[bad.any(axis=1)][0], want[bad.any(axis=1)][0])


# ---- 1. the normals table ---------------------------------------------------------------------------------------------------------
def _table_scene(scale):
    s = _test_scene(scale)
    for _, v, t in edge_meshes():
        s.meshes.append(((v * F(scale)).astype(F), t, 1))
    return s


@pytest.mark.parametrize("scale_exp", [0, -20, 20, -40, 40])
def test_normals_table_equals_the_numpy_restatement(rpt, torch_cuda, scale_exp):
    s = _table_scene(2.0 ** scale_exp)
    n = len(s.meshes)
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        # in two calls: the meshes not named keep their mode
        t.set_mesh_shading({m: "smooth" for m in range(0, n, 2)})
        _assert_normals(t, range(0, n, 2), "every second mesh at scale 2^%d" % scale_exp)
        out = np.zeros((len(s.meshes[1][0]), 3), F)
        assert rpt.lib().rpt_download_mesh_normals(t._h, 1, out.ctypes.data, len(out)) == rpt._abi.RPT_ERR_INVALID_ARG
        assert b"mesh 1 is FLAT" in rpt.lib().rpt_last_error(t._h)
        t.set_mesh_shading({m: "smooth" for m in range(1, n, 2)})
        _assert_normals(t, range(n), "every mesh at scale 2^%d" % scale_exp)
        live = [bool(t.mesh_normals(m).any()) for m in range(n)]
        if abs(scale_exp) == 40:
            assert not any(live), "l2 under- or overflows: every normal is (0, 0, 0)"
        else:
            names = ["icosphere", "torus", "odd triangles"] + [what for what, _, _ in edge_meshes()]
            assert [nm for nm, l in zip(names, live) if not l] == ["two coincident triangles of opposite winding"]
            for m in (0, 1):
                assert np.allclose(np.linalg.norm(t.mesh_normals(m).astype(np.float64), axis=1), 1.0, atol=1e-6)
            unnamed = t.mesh_normals(names.index("a vertex no triangle names"))
            assert not unnamed[3].any() and unnamed[:3].any(axis=1).all()
        buf = rpt.ColorBuffer(32, 24)
        t.render_n(buf, 1)
        assert _choice(rpt, t) & (MESH_BIT | SMOOTH_BIT) == MESH_BIT | SMOOTH_BIT
    finally:
        t.close()


# ---- 2. the normal at a hit -------------------------------------------------------------------------------------------------------
def _normal_query(rpt, torch, tracer, rays, flags):
    n = len(rays)
    dev = torch.from_numpy(np.ascontiguousarray(rays, dtype=F)).cuda()
    out = torch.zeros(n, 4, dtype=torch.int32, device="cuda")
    rpt._lib.check(rpt.lib().rpt_debug_mesh_normal_query(tracer._h, dev.data_ptr(), n, out.data_ptr(), flags, None), tracer._h)
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    return o[:, 0].astype(np.int64) - (o[:, 0] == 0xFFFFFFFF) * (1 << 32), o[:, 1:4].copy().view(F)


def _restate_query(scene, smooth, rays):
    """-> (index or -1, normal [n, 3] f32, which hits fell back or are flat) by the ordered loop and include/rpt.h's normal."""
    tris = _mesh_tris(scene)
    _, index, _ = brute_force(tris, rays, False)
    vn, corner, is_smooth, first = [], [], [], 0
    for m, (v, t, _) in enumerate(scene.meshes):
        vn.append(restate_vertex_normals(v, t) if m in smooth else np.zeros((len(v), 3), F))
        corner.append(np.asarray(t, np.int64) + first)
        is_smooth.append(np.full(len(t), m in smooth))
        first += len(v)
    vn, corner, is_smooth = np.concatenate(vn), np.concatenate(corner), np.concatenate(is_smooth)
    hit = index >= 0
    k = index[hit]
    a, e1, e2 = tris[k, 0], tris[k, 1] - tris[k, 0], tris[k, 2] - tris[k, 0]
    zero = np.zeros((len(k), 3), F)
    sm = is_smooth[k][:, None]
    # a FLAT mesh's triangle: zero corner normals give l2 = 0, the statement's fall-back, which is the flat normal
    nrm, fell = restate_hit_normals(rays[hit, 0:3], rays[hit, 3:6], a, e1, e2, np.where(sm, vn[corner[k, 0]], zero),
                                    np.where(sm, vn[corner[k, 1]], zero), np.where(sm, vn[corner[k, 2]], zero))
    want = np.zeros((len(rays), 3), F)
    want[hit] = nrm
    flat = np.zeros(len(rays), bool)
    flat[hit] = fell
    return index, want, flat


@pytest.mark.parametrize("scale_exp", [0, -20, 20, -40, 40])
def test_hit_normals_equal_the_numpy_restatement(rpt, torch_cuda, scale_exp):
    """The icosphere and the odd triangles SMOOTH, the torus FLAT."""
    scale = 2.0 ** scale_exp
    s = _test_scene(scale)
    smooth = (0, 2)
    rng = np.random.default_rng(3000 + scale_exp)
    rays = _rays(_mesh_tris(s), 16_000, rng, scale)
    sizes = dict(sizes=((96, 54, 5), (64, 48, 1)), resident=None)
    t = rpt.Tracer(s, device=0, seed=6)
    try:
        flat_frames = _frames(rpt, t, **sizes)
        assert not _choice(rpt, t) & SMOOTH_BIT
        t.set_mesh_shading({m: "smooth" for m in smooth})
        index, want, fell = _restate_query(s, smooth, rays)
        for brute in (False, True):
            got_i, got_n = _normal_query(rpt, torch_cuda, t, rays, rpt._abi.RPT_MESH_QUERY_BRUTE if brute else 0)
            assert np.array_equal(got_i, index), "index (brute %s): %d rays differ" % (brute, int((got_i != index).sum()))
            bad = np.nonzero(~_bits_equal(got_n, want).all(axis=1))[0]
            assert len(bad) == 0, "normal (brute %s): %d rays differ, first %s: got %s want %s" % (brute, len(bad), bad[:3], got_n[bad[:3]], want[bad[:3]])
        hit = index >= 0
        assert hit.mean() > 0.2
        frames = _frames(rpt, t, **sizes)
        assert _choice(rpt, t) & SMOOTH_BIT
        if abs(scale_exp) == 40:
            assert fell[hit].all(), "every vertex normal is (0, 0, 0): every answer is the flat normal"
            _assert_frames(frames, flat_frames, "scale 2^%d: smooth against flat" % scale_exp)
        else:
            assert 0.1 < fell[hit].mean() < 0.9, "interpolated and flat answers both occur"
            interp = hit & ~fell
            assert np.allclose(np.linalg.norm(want[interp].astype(np.float64), axis=1), 1.0, atol=1e-6)
    finally:
        t.close()


# ---- 3. frames --------------------------------------------------------------------------------------------------------------------
def test_smooth_frames_do_not_depend_on_the_dispatch_and_flat_again_is_flat(rpt, torch_cuda):
    from test_gpu_mesh import _small_mesh_scene
    w, h, spp = 80, 48, 6
    s = _small_mesh_scene()

    def render(t):
        buf = rpt.DeviceColorBuffer(w, h)
        t.render_n(buf, spp)
        torch_cuda.cuda.synchronize()
        return buf.pixels.cpu().numpy(), _choice(rpt, t)

    t = rpt.Tracer(s, device=0, seed=3)
    try:
        never, choice = render(t)
        assert choice & MESH_BIT and not choice & SMOOTH_BIT
        t.set_mesh_shading({0: "smooth"})
        one, choice = render(t)
        assert choice & MESH_BIT and choice & SMOOTH_BIT
        t.set_mesh_shading({1: "smooth"})
        ref, choice = render(t)
        assert choice & SMOOTH_BIT and np.isfinite(ref).all() and ref[..., :3].mean() > 0.01
        assert not _same(one, never) and not _same(ref, one) and not _same(ref, never), "each smooth mesh changes the picture"
        for disp in ((0, 12, 64, 0), (1, 0, 64, 0), (1, 1000, 1, 0), (2, 1000, 2, 7)):      # incl. chunked launches (unit_rounds 1000)
            t.set_dispatch(*disp)
            got, choice = render(t)
            assert _same(got, ref) and choice & SMOOTH_BIT, disp
        t.set_dispatch(1, 12, 64, 0)
        t.render_resident(w, h, spp)
        assert _same(t.resident_to_host(w, h).pixels.reshape(h, w, 4), ref.reshape(h, w, 4)), "resident"
        # back to FLAT, one mesh at a time: bit 26 goes with the last one, and the frames are the never-smoothed ones
        t.set_mesh_shading({1: "flat"})
        got, choice = render(t)
        assert _same(got, one) and choice & SMOOTH_BIT
        t.set_mesh_shading({0: "flat", 1: "flat"})
        got, choice = render(t)
        assert _same(got, never) and choice & MESH_BIT and not choice & SMOOTH_BIT
        out = np.zeros((len(s.meshes[0][0]), 3), F)
        assert rpt.lib().rpt_download_mesh_normals(t._h, 0, out.ctypes.data, len(out)) == rpt._abi.RPT_ERR_INVALID_ARG
    finally:
        t.close()
    m = rpt.Tracer(s, devices=[0, 0], seed=3)
    try:
        _all_smooth(m)
        m.render_resident(w, h, spp)
        assert _same(m.resident_to_host(w, h).pixels.reshape(h, w, 4), ref.reshape(h, w, 4)), "device listed twice"
        _assert_normals(m, (0, 1), "device listed twice")
    finally:
        m.close()


# ---- 4. moves ---------------------------------------------------------------------------------------------------------------------
_fresh = {}


def _fresh_smooth_frames(rpt, phase):
    """The yardstick, once per phase: a fresh context that uploads the moved scene and then sets every mesh SMOOTH."""
    from rust_pathtracer_amd import scenes
    if phase not in _fresh:
        moved = scenes.mesh_scene_moved(_small_scene(), phase)
        b = rpt.Tracer(_with_vertices(_small_scene, moved), device=0, seed=8)
        try:
            _all_smooth(b)
            _fresh[phase] = (moved, _frames(rpt, b))
        finally:
            b.close()
    return _fresh[phase]


def _move(torch, t, form, moved):
    if form == "update":
        t.update_meshes(dict(enumerate(moved)))
    elif form == "rebuild":
        t.rebuild_meshes(dict(enumerate(moved)))
    else:
        src = {m: torch.from_numpy(np.ascontiguousarray(v, F)).to("cuda:0") for m, v in enumerate(moved)}
        (t.update_meshes_device if form == "update_device" else t.rebuild_meshes_device)(src)


@pytest.mark.parametrize("form", ["update", "rebuild", "update_device", "rebuild_device"])
def test_normals_and_frames_follow_every_kind_of_move(rpt, torch_cuda, form):
    still, still_frames = _fresh_smooth_frames(rpt, 0)
    t = rpt.Tracer(_small_scene(), device=0, seed=8)
    try:
        _all_smooth(t)
        _assert_frames(_frames(rpt, t), still_frames, "before any move")
        for phase in (0.05, 2.0):                                     # a small and a large move
            moved, want = _fresh_smooth_frames(rpt, phase)
            _move(torch_cuda, t, form, moved)
            for m in (0, 1):
                assert np.array_equal(t.mesh_vertices(m).view(np.uint32), moved[m].view(np.uint32))
            _assert_normals(t, (0, 1), "%s, phase %g" % (form, phase))
            got = _frames(rpt, t)
            assert _choice(rpt, t) & SMOOTH_BIT
            _assert_frames(got, want, "%s, phase %g: against a fresh upload" % (form, phase))
            assert not _same(got[0], still_frames[0])
        # a rebuild over the positions the context holds reorders slots and leaves every normal's bytes where they were
        before = [t.mesh_normals(m) for m in (0, 1)]
        assert rpt.lib().rpt_rebuild_meshes(t._h, None, 0) == rpt._abi.RPT_OK
        for m in (0, 1):
            assert np.array_equal(t.mesh_normals(m).view(np.uint32), before[m].view(np.uint32)), m
        _assert_frames(_frames(rpt, t), want, "after rpt_rebuild_meshes(ctx, NULL, 0)")
        # and the modes survive all of it: one mesh back to FLAT after the moves
        t.set_mesh_shading({1: "flat"})
        _assert_normals(t, (0,), "mesh 0 after mesh 1 went FLAT")
    finally:
        t.close()


@pytest.mark.parametrize("form", ["update", "rebuild"])
def test_the_order_of_set_mesh_shading_and_the_first_move_does_not_matter(rpt, torch_cuda, form):
    moved, want = _fresh_smooth_frames(rpt, 2.0)
    t = rpt.Tracer(_small_scene(), device=0, seed=8)
    try:
        _move(torch_cuda, t, form, moved)                             # the context's first move, then the shading
        _all_smooth(t)
        _assert_normals(t, (0, 1), "%s first" % form)
        _assert_frames(_frames(rpt, t), want, "%s, then rpt_set_mesh_shading" % form)
    finally:
        t.close()


# ---- 5. rejections ----------------------------------------------------------------------------------------------------------------
def test_rejected_calls_leave_modes_normals_and_frames(rpt, torch_cuda):
    A, lib = rpt._abi, rpt.lib()
    sizes = dict(sizes=((64, 48, 2),), resident=None)
    t = rpt.Tracer(_small_scene(), device=0, seed=5)
    try:
        flat = _frames(rpt, t, **sizes)
        t.set_mesh_shading({0: "smooth"})
        ref = _frames(rpt, t, **sizes)
        normals = t.mesh_normals(0)
        assert not _same(ref[0], flat[0])

        def items(*pairs):
            arr = (A.rpt_mesh_shading * len(pairs))()
            for it, (m, mode) in zip(arr, pairs):
                it.mesh, it.mode = m, mode
            return arr

        S, FL = A.RPT_MESH_SHADING_SMOOTH, A.RPT_MESH_SHADING_FLAT
        cases = [("NULL items", None, 1, "items is NULL"),
                 ("mesh out of range", items((1, S), (2, S)), 2, "item 1: mesh 2 out of range"),
                 ("named twice", items((1, S), (0, FL), (1, FL)), 3, "item 2: mesh 1 is named twice"),
                 ("a mode that is neither", items((1, S), (0, 2)), 2, "item 1: mode 2"),
                 ("out of range before the mode", items((7, 9)), 1, "item 0: mesh 7 out of range")]
        for what, arr, n, message in cases:
            assert lib.rpt_set_mesh_shading(t._h, arr, n) == A.RPT_ERR_INVALID_ARG, what
            err = lib.rpt_last_error(t._h).decode()
            assert err.startswith("rpt_set_mesh_shading: ") and message in err, (what, err)
            assert np.array_equal(t.mesh_normals(0).view(np.uint32), normals.view(np.uint32)), what
            out = np.zeros((len(t.scene().meshes[1][0]), 3), F)
            assert lib.rpt_download_mesh_normals(t._h, 1, out.ctypes.data, len(out)) == A.RPT_ERR_INVALID_ARG, "%s: mesh 1 is still FLAT" % what
            _assert_frames(_frames(rpt, t, **sizes), ref, what)
        assert lib.rpt_set_mesh_shading(t._h, None, 0) == A.RPT_OK     # nothing to do
        _assert_frames(_frames(rpt, t, **sizes), ref, "n_items == 0")
        # rpt_download_mesh_normals' own answers
        out = np.zeros((len(normals) + 1, 3), F)
        assert lib.rpt_download_mesh_normals(t._h, 0, out.ctypes.data, len(normals) + 1) == A.RPT_ERR_INVALID_ARG
        assert lib.rpt_download_mesh_normals(t._h, 0, None, len(normals)) == A.RPT_ERR_INVALID_ARG
        assert lib.rpt_download_mesh_normals(t._h, 2, out.ctypes.data, 1) == A.RPT_ERR_INVALID_ARG
        # a rejected move leaves the normals as they were
        bad = np.array(t.scene().meshes[0][0], F, copy=True)
        bad[3, 1] = np.nan
        with pytest.raises(Exception):
            t.update_meshes({0: bad})
        with pytest.raises(Exception):
            t.rebuild_meshes({0: bad[:-1]})
        assert np.array_equal(t.mesh_normals(0).view(np.uint32), normals.view(np.uint32))
        _assert_frames(_frames(rpt, t, **sizes), ref, "after rejected moves")
        # an upload leaves every mesh FLAT again
        t.upload_scene()
        _assert_frames(_frames(rpt, t, **sizes), flat, "after rpt_upload_scene")
        assert not _choice(rpt, t) & SMOOTH_BIT
        out = np.zeros((len(normals), 3), F)
        assert lib.rpt_download_mesh_normals(t._h, 0, out.ctypes.data, len(out)) == A.RPT_ERR_INVALID_ARG
        # without a mesh scene
        t._scene = rpt.AnalyticalScene()
        t.upload_scene()
        assert lib.rpt_set_mesh_shading(t._h, items((0, S)), 1) == A.RPT_ERR_NO_SCENE
        assert lib.rpt_set_mesh_shading(t._h, None, 0) == A.RPT_ERR_NO_SCENE       # no scene comes before n_items == 0
        assert lib.rpt_download_mesh_normals(t._h, 0, out.ctypes.data, len(out)) == A.RPT_ERR_NO_SCENE
    finally:
        t.close()


# ---- 6. the product library -------------------------------------------------------------------------------------------------------
CHILD = r'''
import hashlib, json, os, sys
os.environ.pop("RPT_LIB", None)                      # a plain import: the product
import importlib.util
spec = importlib.util.spec_from_file_location("rust_pathtracer_amd", os.path.join(%(root)r, "rust-pathtracer_amd", "__init__.py"),
                                              submodule_search_locations=[os.path.join(%(root)r, "rust-pathtracer_amd")])
rpt = importlib.util.module_from_spec(spec); sys.modules["rust_pathtracer_amd"] = rpt; spec.loader.exec_module(rpt)
from rust_pathtracer_amd import scenes
s = scenes.mesh_scene(subdivisions=2, n_major=16, n_minor=8)
t = rpt.Tracer(s, device=0, seed=4)
t.set_mesh_shading({0: "smooth", 1: "smooth"})
t.update_meshes(dict(enumerate(scenes.mesh_scene_moved(s, 1.0))))
buf = rpt.ColorBuffer(96, 54)
t.render_n(buf, 3)
normals = t.mesh_normals(0)
t.close()
print("RESULT " + json.dumps({"path": rpt._lib.LIB_PATH, "hooks": int(rpt.lib().rpt_build_has_test_hooks()),
                              "frame": hashlib.sha1(buf.image().tobytes()).hexdigest(), "normals": hashlib.sha1(normals.tobytes()).hexdigest()}))
'''


def test_the_product_library_shades_smooth_like_the_test_build(rpt, torch_cuda):
    from rust_pathtracer_amd import scenes
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600,
                       env={k: v for k, v in os.environ.items() if k != "RPT_LIB"})
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert os.path.samefile(got["path"], os.path.join(ROOT, "rust-pathtracer_amd", "librpt_hip.so")) and got["hooks"] == 0
    s = _small_scene()
    t = rpt.Tracer(s, device=0, seed=4)
    try:
        flat = _frames(rpt, t, sizes=((96, 54, 3),), resident=None)[0]
        _all_smooth(t)
        t.update_meshes(dict(enumerate(scenes.mesh_scene_moved(s, 1.0))))
        here = _frames(rpt, t, sizes=((96, 54, 3),), resident=None)[0]
        assert _choice(rpt, t) & SMOOTH_BIT
        normals = t.mesh_normals(0)
    finally:
        t.close()
    assert not _same(here, flat)
    assert got["frame"] == hashlib.sha1(here.tobytes()).hexdigest(), "the product library's smooth frame differs from the test build's"
    assert got["normals"] == hashlib.sha1(normals.tobytes()).hexdigest()
