"""rpt_update_meshes on the GPU (include/rpt.h, "moving meshes"): new vertex positions through a refit of the hierarchy on the device.

Everything is bit for bit, and nothing takes the refit's own output as truth:
* frames after an update equal the frames of a FRESH context that uploads the moved scene (the unchanged upload path), move after
  move, through rpt_render and the resident buffer, also beyond 2^60, across an upload of another scene class, and on a context
  with the device listed twice;
* the walk over the refitted tables equals tests/test_gpu_mesh.py's numpy restatement of the ordered loop over the moved triangles;
* the tables themselves (rpt_debug_mesh_tables) equal a numpy float32 restatement of the rows and of the boxes, bottom-up;
* a rejected update leaves the scene as it was; the product library renders the test build's frame after an update.
Every test asserts through rpt_debug_kernel_choice that the mesh kernel ran (bit 25)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_mesh import _mesh_tris, _query, _rays, _test_scene, brute_force
from test_gpu_mesh_f64 import _scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH_BIT = 1 << 25


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _choice(rpt, t):
    choice = C.c_uint32(0)
    rpt._lib.check(rpt.lib().rpt_debug_kernel_choice(t._h, C.byref(choice)), t._h)
    return choice.value


def _frames(rpt, t, sizes=((96, 54, 5), (64, 48, 1)), resident=(96, 54, 3)):
    """The frames a test compares: through rpt_render at `sizes`, then a resident render after rpt_resident_reset."""
    out = []
    for w, h, spp in sizes:
        buf = rpt.ColorBuffer(w, h)
        t.render_n(buf, spp)
        assert _choice(rpt, t) & MESH_BIT, "the mesh kernel ran"
        out.append(buf.image().copy())
    if resident:
        w, h, spp = resident
        t.resident_reset()
        t.render_resident(w, h, spp)
        assert _choice(rpt, t) & MESH_BIT
        out.append(t.resident_to_host(w, h).image().copy())
    return out


def _assert_frames(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), "%s: frame %d differs in %d values" % (what, k, int((g.view(np.uint32) != w.view(np.uint32)).sum()))


def _with_vertices(make, arrays):
    """A new scene from `make()` with its meshes' vertex arrays replaced by copies of `arrays`."""
    s = make()
    s.meshes = [(np.array(v, np.float32, copy=True), t, m) for v, (_, t, m) in zip(arrays, s.meshes)]
    return s


def _fresh_frames(rpt, make, arrays, seed, **kw):
    """The yardstick: a fresh context that uploads the moved scene."""
    b = rpt.Tracer(_with_vertices(make, arrays), device=0, seed=seed)
    try:
        return _frames(rpt, b, **kw)
    finally:
        b.close()


def _moves(scene):
    """[(what, {mesh: new vertices})] for a scene of scenes.mesh_scene()'s two meshes; each move starts from where the last one ended."""
    from rust_pathtracer_amd import scenes
    v0, v1 = (np.asarray(v, np.float32) for v, _, _ in scene.meshes)
    small, large = scenes.mesh_scene_moved(scene, 0.05), scenes.mesh_scene_moved(scene, 2.0)
    c0, c1 = 0.5 * (v0.min(0) + v0.max(0)), 0.5 * (v1.min(0) + v1.max(0))
    return [("small ripple", {0: small[0], 1: small[1]}),
            ("large ripple and rotation", {0: large[0], 1: large[1]}),
            ("both meshes onto each other", {0: (v0 - c0).astype(np.float32), 1: (v1 - c1).astype(np.float32)}),
            ("one mesh collapsed to a point", {1: np.tile(np.float32([0.3, 0.2, 0.1]), (len(v1), 1))}),
            ("back to the original", {0: v0.copy(), 1: v1.copy()})]


# ---- 1. frames equal a fresh upload's ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_frames_after_an_update_equal_a_fresh_upload(rpt, torch_cuda, which):
    what, _ = _scenes()[which]
    make = lambda: _scenes()[which][1]                                # noqa: E731
    seed = 21 + which
    a = rpt.Tracer(make(), device=0, seed=seed)
    try:
        first = _frames(rpt, a)
        assert all(np.isfinite(f).all() for f in first) and first[0][..., :3].mean() > 0.01
        stats = _mesh_stats(rpt, a)
        moved_frames = []
        for name, updates in _moves(make()):
            a.update_meshes(updates)
            got = _frames(rpt, a)
            want = _fresh_frames(rpt, make, [v for v, _, _ in a.scene().meshes], seed)
            _assert_frames(got, want, "%s, %s" % (what, name))
            assert _mesh_stats(rpt, a) == stats, name                 # the hierarchy kept its shape
            moved_frames.append(got)
        _assert_frames(moved_frames[-1], first, "%s: back to the original" % what)
        for k in range(4):                                            # (the moves do move the picture)
            assert not _same(moved_frames[k][0], first[0]), k
    finally:
        a.close()


def _mesh_stats(rpt, t):
    nodes, depth, ms = C.c_uint32(0), C.c_uint32(0), C.c_float(0.0)
    rpt._lib.check(rpt.lib().rpt_debug_mesh_stats(t._h, C.byref(nodes), C.byref(depth), C.byref(ms)), t._h)
    return nodes.value, depth.value


# ---- 2. the walk against numpy ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_exp", [0, -20, 20])
def test_walks_after_a_large_move_equal_the_ordered_loop(rpt, torch_cuda, scale_exp):
    from rust_pathtracer_amd import scenes
    scale = 2.0 ** scale_exp
    s = _test_scene(scale)
    rng = np.random.default_rng(2000 + scale_exp)
    moved = scenes.mesh_scene_moved(s, 2.0)                           # the icosphere and the torus; then the odd triangles, shaken
    moved[2] = (moved[2] + rng.uniform(-0.3, 0.3, moved[2].shape) * scale).astype(np.float32)
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        before = _mesh_tris(s)
        t.update_meshes(dict(enumerate(moved)))
        tris = _mesh_tris(t.scene())
        assert tris.shape == before.shape and (tris != before).mean() > 0.5
        rays = _rays(tris, 48_000 if scale_exp == 0 else 24_000, rng, scale)
        for use_max in (False, True):
            want = brute_force(tris, rays, use_max)
            flags = rpt._abi.RPT_MESH_QUERY_USE_MAX if use_max else 0
            for brute in (False, True):
                got = _query(rpt, torch_cuda, t, rays, flags | (rpt._abi.RPT_MESH_QUERY_BRUTE if brute else 0))
                for name, g, w in zip(("t bits", "index", "any_hit"), got, want):
                    bad = np.nonzero(g != w)[0]
                    assert len(bad) == 0, "%s (brute %s, use_max %s): %d rays differ, first %s: got %s want %s" % (
                        name, brute, use_max, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])
        assert (want[1] >= 0).mean() > 0.2 and want[2].mean() > 0.05    # the sample does hit things
        buf = rpt.ColorBuffer(32, 24)
        t.render_n(buf, 1)
        assert _choice(rpt, t) & MESH_BIT
    finally:
        t.close()


# ---- 3. the tables ----------------------------------------------------------------------------------------------------------------
def _tables(rpt, t):
    out = []
    for which, stride in ((0, 48), (1, 64)):
        n = C.c_uint64(0)
        assert rpt.lib().rpt_debug_mesh_tables(t._h, which, None, 0, C.byref(n)) == rpt._abi.RPT_ERR_INVALID_ARG      # (asks for the size)
        assert n.value and n.value % stride == 0
        buf = np.zeros(n.value // 4, np.uint32)
        rpt._lib.check(rpt.lib().rpt_debug_mesh_tables(t._h, which, buf.ctypes.data, buf.nbytes, C.byref(n)), t._h)
        out.append(buf.reshape(-1, stride // 4))
    return out


def _min(a, b):
    return np.where(b < a, b, a)                                      # std::min(a, b): a unless b is smaller


def _max(a, b):
    return np.where(a < b, b, a)


def _restate_tables(tris, rows0, nodes0):
    """The two tables for moved triangles `tris` [T, 3, 3] f32 (flattened order), in numpy float32: the shape — slot order, .w words,
    child words — from the uploaded tables `rows0` / `nodes0`; rows {a, b - a, c - a}; a triangle's box from its vertices and
    a + min(0, e1, e2) / a + max(0, e1, e2) (csrc/host_bvh.h, triangle_box); boxes bottom-up over the child words."""
    f32 = np.float32
    order = rows0[:, 3]
    v = tris.astype(f32)[order]                                       # [slot, corner, xyz]
    a, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    rows = rows0.copy()
    rows[:, 0:3], rows[:, 4:7], rows[:, 8:11] = a.view(np.uint32), e1.view(np.uint32), e2.view(np.uint32)
    lo = np.full_like(a, np.inf)
    hi = np.full_like(a, -np.inf)
    for k in range(3):
        lo, hi = _min(lo, v[:, k]), _max(hi, v[:, k])
    lo = _min(lo, a + _min(_min(np.zeros_like(a), e1), e2))
    hi = _max(hi, a + _max(_max(np.zeros_like(a), e1), e2))
    nodes = nodes0.copy()
    boxes = nodes[:, :12].view(f32)                                   # (a view: writes land in `nodes`)
    for i in range(len(nodes) - 1, -1, -1):                           # pre-order: a node's children have larger indices
        for c in range(2):
            ch = int(nodes0[i, 12 + c])
            blo, bhi = np.full(3, np.inf, f32), np.full(3, -np.inf, f32)
            if ch & 0x80000000:
                cnt, first = (ch >> 27) & 15, ch & ((1 << 27) - 1)
                for s in range(first, first + cnt):
                    blo, bhi = _min(blo, lo[s]), _max(bhi, hi[s])
            else:
                assert i < ch < len(nodes)
                for side in (0, 6):
                    blo, bhi = _min(blo, boxes[ch, side:side + 3]), _max(bhi, boxes[ch, side + 3:side + 6])
            boxes[i, 6 * c:6 * c + 3], boxes[i, 6 * c + 3:6 * c + 6] = blo, bhi
    return rows, nodes


def _table_scenes():
    from rust_pathtracer_amd import scenes
    one = scenes.mesh_scene(subdivisions=1, n_major=6, n_minor=4)
    one.meshes = [(np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0.5], [5, 5, 5]]), np.uint32([[2, 0, 1]]), 0)]      # (one unused vertex)
    many = scenes.mesh_scene(subdivisions=2, n_major=12, n_minor=6)
    rng = np.random.default_rng(5)
    nine_v = rng.uniform(-1, 1, (11, 3)).astype(np.float32) + np.float32([0, 1.5, 0])
    nine_t = np.uint32([[k, k + 1, k + 2] for k in range(9)])
    tiny, ulp = np.float32(2.0 ** -126), np.float32(2.0 ** -149)
    sub_v = np.float32([[tiny, -tiny, 0], [tiny + ulp, -tiny, ulp], [tiny, -tiny - 3 * ulp, -ulp], [0.5, 0.5, 0.5], [0.5 + 2.0 ** -24, 0.5, 0.5]])
    sub_t = np.uint32([[0, 1, 2], [0, 3, 4], [2, 1, 3]])
    many.meshes += [(nine_v, nine_t, 1), (sub_v, sub_t, 0)]
    return [("one triangle", one), ("icosphere, torus, nine triangles, subnormal edges", many)]


@pytest.mark.parametrize("which", [0, 1])
def test_tables_after_an_update_equal_the_restatement(rpt, torch_cuda, which):
    what, s = _table_scenes()[which]
    original = [np.array(v, np.float32, copy=True) for v, _, _ in s.meshes]
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        rows0, nodes0 = _tables(rpt, t)
        stats = _mesh_stats(rpt, t)
        assert stats[0] == len(nodes0) and len(rows0) == len(_mesh_tris(s))
        if which == 0:
            assert len(nodes0) == 1 and nodes0[0, 13] == 0x80000000, "a root with an empty child"
        # the restatement itself reproduces the upload's tables (so a mismatch below is the refit's)
        r, n = _restate_tables(_mesh_tris(s), rows0, nodes0)
        assert np.array_equal(r, rows0) and np.array_equal(n, nodes0), what
        # the uploaded vertices once more: nothing changes
        t.update_meshes(dict(enumerate(original)))
        rows, nodes = _tables(rpt, t)
        assert np.array_equal(rows, rows0) and np.array_equal(nodes, nodes0), what
        # a move: the numpy restatement, byte for byte
        rng = np.random.default_rng(77 + which)
        moved = [(v * np.float32(1.5) + rng.uniform(-0.4, 0.4, v.shape)).astype(np.float32) for v in original]
        if which == 1:                                                # the subnormal mesh moves by subnormal amounts: its edges stay subnormal
            ulp = np.float32(2.0 ** -149)
            moved[3] = original[3].copy()
            moved[3][:3] += np.float32([[2, 0, -1], [0, 5, 0], [-3, 1, 1]]) * ulp
        t.update_meshes(dict(enumerate(moved)))
        tris = _mesh_tris(t.scene())
        want_rows, want_nodes = _restate_tables(tris, rows0, nodes0)
        rows, nodes = _tables(rpt, t)
        assert np.array_equal(rows[:, [3, 7, 11]], rows0[:, [3, 7, 11]]) and np.array_equal(nodes[:, 12:], nodes0[:, 12:]), "the shape moved"
        assert np.array_equal(rows, want_rows), "%s: %d row words differ" % (what, int((rows != want_rows).sum()))
        assert np.array_equal(nodes, want_nodes), "%s: %d node words differ" % (what, int((nodes != want_nodes).sum()))
        assert not np.array_equal(rows, rows0) and not np.array_equal(nodes, nodes0)
        if which == 1:
            e = np.abs(rows[:, [4, 5, 6, 8, 9, 10]].view(np.float32))
            assert ((e > 0) & (e < np.float32(2.0 ** -126))).sum() >= 4, "subnormal edge components are kept"
        if which == 0:
            assert np.array_equal(nodes[0, 6:12].view(np.float32), np.float32([np.inf] * 3 + [-np.inf] * 3)), "the empty child's box"
        assert _mesh_stats(rpt, t) == stats
        # and back: the upload's bytes
        t.update_meshes(dict(enumerate(original)))
        rows, nodes = _tables(rpt, t)
        assert np.array_equal(rows, rows0) and np.array_equal(nodes, nodes0), what
        assert _mesh_stats(rpt, t) == stats
        buf = rpt.ColorBuffer(32, 24)
        t.render_n(buf, 1)
        assert _choice(rpt, t) & MESH_BIT
    finally:
        t.close()


# ---- 4. rejected updates leave the scene ------------------------------------------------------------------------------------------
def _small_scene():
    from rust_pathtracer_amd import scenes
    return scenes.mesh_scene(subdivisions=2, n_major=16, n_minor=8)


def test_rejected_updates_leave_the_scene(rpt, torch_cuda):
    from rust_pathtracer_amd import scenes
    A, lib = rpt._abi, rpt.lib()
    sizes = dict(sizes=((64, 48, 2),), resident=None)
    t = rpt.Tracer(_small_scene(), device=0, seed=5)
    try:
        ref = _frames(rpt, t, **sizes)
        v0, v1 = (np.array(v, np.float32, copy=True) for v, _, _ in t.scene().meshes)
        ptr = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))        # noqa: E731

        def ups(*items):
            arr = (A.rpt_mesh_vertices * len(items))()
            for u, (m, n, p) in zip(arr, items):
                u.mesh, u.n_vertices, u.vertices = m, n, p
            return arr

        nan, pinf, ninf = v1.copy(), v1.copy(), v0.copy()
        nan[7, 1], pinf[0, 0], ninf[len(v0) - 1, 2] = np.nan, np.inf, -np.inf
        cases = [("NULL updates", None, 1, "updates is NULL"),
                 ("mesh out of range", ups((2, len(v0), ptr(v0))), 1, "mesh 2 out of range"),
                 ("named twice", ups((1, len(v1), ptr(v1)), (1, len(v1), ptr(v1))), 2, "mesh 1 is named twice"),
                 ("one vertex short", ups((0, len(v0) - 1, ptr(v0))), 1, "mesh 0: n_vertices"),
                 ("no vertices", ups((0, 0, None)), 1, "mesh 0: n_vertices"),
                 ("NULL vertices", ups((1, len(v1), None)), 1, "mesh 1: vertices is NULL"),
                 ("NaN", ups((1, len(v1), ptr(nan))), 1, "mesh 1 vertex 7 is not finite"),
                 ("+inf", ups((0, len(v0), ptr(v0)), (1, len(v1), ptr(pinf))), 2, "mesh 1 vertex 0 is not finite"),
                 ("-inf", ups((0, len(v0), ptr(ninf))), 1, "mesh 0 vertex %d is not finite" % (len(v0) - 1))]
        for what, arr, n, message in cases:
            assert lib.rpt_update_meshes(t._h, arr, n) == A.RPT_ERR_INVALID_ARG, what
            assert message.encode() in lib.rpt_last_error(t._h), (what, lib.rpt_last_error(t._h))
            _assert_frames(_frames(rpt, t, **sizes), ref, what)
        assert lib.rpt_update_meshes(t._h, None, 0) == A.RPT_OK        # nothing to do
        _assert_frames(_frames(rpt, t, **sizes), ref, "no updates")
        # ... and a valid one is accepted after them
        moved = scenes.mesh_scene_moved(t.scene(), 0.5)
        t.update_meshes({1: moved[1]})
        got = _frames(rpt, t, **sizes)
        assert not _same(got[0], ref[0])
        _assert_frames(got, _fresh_frames(rpt, _small_scene, [v0, moved[1]], 5, **sizes), "a valid update after the rejected ones")
        assert lib.rpt_update_meshes(None, ups((0, len(v0), ptr(v0))), 1) == A.RPT_ERR_INVALID_ARG
    finally:
        t.close()
    # no mesh scene: a fresh context, and the other scene classes
    one = ups((0, len(v0), ptr(v0)))
    h = C.c_void_p()
    rpt._lib.check(lib.rpt_create(C.byref(h), 0))
    assert lib.rpt_update_meshes(h, one, 1) == A.RPT_ERR_NO_SCENE and b"scene with meshes" in lib.rpt_last_error(h)
    lib.rpt_destroy(h)
    empty = _small_scene()
    empty.meshes = [(v0, np.zeros((0, 3), np.uint32), 0)]            # meshes without a triangle: not a mesh scene
    for what, s in (("analytical", rpt.AnalyticalScene()), ("large", scenes.random_spheres_scene(300, 5)), ("sdf", scenes.sdf_scene()),
                    ("meshes without triangles", empty)):
        o = rpt.Tracer(s, device=0, seed=5)
        buf = rpt.ColorBuffer(48, 32)
        o.render_n(buf, 1)
        before = buf.image().copy()
        assert lib.rpt_update_meshes(o._h, one, 1) == A.RPT_ERR_NO_SCENE, what
        buf = rpt.ColorBuffer(48, 32)
        o.render_n(buf, 1)
        assert _same(buf.image(), before), what
        o.close()


# ---- 5. beyond 2^60 ---------------------------------------------------------------------------------------------------------------
def test_a_vertex_beyond_2_60_and_back(rpt, torch_cuda):
    from rust_pathtracer_amd import scenes
    make = lambda: scenes.mesh_scene(subdivisions=1, n_major=6, n_minor=4)      # noqa: E731  (128 triangles: the loop serves every ray)
    sizes = dict(sizes=((64, 48, 2),), resident=(48, 32, 1))
    t = rpt.Tracer(make(), device=0, seed=9)
    try:
        first = _frames(rpt, t, **sizes)
        v0, v1 = (np.array(v, np.float32, copy=True) for v, _, _ in t.scene().meshes)
        far = v1.copy()
        far[5, 0] = np.float32(2.0 ** 61)
        t.update_meshes({1: far})
        got = _frames(rpt, t, **sizes)
        _assert_frames(got, _fresh_frames(rpt, make, [v0, far], 9, **sizes), "a vertex at 2^61")
        assert not _same(got[0], first[0])
        t.update_meshes({0: v0})                                      # another mesh's update does not bring the walk back; the frame stays
        _assert_frames(_frames(rpt, t, **sizes), got, "2^61, the other mesh updated")
        t.update_meshes({1: v1})
        _assert_frames(_frames(rpt, t, **sizes), first, "back from 2^61")
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, [v0, v1], 9, **sizes), "back from 2^61, fresh")
    finally:
        t.close()


# ---- 6. context life --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_updates_across_uploads_on_one_context(rpt, torch_cuda, oracle, devices):
    from rust_pathtracer_amd import scenes
    make = _small_scene
    seed = 13
    sizes = dict(sizes=((96, 54, 5), (64, 48, 1)), resident=(96, 54, 3))
    t = rpt.Tracer(make(), seed=seed, **(dict(devices=devices) if devices else dict(device=0)))
    try:
        m1 = scenes.mesh_scene_moved(make(), 0.7)
        t.update_meshes(dict(enumerate(m1)))
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, m1, seed, **sizes), "first update")
        mesh_scene = t.scene()
        t._scene = rpt.AnalyticalScene()
        t.upload_scene()
        assert rpt.lib().rpt_update_meshes(t._h, (rpt._abi.rpt_mesh_vertices * 1)(), 1) == rpt._abi.RPT_ERR_NO_SCENE
        buf = rpt.ColorBuffer(64, 48)
        t.render_n(buf, 2)
        want = oracle.render(oracle.scene_analytical(), 64, 48, 2, seed=seed)
        assert _same(buf.image(), want), "the analytical scene between two mesh scenes"
        t._scene = mesh_scene                                         # the moved scene, uploaded (update_meshes replaced its arrays)
        t.upload_scene()
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, m1, seed, **sizes), "the moved scene uploaded again")
        m2 = scenes.mesh_scene_moved(make(), 2.0)
        t.update_meshes({0: m2[0]})
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, [m2[0], m1[1]], seed, **sizes), "second update")
        t.update_meshes({1: m2[1]})
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, m2, seed, **sizes), "third update")
    finally:
        t.close()


# ---- 7. the product library -------------------------------------------------------------------------------------------------------
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
t.update_meshes(dict(enumerate(scenes.mesh_scene_moved(s, 1.0))))
buf = rpt.ColorBuffer(96, 54)
t.render_n(buf, 3)
t.close()
print("RESULT " + json.dumps({"path": rpt._lib.LIB_PATH, "hooks": int(rpt.lib().rpt_build_has_test_hooks()),
                              "frame": hashlib.sha1(buf.image().tobytes()).hexdigest()}))
'''


def test_the_product_library_updates_like_the_test_build(rpt, torch_cuda):
    from rust_pathtracer_amd import scenes
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600,
                       env={k: v for k, v in os.environ.items() if k != "RPT_LIB"})
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert os.path.samefile(got["path"], os.path.join(ROOT, "rust-pathtracer_amd", "librpt_hip.so")) and got["hooks"] == 0
    s = _small_scene()
    moved = scenes.mesh_scene_moved(s, 1.0)
    t = rpt.Tracer(s, device=0, seed=4)
    try:
        t.update_meshes(dict(enumerate(moved)))
        here = _frames(rpt, t, sizes=((96, 54, 3),), resident=None)[0]
    finally:
        t.close()
    assert got["frame"] == hashlib.sha1(here.tobytes()).hexdigest(), "the product library's frame differs from the test build's"
    _assert_frames([here], _fresh_frames(rpt, _small_scene, moved, 4, sizes=((96, 54, 3),), resident=None), "against a fresh upload")
