"""rpt_update_meshes_device / rpt_rebuild_meshes_device / rpt_download_mesh_vertices on the GPU (include/rpt.h, "moving meshes from
device memory"): new positions read from device memory, through an optional per-mesh transform applied on the device.

Everything is bit for bit, and nothing takes the calls' own output as truth:
* the positions the context holds afterwards equal a numpy float32 restatement of the transform (tests/test_mesh_move_host.py);
* frames equal the frames of a FRESH context that uploads those numpy positions (the unchanged upload path), on one device and with
  the device listed twice, for both forms;
* the triangle and node tables equal, byte for byte, those of a second context given the same positions through the HOST forms;
* a rejected call — by a host check, or by the device check — leaves frames, tables and positions as they were;
* the source may come from another stream without the test synchronising, and may be overwritten as soon as the call returns.
The suite never hands the calls a pageable host pointer or a freed one: the not-device-memory case uses a page-locked tensor, which
a kernel could read, so nothing can fault even if the validation were missing.
Every frame comparison asserts through rpt_debug_kernel_choice that the mesh kernel ran (bit 25)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_mesh_update import (_assert_frames, _frames, _fresh_frames, _mesh_stats, _same, _small_scene, _table_scenes, _tables)
from test_mesh_move_host import IDENTITY, restate_move, transforms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FORMS = ("update", "rebuild")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _dev(torch, a):
    """A CUDA copy of `a` that the default stream has finished writing."""
    t = torch.from_numpy(np.ascontiguousarray(a, F).reshape(-1, 3).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _move(t, form, sources):
    (t.update_meshes_device if form == "update" else t.rebuild_meshes_device)(sources)


def _move_host(t, form, updates):
    (t.update_meshes if form == "update" else t.rebuild_meshes)(updates)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _arrays(t):
    return [np.array(v, F, copy=True).reshape(-1, 3) for v, _, _ in t.scene().meshes]


def _held(t):
    return [t.mesh_vertices(m) for m in range(len(t.scene().meshes))]


def _assert_positions(got, want, what):
    assert len(got) == len(want)
    for m, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), "%s: mesh %d: %d words differ" % (what, m, int((_bits(g) != _bits(w)).sum()))


def _translation(d):
    t = IDENTITY.copy()
    t[[3, 7, 11]] = d
    return t


def _walk(rpt, t):
    n = C.c_uint32(99)
    rpt._lib.check(rpt.lib().rpt_debug_mesh_walk(t._h, C.byref(n)), t._h)
    return n.value


# ---- 1. positions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_positions_equal_the_numpy_restatement(rpt, torch_cuda, form):
    what, s = _table_scenes()[1]                                      # four meshes, subnormal coordinates among them
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        cur = _arrays(t)
        _assert_positions(_held(t), cur, "before any update (the host's copy of the upload)")
        src = [v.copy() for v in cur]
        src[0][0] = [-0.0, 0.0, -0.0]                                 # zeros of both signs in the source
        src[2][3] = [0.0, -0.0, 1.0]
        dev = [_dev(torch_cuda, v) for v in src]
        for name, xf in transforms()[:4]:                             # (the fifth overflows: test_rejected_calls_leave_the_scene)
            named = (0, 2, 3) if name != "identity" else (0, 2)
            _move(t, form, {m: (dev[m], xf) if xf is not None else dev[m] for m in named})
            for m in named:
                cur[m] = restate_move(src[m], xf)
            _assert_positions(_held(t), cur, "%s, %s (mesh 1 is not named: unchanged)" % (form, name))
            if name == "NULL":
                assert _bits(cur[0])[0, 0] == 0x80000000 and _bits(t.mesh_vertices(0))[0, 0] == 0x80000000, "-0 is kept without a transform"
            if name == "identity":
                assert list(_bits(t.mesh_vertices(0))[0]) == [0, 0, 0] and list(_bits(t.mesh_vertices(2))[3]) == [0, 0, 0x3F800000], "an identity loses it"
        assert np.array_equal(_bits(cur[1]), _bits(_arrays(t)[1]))
        # a pair (tensor, None) is a tensor alone; a mesh may be moved by 12 floats of any shape
        _move(t, form, {1: (dev[1], None), 3: (dev[3], np.float64(transforms()[2][1]).reshape(3, 4).tolist())})
        cur[1], cur[3] = src[1], restate_move(src[3], transforms()[2][1])
        _assert_positions(_held(t), cur, "%s, second round" % form)
        buf = rpt.ColorBuffer(32, 24)
        t.render_n(buf, 1)
    finally:
        t.close()


# ---- 2. frames equal a fresh upload's ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("form", FORMS)
def test_frames_equal_a_fresh_upload_of_the_numpy_positions(rpt, torch_cuda, form, devices):
    from rust_pathtracer_amd import scenes
    make, seed = _small_scene, 31
    t = rpt.Tracer(make(), seed=seed, **(dict(devices=devices) if devices else dict(device=0)))
    try:
        first = _frames(rpt, t)
        v0, v1 = _arrays(t)
        # moved positions, no transform
        moved = scenes.mesh_scene_moved(make(), 0.7)
        _move(t, form, {m: _dev(torch_cuda, v) for m, v in enumerate(moved)})
        got = _frames(rpt, t)
        _assert_frames(got, _fresh_frames(rpt, make, moved, seed), "%s: moved positions" % form)
        assert not _same(got[0], first[0])
        _assert_positions(_held(t), [np.asarray(v, F) for v in moved], "moved positions")
        # a rigid move of the torus from ONE rest tensor, three frames running: nothing drifts
        rest = _dev(torch_cuda, v1)
        frames = []
        for k, angle in enumerate((0.3, 0.9, 2.1)):
            c, s = np.cos(angle), np.sin(angle)
            xf = F([c, -s, 0, 0.1 * k, s, c, 0, -0.05 * k, 0, 0, 1, 0.2])
            _move(t, form, {1: (rest, xf)})
            frames.append(_frames(rpt, t))
            _assert_frames(frames[-1], _fresh_frames(rpt, make, [moved[0], restate_move(v1, xf)], seed), "%s: rigid move %d of the rest pose" % (form, k))
        assert not _same(frames[0][0], frames[2][0])
        assert np.array_equal(rest.cpu().numpy(), v1), "the rest tensor is read, never written"
        # both meshes onto each other, each by a translation
        c0, c1 = 0.5 * (v0.min(0) + v0.max(0)), 0.5 * (v1.min(0) + v1.max(0))
        _move(t, form, {0: (_dev(torch_cuda, v0), _translation(-c0)), 1: (rest, _translation(-c1))})
        want = [restate_move(v0, _translation(-c0)), restate_move(v1, _translation(-c1))]
        _assert_frames(_frames(rpt, t), _fresh_frames(rpt, make, want, seed), "%s: both meshes onto each other" % form)
    finally:
        t.close()


# ---- 3. the tables equal the host form's -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("form", FORMS)
def test_tables_equal_the_host_forms(rpt, torch_cuda, form, which):
    what, _ = _table_scenes()[which]
    a = rpt.Tracer(_table_scenes()[which][1], device=0, seed=1)
    b = rpt.Tracer(_table_scenes()[which][1], device=0, seed=1)
    try:
        rows0, nodes0 = _tables(rpt, a)
        src = _arrays(a)
        rng = np.random.default_rng(40 + which)
        for step, (name, xf) in enumerate(transforms()[:4]):
            shaken = [(v + rng.uniform(-0.2, 0.2, v.shape)).astype(F) for v in src]
            _move(a, form, {m: (_dev(torch_cuda, v), xf) for m, v in enumerate(shaken)})
            want = [restate_move(v, xf) for v in shaken]
            _move_host(b, form, dict(enumerate(want)))
            (ra, na), (rb, nb) = _tables(rpt, a), _tables(rpt, b)
            assert np.array_equal(ra, rb), "%s, %s, %s: %d row words differ from the host form's" % (what, form, name, int((ra != rb).sum()))
            assert np.array_equal(na, nb), "%s, %s, %s: %d node words differ from the host form's" % (what, form, name, int((na != nb).sum()))
            assert _mesh_stats(rpt, a) == _mesh_stats(rpt, b)
            assert not np.array_equal(ra, rows0)
            _assert_positions(_held(a), want, name)
            _assert_positions(_held(b), want, name + " (the host form's context)")
        if form == "update":
            assert np.array_equal(na[:, 12:], nodes0[:, 12:]), "an update keeps the shape"
    finally:
        a.close()
        b.close()


# ---- 4. rejected calls leave the scene --------------------------------------------------------------------------------------------
def _scene_with_an_unused_vertex():
    """_small_scene() with one more vertex in front of the torus's, which no triangle uses."""
    s = _small_scene()
    v, idx, mat = s.meshes[1]
    s.meshes[1] = (np.vstack([F([[9, 9, 9]]), np.asarray(v, F)]), np.asarray(idx, np.uint32) + np.uint32(1), mat)
    return s


def _sources(A, *items):
    """(array of rpt_mesh_source, what it points to) for items (mesh, n_vertices, device pointer or None, transform or None)"""
    arr, keep = (A.rpt_mesh_source * max(1, len(items)))(), []
    for s, (m, n, p, xf) in zip(arr, items):
        s.mesh, s.n_vertices, s.vertices_dev = m, n, p
        if xf is not None:
            xf = np.ascontiguousarray(xf, F)
            s.transform = xf.ctypes.data_as(C.POINTER(C.c_float))
            keep.append(xf)
    return arr, keep


@pytest.mark.parametrize("form", FORMS)
def test_rejected_calls_leave_the_scene(rpt, torch_cuda, form):
    torch = torch_cuda
    A, lib = rpt._abi, rpt.lib()
    call = lib.rpt_update_meshes_device if form == "update" else lib.rpt_rebuild_meshes_device
    name = ("rpt_%s_meshes_device: " % form).encode()
    sizes = dict(sizes=((64, 48, 2),), resident=None)
    t = rpt.Tracer(_scene_with_an_unused_vertex(), device=0, seed=5)
    try:
        v0, v1 = _arrays(t)
        n0, n1 = len(v0), len(v1)
        d0, d1 = _dev(torch, v0), _dev(torch, v1)
        nan_inf, inf, big = v1.copy(), v1.copy(), v0.copy()
        nan_inf[0, 1], nan_inf[7, 0] = np.nan, np.inf                 # the NaN at the vertex no triangle uses, below the infinity
        inf[7, 2] = -np.inf
        big[11, 0] = F(2.0 ** 30)                                     # finite here, 2^130 through the transform
        d_nan_inf, d_inf, d_big = _dev(torch, nan_inf), _dev(torch, inf), _dev(torch, big)
        pinned = torch.from_numpy(v1.copy()).pin_memory()             # page-locked HOST memory: readable by a kernel, and still refused
        assert pinned.is_pinned() and not pinned.is_cuda
        bad_t, inf_t = IDENTITY.copy(), IDENTITY.copy()
        bad_t[5], inf_t[11] = np.nan, np.inf
        p = lambda x: x.data_ptr()                                    # noqa: E731
        INV = A.RPT_ERR_INVALID_ARG
        cases = [("NULL sources", (None, []), 1, INV, b"sources is NULL"),
                 ("mesh out of range", _sources(A, (2, n0, p(d0), None)), 1, INV, b"mesh 2 out of range"),
                 ("named twice", _sources(A, (1, n1, p(d1), None), (1, n1, p(d1), None)), 2, INV, b"mesh 1 is named twice"),
                 ("one vertex short", _sources(A, (0, n0 - 1, p(d0), None)), 1, INV, b"mesh 0: n_vertices"),
                 ("no vertices", _sources(A, (0, 0, None, None)), 1, INV, b"mesh 0: n_vertices"),
                 ("NULL vertices_dev", _sources(A, (1, n1, None, None)), 1, INV, b"mesh 1: vertices_dev is NULL"),
                 ("page-locked host memory", _sources(A, (0, n0, p(d0), None), (1, n1, p(pinned), None)), 2, INV, b"mesh 1: vertices_dev is not device memory"),
                 ("NaN in the transform", _sources(A, (1, n1, p(d1), bad_t)), 1, INV, b"mesh 1: transform entry 5 is not finite"),
                 ("infinity in the transform", _sources(A, (0, n0, p(d0), inf_t)), 1, INV, b"mesh 0: transform entry 11 is not finite"),
                 ("NaN below an infinity, at an unused vertex", _sources(A, (0, n0, p(d0), None), (1, n1, p(d_nan_inf), None)), 2, INV, b"mesh 1 vertex 0 is not finite"),
                 ("the same through an identity", _sources(A, (1, n1, p(d_nan_inf), IDENTITY)), 1, INV, b"mesh 1 vertex 0 is not finite"),
                 ("-inf", _sources(A, (1, n1, p(d_inf), _translation(F([1, 2, 3])))), 1, INV, b"mesh 1 vertex 7 is not finite"),
                 ("overflow through the transform", _sources(A, (0, n0, p(d_big), transforms()[4][1]), (1, n1, p(d1), None)), 2, INV, b"mesh 0 vertex 11 is not finite")]
        assert np.isfinite(restate_move(big, transforms()[4][1])).sum() == big.size - 1, "one coordinate overflows, and only one"
        moved = [(v0 * F(1.1)).astype(F), (v1 + F(0.15)).astype(F)]
        for phase in ("before any update", "after a device-source call", "after a host update"):
            if phase == "after a device-source call":
                _move(t, form, {0: _dev(torch, moved[0]), 1: (d1, _translation(F([0.15, 0.15, 0.15])))})
                _assert_positions(_held(t), moved, phase)
            if phase == "after a host update":
                moved = [v0, (v1 - F(0.1)).astype(F)]
                t.update_meshes(dict(enumerate(moved)))
            ref, tables, held, stats = _frames(rpt, t, **sizes), _tables(rpt, t), _held(t), _mesh_stats(rpt, t)
            for what, (arr, _keep), n, status, message in cases:
                assert call(t._h, arr, n) == status, (phase, what, lib.rpt_last_error(t._h))
                err = lib.rpt_last_error(t._h)
                assert err.startswith(name) and message in err, (phase, what, err)
                _assert_frames(_frames(rpt, t, **sizes), ref, "%s, %s" % (phase, what))
                now = _tables(rpt, t)
                assert np.array_equal(now[0], tables[0]) and np.array_equal(now[1], tables[1]), (phase, what)
                _assert_positions(_held(t), held, "%s, %s" % (phase, what))
                assert _mesh_stats(rpt, t) == stats and _walk(rpt, t) == 1
            assert lib.rpt_update_meshes_device(t._h, None, 0) == A.RPT_OK      # nothing to do
            _assert_positions(_held(t), held, phase + ", no sources")
        # a rebuild over the positions the context holds sees the old ones
        assert lib.rpt_rebuild_meshes_device(t._h, None, 0) == A.RPT_OK
        _assert_positions(_held(t), moved, "rebuilt in place")
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, _scene_with_an_unused_vertex, moved, 5, **sizes), "rebuilt in place after the rejections")
        # ... and a valid call is accepted after them
        _move(t, form, {1: (d1, None)})
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, _scene_with_an_unused_vertex, [moved[0], v1], 5, **sizes), "a valid call after the rejected ones")
        # the download's own checks
        out = np.zeros((n1, 3), F)
        assert lib.rpt_download_mesh_vertices(t._h, 2, out.ctypes.data, n1) == INV and b"mesh 2 out of range" in lib.rpt_last_error(t._h)
        assert lib.rpt_download_mesh_vertices(t._h, 1, out.ctypes.data, n1 - 1) == INV and b"n_vertices" in lib.rpt_last_error(t._h)
        assert lib.rpt_download_mesh_vertices(t._h, 1, None, n1) == INV
        assert lib.rpt_download_mesh_vertices(t._h, 1, out.ctypes.data, n1) == A.RPT_OK and np.array_equal(_bits(out), _bits(v1))
    finally:
        t.close()
    # no mesh scene: a fresh context, and another scene class
    one, _keep = _sources(A, (0, n0, p(d0), None))
    h = C.c_void_p()
    rpt._lib.check(lib.rpt_create(C.byref(h), 0))
    assert call(h, one, 1) == A.RPT_ERR_NO_SCENE and b"scene with meshes" in lib.rpt_last_error(h)
    assert lib.rpt_download_mesh_vertices(h, 0, out.ctypes.data, n1) == A.RPT_ERR_NO_SCENE
    assert lib.rpt_rebuild_meshes_device(h, None, 0) == A.RPT_ERR_NO_SCENE and lib.rpt_last_error(h).startswith(b"rpt_rebuild_meshes_device: ")
    lib.rpt_destroy(h)
    o = rpt.Tracer(rpt.AnalyticalScene(), device=0, seed=5)
    buf = rpt.ColorBuffer(48, 32)
    o.render_n(buf, 1)
    before = buf.image().copy()
    assert call(o._h, one, 1) == A.RPT_ERR_NO_SCENE
    buf = rpt.ColorBuffer(48, 32)
    o.render_n(buf, 1)
    assert _same(buf.image(), before)
    o.close()


# ---- 5. beyond 2^60 and back, through the transform -------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_a_translation_beyond_2_60_and_back(rpt, torch_cuda, form):
    from rust_pathtracer_amd import scenes
    make = lambda: scenes.mesh_scene(subdivisions=1, n_major=6, n_minor=4)      # noqa: E731  (128 triangles: the loop serves every ray)
    sizes = dict(sizes=((64, 48, 2),), resident=(48, 32, 1))
    t = rpt.Tracer(make(), device=0, seed=9)
    try:
        first = _frames(rpt, t, **sizes)
        assert _walk(rpt, t) == 1
        v0, v1 = _arrays(t)
        rest = _dev(torch_cuda, v1)
        far = _translation(F([2.0 ** 61, 0, 0]))
        _move(t, form, {1: (rest, far)})
        want = restate_move(v1, far)
        assert np.isfinite(want).all() and np.abs(want).max() >= 2.0 ** 60
        assert _walk(rpt, t) == 0, "a coordinate beyond 2^60: the ordered loop serves the rays"
        got = _frames(rpt, t, **sizes)
        _assert_frames(got, _fresh_frames(rpt, make, [v0, want], 9, **sizes), "%s: the torus at 2^61" % form)
        assert not _same(got[0], first[0])
        _assert_positions(_held(t), [v0, want], "at 2^61")
        _move(t, form, {0: _dev(torch_cuda, v0)})                     # the other mesh: the loop still serves
        assert _walk(rpt, t) == 0
        _assert_frames(_frames(rpt, t, **sizes), got, "2^61, the other mesh moved")
        _move(t, form, {1: rest})                                     # back, word for word
        assert _walk(rpt, t) == 1, "back below 2^60: the walk is on again"
        _assert_frames(_frames(rpt, t, **sizes), first, "%s: back from 2^61" % form)
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, [v0, v1], 9, **sizes), "back from 2^61, fresh")
    finally:
        t.close()


# ---- 5b. many workgroups: the grid's stride, the tail guard, every wave's part of the reduction, the atomics across workgroups ------
def _larger_scene():
    """2 562 and 1 152 vertices: 11 workgroups with a tail of 2 threads, 5 with a tail of 128 (two waves)."""
    from rust_pathtracer_amd import scenes
    return scenes.mesh_scene(subdivisions=4, n_major=48, n_minor=24)


@pytest.mark.parametrize("form", FORMS)
def test_meshes_of_many_workgroups(rpt, torch_cuda, form):
    torch = torch_cuda
    A, lib = rpt._abi, rpt.lib()
    call = lib.rpt_update_meshes_device if form == "update" else lib.rpt_rebuild_meshes_device
    sizes = dict(sizes=((64, 48, 2),), resident=None)
    t = rpt.Tracer(_larger_scene(), device=0, seed=23)
    try:
        v0, v1 = _arrays(t)
        assert (len(v0), len(v1)) == (2562, 1152) and len(v0) % 256 and len(v1) % 256
        # positions, word for word, for every transform that is accepted; frames for the last
        rng = np.random.default_rng(8)
        for name, xf in transforms()[:4]:
            src = [(v + rng.uniform(-0.05, 0.05, v.shape)).astype(F) for v in (v0, v1)]
            _move(t, form, {m: (_dev(torch, v), xf) for m, v in enumerate(src)})
            want = [restate_move(v, xf) for v in src]
            _assert_positions(_held(t), want, "%s, %s" % (form, name))
        xf = transforms()[2][1]
        _move(t, form, {0: (_dev(torch, v0), xf), 1: (_dev(torch, v1), xf)})
        cur = [restate_move(v0, xf), restate_move(v1, xf)]
        _assert_positions(_held(t), cur, "%s, the rotation" % form)
        ref = _frames(rpt, t, **sizes)
        _assert_frames(ref, _fresh_frames(rpt, _larger_scene, cur, 23, **sizes), "%s: 2 562 + 1 152 vertices" % form)
        # the lowest vertex that is not finite, wherever the workgroups and waves that saw the others ran
        planted = [(1, {1030: np.nan, 1100: np.inf}, 1030, "the last workgroup's tail: wave 0 before wave 1"),
                   (1, {1100: np.nan, 1030: -np.inf, 1151: np.nan}, 1030, "the same, the other way round, and the very last vertex"),
                   (1, {700: np.nan, 900: np.inf, 1151: np.inf}, 700, "wave 2 of workgroup 2 before workgroups 3 and 4"),
                   (1, {255: np.inf, 256: np.nan}, 255, "the last thread of workgroup 0 before the first of workgroup 1"),
                   (0, {2561: np.nan}, 2561, "the last of two threads in the eleventh workgroup"),
                   (0, {2560: np.inf, 2561: np.nan, 2000: np.nan}, 2000, "wave 3 of workgroup 7 before the tail"),
                   (0, {191: np.nan, 2561: np.inf}, 191, "wave 2 of workgroup 0 before the tail")]
        tables = _tables(rpt, t)
        for m, plant, lowest, what in planted:
            bad = [v0.copy(), v1.copy()]
            for v, x in plant.items():
                bad[m][v, v % 3] = x
            for xform in (None, IDENTITY):
                d = [_dev(torch, v) for v in bad]
                arr, _keep = _sources(A, (0, len(v0), d[0].data_ptr(), xform), (1, len(v1), d[1].data_ptr(), xform))
                assert call(t._h, arr, 2) == A.RPT_ERR_INVALID_ARG, what
                assert ("mesh %d vertex %d is not finite" % (m, lowest)).encode() in lib.rpt_last_error(t._h), (what, lib.rpt_last_error(t._h))
                _assert_positions(_held(t), cur, what)
        now = _tables(rpt, t)
        assert np.array_equal(now[0], tables[0]) and np.array_equal(now[1], tables[1])
        _assert_frames(_frames(rpt, t, **sizes), ref, "after the rejections")
        # a coordinate beyond 2^60 that only one late thread sees
        assert _walk(rpt, t) == 1
        for m, vertex, what in ((0, 2561, "the tail of the eleventh workgroup"), (1, 1000, "wave 3 of workgroup 3"), (1, 1151, "the last vertex")):
            far = [v0.copy(), v1.copy()]
            far[m][vertex, 1] = F(-(2.0 ** 61))
            _move(t, form, {0: _dev(torch, far[0]), 1: _dev(torch, far[1])})
            assert _walk(rpt, t) == 0, what
            _assert_positions(_held(t), far, what)
            _move(t, form, {m: _dev(torch, (v0, v1)[m])})
            assert _walk(rpt, t) == 1, what + ", back"
        _assert_positions(_held(t), [v0, v1], "back")
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, _larger_scene, [v0, v1], 23, **sizes), "%s: back at the uploaded positions" % form)
    finally:
        t.close()


# ---- 5c. the 2^60 rule looks at referenced vertices only, mesh by mesh --------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_an_unreferenced_vertex_beyond_2_60_keeps_the_walk(rpt, torch_cuda, form):
    """Mesh 1's vertex 0 is used by no triangle while every vertex of mesh 0 is used: a `referenced` table read without the mesh's
    offset, or one that never reached the device, answers differently."""
    make = _scene_with_an_unused_vertex
    sizes = dict(sizes=((64, 48, 2),), resident=None)
    t = rpt.Tracer(make(), device=0, seed=6)
    try:
        v0, v1 = _arrays(t)
        far = v1.copy()
        far[0] = [2.0 ** 61, -3.0e38, 2.0 ** 100]
        _move(t, form, {1: _dev(torch_cuda, far)})
        assert _walk(rpt, t) == 1, "no triangle uses the vertex: the walk stays on"
        _assert_positions(_held(t), [v0, far], "an unused vertex beyond 2^60")
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, [v0, far], 6, **sizes), "%s: an unused vertex beyond 2^60" % form)
        _move(t, form, {1: (_dev(torch_cuda, v1), _translation(F([2.0 ** 61, 0, 0])))})      # now the referenced ones as well
        assert _walk(rpt, t) == 0
        far0 = v0.copy()
        far0[1, 2] = F(2.0 ** 61)
        _move(t, form, {0: _dev(torch_cuda, far0), 1: _dev(torch_cuda, far)})              # mesh 0's vertex 1 IS used
        assert _walk(rpt, t) == 0
        _move(t, form, {0: _dev(torch_cuda, v0)})
        assert _walk(rpt, t) == 1
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, [v0, far], 6, **sizes), "%s: back, the unused vertex still far" % form)
    finally:
        t.close()


# ---- 6. ordering ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_the_source_is_ordered_behind_its_producer_and_consumed_at_return(rpt, torch_cuda, form):
    torch = torch_cuda
    make, seed = _small_scene, 41
    sizes = dict(sizes=((96, 54, 5), (64, 48, 1)), resident=(96, 54, 3))
    t = rpt.Tracer(make(), device=0, seed=seed)
    try:
        v0, v1 = _arrays(t)
        rest = _dev(torch, v1)
        stream = torch.cuda.Stream(device="cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):                               # a producer on a stream of its own, still running when the call is made
            src = rest.clone()
            for k in range(200):
                src = src * 1.001 + 0.0005
            _move(t, form, {1: src})                                  # no synchronisation by the test
        want = src.cpu().numpy()                                      # what the producer computed, read after the call
        assert np.isfinite(want).all() and np.abs(want - v1).max() > 0.05
        _assert_positions(_held(t), [v0, want], "a source produced on another stream")
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, [v0, want], seed, **sizes), "%s: a source produced on another stream" % form)
        # the source is overwritten as soon as the call returns
        src2 = _dev(torch, v1 + F(0.25))
        _move(t, form, {1: (src2, _translation(F([0, 0.1, 0])))})
        src2.fill_(float("nan"))
        want = restate_move(v1 + F(0.25), _translation(F([0, 0.1, 0])))
        got = _frames(rpt, t, **sizes)
        torch.cuda.synchronize()
        assert bool(torch.isnan(src2).all())
        _assert_positions(_held(t), [v0, want], "a source overwritten after the call")
        _assert_frames(got, _fresh_frames(rpt, make, [v0, want], seed, **sizes), "%s: a source overwritten after the call" % form)
    finally:
        t.close()


# ---- 7. one context, many calls ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_host_and_device_forms_on_one_context(rpt, torch_cuda, devices):
    from rust_pathtracer_amd import scenes
    torch = torch_cuda
    make, seed = _small_scene, 19
    t = rpt.Tracer(make(), seed=seed, **(dict(devices=devices) if devices else dict(device=0)))

    def check(cur, what):
        _assert_frames(_frames(rpt, t), _fresh_frames(rpt, make, cur, seed), what)
        _assert_positions(_held(t), cur, what)

    try:
        m1, m2 = scenes.mesh_scene_moved(make(), 0.7), scenes.mesh_scene_moved(make(), 2.0)
        cur = [np.asarray(v, F) for v in m1]
        t.update_meshes(dict(enumerate(m1)))
        check(cur, "host update")
        t.update_meshes_device({0: _dev(torch, m2[0])})
        cur[0] = np.asarray(m2[0], F)
        check(cur, "device update")
        xf = F([0, 0, 1, 0.1, 1, 0, 0, 0, 0, 1, 0, -0.2])
        t.rebuild_meshes_device({1: (_dev(torch, m2[1]), xf)})
        cur[1] = restate_move(m2[1], xf)
        check(cur, "device rebuild")
        rebuilt = _tables(rpt, t)
        t.rebuild_meshes()                                            # over the positions the context holds: the same tables
        check(cur, "host rebuild in place")
        again = _tables(rpt, t)
        assert np.array_equal(rebuilt[0], again[0]) and np.array_equal(rebuilt[1], again[1]), "the same positions gave other tables"
        assert not np.array_equal(_bits(np.asarray(t.scene().meshes[1][0], F)), _bits(cur[1])), "the wrapper's array is stale until an upload"
        t.upload_scene()                                              # the wrapper reads the moved positions back first
        _assert_positions(_arrays(t), cur, "the wrapper's scene after upload_scene()")
        check(cur, "upload after the device-source calls")
        t.update_meshes_device({1: (_dev(torch, m1[1]), IDENTITY)})
        cur[1] = restate_move(m1[1], IDENTITY)
        check(cur, "device update after the upload")
        t.update_meshes({1: m2[1]})                                   # a host update names the mesh's array again: nothing stale
        cur[1] = np.asarray(m2[1], F)
        t.upload_scene()
        check(cur, "upload after a host update")
    finally:
        t.close()


# ---- 8. the product library -------------------------------------------------------------------------------------------------------
CHILD = r'''
import hashlib, json, os, sys
os.environ.pop("RPT_LIB", None)                      # a plain import: the product
import importlib.util
import numpy as np
import torch
spec = importlib.util.spec_from_file_location("rust_pathtracer_amd", os.path.join(%(root)r, "rust-pathtracer_amd", "__init__.py"),
                                              submodule_search_locations=[os.path.join(%(root)r, "rust-pathtracer_amd")])
rpt = importlib.util.module_from_spec(spec); sys.modules["rust_pathtracer_amd"] = rpt; spec.loader.exec_module(rpt)
from rust_pathtracer_amd import scenes
s = scenes.mesh_scene(subdivisions=2, n_major=16, n_minor=8)
moved = scenes.mesh_scene_moved(s, 1.0)
t = rpt.Tracer(s, device=0, seed=4)
xf = np.float32(%(xf)r)
t.update_meshes_device({0: torch.from_numpy(np.ascontiguousarray(moved[0], np.float32)).to("cuda:0")})
t.rebuild_meshes_device({1: (torch.from_numpy(np.ascontiguousarray(moved[1], np.float32)).to("cuda:0"), xf)})
buf = rpt.ColorBuffer(96, 54)
t.render_n(buf, 3)
held = t.mesh_vertices(1)
t.close()
print("RESULT " + json.dumps({"path": rpt._lib.LIB_PATH, "hooks": int(rpt.lib().rpt_build_has_test_hooks()),
                              "frame": hashlib.sha1(buf.image().tobytes()).hexdigest(), "held": hashlib.sha1(held.tobytes()).hexdigest()}))
'''


def test_the_product_library_moves_like_the_test_build(rpt, torch_cuda):
    from rust_pathtracer_amd import scenes
    xf = [0.8, -0.6, 0.0, 0.1, 0.6, 0.8, 0.0, 0.0, 0.0, 0.0, 1.0, -0.1]
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "xf": xf}], capture_output=True, text=True, timeout=600,
                       env={k: v for k, v in os.environ.items() if k != "RPT_LIB"})
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert os.path.samefile(got["path"], os.path.join(ROOT, "rust-pathtracer_amd", "librpt_hip.so")) and got["hooks"] == 0
    s = _small_scene()
    moved = scenes.mesh_scene_moved(s, 1.0)
    want = [np.asarray(moved[0], F), restate_move(moved[1], F(xf))]
    assert got["held"] == hashlib.sha1(want[1].tobytes()).hexdigest(), "the product library holds other positions than the restatement"
    t = rpt.Tracer(s, device=0, seed=4)
    try:
        t.update_meshes_device({0: _dev(torch_cuda, moved[0])})
        t.rebuild_meshes_device({1: (_dev(torch_cuda, moved[1]), F(xf))})
        here = _frames(rpt, t, sizes=((96, 54, 3),), resident=None)[0]
    finally:
        t.close()
    assert got["frame"] == hashlib.sha1(here.tobytes()).hexdigest(), "the product library's frame differs from the test build's"
    _assert_frames([here], _fresh_frames(rpt, _small_scene, want, 4, sizes=((96, 54, 3),), resident=None), "against a fresh upload")
