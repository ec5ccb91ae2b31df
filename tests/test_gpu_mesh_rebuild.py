"""rpt_rebuild_meshes on the GPU (include/rpt.h, "rebuilding a moved mesh's hierarchy"): new vertex positions and a NEW hierarchy, built
on the device.

As for an update, everything is bit for bit and nothing takes the build's own output as truth:
* frames after a rebuild equal the frames of a FRESH context that uploads the moved scene (the unchanged upload path: host SAH);
* the walk over the rebuilt tables equals the same query under RPT_MESH_QUERY_BRUTE, a fresh upload's answers, and
  tests/test_gpu_mesh.py's numpy restatement of the ordered loop;
* the tables (rpt_debug_mesh_tables) hold the hierarchy's invariants — a permutation of the triangles with their materials, every
  slot in exactly one leaf of 1-8, depth <= 24, a parent below its children, every box the exact union below it — and two rebuilds
  give the same bytes;
* a scene whose Morton splits alone would be deeper than the walk's stack stays within it;
* a rejected call leaves frames and tables untouched; the product library rebuilds like the test build.
Every frame comparison asserts through rpt_debug_kernel_choice that the mesh kernel ran (test_gpu_mesh_update.py, _frames)."""
import bisect
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
from test_gpu_mesh_update import (MESH_BIT, _assert_frames, _choice, _frames, _fresh_frames, _mesh_stats, _moves, _restate_tables, _same,
                                  _small_scene, _table_scenes, _tables, _with_vertices)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF, COUNT_SHIFT, SLOT_MASK, MAX_DEPTH, LEAF_MAX = 0x80000000, 27, (1 << 27) - 1, 24, 8


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _arrays(t):
    return [np.array(v, np.float32, copy=True) for v, _, _ in t.scene().meshes]


def _check_tables(rpt, t, what):
    """The invariants of the hierarchy the context's first device holds, in numpy; -> (rows, nodes)."""
    s = t.scene()
    tris = _mesh_tris(s)
    rows, nodes = _tables(rpt, t)
    n, n_nodes = len(tris), len(nodes)
    assert len(rows) == n, what
    # the rows: a permutation of the flattened triangles, each with its mesh's material, the unused word zero
    order = rows[:, 3].astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(n)), "%s: the rows' flattened indices are not a permutation" % what
    material = np.concatenate([np.full(len(tr), m, np.uint32) for _, tr, m in s.meshes])
    assert np.array_equal(rows[:, 11], material[order]) and not rows[:, 7].any(), "%s: the materials did not travel with the rows" % what
    # the shape: breadth-first, every slot in exactly one leaf of 1..8, no leaf deeper than the walk's stack
    child = nodes[:, 12:14].astype(np.int64)
    assert not nodes[:, 14:].any(), what
    depth = np.full(n_nodes, -1, np.int64)
    depth[0] = 0
    covered = np.zeros(n, np.int64)
    deepest = 0
    for i in range(n_nodes):
        assert depth[i] >= 0, "%s: node %d has no parent below it" % (what, i)
        for c in range(2):
            ch = int(child[i, c])
            if ch & LEAF:
                cnt, first = (ch >> COUNT_SHIFT) & 15, ch & SLOT_MASK
                if cnt == 0:
                    assert n <= LEAF_MAX and i == 0 and c == 1 and ch == LEAF, "%s: an empty child at node %d" % (what, i)
                    continue
                assert cnt <= LEAF_MAX and first + cnt <= n, (what, i, cnt, first)
                covered[first:first + cnt] += 1
                deepest = max(deepest, int(depth[i]) + 1)
            else:
                assert i < ch < n_nodes and depth[ch] < 0, "%s: node %d's child %d" % (what, i, ch)
                depth[ch] = depth[i] + 1
    assert (covered == 1).all(), "%s: %d slots are not in exactly one leaf" % (what, int((covered != 1).sum()))
    assert (np.diff(depth) >= 0).all(), "%s: the levels are not contiguous" % what
    stats = _mesh_stats(rpt, t)
    assert deepest <= MAX_DEPTH and stats == (n_nodes, deepest), (what, stats, n_nodes, deepest)
    if n <= LEAF_MAX:
        assert n_nodes == 1 and child[0, 0] == (LEAF | (n << COUNT_SHIFT)), what
    # the floats: rows {a, b - a, c - a} and every box the exact union below it, byte for byte, for THIS shape
    want_rows, want_nodes = _restate_tables(tris, rows, nodes)
    assert np.array_equal(rows, want_rows), "%s: %d row words differ" % (what, int((rows != want_rows).sum()))
    assert np.array_equal(nodes, want_nodes), "%s: %d node words differ" % (what, int((nodes != want_nodes).sum()))
    return rows, nodes


# ---- 1. frames equal a fresh upload's ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_frames_after_a_rebuild_equal_a_fresh_upload(rpt, torch_cuda, which):
    """A small and a large move, the meshes onto each other, a mesh collapsed to one point (every Morton code of it equal: the index
    bits and the middle rule decide), and back; then a rebuild in place after an update."""
    what, _ = _scenes()[which]
    make = lambda: _scenes()[which][1]                                # noqa: E731
    seed = 31 + which
    a = rpt.Tracer(make(), device=0, seed=seed)
    try:
        first = _frames(rpt, a)
        shapes = []
        for name, updates in _moves(make()):
            a.rebuild_meshes(updates)
            got = _frames(rpt, a)
            want = _fresh_frames(rpt, make, _arrays(a), seed)
            _assert_frames(got, want, "%s, rebuilt after %s" % (what, name))
            rows, nodes = _check_tables(rpt, a, "%s, %s" % (what, name))
            shapes.append((rows[:, 3].copy(), nodes[:, 12:14].copy()))
        _assert_frames(got, first, "%s: back to the original" % what)
        assert not np.array_equal(shapes[0][0], shapes[3][0]), "the collapse changed the leaf order"
        # n_updates == 0 after an update: the refitted shape is replaced by one for the present positions
        large = _moves(make())[1][1]
        a.update_meshes(large)
        refitted = _frames(rpt, a)
        before = _tables(rpt, a)
        a.rebuild_meshes()
        _assert_frames(_frames(rpt, a), refitted, "%s: rebuilt in place" % what)
        _assert_frames(refitted, _fresh_frames(rpt, make, _arrays(a), seed), "%s: rebuilt in place, against a fresh upload" % what)
        rows, nodes = _check_tables(rpt, a, "%s, in place" % what)
        assert not np.array_equal(rows[:, 3], before[0][:, 3]), "a rebuild in place gave the refitted order"
        assert np.array_equal(rows[:, 3], shapes[1][0]) and np.array_equal(nodes[:, 12:14], shapes[1][1]), "the same positions gave another shape"
    finally:
        a.close()


def test_a_scene_of_at_most_eight_triangles(rpt, torch_cuda):
    """Eight triangles in three meshes, then one: a root with one leaf beside an empty child, as the upload builds it."""
    from rust_pathtracer_amd import scenes

    def eight():
        s = scenes.mesh_scene(subdivisions=1, n_major=6, n_minor=4)
        rng = np.random.default_rng(8)
        v = rng.uniform(-0.8, 0.8, (10, 3)).astype(np.float32) + np.float32([0, 0.3, 0.4])
        s.meshes = [(v[:7], np.uint32([[0, 1, 2], [2, 3, 4], [4, 5, 6], [0, 3, 6], [1, 4, 6]]), 0),
                    (v[7:], np.uint32([[0, 1, 2]]), 1), (v[:4].copy(), np.uint32([[0, 1, 3], [1, 2, 3]]), 0)]
        return s

    def one():
        s = eight()
        s.meshes = s.meshes[1:2]
        return s

    sizes = dict(sizes=((64, 48, 3),), resident=(48, 32, 2))
    t = rpt.Tracer(eight(), device=0, seed=3)
    try:
        for n_tris, make in ((8, eight), (1, one)):
            if n_tris == 1:                                           # (another upload on the context that has rebuilt)
                t._scene = one()
                t.upload_scene()
            moved = [(v * np.float32(1.3) + np.float32(0.1)).astype(np.float32) for v in _arrays(t)]
            t.rebuild_meshes(dict(enumerate(moved)))
            _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, moved, 3, **sizes), "%d triangles" % n_tris)
            rows, nodes = _check_tables(rpt, t, "%d triangles" % n_tris)
            assert len(nodes) == 1 and len(rows) == n_tris and nodes[0, 13] == LEAF
            assert np.array_equal(nodes[0, 6:12].view(np.float32), np.float32([np.inf] * 3 + [-np.inf] * 3)), "the empty child's box"
            assert _mesh_stats(rpt, t) == (1, 1)
            t.update_meshes({0: moved[0] + np.float32(0.05)})         # ... and the refit walks the one-node plan
            _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, _arrays(t), 3, **sizes), "%d triangles, updated" % n_tris)
    finally:
        t.close()


def test_a_vertex_beyond_2_60_and_back(rpt, torch_cuda):
    """use_bvh follows the positions through a rebuild, and the tables a rebuild leaves while the loop serves are valid: the update
    that brings the vertex back turns the walk on over them."""
    from rust_pathtracer_amd import scenes
    make = lambda: scenes.mesh_scene(subdivisions=1, n_major=6, n_minor=4)      # noqa: E731
    sizes = dict(sizes=((64, 48, 2),), resident=(48, 32, 1))
    t = rpt.Tracer(make(), device=0, seed=9)
    try:
        first = _frames(rpt, t, **sizes)
        v0, v1 = _arrays(t)
        far = v1.copy()
        far[5, 0] = np.float32(2.0 ** 61)
        far[9, 2] = np.float32(-3.0e38)
        t.rebuild_meshes({1: far})
        got = _frames(rpt, t, **sizes)
        _assert_frames(got, _fresh_frames(rpt, make, [v0, far], 9, **sizes), "a vertex at 2^61")
        assert not _same(got[0], first[0])
        _check_tables(rpt, t, "a vertex at 2^61")
        t.rebuild_meshes({0: v0})                                     # the other mesh: the loop still serves
        _assert_frames(_frames(rpt, t, **sizes), got, "2^61, the other mesh rebuilt")
        t.update_meshes({1: v1})                                      # back, by a refit of the tables built beyond 2^60
        _assert_frames(_frames(rpt, t, **sizes), first, "back from 2^61 by an update")
        _check_tables(rpt, t, "back from 2^61 by an update")
        t.rebuild_meshes({1: far})
        t.rebuild_meshes({1: v1})
        _assert_frames(_frames(rpt, t, **sizes), first, "back from 2^61 by a rebuild")
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, [v0, v1], 9, **sizes), "back from 2^61, fresh")
    finally:
        t.close()


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_rebuild_update_rebuild_upload_on_one_context(rpt, torch_cuda, oracle, devices):
    from rust_pathtracer_amd import scenes
    make = _small_scene
    seed = 17
    sizes = dict(sizes=((96, 54, 5), (64, 48, 1)), resident=(96, 54, 3))
    t = rpt.Tracer(make(), seed=seed, **(dict(devices=devices) if devices else dict(device=0)))
    try:
        m1 = scenes.mesh_scene_moved(make(), 2.0)
        t.rebuild_meshes(dict(enumerate(m1)))
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, m1, seed, **sizes), "rebuild")
        rebuilt = _check_tables(rpt, t, "rebuild")
        m2 = scenes.mesh_scene_moved(make(), 0.7)
        t.update_meshes({1: m2[1]})                                   # a refit of the rebuilt shape
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, [m1[0], m2[1]], seed, **sizes), "update after the rebuild")
        rows, nodes = _check_tables(rpt, t, "update after the rebuild")
        assert np.array_equal(rows[:, [3, 7, 11]], rebuilt[0][:, [3, 7, 11]]) and np.array_equal(nodes[:, 12:], rebuilt[1][:, 12:]), "the update kept the rebuilt shape"
        t.rebuild_meshes({0: m2[0]})
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, m2, seed, **sizes), "second rebuild")
        _check_tables(rpt, t, "second rebuild")
        mesh_scene = t.scene()
        t._scene = rpt.AnalyticalScene()
        t.upload_scene()                                              # drops everything the rebuilds allocated
        assert rpt.lib().rpt_rebuild_meshes(t._h, None, 0) == rpt._abi.RPT_ERR_NO_SCENE
        buf = rpt.ColorBuffer(64, 48)
        t.render_n(buf, 2)
        assert _same(buf.image(), oracle.render(oracle.scene_analytical(), 64, 48, 2, seed=seed)), "the analytical scene after the mesh scene"
        t._scene = mesh_scene
        t.upload_scene()
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, m2, seed, **sizes), "the moved scene uploaded again")
        t.update_meshes({0: m1[0]})                                   # the upload's shape, then a first rebuild once more
        t.rebuild_meshes({1: m1[1]})
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, m1, seed, **sizes), "update, then rebuild, after the upload")
        rows, nodes = _check_tables(rpt, t, "update, then rebuild, after the upload")
        assert np.array_equal(rows, rebuilt[0]) and np.array_equal(nodes, rebuilt[1]), "the same positions gave other tables"
    finally:
        t.close()


# ---- 2. the walk ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_exp", [0, -20, 20])
def test_walks_over_the_rebuilt_hierarchy(rpt, torch_cuda, scale_exp):
    from rust_pathtracer_amd import scenes
    scale = 2.0 ** scale_exp
    s = _test_scene(scale)
    rng = np.random.default_rng(3000 + scale_exp)
    moved = scenes.mesh_scene_moved(s, 2.0)
    moved[2] = (moved[2] + rng.uniform(-0.3, 0.3, moved[2].shape) * scale).astype(np.float32)
    t = rpt.Tracer(s, device=0, seed=1)
    fresh = None
    try:
        t.rebuild_meshes(dict(enumerate(moved)))
        tris = _mesh_tris(t.scene())
        fresh = rpt.Tracer(_with_vertices(lambda: _test_scene(scale), moved), device=0, seed=1)
        rays = _rays(tris, 48_000 if scale_exp == 0 else 24_000, rng, scale)
        for use_max in (False, True):
            want = brute_force(tris, rays, use_max)
            flags = rpt._abi.RPT_MESH_QUERY_USE_MAX if use_max else 0
            walk = _query(rpt, torch_cuda, t, rays, flags)
            loop = _query(rpt, torch_cuda, t, rays, flags | rpt._abi.RPT_MESH_QUERY_BRUTE)
            uploaded = _query(rpt, torch_cuda, fresh, rays, flags)
            for against, other in (("the ordered loop on the device", loop), ("a fresh upload's walk", uploaded), ("numpy's ordered loop", want)):
                for name, g, w in zip(("t bits", "index", "any_hit"), walk, other):
                    bad = np.nonzero(g != w)[0]
                    assert len(bad) == 0, "%s against %s (use_max %s): %d rays differ, first %s: got %s want %s" % (
                        name, against, use_max, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])
        assert (want[1] >= 0).mean() > 0.2 and want[2].mean() > 0.05
        _check_tables(rpt, t, "scale 2^%d" % scale_exp)
    finally:
        t.close()
        if fresh:
            fresh.close()


# ---- 3. the tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_tables_after_a_rebuild(rpt, torch_cuda, which):
    what, s = _table_scenes()[which]
    original = [np.array(v, np.float32, copy=True) for v, _, _ in s.meshes]
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        t.rebuild_meshes()                                            # the uploaded positions, a first rebuild without a move
        rows0, nodes0 = _check_tables(rpt, t, what)
        rng = np.random.default_rng(177 + which)
        moved = [(v * np.float32(1.5) + rng.uniform(-0.4, 0.4, v.shape)).astype(np.float32) for v in original]
        t.rebuild_meshes(dict(enumerate(moved)))
        rows1, nodes1 = _check_tables(rpt, t, what + ", moved")
        t.rebuild_meshes(dict(enumerate(moved)))                      # once more: the same bytes
        rows2, nodes2 = _tables(rpt, t)
        assert np.array_equal(rows1, rows2) and np.array_equal(nodes1, nodes2), "two rebuilds of the same positions differ"
        t.rebuild_meshes()
        rows2, nodes2 = _tables(rpt, t)
        assert np.array_equal(rows1, rows2) and np.array_equal(nodes1, nodes2), "a rebuild in place of rebuilt tables differs"
        t.rebuild_meshes(dict(enumerate(original)))
        rows3, nodes3 = _tables(rpt, t)
        assert np.array_equal(rows3, rows0) and np.array_equal(nodes3, nodes0), "back at the uploaded positions: other tables than the first rebuild's"
        buf = rpt.ColorBuffer(32, 24)
        t.render_n(buf, 1)
        assert _choice(rpt, t) & MESH_BIT
    finally:
        t.close()


# ---- 4. the depth rule ------------------------------------------------------------------------------------------------------------
def _morton_only_depth(tris):
    """Depth of the hierarchy the keys' highest-differing-bit splits alone would give (leaves of at most 8), for the flattened
    triangles `tris`: include/rpt.h's key restated — centroid of the triangle's box in f32, 10 bits per axis within the centroids'
    bounds (f64), x highest, the flattened index below."""
    v = tris.astype(np.float32)
    lo, hi = v.min(1), v.max(1)                                       # (no edge here is so long that a + (b - a) leaves the vertices' box)
    c = lo * np.float32(0.5) + hi * np.float32(0.5)
    cmin, cmax = c.min(0).astype(np.float64), c.max(0).astype(np.float64)
    q = np.minimum(np.floor((c.astype(np.float64) - cmin) / (cmax - cmin) * 1024.0), 1023.0).astype(np.uint64)
    keys = np.zeros(len(v), np.uint64)
    for bit in range(10):
        for axis in range(3):
            keys |= ((q[:, axis] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(26 + 3 * bit + 2 - axis)
    keys |= np.arange(len(v), dtype=np.uint64)
    keys = [int(k) for k in np.sort(keys)]

    def depth(b, e, d):
        if e - b <= LEAF_MAX:
            return d
        bit = (keys[b] ^ keys[e - 1]).bit_length() - 1
        m = bisect.bisect_left(keys, ((keys[b] >> bit) | 1) << bit, b, e)      # the first key of the range with that bit set
        return max(depth(b, m, d + 1), depth(m, e, d + 1))
    return depth(0, len(keys), 0)


def test_a_scene_that_presses_on_the_depth_rule(rpt, torch_cuda):
    """A dense cluster at (1, 1, 1), and triangles at 2^-i (1, 1, 1) for i up to 40, nine per position — and, for the ten positions
    the 10-bit cells still tell apart, at 2^-i on each axis alone, so that every bit of the Morton code peels a few triangles off
    the rest.  Those splits alone are deeper than the walk's 24-entry stack (asserted); the build stays within it and the frames
    are a fresh upload's.  Run once: a correctness case."""
    from rust_pathtracer_amd import scenes

    def make():
        s = scenes.mesh_scene(subdivisions=1, n_major=6, n_minor=4)
        rng = np.random.default_rng(40)
        n_cluster = 30000
        centres = (rng.uniform(-0.02, 0.02, (n_cluster, 3)) + [1.0, 1.0, 1.0]).astype(np.float32)
        cluster = centres[:, None, :] + rng.uniform(-0.004, 0.004, (n_cluster, 3, 3)).astype(np.float32)
        chain = []
        for i in range(41):
            for axes in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)) if i <= 10 else ((1, 1, 1),):
                p = np.float32(2.0 ** -i) * np.float32(axes)
                for r in range(9):
                    e = rng.uniform(-0.2, 0.2, (3, 3)).astype(np.float32) * np.float32(2.0 ** -i)
                    chain.append(p + (e - e.mean(0, dtype=np.float32)))
        chain = np.float32(chain)
        s.meshes = [(m.reshape(-1, 3), np.arange(3 * len(m), dtype=np.uint32).reshape(-1, 3), k) for k, m in enumerate((chain, cluster))]
        return s

    s = make()
    alone = _morton_only_depth(_mesh_tris(s))
    assert alone > MAX_DEPTH, "the scene does not press on the rule: its Morton splits alone are %d deep" % alone
    sizes = dict(sizes=((96, 54, 2),), resident=(64, 48, 1))
    t = rpt.Tracer(s, device=0, seed=6)
    try:
        t.rebuild_meshes()
        nodes, depth = _mesh_stats(rpt, t)
        print("morton-only depth %d, built depth %d, %d nodes" % (alone, depth, nodes))
        assert depth <= MAX_DEPTH
        _check_tables(rpt, t, "the pressing scene")
        _assert_frames(_frames(rpt, t, **sizes), _fresh_frames(rpt, make, _arrays(t), 6, **sizes), "the pressing scene")
    finally:
        t.close()


# ---- 5. rejected calls ------------------------------------------------------------------------------------------------------------
def test_rejected_rebuilds_leave_the_scene(rpt, torch_cuda):
    from rust_pathtracer_amd import scenes
    A, lib = rpt._abi, rpt.lib()
    sizes = dict(sizes=((64, 48, 2),), resident=None)
    t = rpt.Tracer(_small_scene(), device=0, seed=5)
    try:
        t.rebuild_meshes()                                            # (so that rebuilt tables are what a rejected call must leave)
        ref = _frames(rpt, t, **sizes)
        ref_tables = _tables(rpt, t)
        v0, v1 = _arrays(t)
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
            assert lib.rpt_rebuild_meshes(t._h, arr, n) == A.RPT_ERR_INVALID_ARG, what
            err = lib.rpt_last_error(t._h)
            assert message.encode() in err and err.startswith(b"rpt_rebuild_meshes: ") and b"rpt_update_meshes" not in err, (what, err)
            _assert_frames(_frames(rpt, t, **sizes), ref, what)
            for got, want in zip(_tables(rpt, t), ref_tables):
                assert np.array_equal(got, want), what
        # ... and a valid one is accepted after them
        moved = scenes.mesh_scene_moved(t.scene(), 0.5)
        t.rebuild_meshes({1: moved[1]})
        got = _frames(rpt, t, **sizes)
        assert not _same(got[0], ref[0])
        _assert_frames(got, _fresh_frames(rpt, _small_scene, [v0, moved[1]], 5, **sizes), "a valid rebuild after the rejected ones")
        assert lib.rpt_rebuild_meshes(None, ups((0, len(v0), ptr(v0))), 1) == A.RPT_ERR_INVALID_ARG
        assert b"rpt_rebuild_meshes" in lib.rpt_last_error(None)
    finally:
        t.close()
    # no mesh scene: a fresh context, and the other scene classes — with and without updates
    one = ups((0, len(v0), ptr(v0)))
    h = C.c_void_p()
    rpt._lib.check(lib.rpt_create(C.byref(h), 0))
    for arr, n in ((one, 1), (None, 0)):
        assert lib.rpt_rebuild_meshes(h, arr, n) == A.RPT_ERR_NO_SCENE
        err = lib.rpt_last_error(h)
        assert b"scene with meshes" in err and err.startswith(b"rpt_rebuild_meshes: "), err
    lib.rpt_destroy(h)
    empty = _small_scene()
    empty.meshes = [(v0, np.zeros((0, 3), np.uint32), 0)]
    for what, s in (("analytical", rpt.AnalyticalScene()), ("large", scenes.random_spheres_scene(300, 5)), ("sdf", scenes.sdf_scene()),
                    ("meshes without triangles", empty)):
        o = rpt.Tracer(s, device=0, seed=5)
        buf = rpt.ColorBuffer(48, 32)
        o.render_n(buf, 1)
        before = buf.image().copy()
        assert lib.rpt_rebuild_meshes(o._h, one, 1) == A.RPT_ERR_NO_SCENE, what
        assert lib.rpt_rebuild_meshes(o._h, None, 0) == A.RPT_ERR_NO_SCENE, what
        buf = rpt.ColorBuffer(48, 32)
        o.render_n(buf, 1)
        assert _same(buf.image(), before), what
        o.close()


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
t.rebuild_meshes(dict(enumerate(scenes.mesh_scene_moved(s, 1.0))))
buf = rpt.ColorBuffer(96, 54)
t.render_n(buf, 3)
t.close()
print("RESULT " + json.dumps({"path": rpt._lib.LIB_PATH, "hooks": int(rpt.lib().rpt_build_has_test_hooks()),
                              "frame": hashlib.sha1(buf.image().tobytes()).hexdigest()}))
'''


def test_the_product_library_rebuilds_like_the_test_build(rpt, torch_cuda):
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
        t.rebuild_meshes(dict(enumerate(moved)))
        here = _frames(rpt, t, sizes=((96, 54, 3),), resident=None)[0]
    finally:
        t.close()
    assert got["frame"] == hashlib.sha1(here.tobytes()).hexdigest(), "the product library's frame differs from the test build's"
    _assert_frames([here], _fresh_frames(rpt, _small_scene, moved, 4, sizes=((96, 54, 3),), resident=None), "against a fresh upload")
