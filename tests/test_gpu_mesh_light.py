"""Mesh lights on the GPU (include/rpt.h, "mesh lights"): next-event estimation on emissive triangle meshes, through a table the
library computes on the device and keeps current through every call that moves a mesh.

Nothing takes the device's own output as truth:
* the table (rpt_download_mesh_light_table) equals tests/test_mesh_light_host.py's numpy restatement — the integers exactly, A_tot's
  bits — on meshes of 1, 255, 256, 257 and 5 003 triangles, on the degenerate and dark cases, with ON and OFF meshes side by side;
* after every kind of move the table equals the restatement on the positions the context holds and that of a fresh upload of the
  moved scene followed by rpt_set_mesh_lights, and the frames are that context's, bit for bit;
* the sampler (rpt_debug_mesh_light_sample) equals the numpy float32 restatement in this file bit for bit, at both ends of the draw,
  on both sides of a CDF step, for r1 = 0, in the triangle's plane, from the back, and on a dark mesh;
* rpt_debug_kernel_choice's bit 27 is set exactly while a mesh is ON, and going back to OFF gives the frames of a context that never
  heard of mesh lights; every rejected call leaves the frames as they were;
* the frames with the lamp ON and OFF estimate the same integral, the ON ones with less variance;
* a context over one device listed twice renders the one-context frame."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_mesh_update import _assert_frames, _choice, _frames, _same, _small_scene, _with_vertices
from test_mesh_light_host import _cross, _dot, edge_meshes, restate_table, sized_meshes, strip

pytestmark = pytest.mark.gpu

F = np.float32
MESH_BIT, SMOOTH_BIT, LIGHT_BIT = 1 << 25, 1 << 26, 1 << 27
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _light_scene(extra=(), **kw):
    """scenes.mesh_light_scene() (the object, mesh 0, and the lamp, mesh 1) plus `extra` meshes [(vertices, indices)], which take the
    lamp's emissive material."""
    from rust_pathtracer_amd import scenes
    s = scenes.mesh_light_scene(**kw)
    for v, t in extra:
        s.meshes.append((np.ascontiguousarray(v, F), np.ascontiguousarray(t, np.uint32), 1))
    return s


def _assert_tables(t, meshes, what):
    """The context's tables of `meshes` equal the restatement on the positions the context holds."""
    out = {}
    for m in meshes:
        _, idx, _ = t.scene().meshes[m]
        cdf, e, area = t.mesh_light_table(m)
        want_cdf, want_e, want_area = restate_table(t.mesh_vertices(m), idx)
        assert np.array_equal(cdf, want_cdf), "%s, mesh %d: %d of %d sums differ" % (what, m, int((cdf != want_cdf).sum()), len(cdf))
        assert e == want_e and area.view(np.uint32) == want_area.view(np.uint32), (what, m, e, want_e, area, want_area)
        out[m] = (cdf, e, area)
    return out


def _is_off(rpt, t, m):
    n = len(np.asarray(t.scene().meshes[m][1]).reshape(-1, 3))
    cdf = np.zeros(max(n, 1), np.uint64)
    e, area = C.c_int32(0), C.c_float(0.0)
    rc = rpt.lib().rpt_download_mesh_light_table(t._h, m, cdf.ctypes.data, n, C.byref(e), C.byref(area))
    return rc == rpt._abi.RPT_ERR_INVALID_ARG and b"is OFF" in rpt.lib().rpt_last_error(t._h)


# ---- 1. the table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["sizes", "edges"])
def test_table_equals_the_numpy_restatement(rpt, torch_cuda, which):
    """`sizes`: meshes of 1, 255, 256, 257 and 5 003 triangles (the scan's seams: 256 faces per workgroup, and a second level at
    5 003 together with the others).  `edges`: a degenerate triangle, areas that span more than 2^36, one triangle, no triangle, an
    overflowing edge, only degenerate triangles.  In two calls, so that ON meshes stand next to OFF ones and meshes not named keep
    their mode; the scene's own object stays OFF throughout."""
    named = sized_meshes() if which == "sizes" else edge_meshes()
    s = _light_scene([(v, t) for _, v, t in named])
    n = len(s.meshes)
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        first = list(range(1, n, 2))
        t.set_mesh_lights({m: True for m in first})
        _assert_tables(t, first, "%s: every second mesh" % which)
        for m in range(0, n, 2):
            assert _is_off(rpt, t, m), m
        buf = rpt.ColorBuffer(32, 24)
        t.render_n(buf, 1)
        assert _choice(rpt, t) & (MESH_BIT | LIGHT_BIT) == MESH_BIT | LIGHT_BIT and np.isfinite(buf.image()).all()
        t.set_mesh_lights({m: True for m in range(2, n, 2)})
        got = _assert_tables(t, range(1, n), "%s: every mesh but the object" % which)
        assert _is_off(rpt, t, 0)
        dark = [named[m - 2][0] for m in range(2, n) if got[m][2] == 0]
        assert dark == ([] if which == "sizes" else ["no triangle", "an overflowing edge", "only degenerate triangles"])
        for m in range(2, n):
            if got[m][2] == 0:
                assert not got[m][0].any() and got[m][1] == 0
        # a wrong n_triangles, and a mesh out of range
        cdf = np.zeros(8, np.uint64)
        e, area = C.c_int32(0), C.c_float(0.0)
        A = rpt._abi
        assert rpt.lib().rpt_download_mesh_light_table(t._h, 1, cdf.ctypes.data, 3, C.byref(e), C.byref(area)) == A.RPT_ERR_INVALID_ARG
        assert b"n_triangles 3" in rpt.lib().rpt_last_error(t._h)
        assert rpt.lib().rpt_download_mesh_light_table(t._h, n, cdf.ctypes.data, 2, C.byref(e), C.byref(area)) == A.RPT_ERR_INVALID_ARG
        assert rpt.lib().rpt_download_mesh_light_table(t._h, 1, cdf.ctypes.data, 2, None, C.byref(area)) == A.RPT_ERR_INVALID_ARG
        t.render_n(buf, 1)
        assert np.isfinite(buf.image()).all()
    finally:
        t.close()


# ---- 2. moves ---------------------------------------------------------------------------------------------------------------------
def _lit_small_scene():
    """test_gpu_mesh_update's small mesh scene (an icosphere of 320 and a torus of 256 triangles) with the shadow rays' flag and an
    emissive torus."""
    s = _small_scene()
    s.any_hit_uses_max_dist = True
    s.materials[1].fields["emission"] = (4.0, 3.0, 2.0)
    return s


def _all_on(t):
    t.set_mesh_lights({m: True for m in range(len(t.scene().meshes))})


def _fresh(rpt, arrays):
    """The yardstick: a fresh context that uploads the scene with these positions and then turns every mesh ON."""
    b = rpt.Tracer(_with_vertices(_lit_small_scene, arrays), device=0, seed=8)
    try:
        _all_on(b)
        return _frames(rpt, b), {m: b.mesh_light_table(m) for m in (0, 1)}
    finally:
        b.close()


def _assert_same_tables(got, want, what):
    for m in want:
        assert np.array_equal(got[m][0], want[m][0]) and got[m][1] == want[m][1] and got[m][2].view(np.uint32) == want[m][2].view(np.uint32), (what, m)


MATRIX = np.array([[0.96, -0.28, 0.0, 0.05], [0.28, 0.96, 0.0, -0.02], [0.0, 0.0, 1.25, 0.01]], F)


@pytest.mark.parametrize("form", ["update", "rebuild", "update_device", "rebuild_device"])
def test_tables_and_frames_follow_every_kind_of_move(rpt, torch_cuda, form):
    from rust_pathtracer_amd import scenes
    s = _lit_small_scene()
    rest = [np.array(v, F, copy=True) for v, _, _ in s.meshes]
    t = rpt.Tracer(s, device=0, seed=8)
    try:
        _all_on(t)
        before = _assert_tables(t, (0, 1), "before any move")
        want_frames, want_tables = _fresh(rpt, rest)
        still = _frames(rpt, t)
        _assert_frames(still, want_frames, "before any move")
        _assert_same_tables(before, want_tables, "before any move")
        moved = scenes.mesh_scene_moved(s, 0.7)
        if form == "update":
            t.update_meshes(dict(enumerate(moved)))
        elif form == "rebuild":
            t.rebuild_meshes(dict(enumerate(moved)))
        else:                                                         # the device forms: mesh 0 as it is, mesh 1 through a 3x4 matrix
            src = {0: torch_cuda.from_numpy(moved[0]).to("cuda:0"), 1: (torch_cuda.from_numpy(rest[1]).to("cuda:0"), MATRIX)}
            (t.update_meshes_device if form == "update_device" else t.rebuild_meshes_device)(src)
        held = [t.mesh_vertices(m) for m in (0, 1)]
        assert not np.array_equal(held[1], rest[1]) and np.array_equal(held[0].view(np.uint32), moved[0].view(np.uint32))
        after = _assert_tables(t, (0, 1), form)
        assert not np.array_equal(after[0][0], before[0][0]) and (form in ("update", "rebuild") or after[1][2] != before[1][2])
        want_frames, want_tables = _fresh(rpt, held)
        _assert_same_tables(after, want_tables, "%s: against a fresh upload" % form)
        got = _frames(rpt, t)
        assert _choice(rpt, t) & LIGHT_BIT
        _assert_frames(got, want_frames, "%s: against a fresh upload" % form)
        assert not _same(got[0], still[0])
        # a rebuild with unchanged positions reorders slots and leaves every table bit for bit
        assert rpt.lib().rpt_rebuild_meshes(t._h, None, 0) == rpt._abi.RPT_OK
        _assert_same_tables({m: t.mesh_light_table(m) for m in (0, 1)}, after, "after rpt_rebuild_meshes(ctx, NULL, 0)")
        _assert_frames(_frames(rpt, t), want_frames, "after rpt_rebuild_meshes(ctx, NULL, 0)")
        # a rejected move leaves tables and frames as they were
        bad = np.array(held[0], F, copy=True)
        bad[3, 1] = np.nan
        with pytest.raises(Exception):
            t.update_meshes({0: bad})
        with pytest.raises(Exception):
            t.rebuild_meshes({0: bad[:-1]})
        _assert_same_tables({m: t.mesh_light_table(m) for m in (0, 1)}, after, "after rejected moves")
        _assert_frames(_frames(rpt, t), want_frames, "after rejected moves")
    finally:
        t.close()


def test_the_order_of_set_mesh_lights_and_the_first_move_does_not_matter(rpt, torch_cuda):
    from rust_pathtracer_amd import scenes
    s = _lit_small_scene()
    moved = scenes.mesh_scene_moved(s, 0.7)
    want_frames, want_tables = _fresh(rpt, moved)
    t = rpt.Tracer(s, device=0, seed=8)
    try:
        t.rebuild_meshes(dict(enumerate(moved)))                     # the context's first move, then the lights
        _all_on(t)
        _assert_same_tables(_assert_tables(t, (0, 1), "rebuild first"), want_tables, "rebuild first")
        _assert_frames(_frames(rpt, t), want_frames, "rebuild, then rpt_set_mesh_lights")
    finally:
        t.close()


# ---- 3. the sampler ---------------------------------------------------------------------------------------------------------------
def restate_samples(v, idx, table, scatter, r0a, r0b, r1, r2):
    """include/rpt.h, "sampling an ON mesh", on float32 arrays, one rounding per operation; the pick in Python integers.
    -> (k [n] int64 or -1, direction, normal [n, 3] f32, dist, pdf [n] f32)."""
    cdf, _, a_tot = table
    n = len(scatter)
    zero3, zero = np.zeros((n, 3), F), np.zeros(n, F)
    if not a_tot > 0:
        return np.full(n, -1, np.int64), zero3, zero3.copy(), zero, zero.copy()
    v = np.ascontiguousarray(v, F).reshape(-1, 3)
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    q_all = int(cdf[-1])
    ja, jb = (r0a * F(16777216.0)).astype(np.int64), (r0b * F(16777216.0)).astype(np.int64)
    big = [((int(x) << 24) | int(y)) for x, y in zip(ja, jb)]
    tt = np.array([(j * q_all) >> 48 for j in big], np.uint64)
    assert (tt < q_all).all()
    k = np.searchsorted(cdf, tt, side="right")                       # the first index with C_k > T
    assert (np.diff(np.concatenate([[0], cdf.astype(object)]))[k] > 0).all()
    with np.errstate(all="ignore"):
        a, b, c = v[idx[k, 0]], v[idx[k, 1]], v[idx[k, 2]]
        e1, e2 = b - a, c - a
        su = np.sqrt(r1)
        bu = F(1.0) - su
        bv = r2 * su
        p = (a + bu[:, None] * e1) + bv[:, None] * e2
        d = p - scatter
        dist = np.sqrt(_dot(d, d))
        dist_sq = dist * dist
        d = d / dist[:, None]
        g = _cross(e1, e2)
        nrm = g / np.sqrt(_dot(g, g))[:, None]
        cs = _dot(nrm, d)
        normal = np.where((cs > 0)[:, None], -nrm, nrm)
        pdf = dist_sq / (a_tot * np.abs(cs))
    for x in (su, p, d, dist, nrm, cs, normal, pdf):
        assert x.dtype == F
    return k.astype(np.int64), d, normal, dist, pdf


def _sample(rpt, torch, t, rec):
    n = len(rec)
    dev = torch.from_numpy(np.ascontiguousarray(rec, F)).cuda()
    out = torch.zeros(n, 9, dtype=torch.int32, device="cuda")
    rpt._lib.check(rpt.lib().rpt_debug_mesh_light_sample(t._h, dev.data_ptr(), n, out.data_ptr(), None), t._h)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _draws_for(cdf, targets):
    """-> (r0a, r0b) whose J gives T = (J * Q) >> 48 equal to each of `targets` (Q <= 2^48: every T below Q is reached)."""
    q_all = int(cdf[-1])
    assert q_all <= 1 << 48
    out = []
    for tt in targets:
        j = -((-int(tt) << 48) // q_all)                              # the smallest J with J * Q >= T * 2^48
        assert j < 1 << 48 and (j * q_all) >> 48 == int(tt)
        out.append((F(j >> 24) / F(16777216.0), F(j & 0xFFFFFF) / F(16777216.0)))
    return np.array(out, F).reshape(-1, 2)


def test_sampler_equals_the_numpy_restatement(rpt, torch_cuda):
    """About 10^4 records over four ON meshes — a quad of two triangles in the plane y = 1.4, a strip of 257 triangles, one of
    5 003, and a mesh of degenerate triangles only (dark) — next to the OFF object and the OFF lamp."""
    rng = np.random.default_rng(77)
    quad = (np.array([[-0.15, 1.4, 0.85], [0.15, 1.4, 0.85], [0.15, 1.4, 1.15], [-0.15, 1.4, 1.15]], F), np.array([[0, 1, 2], [0, 2, 3]], np.uint32))
    extra = [quad, strip(257, 357), strip(5003, 5103), [m for m in edge_meshes() if m[0] == "only degenerate triangles"][0][1:]]
    s = _light_scene(extra)
    t = rpt.Tracer(s, device=0, seed=2)
    A = rpt._abi
    try:
        dummy = torch_cuda.zeros(16, dtype=torch_cuda.float32, device="cuda")
        assert rpt.lib().rpt_debug_mesh_light_sample(t._h, dummy.data_ptr(), 1, dummy.data_ptr(), None) == A.RPT_ERR_INVALID_ARG
        assert b"no mesh is ON" in rpt.lib().rpt_last_error(t._h)
        t.set_mesh_lights({2: True, 3: True, 4: True, 5: True})
        tables = _assert_tables(t, (2, 3, 4, 5), "the sampler's scene")
        assert tables[5][2] == 0 and all(tables[m][2] > 0 for m in (2, 3, 4))
        total = 0
        for ordinal, m in enumerate((2, 3, 4, 5)):
            v, idx, _ = s.meshes[m]
            v = np.asarray(v, F).reshape(-1, 3)
            cdf = tables[m][0]
            n = 2600
            lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
            scatter = rng.uniform(lo - 1.5, hi + 1.5, (n, 3)).astype(F)
            draws = (rng.integers(0, 1 << 24, (n, 4)).astype(F) / F(16777216.0)).astype(F)
            special = n_on = 0
            if tables[m][2] > 0:
                one = F((1 << 24) - 1) / F(16777216.0)
                draws[0, :2] = 0.0                                    # J = 0
                draws[1, :2] = one                                    # J = 2^48 - 1
                draws[2:12, 2] = 0.0                                  # r1 = 0: the point is corner b
                special = 12
                if int(cdf[-1]) <= 1 << 48:
                    steps = np.unique(cdf[cdf > 0])[:40].astype(object)
                    on = _draws_for(cdf, [c for c in steps if c < int(cdf[-1])])          # T == C_k: the next triangle with q > 0
                    below = _draws_for(cdf, [c - 1 for c in steps])                       # T == C_k - 1: still triangle k
                    both = np.concatenate([on, below])
                    draws[special:special + len(both), :2] = both
                    special += len(both)
                    n_on = len(on)
            if m == 2:                                                # the quad: in its plane (c == 0), and from above (the normal turns)
                scatter[special:special + 40, 1] = F(1.4)
                scatter[special + 40:special + 300, 1] = rng.uniform(1.5, 3.0, 260).astype(F)
            rec = np.concatenate([scatter, draws, np.full((n, 1), ordinal, np.uint32).view(F)], 1)
            got = _sample(rpt, torch_cuda, t, rec)
            k, d, normal, dist, pdf = restate_samples(v, idx, tables[m], scatter, *draws.T)
            want = np.concatenate([np.where(k < 0, NONE, k).astype(np.uint32)[:, None], d.view(np.uint32), normal.view(np.uint32),
                                   dist.view(np.uint32)[:, None], pdf.view(np.uint32)[:, None]], 1)
            same = (got == want) | (np.isnan(got.view(F)) & np.isnan(want.view(F)))
            same[:, 0] = got[:, 0] == want[:, 0]
            bad = np.nonzero(~same.all(axis=1))[0]
            assert len(bad) == 0, "mesh %d: %d records differ, first %s: got %s want %s" % (m, len(bad), bad[:3], got[bad[:3]], want[bad[:3]])
            total += n
            if m == 5:
                assert not got[:, 1:].any() and (got[:, 0] == NONE).all(), "a dark mesh leaves LightSampleRec::new()'s zeros"
                continue
            assert len(np.unique(k)) > min(len(idx), 200) // 2 and np.isfinite(pdf[special + 300:]).mean() > 0.99
            if m == 2:
                cs = _dot(normal, d)
                plane = slice(special, special + 40)
                assert (cs[plane] == 0).all() and np.isinf(pdf[plane]).all(), "a scatter point in the plane: c == 0, the facing test fails"
                above = slice(special + 40, special + 300)
                assert (normal[above, 1] > 0).all() and (cs[above] < 0).all(), "from the back the normal turns toward the point"
                assert (normal[special + 300:][scatter[special + 300:, 1] < 1.39, 1] < 0).all()
            if n_on:                                                  # (records 12 .. 12 + n_on: T == C_k; the next ones: T == C_k - 1, same steps)
                assert (k[12:12 + n_on] > k[12 + n_on:12 + 2 * n_on]).all(), "T == C_k picks a triangle after k, T == C_k - 1 still k"
        assert total >= 10000
        # an ordinal past the ON meshes: zeros
        rec = np.zeros((4, 8), F)
        rec[:, 7] = np.array([4, 5, 1000, NONE], np.uint32).view(F)
        got = _sample(rpt, torch_cuda, t, rec)
        assert (got[:, 0] == NONE).all() and not got[:, 1:].any()
    finally:
        t.close()


# ---- 4. kernel choice and the way back --------------------------------------------------------------------------------------------
def test_bit_27_and_the_way_back(rpt, torch_cuda):
    sizes = dict(sizes=((64, 48, 3), (32, 24, 1)), resident=(64, 48, 2))
    s = _light_scene(sphere_light=True)
    t = rpt.Tracer(s, device=0, seed=3)
    u = rpt.Tracer(_light_scene(sphere_light=True), device=0, seed=3)       # the untouched context
    try:
        never = _frames(rpt, t, **sizes)
        choice = _choice(rpt, t)
        assert choice & MESH_BIT and not choice & (LIGHT_BIT | SMOOTH_BIT)
        _assert_frames(_frames(rpt, u, **sizes), never, "two contexts, one scene")
        t.set_mesh_lights({1: True})
        on = _frames(rpt, t, **sizes)
        assert _choice(rpt, t) & (MESH_BIT | LIGHT_BIT | SMOOTH_BIT) == MESH_BIT | LIGHT_BIT
        assert not _same(on[0], never[0]) and np.isfinite(on[0]).all()
        t.set_mesh_lights({0: True})                                  # the object is not emissive: a light that adds nothing but is picked
        both = _frames(rpt, t, **sizes)
        assert not _same(both[0], on[0]) and _choice(rpt, t) & LIGHT_BIT
        t.set_mesh_lights({0: False})
        _assert_frames(_frames(rpt, t, **sizes), on, "one mesh OFF again")
        # ON and SMOOTH: one kernel, both bits; the smooth object changes the picture, and FLAT again is the ON frame
        t.set_mesh_shading({0: "smooth"})
        smooth_on = _frames(rpt, t, **sizes)
        assert _choice(rpt, t) & (MESH_BIT | LIGHT_BIT | SMOOTH_BIT) == MESH_BIT | LIGHT_BIT | SMOOTH_BIT
        assert not _same(smooth_on[0], on[0])
        t.set_mesh_lights({1: False})                                 # the last ON mesh goes: the smooth kernel alone
        u.set_mesh_shading({0: "smooth"})
        _assert_frames(_frames(rpt, t, **sizes), _frames(rpt, u, **sizes), "SMOOTH, lights OFF again: the smooth kernel's frames")
        assert _choice(rpt, t) == _choice(rpt, u) and _choice(rpt, t) & (LIGHT_BIT | SMOOTH_BIT) == SMOOTH_BIT
        t.set_mesh_lights({1: True})
        _assert_frames(_frames(rpt, t, **sizes), smooth_on, "ON again over a SMOOTH mesh")
        t.set_mesh_shading({0: "flat"})
        _assert_frames(_frames(rpt, t, **sizes), on, "FLAT again, still ON")
        assert _choice(rpt, t) & (LIGHT_BIT | SMOOTH_BIT) == LIGHT_BIT
        t.set_mesh_lights({1: False})
        u.set_mesh_shading({0: "flat"})
        _assert_frames(_frames(rpt, t, **sizes), never, "ON then OFF: the untouched context's frames")
        _assert_frames(_frames(rpt, u, **sizes), never, "the untouched context")
        assert _choice(rpt, t) == _choice(rpt, u) == choice
        assert _is_off(rpt, t, 1)
        # the frames do not depend on how they are dispatched
        t.set_mesh_lights({1: True})
        for disp in ((0, 12, 64, 0), (1, 1000, 1, 0), (2, 1000, 2, 7)):
            t.set_dispatch(*disp)
            _assert_frames(_frames(rpt, t, **sizes), on, str(disp))
        # an upload leaves every mesh OFF
        t.upload_scene()
        _assert_frames(_frames(rpt, t, **sizes), never, "after rpt_upload_scene")
        assert not _choice(rpt, t) & LIGHT_BIT and _is_off(rpt, t, 1)
    finally:
        t.close()
        u.close()


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------------
def test_every_answer_and_a_rejected_call_changes_nothing(rpt, torch_cuda):
    """Every answer of rpt_set_mesh_lights but two: RPT_ERR_HIP needs a failing runtime, and the 2^24 rule a scene of 16.7 million
    lights (a gigabyte of them) — tests/light_harness.cpp holds that rule's arithmetic and its place in the order."""
    A, lib = rpt._abi, rpt.lib()
    sizes = dict(sizes=((64, 48, 2),), resident=None)
    t = rpt.Tracer(_light_scene(), device=0, seed=5)
    try:
        off = _frames(rpt, t, **sizes)
        t.set_mesh_lights({1: True})
        ref = _frames(rpt, t, **sizes)
        table = t.mesh_light_table(1)
        assert not _same(ref[0], off[0])

        def items(*pairs):
            arr = (A.rpt_mesh_light * len(pairs))()
            for it, (m, mode) in zip(arr, pairs):
                it.mesh, it.mode = m, mode
            return arr

        ON, OFF = A.RPT_MESH_LIGHT_ON, A.RPT_MESH_LIGHT_OFF
        assert lib.rpt_set_mesh_lights(None, items((0, ON)), 1) == A.RPT_ERR_INVALID_ARG
        cases = [("NULL items", None, 1, "items is NULL"),
                 ("mesh out of range", items((0, ON), (2, ON)), 2, "item 1: mesh 2 out of range"),
                 ("named twice", items((0, ON), (1, OFF), (0, OFF)), 3, "item 2: mesh 0 is named twice"),
                 ("a mode that is neither", items((0, ON), (1, 2)), 2, "item 1: mode 2"),
                 ("out of range before the mode", items((7, 9)), 1, "item 0: mesh 7 out of range")]
        for what, arr, n, message in cases:
            assert lib.rpt_set_mesh_lights(t._h, arr, n) == A.RPT_ERR_INVALID_ARG, what
            err = lib.rpt_last_error(t._h).decode()
            assert err.startswith("rpt_set_mesh_lights: ") and message in err, (what, err)
            assert _is_off(rpt, t, 0), "%s: mesh 0 is still OFF" % what
            _assert_same_tables({1: t.mesh_light_table(1)}, {1: table}, what)
            _assert_frames(_frames(rpt, t, **sizes), ref, what)
        assert lib.rpt_set_mesh_lights(t._h, None, 0) == A.RPT_OK      # nothing to do
        _assert_frames(_frames(rpt, t, **sizes), ref, "n_items == 0")
        # a scene without RPT_SCENE_ANYHIT_USES_MAX_DIST: unsupported, before the items are looked at
        t.scene().any_hit_uses_max_dist = False
        t.upload_scene()
        plain = _frames(rpt, t, **sizes)
        for arr, n in ((items((1, ON)), 1), (None, 1), (items((9, 9)), 1), (None, 0)):
            assert lib.rpt_set_mesh_lights(t._h, arr, n) == A.RPT_ERR_UNSUPPORTED
            assert b"RPT_SCENE_ANYHIT_USES_MAX_DIST" in lib.rpt_last_error(t._h)
        _assert_frames(_frames(rpt, t, **sizes), plain, "after the unsupported calls")
        assert not _choice(rpt, t) & LIGHT_BIT
        # without a mesh scene
        t._scene = rpt.AnalyticalScene()
        t.upload_scene()
        buf = rpt.ColorBuffer(32, 24)
        t.render_n(buf, 1)
        before = buf.image().copy()
        assert lib.rpt_set_mesh_lights(t._h, items((0, ON)), 1) == A.RPT_ERR_NO_SCENE
        assert lib.rpt_set_mesh_lights(t._h, None, 0) == A.RPT_ERR_NO_SCENE        # no scene comes before n_items == 0
        cdf = np.zeros(2, np.uint64)
        e, area = C.c_int32(0), C.c_float(0.0)
        assert lib.rpt_download_mesh_light_table(t._h, 0, cdf.ctypes.data, 2, C.byref(e), C.byref(area)) == A.RPT_ERR_NO_SCENE
        dummy = torch_cuda.zeros(16, dtype=torch_cuda.float32, device="cuda")
        assert lib.rpt_debug_mesh_light_sample(t._h, dummy.data_ptr(), 1, dummy.data_ptr(), None) == A.RPT_ERR_NO_SCENE
        buf = rpt.ColorBuffer(32, 24)
        t.render_n(buf, 1)
        assert _same(buf.image(), before)
    finally:
        t.close()


# ---- 6. unbiased, and worth having ------------------------------------------------------------------------------------------------
K_FRAMES = 1024


def test_on_and_off_estimate_the_same_integral_and_on_with_less_variance(rpt, torch_cuda):
    """scenes.mesh_light_scene() at 32 x 24, K one-sample frames with seeds 1000 .. 1000 + K - 1, the lamp OFF and then ON; per
    frame the mean over all pixels and the three colour channels.  The means of the two runs agree within 5 standard errors (of
    their difference: the root of the sum of the two runs' squared standard errors, each from its own K per-frame means), the OFF
    run's standard error is below 5 % of its mean, and the ON run's per-frame means have the lower variance.
    Measured on an MI355X with K = 256 (seeds 1000 .. 1255): OFF mean 0.036764, standard error 0.002567 (6.98 % of the mean: too
    many for the 5 % this test asks, so 256 frames are too few); ON mean 0.036999, standard error 0.000067; the means 0.09 standard
    errors apart; variance ratio ON / OFF 0.0007.  The OFF run's per-frame standard deviation is 1.12 of its mean (many frames of
    768 one-sample pixels find the 0.09-square lamp not once), so K frames leave 1.12 / sqrt(K): 4.9 % at 512, too close to the
    bound to rely on, 3.5 % at 1 024.  Hence K = 1 024; the test prints its own figures (pytest -s)."""
    w, h = 32, 24
    t = rpt.Tracer(_light_scene(), device=0, seed=1000)

    def run():
        means = []
        for k in range(K_FRAMES):
            t.seed = 1000 + k
            buf = rpt.ColorBuffer(w, h)
            t.render_n(buf, 1)
            means.append(float(np.asarray(buf.image(), np.float64)[..., :3].mean()))
        return np.array(means)

    try:
        off = run()
        assert not _choice(rpt, t) & LIGHT_BIT
        t.set_mesh_lights({1: True})
        on = run()
        assert _choice(rpt, t) & LIGHT_BIT
    finally:
        t.close()
    se_off, se_on = off.std(ddof=1) / np.sqrt(K_FRAMES), on.std(ddof=1) / np.sqrt(K_FRAMES)
    ratio = on.var(ddof=1) / off.var(ddof=1)
    print("mesh lights, K = %d: OFF mean %.6f se %.6f (%.2f %%), ON mean %.6f se %.6f, variance ratio ON / OFF %.4f, difference %.2f se"
          % (K_FRAMES, off.mean(), se_off, 100 * se_off / off.mean(), on.mean(), se_on, ratio, abs(on.mean() - off.mean()) / np.hypot(se_off, se_on)))
    assert off.mean() > 0 and se_off < 0.05 * off.mean(), "K is too small for the OFF run"
    assert abs(on.mean() - off.mean()) <= 5.0 * np.hypot(se_off, se_on)
    assert ratio < 1.0


# ---- 7. multi-rank on one GPU -----------------------------------------------------------------------------------------------------
def test_a_device_listed_twice_renders_the_one_context_frame(rpt, torch_cuda):
    w, h, spp = 64, 48, 4
    s = _light_scene(sphere_light=True)
    t = rpt.Tracer(s, device=0, seed=9)
    try:
        t.set_mesh_lights({1: True})
        t.render_resident(w, h, spp)
        ref = t.resident_to_host(w, h).pixels.copy()
        table = t.mesh_light_table(1)
    finally:
        t.close()
    m = rpt.Tracer(_light_scene(sphere_light=True), devices=[0, 0], seed=9)
    try:
        m.set_mesh_lights({1: True})
        m.render_resident(w, h, spp)
        assert _same(m.resident_to_host(w, h).pixels.reshape(h, w, 4), ref.reshape(h, w, 4)), "device listed twice"
        _assert_same_tables({1: m.mesh_light_table(1)}, {1: table}, "device listed twice")
        moved = np.asarray(s.meshes[1][0], F) + F(0.125)
        m.update_meshes({1: moved})
        _assert_tables(m, (1,), "device listed twice, after a move")
        m.render_resident(w, h, spp)
        assert np.isfinite(m.resident_to_host(w, h).pixels).all()
    finally:
        m.close()
