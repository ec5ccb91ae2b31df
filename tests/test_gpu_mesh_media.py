"""Mesh media on the device (include/rpt.h, "mesh media"), bit for bit where the statement allows it: the probe of the join — which
medium a winning triangle carries, dot(l, G) against the FLAT normal and in_medium after step 4 — equals a numpy float32 restatement
over 4096 rays on a SMOOTH, normal-mapped mesh, through the walk and the ordered loop; a white ABSORB medium and a zero-density
EMISSIVE one render the frames without a medium in each of the eight forms, with rpt_debug_mesh_form saying 28 .. 35 and bit 24 of
rpt_debug_kernel_choice set, so the new kernels ran; setting every medium back to NONE returns the old form and the old frames, and
a scene on which the call was never made reports the form it always had; every rejected call says why and is followed by the render
of before; every kind of move gives the frames of a fresh upload plus the same set call; rpt_download_mesh_medium returns what was
set; Russian roulette renders and the relaxed forms stay refused; and with a SCATTER fog in the icosphere the lamp ON and OFF, and
the sky SAMPLED and BACKGROUND_ONLY, estimate one mean.  Scenes: scenes.mesh_media_scene (82 triangles); frames 64 x 48 and a
ragged 37 x 21 at 1 and 5 samples."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_mesh import _mesh_tris, _rays, brute_force
from test_gpu_mesh_compose_f64 import CASES, inputs
from test_gpu_mesh_light import MATRIX, _lit_small_scene
from test_gpu_mesh_material_map_f64 import mesh_form, set_composed
from test_gpu_mesh_update import _assert_frames, _choice, _frames, _same, _with_vertices
from test_mesh_media_host import MED_FORM_FIRST, NO_MEDIUM, restate_side

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = dict(sizes=((64, 48, 1), (64, 48, 5), (37, 21, 1), (37, 21, 5)), resident=None)
ONE = dict(sizes=((64, 48, 1),), resident=None)
MEDIA_BIT = 1 << 24
WHITE = dict(type="absorb", density=7.5, color=(1.0, 1.0, 1.0))
DARK = dict(type="emissive", density=0.0, color=(0.3, 0.6, 0.9))
AMBER = dict(type="absorb", density=3.0, color=(0.9, 0.45, 0.3))
FOG = dict(type="scatter", density=2.5, color=(0.85, 0.9, 0.95), anisotropy=0.6)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def form_of(case):
    """28 .. 35: the medium over the emission-mapped form over the kernel the composed file's case runs."""
    return MED_FORM_FIRST + sorted(CASES).index(case)


def _glass_scene():
    from rust_pathtracer_amd import scenes
    return scenes.mesh_media_scene(None)[0]


# ---- 1. the probe -------------------------------------------------------------------------------------------------------------------
def _media_query(rpt, torch, tracer, rays9, flags):
    n = len(rays9)
    dev = torch.from_numpy(np.ascontiguousarray(rays9, dtype=F)).cuda()
    out = torch.full((n, 4), 0x55, dtype=torch.int32, device="cuda")
    rpt._lib.check(rpt.lib().rpt_debug_mesh_media_query(tracer._h, dev.data_ptr(), n, out.data_ptr(), flags, None), tracer._h)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def test_the_probe_equals_the_numpy_restatement(rpt, torch_cuda):
    """This test fails without the feature, at its set_mesh_media.  4096 rays — test_gpu_mesh's hard cases, rays in a triangle's
    plane included — on the composed file's case E inputs (mesh 0 SMOOTH, both meshes normal-mapped), the medium on mesh 0 only.
    Half of the `l` are grazing: a vector of the winning triangle's plane plus a few ulps of its normal, so that dot(l, G) lies
    within a few ulps of 0 on both sides; a bent normal in G's place would give other words."""
    s = _glass_scene()
    tris = _mesh_tris(s)
    rng = np.random.default_rng(9100)
    rays = _rays(tris, 4096, rng)
    index, = brute_force(tris, rays, False)[1:2]
    l = rng.normal(size=(len(rays), 3))
    k = np.maximum(index, 0)
    e1, e2 = (tris[k, 1] - tris[k, 0]).astype(np.float64), (tris[k, 2] - tris[k, 0]).astype(np.float64)
    g = np.cross(e1, e2)
    g /= np.maximum(np.linalg.norm(g, axis=1), 1e-300)[:, None]
    graze = rng.uniform(-1, 1, (len(rays), 2))
    in_plane = graze[:, :1] * e1 + graze[:, 1:] * e2
    in_plane /= np.maximum(np.linalg.norm(in_plane, axis=1), 1e-300)[:, None]
    l[::2] = (in_plane + g * (rng.integers(-4, 5, (len(rays), 1)) * 2.0 ** -24))[::2]
    rays9 = np.concatenate([rays[:, :6], l.astype(F)], 1).astype(F)
    want_side, flat_differs = restate_side(s, tris, rays9, index)
    mesh0 = (index >= 0) & (index < 80)
    want_ord = np.where(mesh0, 0, NO_MEDIUM).astype(np.uint32)
    want_in = (mesh0 & (want_side < 0)).astype(np.uint32)
    t = rpt.Tracer(s, device=0, seed=2)
    try:
        set_composed(t, inputs(s, "E"))
        r1 = torch_cuda.zeros(9, device="cuda")
        o1 = torch_cuda.zeros(4, dtype=torch_cuda.int32, device="cuda")
        assert rpt.lib().rpt_debug_mesh_media_query(t._h, r1.data_ptr(), 1, o1.data_ptr(), 0, None) == rpt._abi.RPT_ERR_INVALID_ARG
        assert b"no mesh carries a medium" in rpt.lib().rpt_last_error(t._h)
        t.set_mesh_media({0: FOG})
        for brute in (False, True):
            got = _media_query(rpt, torch_cuda, t, rays9, rpt._abi.RPT_MESH_QUERY_BRUTE if brute else 0)
            got_i = got[:, 0].astype(np.int64) - (got[:, 0] == 0xFFFFFFFF) * (1 << 32)
            assert np.array_equal(got_i, index), "index (brute %s): %d rays differ" % (brute, int((got_i != index).sum()))
            assert np.array_equal(got[:, 1], want_ord), "the medium ordinal (brute %s)" % brute
            bad = np.nonzero(got[:, 2] != want_side.view(np.uint32))[0]
            assert len(bad) == 0, "dot(l, G) (brute %s): %d rays differ, first %s: got %s want %s" % (
                brute, len(bad), bad[:3], got[bad[:3], 2].view(F), want_side[bad[:3]])
            assert np.array_equal(got[:, 3], want_in), "in_medium (brute %s)" % brute
        hit = index >= 0
        near = hit & (np.abs(want_side) < 1e-6)
        assert mesh0.mean() > 0.1 and (index >= 80).sum() >= 10 and (~hit).sum() > 100, "both meshes and misses occur"
        assert near.sum() > 500 and (want_side[near] < 0).sum() > 100 and (want_side[near] > 0).sum() > 100, "grazing on both sides"
        assert 0.2 < want_in[mesh0].mean() < 0.8 and not want_in[~mesh0].any()
        assert flat_differs > 0.5, "the smooth normal is not the flat one on most hits of mesh 0: a wrong normal would show"
        t.set_mesh_media({0: None, 1: AMBER})                         # the ordinal moves to the lamp
        got = _media_query(rpt, torch_cuda, t, rays9, 0)
        assert np.array_equal(got[:, 1], np.where(index >= 80, 0, NO_MEDIUM).astype(np.uint32))
        assert np.array_equal(got[:, 3], ((index >= 80) & (want_side < 0)).astype(np.uint32))
    finally:
        t.close()


# ---- 2. identities, in each of the eight forms ------------------------------------------------------------------------------------------
def test_expf_of_minus_zero_is_one(oracle):
    """What the white ABSORB identity rests on: (1 - 1) * seg * density = 0, its negation -0, and rpt_expf(-0.0f) exactly 1."""
    e = oracle.math(7, np.array([-0.0, 0.0], F))
    assert e.view(np.uint32).tolist() == [0x3F800000, 0x3F800000]


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_white_absorb_and_a_dark_emissive_medium_are_the_frames_without_a_medium(rpt, torch_cuda, case):
    """The glass icosphere under the composed file's case (A .. H: the eight textured forms).  ABSORB of colour (1, 1, 1) at any
    density multiplies by exp(-0) = 1; EMISSIVE of density 0 adds 0; neither draws a number.  The base form's frame is the
    reference; a coloured ABSORB medium and a fog are no identities; every medium back to NONE is the old form and the old frames."""
    s = _glass_scene()
    t = rpt.Tracer(s, device=0, seed=4)
    try:
        set_composed(t, inputs(s, case))
        plain = _frames(rpt, t, **SIZES)
        base = mesh_form(rpt, t)
        assert base < 28 and not _choice(rpt, t) & MEDIA_BIT
        assert np.isfinite(plain[0]).all() and plain[0][..., :3].mean() > 0.005
        for what, medium in (("white ABSORB", WHITE), ("zero-density EMISSIVE", DARK)):
            t.set_mesh_media({0: medium, 1: medium})
            _assert_frames(_frames(rpt, t, **SIZES), plain, "case %s: %s" % (case, what))
            assert mesh_form(rpt, t) == form_of(case), "the media kernel ran"
            assert _choice(rpt, t) & MEDIA_BIT
        seen = []
        for medium in (AMBER, FOG, dict(type="emissive", density=0.5, color=(0.2, 0.6, 0.9))):
            t.set_mesh_media({0: medium, 1: None})
            seen.append(_frames(rpt, t, **ONE)[0])
            assert mesh_form(rpt, t) == form_of(case) and np.isfinite(seen[-1]).all()
            assert not _same(seen[-1], plain[0]), "case %s: %s changes the frame" % (case, medium["type"])
        assert not _same(seen[0], seen[1]) and not _same(seen[1], seen[2])
        t.set_mesh_media({0: None})
        _assert_frames(_frames(rpt, t, **SIZES), plain, "case %s: every medium NONE" % case)
        assert mesh_form(rpt, t) == base and not _choice(rpt, t) & MEDIA_BIT
    finally:
        t.close()


def test_the_forms_of_the_cases_are_28_to_35():
    assert [form_of(c) for c in sorted(CASES)] == list(range(28, 36))


def test_a_bare_scene_reaches_the_media_form_and_returns_to_its_own(rpt, torch_cuda):
    """No texture, no mesh ON, nothing SMOOTH: the flat form (11), then form 28 through the media's own empty tables, then 11 again.
    A scene on which the call was never made reports the form it always had.  Step by step the features below form 28 arrive while
    the medium stays: SMOOTH, the lamp ON, a texture — the white medium stays an identity under each."""
    from rust_pathtracer_amd import scenes
    s = _glass_scene()
    t = rpt.Tracer(s, device=0, seed=5)
    try:
        plain = _frames(rpt, t, **SIZES)
        assert mesh_form(rpt, t) == 11
        t.set_mesh_media({0: WHITE})
        _assert_frames(_frames(rpt, t, **SIZES), plain, "a white medium on the bare scene")
        assert mesh_form(rpt, t) == 28 and _choice(rpt, t) & MEDIA_BIT
        t.set_mesh_media({0: AMBER})
        amber = _frames(rpt, t, **SIZES)
        assert not _same(amber[0], plain[0]) and np.isfinite(amber[0]).all()
        t.set_mesh_media({0: None})
        _assert_frames(_frames(rpt, t, **SIZES), plain, "NONE again")
        assert mesh_form(rpt, t) == 11
        uv = scenes.spherical_uvs(np.asarray(s.meshes[0][0], F), (0.0, 0.0, 0.0))
        steps = (("smooth", lambda x: x.set_mesh_shading({0: "smooth"})), ("the lamp ON", lambda x: x.set_mesh_lights({1: True})),
                 ("a texture", lambda x: x.set_mesh_textures({0: dict(uvs=uv, texels=scenes.checker_texture(4, 4), wrap="repeat", filter="nearest", gamma=1.0)})))
        for what, step in steps:
            step(t)
            t.set_mesh_media({0: None})
            want = _frames(rpt, t, **ONE)
            assert mesh_form(rpt, t) < 28
            t.set_mesh_media({0: WHITE})
            _assert_frames(_frames(rpt, t, **ONE), want, "a white medium under %s" % what)
            assert mesh_form(rpt, t) == 28
        t.upload_scene()                                             # an upload drops every medium
        _assert_frames(_frames(rpt, t, **ONE), plain[:1], "after an upload")
        assert mesh_form(rpt, t) == 11 and t.download_mesh_medium(0)["type"] is None
    finally:
        t.close()
    b = rpt.Tracer(_glass_scene(), device=0, seed=5)                  # never touched
    try:
        _assert_frames(_frames(rpt, b, **SIZES), plain, "a context on which the call was never made")
        assert mesh_form(rpt, b) == 11 and not _choice(rpt, b) & MEDIA_BIT
    finally:
        b.close()


def test_roulette_renders_and_the_relaxed_forms_stay_refused(rpt, torch_cuda):
    A = rpt._abi
    t = rpt.Tracer(_glass_scene(), device=0, seed=6)
    try:
        t.set_mesh_media({0: FOG})
        px = np.zeros((48, 64, 4), F)
        lib = rpt.lib()
        assert lib.rpt_render(t._h, px.ctypes.data, 64, 48, 0, 2, 6, A.RPT_RENDER_RUSSIAN_ROULETTE) == A.RPT_OK
        again = np.zeros((48, 64, 4), F)
        assert lib.rpt_render(t._h, again.ctypes.data, 64, 48, 0, 2, 6, A.RPT_RENDER_RUSSIAN_ROULETTE) == A.RPT_OK
        assert mesh_form(rpt, t) == 28 and np.isfinite(px).all() and px[..., :3].mean() > 0.005 and _same(px, again)
        for flag in (A.RPT_RENDER_FAST_MATH, A.RPT_RENDER_NESTED_LOOPS, A.RPT_RENDER_SMALL_COMPACT):
            assert lib.rpt_render(t._h, again.ctypes.data, 64, 48, 0, 1, 6, flag) == A.RPT_ERR_UNSUPPORTED
    finally:
        t.close()


# ---- 3. answers -------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_say_why_and_change_nothing(rpt, torch_cuda):
    A, lib = rpt._abi, rpt.lib()
    from rust_pathtracer_amd import scenes
    t = rpt.Tracer(_glass_scene(), device=0, seed=10)
    try:
        t.set_mesh_media({0: FOG})
        ref = _frames(rpt, t, **ONE)
        held = t.download_mesh_medium(0)

        def items(*rows):
            arr = (A.rpt_mesh_medium * len(rows))()
            for it, r in zip(arr, rows):
                r = dict(dict(mesh=0, medium_type=A.RPT_MEDIUM_ABSORB, density=1.0, color=(0.5, 0.5, 0.5), anisotropy=0.0), **r)
                it.mesh, it.medium_type, it.density, it.anisotropy = r["mesh"], r["medium_type"], r["density"], r["anisotropy"]
                it.color[0], it.color[1], it.color[2] = r["color"]
            return arr

        nan, inf = float("nan"), float("inf")
        # in the stated order; each case but the last carries the NEXT check's fault as well, so the order itself is held
        cases = [("NULL items", None, 1, "items is NULL"),
                 ("mesh out of range", items(dict(mesh=2, medium_type=9)), 1, "mesh 2 out of range"),
                 ("named twice", items(dict(), dict(medium_type=9)), 2, "item 1: mesh 0 is named twice"),
                 ("type", items(dict(medium_type=4, density=-1.0)), 1, "medium_type 4"),
                 ("negative density", items(dict(density=-1.0, color=(nan, 0, 0))), 1, "density -1"),
                 ("infinite density", items(dict(density=inf, color=(nan, 0, 0))), 1, "density inf"),
                 ("nan density", items(dict(density=nan, color=(nan, 0, 0))), 1, "density"),
                 ("colour", items(dict(color=(0.5, inf, 0.5), anisotropy=nan)), 1, "the colour is not finite"),
                 ("anisotropy", items(dict(anisotropy=nan)), 1, "the anisotropy is not finite"),
                 ("a NONE item is checked as well", items(dict(medium_type=A.RPT_MEDIUM_NONE, density=-2.0)), 1, "density -2"),
                 ("a good item before a bad one stores nothing", items(dict(mesh=1), dict(mesh=0, anisotropy=inf)), 2, "item 1: mesh 0: the anisotropy")]
        for what, arr, n, says in cases:
            assert lib.rpt_set_mesh_media(t._h, arr, n) == A.RPT_ERR_INVALID_ARG, what
            err = lib.rpt_last_error(t._h).decode()
            assert err.startswith("rpt_set_mesh_media: ") and says in err, (what, err)
            _assert_frames(_frames(rpt, t, **ONE), ref, "after the rejected call: %s" % what)
        assert t.download_mesh_medium(0) == held and t.download_mesh_medium(1)["type"] is None
        assert mesh_form(rpt, t) == 28
        assert lib.rpt_set_mesh_media(t._h, None, 0) == A.RPT_OK
        _assert_frames(_frames(rpt, t, **ONE), ref, "n_items == 0 does nothing")
        out = A.rpt_mesh_medium()
        assert lib.rpt_download_mesh_medium(t._h, 2, C.byref(out)) == A.RPT_ERR_INVALID_ARG and b"mesh 2 out of range" in lib.rpt_last_error(t._h)
        assert lib.rpt_download_mesh_medium(t._h, 0, None) == A.RPT_ERR_INVALID_ARG
        b = rpt.Tracer(scenes.six_primitive_scene(), device=0, seed=1)      # no scene with meshes
        try:
            assert lib.rpt_set_mesh_media(b._h, items(dict()), 1) == A.RPT_ERR_NO_SCENE
            assert lib.rpt_set_mesh_media(b._h, None, 1) == A.RPT_ERR_NO_SCENE             # no scene comes before NULL items
            assert lib.rpt_download_mesh_medium(b._h, 0, C.byref(out)) == A.RPT_ERR_NO_SCENE
        finally:
            b.close()
    finally:
        t.close()


def test_download_returns_what_was_set(rpt, torch_cuda):
    t = rpt.Tracer(_glass_scene(), device=0, seed=11)
    try:
        none = dict(type=None, density=F(0), color=(F(0), F(0), F(0)), anisotropy=F(0))
        assert t.download_mesh_medium(0) == none and t.download_mesh_medium(1) == none, "before any call"
        t.set_mesh_media({0: dict(type="scatter", density=2.5, color=(0.1, 0.2, 0.3), anisotropy=0.97)})
        got = t.download_mesh_medium(0)
        assert got == dict(type="scatter", density=F(2.5), color=(F(0.1), F(0.2), F(0.3)), anisotropy=F(0.9)), got
        assert t.download_mesh_medium(1) == none
        t.set_mesh_media({1: dict(type="emissive", density=0.25, color=(3.0, 2.0, 1.0), anisotropy=-5.0)})      # mesh 0 stays
        assert t.download_mesh_medium(0) == got
        assert t.download_mesh_medium(1) == dict(type="emissive", density=F(0.25), color=(F(3), F(2), F(1)), anisotropy=F(-0.9))
        t.set_mesh_media({0: dict(type=None, density=4.0, color=(1.0, 1.0, 1.0))})           # NONE drops the other fields
        assert t.download_mesh_medium(0) == none and t.download_mesh_medium(1)["type"] == "emissive"
    finally:
        t.close()


# ---- 4. moves -----------------------------------------------------------------------------------------------------------------------
def _moving_scene():
    from rust_pathtracer_amd import scenes
    s = _lit_small_scene()                                            # an icosphere of 320 and an emissive torus of 256 triangles
    s.materials[0] = scenes.full_material(rgb=(0.95, 0.95, 0.95), roughness=0.05, spec_trans=1.0, ior=1.45)
    return s


def _set_up_moving(t):
    t.set_mesh_lights({1: True})
    t.set_mesh_media({0: FOG, 1: dict(type="emissive", density=0.3, color=(0.4, 0.1, 0.1))})


def _fresh(rpt, arrays):
    """The yardstick: a fresh context that uploads the scene with these positions and then makes the same set calls."""
    b = rpt.Tracer(_with_vertices(_moving_scene, arrays), device=0, seed=8)
    try:
        _set_up_moving(b)
        return _frames(rpt, b, **SIZES)
    finally:
        b.close()


@pytest.mark.parametrize("form", ["update", "rebuild", "update_device", "rebuild_device"])
def test_media_frames_follow_every_kind_of_move(rpt, torch_cuda, form):
    from rust_pathtracer_amd import scenes
    s = _moving_scene()
    rest = [np.array(v, F, copy=True) for v, _, _ in s.meshes]
    t = rpt.Tracer(s, device=0, seed=8)
    try:
        _set_up_moving(t)
        still = _frames(rpt, t, **SIZES)
        _assert_frames(still, _fresh(rpt, rest), "before any move")
        held = [t.download_mesh_medium(m) for m in (0, 1)]
        moved = scenes.mesh_scene_moved(s, 0.7)
        if form == "update":
            t.update_meshes(dict(enumerate(moved)))
        elif form == "rebuild":
            t.rebuild_meshes(dict(enumerate(moved)))
        else:                                                         # the device forms: mesh 0 as it is, mesh 1 through a 3x4 matrix
            src = {0: torch_cuda.from_numpy(moved[0]).to("cuda:0"), 1: (torch_cuda.from_numpy(rest[1]).to("cuda:0"), MATRIX)}
            (t.update_meshes_device if form == "update_device" else t.rebuild_meshes_device)(src)
        now = [t.mesh_vertices(m) for m in (0, 1)]
        got = _frames(rpt, t, **SIZES)
        assert mesh_form(rpt, t) == 28
        _assert_frames(got, _fresh(rpt, now), "%s: against a fresh upload" % form)
        assert not _same(got[0], still[0])
        assert [t.download_mesh_medium(m) for m in (0, 1)] == held, "a move leaves the media alone"
    finally:
        t.close()


# ---- 5. unbiased ------------------------------------------------------------------------------------------------------------------
K_FRAMES = 256


def _means(rpt, t, seed0, w=32, h=24):
    means = []
    for k in range(K_FRAMES):
        t.seed = seed0 + k
        buf = rpt.ColorBuffer(w, h)
        t.render_n(buf, 1)
        means.append(float(np.asarray(buf.image(), np.float64)[..., :3].mean()))
    return np.array(means)


def _report(what, names, off, on):
    se_off, se_on = off.std(ddof=1) / np.sqrt(K_FRAMES), on.std(ddof=1) / np.sqrt(K_FRAMES)
    ratio = on.var(ddof=1) / off.var(ddof=1)
    apart = abs(on.mean() - off.mean()) / np.hypot(se_off, se_on)
    print("mesh media, %s, K = %d: %s mean %.6f se %.6f, %s mean %.6f se %.6f, variance ratio %s / %s %.4f, difference %.2f se"
          % (what, K_FRAMES, names[0], off.mean(), se_off, names[1], on.mean(), se_on, names[1], names[0], ratio, apart))
    assert off.mean() > 0 and on.mean() > 0
    assert abs(on.mean() - off.mean()) <= 5.0 * np.hypot(se_off, se_on)
    assert ratio < 1.0


def test_the_lamp_on_and_off_estimate_one_mean_through_a_fog(rpt, torch_cuda):
    """scenes.mesh_media_scene("scatter") at 32 x 24, K = 256 one-sample frames with seeds 3000 .. 3255, the lamp mesh OFF and then
    ON; per frame the mean over all pixels and the three colour channels.  The mesh-light test's criterion: the two runs' means
    differ by at most 5 standard errors of their difference, and the ON run's per-frame means have the lower variance.  A light
    estimate at a scatter point that used another pick, an offset origin or a wrong attenuation would shift the ON mean alone.
    The test prints its figures (pytest -s).  Measured on an MI355X: OFF mean 0.051169, standard error 0.002955; ON mean 0.051568,
    standard error 0.001122; the means 0.13 standard errors apart; variance ratio ON / OFF 0.1441."""
    from rust_pathtracer_amd import scenes
    s, media = scenes.mesh_media_scene("scatter")
    t = rpt.Tracer(s, device=0, seed=3000)
    try:
        t.set_mesh_media(media)
        off = _means(rpt, t, 3000)
        assert mesh_form(rpt, t) == 28
        t.set_mesh_lights({1: True})
        on = _means(rpt, t, 3000)
        assert mesh_form(rpt, t) == 28
    finally:
        t.close()
    _report("the lamp", ("OFF", "ON"), off, on)


def test_the_sky_sampled_and_background_only_estimate_one_mean_through_a_fog(rpt, torch_cuda):
    """The same under scenes.mesh_env_scene()'s sky on the glass scene, the lamp OFF: BACKGROUND_ONLY, then SAMPLED — the pick's last
    light, never attenuated (its distance is infinite).  Measured on an MI355X: BACKGROUND_ONLY mean 4.121965, standard error
    0.148879; SAMPLED mean 4.000801, standard error 0.013657; 0.81 standard errors apart; variance ratio SAMPLED / BACKGROUND_ONLY
    0.0084."""
    from rust_pathtracer_amd import scenes
    s, media = scenes.mesh_media_scene("scatter")
    s.lights = []
    image = scenes.mesh_env_scene()[1]
    t = rpt.Tracer(s, device=0, seed=4000)
    try:
        t.set_mesh_media(media)
        t.set_environment(image, sampled=False)
        off = _means(rpt, t, 4000)
        assert mesh_form(rpt, t) == 29
        t.set_environment(image, sampled=True)
        on = _means(rpt, t, 4000)
        assert mesh_form(rpt, t) == 29
    finally:
        t.close()
    _report("the sky", ("BACKGROUND_ONLY", "SAMPLED"), off, on)
