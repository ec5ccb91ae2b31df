"""Radiance queries on an MI355X (include/rpt.h, "radiance queries"): rpt_radiance_device / rpt_radiance / rpt_camera_sample_rays_device.

1. radiance over the camera's sample rays leaves the very words a render leaves, in all 36 render forms, for frames 0, 1 and 1000
   (frame 1 from a non-zero buffer) at 50 x 37 — 1 850 rays, a ragged last workgroup.  This fails without the feature.
2. camera_sample_rays equals the GEN_RAY probe fed the oracle's two first draws of each pixel's stream.
3. one launch of S samples equals S one-sample launches, on rays of mixed cost, in the heaviest form and on the flat scene; a call
   above kMaxSppPerLaunch equals the two calls that split it.
4. ragged batches, first_index, the host form, a second stream.
5. a miss is the constant background's three words and alpha 1.
6. the four move calls and a setter (media on, off) are seen: the result equals a fresh upload's.
7. rejected calls return their status and write nothing; a radiance call changes no frame and not rpt_debug_mesh_form.

Everything is compared as uint32 words: this file has no tolerance."""
import ctypes as C

import numpy as np
import pytest

import query_np as Q
import test_mesh_frames_f64 as TF
from query_np import MATRIX
from test_gpu_mesh_compose_f64 import CASES, inputs
from test_gpu_mesh_frames_f64 import FORMS, assert_form, open_tracer
from test_gpu_mesh_material_map_f64 import mesh_form, set_composed
from test_mesh_media_f64 import MEDIA
from test_mesh_media_f64 import scene as media_scene

pytestmark = pytest.mark.gpu
F = np.float32
SIZE = (50, 37)
N = SIZE[0] * SIZE[1]
FRAMES = (0, 1, 1000)
MAX_SPP = 512                                                       # kMaxSppPerLaunch (csrc/kernel_common.h)
PATTERN = 0x5A5A5A5A
MED_FORM_FIRST = 28
ALL_FORMS = sorted([(FORMS[k], k[0], k[1]) for k in FORMS] + [(MED_FORM_FIRST + i, "media", c) for i, c in enumerate(sorted(CASES))])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _words(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _open(rpt, stack, case, seed):
    """A Tracer that renders in the form of ALL_FORMS' entry (stack, case)."""
    if stack != "media":
        return open_tracer(rpt, stack, case, seed)
    s = media_scene()
    t = rpt.Tracer(s, device=0, seed=seed)
    set_composed(t, inputs(s, case))
    t.set_mesh_media({0: MEDIA[case]})
    return t


def _start(torch, frame):
    """The buffer a frame starts from, [N, 4] on the device: zeros for frame 0, else fixed non-zero values (alpha included)."""
    if frame == 0:
        return torch.zeros((N, 4), dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cpu").manual_seed(100 + frame)
    return (torch.rand((N, 4), generator=g, dtype=torch.float32) * 2.0 + 0.125).cuda()


def _render(rpt, torch, t, start, frame, spp=1):
    buf = rpt.DeviceColorBuffer(*SIZE)
    buf.pixels.copy_(start.view(buf.pixels.shape))
    buf.frames = frame
    t.render_n(buf, spp)
    torch.cuda.synchronize()
    return buf.pixels.cpu().numpy().reshape(N, 4)


# ---- 1. radiance over the camera's sample rays is the render ----------------------------------------------------------------------------
def test_all_36_forms_are_listed():
    assert [f for f, _, _ in ALL_FORMS] == list(range(36))


@pytest.mark.parametrize("form,stack,case", ALL_FORMS, ids=["form%02d" % f for f, _, _ in ALL_FORMS])
def test_radiance_over_the_camera_s_sample_rays_is_the_render(rpt, torch_cuda, form, stack, case):
    """All four words of every pixel, as uint32.  Wrong here: the stream key, the two discarded draws, the blend or its weight, the
    form choice, one empty table."""
    t = _open(rpt, stack, case, 3)
    try:
        for frame in FRAMES:
            start = _start(torch_cuda, frame)
            want = _render(rpt, torch_cuda, t, start, frame)
            assert_form(rpt, t, form) if form < MED_FORM_FIRST else None
            assert mesh_form(rpt, t) == form
            out = start.clone()
            rays = t.camera_sample_rays(SIZE[0], SIZE[1], frame)
            got = t.radiance(rays, frames_done=frame, out=out)
            torch_cuda.cuda.synchronize()
            assert got is out
            got = got.cpu().numpy()
            differ = (_words(got) != _words(want)).any(axis=1)
            assert not differ.any(), "form %d, frame %d: %d of %d pixels differ, first %s: %s against %s" % (
                form, frame, int(differ.sum()), N, np.nonzero(differ)[0][:3], got[differ][0], want[differ][0])
            assert np.isfinite(want).all() and (_words(want) != _words(start.cpu().numpy())).any(axis=1).all(), "the frame changed every pixel"
            assert mesh_form(rpt, t) == form, "rpt_debug_mesh_form is the last RENDER's"
    finally:
        t.close()


# ---- 2. the camera's sample rays ------------------------------------------------------------------------------------------------------------
def _gen_ray_probe(rpt, torch, tracer, px, py, offx, offy, width, height):
    A = rpt._abi
    rec = np.zeros((len(px), A.RPT_PROBE_IN_STRIDE), F)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = px, py, offx, offy
    dev = torch.from_numpy(rec).cuda()
    out = torch.empty(len(px), A.RPT_PROBE_OUT_STRIDE, dtype=torch.float32, device="cuda")
    params = np.array([width, height], F)
    rpt._lib.check(rpt.lib().rpt_probe_fn(tracer._h, A.RPT_PROBE_FN_GEN_RAY, dev.data_ptr(), out.data_ptr(), len(px), params.ctypes.data, None), tracer._h)
    torch.cuda.synchronize()
    return out.cpu().numpy()[:, 0:6]


@pytest.mark.parametrize("size", [(50, 37), (1, 1)], ids=["50x37", "1x1"])
def test_camera_sample_rays_equal_the_gen_ray_probe(rpt, oracle, torch_cuda, size):
    w, h = size
    seed, frame = 7, 5
    s = Q.small_scene()
    s.camera = rpt.Pinhole((2.0, 1.0, -3.0), (0.5, 0.0, 1.0), 35.0)
    t = rpt.Tracer(s, device=0, seed=seed)
    try:
        got = t.camera_sample_rays(w, h, frame)
        torch_cuda.cuda.synchronize()
        got = got.cpu().numpy()
        assert got.shape == (w * h, 8)
        # what a render launch computes for pixel (x, y), row 0 on top (csrc/kernel_common.h, pixel_coords), in float32
        y, x = np.divmod(np.arange(w * h), w)
        j = (h - 1 - y).astype(F)
        px = x.astype(F) / F(w)
        py = F(1.0) - (F(h) - j) / F(h)
        draws = np.stack([oracle.rng_f32(seed, frame, int(p), 2) for p in range(w * h)])
        want = _gen_ray_probe(rpt, torch_cuda, t, px, py, draws[:, 0], draws[:, 1], w, h)
        assert np.array_equal(_words(got[:, 0:3]), _words(want[:, 0:3])), "origins"
        assert np.array_equal(_words(got[:, 4:7]), _words(want[:, 3:6])), "directions: %d differ" % int((_words(got[:, 4:7]) != _words(want[:, 3:6])).any(axis=1).sum())
        assert (_words(got[:, 3]) == Q.INF_BITS).all() and not _words(got[:, 7]).any(), "max_dist is +inf, reserved 0"
        if w * h > 1:
            centre = t.camera_rays(w, h).cpu().numpy()
            assert (_words(centre[:, 4:7]) != _words(got[:, 4:7])).any(axis=1).mean() > 0.9, "the jitter is there"
            other = t.camera_sample_rays(w, h, frame + 1).cpu().numpy()
            assert (_words(other[:, 4:7]) != _words(got[:, 4:7])).any(axis=1).mean() > 0.9, "and depends on the frame"
    finally:
        t.close()


# ---- 3. one launch is its one-sample launches ------------------------------------------------------------------------------------------------
def _mixed_rays(scene, n, seed):
    """n rpt_rays of mixed cost, every one finite with a unit direction: a third aimed at the sky (from above the scene, upward), the
    rest from around the scene into its meshes (at points on random triangles).  -> ([n, 8] f32, which are the sky's)."""
    rng = np.random.default_rng(seed)
    tris = Q.mesh_tris(scene).astype(np.float64)
    verts = tris.reshape(-1, 3)
    lo, hi = verts.min(0), verts.max(0)
    centre, ext = 0.5 * (lo + hi), (hi - lo).max()
    tri = tris[rng.integers(0, len(tris), n)]
    w = rng.dirichlet([1, 1, 1], n)
    target = (w[:, :, None] * tri).sum(1)
    o = centre + rng.normal(size=(n, 3)) * ext
    o[:, 1] = np.abs(o[:, 1] - centre[1]) + centre[1]                # (above the floor)
    d = target - o
    sky = rng.random(n) < 1.0 / 3.0
    up = rng.normal(size=(n, 3))
    up[:, 1] = np.abs(up[:, 1]) + 0.5
    o[sky] = (np.array([centre[0], hi[1] + 2.0 * ext, centre[2]]) + rng.normal(size=(n, 3)))[sky]
    d[sky] = up[sky]
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    r8 = np.zeros((n, 8), F)
    r8[:, 0:3], r8[:, 4:7] = o.astype(F), d.astype(F)
    r8[:, 3] = F(3.0e38)
    assert np.isfinite(r8).all()
    return r8, sky


def _heaviest(rpt, seed):
    """media + environment + normal map + cutout: the case of form 35."""
    case = sorted(CASES)[35 - MED_FORM_FIRST]
    return _open(rpt, "media", case, seed)


@pytest.mark.parametrize("which", ["heaviest", "flat"])
def test_one_launch_is_its_one_sample_launches(rpt, torch_cuda, which):
    t = _heaviest(rpt, 3) if which == "heaviest" else open_tracer(rpt, "single", TF.FLAT + " composed", 3)
    try:
        r8, sky = _mixed_rays(t.scene(), N, 77)
        assert 0.25 < sky.mean() < 0.42
        dev = torch_cuda.from_numpy(r8).cuda()
        for earlier, n in ((0, 2), (0, 5), (0, 16), (3, 5)):
            one = torch_cuda.zeros((N, 4), dtype=torch_cuda.float32, device="cuda")
            if earlier:
                t.radiance(dev, spp=earlier, out=one)
            two = one.clone()
            t.radiance(dev, spp=n, frames_done=earlier, out=one)
            for k in range(n):
                t.radiance(dev, spp=1, frames_done=earlier + k, out=two)
            torch_cuda.cuda.synchronize()
            got, want = one.cpu().numpy(), two.cpu().numpy()
            assert np.isfinite(want).all() and want[:, :3].max() > 0.01
            differ = (_words(got) != _words(want)).any(axis=1)
            assert not differ.any(), "%s, %d samples on %d earlier: %d rays differ, first %s" % (which, n, earlier, int(differ.sum()), np.nonzero(differ)[0][:3])
        # a call above the samples one launch holds is the two calls that split it
        few = dev[:64].contiguous()
        one = t.radiance(few, spp=MAX_SPP + 3)
        two = t.radiance(few, spp=MAX_SPP)
        t.radiance(few, spp=3, frames_done=MAX_SPP, out=two)
        torch_cuda.cuda.synchronize()
        assert np.array_equal(_words(one.cpu().numpy()), _words(two.cpu().numpy())), "%d samples" % (MAX_SPP + 3)
    finally:
        t.close()


# ---- 4. batches and keys ------------------------------------------------------------------------------------------------------------------
def test_batches_keys_the_host_form_and_a_second_stream(rpt, torch_cuda):
    t = _heaviest(rpt, 5)
    try:
        r8, _ = _mixed_rays(t.scene(), 600, 78)
        dev = torch_cuda.from_numpy(r8).cuda()
        whole = t.radiance(dev, spp=2, frames_done=4)
        torch_cuda.cuda.synchronize()
        whole = _words(whole.cpu().numpy())
        assert len(np.unique(whole[:, 0])) > 300
        for n in (1, 255, 256, 257):
            guard = torch_cuda.full((n + 1, 4), 0.0, dtype=torch_cuda.float32, device="cuda")
            guard[n] = 123.0
            t.radiance(dev[:n].contiguous(), spp=2, frames_done=4, out=guard[:n])
            torch_cuda.cuda.synchronize()
            got = guard.cpu().numpy()
            assert np.array_equal(_words(got[:n]), whole[:n]) and (got[n] == 123.0).all(), "n = %d" % n
        for k in (0, 1, 300):
            part = t.radiance(dev[k:].contiguous(), spp=2, frames_done=4, first_index=k)
            torch_cuda.cuda.synchronize()
            assert np.array_equal(_words(part.cpu().numpy()), whole[k:]), "first_index = %d" % k
        wrapped = t.radiance(dev[:8].contiguous(), spp=2, frames_done=4, first_index=2 ** 32 - 3)     # indices ... 0xFFFFFFFF, 0, 1, ...: it wraps
        torch_cuda.cuda.synchronize()
        origin = torch_cuda.cat([dev[3:8], dev[3:8]]).contiguous()
        again = t.radiance(origin[:5].contiguous(), spp=2, frames_done=4, first_index=0)
        torch_cuda.cuda.synchronize()
        # rays 3 .. 7 of `wrapped` ran on stream indices 0 .. 4, as rays 0 .. 4 of `again` (the same rays) did
        assert np.array_equal(_words(wrapped.cpu().numpy())[3:8], _words(again.cpu().numpy()))
        host = t.radiance(r8, spp=2, frames_done=4)
        assert isinstance(host, np.ndarray) and np.array_equal(_words(host), whole), "the host form"
        acc = host.copy()
        assert t.radiance(r8, spp=1, frames_done=6, out=acc) is acc
        more = t.radiance(dev, spp=1, frames_done=6, out=torch_cuda.from_numpy(host).cuda())
        torch_cuda.cuda.synchronize()
        assert np.array_equal(_words(acc), _words(more.cpu().numpy())) and (_words(acc) != whole).any(), "out accumulates in place"
        side = torch_cuda.cuda.Stream()
        side.wait_stream(torch_cuda.cuda.current_stream())
        with torch_cuda.cuda.stream(side):
            other = t.radiance(dev, spp=2, frames_done=4)
        side.synchronize()
        assert np.array_equal(_words(other.cpu().numpy()), whole), "a second stream"
    finally:
        t.close()


# ---- 5. a miss is the background --------------------------------------------------------------------------------------------------------
def test_a_miss_is_the_background_exactly(rpt, torch_cuda):
    s = Q.small_scene()
    colour = (F(0.25), F(0.5), F(0.75))
    s.background = dict(kind=rpt._abi.RPT_BG_CONSTANT, colour_a=tuple(float(c) for c in colour), colour_b=(0.0, 0.0, 0.0), gamma=2.2, scale=1.0)
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        rng = np.random.default_rng(5)
        n = 300
        d = rng.normal(size=(n, 3))
        d[:, 1] = np.abs(d[:, 1]) + 0.2
        r7 = np.concatenate([np.array([0.0, 50.0, 0.0]) + rng.normal(size=(n, 3)), d, np.full((n, 1), 3.0e38)], 1).astype(F)
        r8 = Q.to_rpt_rays(r7)[:n]
        assert (t.trace(r8)["kind"] == Q.HIT_NONE).all(), "the rays miss everything"
        got = t.radiance(torch_cuda.from_numpy(r8).cuda())
        torch_cuda.cuda.synchronize()
        got = got.cpu().numpy()
        want = np.tile(np.array(colour + (F(1.0),), F), (n, 1))
        assert np.array_equal(_words(got), _words(want)), got[:2]
    finally:
        t.close()


# ---- 6. state ---------------------------------------------------------------------------------------------------------------------------
def _state_rays(scene):
    return _mixed_rays(scene, 2048, 9500)[0]


def _estimate(torch, t, r8):
    out = t.radiance(torch.from_numpy(r8).cuda(), spp=2)
    torch.cuda.synchronize()
    return _words(out.cpu().numpy())


@pytest.mark.parametrize("move", ["update_meshes", "rebuild_meshes", "update_meshes_device", "rebuild_meshes_device"])
def test_radiance_sees_every_move(rpt, torch_cuda, move):
    from rust_pathtracer_amd import scenes
    s = Q.small_scene()
    r8 = _state_rays(s)
    t = rpt.Tracer(s, device=0, seed=1)
    try:
        t.set_mesh_shading({0: "smooth"})
        before = _estimate(torch_cuda, t, r8)
        moved = scenes.mesh_scene_moved(s, 0.5)
        if move.endswith("_device"):
            getattr(t, move)({m: (torch_cuda.from_numpy(v).cuda(), MATRIX) for m, v in enumerate(moved)})
            held = [t.mesh_vertices(m) for m in range(len(moved))]
        else:
            getattr(t, move)(dict(enumerate(moved)))
            held = moved
        after = _estimate(torch_cuda, t, r8)
    finally:
        t.close()
    f = rpt.Tracer(Q.with_vertices(Q.small_scene, held), device=0, seed=1)
    try:
        f.set_mesh_shading({0: "smooth"})
        want = _estimate(torch_cuda, f, r8)
    finally:
        f.close()
    diff = (after != want).any(axis=1)
    assert not diff.any(), "%s: %d rays differ from a fresh upload, first %s" % (move, int(diff.sum()), np.nonzero(diff)[0][:3])
    assert (after != before).any(axis=1).mean() > 0.2, "the move matters"


def test_radiance_sees_a_setter_on_and_off(rpt, torch_cuda):
    s = media_scene()
    r8 = _state_rays(s)
    case = sorted(CASES)[0]
    t = rpt.Tracer(s, device=0, seed=2)
    try:
        none = _estimate(torch_cuda, t, r8)
        t.set_mesh_media({0: MEDIA[case]})
        on = _estimate(torch_cuda, t, r8)
        assert (on != none).any(axis=1).mean() > 0.02, "the medium matters"
        f = rpt.Tracer(s, device=0, seed=2)
        try:
            f.set_mesh_media({0: MEDIA[case]})
            assert np.array_equal(_estimate(torch_cuda, f, r8), on), "ON: a fresh context with the medium set"
        finally:
            f.close()
        t.set_mesh_media({0: None})
        assert np.array_equal(_estimate(torch_cuda, t, r8), none), "OFF again: a context that never had a medium"
    finally:
        t.close()


# ---- 7. rejected calls, no side effects -----------------------------------------------------------------------------------------------
def test_rejected_calls_return_their_status_and_write_nothing(rpt, torch_cuda):
    A, lib = rpt._abi, rpt.lib()
    s = Q.small_scene()
    r8 = _state_rays(s)[:256].copy()
    dev = torch_cuda.from_numpy(r8).cuda()
    out = torch_cuda.full((257, 4), PATTERN, dtype=torch_cuda.int32, device="cuda")
    cam = torch_cuda.full((4 * 4 + 1, 8), PATTERN, dtype=torch_cuda.int32, device="cuda")
    p_r, p_o, p_c = dev.data_ptr(), out.data_ptr(), cam.data_ptr()

    def untouched():
        torch_cuda.cuda.synchronize()
        return bool((out == PATTERN).all() and (cam == PATTERN).all())

    def radiance_device(h, rays, n, o, spp=1, flags=0):
        return lib.rpt_radiance_device(h, rays, n, o, 0, spp, 1, 0, flags, None)

    def every_call(h, status, what):
        assert radiance_device(h, p_r, 256, p_o) == status, what
        assert lib.rpt_camera_sample_rays_device(h, 4, 4, 0, 1, p_c, None) == status, what
        o = np.full((256, 4), PATTERN, np.uint32)
        assert lib.rpt_radiance(h, r8.ctypes.data, 256, o.ctypes.data, 0, 1, 1, 0, 0) == status, what
        assert (o == PATTERN).all() and untouched(), what

    t = rpt.Tracer(s, device=0, seed=1)
    try:
        bad = A.RPT_ERR_INVALID_ARG
        assert radiance_device(None, p_r, 256, p_o) == bad and b"ctx is NULL" in lib.rpt_last_error(None)
        assert lib.rpt_camera_sample_rays_device(None, 4, 4, 0, 1, p_c, None) == bad and lib.rpt_radiance(None, r8.ctypes.data, 256, r8.ctypes.data, 0, 1, 1, 0, 0) == bad
        assert radiance_device(t._h, p_r + 4, 255, p_o) == bad and b"16-byte aligned" in lib.rpt_last_error(t._h)
        assert radiance_device(t._h, p_r, 256, p_o + 8) == bad
        assert lib.rpt_camera_sample_rays_device(t._h, 4, 4, 0, 1, p_c + 8, None) == bad
        assert radiance_device(t._h, p_r, 256, p_o, flags=1) == bad and b"reserved" in lib.rpt_last_error(t._h)
        o = np.full((256, 4), PATTERN, np.uint32)
        assert lib.rpt_radiance(t._h, r8.ctypes.data, 256, o.ctypes.data, 0, 1, 1, 0, 0x80000000) == bad and (o == PATTERN).all()
        assert radiance_device(t._h, None, 256, p_o) == bad and b"NULL array" in lib.rpt_last_error(t._h)
        assert radiance_device(t._h, p_r, 256, None) == bad
        assert lib.rpt_radiance(t._h, None, 3, o.ctypes.data, 0, 1, 1, 0, 0) == bad and lib.rpt_radiance(t._h, r8.ctypes.data, 3, None, 0, 1, 1, 0, 0) == bad
        assert lib.rpt_camera_sample_rays_device(t._h, 4, 4, 0, 1, None, None) == bad
        assert lib.rpt_camera_sample_rays_device(t._h, 0, 4, 0, 1, p_c, None) == bad and lib.rpt_camera_sample_rays_device(t._h, 4, 0, 0, 1, p_c, None) == bad
        assert radiance_device(t._h, p_r, 0x7FFFFFFF * 256 + 1, p_o) == bad and b"workgroups" in lib.rpt_last_error(t._h)
        assert radiance_device(t._h, p_r, 2 ** 64 - 1, p_o) == bad
        assert untouched() and (o == PATTERN).all()
        # spp == 0 or n == 0 is RPT_OK and launches nothing, NULL arrays or not
        assert radiance_device(t._h, None, 0, None) == A.RPT_OK and radiance_device(t._h, p_r, 256, p_o, spp=0) == A.RPT_OK
        assert lib.rpt_radiance(t._h, None, 0, None, 0, 1, 1, 0, 0) == A.RPT_OK and lib.rpt_radiance(t._h, r8.ctypes.data, 256, o.ctypes.data, 0, 0, 1, 0, 0) == A.RPT_OK
        assert untouched() and (o == PATTERN).all()
        # a misaligned pointer is rejected whatever n is
        assert radiance_device(t._h, p_r + 4, 0, None) == bad and radiance_device(t._h, None, 0, p_o + 4) == bad
        # a scene that is not a mesh scene
        t._scene = rpt.AnalyticalScene()
        t.upload_scene()
        every_call(t._h, A.RPT_ERR_UNSUPPORTED, "an analytical scene")
    finally:
        t.close()
    h = C.c_void_p()
    assert lib.rpt_create(C.byref(h), 0) == A.RPT_OK
    try:
        every_call(h, A.RPT_ERR_NO_SCENE, "no scene at all")
    finally:
        lib.rpt_destroy(h)
    m = rpt.Tracer(s, devices=[0, 0], seed=1)
    try:
        every_call(m._h, A.RPT_ERR_UNSUPPORTED, "two local devices")
        assert b"one local device" in lib.rpt_last_error(m._h)
    finally:
        m.close()


def test_radiance_changes_no_frame_and_no_form(rpt, torch_cuda):
    s = Q.small_scene()
    r8 = _state_rays(s)
    t = rpt.Tracer(s, device=0, seed=4)
    try:
        t.set_mesh_shading({0: "smooth"})

        def frame():
            buf = rpt.DeviceColorBuffer(64, 48)
            t.render_n(buf, 2)
            torch_cuda.cuda.synchronize()
            choice = C.c_uint32()
            assert rpt.lib().rpt_debug_kernel_choice(t._h, C.byref(choice)) == 0
            return buf.pixels.cpu().numpy().view(np.uint32), Q.mesh_form(rpt, t), choice.value

        before, form, choice = frame()
        dev = torch_cuda.from_numpy(r8).cuda()
        for k in range(3):
            t.radiance(dev, spp=1 + k)
            t.radiance(r8[:300], spp=2)
            t.radiance(t.camera_sample_rays(64, 48, k), frames_done=k)
            c = C.c_uint32()
            assert rpt.lib().rpt_debug_kernel_choice(t._h, C.byref(c)) == 0
            assert Q.mesh_form(rpt, t) == form and c.value == choice, "the debug hooks report the last RENDER"
        after, form_after, choice_after = frame()
        assert np.array_equal(before, after) and form_after == form and choice_after == choice
    finally:
        t.close()
