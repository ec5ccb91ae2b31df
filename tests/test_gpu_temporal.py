"""Temporal accumulation on the device (include/rpt.h, "temporal accumulation"; csrc/k_tacc.hip), bit for bit against its float32
restatement (tests/tacc_np.py):

- fuzzed frame pairs (tests/tacc_fuzz.py) at shapes that cross every seam of the 32 x 8 tiles, under camera pairs that are identical
  (the IDENTITY form), pan by 0.3 and 5.7 pixels, yaw a third of the image away, dolly, and face away, with and without
  prev_positions, and the first frame: every word of `out` and `history`;
- the host form, a second stream, `out` supplied by the caller, and every rejected call, which writes nothing;
- real records: under a static camera eight 1-spp frames accumulate to their running mean bit for bit; under a moving camera the
  accumulated frame is nearer the converged one than the last 1-spp frame."""
import ctypes as C

import numpy as np
import pytest

import gdn_fuzz
import tacc_fuzz
import tacc_np

pytestmark = pytest.mark.gpu
F = np.float32
# one tile is 32 x 8
SHAPES = [(1, 1), (3, 2), (32, 8), (31, 7), (33, 9), (31, 9), (33, 7), (65, 40), (97, 70)]
PAIRS = ("identical", "pan 0.3 px", "pan 5.7 px", "yaw a third", "dolly 10 %", "facing away")


@pytest.fixture(scope="module")
def tan(oracle):
    return lambda x: oracle.math(100, np.array([x], F))[0]


def same_words(a, b):
    a, b = np.ascontiguousarray(a, F).reshape(-1), np.ascontiguousarray(b, F).reshape(-1)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same(got, want, what):
    same = same_words(got, want)
    assert same.all(), "%s: %d of %d words differ, first at %s" % (what, (~same).sum(), same.size, np.argwhere(~same)[:4].ravel().tolist())


def c_camera(rpt, cam):
    c = rpt._abi.rpt_camera()
    c.origin, c.center, c.fov_deg = rpt._abi.F3(*[float(v) for v in cam[0:3]]), rpt._abi.F3(*[float(v) for v in cam[3:6]]), float(cam[6])
    return c


def run_device(rpt, case, cam, prev_cam, params, first=False, stream=None):
    """rpt_temporal_accumulate_device on a fuzz case: (out [h, w, 4], history [n, 8]) as numpy, the inputs checked untouched."""
    import torch
    from rust_pathtracer_amd.api import _ctx_for
    lib, ctx = rpt.lib(), _ctx_for(0)
    h, w = case["pixels"].shape[:2]
    n = w * h
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in case.items() if v is not None}
    out = torch.full((h, w, 4), -7.0, dtype=torch.float32, device="cuda")
    hist = torch.full((n, 8), -7.0, dtype=torch.float32, device="cuda")
    a, b = c_camera(rpt, cam), c_camera(rpt, prev_cam)
    ptr = lambda k: C.c_void_p(dev[k].data_ptr()) if k in dev and not (first and k.startswith("prev_")) else None       # noqa: E731
    s = torch.cuda.current_stream() if stream is None else stream
    s.wait_stream(torch.cuda.current_stream())                         # (the fills above)
    rc =lib.rpt_temporal_accumulate_device(ctx, ptr("pixels"), ptr("guides"), C.addressof(a), ptr("prev_guides"), ptr("prev_history"),
                                            None if first else C.addressof(b), ptr("prev_positions"), C.c_void_p(out.data_ptr()), C.c_void_p(hist.data_ptr()),
                                            w, h, C.c_float(params[0]), C.c_float(params[1]), C.c_float(params[2]), 0, C.c_void_p(s.cuda_stream))
    assert rc == rpt._abi.RPT_OK, lib.rpt_last_error(ctx)
    s.synchronize()
    for k, v in dev.items():
        assert_same(v.cpu().numpy(), case[k], "the input %s is not touched" % k)
    return out.cpu().numpy(), hist.cpu().numpy()


def want_of(case, cam, prev_cam, params, tan, first=False):
    if first:
        return tacc_np.accumulate(case["pixels"], case["guides"], cam, None, None, None, None, *params, tan)[:2]
    return tacc_np.accumulate(case["pixels"], case["guides"], cam, case["prev_guides"], case["prev_history"], prev_cam, case["prev_positions"], *params, tan)[:2]


# ---- bit for bit ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES)
def test_the_kernels_are_the_restatement_bit_for_bit(rpt, tan, w, h):
    pairs = tacc_fuzz.camera_pairs(w, h)
    j = SHAPES.index((w, h))
    seen = 0
    for k, name in enumerate(PAIRS):
        prev_cam, cam = pairs[name]
        for with_pp in (False, True):
            params = tacc_fuzz.PARAMS[(j + k + with_pp) % len(tacc_fuzz.PARAMS)]
            case = tacc_fuzz.fuzz_case(w, h, 100 * w + 10 * k + with_pp, prev_cam, cam, params[0], with_pp)
            what = "%dx%d %s%s, n_max %g normal_min %g plane_k %g" % (w, h, name, " with prev_positions" if with_pp else "", *params)
            out, hist = run_device(rpt, case, cam, prev_cam, params)
            want_out, want_hist = want_of(case, cam, prev_cam, params, tan)
            assert_same(out, want_out, what + ": out")
            assert_same(hist, want_hist, what + ": history")
            seen += int((want_hist[:, 3] > 1).sum())
    if w * h > 6:
        assert seen > 0, "no case of this shape found any history"
    prev_cam, cam = pairs["pan 0.3 px"]
    case = tacc_fuzz.fuzz_case(w, h, 7 * w + h, prev_cam, cam, 32.0)
    out, hist = run_device(rpt, case, cam, prev_cam, tacc_fuzz.PARAMS[0], first=True)
    want_out, want_hist = want_of(case, cam, prev_cam, tacc_fuzz.PARAMS[0], tan, first=True)
    assert_same(out, want_out, "%dx%d, the first frame: out" % (w, h))
    assert_same(hist, want_hist, "%dx%d, the first frame: history" % (w, h))
    assert (hist[:, 3] == 1.0).all() and (hist[:, 6:8].view(np.uint32) == 0).all()


# ---- host form, streams, out, rejected calls ----------------------------------------------------------------------------------------------
def test_the_host_form_a_second_stream_and_the_accumulators_own_buffers(rpt, tan):
    import torch
    w, h = 65, 40
    prev_cam, cam = tacc_fuzz.camera_pairs(w, h)["pan 5.7 px"]
    params = tacc_fuzz.PARAMS[0]
    case = tacc_fuzz.fuzz_case(w, h, 3, prev_cam, cam, params[0])
    want_out, want_hist = want_of(case, cam, prev_cam, params, tan)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out, hist = run_device(rpt, case, cam, prev_cam, params, stream=side)
    assert_same(out, want_out, "a second stream: out")
    assert_same(hist, want_hist, "a second stream: history")
    out, hist = rpt.temporal_accumulate(case["pixels"], case["guides"], c_camera(rpt, cam), case["prev_guides"], case["prev_history"], c_camera(rpt, prev_cam),
                                        None, *params)
    assert_same(out, want_out, "rpt_temporal_accumulate on host arrays: out")
    assert_same(hist, want_hist, "rpt_temporal_accumulate on host arrays: history")
    out, hist = rpt.temporal_accumulate(case["pixels"], case["guides"], c_camera(rpt, cam))
    first_out, first_hist = want_of(case, cam, prev_cam, params, tan, first=True)
    assert_same(out, first_out, "the host form, first frame: out")
    assert_same(hist, first_hist, "the host form, first frame: history")
    # TemporalAccumulator: two frames into an `out` of the caller's, then reset()
    acc = rpt.TemporalAccumulator(w, h)
    buf, mine = rpt.DeviceColorBuffer(w, h), rpt.DeviceColorBuffer(w, h)
    g0, g1 = (torch.from_numpy(case[k]).cuda() for k in ("prev_guides", "guides"))
    pin = lambda c: rpt.Pinhole(tuple(float(v) for v in c[0:3]), tuple(float(v) for v in c[3:6]), float(c[6]))      # noqa: E731
    buf.pixels.copy_(torch.from_numpy(case["pixels"]))
    r0 = acc.accumulate(buf, g0, pin(prev_cam))
    h0 = acc.history().cpu().numpy()
    r1 = acc.accumulate(buf, g1, pin(cam), out=mine)
    torch.cuda.synchronize()
    assert r1 is mine and r0 is not mine
    w0 = tacc_np.accumulate(case["pixels"], case["prev_guides"], prev_cam, None, None, None, None, *params, tan)
    assert_same(r0.pixels.cpu().numpy(), w0[0], "accumulator, frame 1")
    assert_same(h0, w0[1], "accumulator, frame 1: history")
    w1 = tacc_np.accumulate(case["pixels"], case["guides"], cam, case["prev_guides"], w0[1], prev_cam, None, *params, tan)
    assert_same(mine.pixels.cpu().numpy(), w1[0], "accumulator, frame 2 into the caller's buffer")
    assert_same(acc.history().cpu().numpy(), w1[1], "accumulator, frame 2: history")
    assert_same(acc.samples().cpu().numpy(), w1[1][:, 3], "samples()")
    with np.errstate(all="ignore"):
        var = np.maximum(w1[1][:, 5] - w1[1][:, 4] * w1[1][:, 4], F(0.0))
    assert_same(acc.variance().cpu().numpy(), var, "variance()")
    acc.reset()
    assert_same(acc.accumulate(buf, g1, pin(cam)).pixels.cpu().numpy(), first_out, "after reset(): a first frame")


def test_rejected_calls_write_nothing(rpt):
    import torch
    from rust_pathtracer_amd.api import _ctx_for
    A, lib, ctx = rpt._abi, rpt.lib(), _ctx_for(0)
    w, h = 40, 24
    n = w * h
    prev_cam, cam = tacc_fuzz.camera_pairs(w, h)["pan 0.3 px"]
    case = tacc_fuzz.fuzz_case(w, h, 9, prev_cam, cam, 32.0, True)
    dev = {k: torch.from_numpy(np.concatenate([v.reshape(-1), np.zeros(64, F)])).cuda() for k, v in case.items()}
    sink = torch.full((12 * n + 64,), -7.0, dtype=torch.float32, device="cuda")          # out: 4 n words, history: 8 n words
    base = sink.data_ptr()
    assert base % 256 == 0 and all(v.data_ptr() % 256 == 0 for v in dev.values())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    inf, nan = float("inf"), float("nan")
    cams = dict(a=c_camera(rpt, cam), b=c_camera(rpt, prev_cam))
    degenerate = c_camera(rpt, tacc_np.camera((1, 2, 3), (1, 2, 3), 60))
    nan_cam = c_camera(rpt, tacc_np.camera((1, nan, 3), (0, 0, 0), 60))
    inf_fov = c_camera(rpt, tacc_np.camera((1, 2, 3), (0, 0, 0), inf))
    p = {k: v.data_ptr() for k, v in dev.items()}

    def call(px=p["pixels"], g=p["guides"], a=C.addressof(cams["a"]), pg=p["prev_guides"], ph=p["prev_history"], b=C.addressof(cams["b"]),
             pp=p["prev_positions"], out=base, hist=base + 16 * n, ww=w, hh=h, n_max=32.0, nm=0.9, pk=1000.0, flags=0):
        v = lambda x: C.c_void_p(x) if x else None                      # noqa: E731
        return lib.rpt_temporal_accumulate_device(ctx, v(px), v(g), v(a), v(pg), v(ph), v(b), v(pp), v(out), v(hist), ww, hh, C.c_float(n_max), C.c_float(nm),
                                                  C.c_float(pk), flags, stream)

    bad = [dict(pg=0), dict(ph=0), dict(b=0), dict(pg=0, ph=0), dict(pg=0, b=0), dict(ph=0, b=0),                 # partial NULLs
           dict(px=0), dict(g=0), dict(a=0), dict(out=0), dict(hist=0),
           dict(px=p["pixels"] + 4), dict(g=p["guides"] + 8), dict(pg=p["prev_guides"] + 4), dict(ph=p["prev_history"] + 8), dict(pp=p["prev_positions"] + 4),
           dict(out=base + 4), dict(hist=base + 16 * n + 8),                                                       # misaligned
           dict(n_max=0.5), dict(n_max=nan), dict(n_max=inf), dict(nm=-1.5), dict(nm=1.5), dict(nm=nan), dict(pk=-1.0), dict(pk=nan), dict(pk=inf),
           dict(flags=1), dict(ww=0), dict(hh=0), dict(ww=65536),
           dict(a=C.addressof(degenerate)), dict(b=C.addressof(degenerate)), dict(a=C.addressof(nan_cam)), dict(b=C.addressof(inf_fov)),
           dict(hist=base + 16), dict(out=p["pixels"]), dict(hist=p["prev_history"] + 16), dict(out=p["guides"] + 64 * n - 16)]     # overlaps
    for kw in bad:
        assert call(**kw) == A.RPT_ERR_INVALID_ARG, kw
    assert b"overlap" in (call(hist=base + 16), lib.rpt_last_error(ctx))[1] and b"aligned" in (call(out=base + 4), lib.rpt_last_error(ctx))[1]
    host_out, host_hist = np.full((n, 4), -7.0, F), np.full((n, 8), -7.0, F)
    assert lib.rpt_temporal_accumulate(ctx, case["pixels"].ctypes.data, case["guides"].ctypes.data, C.addressof(cams["a"]), case["prev_guides"].ctypes.data, None,
                                       C.addressof(cams["b"]), None, host_out.ctypes.data, host_hist.ctypes.data, w, h, C.c_float(32.0), C.c_float(0.9),
                                       C.c_float(1000.0), 0) == A.RPT_ERR_INVALID_ARG
    assert lib.rpt_temporal_accumulate(ctx, case["pixels"].ctypes.data, case["guides"].ctypes.data, C.addressof(cams["a"]), None, None, None, None,
                                       host_out.ctypes.data, host_hist.ctypes.data, w, h, C.c_float(0.0), C.c_float(0.9), C.c_float(1000.0), 0) == A.RPT_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (sink.cpu().numpy() == -7.0).all() and (host_out == -7.0).all() and (host_hist == -7.0).all(), "a rejected call wrote something"
    for k, v in dev.items():
        assert_same(v.cpu().numpy()[:case[k].size], case[k], "the input %s is not touched" % k)
    assert call() == A.RPT_OK                                           # out and history adjacent: accepted
    torch.cuda.synchronize()
    got = sink.cpu().numpy()
    assert not (got[:12 * n] == -7.0).all() and (got[12 * n:] == -7.0).all(), "written beyond the history"


# ---- real records ----------------------------------------------------------------------------------------------------------------------------
def _tracer(rpt, origin=None, seed=1):
    from rust_pathtracer_amd import scenes
    s, _ = scenes.mesh_texture_scene()
    if origin is not None:
        s.camera = rpt.Pinhole(origin, s.camera.center, s.camera.fov)
    return rpt.Tracer(s, device=0, seed=seed), s.camera


def _one_sample_frame(rpt, t, w, h, seed):
    buf = rpt.DeviceColorBuffer(w, h)
    t.seed = seed
    t.render(buf)
    return buf


def test_a_static_camera_accumulates_the_running_mean_bit_for_bit(rpt):
    """scenes.mesh_texture_scene() at 64 x 48, guides from Tracer.denoise_guides: eight 1-spp frames of distinct seeds, each rendered
    into a zeroed buffer, accumulate (IDENTITY form, real guide records on both sides) to numpy's running mean in a render's blend
    order, and every pixel has 8 samples."""
    import torch
    w, h = 64, 48
    t, cam = _tracer(rpt)
    try:
        acc = rpt.TemporalAccumulator(w, h)
        guides = t.denoise_guides(w, h)
        mean = None
        for k in range(1, 9):
            buf = _one_sample_frame(rpt, t, w, h, 100 + k)
            out = acc.accumulate(buf, guides if k & 1 else guides.clone(), cam)
            torch.cuda.synchronize()
            frame = buf.pixels.cpu().numpy()[..., 0:3]
            assert np.isfinite(frame).all()
            al = F(F(1.0) / F(k))
            mean = frame.copy() if k == 1 else ((F(1.0) - al) * mean).astype(F) + (frame * al).astype(F)
            assert_same(out.pixels.cpu().numpy()[..., 0:3], mean, "frame %d" % k)
        assert (acc.samples().cpu().numpy() == 8.0).all()
        assert (acc.variance().cpu().numpy() > 0).any()
    finally:
        t.close()


def test_a_moving_camera_accumulates_towards_the_converged_frame(rpt):
    """The same scene; the origin moves sideways so that the image shifts about one pixel per frame, for eight frames.  A 4096-spp frame
    at the last camera is the truth, RMSE in compressed space (gdn_fuzz.rmse_compressed).  Conditions: the accumulated frame is nearer
    the truth than the last 1-spp frame, and at least half of the pixels have n' > 1 after the second frame.  Printed, not conditions:
    accumulation followed by the guided filter against the guided filter alone on the last frame, and the mean of samples().
    Measured on an MI355X: the last 1-spp frame 0.1323, accumulated 0.0368; the guided filter alone 0.0486, accumulated then
    filtered 0.0154; mean of samples() 7.71; 99.1 % of the pixels have n' > 1 after the second frame."""
    import torch
    w, h = 64, 48
    ref_t, cam0 = _tracer(rpt, seed=2)
    dist = float(np.sqrt(sum((a - b) ** 2 for a, b in zip(cam0.origin, cam0.center))))
    step = 2.0 * np.tan(np.radians(cam0.fov) * 0.5) * dist / w          # one pixel at the center's depth
    ref_t.close()
    acc = rpt.TemporalAccumulator(w, h)
    t = None
    try:
        for k in range(8):
            origin = (cam0.origin[0] + (k - 7) * step, cam0.origin[1], cam0.origin[2])
            t, cam = _tracer(rpt, origin)
            guides = t.denoise_guides(w, h)
            last = _one_sample_frame(rpt, t, w, h, 200 + k)
            out = acc.accumulate(last, guides, cam)
            torch.cuda.synchronize()
            if k == 1:
                share = float((acc.samples() > 1).float().mean())
                print("after the second frame %.1f %% of the pixels have n' > 1" % (100 * share))
                assert share >= 0.5
            if k < 7:
                t.close()
                t = None
        ref = rpt.DeviceColorBuffer(w, h)
        t.seed = 2
        t.render_n(ref, 4096)
        filtered_acc, filtered_last = out.denoise_guided(guides), last.denoise_guided(guides)
        torch.cuda.synchronize()
        want = ref.pixels.cpu().numpy()
        e_last, e_acc, e_facc, e_flast = (gdn_fuzz.rmse_compressed(x.pixels.cpu().numpy(), want) for x in (last, out, filtered_acc, filtered_last))
        print("mesh_texture_scene 64x48, eight frames one pixel apart, against 4096 spp, RMSE in compressed space: the last 1-spp frame %.4f, accumulated %.4f; "
              "guided filter alone %.4f, accumulated then filtered %.4f; mean of samples() %.2f" % (e_last, e_acc, e_flast, e_facc, float(acc.samples().mean())))
        assert e_acc < e_last
    finally:
        if t is not None:
            t.close()
