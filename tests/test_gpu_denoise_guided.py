"""The guided denoiser on the device (include/rpt.h, "guided denoiser"; csrc/k_gdn.hip), bit for bit against its float32 restatement
(tests/gdn_np.py):

- the filter on fuzzed frames and guides (tests/gdn_fuzz.py) at shapes that cross every seam of the 32 x 16 fused tiles and the
  16 x 16 step tiles, iterations 1-6 (gdn_fused_kernel<1>, <2>, and gdn_step_kernel at steps 4 to 32), normal_k and plane_k at 0 and
  large, an edge_k whose k_i overflows; with neutral guides the very words of rpt_denoise_device, on the device, at every shape;
- the pack on real records of a textured and a normal-mapped mesh scene, misses included, and a rendered frame of that scene
  through the filter;
- quality on a rendered frame: nearer the 4096-spp frame than the colour-only filter and than the input;
- the host forms, two streams, the growth of the context's scratch buffer, and rejected calls, which write nothing."""
import ctypes as C

import numpy as np
import pytest

import gdn_fuzz
import gdn_np

pytestmark = pytest.mark.gpu
F = np.float32
# one tile of the fused kernel is 32 x 16, one of the step kernel 16 x 16
SHAPES = [(1, 1), (3, 2), (32, 16), (31, 15), (33, 17), (31, 17), (33, 15), (65, 40), (97, 70)]


def same_words(a, b):
    a, b = np.ascontiguousarray(a, F).reshape(-1), np.ascontiguousarray(b, F).reshape(-1)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same(got, want, what):
    same = same_words(got, want)
    assert same.all(), "%s: %d of %d words differ, first at %s" % (what, (~same).sum(), same.size, np.argwhere(~same)[:4].ravel().tolist())


def device_buffer(rpt, img):
    import torch
    h, w = img.shape[:2]
    buf = rpt.DeviceColorBuffer(w, h)
    buf.pixels.copy_(torch.from_numpy(np.ascontiguousarray(img, F)))
    return buf


def run_guided(rpt, img, guides, it, ek, nk, pk):
    import torch
    buf = device_buffer(rpt, img)
    out = buf.denoise_guided(torch.from_numpy(guides).cuda(), it, ek, nk, pk)
    torch.cuda.synchronize()
    assert_same(buf.pixels.cpu().numpy(), img, "the input is not touched")
    return out.pixels.cpu().numpy()


# ---- the filter ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES)
def test_the_filter_is_the_restatement_bit_for_bit(rpt, w, h):
    img, g = gdn_fuzz.fuzz_frame(w, h, 100 * w + h)
    j = SHAPES.index((w, h))
    for it in range(1, 7):
        nk, pk, ek = gdn_fuzz.PARAMS[(it + j) % len(gdn_fuzz.PARAMS)]
        what = "%dx%d x%d, edge_k %g normal_k %g plane_k %g" % (w, h, it, ek, nk, pk)
        assert_same(run_guided(rpt, img, g, it, ek, nk, pk), gdn_np.denoise_guided(img, g, it, ek, nk, pk), what)


@pytest.mark.parametrize("w,h", SHAPES)
def test_neutral_guides_give_the_words_of_rpt_denoise_device(rpt, w, h):
    import torch
    img, _ = gdn_fuzz.fuzz_frame(w, h, 7 * w + h)
    buf = device_buffer(rpt, img)
    g = torch.from_numpy(gdn_np.neutral_guides(w * h)).cuda()
    for it in range(1, 7):
        ek = (2.0, 1e-6, 3e37, 0.5, 1e3, 8.0)[it - 1]
        want = buf.denoise(it, ek).pixels.cpu().numpy()
        got = buf.denoise_guided(g, it, ek, 1e30 if it & 1 else 4.0, 0.0 if it & 2 else 1000.0).pixels.cpu().numpy()
        assert_same(got, want, "%dx%d x%d edge_k %g" % (w, h, it, ek))


# ---- the pack, on real records ----------------------------------------------------------------------------------------------------------------
def _records(rpt, t, w, h):
    import torch
    rays = t.camera_rays(w, h)
    n = w * h
    hits = torch.empty((n, 8), dtype=torch.float32, device=rays.device)
    surf = torch.empty((n, 16), dtype=torch.float32, device=rays.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rpt._lib.check(rpt.lib().rpt_trace_rays_device(t._h, rays.data_ptr(), n, hits.data_ptr(), surf.data_ptr(), 0, stream), t._h)
    return rays, hits, surf


def _textured_tracer(rpt, normal_maps, seed, gamma=2.2):
    """scenes.mesh_texture_scene() (mesh_normal_map_scene() is that scene and a bump map) under two checker textures, or, gamma None,
    as the function returns it."""
    from rust_pathtracer_amd import scenes
    s, uvs, bump = scenes.mesh_normal_map_scene()
    t = rpt.Tracer(s, device=0, seed=seed)
    if gamma is None:
        return t
    t.set_mesh_textures({0: dict(uvs=uvs[0], texels=scenes.checker_texture(64, 64), gamma=gamma),
                         1: dict(uvs=uvs[1], texels=scenes.checker_texture(32, 32, (255, 120, 60), (30, 60, 200), 4), gamma=gamma)})
    if normal_maps:
        t.set_mesh_normal_maps({0: dict(texels=bump), 1: dict(texels=bump, strength=2.0)})
    return t


@pytest.mark.parametrize("normal_maps", [False, True])
def test_the_pack_is_numpy_f32_bit_for_bit_and_a_frame_filters_like_the_restatement(rpt, normal_maps):
    import torch
    w, h = 40, 30
    t = _textured_tracer(rpt, normal_maps, 1)
    try:
        rays, hits, surf = _records(rpt, t, w, h)
        got = rpt.pack_guides(rays, hits, surf)
        torch.cuda.synchronize()
        r, hh, sf = (x.cpu().numpy() for x in (rays, hits, surf))
        want = gdn_np.pack(r, hh, sf)
        kinds = hh.view(np.uint32)[:, 1]
        assert (kinds == 0).sum() > 20 and (kinds == 3).sum() > 50 and (kinds == 2).sum() > 100, "misses, triangles and the floor"
        if normal_maps:
            assert (sf[kinds == 3][:, 0:3] != sf[kinds == 3][:, 3:6]).any(), "the map bends ns away from ng"
        assert_same(got.cpu().numpy(), want, "rpt_denoise_guides_device")
        assert_same(t.denoise_guides(w, h).cpu().numpy(), want, "Tracer.denoise_guides")
        assert_same(rpt.pack_guides(r, hh, sf), want, "rpt_denoise_guides on host arrays")
        buf = rpt.DeviceColorBuffer(w, h)
        t.render_n(buf, 4)
        torch.cuda.synchronize()
        img = buf.pixels.cpu().numpy()
        out = buf.denoise_guided(got).pixels.cpu().numpy()
        assert_same(out, gdn_np.denoise_guided(img, want, 4, 0.25, 4.0, 1000.0), "a rendered frame, the defaults")
        assert not same_words(out, img).all()
    finally:
        t.close()


# ---- quality on a rendered frame --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [None, 1.0, 2.2])
def test_guided_is_nearer_the_converged_frame_than_colour_only_and_than_the_input(rpt, gamma):
    """scenes.mesh_texture_scene() at 64 x 48, 4 spp against 4096 spp, RMSE in compressed space, both filters at their defaults.  The
    inequalities are conditions, not tuned thresholds: guided < colour-only and guided < input on the scene as the function returns
    it.  Measured on an MI355X: input 0.0626, colour-only 0.0272, guided 0.0186.

    The same scene under two checker textures is measured beside it, and there the first inequality is NOT a condition, because it
    does not hold at every contrast (the figures are printed; README has them): with the bytes linear (gamma 1.0, albedo contrast
    6 : 1) input 0.0641, colour-only 0.0342, guided 0.0312; decoded with gamma 2.2 (contrast 60 : 1, the dark fields at FLOOR) input
    0.0655, colour-only 0.0351, guided 0.0434 — the floor and the background gain as before (0.0392 -> 0.0254, 0.0041 -> 0.0023) and
    the two textured meshes lose (0.0488 -> 0.0657, 0.0453 -> 0.1084).  The cause is in the guide, not in the kernels (which equal
    the restatement bit for bit on these very frames): a guide's albedo is sampled at the pixel's centre while the pixel's colour is
    the mean over its footprint, so a pixel that straddles a texture edge is divided by an albedo up to 60 times too small or too
    large, and the filter spreads that.  A 64 x 48 frame has few pixels on the meshes that do not straddle one."""
    import torch
    w, h = 64, 48
    t = _textured_tracer(rpt, False, 1, gamma)
    ref_t = _textured_tracer(rpt, False, 2, gamma)
    try:
        ref, noisy = rpt.DeviceColorBuffer(w, h), rpt.DeviceColorBuffer(w, h)
        ref_t.render_n(ref, 4096)
        t.render_n(noisy, 4)
        guides = t.denoise_guides(w, h)
        guided, plain = noisy.denoise_guided(guides), noisy.denoise()
        torch.cuda.synchronize()
        want = ref.pixels.cpu().numpy()
        e_in, e_plain, e_guided = (gdn_fuzz.rmse_compressed(x.pixels.cpu().numpy(), want) for x in (noisy, plain, guided))
        print("mesh_texture_scene (%s) 64x48, 4 spp against 4096 spp, RMSE in compressed space: input %.4f, colour-only %.4f, guided %.4f" % (
            "as returned" if gamma is None else "checker textures, gamma %g" % gamma, e_in, e_plain, e_guided))
        assert e_guided < e_in
        if gamma is None:
            assert e_guided < e_plain
    finally:
        t.close()
        ref_t.close()


# ---- host forms, streams, scratch, arguments -------------------------------------------------------------------------------------------------
def test_host_forms_two_streams_and_scratch_growth(rpt):
    """One context: 64x48 x4, 320x200 x5 (the scratch buffer grows), 64x48 x4 of the colour-only filter (the same scratch buffer),
    320x200 x5 and 64x48 x3, on two streams in turn; then the host form."""
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    runs = [(64, 48, 4), (320, 200, 5), (64, 48, 4), (320, 200, 5), (64, 48, 3)]
    frames = [gdn_fuzz.fuzz_frame(w, h, 50 + j) for j, (w, h, _) in enumerate(runs)]
    ins = [device_buffer(rpt, img) for img, _ in frames]
    gs = [torch.from_numpy(g).cuda() for _, g in frames]
    torch.cuda.synchronize()
    outs = []
    for j, ((w, h, it), b, g) in enumerate(zip(runs, ins, gs)):
        s = streams[j % 2]
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            outs.append(b.denoise_guided(g, it) if j != 2 else b.denoise(it, 2.0))      # (the colour-only filter shares the scratch buffer)
            b.pixels.record_stream(s)
            g.record_stream(s)
    torch.cuda.synchronize()
    for j, ((w, h, it), b, o, (img, g)) in enumerate(zip(runs, ins, outs, frames)):
        want = gdn_np.denoise_guided(img, g, it, 0.25, 4.0, 1000.0) if j != 2 else b.denoise(it, 2.0).pixels.cpu().numpy()
        assert_same(o.pixels.cpu().numpy(), want, "run %d: %dx%d x%d" % (j, w, h, it))
        assert_same(b.pixels.cpu().numpy(), img, "run %d: the input is not touched" % j)
    img, g = frames[4]
    host = rpt.ColorBuffer(64, 48)
    host.pixels[:] = img.reshape(-1)
    assert_same(host.denoise_guided(g, 3).image(), outs[4].pixels.cpu().numpy(), "rpt_denoise_guided on host buffers")


def test_rejected_calls_write_nothing(rpt):
    import torch
    from rust_pathtracer_amd.api import _ctx_for
    A, lib, ctx = rpt._abi, rpt.lib(), _ctx_for(0)
    w, h = 40, 24
    n = w * h * 4
    nbytes = n * 4
    img, g = gdn_fuzz.fuzz_frame(w, h, 9)
    arena = torch.zeros(3 * n + 64, dtype=torch.float32, device="cuda")
    guides = torch.from_numpy(np.concatenate([g.reshape(-1), np.zeros(64, F)])).cuda()
    base, gbase = arena.data_ptr(), guides.data_ptr()
    assert base % 256 == 0 and gbase % 256 == 0
    arena[:n].copy_(torch.from_numpy(img.reshape(-1)))
    arena[n:].fill_(-7.0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    inf, nan = float("inf"), float("nan")

    def call(src=base, gd=gbase, dst=base + nbytes, it=3, ek=0.25, nk=4.0, pk=1000.0, flags=0, ww=w):
        return lib.rpt_denoise_guided_device(ctx, C.c_void_p(src), C.c_void_p(gd), C.c_void_p(dst), ww, h, it, C.c_float(ek), C.c_float(nk),
                                             C.c_float(pk), flags, stream)

    bad = [dict(dst=base + 16), dict(src=base + 16, dst=base), dict(dst=base + nbytes + 8), dict(src=base + 8, dst=base + 2 * nbytes), dict(gd=gbase + 4),
           dict(gd=base + nbytes + 64), dict(it=0), dict(it=7), dict(ek=0.0), dict(ek=nan), dict(ek=-1.0), dict(ek=inf), dict(nk=-1.0), dict(nk=inf),
           dict(nk=nan), dict(pk=-1.0), dict(pk=inf), dict(pk=nan), dict(flags=1), dict(ww=0), dict(src=0), dict(gd=0), dict(dst=0)]
    for kw in bad:
        assert call(**kw) == A.RPT_ERR_INVALID_ARG, kw
    assert b"overlap" in (call(dst=base + 16), lib.rpt_last_error(ctx))[1] and b"aligned" in (call(gd=gbase + 4), lib.rpt_last_error(ctx))[1]
    rays = torch.zeros(16 * 8 + 4, dtype=torch.float32, device="cuda")
    out = torch.full((16 * 16 + 4,), -7.0, dtype=torch.float32, device="cuda")

    def pack(r=rays.data_ptr(), hh=rays.data_ptr(), s=guides.data_ptr(), o=out.data_ptr(), count=16):
        return lib.rpt_denoise_guides_device(ctx, C.c_void_p(r), C.c_void_p(hh), C.c_void_p(s), count, C.c_void_p(o), stream)

    for kw in (dict(r=0), dict(hh=0), dict(s=0), dict(o=0), dict(o=out.data_ptr() + 4), dict(r=rays.data_ptr() + 8), dict(o=out.data_ptr() + 4, count=0),
               dict(count=256 * 0x7FFFFFFF + 1)):
        assert pack(**kw) == A.RPT_ERR_INVALID_ARG, kw
    assert pack(count=0) == A.RPT_OK and pack(r=0, hh=0, s=0, o=0, count=0) == A.RPT_OK
    torch.cuda.synchronize()
    assert (arena[n:].cpu().numpy() == -7.0).all() and (out.cpu().numpy() == -7.0).all(), "a rejected call wrote something"
    assert_same(arena[:n].cpu().numpy(), img, "the input is not touched")
    assert call() == A.RPT_OK                                                                              # adjacent buffers: accepted
    torch.cuda.synchronize()
    assert_same(arena[n:2 * n].cpu().numpy(), gdn_np.denoise_guided(img, g, 3, 0.25, 4.0, 1000.0), "adjacent buffers")
    assert (arena[2 * n:].cpu().numpy() == -7.0).all(), "written beyond the output"
    assert pack() == A.RPT_OK
    torch.cuda.synchronize()
    assert_same(out[:256].cpu().numpy(), gdn_np.neutral_guides(16), "all-zero hits are misses")
    assert (out[256:].cpu().numpy() == -7.0).all(), "written beyond the guides"
    host = np.full((w * h, 4), -7.0, F)
    assert lib.rpt_denoise_guided(ctx, img.ctypes.data, g.ctypes.data, host.ctypes.data, w, h, 9, C.c_float(0.25), C.c_float(4.0), C.c_float(1000.0), 0) == A.RPT_ERR_INVALID_ARG
    assert lib.rpt_denoise_guides(ctx, None, None, None, 3, None) == A.RPT_ERR_INVALID_ARG
    assert (host == -7.0).all()
