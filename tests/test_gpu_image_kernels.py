"""The kernels that run after a frame is rendered, against the CPU oracle bit for bit and against float64: the a-trous denoiser
(csrc/denoise.hip), the u8 conversions and the scatter of gathered rank tiles (csrc/k_util.hip).

- the denoiser at every fused form (denoise_fused_kernel<1..3>, and denoise_step_kernel beyond three iterations) on shapes
  that straddle the fused kernel's 32-pixel tiles and the step kernel's 16-pixel blocks, with special values on tile corners,
  seams and image borders, at every edge_k of tests/test_denoise_f64.py and where k_i underflows or overflows; the benchmarked
  1080p and 4K forms; scratch growth across calls on one context and two streams; the argument checks;
- the u8 conversion at every one of its 255 step boundaries, through the device, host and resident entry points;
- convert_to_u8_at where the blit is clipped or misses the frame;
- the scatter with a payload that names each value's source.

A CPU test at the end checks that every image-side kernel of the product library's code object is run by a case here (or by
the module named for it)."""
import ctypes as C
import os

import numpy as np
import pytest

import dn_f64
from kernel_census import code_object_kernels
from test_denoise_f64 import EDGE_KS, u8_boundary_values, u8_frame, u8_specials, assert_u8_is_truncation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = os.path.join(ROOT, "rust-pathtracer_amd", "librpt_hip.so")


def dn_kernels(iterations):
    """The kernels rptlaunch::denoise launches for `iterations` (the default build)."""
    return {"denoise_fused_kernel<%d>" % min(iterations, 3)} | ({"denoise_step_kernel"} if iterations > 3 else set())


# ---- the denoiser -----------------------------------------------------------------------------------------------------------
ALL_KS = EDGE_KS + (1.4e-45, 3e38)
SPECIALS = (np.nan, np.inf, -np.inf, -1.0, -0.5, -2.0, 1e30, 3.4e38, 1.4e-45, -0.0, 4000.0)


def seam_frame(w, h, seed):
    """Random colours in [0, 2) with a hard edge, every special value placed at x, y in {0, 31, 32, 33, w-1} (tile corners,
    seams, image borders), one channel or all three."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0, 2, (h, w, 4)).astype(np.float32)
    img[:, (2 * w) // 3:, :3] = (2.5, 0.2, 0.05)
    xs = sorted(set(v for v in (0, 31, 32, 33, w - 1) if v < w))
    ys = sorted(set(v for v in (0, 31, 32, 33, h - 1) if v < h))
    spots = [(y, x) for y in ys for x in xs]
    rng.shuffle(spots)
    for i, (y, x) in enumerate(spots):
        v = SPECIALS[i % len(SPECIALS)]
        if i % 3 == 2:
            img[y, x, :3] = v
        else:
            img[y, x, int(rng.integers(0, 3))] = v
    return img


_renders = {}


def rendered(oracle, w, h):
    if (w, h) not in _renders:
        _renders[(w, h)] = oracle.render(oracle.scene_analytical(), w, h, 2, seed=3)
    return _renders[(w, h)]


def f64_window(img, it, k, y0, y1, x0, x1):
    """The restatement on rows y0:y1, columns x0:x1 only, computed on that window plus the filter's footprint (2^it - 1 pixels):
    equal to the whole image's there, for a fraction of the cost."""
    h, w = img.shape[:2]
    r = (1 << it) - 1
    a0, a1, b0, b1 = max(0, y0 - r), min(h, y1 + r), max(0, x0 - r), min(w, x1 + r)
    return dn_f64.denoise(img[a0:a1, b0:b1], it, k)[y0 - a0:y1 - a0, x0 - b0:x1 - b0]


def run_device(rpt, img, it, k):
    import torch
    h, w = img.shape[:2]
    buf = rpt.DeviceColorBuffer(w, h)
    buf.pixels.copy_(torch.from_numpy(img))
    got = buf.denoise(it, k)
    torch.cuda.synchronize()
    return got.pixels.cpu().numpy(), buf.pixels.cpu().numpy()


def check_denoise(rpt, oracle, img, it, k, what, windows=None):
    from test_gpu_parity import assert_bit_identical
    h, w = img.shape[:2]
    got, after = run_device(rpt, img, it, k)
    assert_bit_identical(got, oracle.denoise(img, w, h, it, k), what)
    assert_bit_identical(after, img, what + ": the input is not touched")
    for y0, y1, x0, x1 in windows or [(0, h, 0, w)]:
        dn_f64.check(got[y0:y1, x0:x1], f64_window(img, it, k, y0, y1, x0, x1), it, what + " against float64")


DN_SHAPES = [(1, 1), (1, 257), (257, 1), (31, 33), (32, 32), (33, 31), (63, 65), (64, 64), (65, 97), (200, 150)]
DN_CASES = [(w, h, it) for (w, h) in DN_SHAPES for it in range(1, 7)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,it", DN_CASES)
def test_denoiser_matrix(rpt, oracle, w, h, it):
    """A rendered frame and a frame of special values on the tile seams, at two edge_k each (all seven over a shape's six
    iteration counts)."""
    i = DN_SHAPES.index((w, h)) + it
    check_denoise(rpt, oracle, rendered(oracle, w, h), it, ALL_KS[i % len(ALL_KS)], "render %dx%d x%d" % (w, h, it))
    k = ALL_KS[(i + 3) % len(ALL_KS)]
    check_denoise(rpt, oracle, seam_frame(w, h, w * 1000 + h + it), it, k, "seams %dx%d x%d edge_k %g" % (w, h, it, k))


def large_frame(w, h, seed):
    """A benchmark-sized frame without the cost of a CPU render: a smooth gradient, 1-spp-like noise, fireflies, and the special
    values on tile seams and borders."""
    rng = np.random.default_rng(seed)
    img = seam_frame(w, h, seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = (0.2 + 0.6 * xx / w)[..., None] * np.array([1.0, 0.8, 0.6], np.float32)
    noise = rng.exponential(1.0, (h, w, 1)).astype(np.float32)
    keep = ~np.isfinite(img[..., :3]) | (img[..., :3] < 0) | (img[..., :3] > 10)
    img[..., :3] = np.where(keep, img[..., :3], base * noise)
    return img


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,it", [(1920, 1080, 3), (1920, 1080, 6), (3840, 2160, 3), (3840, 2160, 6)])
def test_denoiser_at_the_benchmarked_sizes(rpt, oracle, w, h, it):
    """bench.py's denoise forms (3 iterations) and the deepest one; float64 on a corner window and on one across tile seams."""
    img = large_frame(w, h, w + it)
    check_denoise(rpt, oracle, img, it, 2.0, "%dx%d x%d" % (w, h, it),
                  windows=[(0, 96, 0, 96), (h - 70, h, w - 70, w), (h // 2 - 40, h // 2 + 40, w // 2 - 40, w // 2 + 40)])


@pytest.mark.gpu
def test_denoiser_scratch_growth_and_two_streams(rpt, oracle):
    """One context: 64x48 x4, 1920x1080 x5 (the scratch buffer grows), 64x48 x4 again, on two streams in turn."""
    import torch
    from test_gpu_parity import assert_bit_identical
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    runs = [(64, 48, 4), (1920, 1080, 5), (64, 48, 4), (1920, 1080, 5), (64, 48, 4)]
    imgs = [seam_frame(w, h, 50 + j) for j, (w, h, _) in enumerate(runs)]
    ins = [rpt.DeviceColorBuffer(w, h) for (w, h, _) in runs]
    for b, img in zip(ins, imgs):
        b.pixels.copy_(torch.from_numpy(img))
    torch.cuda.synchronize()
    outs = []
    for j, ((w, h, it), b) in enumerate(zip(runs, ins)):
        s = streams[j % 2]
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            outs.append(b.denoise(it, 2.0))
            b.pixels.record_stream(s)
    torch.cuda.synchronize()
    for j, ((w, h, it), b, o, img) in enumerate(zip(runs, ins, outs, imgs)):
        assert_bit_identical(o.pixels.cpu().numpy(), oracle.denoise(img, w, h, it, 2.0), "run %d: %dx%d x%d" % (j, w, h, it))
        assert_bit_identical(b.pixels.cpu().numpy(), img, "run %d: the input is not touched" % j)


@pytest.mark.gpu
def test_denoiser_argument_edges(rpt, oracle):
    import torch
    from test_gpu_parity import assert_bit_identical
    from rust_pathtracer_amd.api import _ctx_for
    A = rpt._abi
    lib = rpt.lib()
    ctx = _ctx_for(0)
    w, h = 40, 24
    n = w * h * 4
    nbytes = n * 4
    img = seam_frame(w, h, 9)
    arena = torch.zeros(3 * n + 64, dtype=torch.float32, device="cuda")
    base = arena.data_ptr()
    assert base % 256 == 0
    arena[:n].copy_(torch.from_numpy(img.reshape(-1)))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    want = oracle.denoise(img, w, h, 3, 2.0)

    def call(src, dst, it=3, k=2.0):
        return lib.rpt_denoise_device(ctx, C.c_void_p(src), C.c_void_p(dst), w, h, it, C.c_float(k), stream)

    assert call(base, base + 16) == A.RPT_ERR_INVALID_ARG and b"overlap" in lib.rpt_last_error(ctx)     # partial overlap
    assert call(base + 16, base) == A.RPT_ERR_INVALID_ARG and b"overlap" in lib.rpt_last_error(ctx)
    assert call(base, base + nbytes + 8) == A.RPT_ERR_INVALID_ARG and b"aligned" in lib.rpt_last_error(ctx)   # misaligned by 8
    assert call(base + 8, base + 2 * nbytes) == A.RPT_ERR_INVALID_ARG and b"aligned" in lib.rpt_last_error(ctx)
    for k in (float("inf"), -0.0, 0.0, -2.0, float("nan")):
        assert call(base, base + nbytes, k=k) == A.RPT_ERR_INVALID_ARG, k
    assert call(base, base + nbytes) == A.RPT_OK                                                          # adjacent: accepted
    torch.cuda.synchronize()
    assert_bit_identical(arena[n:2 * n].cpu().numpy().reshape(h, w, 4), want, "adjacent buffers")
    assert call(base, base + nbytes, k=1.4e-45) == A.RPT_OK                                               # the smallest subnormal
    torch.cuda.synchronize()
    assert_bit_identical(arena[n:2 * n].cpu().numpy().reshape(h, w, 4), oracle.denoise(img, w, h, 3, 1.4e-45), "edge_k 1.4e-45")
    assert_bit_identical(arena[:n].cpu().numpy().reshape(h, w, 4), img, "the input is not touched")
    assert np.all(arena[2 * n:].cpu().numpy() == 0.0), "written beyond the output"
    host = rpt.ColorBuffer(w, h)
    host.pixels[:] = img.reshape(-1)
    assert_bit_identical(host.denoise(3, 2.0).image(), want, "rpt_denoise on host buffers")


# ---- u8 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_u8_at_every_step_boundary(rpt, oracle):
    """1021 x 1027 (not a multiple of 256 pixels), 1 x 1 and 1021 x 3: the device, host and resident conversions equal the
    oracle byte for byte, and the float64 truncation except within 2 ulp(f32) of an integer."""
    import torch
    from rust_pathtracer_amd.api import _convert_to_u8_tensor, _ctx_for
    colour, alpha = u8_boundary_values()
    sp = u8_specials()
    frames = [(1021, 1027, u8_frame(colour, alpha, sp, 1021, 1027)), (1, 1, sp[-1:].repeat(4).reshape(1, 1, 4)),
              (1021, 3, u8_frame(sp, sp[::-1], sp, 1021, 3))]
    tracer = rpt.Tracer(rpt.AnalyticalScene(), device=0, seed=1)
    try:
        for w, h, img in frames:
            what = "%dx%d" % (w, h)
            want = oracle.convert_to_u8(img, w, h)
            dev = torch.from_numpy(np.ascontiguousarray(img)).cuda()
            got = _convert_to_u8_tensor(dev, w, h).cpu().numpy().reshape(-1)
            assert np.array_equal(got, want), what + ": rpt_convert_to_u8_device"
            host = np.zeros(w * h * 4, np.uint8)
            ctx = _ctx_for(0)
            rpt._lib.check(rpt.lib().rpt_convert_to_u8(ctx, np.ascontiguousarray(img).ctypes.data, host.ctypes.data, w, h), ctx)
            assert np.array_equal(host, want), what + ": rpt_convert_to_u8"
            buf = rpt.ColorBuffer(w, h)
            buf.pixels[:] = img.reshape(-1)
            tracer.resident_upload(buf)
            assert np.array_equal(tracer.resident_to_u8(w, h), want), what + ": rpt_resident_download_u8"
            n_exc, n_diff = assert_u8_is_truncation(got, img, what, limit=w * h > 10000)
            print("u8 %s: %d values within 2 ulp(f32) of an integer, %d differ from the f64 truncation" % (what, n_exc, n_diff))
    finally:
        tracer.close()


U8_AT_CASES = [
    (96, 64, (0, 0, 40, 30)),          # a frame smaller than the buffer
    (96, 64, (300, 5, 200, 150)),      # beyond the frame in x
    (96, 64, (5, 300, 200, 150)),      # in y
    (96, 64, (300, 300, 200, 150)),    # in both
    (96, 64, (199, 10, 200, 150)),     # at0 = frame width - 1
    (96, 64, (0, 0, 1, 1)),            # a 1 x 1 frame
    (1, 1, (0, 0, 200, 150)),          # a 1 x 1 buffer
    (1, 1, (0, 0, 1, 1)),
    (96, 64, (3, 2, 97, 61)),          # frames of a pixel count that is not a multiple of 256
    (40, 3, (0, 0, 1021, 3)),
    (96, 64, (7, 11, 50, 40)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("bw,bh,at", U8_AT_CASES)
def test_convert_to_u8_at_edges(rpt, oracle, bw, bh, at):
    """Every byte of the frame: the blit's pixels equal the oracle's, the rest keep their (random) contents."""
    import torch
    sp = u8_specials()
    rng = np.random.default_rng(bw * 7 + at[0] * 3 + at[1])
    img = rng.uniform(-0.2, 1.2, (bh, bw, 4)).astype(np.float32)
    img.reshape(-1)[::7][:len(sp)] = sp[:len(img.reshape(-1)[::7])]
    buf = rpt.DeviceColorBuffer(bw, bh)
    buf.pixels.copy_(torch.from_numpy(img))
    before = rng.integers(0, 256, (at[3], at[2], 4), dtype=np.uint8)
    frame = torch.from_numpy(before.copy()).cuda()
    buf.convert_to_u8_at(frame, at)
    torch.cuda.synchronize()
    want = oracle.convert_to_u8_at(img, bw, bh, before.copy(), at)
    assert np.array_equal(frame.cpu().numpy(), want)


# ---- the scatter -------------------------------------------------------------------------------------------------------------
def scatter_payload(world, rows_padded, w):
    """[world, rows_padded, w, 4] uint32: rank << 27 | local row << 15 | column << 2 | channel, every value a finite f32."""
    assert world <= 8 and rows_padded <= 4096 and w <= 8192
    r = np.arange(world, dtype=np.uint32)[:, None, None, None] << 27
    lr = np.arange(rows_padded, dtype=np.uint32)[None, :, None, None] << 15
    c = np.arange(w, dtype=np.uint32)[None, None, :, None] << 2
    ch = np.arange(4, dtype=np.uint32)[None, None, None, :]
    return r | lr | c | ch


def scatter_want(lib, gathered, h, tile_rows, world):
    """The image from rpt_tile_copy_plan: each rank's full blocks and its ragged block, every image row exactly once."""
    from rust_pathtracer_amd import _abi
    src = np.full((h, 2), -1, np.int64)
    for rank in range(world):
        p = _abi.rpt_tile_plan()
        assert lib.rpt_tile_copy_plan(h, tile_rows, rank, world, C.byref(p)) == 0
        for b in range(p.full_blocks):
            for j in range(p.block_rows):
                g = p.host_row0 + b * p.host_row_stride + j
                assert src[g, 0] < 0
                src[g] = (rank, b * p.block_rows + j)
        for j in range(p.ragged_rows):
            g = p.ragged_host_row0 + j
            assert src[g, 0] < 0
            src[g] = (rank, p.ragged_tile_row0 + j)
    assert (src >= 0).all(), "rows no rank owns"
    return gathered[src[:, 0], src[:, 1]]


SCATTER_CASES = [(37, 29, 4, w) for w in range(1, 9)] + [       # (width, height, tile_rows, world)
    (1, 50, 3, 3), (5, 5, 2, 8), (16, 7, 16, 2), (33, 100, 7, 5), (64, 64, 1, 8), (3840, 2160, 2, 8), (3840, 2160, 16, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,tile_rows,world", SCATTER_CASES)
def test_untile_scatter(rpt, w, h, tile_rows, world):
    """tile_rows that do not divide the height, more ranks than row blocks (5 rows, blocks of 2, 8 ranks), width 1, padding
    beyond what is needed, 3840 x 2160 at world 8."""
    import torch
    from rust_pathtracer_amd.api import _ctx_for
    lib = rpt.lib()
    need = lib.rpt_tile_rows_padded(h, tile_rows, world)
    for rows_padded in (need, need + 3):
        g = scatter_payload(world, rows_padded, w)
        want = scatter_want(lib, g, h, tile_rows, world)
        dev = torch.from_numpy(g.view(np.float32)).cuda()
        image = torch.zeros(h + 1, w, 4, dtype=torch.float32, device="cuda")                 # (+1 row: nothing is written there)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.rpt_untile_device(_ctx_for(0), dev.data_ptr(), image.data_ptr(), w, h, tile_rows, world, rows_padded, stream) == 0
        torch.cuda.synchronize()
        got = image.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:h], want), "world %d, tile_rows %d, rows_padded %d" % (world, tile_rows, rows_padded)
        assert not got[h].any()
    if need > 1:
        assert lib.rpt_untile_device(_ctx_for(0), dev.data_ptr(), image.data_ptr(), w, h, tile_rows, world, need - 1, stream) != 0


# ---- the census --------------------------------------------------------------------------------------------------------------
EXERCISED_ELSEWHERE = {"sched_order_kernel": "test_gpu_dispatch.py", "sched_init_kernel": "test_gpu_dispatch.py"}


def covered_here():
    out = set()
    for _, _, it in DN_CASES:
        out |= dn_kernels(it)
    return out | {"convert_to_u8_kernel", "convert_to_u8_at_kernel", "untile_kernel"}


def test_every_image_kernel_is_run_by_a_case():
    """The product library's kernels that are not render_* kernels: exactly the four reachable denoiser forms, the two u8
    conversions, the scatter and the scheduler's two kernels, each run by a case of this module or the module named for it."""
    if not os.path.exists(PRODUCT):
        pytest.skip("the library is not built")
    for m in set(EXERCISED_ELSEWHERE.values()):
        assert os.path.exists(os.path.join(ROOT, "tests", m))
    have = set(k for k in code_object_kernels(PRODUCT) if not k.startswith("render_"))
    want = covered_here() | set(EXERCISED_ELSEWHERE)
    assert have == want, "not covered: %s; covered but gone: %s" % (sorted(have - want), sorted(want - have))
    assert sorted(k for k in have if k.startswith("denoise_")) == [
        "denoise_fused_kernel<1>", "denoise_fused_kernel<2>", "denoise_fused_kernel<3>", "denoise_step_kernel"]
