"""Parity of the HIP path with the CPU oracle, through the C ABI (needs an MI355X).

Tolerance: NONE.  Both sides compute in f32 with the reference's operation order,
correctly rounded divide/sqrt and the shared strict libm stand-in, so every pixel must be
BIT-IDENTICAL (NaNs, if any, in the same places).  BASELINE.json's "per-pixel L2 error
< 1e-4 after 256 spp" is therefore met with error exactly 0.
"""
import ctypes as C
import os

import numpy as np
import pytest

import conftest

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_identical(got, want, what=""):
    got = np.asarray(got, dtype=np.float32)
    want = np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), "%s: NaN positions differ (%d vs %d)" % (what, nan_g.sum(), nan_w.sum())
    ok = nan_g | (bits(got) == bits(want))
    if not ok.all():
        idx = np.argwhere(~ok)
        first = tuple(idx[0])
        diff = np.abs(got[~ok].astype(np.float64) - want[~ok].astype(np.float64))
        raise AssertionError("%s: %d of %d values differ; first at %s: got %r want %r; max |diff| %g" %
                             (what, (~ok).sum(), ok.size, first, got[first], want[first], diff.max()))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def tracer(rpt, torch_cuda):
    t = rpt.Tracer(rpt.AnalyticalScene(), device=0, seed=1)
    yield t
    t.close()


def _probe(rpt, torch, tracer, fn, a, b=None):
    ta = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    tb = torch.from_numpy(np.ascontiguousarray(b if b is not None else np.zeros_like(a), dtype=np.float32)).cuda()
    out = torch.empty_like(ta)
    stream = torch.cuda.current_stream().cuda_stream
    rpt._lib.check(rpt.lib().rpt_probe_math(tracer._h, fn, ta.data_ptr(), tb.data_ptr(), out.data_ptr(), ta.numel(),
                                            C.c_void_p(stream)), tracer._h)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _random_floats(rng, n):
    """All f32 bit patterns: uniform over the encodings (covers subnormals, inf, NaN)."""
    return rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("fn,name", [(0, "sin"), (1, "cos")])
def test_probe_sincos(rpt, torch_cuda, tracer, oracle, fn, name):
    rng = np.random.default_rng(10 + fn)
    a = np.concatenate([rng.uniform(0, 2 * np.pi, 2_000_000), rng.uniform(-1e4, 1e4, 1_000_000),
                        [0.0, -0.0, np.pi, 2 * np.pi, np.inf, -np.inf, np.nan, 1e-40, 6.2831855]]).astype(np.float32)
    assert_bit_identical(_probe(rpt, torch_cuda, tracer, fn, a), oracle.math(fn, a), name)


def test_probe_log2(rpt, torch_cuda, tracer, oracle):
    rng = np.random.default_rng(12)
    a = np.concatenate([_random_floats(rng, 2_000_000), rng.uniform(1e-6, 1e-2, 1_000_000).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, np.inf, -1.0, np.nan, 1e-45, 3.4e38], dtype=np.float32)])
    assert_bit_identical(_probe(rpt, torch_cuda, tracer, 2, a), oracle.math(2, a), "log2")


def test_probe_pow(rpt, torch_cuda, tracer, oracle):
    rng = np.random.default_rng(13)
    n = 1_000_000
    a = np.concatenate([rng.uniform(0, 1.5, n), rng.uniform(1e-6, 1e-2, n), _random_floats(rng, n),
                        [0.0, -0.0, 1.0, np.inf, -1.0, -8.0, -8.0, np.nan, 2.0, 0.5]]).astype(np.float32)
    b = np.concatenate([np.full(n, 2.2), rng.uniform(0, 1, n), _random_floats(rng, n),
                        [0.5, 0.5, np.nan, 2.0, np.inf, 3.0, 0.5, 0.0, 200.0, -200.0]]).astype(np.float32)
    b[n // 2:n] = 0.4545
    b[: n // 4] = 0.5
    assert_bit_identical(_probe(rpt, torch_cuda, tracer, 3, a, b), oracle.math(3, a, b), "pow")


def test_device_libm_against_float64(rpt, torch_cuda, tracer):
    """include/rpt_strict_math.h is the one source oracle and kernels share, so "HIP equals oracle" on sin / cos / log2 / pow says
    that two compilers agree on it, not that it is right.  This test does not load the oracle: what the DEVICE
    returns against NumPy's float64 functions, in ulps of the float32 result — the bounds the header claims (sin / cos 1.5 ulp on the
    path's domain, log2 / pow / exp / log 0.5001: almost always the correctly rounded float32), and division and square root
    correctly rounded outright (0.5 ulp, and equal to the rounded float64 result)."""
    A = rpt._abi
    rng = np.random.default_rng(77)
    n = 1_000_000

    def ulps(got, ref64):
        ref32 = ref64.astype(np.float32)
        return np.abs(got.astype(np.float64) - ref64) / np.spacing(np.abs(ref32)).astype(np.float64)

    x = rng.uniform(0, 2 * np.pi, n).astype(np.float32)
    for fn, f in ((0, np.sin), (1, np.cos)):
        got, ref = _probe(rpt, torch_cuda, tracer, fn, x), f(x.astype(np.float64))
        big = np.abs(ref) > 1e-3                                     # (near a zero the ulp is tiny: the absolute error counts there)
        assert ulps(got, ref)[big].max() <= 1.5 and np.abs(got - ref).max() < 1.2e-7, f.__name__
    x = rng.integers(0x00800000, 0x7f7fffff, size=n, dtype=np.uint32).view(np.float32)          # every positive normal f32
    got, ref = _probe(rpt, torch_cuda, tracer, 2, x), np.log2(x.astype(np.float64))
    assert ulps(got, ref).max() <= 0.5001 and (got == ref.astype(np.float32)).mean() > 0.99999, "log2"
    got, ref = _probe(rpt, torch_cuda, tracer, A.RPT_PROBE_LOG, x), np.log(x.astype(np.float64))
    assert ulps(got, ref).max() <= 0.5001, "log"
    # pow as the path uses it: the background's x^2.2 (scene.rs:32-34), convert_to_u8's x^0.4545 (buffer.rs:59), sqrt-like 0.5, any y in (0, 3)
    a = rng.uniform(1e-4, 4.0, n).astype(np.float32)
    for b in (np.full(n, 2.2, dtype=np.float32), np.full(n, 0.4545, dtype=np.float32), np.full(n, 0.5, dtype=np.float32), rng.uniform(0, 3, n).astype(np.float32)):
        got, ref = _probe(rpt, torch_cuda, tracer, 3, a, b), np.power(a.astype(np.float64), b.astype(np.float64))
        assert ulps(got, ref).max() <= 0.5001, "pow, y = %r" % (b[0],)
    x = rng.uniform(-80, 80, n).astype(np.float32)
    got, ref = _probe(rpt, torch_cuda, tracer, A.RPT_PROBE_EXP, x), np.exp(x.astype(np.float64))
    assert ulps(got, ref).max() <= 0.5001, "exp"
    # the IEEE operations: the float64 quotient / root of two float32s rounds to the correctly rounded float32 (double rounding cannot
    # bite: 53 >= 2 * 24 + 2), results in the normal range
    a, b = rng.uniform(-1e3, 1e3, n).astype(np.float32), rng.uniform(0.01, 1e3, n).astype(np.float32)
    assert np.array_equal(_probe(rpt, torch_cuda, tracer, A.RPT_PROBE_DIV, a, b), (a.astype(np.float64) / b.astype(np.float64)).astype(np.float32)), "divide"
    assert np.array_equal(_probe(rpt, torch_cuda, tracer, 5, b), np.sqrt(b.astype(np.float64)).astype(np.float32)), "square root"


def test_probe_div_sqrt_are_correctly_rounded(rpt, torch_cuda, tracer, oracle):
    rng = np.random.default_rng(14)
    n = 3_000_000
    a, b = _random_floats(rng, n), _random_floats(rng, n)
    assert_bit_identical(_probe(rpt, torch_cuda, tracer, 4, a, b), oracle.math(4, a, b), "div")
    a2 = np.concatenate([rng.uniform(-4, 4, n), rng.uniform(0, 1e-38, 1000)]).astype(np.float32)
    b2 = np.concatenate([rng.uniform(-4, 4, n), rng.uniform(0, 1e-38, 1000)]).astype(np.float32)
    assert_bit_identical(_probe(rpt, torch_cuda, tracer, 4, a2, b2), oracle.math(4, a2, b2), "div (moderate range)")
    assert_bit_identical(_probe(rpt, torch_cuda, tracer, 5, a), oracle.math(5, a), "sqrt")
    assert_bit_identical(_probe(rpt, torch_cuda, tracer, 5, np.abs(a2)), oracle.math(5, np.abs(a2)), "sqrt (moderate range)")


def test_probe_library_divide_is_the_ieee_divide(rpt, torch_cuda, tracer, oracle):
    """The library divides through a shorter sequence than hipcc's (dev_math.h: one refined reciprocal shared by the numerators of
    one denominator, one correction; proven on all significand pairs by tools/proofs/div_exhaustive.hip) inside a guarded exponent
    range, and through hipcc's divide outside it.  Here: every kind of operand at the seams — all bit patterns, exponents around
    the guard's limits (2^-61, 2^60), denormals, zeros of both signs, infinities, NaNs, numerators far smaller than the denominator —
    single quotients (RPT_PROBE_DIV) and the three-quotient forms of divs3 / normalize (RPT_PROBE_DIV3)."""
    A = rpt._abi
    rng = np.random.default_rng(33)
    n = 2_000_000
    def mixed(k):
        mant = rng.integers(0, 2 ** 23, size=k, dtype=np.uint64)
        sign = rng.integers(0, 2, size=k, dtype=np.uint64) << 31
        seam = rng.choice(np.array([1, 2, 60, 64, 65, 66, 67, 68, 69, 126, 127, 128, 185, 186, 187, 188, 189, 190, 253, 254], dtype=np.uint64), size=k)
        return (sign | (seam << 23) | mant).astype(np.uint32).view(np.float32)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-39, 1.0, -1.0, 3.0, 1e30, 1e-30, 2.0 ** -61, 2.0 ** 60, 2.0 ** 59.5], dtype=np.float32)
    grid_a, grid_b = np.meshgrid(specials, specials)
    for a, b, what in ((_random_floats(rng, n), _random_floats(rng, n), "all bit patterns"),
                       (mixed(n), mixed(n), "exponents at the guard's seams"),
                       (rng.uniform(-4, 4, n).astype(np.float32), rng.uniform(-4, 4, n).astype(np.float32), "moderate range"),
                       (mixed(n), rng.uniform(0.1, 10, n).astype(np.float32), "seam numerators, ordinary denominators"),
                       (grid_a.ravel().copy(), grid_b.ravel().copy(), "special values, all pairs")):
        assert_bit_identical(_probe(rpt, torch_cuda, tracer, A.RPT_PROBE_DIV, a, b), oracle.math(4, a, b), "fdiv, " + what)
        assert_bit_identical(_probe(rpt, torch_cuda, tracer, A.RPT_PROBE_DIV3, a, b), oracle.math(9, a, b), "divs3, " + what)
        # the library's square root (same construction: tools/proofs/sqrt_exhaustive.hip) on the same operands
        assert_bit_identical(_probe(rpt, torch_cuda, tracer, A.RPT_PROBE_SQRT, a), oracle.math(5, a), "fsqrt, " + what)
        assert_bit_identical(_probe(rpt, torch_cuda, tracer, A.RPT_PROBE_SQRT, np.abs(b)), oracle.math(5, np.abs(b)), "fsqrt of |b|, " + what)


def test_probe_rng_first_draw(rpt, torch_cuda, tracer, oracle):
    n = 4096
    seed, frame = 1, 7
    a = np.full(n, seed, dtype=np.uint32).view(np.float32)
    b = np.full(n, frame, dtype=np.uint32).view(np.float32)
    got = _probe(rpt, torch_cuda, tracer, 6, a, b)
    want = np.array([oracle.rng_f32(seed, frame, p, 1)[0] for p in range(n)], dtype=np.float32)
    assert_bit_identical(got, want, "rng")


@pytest.mark.parametrize("w,h,spp", [(64, 48, 4), (160, 120, 8), (100, 75, 3), (17, 9, 2)])
def test_render_matches_oracle(rpt, tracer, oracle, w, h, spp):
    buf = rpt.ColorBuffer(w, h)
    tracer.render_n(buf, spp)
    want = oracle.render(oracle.scene_analytical(), w, h, spp, seed=1)
    assert buf.frames == spp
    assert_bit_identical(buf.image(), want, "render %dx%dx%d" % (w, h, spp))


def test_a_sample_that_is_not_finite_is_blended_as_black(rpt, tracer, oracle, torch_cuda):
    """configs[1]'s frame as bench.py renders it (1920x1080 x 256 spp in one launch on a device buffer, seed 1): sample 188 of
    pixel (row 177, col 1624) and sample 192 of (725, 1817) are NaN (the reference's BSDF on a degenerate direction).  Blended as
    black (kernel_common.h, blend) the frame is finite, and those rows are the oracle's bit for bit."""
    w, h, spp, rows = 1920, 1080, 256, [177, 725]
    desc = oracle.scene_analytical()
    assert np.isnan(oracle.sample_pixels(desc, [1624, 1817], rows, [188, 192], w, h)).all()
    buf = rpt.DeviceColorBuffer(w, h, device="cuda:0")
    tracer.render_n(buf, spp)
    torch_cuda.cuda.synchronize()
    got = buf.pixels.cpu().numpy()
    assert np.isfinite(got).all(), "%d values not finite" % (~np.isfinite(got)).sum()
    want = oracle.render_rows(desc, w, h, spp, rows, seed=1)
    assert_bit_identical(got[rows], want[rows], "rows %s of %dx%dx%d" % (rows, w, h, spp))


@pytest.mark.parametrize("w,h,spp", [(64, 48, 1), (100, 75, 3), (17, 9, 7), (160, 120, 5)])
def test_compact_kernel_matches_oracle(rpt, oracle, w, h, spp):
    """The kernel a one-sample launch of a small scene takes (paths re-dealt through LDS before every stage), forced at other
    sample counts too so that its regeneration path runs; ragged tiles; resumed accumulation; with and without roulette."""
    for rflags in (0, rpt._abi.RPT_RENDER_RUSSIAN_ROULETTE):
        t = rpt.Tracer(rpt.AnalyticalScene(), device=0, seed=4)
        t.flags = rpt._abi.RPT_RENDER_SMALL_COMPACT | rflags
        buf = rpt.ColorBuffer(w, h)
        t.render_n(buf, spp)
        t.render_n(buf, 1)
        want = oracle.render(oracle.scene_analytical(), w, h, spp + 1, seed=4, render_flags=rflags)
        assert_bit_identical(buf.image(), want, "compact kernel %dx%d spp %d flags %d" % (w, h, spp, rflags))
        t.close()


def test_render_800x600_1spp_config1(rpt, tracer, oracle):
    """BASELINE.json configs[0]: the reference's own window size, one render() call."""
    buf = rpt.ColorBuffer(800, 600)
    tracer.render(buf)
    want = oracle.render(oracle.scene_analytical(), 800, 600, 1, seed=1)
    assert_bit_identical(buf.image(), want, "800x600x1")


def test_render_golden_fixture(rpt, tracer):
    import os
    path = os.path.join(os.path.dirname(__file__), "golden", "analytical_64x48_spp4_seed1.npy")
    want = np.load(path)
    buf = rpt.ColorBuffer(64, 48)
    tracer.render_n(buf, 4)
    assert_bit_identical(buf.image(), want, "golden 64x48x4")


def test_folded_spp_equals_repeated_render_calls(rpt, tracer):
    """One launch of S samples == S reference-style render() calls (ColorBuffer.frames semantics)."""
    w, h = 96, 64
    a = rpt.ColorBuffer(w, h)
    for _ in range(6):
        tracer.render(a)
    b = rpt.ColorBuffer(w, h)
    tracer.render_n(b, 6)
    c = rpt.ColorBuffer(w, h)
    tracer.render_n(c, 2)
    tracer.render_n(c, 4)
    assert a.frames == b.frames == c.frames == 6
    assert_bit_identical(a.image(), b.image(), "6x1 vs 1x6")
    assert_bit_identical(a.image(), c.image(), "6x1 vs 2+4")


def test_resume_from_frames(rpt, tracer, oracle):
    """The ColorBuffer is the whole progressive state (buffer.rs:6-14): continuing from frames=5."""
    w, h = 48, 32
    desc = oracle.scene_analytical()
    base = oracle.render(desc, w, h, 5, seed=1)
    want = oracle.render(desc, w, h, 3, seed=1, frames_done=5, pixels=base.copy())
    buf = rpt.ColorBuffer(w, h)
    buf.pixels[:] = base.reshape(-1)
    buf.frames = 5
    tracer.render_n(buf, 3)
    assert_bit_identical(buf.image(), want, "resume")


def test_device_buffer_and_seed(rpt, torch_cuda, oracle):
    w, h, spp = 80, 60, 4
    t = rpt.Tracer(rpt.AnalyticalScene(), device=0, seed=0xDEADBEEF12345)
    buf = rpt.DeviceColorBuffer(w, h)
    t.render_n(buf, spp)
    torch_cuda.cuda.synchronize()
    want = oracle.render(oracle.scene_analytical(), w, h, spp, seed=0xDEADBEEF12345)
    assert_bit_identical(buf.pixels.cpu().numpy(), want, "device buffer, 64-bit seed")
    t.close()


@pytest.mark.parametrize("world,tile_rows", [(2, 2), (3, 4), (8, 2), (4, 16)])
def test_row_tiling_is_independent_of_world(rpt, torch_cuda, tracer, world, tile_rows):
    """Virtual ranks on one GPU: render each rank's tile, concatenate rank-major (what an
    all-gather returns), untile, and compare with the single-GPU image bit for bit."""
    from rust_pathtracer_amd import tiling
    torch = torch_cuda
    w, h, spp = 72, 54, 3
    full = rpt.DeviceColorBuffer(w, h)
    tracer.render_n(full, spp)
    rows_padded = tiling.padded_rows(h, tile_rows, world)
    gathered = torch.zeros(world, rows_padded, w, 4, dtype=torch.float32, device="cuda")
    total = 0
    for r in range(world):
        total += tiling.tile_row_count(h, tile_rows, r, world)
        tracer.render_tile(gathered[r], w, h, 0, spp, tile_rows, r, world)
    assert total == h
    img = tiling.untile(gathered, w, h, tile_rows, world, tracer)
    torch.cuda.synchronize()
    assert_bit_identical(img.cpu().numpy(), full.pixels.cpu().numpy(), "world=%d" % world)


def test_convert_to_u8(rpt, torch_cuda, tracer, oracle):
    w, h = 64, 48
    buf = rpt.DeviceColorBuffer(w, h)
    tracer.render_n(buf, 4)
    # poke edge cases: negative, > 1, NaN, inf
    buf.pixels[0, 0] = torch_cuda.tensor([-1.0, 2.0, float("nan"), float("inf")], device="cuda")
    got = buf.convert_to_u8().cpu().numpy().reshape(-1)
    want = oracle.convert_to_u8(buf.pixels.cpu().numpy(), w, h)
    assert np.array_equal(got, want)


def test_custom_scene_layered_materials_and_max_dist(rpt, oracle):
    """A scene that is not the stock one: 3 spheres, 2 planes, 2 lights, emissive patch,
    transmissive sphere, constant background, any_hit honouring max_dist."""
    s = rpt.Scene()
    s.camera = rpt.Pinhole((0.5, 1.0, 4.0), (0.0, 0.2, 0.0), 65.0)
    s.materials = [
        rpt.Material(rgb=(0.9, 0.9, 0.9), spec_trans=1.0, roughness=0.02, ior=1.45),
        rpt.Material(rgb=(0.2, 0.5, 0.9), sheen=0.7, sheen_tint=0.5, subsurface=0.3, roughness=0.6),
        rpt.Material(rgb=(0.8, 0.7, 0.2), metallic=1.0, anisotropic=0.6, roughness=0.3, specular_tint=0.4),
        rpt.Material(rgb=(0.5, 0.5, 0.5), roughness=0.9),
        rpt.Material(emission=(0.3, 0.1, 0.0), rgb=(0.3, 0.3, 0.3)),
    ]
    s.spheres = [((-1.4, 0.0, 0.0), 1.0, 0), ((1.0, -0.2, 0.3), 0.8, 1), ((0.0, 0.5, -2.0), 1.5, 2)]
    s.planes = [((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), 1e-4, 3), ((0.0, 0.0, 1.0), (0.0, 0.0, -6.0), 1e-4, 4)]
    s.lights = [rpt.AnalyticalLight.spherical((3.0, 3.0, 2.0), 0.7, (6.0, 5.0, 4.0)),
                rpt.AnalyticalLight.spherical((-3.0, 2.5, 1.0), 0.4, (2.0, 3.0, 6.0))]
    s.background = dict(kind=rpt._abi.RPT_BG_CONSTANT, colour_a=(0.05, 0.06, 0.08), colour_b=(0, 0, 0), gamma=2.2, scale=1.0)
    s.any_hit_uses_max_dist = True
    s.max_depth = 6
    w, h, spp = 96, 72, 4
    t = rpt.Tracer(s, device=0, seed=3)
    buf = rpt.ColorBuffer(w, h)
    t.render_n(buf, spp)
    want = oracle.render(s.describe(), w, h, spp, seed=3)
    assert_bit_identical(buf.image(), want, "custom scene")
    t.close()


def test_error_paths(rpt):
    lib = rpt.lib()
    h = C.c_void_p()
    assert lib.rpt_create(C.byref(h), 9999) == rpt._abi.RPT_ERR_INVALID_ARG
    assert lib.rpt_create(C.byref(h), 0) == 0
    px = np.zeros(16, dtype=np.float32)
    assert lib.rpt_render(h, px.ctypes.data, 2, 2, 0, 1, 1, 0) == rpt._abi.RPT_ERR_NO_SCENE
    assert b"no scene" in lib.rpt_last_error(h)
    runaway = rpt.AnalyticalScene()
    runaway.max_depth = 1 << 20
    d = runaway.describe()
    assert lib.rpt_upload_scene(h, C.byref(d)) == rpt._abi.RPT_ERR_INVALID_ARG
    too_many_planes = rpt.Scene()
    too_many_planes.materials = [rpt.Material(rgb=(1, 1, 1))]
    too_many_planes.planes = [((0.0, 1.0, 0.0), (0.0, -float(i), 0.0), 1e-4, 0) for i in range(5)]
    d = too_many_planes.describe()
    assert lib.rpt_upload_scene(h, C.byref(d)) == rpt._abi.RPT_ERR_UNSUPPORTED
    lib.rpt_destroy(h)


def test_cpp_host_mirror_runs_the_reference_main_loop(rpt, oracle, tmp_path):
    """include/rpt.hpp (C++ mirror of ColorBuffer / AnalyticalScene / Tracer) driven like
    renderer/src/main.rs:36-42,118-122 — BASELINE.json configs[0]'s 800x600 frame, host buffers,
    render + convert_to_u8 per frame — must equal the oracle bit for bit."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "render_cpp")
    deps = [os.path.join(root, "include", "rpt.h"), os.path.join(root, "include", "rpt.hpp"), os.path.join(root, "examples", "render_cpp.cpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "render_cpp.cpp"),
                        "-L", os.path.join(root, "rust-pathtracer_amd"), "-lrpt_hip",
                        "-Wl,-rpath," + os.path.join(root, "rust-pathtracer_amd"), "-o", exe], check=True)
    w, h, frames = 800, 600, 2
    base = str(tmp_path / "out")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(root, "rust-pathtracer_amd") + ":" + env.get("LD_LIBRARY_PATH", "")
    subprocess.run([exe, str(w), str(h), str(frames), base], check=True, env=env)
    got = np.fromfile(base + ".f32", dtype=np.float32).reshape(h, w, 4)
    want = oracle.render(oracle.scene_analytical(), w, h, frames, seed=1)
    assert_bit_identical(got, want, "C++ mirror 800x600x2")
    got8 = np.fromfile(base + ".u8", dtype=np.uint8)
    assert np.array_equal(got8, oracle.convert_to_u8(want, w, h))


@pytest.mark.parametrize("n_spheres,n_lights", [(300, 16), (9, 2), (40, 5), (3000, 16), (64, 1)])
def test_large_scene_matches_oracle(rpt, oracle, n_spheres, n_lights):
    """BASELINE.json configs[4]'s shape at a size the oracle finishes in seconds: random spheres with
    full materials, a checker plane, a grid of spherical lights; the kernel streams the tables from HBM."""
    from rust_pathtracer_amd import scenes
    s = scenes.random_spheres_scene(n_spheres=n_spheres, n_lights=n_lights, seed=0x5EED0005)
    w, h, spp = 96, 54, 3
    t = rpt.Tracer(s, device=0, seed=5)
    # (from 64 spheres up: the grid walk inside the megakernel; below: its brute-force loops)
    for flags in (0,):
        t.flags = flags
        buf = rpt.ColorBuffer(w, h)
        t.render_n(buf, spp)
        want = oracle.render(s.describe(), w, h, spp, seed=5)
        assert_bit_identical(buf.image(), want, "large scene %d spheres flags=%d" % (n_spheres, flags))
    t.close()


@pytest.mark.parametrize("cam,look,reach", [((0.0, 60.0, 330.0), (0.0, 4.0, -60.0), None), ((250.0, 9.0, -60.0), (0.0, 5.0, -60.0), None),
                                            ((0.0, 6.0, 14.0), (0.0, 2.0, -40.0), "0"), ((0.0, 6.0, 14.0), (0.0, 2.0, -40.0), "0.6")])
def test_large_scene_both_tiers_of_cell_lists(rpt, oracle, cam, look, reach, monkeypatch):
    """The grid keeps two tiers of cell lists (host_scene.h: less padding, shorter lists, for ray origins near the grid).  A camera
    beyond the near tier's reach sends its primary rays through the far tier and every bounce through the near one; then the
    benchmark's camera with the near tier switched off and with a reach that ends inside the scene (paths change tier as they
    bounce).  All bit-identical to the oracle's ordered loop over every sphere, in both forms."""
    from rust_pathtracer_amd import scenes
    if reach is not None:
        monkeypatch.setenv("RPT_GRID_NEAR_REACH", reach)              # (the library reads its knobs once per process:
        rpt.lib().rpt_debug_reload_knobs()                            #  the test build's hook reads them again)
    s = scenes.random_spheres_scene(n_spheres=1200, n_lights=9, seed=0x5EED0011)
    s.camera = rpt.Pinhole(cam, look, 40.0)
    w, h, spp = 112, 63, 3
    t = rpt.Tracer(s, device=0, seed=7)
    want = oracle.render(s.describe(), w, h, spp, seed=7)
    for flags in (0,):
        t.flags = flags
        buf = rpt.ColorBuffer(w, h)
        t.render_n(buf, spp)
        assert_bit_identical(buf.image(), want, "tiers cam=%s reach=%s flags=%d" % (cam, reach, flags))
    t.close()


@pytest.mark.parametrize("w,h,spp,depth,rr", [(70, 37, 5, 4, False), (33, 65, 3, 9, True), (200, 120, 2, 1, False), (64, 64, 40, 30, True)])
def test_large_scene_ragged_tiles_deep_paths_and_resume(rpt, oracle, w, h, spp, depth, rr):
    """Large scenes over ragged tiles (sizes that are not multiples of the 16x16 tile), depth 1, deep paths with Russian roulette,
    and a resumed accumulation: bit-identical to the oracle."""
    from rust_pathtracer_amd import scenes
    s = scenes.random_spheres_scene(n_spheres=400, n_lights=5, seed=0x5EED0007)
    s.max_depth = depth
    rflags = rpt._abi.RPT_RENDER_RUSSIAN_ROULETTE if rr else 0
    t = rpt.Tracer(s, device=0, seed=9)
    t.flags = rflags
    buf = rpt.ColorBuffer(w, h)
    t.render_n(buf, spp)
    t.render_n(buf, 2)                                                # resumes at frames_done = spp
    want = oracle.render(s.describe(), w, h, spp + 2, seed=9, render_flags=rflags)
    assert_bit_identical(buf.image(), want, "large scene %dx%d spp %d depth %d" % (w, h, spp, depth))
    t.close()


def test_large_scene_needs_full_sphere_materials(rpt):
    s = rpt.Scene()
    s.materials = [rpt.Material(rgb=(1, 1, 1))]                    # a partial patch
    s.spheres = [((float(i), 0.0, 0.0), 0.4, 0) for i in range(9)]
    h = C.c_void_p()
    assert rpt.lib().rpt_create(C.byref(h), 0) == 0
    d = s.describe()
    assert rpt.lib().rpt_upload_scene(h, C.byref(d)) == rpt._abi.RPT_ERR_UNSUPPORTED
    assert b"full sphere materials" in rpt.lib().rpt_last_error(h)
    rpt.lib().rpt_destroy(h)


def test_sdf_scene_matches_oracle(rpt, oracle):
    """BASELINE.json configs[3]: sphere-marched smooth-union blob (divergent march lengths), analytical
    sphere, checker plane, spherical light — bit-identical to the oracle in all three kernel forms (resumable
    march, march inside the bounce, nested loops)."""
    from rust_pathtracer_amd import scenes
    w, h, spp = 128, 72, 4
    for use_max in (False, True):                  # shadow marches may stop at max_dist only when any_hit honours it
        s = scenes.sdf_scene()
        s.any_hit_uses_max_dist = use_max
        t = rpt.Tracer(s, device=0, seed=9)
        want = oracle.render(s.describe(), w, h, spp, seed=9)
        for flags in (0,):
            t.flags = flags
            buf = rpt.ColorBuffer(w, h)
            t.render_n(buf, spp)
            assert_bit_identical(buf.image(), want, "sdf scene use_max=%s flags=%d" % (use_max, flags))
        t.close()


@pytest.mark.parametrize("w,h", [(13, 11), (43, 21), (65, 9), (23, 17), (9, 41)])
def test_sdf_marches_handed_between_lanes_in_partly_filled_waves(rpt, oracle, w, h):
    """The SDF march kernel hands a waiting path march to an idle lane of its wave, pairing offers and idle lanes by rank with
    ballots, ds_permute and ds_bpermute (k_sdf.hip) — which is only right while every lane the ranks can name is alive.  Frames whose
    width is 1..7 mod 8 (and heights off the 8-row grid) have waves with 1 to 7 live columns: lanes without a pixel must neither
    break the pairing (a bpermute that names a lane that has left the kernel reads 0, i.e. takes lane 0's march: ADVICE r5) nor be
    lost as helpers.  Depth 4, enough samples that many shadow marches are in flight with path marches behind them; every kernel
    form an SDF scene can take (sized / table / general), with and without max_dist in any_hit; bit for bit against the oracle."""
    from rust_pathtracer_amd import scenes
    for use_max, spp, env in ((False, 9, {}), (True, 5, {}), (False, 6, {"RPT_NO_SIZED_KERNELS": "1"}),
                              (False, 6, {"RPT_NO_SIZED_KERNELS": "1", "RPT_NO_MATERIAL_TABLE": "1"})):
        s = scenes.sdf_scene()
        s.any_hit_uses_max_dist = use_max
        assert s.recursion_depth() >= 3
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        rpt.lib().rpt_debug_reload_knobs()
        try:
            t = rpt.Tracer(s, device=0, seed=17)
            buf = rpt.ColorBuffer(w, h)
            t.render_n(buf, spp)
            t.render_n(buf, 2)                                      # and once more on top (the running mean carries over)
            t.close()
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            rpt.lib().rpt_debug_reload_knobs()
        want = oracle.render(s.describe(), w, h, spp + 2, seed=17)
        assert_bit_identical(buf.image(), want, "sdf scene %dx%d x %d spp, use_max=%s %s" % (w, h, spp + 2, use_max, env))


@pytest.mark.parametrize("room,min_lanes", [(1, 8), (17, 3), (40, 1), (64, 8), (64, 64)])
def test_sdf_second_room_at_its_ends(rpt, oracle, room, min_lanes):
    """The SDF march kernel cuts its block behind closest_hit's acceptance: surface hits wait in a room of their own until
    RPT_SDF_SHADE_ROOM lanes do (default 40; k_sdf.hip), beside the march phases' own minimum (RPT_SDF_MARCH_MIN_LANES).  Neither knob
    can change a pixel — they decide WHEN a lane's next block runs — at their ends least of all: a room that fires for one lane, one
    that needs the whole wave (and therefore mostly fires because nobody else can go on), march phases of one lane or of none below 64."""
    from rust_pathtracer_amd import scenes
    s = scenes.sdf_scene()
    w, h, spp = 83, 45, 7
    old = {k: os.environ.get(k) for k in ("RPT_SDF_SHADE_ROOM", "RPT_SDF_MARCH_MIN_LANES")}
    os.environ.update(RPT_SDF_SHADE_ROOM=str(room), RPT_SDF_MARCH_MIN_LANES=str(min_lanes))
    rpt.lib().rpt_debug_reload_knobs()
    try:
        t = rpt.Tracer(s, device=0, seed=23)
        buf = rpt.ColorBuffer(w, h)
        t.render_n(buf, spp)
        t.close()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        rpt.lib().rpt_debug_reload_knobs()
    assert_bit_identical(buf.image(), oracle.render(s.describe(), w, h, spp, seed=23), "sdf scene, second room at %d lanes, march phases of >= %d" % (room, min_lanes))


def _with_ground_sphere(s, where):
    """The classic r = 1000 ground sphere in a field of small ones: far beyond 8 x the median radius, so the grid keeps it out
    and every walk tests it up front (host_scene.h, pick_oversize) — as sphere 0 (the unconditional first test of
    analytical.rs:43) or as the last one."""
    from rust_pathtracer_amd import scenes
    s.materials.append(scenes.full_material(rgb=(0.4, 0.5, 0.3), roughness=0.9))
    ground = ((0.0, -1001.5, -60.0), 1000.0, len(s.materials) - 1)
    if where == "first":
        s.spheres.insert(0, ground)
    else:
        s.spheres.append(ground)
    return s


@pytest.mark.parametrize("n_spheres,ground", [(64, None), (3000, None), (1500, "first"), (1500, "last")])
def test_grid_queries_equal_brute_force(rpt, torch_cuda, n_spheres, ground):
    """The uniform grid must answer exactly like the reference's ordered loop over all spheres: nearest t
    (bitwise), winning index, and any-hit, for rays from everywhere — floor points, sphere surfaces at
    grazing angles, the camera, and origins tens of thousands of units away, where the f32 sphere test is
    noise and the grid hands the ray to the brute-force loop."""
    from rust_pathtracer_amd import scenes
    torch = torch_cuda
    s = scenes.random_spheres_scene(n_spheres=n_spheres, n_lights=16, seed=0x5EED0005)
    if ground:
        _with_ground_sphere(s, ground)
        n_spheres += 1
    t = rpt.Tracer(s, device=0, seed=5)
    rng = np.random.default_rng(n_spheres)
    N = 1_000_000
    sph = np.array([list(c) + [r] for c, r, m in s.spheres], dtype=np.float32)
    pick = rng.integers(0, n_spheres, N)
    nrm = rng.normal(size=(N, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    o = sph[pick, :3] + (sph[pick, 3:4] + 0.005) * nrm
    third = N // 3
    o[:third] = np.stack([rng.uniform(-70, 70, third), np.full(third, -0.995), rng.uniform(-130, 10, third)], axis=1)
    o[third:third + 1000] = (0.0, 6.0, 14.0)
    d = rng.normal(size=(N, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    tang = np.cross(nrm, d); tang /= np.linalg.norm(tang, axis=1, keepdims=True) + 1e-30
    graz = tang + nrm * rng.normal(scale=0.02, size=(N, 1)); graz /= np.linalg.norm(graz, axis=1, keepdims=True)
    d[2 * third:] = graz[2 * third:]
    far = rng.integers(0, N, N // 10)
    o[far] = o[far] - d[far] * rng.uniform(50.0, 60000.0, (len(far), 1))
    maxd = rng.uniform(0.5, 150.0, N); maxd[far] = rng.uniform(10.0, 1e5, len(far))
    rays = torch.from_numpy(np.concatenate([o, d, maxd[:, None]], axis=1).astype(np.float32)).cuda()
    res = []
    for use_grid in (1, 0):
        out = torch.zeros(N, 3, dtype=torch.int32, device="cuda")
        rpt._lib.check(rpt.lib().rpt_probe_rays(t._h, rays.data_ptr(), out.data_ptr(), N, use_grid, None), t._h)
        torch.cuda.synchronize()
        res.append(out.cpu().numpy())
    assert (res[1][:, 1] != -1).sum() > N // 20 and res[1][:, 2].sum() > N // 20      # the sample does hit things
    assert np.array_equal(res[0], res[1])
    t.close()


@pytest.mark.parametrize("n_spheres", [800, 10000])
def test_grid_queries_at_the_reach_of_each_tier(rpt, torch_cuda, n_spheres):
    """The cell lists of a tier are padded for the FARTHEST origin the tier serves (host_scene.h): rays from just inside and just
    outside the near tier's reach (1.5 half-diagonals of the grid box) and the far tier's (6), aimed to graze spheres all over the scene
    — where the reference's f32 test is at its noisiest for that tier — must still be answered like the loop over all spheres."""
    from rust_pathtracer_amd import scenes
    torch = torch_cuda
    s = scenes.random_spheres_scene(n_spheres=n_spheres, n_lights=4, seed=0x5EED0021)
    t = rpt.Tracer(s, device=0, seed=5)
    rng = np.random.default_rng(n_spheres + 1)
    sph = np.array([list(c) + [r] for c, r, m in s.spheres], dtype=np.float64)
    lo, hi = (sph[:, :3] - sph[:, 3:4]).min(0), (sph[:, :3] + sph[:, 3:4]).max(0)
    centre, hd = 0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo)
    N = 400_000
    shell = rng.choice([1.5 * 0.98, 1.5 * 0.999, 1.5 * 1.002, 1.5 * 1.03, 6.0 * 0.97, 6.0 * 0.999, 6.0 * 1.002], N)
    u = rng.normal(size=(N, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = centre + (shell * hd)[:, None] * u
    pick = rng.integers(0, n_spheres, N)
    to_c = sph[pick, :3] - o
    dist = np.linalg.norm(to_c, axis=1, keepdims=True)
    perp = np.cross(to_c, rng.normal(size=(N, 3))); perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    miss = sph[pick, 3:4] + rng.normal(scale=0.03, size=(N, 1)) * (1.0 + dist / 200.0)      # pass this far from the centre: grazing, in and out
    d = to_c + perp * miss; d /= np.linalg.norm(d, axis=1, keepdims=True)
    maxd = rng.uniform(0.5, 2.0, N) * dist[:, 0]
    rays = torch.from_numpy(np.concatenate([o, d, maxd[:, None]], axis=1).astype(np.float32)).cuda()
    res = []
    for use_grid in (1, 0):
        out = torch.zeros(N, 3, dtype=torch.int32, device="cuda")
        rpt._lib.check(rpt.lib().rpt_probe_rays(t._h, rays.data_ptr(), out.data_ptr(), N, use_grid, None), t._h)
        torch.cuda.synchronize()
        res.append(out.cpu().numpy())
    assert (res[1][:, 1] != -1).sum() > N // 10                     # grazing rays do hit
    assert np.array_equal(res[0], res[1])
    t.close()


@pytest.mark.parametrize("where", ["first", "last"])
def test_scene_with_a_giant_ground_sphere_matches_oracle(rpt, torch_cuda, oracle, where):
    from rust_pathtracer_amd import scenes
    s = _with_ground_sphere(scenes.random_spheres_scene(n_spheres=600, n_lights=4), where)
    s.planes = []                                           # the ground sphere is the floor
    w, h, spp = 96, 64, 3
    t = rpt.Tracer(s, device=0, seed=9)
    buf = rpt.DeviceColorBuffer(w, h)
    t.render_n(buf, spp)
    torch_cuda.cuda.synchronize()
    assert_bit_identical(buf.pixels.cpu().numpy(), oracle.render(s.describe(), w, h, spp, seed=9), "ground sphere %s" % where)
    t.close()


def _oracle_rows(oracle, desc, w, h, spp, rows, seed=1):
    """The oracle's version of complete rows of a full-size frame (row ranges are independent)."""
    out = {}
    for r in rows:
        px = np.zeros((h, w, 4), dtype=np.float32)
        oracle.render(desc, w, h, spp, seed=seed, pixels=px, rows=(r, r + 1))
        out[r] = px[r].copy()
    return out


def _every_pixel_is_finite(oracle, desc, img, w, h, spp, seed=1, limit=4):
    """The reference has no NaN guards: over 5e8 samples a few hit a 0/0 of the BSDF code.  Such a sample is
    blended as black (kernel_common.h, blend), so no pixel of the frame is NaN or infinite; if one is, its rows are compared with the
    oracle's before the test fails, to tell the kernel's fault from the oracle's."""
    bad = np.argwhere(~np.isfinite(img).all(axis=2))
    for r in sorted({int(b[0]) for b in bad})[:limit]:
        assert_bit_identical(img[r], _oracle_rows(oracle, desc, w, h, spp, (r,), seed)[r], "row %d (has a non-finite pixel)" % r)
    assert len(bad) == 0, "%d pixels not finite, first %s" % (len(bad), bad[:4].tolist())


def test_full_size_config2_rows_match_oracle(rpt, torch_cuda, tracer, oracle):
    """BASELINE.json configs[1] at FULL size: AnalyticalScene 1920x1080 x 256 spp on the GPU; the oracle
    recomputes complete rows through the sky, the spheres and the floor and they must be bit-identical.
    Also at full size: the frame does not depend on the row tiling (8 virtual ranks) and is deterministic."""
    from rust_pathtracer_amd import tiling
    torch = torch_cuda
    w, h, spp = 1920, 1080, 256
    buf = rpt.DeviceColorBuffer(w, h)
    tracer.render_n(buf, spp)
    torch.cuda.synchronize()
    img = buf.pixels.cpu().numpy()
    assert np.all(img[..., 3] == 1.0)
    _every_pixel_is_finite(oracle, oracle.scene_analytical(), img, w, h, spp)
    for r, want in _oracle_rows(oracle, oracle.scene_analytical(), w, h, spp, (37, 541, 1003)).items():
        assert_bit_identical(img[r], want, "c2 row %d" % r)
    # tiling independence + determinism at full size (checksums over the whole frame)
    world, tile_rows = 8, 2
    gathered = torch.zeros(world, tiling.padded_rows(h, tile_rows, world), w, 4, dtype=torch.float32, device="cuda")
    for r in range(world):
        tracer.render_tile(gathered[r], w, h, 0, spp, tile_rows, r, world)
    tiled = tiling.untile(gathered, w, h, tile_rows, world, tracer)
    torch.cuda.synchronize()
    assert torch.equal(tiled.view(torch.int32), buf.pixels.view(torch.int32))


def test_full_size_config3_rank_tile_matches_oracle(rpt, torch_cuda, tracer, oracle):
    """BASELINE.json configs[2] at FULL size, one rank's share: 3840x2160 x 1024 spp row-tiled over 8 GPUs
    (cyclic 2-row blocks); this test renders rank 3's tile (270 rows) and checks two of its rows (global
    rows 6 and 1638) against the oracle bit for bit."""
    from rust_pathtracer_amd import tiling
    torch = torch_cuda
    w, h, spp, world, tile_rows, rank = 3840, 2160, 1024, 8, 2, 3
    rows = tiling.tile_global_rows(h, tile_rows, rank, world)
    assert len(rows) == 270
    tile = torch.zeros(len(rows), w, 4, dtype=torch.float32, device="cuda")
    tracer.render_tile(tile, w, h, 0, spp, tile_rows, rank, world)
    torch.cuda.synchronize()
    got = tile.cpu().numpy()
    for lr in (0, 204):
        g = rows[lr]
        want = _oracle_rows(oracle, oracle.scene_analytical(), w, h, spp, (g,))[g]
        assert_bit_identical(got[lr], want, "c3 rank %d local row %d (global %d)" % (rank, lr, g))


def _random_small_scene(rpt, rng):
    A = rpt._abi
    s = rpt.Scene()
    s.camera = rpt.Pinhole(tuple(rng.uniform(-1, 1, 3) + (0, 0.5, 4)), tuple(rng.uniform(-0.5, 0.5, 3)), float(rng.uniform(30, 100)))
    if rng.random() < 0.5:
        s.background = dict(kind=A.RPT_BG_GRADIENT_Y, colour_a=tuple(rng.uniform(0.5, 1, 3)), colour_b=tuple(rng.uniform(0.2, 1, 3)),
                            gamma=float(rng.choice([2.2, 1.0, 0.4545])), scale=float(rng.uniform(0.2, 1)))
    else:
        s.background = dict(kind=A.RPT_BG_CONSTANT, colour_a=tuple(rng.uniform(0, 0.5, 3)), colour_b=(0, 0, 0), gamma=2.2, scale=1.0)
    fields = {"rgb": lambda: tuple(rng.uniform(0, 1, 3)), "emission": lambda: tuple(rng.uniform(0, 0.5, 3) * (rng.random() < 0.3)),
              "anisotropic": lambda: float(rng.uniform(0, 1)), "metallic": lambda: float(rng.choice([0.0, 1.0, rng.uniform(0, 1)])),
              "roughness": lambda: float(rng.choice([0.0, 0.001, rng.uniform(0.02, 1)])), "subsurface": lambda: float(rng.uniform(0, 1)),
              "specular_tint": lambda: float(rng.uniform(0, 1)), "sheen": lambda: float(rng.uniform(0, 1)), "sheen_tint": lambda: float(rng.uniform(0, 1)),
              "clearcoat": lambda: float(rng.choice([0.0, 1.0])), "clearcoat_gloss": lambda: float(rng.uniform(0, 1)),
              "spec_trans": lambda: float(rng.choice([0.0, 0.0, 1.0, rng.uniform(0, 1)])), "ior": lambda: float(rng.uniform(1.05, 2.2))}
    n_mat = int(rng.integers(1, 9))
    s.materials = []
    for _ in range(n_mat):
        names = [k for k in fields if rng.random() < 0.4]
        kw = {k: fields[k]() for k in names}
        checker = (0.5, 100.0, float(rng.uniform(0.1, 0.9)), float(rng.uniform(0.0, 0.3))) if rng.random() < 0.2 else None
        s.materials.append(rpt.Material(checker_dir=checker, **kw))
    s.spheres = [(tuple(rng.uniform(-2, 2, 3) * (1, 0.6, 1)), float(rng.uniform(0.3, 1.1)), int(rng.integers(0, n_mat)))
                 for _ in range(int(rng.integers(0, 9)))]
    s.planes = []
    for _ in range(int(rng.integers(0, 5))):
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        if rng.random() < 0.6:
            n = np.array([0.0, 1.0, 0.0])
        s.planes.append((tuple(n), tuple(-n * rng.uniform(1.0, 3.0)), 1e-4, int(rng.integers(0, n_mat)), float(rng.choice([0.0, 0.0, 25.0]))))
    s.lights = [rpt.AnalyticalLight.spherical(tuple(rng.uniform(-4, 4, 3) + (0, 3, 0)), float(rng.uniform(0.2, 1.2)), tuple(rng.uniform(1, 8, 3)))
                for _ in range(int(rng.integers(0, 5)))]
    if s.lights and rng.random() < 0.2:                      # the declared-but-unsampled light types are no-ops (tracer.rs:217)
        s.lights[0].light_type = int(rng.choice([A.RPT_LIGHT_RECTANGULAR, A.RPT_LIGHT_DISTANT]))
    s.max_depth = int(rng.integers(1, 7))
    s.eps = float(rng.choice([0.005, 0.001, 0.02]))
    s.any_hit_uses_max_dist = bool(rng.random() < 0.5)
    return s


@pytest.mark.parametrize("seed", range(48))
def test_random_small_scenes_match_oracle(rpt, oracle, seed):
    """Fuzz: random primitive counts (including none), partial material patches (so the layering of
    analytical.rs:56-58/82-85 matters), emissive / transmissive / anisotropic materials, both backgrounds,
    depth 1-6, both any_hit modes, finite planes, unsampled light types, odd image sizes."""
    rng = np.random.default_rng(1000 + seed)
    s = _random_small_scene(rpt, rng)
    w, h, spp = int(rng.integers(1, 70)), int(rng.integers(1, 50)), int(rng.integers(1, 4))
    t = rpt.Tracer(s, device=0, seed=seed)
    # a third each: nested loops; the default (one-sample launches: the compacting kernel, otherwise the megakernel); the
    # compacting kernel forced
    t.flags = (rpt._abi.RPT_RENDER_NESTED_LOOPS, 0, rpt._abi.RPT_RENDER_SMALL_COMPACT)[seed % 3]
    buf = rpt.ColorBuffer(w, h)
    t.render_n(buf, spp)
    want = oracle.render(s.describe(), w, h, spp, seed=seed)
    assert_bit_identical(buf.image(), want, "fuzz seed %d (%dx%d x%d, %d spheres %d planes %d lights depth %d)" %
                         (seed, w, h, spp, len(s.spheres), len(s.planes), len(s.lights), s.max_depth))
    t.close()


@pytest.mark.parametrize("seed", range(16))
def test_random_large_scenes_match_oracle_in_both_forms(rpt, oracle, seed):
    """Fuzz the large-scene path: 64-500 spheres of mixed sizes (sometimes a giant one, kept out of the grid), 0-6 lights
    (none: no shadow rays at all), 0-2 planes (finite or not), depth 1-6, both any_hit modes, roulette now and then, odd frame
    sizes — the wavefront form and the megakernel, each against the oracle."""
    from rust_pathtracer_amd import scenes
    A = rpt._abi
    rng = np.random.default_rng(9000 + seed)
    s = scenes.random_spheres_scene(n_spheres=int(rng.integers(64, 500)), n_lights=int(rng.integers(0, 7)), seed=int(rng.integers(1, 2**31)))
    if seed % 4 == 0:
        c, _, m = s.spheres[int(rng.integers(0, len(s.spheres)))]
        s.spheres[int(rng.integers(0, len(s.spheres)))] = ((0.0, -500.0, -60.0), 499.5, m)            # a ground sphere
    if seed % 5 == 1:
        s.planes = []
    elif seed % 5 == 2:
        s.planes = s.planes + [((0.0, 0.0, 1.0), (0.0, 0.0, -130.0), 1e-4, s.planes[0][3], 0.0)]      # a back wall, infinite
    s.max_depth = int(rng.integers(1, 7))
    s.any_hit_uses_max_dist = bool(rng.random() < 0.5)
    w, h, spp = int(rng.integers(8, 90)), int(rng.integers(8, 60)), int(rng.integers(1, 4))
    rflags = A.RPT_RENDER_RUSSIAN_ROULETTE if seed % 3 == 0 else 0
    want = oracle.render(s.describe(), w, h, spp, seed=seed, render_flags=rflags)
    t = rpt.Tracer(s, device=0, seed=seed)
    for form in (0,):
        t.flags = form | rflags
        buf = rpt.ColorBuffer(w, h)
        t.render_n(buf, spp)
        assert_bit_identical(buf.image(), want, "large fuzz seed %d form %d (%dx%d x%d, %d spheres %d lights %d planes depth %d)" %
                             (seed, form, w, h, spp, len(s.spheres), len(s.lights), len(s.planes), s.max_depth))
    t.close()


def _random_sdf_scene(rpt, seed):
    """-> (scene, rng, prims): 1-8 random spheres/tori, any smoothing radius, short and long step budgets, on top of a random analytical
    scene (none at all when seed % 4 == 1, no lights when seed % 4 == 2).  Also tests/test_media_sdf_f64.py's SDF fuzz."""
    A = rpt._abi
    rng = np.random.default_rng(7000 + seed)
    s = _random_small_scene(rpt, rng)
    if seed % 4 == 1:
        s.spheres, s.planes = [], []
    if seed % 4 == 2:
        s.lights = []
    prims = []
    for _ in range(int(rng.integers(1, 9))):
        c = tuple(rng.uniform(-1.5, 1.5, 3) * (1, 0.5, 1))
        if rng.random() < 0.4:
            prims.append((A.RPT_SDF_TORUS_Y, c, (float(rng.uniform(0.4, 1.3)), float(rng.uniform(0.08, 0.3)))))
        else:
            prims.append((A.RPT_SDF_SPHERE, c, (float(rng.uniform(0.2, 0.9)), 0.0)))
    s.sdf = dict(prims=prims, material=int(rng.integers(0, len(s.materials))), smooth_k=float(rng.choice([0.05, 0.35, 1.0])),
                 max_steps=int(rng.choice([1, 7, 48, 200])), hit_eps=float(rng.choice([1e-3, 1e-2])), max_t=float(rng.choice([8.0, 60.0])),
                 normal_eps=float(rng.choice([1e-3, 1e-2])))
    return s, rng, prims


@pytest.mark.parametrize("seed", range(20))
def test_random_sdf_scenes_match_oracle(rpt, oracle, seed):
    """Fuzz the SDF object: 1-8 random spheres/tori, any smoothing radius, short and long step budgets, on top of
    random analytical scenes (including none at all, where the SDF hit is accepted unconditionally, and no
    lights, where no shadow ray is marched) — in all three kernel forms."""
    s, rng, prims = _random_sdf_scene(rpt, seed)
    w, h, spp = int(rng.integers(8, 90)), int(rng.integers(8, 60)), int(rng.integers(1, 4))
    want = oracle.render(s.describe(), w, h, spp, seed=seed)
    t = rpt.Tracer(s, device=0, seed=seed)
    for flags in (0,):
        t.flags = flags
        buf = rpt.ColorBuffer(w, h)
        t.render_n(buf, spp)
        assert_bit_identical(buf.image(), want, "sdf fuzz seed %d flags %d (%dx%d x%d, %d sdf prims, %d spheres %d planes %d lights depth %d)" %
                             (seed, flags, w, h, spp, len(prims), len(s.spheres), len(s.planes), len(s.lights), s.max_depth))
    t.close()


def test_full_size_config4_sdf_rows_match_oracle(rpt, torch_cuda, oracle):
    """BASELINE.json configs[3] at FULL size: the SDF sphere-march scene 1920x1080 x 64 spp; rows through
    the sky, the blob and the floor recomputed by the oracle, bit-identical."""
    from rust_pathtracer_amd import scenes
    s = scenes.sdf_scene()
    w, h, spp = 1920, 1080, 64
    t = rpt.Tracer(s, device=0, seed=1)
    buf = rpt.DeviceColorBuffer(w, h)
    t.render_n(buf, spp)
    torch_cuda.cuda.synchronize()
    img = buf.pixels.cpu().numpy()
    _every_pixel_is_finite(oracle, s.describe(), img, w, h, spp)
    for r, want in _oracle_rows(oracle, s.describe(), w, h, spp, (150, 620, 1000)).items():
        assert_bit_identical(img[r], want, "c4 row %d" % r)
    t.close()


def test_full_size_config5_frame(rpt, torch_cuda, oracle):
    """BASELINE.json configs[4] at FULL resolution (10 000 spheres + 16 lights, 4096x4096; 2 of its 512 spp,
    the oracle's brute force being what it is): two complete rows bit-identical to the oracle, and the
    WHOLE frame identical between the grid traversal and the brute-force loops on the GPU."""
    import os
    from rust_pathtracer_amd import scenes
    torch = torch_cuda
    s = scenes.random_spheres_scene(10000, 16)
    w, h, spp = 4096, 4096, 2
    t = rpt.Tracer(s, device=0, seed=1)
    grid = rpt.DeviceColorBuffer(w, h)
    t.render_n(grid, spp)
    torch.cuda.synchronize()
    img = grid.pixels.cpu().numpy()
    for r, want in _oracle_rows(oracle, s.describe(), w, h, spp, (1800, 3000)).items():
        assert_bit_identical(img[r], want, "c5 row %d" % r)
    os.environ["RPT_NO_GRID"] = "1"
    rpt.lib().rpt_debug_reload_knobs()                     # (knobs are read once per process: the test build's hook reads them again)
    try:
        t.upload_scene()                                   # re-upload without the grid
        brute = rpt.DeviceColorBuffer(w, h)
        t.render_n(brute, spp)
        torch.cuda.synchronize()
    finally:
        del os.environ["RPT_NO_GRID"]
    assert torch.equal(brute.pixels.view(torch.int32), grid.pixels.view(torch.int32))
    t.close()


def test_full_config5_all_512_spp_pixels_match_oracle(rpt, torch_cuda, oracle):
    """BASELINE.json configs[4] in FULL: 10 000 spheres + 16 lights, 4096x4096, all 512 spp (8.6 G samples, one launch
    sequence).  The oracle cannot brute-force whole rows of that in test time, so it recomputes 512 pixels spread over the
    frame: the radiance of each of their 512 samples (sample_pixels), folded into the running mean with the reference's
    expression in f32 (tracer.rs:105-117) — bit-identical to the GPU's pixels."""
    from rust_pathtracer_amd import scenes
    torch = torch_cuda
    s = scenes.random_spheres_scene(10000, 16)
    w, h, spp = 4096, 4096, 512
    t = rpt.Tracer(s, device=0, seed=1)
    buf = rpt.DeviceColorBuffer(w, h)
    t.render_n(buf, spp)
    torch.cuda.synchronize()
    assert buf.frames == spp
    rng = np.random.default_rng(5)
    cols = rng.integers(0, w, size=512).astype(np.uint32)
    rows = np.concatenate([rng.integers(h // 2, h, size=448), rng.integers(0, h // 2, size=64)]).astype(np.uint32)   # mostly below the horizon
    got = buf.pixels[torch.from_numpy(rows.astype(np.int64)).cuda(), torch.from_numpy(cols.astype(np.int64)).cuda()].cpu().numpy()
    desc = s.describe()
    rad = oracle.sample_pixels(desc, np.repeat(cols, spp), np.repeat(rows, spp), np.tile(np.arange(spp, dtype=np.uint64), len(cols)), w, h, seed=1)
    rad = rad.reshape(len(cols), spp, 3)
    acc = np.zeros((len(cols), 4), dtype=np.float32)
    one = np.float32(1.0)
    for k in range(spp):
        v = one / np.float32(k + 1)                                                        # tracer.rs:115
        colour = np.concatenate([rad[:, k, :], np.ones((len(cols), 1), dtype=np.float32)], axis=1)
        acc = (one - v) * acc + colour * v                                                 # mix_color, tracer.rs:108-113
    assert_bit_identical(got, acc, "c5, 512 spp, 512 pixels")
    t.close()


def test_reserved_flag_bits_are_refused(rpt, torch_cuda):
    """Until ABI 3 seven more render flags named measured-slower kernel forms kept for A/B runs; the forms are gone and their bits
    are reserved: the library answers them with RPT_ERR_INVALID_ARG instead of silently running something else."""
    from rust_pathtracer_amd import scenes
    t = rpt.Tracer(scenes.sdf_scene(), device=0, seed=1)
    buf = rpt.DeviceColorBuffer(16, 16)
    for bit in (2, 3, 4, 6, 7, 9, 10, 11, 31):
        t.flags = 1 << bit
        with pytest.raises(rpt.RptError) as e:
            t.render_n(buf, 1)
        assert e.value.status == rpt._abi.RPT_ERR_INVALID_ARG
    # the nested-loop baseline exists for the reference's scene class only
    t.flags = rpt._abi.RPT_RENDER_NESTED_LOOPS
    with pytest.raises(rpt.RptError) as e:
        t.render_n(buf, 1)
    assert e.value.status == rpt._abi.RPT_ERR_UNSUPPORTED
    t.close()


def test_two_contexts_on_two_threads(rpt, oracle):
    """A context is used by one thread at a time, but different contexts may run concurrently
    (the reference's Tracer is Send; include/rpt.h conventions)."""
    import threading
    results = {}

    def work(name, seed):
        t = rpt.Tracer(rpt.AnalyticalScene(), device=0, seed=seed)
        buf = rpt.ColorBuffer(120, 90)
        for _ in range(4):
            t.render_n(buf, 2)
        results[name] = buf.image().copy()
        t.close()

    threads = [threading.Thread(target=work, args=("a", 21)), threading.Thread(target=work, args=("b", 22))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    d = oracle.scene_analytical()
    assert_bit_identical(results["a"], oracle.render(d, 120, 90, 8, seed=21), "thread a")
    assert_bit_identical(results["b"], oracle.render(d, 120, 90, 8, seed=22), "thread b")


def test_resident_buffer_interactive_loop(rpt, tracer, oracle):
    """renderer/src/main.rs:113-124 with the ColorBuffer kept on the device: N x {render; convert_to_u8}.
    The f32 pixels and the u8 frame after 5 redraws equal the oracle's, and a size change starts afresh."""
    w, h = 160, 120
    tracer.resident_reset()
    frame = None
    for _ in range(5):
        tracer.render_resident(w, h)                 # pt.render(&mut buffer)
        frame = tracer.resident_to_u8(w, h)          # buffer.convert_to_u8(frame)
    assert tracer.resident_frames() == 5
    want = oracle.render(oracle.scene_analytical(), w, h, 5, seed=1)
    buf = tracer.resident_to_host(w, h)
    assert buf.frames == 5
    assert_bit_identical(buf.image(), want, "resident f32")
    assert np.array_equal(frame, oracle.convert_to_u8(want, w, h))
    tracer.render_resident(64, 48, 2)                # new size: ColorBuffer::new
    assert tracer.resident_frames() == 2
    assert_bit_identical(tracer.resident_to_host(64, 48).image(), oracle.render(oracle.scene_analytical(), 64, 48, 2, seed=1), "resident resized")
    tracer.resident_reset()


@pytest.mark.parametrize("at", [(10, 7, 200, 150), (0, 0, 96, 64), (150, 100, 200, 150), (3, 60, 64, 70)])
def test_convert_to_u8_at(rpt, torch_cuda, tracer, oracle, at):
    """ColorBuffer::convert_to_u8_at (buffer.rs:67-89): the blit with the reference's strict bounds, row shift
    and missing gamma; untouched frame pixels keep their contents; clipping at the frame edges."""
    torch = torch_cuda
    w, h = 96, 64
    buf = rpt.DeviceColorBuffer(w, h)
    tracer.render_n(buf, 3)
    buf.pixels[5, 5] = torch.tensor([-1.0, 2.0, float("nan"), 0.5], device="cuda")
    frame = torch.full((at[3], at[2], 4), 77, dtype=torch.uint8, device="cuda")
    buf.convert_to_u8_at(frame, at)
    torch.cuda.synchronize()
    want = np.full((at[3], at[2], 4), 77, dtype=np.uint8)
    oracle.convert_to_u8_at(buf.pixels.cpu().numpy(), w, h, want, at)
    assert np.array_equal(frame.cpu().numpy(), want)
    assert (want != 77).any() or at[0] >= at[2]


def test_fast_math_mode_is_statistically_equivalent(rpt, torch_cuda, oracle):
    """RPT_RENDER_FAST_MATH (relaxed divide/sqrt, FMA contraction) is NOT bit-identical: an ulp-level difference
    occasionally flips a branch.  It must agree with the exact kernel within these statistical bounds at 64 spp:
    median |diff| < 2e-6, at most 2 % of the pixels off by more than 1e-3 (flipped samples), equal image mean to
    1e-4 — and the strict kernel must be untouched by the extra build (still equal to the oracle)."""
    torch = torch_cuda
    w, h, spp = 256, 144, 64
    t = rpt.Tracer(rpt.AnalyticalScene(), device=0, seed=1)
    exact = rpt.DeviceColorBuffer(w, h)
    t.render_n(exact, spp)
    t.flags = rpt._abi.RPT_RENDER_FAST_MATH
    fast = rpt.DeviceColorBuffer(w, h)
    t.render_n(fast, spp)
    torch.cuda.synchronize()
    a = exact.pixels.cpu().numpy()[..., :3].astype(np.float64)
    b = fast.pixels.cpu().numpy()[..., :3].astype(np.float64)
    assert not np.isnan(b).any()
    d = np.abs(a - b)
    assert not np.array_equal(a, b)                       # it really is a different arithmetic
    assert np.median(d) < 2e-6
    assert (d.max(axis=2) > 1e-3).mean() < 0.02
    assert abs(a.mean() - b.mean()) < 1e-4
    want = oracle.render(oracle.scene_analytical(), w, h, spp, seed=1)
    assert_bit_identical(exact.pixels.cpu().numpy(), want, "strict kernel next to the fast build")
    t.close()


def test_fast_math_mode_in_the_other_kernels(rpt, torch_cuda):
    """The relaxed-arithmetic build of the kernels added in round 2 — the compacting kernel of one-sample launches and the
    wavefront form of large scenes — runs, and stays within the same statistical distance of the strict kernels."""
    from rust_pathtracer_amd import scenes
    A = rpt._abi
    cases = [("compact", rpt.AnalyticalScene(), A.RPT_RENDER_SMALL_COMPACT, 256, 144, 32),
             ("large scene", scenes.random_spheres_scene(n_spheres=400, n_lights=6), 0, 192, 108, 24)]
    for name, scene, form, w, h, spp in cases:
        t = rpt.Tracer(scene, device=0, seed=2)
        t.flags = form
        exact = rpt.DeviceColorBuffer(w, h)
        t.render_n(exact, spp)
        t.flags = form | A.RPT_RENDER_FAST_MATH
        fast = rpt.DeviceColorBuffer(w, h)
        t.render_n(fast, spp)
        torch_cuda.cuda.synchronize()
        a = exact.pixels.cpu().numpy()[..., :3].astype(np.float64)
        b = fast.pixels.cpu().numpy()[..., :3].astype(np.float64)
        assert not np.isnan(b).any(), name
        d = np.abs(a - b)
        assert np.median(d) < 5e-6, name
        assert (d.max(axis=2) > 1e-2).mean() < 0.05, name
        assert abs(a.mean() - b.mean()) < 2e-3, name
        t.close()
