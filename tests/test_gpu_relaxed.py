"""The relaxed-arithmetic kernels (RPT_RENDER_FAST_MATH: the four render translation units built a second time with hipcc's fast divide /
sqrt and FMA contraction, kernel suffix _fast; build.py RELAXED) against the f64 oracle (liboracle_f64.so), in every instantiation.
Needs an MI355X.

They are not bit-identical to the reference arithmetic, so each frame is held to bounds of the f64 frame of the same scene, seed, spp
and flags (tests/f64_compare.py): finite; median |delta| <= 4 x the strict frame's; flipped pixels <= 2.5 x the strict frame's + 6
pixels; the largest |delta| <= max(2 x the strict frame's, 8) samples; |mean delta| <= 4 standard errors + 1e-6.  "The strict frame"
is the f32 oracle's (which the strict kernels equal bit for bit) against the same f64 frame, computed in the same test run.

Measured on an MI355X (the `RELAXED` lines this module prints, -s), relaxed over strict: flipped pixels x0.25-2.0 (small scenes'
megakernel forms x0.25-2.0, compacting x1.0-1.6, SDF x0.83-1.30, large x0.94; extensions and random scenes x0.89-1.50), median
|delta| x0.73-2.0; the mean delta within 2 standard errors everywhere.  The factors 2.5 (+ 6 pixels) and 4 leave room for the run-to-run
spread of a few-pixel count; DESIGN.md §2 has the table.

Inside the relaxed build there is no tolerance: the same kernel gives the same bits whatever the scheduling (fresh contexts, chunked
dispatch, split launches, virtual ranks).  The list of instantiations is checked against the _fast kernels of the loaded library's
gfx950 code object, so a kernel added without a case fails here."""
import ctypes as C

import numpy as np
import pytest

import conftest
import f64_compare as F
from kernel_census import COMPACT_BIT, NESTED_BIT, RELAXED_BIT, kernel_of
from kernel_census import code_object_kernels as _code_object_kernels

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def oracle_f64():
    conftest._build_oracle()
    import oracle_lib
    return oracle_lib.Oracle("liboracle_f64.so")


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _sdf(rpt, n_prims, spheres=1, lights=1):
    """An SDF object of n_prims primitives over one plane, with `spheres` analytical spheres and `lights` lights."""
    from rust_pathtracer_amd import scenes
    A = rpt._abi
    s = scenes.sdf_scene()
    more = [(A.RPT_SDF_SPHERE, (0.6, 0.5, -0.4), (0.4, 0.0)), (A.RPT_SDF_TORUS_Y, (0.2, 0.3, 0.0), (0.7, 0.12))]
    s.sdf["prims"] = (list(s.sdf["prims"]) + more)[:n_prims]
    s.spheres = (list(s.spheres) + [((-1.8, -0.5, 0.9), 0.5, 0)])[:spheres]
    if lights == 2:
        s.lights = list(s.lights) + [rpt.AnalyticalLight.spherical((2.0, 2.5, -1.0), 0.4, (5.0, 6.0, 7.0))]
    return s


def _table(rpt, which):
    from test_gpu_dispatch import _table_scene
    return _table_scene(rpt, which)[0]


def _large(rpt):
    from rust_pathtracer_amd import scenes
    return scenes.random_spheres_scene(300, 5)


NESTED = 1 << 0
# kernel -> (class, scene(rpt), width, height, launches (samples per render_n call), render flags)
#   small scenes' megakernel: launches of 2+ samples; the compacting kernel: launches of one sample, dense up to 3 072 tiles
#   (160 x 96 = 60 tiles), the other form beyond (1 040 x 768 = 3 120 tiles)
DENSE, SPARSE = (160, 96, (1,) * 8), (1040, 768, (1, 1))
CASES = {
    "render_small_nested_kernel_fast": ("small", lambda r: r.AnalyticalScene(), 128, 80, (3, 3), NESTED),
    "render_small_regen_kernel_fast": ("small", lambda r: _table(r, "eight primitives many classes"), 128, 80, (3, 3), 0),
    "render_small_regen_sized_kernel_fast": ("small", lambda r: _table(r, "two checkers"), 128, 80, (3, 3), 0),
    "render_small_regen_sized_table_kernel_fast": ("small", lambda r: r.AnalyticalScene(), 128, 80, (3, 3), 0),
    "render_small_regen_table_kernel_fast": ("small", lambda r: _table(r, "three spheres on a floor"), 128, 80, (3, 3), 0),
    "render_small_regen_maptable_kernel_fast": ("small", lambda r: _table(r, "six spheres two planes"), 128, 80, (3, 3), 0),
    "render_small_compact_dense_sized_table_kernel_fast": ("small", lambda r: r.AnalyticalScene()) + DENSE + (0,),
    "render_small_compact_sized_table_kernel_fast": ("small", lambda r: r.AnalyticalScene()) + SPARSE + (0,),
    "render_small_compact_dense_sized_kernel_fast": ("small", lambda r: _table(r, "two checkers")) + DENSE + (0,),
    "render_small_compact_sized_kernel_fast": ("small", lambda r: _table(r, "two checkers")) + SPARSE + (0,),
    "render_small_compact_dense_table_kernel_fast": ("small", lambda r: _table(r, "one sphere two planes")) + DENSE + (0,),
    "render_small_compact_table_kernel_fast": ("small", lambda r: _table(r, "one sphere two planes")) + SPARSE + (0,),
    "render_small_compact_dense_kernel_fast": ("small", lambda r: _table(r, "three spheres on a floor")) + DENSE + (0,),
    "render_small_compact_kernel_fast": ("small", lambda r: _table(r, "three spheres on a floor")) + SPARSE + (0,),
    "render_sdf_march2_kernel_fast": ("sdf", lambda r: _sdf(r, 5, spheres=2), 112, 64, (3, 3), 0),
    "render_sdf_march2_table_kernel_fast": ("sdf", lambda r: _sdf(r, 3, lights=2), 112, 64, (3, 3), 0),
    "render_large_regen_kernel_fast": ("large", _large, 112, 64, (3, 3), 0),
}
for _n in (1, 2, 3, 4):
    CASES["render_sdf_march2_sized_kernel_fast<%d>" % _n] = ("sdf", lambda r, n=_n: _sdf(r, n, spheres=2), 112, 64, (3, 3), 0)
    CASES["render_sdf_march2_sized_table_kernel_fast<%d>" % _n] = ("sdf", lambda r, n=_n: _sdf(r, n), 112, 64, (3, 3), 0)


def _render(rpt, torch, scene, w, h, launches, flags, seed=1, dispatch=None):
    """The relaxed frame (RPT_RENDER_FAST_MATH | flags) after render_n(n) for n in launches -> (frame, kernel choice of the last launch)."""
    t = rpt.Tracer(scene, device=0, seed=seed)
    t.flags = rpt._abi.RPT_RENDER_FAST_MATH | flags
    if dispatch is not None:
        t.set_dispatch(*dispatch)
    buf = rpt.DeviceColorBuffer(w, h)
    for n in launches:
        t.render_n(buf, n)
    torch.cuda.synchronize()
    choice = C.c_uint32()
    assert rpt.lib().rpt_debug_kernel_choice(t._h, C.byref(choice)) == 0
    img = buf.pixels.cpu().numpy()
    t.close()
    return img, choice.value


def _report(what, cal, dist):
    fr, mr = cal.ratios(dist)
    print("RELAXED %-52s strict: %r\n        %-52s relaxed: %r  (flip x%.2f, median x%.2f)" % (what, cal.strict, "", dist, fr, mr))


def _check(rpt, oracle, oracle_f64, what, scene, frame, w, h, spp, flags=0, seed=1):
    oflags = flags & rpt._abi.RPT_RENDER_RUSSIAN_ROULETTE
    cal = F.Calibrated(oracle, oracle_f64, scene.describe(), w, h, spp, seed=seed, render_flags=oflags)
    dist = cal.distance(frame)
    _report(what, cal, dist)
    cal.check(frame, what)
    return cal, dist


@pytest.mark.parametrize("kernel", sorted(CASES))
def test_every_relaxed_kernel_against_the_f64_oracle(rpt, oracle, oracle_f64, torch_cuda, kernel):
    klass, make, w, h, launches, flags = CASES[kernel]
    scene = make(rpt)
    frame, choice = _render(rpt, torch_cuda, scene, w, h, launches, flags)
    assert kernel_of(choice, klass) == kernel, "aimed at %s, ran %s (choice %#x)" % (kernel, kernel_of(choice, klass), choice)
    _check(rpt, oracle, oracle_f64, kernel, scene, frame, w, h, sum(launches), flags)


def test_the_case_list_is_the_library_s_relaxed_kernels(rpt):
    """Every render_*_fast kernel of the loaded library's gfx950 code object has a case above, and every case names one of them.
    (The code object's metadata, not the host symbol table: the library is built with -fvisibility=hidden.)"""
    names = set(k for k in _code_object_kernels(rpt._lib.LIB_PATH) if k.startswith("render_") and "_fast" in k)
    assert len(names) == 25 and names == set(CASES), "library: %s; cases: %s" % (sorted(names - set(CASES)), sorted(set(CASES) - names))


# ---- extensions under relaxed arithmetic ------------------------------------------------------------------------------------------
def _random_scenes(rpt, k):
    """k seeds of tests/scene_fuzz.random_small_scene whose scale is within 2^-10 ... 2^10 (beyond, the f32 reference's camera and
    checker quantise and the f64 frame is not the f32 picture: test_scaled_scenes)."""
    from scene_fuzz import random_small_scene
    out, seed = [], 100
    while len(out) < k:
        s, log2_k, flags, _ = random_small_scene(rpt, seed)
        if abs(log2_k) <= 10:
            out.append((seed, s, flags))
        seed += 1
    return out


def test_extensions_under_relaxed_arithmetic(rpt, oracle, oracle_f64, torch_cuda):
    """Russian roulette, rectangular and distant lights (RPT_SCENE_SAMPLE_ALL_LIGHT_TYPES) in a small and in a large scene, and random
    small scenes (materials, depths, roulette, 1-8 spheres, 1-4 lights): each against the f64 frame rendered with the same flags.
    (RPT_RENDER_NESTED_LOOPS: its kernel's case above.)"""
    from test_gpu_extensions import _light_zoo
    A = rpt._abi
    w, h = 112, 64
    deep = rpt.AnalyticalScene()
    deep.max_depth = 8
    large_lights = _large(rpt)
    large_lights.sample_all_light_types = True
    large_lights.lights[1] = rpt.AnalyticalLight.rectangular((-10.0, 14.0, -40.0), (20.0, 0.0, 0.0), (0.0, 0.0, 20.0), (8.0, 8.0, 8.0))
    large_lights.lights[2] = rpt.AnalyticalLight.distant((0.3, 1.0, 0.4), (1.0, 0.9, 0.8))
    cases = [("roulette, depth 8", deep, A.RPT_RENDER_RUSSIAN_ROULETTE), ("roulette, sdf", _sdf(rpt, 3), A.RPT_RENDER_RUSSIAN_ROULETTE),
             ("roulette, large", _large(rpt), A.RPT_RENDER_RUSSIAN_ROULETTE), ("all light types", _light_zoo(rpt, True), 0),
             ("all light types, large", large_lights, 0)]
    cases += [("random small scene %d" % seed, s, flags) for seed, s, flags in _random_scenes(rpt, 5)]
    for name, scene, flags in cases:
        frame, choice = _render(rpt, torch_cuda, scene, w, h, (4, 4), flags, seed=2)
        assert choice & RELAXED_BIT, name
        _check(rpt, oracle, oracle_f64, name, scene, frame, w, h, 8, flags, seed=2)


@pytest.mark.parametrize("log2_k", [-31, -20, 30, 31])
def test_scaled_scenes(rpt, oracle, oracle_f64, torch_cuda, log2_k):
    """The stock scene scaled by 2^k (tests/test_gpu_range_guards.py): the strict kernels take their range guards there, the relaxed
    ones have none.  Finite everywhere.  At 2^-31 and 2^-20 the f32 frames are the unscaled scene's and are held to the f64 frame of the
    scaled scene.  From 2^23 up the reference's own f32 camera quantises its rays (origin + lower-left corner + ... - origin at
    |origin| ~ 2^24): the f32 oracle's frame is no longer the f64 picture (every pixel off), so there the relaxed frame is held to the f32
    oracle's frame of the scaled scene — the strict kernels' — with the bounds the unscaled scene's strict frame gives against f64."""
    from test_gpu_range_guards import scaled_stock_scene
    w, h, spp = 112, 64, 8
    s = scaled_stock_scene(rpt, 2.0 ** log2_k)
    frame, _ = _render(rpt, torch_cuda, s, w, h, (4, 4), 0)
    assert np.isfinite(frame).all(), "stock scene x 2^%d: %d non-finite values" % (log2_k, (~np.isfinite(frame)).sum())
    if log2_k < 23:
        _check(rpt, oracle, oracle_f64, "stock scene x 2^%d" % log2_k, s, frame, w, h, spp)
    else:
        unscaled = F.Calibrated(oracle, oracle_f64, rpt.AnalyticalScene().describe(), w, h, spp)
        want = oracle.render(s.describe(), w, h, spp, seed=1)
        dist = F.Distance(frame, want, spp)
        _report("stock scene x 2^%d (against the f32 frame)" % log2_k, unscaled, dist)
        F.compare(frame, want, spp, unscaled.bounds, "stock scene x 2^%d against the f32 oracle's frame" % log2_k)


# ---- bitwise invariances inside the relaxed build ----------------------------------------------------------------------------------
MANY_CHUNKS = (1, 100000, 1, 8)                                       # (tests/test_gpu_dispatch.py: every sample its own chunk)


@pytest.mark.parametrize("klass", ["small", "sdf", "large"])
def test_relaxed_frames_do_not_depend_on_scheduling(rpt, torch_cuda, klass):
    """No tolerance: the same frame from a fresh context, under one-sample chunks, as render_n(3) + render_n(5) (both the megakernel),
    and from 2 and 3 virtual ranks (render_tile + untile)."""
    from rust_pathtracer_amd import tiling
    from test_gpu_parity import assert_bit_identical
    torch = torch_cuda
    scene = {"small": lambda: rpt.AnalyticalScene(), "sdf": lambda: _sdf(rpt, 3), "large": lambda: _large(rpt)}[klass]()
    w, h = 120, 72
    ref, choice = _render(rpt, torch, scene, w, h, (8,), 0)
    assert choice & RELAXED_BIT and not choice & (COMPACT_BIT | NESTED_BIT)
    assert_bit_identical(_render(rpt, torch, scene, w, h, (8,), 0)[0], ref, "%s: a second fresh context" % klass)
    assert_bit_identical(_render(rpt, torch, scene, w, h, (8,), 0, dispatch=MANY_CHUNKS)[0], ref, "%s: one-sample chunks" % klass)
    assert_bit_identical(_render(rpt, torch, scene, w, h, (3, 5), 0)[0], ref, "%s: 3 + 5 samples" % klass)
    for world, tile_rows in ((2, 2), (3, 4)):
        t = rpt.Tracer(scene, device=0, seed=1)
        t.flags = rpt._abi.RPT_RENDER_FAST_MATH
        gathered = torch.zeros(world, tiling.padded_rows(h, tile_rows, world), w, 4, dtype=torch.float32, device="cuda")
        for r in range(world):
            t.render_tile(gathered[r], w, h, 0, 8, tile_rows, r, world)
        img = tiling.untile(gathered, w, h, tile_rows, world, t)
        torch.cuda.synchronize()
        assert_bit_identical(img.cpu().numpy(), ref, "%s: %d virtual ranks" % (klass, world))
        t.close()


# ---- the relaxed build's device math against float64 ----------------------------------------------------------------------------
def _ulps(got, ref64):
    """|got - ref| in ulps of the float32 result (the ulp of a denormal result is 2^-149)."""
    ref32 = ref64.astype(np.float32)
    return np.abs(got.astype(np.float64) - ref64) / np.spacing(np.abs(ref32)).astype(np.float64)


def _wide(rng, n, lo=-60, hi=60):
    """Floats of both signs with exponents uniform in [lo, hi): random significands."""
    e = rng.integers(lo, hi, size=n)
    return (rng.choice([-1.0, 1.0], size=n) * np.ldexp(rng.uniform(1.0, 2.0, size=n), e)).astype(np.float32)


def test_relaxed_device_math_against_float64(rpt, torch_cuda):
    """The relaxed build's arithmetic (k_probes.hip built with build.py's RELAXED flags; rpt_probe_math with RPT_PROBE_RELAXED) against
    NumPy float64, no oracle in the loop.  Claims (include/rpt.h, RPT_RENDER_FAST_MATH; kernel_common.h): the divide and the square
    root within 2.5 ulp over operands in [2^-60, 2^60) and over the whole range (hipcc's sequences scale by the exponent: denormal
    operands and results, huge denominators included); IEEE's answers at zeros, infinities and NaNs; include/rpt_strict_math.h's bounds
    under FMA contraction (sin / cos 1.5 ulp on [0, 2 pi], log2 / pow / exp / log 0.5001 ulp).  Prints the largest error of each."""
    from test_gpu_parity import _probe
    A = rpt._abi
    t = rpt.Tracer(rpt.AnalyticalScene(), device=0, seed=1)
    R = A.RPT_PROBE_RELAXED
    probe = lambda fn, a, b=None: _probe(rpt, torch_cuda, t, fn | R, a, b)      # noqa: E731
    rng = np.random.default_rng(91)
    n = 1_000_000
    worst = {}

    def bound(name, err, limit):
        worst[name] = float(np.max(err))
        assert worst[name] <= limit, "%s: %.3f ulp > %g" % (name, worst[name], limit)

    # divide: operands in the short sequences' range, then across every exponent (denormals included)
    a, b = _wide(rng, n), _wide(rng, n)
    bound("div [2^-60, 2^60)", _ulps(probe(A.RPT_PROBE_DIV, a, b), a.astype(np.float64) / b.astype(np.float64)), 2.5)
    bits = lambda k: rng.integers(0, 0x7F800000, size=k, dtype=np.uint32).view(np.float32) * rng.choice(np.float32([-1, 1]), size=k)   # noqa: E731
    a, b = bits(n), bits(n)
    q64 = a.astype(np.float64) / b.astype(np.float64)
    got = probe(A.RPT_PROBE_DIV, a, b)
    fin = np.abs(q64) < float(np.finfo(np.float32).max)
    bound("div, all finite operands", _ulps(got[fin], q64[fin]), 2.5)
    assert np.all(np.isinf(got[np.abs(q64) > 2.0 ** 128])), "div: an overflowing quotient is an infinity"
    # three quotients by one denominator (divs3: the probe's numerators are a, -b or b / 2, 3a / 4)
    a, b = _wide(rng, n), _wide(rng, n)
    i = np.arange(n)
    num = np.where(i % 3 == 0, a, np.where(i & 4, 0.5 * b, -b.astype(np.float64)))
    num = np.where(i % 3 == 2, np.where(i & 4, 0.0, 0.75 * a.astype(np.float64)), num).astype(np.float32).astype(np.float64)
    bound("div3", _ulps(probe(A.RPT_PROBE_DIV3, a, b), num / b.astype(np.float64)), 2.5)
    # zeros, infinities, NaNs, denormals, the largest and smallest normals: what IEEE division answers
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-40, 1.17549435e-38, 3.4028235e38, 1.0, -3.0, 2.0 ** -60, 2.0 ** 60],
                  dtype=np.float32)
    ga, gb = (g.ravel() for g in np.meshgrid(sp, sp))
    with np.errstate(all="ignore"):
        want = (ga.astype(np.float64) / gb.astype(np.float64))
    got = probe(A.RPT_PROBE_DIV, ga, gb)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "div: NaN where IEEE has none, or the reverse"
    special = ~np.isfinite(want) | (want == 0)
    assert np.array_equal(got[special & ~np.isnan(want)], want[special & ~np.isnan(want)].astype(np.float32)), "div: zeros / infinities"
    fin = np.isfinite(want) & (np.abs(want) < 3.4e38) & (want != 0)
    bound("div, special operands", _ulps(got[fin], want[fin]), 2.5)

    # square root: [2^-60, 2^60), every non-negative finite float, specials
    x = np.abs(_wide(rng, n))
    bound("sqrt [2^-60, 2^60)", _ulps(probe(A.RPT_PROBE_SQRT, x), np.sqrt(x.astype(np.float64))), 2.5)
    x = rng.integers(0, 0x7F800000, size=n, dtype=np.uint32).view(np.float32)
    bound("sqrt, all finite", _ulps(probe(A.RPT_PROBE_SQRT, x), np.sqrt(x.astype(np.float64))), 2.5)
    x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, 1e-45, 1e-40], dtype=np.float32)
    got = probe(A.RPT_PROBE_SQRT, x)
    with np.errstate(all="ignore"):
        want = np.sqrt(x.astype(np.float64)).astype(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[:3].view(np.uint32), want[:3].view(np.uint32)), (got, want)

    # include/rpt_strict_math.h under -ffp-contract=fast
    x = rng.uniform(0, 2 * np.pi, n).astype(np.float32)
    for fn, f in ((A.RPT_PROBE_SIN, np.sin), (A.RPT_PROBE_COS, np.cos)):
        got, ref = probe(fn, x), f(x.astype(np.float64))
        big = np.abs(ref) > 1e-3
        bound(f.__name__, _ulps(got, ref)[big], 1.5)
        assert np.abs(got - ref).max() < 1.2e-7, f.__name__
    x = rng.integers(0x00800000, 0x7f7fffff, size=n, dtype=np.uint32).view(np.float32)
    bound("log2", _ulps(probe(A.RPT_PROBE_LOG2, x), np.log2(x.astype(np.float64))), 0.5001)
    bound("log", _ulps(probe(A.RPT_PROBE_LOG, x), np.log(x.astype(np.float64))), 0.5001)
    a = rng.uniform(1e-4, 4.0, n).astype(np.float32)
    for b in (np.full(n, 2.2, dtype=np.float32), np.full(n, 0.4545, dtype=np.float32), rng.uniform(0, 3, n).astype(np.float32)):
        bound("pow y=%s" % ("%.4g" % b[0] if b[0] == b[-1] else "U(0,3)"),
              _ulps(probe(A.RPT_PROBE_POW, a, b), np.power(a.astype(np.float64), b.astype(np.float64))), 0.5001)
    x = rng.uniform(-80, 80, n).astype(np.float32)
    bound("exp", _ulps(probe(A.RPT_PROBE_EXP, x), np.exp(x.astype(np.float64))), 0.5001)
    t.close()
    print("RELAXED device math, largest error in ulps: " + ", ".join("%s %.3f" % kv for kv in worst.items()))
