"""Every render kernel at the ends of the launch domain (needs an MI355X): a 64-bit frames_done at and beyond 2^24, 2^32, 2^53 and just
below 2^64, a seed with a high word, and frames one pixel wide or high.  tests/test_launch_domain.py (CPU) holds the oracle's key
and weight to independent restatements there and counts the float64 restatement's near ties; this file holds the device to the
oracle, bit for bit, and to the float64 restatement.

STARTS = 2^24 - 2 (the weight's u64 -> f32 conversion starts to round inside the launch: 2^24 + 1 is a tie), 2^32 - 2 (the key's
high word becomes non-zero inside the launch, and every host-side sum frames_done + k carries), 2^53 - 1 (beyond a double's
integers) and 2^64 - 8 (the last words of the counter).  The seed is 0xDEADBEEF12345 throughout (a).

(a) test_every_strict_kernel_at_a_start: each of test_gpu_strict_kernels.CASES' 29 kernels with its scene, flags and launch list,
    buf.frames set to the start before the first launch, once into a zeroed buffer (the key and the weight) and once into a
    buffer of finite random values in [0.1, 1) (the rounding of 1 - v from 2^24 on), confirmed through rpt_debug_kernel_choice and
    compared with oracle.render(..., frames_done=start).  A kernel takes the start STARTS[i % 4], i its index in sorted(CASES);
    ALL_STARTS — one kernel per class: small, sdf, large, one media form — take all four.  Frame sizes (SIZES): 34 x 19 (3 x 2
    tiles, ragged both ways) for every kernel but the sparse compacting forms, whose choice needs more than 3 072 tiles (capi.hip,
    kCompactDenseMaxBlocks): 97 x 7 009 is 7 x 439 = 3 073 tiles, the fewest that select them, each asserted by _assert_ran; their
    first row, last row and every 97th row are compared through oracle.render_rows.  No other kernel choice reads the frame size.
    The teeth: the same launches with every launch's frames_done reduced mod 2^32 (what a counter truncated on the host would
    pass) give another frame whenever a sample's frame has a high word; where none has (2^24 - 2, and the launch lists that do
    not reach 2^32 from 2^32 - 2) the two are the same launches and nothing is asserted.
(b) the carries, all from 2^32 - 2 on the analytical scene at 50 x 37: one launch of 6 samples under the chunked dispatches
    (1, 1000, 1, 0) and (1, 1000, 3, 0) (unit_begin's frames_done + chunk * chunk_spp), render_n of kMaxSppPerLaunch + 3 samples on
    the nested kernel (launch_render's frames_done + done), rpt_resident_upload(frames = start) and rpt_resident_render of 4
    (rpt_resident_frames is then 2^32 + 2), against the oracle's frame; render_tile over 3 virtual ranks against the undivided
    launch.  And the contract (include/rpt.h, "the launch domain"): frames_done + spp > 2^64 - 1 returns RPT_ERR_INVALID_ARG from
    rpt_render, rpt_render_device, rpt_resident_render (against the resident counter), rpt_radiance and rpt_radiance_device, and a
    sentinel buffer stays untouched; the last launch that fits is accepted.
(c) meshes and radiance: the flat form (11) and case B with both maps of test_mesh_frames_f64, 64 x 48, its draws; from
    2^24 - 1, 2^32 - 1 and 2^64 - 4 render_n(buf, 2) into a zeroed buffer against launch_f64 through Tally (TAU / REL_CLEAN /
    NEAR_TIE_MAX), both scaled by frames_done + 2; tally.near is test_launch_domain.DEEP_COUNTS'.  No spreads: the weights are held
    exactly instead — every pixel's alpha, and every word of a flat-scene pixel both of whose samples miss (the background is
    black), equal the blend in numpy float32 with the integer-rounded weights, and the launch equals radiance over the camera's
    sample rays of its two frames, word for word.  One radiance call of kMaxSppPerLaunch + 3 samples from 2^32 - 5 equals its
    one-sample calls.  camera_sample_rays at frame 2^32 + 5 equals the GEN_RAY probe fed the oracle's first two draws.
(d) thin frames, from frames_done = 0, against the oracle: 1 x 1, 1 x 40, 40 x 1, 3 x 2, 16 x 16, 15 x 17, 1 x 1025, 1025 x 1 on the
    small megakernel (3 samples), the dense compacting kernel (three launches of 1), nested, one SDF form, large and the small
    media form, each under the plain dispatch and under (1, 1000, 1, 0); three progressive render_n calls with cost ordering on at
    1 x 1 and 1 x 40, whose order (rpt_debug_sched_read) is a permutation; and for the flat mesh form and form 27 render equals
    radiance over the camera's sample rays and the frame is finite.

Left out: the relaxed build; the SDF and large classes beyond one case each in (b)'s sense (they run in (a) and (d)); frame
counters above 2^64 - 1 in the Python layer (ctypes reduces them mod 2^64 before the library sees them)."""
import ctypes as C

import numpy as np
import pytest

import query_np as Q
import test_launch_domain as LD
import test_mesh_frames_f64 as TF
from test_gpu_mesh_frames_f64 import assert_form, case_tracer, open_tracer
from test_gpu_path_f64 import Tally
from test_gpu_strict_kernels import CASES, _assert_ran, _choice, _reference
from test_path_f64 import NEAR_TIE_MAX, TAU

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF
SEED = LD.BIG_SEED
STARTS = (2 ** 24 - 2, 2 ** 32 - 2, 2 ** 53 - 1, 2 ** 64 - 8)
KERNELS = sorted(CASES)
ALL_STARTS = ("render_small_regen_sized_table_kernel", "render_sdf_march2_kernel", "render_large_regen_kernel", "render_small_regen_media_kernel")
SMALL_SIZE, SPARSE_SIZE = (34, 19), (97, 7009)
SPARSE = ("render_small_compact_kernel", "render_small_compact_sized_kernel", "render_small_compact_sized_table_kernel", "render_small_compact_table_kernel")
# kernel -> the frame size of its case in (a): the smallest that selects the kernel
SIZES = {k: SPARSE_SIZE if k in SPARSE else SMALL_SIZE for k in KERNELS}
MAX_SPP = 512                                                       # kMaxSppPerLaunch (csrc/kernel_common.h)
CARRY_START, CARRY_SIZE = 2 ** 32 - 2, (50, 37)
CHUNKED = (1, 1000, 1, 0)
THIN = ((1, 1), (1, 40), (40, 1), (3, 2), (16, 16), (15, 17), (1, 1025), (1025, 1))
THIN_IDS = ["%dx%d" % s for s in THIN]
# what (d) renders: name -> (the kernel it must run, launches); scene, class and flags are the kernel's in CASES
THIN_KERNELS = {"megakernel": ("render_small_regen_sized_table_kernel", (3,)), "dense compacting": ("render_small_compact_dense_sized_table_kernel", (1, 1, 1)),
                "nested": ("render_small_nested_kernel", (3,)), "sdf": ("render_sdf_march2_kernel", (3,)), "large": ("render_large_regen_kernel", (3,)),
                "small media": ("render_small_regen_media_kernel", (3,))}


def start_of(kernel):
    return STARTS[KERNELS.index(kernel) % len(STARTS)]


A_CASES = [(k, start_of(k)) for k in KERNELS] + [(k, s) for k in ALL_STARTS for s in STARTS if s != start_of(k)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _words(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _launches(rpt, torch, t, w, h, launches, start, fill=None, truncated=False):
    """render_n(n) for n in launches into a buffer that starts from `fill` (zeros without) with .frames = start -> (frame, the
    buffer's .frames).  truncated: every launch receives its frames_done mod 2^32."""
    buf = rpt.DeviceColorBuffer(w, h)
    if fill is not None:
        buf.pixels.copy_(torch.from_numpy(fill))
    buf.frames = start
    for n in launches:
        if truncated:
            buf.frames &= M32
        t.render_n(buf, n)
    torch.cuda.synchronize()
    return buf.pixels.cpu().numpy(), buf.frames


def _oracle_flags(rpt, flags):
    return flags & rpt._abi.RPT_RENDER_RUSSIAN_ROULETTE


def assert_same_words(got, want, what):
    from test_gpu_parity import assert_bit_identical
    assert_bit_identical(got, want, what)


# ---- (a) every strict kernel, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,start", A_CASES, ids=["%s-%#x" % c for c in A_CASES])
def test_every_strict_kernel_at_a_start(rpt, oracle, torch_cuda, kernel, start):
    klass, make, _, _, launches, flags = CASES[kernel]
    w, h = SIZES[kernel]
    spp = sum(launches)
    assert start + spp <= 2 ** 64 - 1 and (w % 16 and h % 16)
    scene = make(rpt)
    desc = scene.describe()
    rows = sorted({0, h - 1} | set(range(0, h, 97))) if kernel in SPARSE else None
    fill = np.random.default_rng([21, KERNELS.index(kernel)]).uniform(0.1, 1.0, (h, w, 4)).astype(np.float32)
    assert np.isfinite(fill).all() and fill.min() >= np.float32(0.1) and fill.max() < 1.0
    t = rpt.Tracer(scene, device=0, seed=SEED)
    t.flags = flags
    try:
        for name, before in (("zeroed", None), ("filled", fill)):
            got, frames = _launches(rpt, torch_cuda, t, w, h, launches, start, fill=before)
            _assert_ran(_choice(rpt, t), klass, kernel)
            assert frames == start + spp
            what = "%s from %#x, %s buffer" % (kernel, start, name)
            pixels = None if before is None else before.copy()
            if rows is None:
                want = oracle.render(desc, w, h, spp, seed=SEED, frames_done=start, pixels=pixels, render_flags=_oracle_flags(rpt, flags))
                assert_same_words(got, want, what)
            else:
                want = oracle.render_rows(desc, w, h, spp, rows, seed=SEED, frames_done=start, pixels=pixels, render_flags=_oracle_flags(rpt, flags))
                assert_same_words(got[rows], want[rows], what + ", rows %s ..." % rows[:3])
            assert np.isfinite(got).all() and _words(got[..., :3]).any()
            if before is None:
                zeroed = got
        # the teeth: a counter truncated to 32 bits between the launches renders another frame, wherever a frame has a high word
        if any((start + k) >> 32 for k in range(spp)):
            other, _ = _launches(rpt, torch_cuda, t, w, h, launches, start, truncated=True)
            assert (_words(other) != _words(zeroed)).any(axis=2).mean() > 0.1, "%s: the frame from %#x is the frame from its low word" % (kernel, start)
    finally:
        t.close()


def test_the_case_list_of_a_is_whole():
    assert len(KERNELS) == 29 and len(A_CASES) == 29 + 4 * 3 and set(SPARSE) <= set(KERNELS)
    assert all((SIZES[k][0] + 15) // 16 * ((SIZES[k][1] + 15) // 16) == (3073 if k in SPARSE else 6) for k in KERNELS)


# ---- (b) the carries -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def carry_want(oracle):
    """spp -> the oracle's analytical frame of spp samples from CARRY_START into a zeroed 50 x 37 buffer; nobody writes to them."""
    made = {}

    def want(spp, flags=0):
        if (spp, flags) not in made:
            made[(spp, flags)] = oracle.render(oracle.scene_analytical(), CARRY_SIZE[0], CARRY_SIZE[1], spp, seed=SEED, frames_done=CARRY_START, render_flags=flags)
            made[(spp, flags)].setflags(write=False)
        return made[(spp, flags)]
    return want


@pytest.mark.parametrize("dispatch", [CHUNKED, (1, 1000, 3, 0)], ids=["chunks-of-1", "chunks-of-3"])
def test_a_chunked_launch_carries_into_the_high_word(rpt, torch_cuda, carry_want, dispatch):
    w, h = CARRY_SIZE
    t = rpt.Tracer(_reference(rpt), device=0, seed=SEED)
    try:
        t.set_dispatch(*dispatch)
        got, frames = _launches(rpt, torch_cuda, t, w, h, (6,), CARRY_START)
        _assert_ran(_choice(rpt, t), "small", "render_small_regen_sized_table_kernel")
    finally:
        t.close()
    assert frames == 2 ** 32 + 4
    assert_same_words(got, carry_want(6), "6 samples from 2^32 - 2 under %s" % (dispatch,))


def test_a_split_nested_render_carries_into_the_high_word(rpt, torch_cuda, carry_want):
    w, h = CARRY_SIZE
    t = rpt.Tracer(_reference(rpt), device=0, seed=SEED)
    t.flags = rpt._abi.RPT_RENDER_NESTED_LOOPS
    try:
        got, _ = _launches(rpt, torch_cuda, t, w, h, (MAX_SPP + 3,), CARRY_START)
        _assert_ran(_choice(rpt, t), "small", "render_small_nested_kernel")
    finally:
        t.close()
    assert_same_words(got, carry_want(MAX_SPP + 3), "%d samples from 2^32 - 2, nested" % (MAX_SPP + 3))


def test_the_resident_counter_carries_into_the_high_word(rpt, torch_cuda, carry_want):
    w, h = CARRY_SIZE
    t = rpt.Tracer(_reference(rpt), device=0, seed=SEED)
    try:
        start = rpt.ColorBuffer(w, h)
        start.frames = CARRY_START
        t.resident_upload(start)
        assert t.resident_frames() == CARRY_START
        t.render_resident(w, h, 4)
        assert t.resident_frames() == 2 ** 32 + 2
        got = t.resident_to_host(w, h)
        assert got.frames == 2 ** 32 + 2
    finally:
        t.close()
    assert_same_words(got.image(), carry_want(4), "resident, 4 samples from 2^32 - 2")


def test_rank_tiles_from_the_high_word_are_the_undivided_launch(rpt, torch_cuda, carry_want):
    from rust_pathtracer_amd import tiling
    torch = torch_cuda
    (w, h), world, tile_rows, spp = CARRY_SIZE, 3, 4, 6
    t = rpt.Tracer(_reference(rpt), device=0, seed=SEED)
    try:
        whole, _ = _launches(rpt, torch, t, w, h, (spp,), CARRY_START)
        gathered = torch.zeros(world, tiling.padded_rows(h, tile_rows, world), w, 4, dtype=torch.float32, device="cuda")
        for r in range(world):
            t.render_tile(gathered[r], w, h, CARRY_START, spp, tile_rows, r, world)
        img = tiling.untile(gathered, w, h, tile_rows, world, t)
        torch.cuda.synchronize()
        got = img.cpu().numpy()
    finally:
        t.close()
    assert np.array_equal(_words(got), _words(whole)), "3 virtual ranks from 2^32 - 2"
    assert_same_words(whole, carry_want(spp), "the undivided launch")


PATTERN = 0x5A5A5A5A
TOP = 2 ** 64 - 1


def test_a_launch_beyond_the_last_frame_is_rejected_and_writes_nothing(rpt, torch_cuda):
    """frames_done + spp <= 2^64 - 1 (include/rpt.h): one sample more and frames + 1 would wrap to 0, the weight be infinite and the
    pixel NaN for good.  Every entry point returns RPT_ERR_INVALID_ARG and leaves its buffer alone; the last launch that fits runs."""
    torch = torch_cuda
    A, lib = rpt._abi, rpt.lib()
    bad = A.RPT_ERR_INVALID_ARG
    w, h = 8, 4
    t = rpt.Tracer(_reference(rpt), device=0, seed=SEED)
    try:
        dev = torch.full((h, w, 4), PATTERN, dtype=torch.int32, device="cuda")
        host = np.full(w * h * 4, PATTERN, np.uint32)
        for frames_done, spp in ((TOP, 1), (TOP - 2, 3), (2 ** 64 - 2 ** 31, 2 ** 31 + 1), (TOP - 5, 2 ** 32 - 1)):
            assert lib.rpt_render_device(t._h, dev.data_ptr(), w, h, frames_done, spp, SEED, 0, h, 0, 1, None) == bad, (frames_done, spp)
            assert b"2^64 - 1" in lib.rpt_last_error(t._h)
            assert lib.rpt_render(t._h, host.ctypes.data, w, h, frames_done, spp, SEED, 0) == bad, (frames_done, spp)
            assert b"2^64 - 1" in lib.rpt_last_error(t._h)
        torch.cuda.synchronize()
        assert bool((dev == PATTERN).all()) and (host == PATTERN).all()
        assert lib.rpt_render_device(t._h, dev.data_ptr(), w, h, TOP, 0, SEED, 0, h, 0, 1, None) == A.RPT_OK, "no sample: nothing to reject"
        torch.cuda.synchronize()
        assert bool((dev == PATTERN).all())
        # the resident path, against the resident counter
        start = rpt.ColorBuffer(w, h)
        start.pixels[:] = 0.25
        start.frames = TOP - 3
        t.resident_upload(start)
        assert lib.rpt_resident_render(t._h, w, h, 4, SEED, 0) == bad and b"2^64 - 1" in lib.rpt_last_error(t._h)
        assert t.resident_frames() == TOP - 3 and (t.resident_to_host(w, h).pixels == np.float32(0.25)).all()
        # the last launch that fits: frames 2^64 - 4 .. 2^64 - 2, every weight 2^-64 (too small to move 0.25: from a zeroed buffer)
        start.pixels[:] = 0.0
        t.resident_upload(start)
        assert lib.rpt_resident_render(t._h, w, h, 3, SEED, 0) == A.RPT_OK
        last = t.resident_to_host(w, h)
        assert last.frames == TOP and np.isfinite(last.pixels).all()
        assert (_words(last.image()[..., 3]) == _words(_alpha_after(TOP - 3, 3))).all(), "the three samples were blended"
        assert lib.rpt_resident_render(t._h, w, h, 1, SEED, 0) == bad and t.resident_frames() == TOP
        # a buffer of another size starts again from frame 0: the full counter does not stand in its way
        assert lib.rpt_resident_render(t._h, w + 1, h, 1, SEED, 0) == A.RPT_OK and t.resident_frames() == 1
    finally:
        t.close()
    m = rpt.Tracer(Q.small_scene(), device=0, seed=SEED)
    try:
        rays = m.camera_sample_rays(w, h, 0)
        out = torch.full((w * h, 4), PATTERN, dtype=torch.int32, device="cuda")
        r8 = rays.cpu().numpy()
        o = np.full((w * h, 4), PATTERN, np.uint32)
        for frames_done, spp in ((TOP, 1), (TOP - 2, 3), (TOP - MAX_SPP, MAX_SPP + 1)):
            assert lib.rpt_radiance_device(m._h, rays.data_ptr(), w * h, out.data_ptr(), frames_done, spp, SEED, 0, 0, None) == bad, (frames_done, spp)
            assert b"2^64 - 1" in lib.rpt_last_error(m._h)
            assert lib.rpt_radiance(m._h, r8.ctypes.data, w * h, o.ctypes.data, frames_done, spp, SEED, 0, 0) == bad, (frames_done, spp)
        torch.cuda.synchronize()
        assert bool((out == PATTERN).all()) and (o == PATTERN).all()
        fits = m.radiance(rays, spp=3, frames_done=TOP - 3)
        torch.cuda.synchronize()
        assert np.isfinite(fits.cpu().numpy()).all()
    finally:
        m.close()


# ---- (c) meshes and radiance ---------------------------------------------------------------------------------------------------------------
def _alpha_after(start, n):
    """Alpha of a zeroed pixel after frames start .. start + n - 1, in numpy float32 with the integer-rounded weights."""
    return LD.blend([np.zeros((1, 3), np.float32)] * n, start, np.zeros((1, 4), np.float32))[0, 3]


@pytest.mark.parametrize("start", LD.DEEP_STARTS, ids=["%#x" % s for s in LD.DEEP_STARTS])
@pytest.mark.parametrize("case", LD.DEEP_CASES)
def test_a_two_sample_mesh_launch_at_depth(rpt, oracle, torch_cuda, case, start):
    torch = torch_cuda
    size = (w, h) = TF.SIZES[0]
    pixels = TF.draws(case)[size]
    t, form = case_tracer(rpt, case)
    try:
        buf = rpt.DeviceColorBuffer(w, h)
        buf.frames = start
        t.render_n(buf, 2)
        torch.cuda.synchronize()
        assert_form(rpt, t, form)
        assert buf.frames == start + 2
        frame = buf.pixels.cpu().numpy()
        # the same launch as radiance over the camera's sample rays of its two frames
        out = torch.zeros((w * h, 4), dtype=torch.float32, device="cuda")
        missed = np.ones(w * h, bool)
        for f in (start, start + 1):
            rays = t.camera_sample_rays(w, h, f)
            t.radiance(rays, frames_done=f, out=out)
            missed &= (t.trace(rays)["kind"] == Q.HIT_NONE).cpu().numpy()
        torch.cuda.synchronize()
        differ = (_words(out.cpu().numpy()) != _words(frame).reshape(w * h, 4)).any(axis=1)
        assert not differ.any(), "case %s from %#x: %d pixels differ from radiance over the sample rays" % (case, start, int(differ.sum()))
    finally:
        t.close()
    scale = float(start + 2)
    mean, margins, _ = TF.launch_f64(oracle, case, size, start, 2)
    tally = Tally(TAU, NEAR_TIE_MAX)
    tally.ran.add("form %d" % form)
    what = "case %s, %d x %d, two samples on %#x earlier" % (case, w, h, start)
    tally.add("%s (form %d)" % (what, form), frame.astype(np.float64) * scale, mean[:, :3] * scale, margins, pixels)
    tally.check(what)
    assert tally.n == TF.N and tally.near == LD.DEEP_COUNTS[case][0][LD.DEEP_STARTS.index(start)]
    # the weights, exactly
    alpha = _alpha_after(start, 2)
    assert (_words(frame[..., 3]) == _words(alpha)).all(), "alpha is ((1 - v0) * 0 + v0) * (1 - v1) + v1 with the integer-rounded weights"
    if case == TF.FLAT:
        assert missed.sum() > 100, "the flat scene has sky"
        black = np.array([0.0, 0.0, 0.0, alpha], np.float32)
        assert (_words(frame).reshape(w * h, 4)[missed] == _words(black)).all(), "a pixel both of whose samples miss is the black background blended"


def test_one_radiance_call_across_the_high_word_is_its_one_sample_calls(rpt, torch_cuda):
    torch = torch_cuda
    start, n = 2 ** 32 - 5, MAX_SPP + 3
    t = open_tracer(rpt, "single", TF.FLAT + " composed", SEED)
    try:
        few = t.camera_sample_rays(64, 48, start)[1600:1664].contiguous()                # the object and the floor
        one = t.radiance(few, spp=n, frames_done=start)
        two = torch.zeros_like(one)
        for k in range(n):
            t.radiance(few, spp=1, frames_done=start + k, out=two)
        torch.cuda.synchronize()
        got, want = one.cpu().numpy(), two.cpu().numpy()
    finally:
        t.close()
    assert np.isfinite(want).all() and want[:, :3].max() > 0.0
    assert np.array_equal(_words(got), _words(want)), "%d samples from 2^32 - 5" % n


def test_camera_sample_rays_beyond_the_low_word(rpt, oracle, torch_cuda):
    from test_gpu_radiance import _gen_ray_probe
    F = np.float32
    w, h = 50, 37
    frame = 2 ** 32 + 5
    s = Q.small_scene()
    s.camera = rpt.Pinhole((2.0, 1.0, -3.0), (0.5, 0.0, 1.0), 35.0)
    t = rpt.Tracer(s, device=0, seed=SEED)
    try:
        got = t.camera_sample_rays(w, h, frame)
        low = t.camera_sample_rays(w, h, frame & M32)
        torch_cuda.cuda.synchronize()
        got, low = got.cpu().numpy(), low.cpu().numpy()
        y, x = np.divmod(np.arange(w * h), w)
        j = (h - 1 - y).astype(F)
        px = x.astype(F) / F(w)
        py = F(1.0) - (F(h) - j) / F(h)
        draws = np.stack([oracle.rng_f32(SEED, frame, int(p), 2) for p in range(w * h)])
        want = _gen_ray_probe(rpt, torch_cuda, t, px, py, draws[:, 0], draws[:, 1], w, h)
    finally:
        t.close()
    assert np.array_equal(_words(got[:, 0:3]), _words(want[:, 0:3])), "origins"
    assert np.array_equal(_words(got[:, 4:7]), _words(want[:, 3:6])), "directions"
    assert (_words(low[:, 4:7]) != _words(got[:, 4:7])).any(axis=1).mean() > 0.9, "frame 5 sends other rays"


# ---- (d) thin frames -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", THIN, ids=THIN_IDS)
@pytest.mark.parametrize("which", sorted(THIN_KERNELS))
def test_a_thin_frame_against_the_oracle(rpt, oracle, torch_cuda, which, size):
    kernel, launches = THIN_KERNELS[which]
    klass, make, _, _, _, flags = CASES[kernel]
    w, h = size
    scene = make(rpt)
    want = oracle.render(scene.describe(), w, h, sum(launches), seed=SEED, render_flags=_oracle_flags(rpt, flags))
    for dispatch in (None, CHUNKED):
        t = rpt.Tracer(scene, device=0, seed=SEED)
        t.flags = flags
        try:
            if dispatch is not None:
                t.set_dispatch(*dispatch)
            got, _ = _launches(rpt, torch_cuda, t, w, h, launches, 0)
            _assert_ran(_choice(rpt, t), klass, kernel)
        finally:
            t.close()
        assert_same_words(got, want, "%s at %d x %d, dispatch %s" % (which, w, h, dispatch))


@pytest.mark.parametrize("size", [(1, 1), (1, 40)], ids=["1x1", "1x40"])
def test_cost_ordered_launches_of_a_thin_frame(rpt, oracle, torch_cuda, size):
    """Three progressive launches with cost ordering on: the order is learned behind launches 1 and 2 (sched_order_kernel over one
    tile, and over three), and what rpt_debug_sched_read returns is a permutation of the tiles."""
    w, h = size
    n_tiles = ((w + 15) // 16) * ((h + 15) // 16)
    t = rpt.Tracer(_reference(rpt), device=0, seed=SEED)
    try:
        t.set_dispatch(1, 12, 64, 1)
        got, frames = _launches(rpt, torch_cuda, t, w, h, (2, 2, 2), 0)
        _assert_ran(_choice(rpt, t), "small", "render_small_regen_sized_table_kernel")
        raw = np.zeros(10 * n_tiles, dtype=np.uint32)
        nt = C.c_uint32(0)
        rpt._lib.check(rpt.lib().rpt_debug_sched_read(t._h, raw.ctypes.data_as(C.POINTER(C.c_uint32)), n_tiles, C.byref(nt)), t._h)
    finally:
        t.close()
    assert frames == 6 and nt.value == n_tiles
    order = raw[4 * n_tiles:5 * n_tiles].astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(n_tiles)), "the dispatch order %s is no permutation of the %d tiles" % (order, n_tiles)
    assert_same_words(got, oracle.render(oracle.scene_analytical(), w, h, 6, seed=SEED), "three cost-ordered launches at %d x %d" % size)


@pytest.mark.parametrize("size", THIN, ids=THIN_IDS)
@pytest.mark.parametrize("form", [11, 27])
def test_a_thin_mesh_frame_is_radiance_over_its_sample_rays(rpt, torch_cuda, form, size):
    torch = torch_cuda
    w, h = size
    t = open_tracer(rpt, "single", TF.FLAT + " composed", SEED) if form == 11 else open_tracer(rpt, "both maps", "H", SEED)
    try:
        buf = rpt.DeviceColorBuffer(w, h)
        t.render_n(buf, 2)
        torch.cuda.synchronize()
        assert_form(rpt, t, form)
        frame = buf.pixels.cpu().numpy().reshape(w * h, 4)
        out = torch.zeros((w * h, 4), dtype=torch.float32, device="cuda")
        for f in (0, 1):
            t.radiance(t.camera_sample_rays(w, h, f), frames_done=f, out=out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
    finally:
        t.close()
    assert np.isfinite(frame).all() and (frame[:, 3] == 1.0).all()
    assert np.array_equal(_words(got), _words(frame)), "form %d at %d x %d" % (form, w, h)
