"""Mesh launches of more than one sample, and of later frames, held to the float64 restatement (needs an MI355X).

Every other float64 comparison of a mesh kernel renders ONE sample of frame 0 into a fresh buffer, which never leaves the first lines
of render_regen_body_tf (csrc/regen_body.h): a lane traces sample 0 of its own pixel, blends it with weight 1 and retires.  What runs
in every real render, and is compared with a reference here only:
  * later frames — s_fkey[s] and s_weight[s] for s > 0, frames_done > 0 (kernel_common.h, lane_setup_ex);
  * a wave sharing its samples — share_next, share_my_turn, share_blended and the BLOCKED wait: a lane that has handed out its own
    samples renders one of another pixel q of its wave, with its OWN mesh stack and hit state, and the blend still enters q's mean in
    sample order;
  * ragged tiles — lanes with no pixel (share_init(.., false)): 50 x 37 fills no tile in either direction.
Every render is 64 x 48 or 50 x 37 into a DeviceColorBuffer, whose .frames is the frames_done the launch receives (api.py).  Every
test asserts rpt_debug_mesh_form and, for forms 0 .. 11, kernel_census.mesh_kernel_of.

(a) test_a_later_frame_is_that_frame_s_sample, cases A .. H with both maps (forms 20 .. 27) and the flat form (11: the composed
    file's scene with nothing set, through test_gpu_mesh_f64.MeshDescScene — tests/test_mesh_frames_f64.py says why), both sizes.  For k
    in 1, 5, 1000 a one-sample render into a zeroed buffer with buf.frames = k.  The device writes rad * v, v = f32(1 / (k + 1)), so
    the sample is (k + 1) * rgb — two f32 roundings, far below REL_CLEAN — and it is compared through Tally with the restated sample
    of frame k and its margin; alpha is the f32 1 / (k + 1) exactly ((1 - v) * 0 + 1 * v).  At k = 1000 this test cannot see a wrong
    WEIGHT through REL_CLEAN, only a wrong stream: 1 / 1000 and 1 / 1001 are 1e-3 apart, within REL_CLEAN, but for alpha.  At
    64 x 48 it sees it through the samples' own tolerances (below); k = 1, k = 5 and (c) see the weight either way.
(b) test_one_launch_is_its_one_sample_launches, all 28 forms, both sizes: render_n(buf, n) in one launch against n launches of
    render_n(buf2, 1) from the same Tracer, as uint32 — n = 2, 5, 16 from frames_done = 0, and n = 5 on top of 3 earlier frames.
    This is the design's own statement ("which lane renders a sample never changes it ... what must not change is the ORDER",
    kernel_common.h above share_init).  At 16 samples it cannot hold unless sharing and the BLOCKED wait are right: lanes on sky or
    black misses finish their own 16 samples while their neighbours are bounces deep.  The test cannot OBSERVE that sharing
    happened; that follows from share_next's code (a lane with own >= spp takes a needy pixel of its wave), not from a read-out.
    With (a) and (c) it reaches every sample count: the one-sample launches are held to the restatement frame by frame.
    The forms: A .. H as test_gpu_mesh_compose_f64 sets them (0 .. 7), with material maps (12 .. 19), with both maps (20 .. 27), and
    the four base forms A .. H do not reach — flat, smooth, lights without textures, textures without lights (11, 10, 9, 8), on the
    scenes of test_gpu_mesh_f64, test_gpu_mesh_smooth_f64, test_gpu_mesh_light_f64 and test_gpu_mesh_texture_f64.
    test_the_forms_are_all_28 holds the table to set(range(28)); each run asserts the form the device reports against it.
(c) test_a_two_sample_launch_against_the_restatement, the cases of (a): render_n(buf, 2) into a fresh buffer, and the same on top of
    one earlier frame whose device pixels are frame_f64's starting accumulator, against frame_f64's mean through Tally with the
    pixel's margin the smaller of its samples'.  Alpha is exactly 1 from a fresh buffer.
(e) test_a_two_sample_launch_at_depth, the cases of (a) at 64 x 48: render_n(buf, 2) into a zeroed buffer whose .frames is 1000
    (998 for case G: test_mesh_frames_f64.deep_of says why), against frame_f64's mean, both times frames_done + 2, through the
    pixels' own tolerances: the weights of the launch's first and second sample (s_weight[s], s = 0 and s > 0) at high counts.
(d) test_the_heaviest_form_does_not_depend_on_the_dispatch: test_gpu_mesh's four set_dispatch settings and the resident render on
    case H with both maps (form 27) at 50 x 37 x 6 samples, bit for bit.

The draws, their near-tie counts (every one under 24 of 200 by the restatement alone) and what the three planted faults move are in
tests/test_mesh_frames_f64.py; the Tally lines here print the same near-tie shares.  No tolerance of this file's own: TAU, REL_CLEAN,
NEAR_TIE_MAX are test_path_f64's.

Measured on an MI355X (written down, not asserted).  Largest clean relative distance, next to REL_CLEAN = 5e-2: (a) 2.5e-3 (case D,
64 x 48, frame 1000; every other comparison below 2e-3, most near 3e-5), (c) 1.5e-3 (case G, 64 x 48, from a fresh buffer).  Near-tie
shares per Tally line equal to the CPU counts, 1 to 23 of 200.  Wall time per test: (a) 0.28 to 0.53 s and (c) 0.19 to 0.25 s, the
restatement of its 600 and 400 new samples included (this file run alone; that host restates a sample in about 0.5 ms); (b) 0.01
to 0.03 s; (d) 0.02 s; the file's 94 tests 13.5 s.

The comparisons of (a), (c) and (e) at 64 x 48 are also held to each sample's or pixel's own f32 tolerance (tests/f32_spread.py,
through Tally.add's spreads): the first 150 clean samples of a frame are restated in eight noisy runs once
(test_mesh_frames_f64.noisy_samples, shared by every comparison that needs the frame, CPU or GPU), a launch's spread comes from those
runs through frame_f64's blend, which carries noise on the weight, both products and the sum.  The 50 x 37 comparisons stay at
REL_CLEAN: their forms and blends are the same, and their launches are held to the one-sample ones bit for bit by (b).  Conditions,
teeth (v = 1 / (f + 2) from frame 500 on: within REL_CLEAN on every clean sample of case A's frame 1000, beyond their own tolerance
on 94 of 150) and the blend's bits with the mode off are in tests/test_mesh_frames_f64.py.  Measured on an MI355X, over the 27 + 18 +
9 comparisons with spreads: largest z 2.51 (the flat case, two samples on 1000 earlier frames), next to Z_MAX = 8.3; median z 0.13 to 0.45, next to Z_MEDIAN = 1.4; wall
time per test with spreads (a) 3.1 to 4.0 s, (c) 2.0 to 2.5 s, (e) 1.0 to 2.6 s, the noisy runs included.  Measurements, not bounds."""
import ctypes as C

import numpy as np
import pytest

import mesh_emap_f64 as ME
import mesh_mmap_f64 as MM
import test_mesh_frames_f64 as TF
from kernel_census import MESH_RENDER_KERNELS, mesh_kernel_of
from test_gpu_mesh_compose_f64 import CASES
from test_gpu_mesh_compose_f64 import _scene as composed_scene
from test_gpu_mesh_compose_f64 import inputs
from test_gpu_mesh_material_map_f64 import mesh_form, set_composed
from test_gpu_path_f64 import Tally
from test_path_f64 import NEAR_TIE_MAX, TAU

pytestmark = pytest.mark.gpu

SIZES = TF.SIZES
SPREAD_SIZE = SIZES[0]                                               # the size whose comparisons are also held to their own f32 tolerances
SIZE_IDS = ["%dx%d" % s for s in SIZES]
LATER = (1, 5, 1000)
assert set(LATER) | {0, 1, 2} <= set(TF.FRAMES), "every frame compared here has its near ties counted on the CPU"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


# ---- the 28 forms: (stack, case) -> the form the launch must report -------------------------------------------------------------------
SINGLES = {"flat": "mesh_regen_kernel", "smooth": "meshsmooth_regen_kernel", "light": "meshlight_regen_kernel", "texture": "meshtex_regen_kernel"}
FORMS = {}
for _case in sorted(CASES):
    _base = MESH_RENDER_KERNELS.index(CASES[_case][4])
    FORMS[("base", _case)] = _base
    FORMS[("material maps", _case)] = 12 + sorted(CASES).index(_case)
    FORMS[("both maps", _case)] = 20 + sorted(CASES).index(_case)
for _single, _kernel in SINGLES.items():
    FORMS[("single", _single)] = MESH_RENDER_KERNELS.index(_kernel)


def open_tracer(rpt, stack, case, seed):
    """-> a Tracer with the form's set calls made: FORMS' key."""
    if stack == "single":
        if case == TF.FLAT + " composed":                             # the flat form on the composed file's scene: the cases of (a) and (c)
            return rpt.Tracer(TF.flat_scene()[0], device=0, seed=seed)
        from test_gpu_mesh_f64 import _scenes as mesh_scenes
        from test_gpu_mesh_light_f64 import _scenes as light_scenes
        from test_gpu_mesh_texture_f64 import GAMMA, MODES, scene_textures
        if case == "light":
            _, s, smooth, on = light_scenes()[0]
        else:
            s = mesh_scenes()[0][1]
        t = rpt.Tracer(s, device=0, seed=seed)
        if case == "smooth":
            t.set_mesh_shading({m: "smooth" for m in range(len(s.meshes))})
        elif case == "light":
            assert not smooth
            t.set_mesh_lights({m: True for m in on})
        elif case == "texture":
            wrap, filt = MODES[0]
            t.set_mesh_textures({m: dict(uvs=uv, texels=img, wrap=("repeat", "clamp")[wrap], filter=("nearest", "bilinear")[filt], gamma=GAMMA)
                                 for m, (uv, img) in scene_textures(s).items()})
        return t
    s = {"base": composed_scene, "material maps": MM.scene, "both maps": ME.scene}[stack]()
    t = rpt.Tracer(s, device=0, seed=seed)
    set_composed(t, inputs(s, case))
    if stack != "base":
        t.set_mesh_material_maps(MM.material_maps())
    if stack == "both maps":
        t.set_mesh_emission_maps(ME.emission_maps())
    return t


def assert_form(rpt, t, form):
    """The launch that has just run took `form`; for the twelve base forms the kernel is the one kernel_census names for the bits."""
    assert mesh_form(rpt, t) == form, "form %d, not %d" % (mesh_form(rpt, t), form)
    if form < len(MESH_RENDER_KERNELS):
        choice = C.c_uint32()
        assert rpt.lib().rpt_debug_kernel_choice(t._h, C.byref(choice)) == 0
        assert mesh_kernel_of(choice.value) == MESH_RENDER_KERNELS[form]


def render(rpt, torch, t, size, n, buf=None, frames=0):
    """render_n of n samples into `buf`, or into a zeroed buffer whose .frames is `frames` -> (the buffer, its pixels on the host)."""
    if buf is None:
        buf = rpt.DeviceColorBuffer(*size)
        buf.frames = frames
    t.render_n(buf, n)
    torch.cuda.synchronize()
    return buf, buf.pixels.cpu().numpy()


def case_tracer(rpt, case):
    """The Tracer and form of a case of (a) and (c): A .. H with both maps, or the flat form on the composed file's scene."""
    if case == TF.FLAT:
        return open_tracer(rpt, "single", TF.FLAT + " composed", TF.SEED), FORMS[("single", "flat")]
    return open_tracer(rpt, "both maps", case, TF.SEED), FORMS[("both maps", case)]


def test_the_forms_are_all_28():
    assert sorted(FORMS.values()) == list(range(28)) and len(MESH_RENDER_KERNELS) == 12
    assert [FORMS[("base", c)] for c in sorted(CASES)] == [7, 6, 5, 4, 3, 2, 1, 0]


# ---- (a) later frames, sample by sample -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("case", TF.ALL_CASES)
def test_a_later_frame_is_that_frame_s_sample(rpt, oracle, torch_cuda, case, size):
    """At k = 1000 this cannot see a wrong weight (but for alpha), only a wrong stream; k = 1, k = 5 and the two-sample launches see
    the weight."""
    pixels = TF.draws(case)[size]
    t, form = case_tracer(rpt, case)
    try:
        for k in LATER:
            tally = Tally(TAU, NEAR_TIE_MAX)
            _, frame = render(rpt, torch_cuda, t, size, 1, frames=k)
            assert_form(rpt, t, form)
            v = np.float32(1.0) / np.float32(k + 1)
            assert (frame[..., 3] == v).all(), "alpha is (1 - v) * 0 + 1 * v"
            restated, margins = TF.restated(oracle, case, size, k)
            tally.ran.add("form %d" % form)
            tally.add("case %s, %d x %d, frame %d (form %d)" % ((case,) + size + (k, form)), frame.astype(np.float64) * float(k + 1),
                      restated, margins, pixels, spreads=TF.sample_spreads(oracle, case, size, k) if size == SPREAD_SIZE else None)
            tally.check("case %s, %d x %d, frame %d" % ((case,) + size + (k,)))
            assert tally.n == TF.N and tally.near == TF.COUNTS[(case, size[0])][0][TF.FRAMES.index(k)]
    finally:
        t.close()


# ---- (b) one launch equals one-sample launches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("stack,case", sorted(FORMS), ids=["%s-%s" % k for k in sorted(FORMS)])
def test_one_launch_is_its_one_sample_launches(rpt, torch_cuda, stack, case, size):
    """Bit for bit.  This cannot observe that a lane rendered another pixel's sample: that follows from share_next's code, not from
    a read-out.  What it observes is that no sample count, and no start, changes what enters a pixel's mean or in which order."""
    form = FORMS[(stack, case)]
    t = open_tracer(rpt, stack, case, 3)
    try:
        for earlier, n in ((0, 2), (0, 5), (0, 16), (3, 5)):
            one, two = rpt.DeviceColorBuffer(*size), rpt.DeviceColorBuffer(*size)
            if earlier:
                render(rpt, torch_cuda, t, size, earlier, buf=one)
                two.pixels.copy_(one.pixels)
                two.frames = one.frames
            _, got = render(rpt, torch_cuda, t, size, n, buf=one)
            assert_form(rpt, t, form)
            for _ in range(n):
                _, want = render(rpt, torch_cuda, t, size, 1, buf=two)
            assert_form(rpt, t, form)
            assert one.frames == two.frames == earlier + n
            assert np.isfinite(want).all() and want[..., :3].max() > 0.01
            differ = (got.view(np.uint32) != want.view(np.uint32)).any(axis=2)
            assert not differ.any(), "form %d, %d x %d, %d samples on %d earlier frames: %d pixels differ, first (row, col) %s" % (
                (form,) + size + (n, earlier, int(differ.sum()), tuple(np.argwhere(differ)[0])))
    finally:
        t.close()


# ---- (c) a two-sample launch against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("case", TF.ALL_CASES)
def test_a_two_sample_launch_against_the_restatement(rpt, oracle, torch_cuda, case, size):
    pixels = TF.draws(case)[size]
    t, form = case_tracer(rpt, case)
    try:
        for launch, (frames_done, _) in enumerate(TF.LAUNCHES):
            buf, acc = None, None
            if frames_done:
                buf, first = render(rpt, torch_cuda, t, size, frames_done)
                acc = np.array([first[r, c] for c, r in pixels], dtype=np.float64)
            buf, frame = render(rpt, torch_cuda, t, size, 2, buf=buf)
            assert_form(rpt, t, form)
            assert buf.frames == frames_done + 2
            if not frames_done:
                assert (frame[..., 3] == 1.0).all(), "alpha is (1 - 1/2) * 1 + 1/2"
            mean, margins, _ = TF.launch_f64(oracle, case, size, frames_done, 2, acc=acc)
            tally = Tally(TAU, NEAR_TIE_MAX)
            tally.ran.add("form %d" % form)
            what = "case %s, %d x %d, two samples on %d earlier" % ((case,) + size + (frames_done,))
            tally.add("%s (form %d)" % (what, form), frame, mean[:, :3], margins, pixels,
                      spreads=TF.launch_spreads(oracle, case, size, frames_done, 2, acc=acc) if size == SPREAD_SIZE else None)
            tally.check(what)
            assert tally.n == TF.N and tally.near == TF.COUNTS[(case, size[0])][2][launch]
            assert np.abs(np.array([frame[r, c, 3] for c, r in pixels], dtype=np.float64) - mean[:, 3]).max() < 1e-6
    finally:
        t.close()


# ---- (e) a two-sample launch at depth ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TF.ALL_CASES)
def test_a_two_sample_launch_at_depth(rpt, oracle, torch_cuda, case):
    """render_n(buf, 2) into a zeroed buffer whose .frames is about 1000 (TF.deep_of), 64 x 48, against frame_f64's mean, both
    times frames_done + 2 — the sum of the two samples, but for a part in a thousand — and held to the pixels' own tolerances: a
    stale or off-by-one weight of the launch's first or second sample is a part in a thousand of one of them."""
    size, deep = SPREAD_SIZE, TF.deep_of(case)
    pixels = TF.draws(case)[size]
    t, form = case_tracer(rpt, case)
    try:
        buf, frame = render(rpt, torch_cuda, t, size, 2, frames=deep)
        assert_form(rpt, t, form)
        assert buf.frames == deep + 2
    finally:
        t.close()
    scale = float(deep + 2)
    mean, margins, _ = TF.launch_f64(oracle, case, size, deep, 2)
    tally = Tally(TAU, NEAR_TIE_MAX)
    tally.ran.add("form %d" % form)
    what = "case %s, %d x %d, two samples on %d earlier" % ((case,) + size + (deep,))
    tally.add("%s (form %d)" % (what, form), frame.astype(np.float64) * scale, mean[:, :3] * scale, margins, pixels,
              spreads=TF.launch_spreads(oracle, case, size, deep, 2, scale=scale))
    tally.check(what)
    assert tally.n == TF.N and tally.near == TF.DEEP_NEAR[case]
    assert np.abs(np.array([frame[r, c, 3] for c, r in pixels], dtype=np.float64) - mean[:, 3]).max() < 1e-9


# ---- (d) dispatch independence of the heaviest form --------------------------------------------------------------------------------------
def test_the_heaviest_form_does_not_depend_on_the_dispatch(rpt, torch_cuda):
    (w, h), spp = SIZES[1], 6
    t = open_tracer(rpt, "both maps", "H", 3)
    try:
        _, ref = render(rpt, torch_cuda, t, (w, h), spp)
        assert_form(rpt, t, 27)
        assert np.isfinite(ref).all() and ref[..., :3].mean() > 0.01
        for disp in ((0, 12, 64, 0), (1, 0, 64, 0), (1, 1000, 1, 0), (2, 1000, 2, 7)):      # incl. chunked launches (unit_rounds 1000)
            t.set_dispatch(*disp)
            _, got = render(rpt, torch_cuda, t, (w, h), spp)
            assert_form(rpt, t, 27)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), disp
        t.set_dispatch(1, 12, 64, 0)
        t.render_resident(w, h, spp)
        assert_form(rpt, t, 27)
        res = t.resident_to_host(w, h).pixels.reshape(h, w, 4)
        assert np.array_equal(res.view(np.uint32), ref.view(np.uint32)), "resident"
    finally:
        t.close()
