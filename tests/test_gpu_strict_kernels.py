"""Every strict render kernel (the product's arithmetic: bit-identical to the CPU oracle) aimed at on purpose, confirmed through
rpt_debug_kernel_choice, and compared with the oracle on every pixel; then the compacting kernel of one-sample launches in each of its
regimes, at their edges.  The GPU tests need an MI355X and are marked one by one: the coverage test reads the library's code object
and runs without a GPU, so that a render kernel added without a case fails the CPU suite.

The compacting kernel (k_compact.hip) has a dense form up to kCompactDenseMaxBlocks (3 072) workgroups and a sparse form beyond.  From
3 x slots workgroups on (capi.hip, launch_render: slots = CUs x 5, or rpt_set_dispatch's unit_slots) its launches run their tiles
in the order the previous launches' costs give, re-learned at launches 1, 2, 4, 8, ...: the reference's own 1080p redraw loop (one
sample per render(), 8 160 workgroups) is such a launch."""
import ctypes as C

import numpy as np
import pytest

from kernel_census import COMPACT_BIT, DENSE_BIT, MEDIA_BIT, kernel_of, render_kernels

TILE = 16


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _table(rpt, which):
    from test_gpu_dispatch import _table_scene
    return _table_scene(rpt, which)[0]


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


def _large(rpt):
    from rust_pathtracer_amd import scenes
    return scenes.random_spheres_scene(300, 5)


def _media(rpt):
    from rust_pathtracer_amd import scenes
    return scenes.media_scene()


def _sdf_fog(rpt):
    """The SDF object full of scattering fog next to a ball of absorbing glass (tests/test_gpu_media.py)."""
    from rust_pathtracer_amd import scenes
    s = scenes.sdf_scene()
    s.media = True
    s.max_depth = 8
    s.any_hit_uses_max_dist = True
    s.materials[0] = rpt.Material(rgb=(0.9, 0.95, 1.0), roughness=0.1, spec_trans=1.0, ior=1.25,
                                  medium=dict(type="scatter", density=2.5, color=(0.7, 0.85, 1.0), anisotropy=-0.3))
    s.materials[1] = rpt.Material(rgb=(1.0, 0.6, 0.3), roughness=0.1, spec_trans=1.0, ior=1.4, medium=dict(type="absorb", density=2.0, color=(1.0, 0.4, 0.1)))
    return s


def _large_media(rpt):
    from rust_pathtracer_amd import scenes
    s = scenes.random_spheres_scene(n_spheres=300, n_lights=5, media=True, n_palette=24)
    s.max_depth = 9
    return s


def _reference(rpt):
    return rpt.AnalyticalScene()


def _general(rpt):
    """Four primitives: neither the reference's table sizes nor a material table in the compacting kernel."""
    return _table(rpt, "three spheres on a floor")


# ---- one case per strict render kernel --------------------------------------------------------------------------------------------
NESTED = 1 << 0
# kernel -> (class, scene(rpt), width, height, launches (samples per render_n call), render flags).  Every frame is ragged (neither side
# a multiple of 16) and every case resumes an accumulation.  Small scenes: launches of 2+ samples take the megakernel, launches of one
# sample the compacting kernel — dense up to 3 072 tiles (170 x 99 = 77 tiles), sparse beyond (1 034 x 771 = 3 185 tiles, below
# 3 x slots on a whole MI355X: not cost-ordered; test_cost_ordered_compacting_launches has those).
MEGA, DENSE, SPARSE = (122, 75, (3, 3)), (170, 99, (1,) * 4), (1034, 771, (1, 1))
OTHER = (118, 69, (3, 3))
CASES = {
    "render_small_nested_kernel": ("small", _reference) + MEGA + (NESTED,),
    "render_small_regen_kernel": ("small", lambda r: _table(r, "eight primitives many classes")) + MEGA + (0,),
    "render_small_regen_sized_kernel": ("small", lambda r: _table(r, "two checkers")) + MEGA + (0,),
    "render_small_regen_sized_table_kernel": ("small", _reference) + MEGA + (0,),
    "render_small_regen_table_kernel": ("small", _general) + MEGA + (0,),
    "render_small_regen_maptable_kernel": ("small", lambda r: _table(r, "six spheres two planes")) + MEGA + (0,),
    "render_small_compact_dense_sized_table_kernel": ("small", _reference) + DENSE + (0,),
    "render_small_compact_sized_table_kernel": ("small", _reference) + SPARSE + (0,),
    "render_small_compact_dense_sized_kernel": ("small", lambda r: _table(r, "two checkers")) + DENSE + (0,),
    "render_small_compact_sized_kernel": ("small", lambda r: _table(r, "two checkers")) + SPARSE + (0,),
    "render_small_compact_dense_table_kernel": ("small", lambda r: _table(r, "one sphere two planes")) + DENSE + (0,),
    "render_small_compact_table_kernel": ("small", lambda r: _table(r, "one sphere two planes")) + SPARSE + (0,),
    "render_small_compact_dense_kernel": ("small", _general) + DENSE + (0,),
    "render_small_compact_kernel": ("small", _general) + SPARSE + (0,),
    "render_sdf_march2_kernel": ("sdf", lambda r: _sdf(r, 5, spheres=2)) + OTHER + (0,),
    "render_sdf_march2_table_kernel": ("sdf", lambda r: _sdf(r, 3, lights=2)) + OTHER + (0,),
    "render_large_regen_kernel": ("large", _large) + OTHER + (0,),
    # participating media: one form per class
    "render_small_regen_media_kernel": ("small", _media, 98, 73, (2, 3), 0),
    "render_small_compact_media_kernel": ("small", _media, 98, 73, (1, 1, 1), 0),
    "render_sdf_march2_media_kernel": ("sdf", _sdf_fog, 86, 61, (2, 2), 0),
    "render_large_regen_media_kernel": ("large", _large_media, 74, 43, (2, 2), 0),
}
for _n in (1, 2, 3, 4):
    CASES["render_sdf_march2_sized_kernel<%d>" % _n] = ("sdf", lambda r, n=_n: _sdf(r, n, spheres=2)) + OTHER + (0,)
    CASES["render_sdf_march2_sized_table_kernel<%d>" % _n] = ("sdf", lambda r, n=_n: _sdf(r, n)) + OTHER + (0,)


def _render(rpt, torch, scene, w, h, launches, flags, seed=1, dispatch=None, keep=False):
    """The frame after render_n(n) for n in launches -> (frame, kernel choice of the last launch[, the open tracer if keep])."""
    t = rpt.Tracer(scene, device=0, seed=seed)
    t.flags = flags
    if dispatch is not None:
        t.set_dispatch(*dispatch)
    buf = rpt.DeviceColorBuffer(w, h)
    for n in launches:
        t.render_n(buf, n)
    torch.cuda.synchronize()
    choice = _choice(rpt, t)
    img = buf.pixels.cpu().numpy()
    if keep:
        return img, choice, t
    t.close()
    return img, choice


def _choice(rpt, t):
    choice = C.c_uint32()
    assert rpt.lib().rpt_debug_kernel_choice(t._h, C.byref(choice)) == 0
    return choice.value


def _want(rpt, oracle, scene, w, h, spp, flags, seed=1):
    return oracle.render(scene.describe(), w, h, spp, seed=seed, render_flags=flags & rpt._abi.RPT_RENDER_RUSSIAN_ROULETTE)


def _assert_ran(choice, klass, kernel):
    assert kernel_of(choice, klass) == kernel, "aimed at %s, ran %s (choice %#x)" % (kernel, kernel_of(choice, klass), choice)


@pytest.mark.gpu
@pytest.mark.parametrize("rr", [False, True], ids=["as-declared", "roulette"])
@pytest.mark.parametrize("kernel", sorted(CASES))
def test_every_strict_kernel_against_the_oracle(rpt, oracle, torch_cuda, kernel, rr):
    from test_gpu_parity import assert_bit_identical
    klass, make, w, h, launches, flags = CASES[kernel]
    assert w % TILE and h % TILE and len(launches) >= 2, "a case renders a ragged frame and resumes its accumulation"
    flags |= rpt._abi.RPT_RENDER_RUSSIAN_ROULETTE if rr else 0
    scene = make(rpt)
    frame, choice = _render(rpt, torch_cuda, scene, w, h, launches, flags, seed=3)
    _assert_ran(choice, klass, kernel)
    assert_bit_identical(frame, _want(rpt, oracle, scene, w, h, sum(launches), flags, seed=3), "%s, roulette %s" % (kernel, rr))


def test_the_case_list_is_the_library_s_strict_kernels(rpt):
    """Every strict render_* kernel of the loaded library's gfx950 code object has a case above, and every case names one of them
    (25 counterparts of the relaxed kernels and four media forms).  Needs no GPU."""
    names = render_kernels(rpt._lib.LIB_PATH, relaxed=False)
    assert len(names) == 29 and names == set(CASES), "library: %s; cases: %s" % (sorted(names - set(CASES)), sorted(set(CASES) - names))


# ---- the compacting kernel's regimes -----------------------------------------------------------------------------------------------
def _tiles(w, rows):
    return ((w + TILE - 1) // TILE) * ((rows + TILE - 1) // TILE)


def _compact_name(which, dense):
    return "render_small_compact_%s%skernel" % ("dense_" if dense else "", "sized_table_" if which == "reference" else "")


def _assert_compact(choice, which, dense):
    assert choice & COMPACT_BIT and bool(choice & DENSE_BIT) == dense and not choice & MEDIA_BIT, hex(choice)
    _assert_ran(choice, "small", _compact_name(which, dense))


def _assert_learned_order(rpt, t, n_tiles):
    """The dispatch order the context's last launch ran (rpt_debug_sched_read) is a permutation of its tiles, and one that launches
    before it learned: neither tile order nor the bottom-rows-first order a context starts from (k_util.hip, sched_init_kernel)."""
    raw = np.zeros(10 * n_tiles, dtype=np.uint32)
    nt = C.c_uint32(0)
    rpt._lib.check(rpt.lib().rpt_debug_sched_read(t._h, raw.ctypes.data_as(C.POINTER(C.c_uint32)), n_tiles, C.byref(nt)), t._h)
    assert nt.value == n_tiles
    order = raw[4 * n_tiles:5 * n_tiles].astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(n_tiles)), "the dispatch order is not a permutation of the %d tiles" % n_tiles
    assert not np.array_equal(order, np.arange(n_tiles)), "the launch ran its tiles in tile order: no cost-ordered launch"
    assert not np.array_equal(order, np.arange(n_tiles)[::-1]), "the launch ran its tiles bottom rows first: no order was learned"


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["reference", "general"])
@pytest.mark.parametrize("h,dense", [(768, True), (769, False)], ids=["1024x768-dense", "1024x769-sparse"])
def test_the_compacting_kernel_at_the_dense_sparse_boundary(rpt, oracle, torch_cuda, which, h, dense):
    """1 024 x 768 is exactly 3 072 workgroups: the dense form.  1 024 x 769 is 3 136, its last tile row one pixel row: the sparse form."""
    from test_gpu_parity import assert_bit_identical
    w = 1024
    assert (_tiles(w, h) <= 3072) == dense
    scene = {"reference": _reference, "general": _general}[which](rpt)
    frame, choice = _render(rpt, torch_cuda, scene, w, h, (1, 1), 0, seed=5)
    _assert_compact(choice, which, dense)
    assert_bit_identical(frame, _want(rpt, oracle, scene, w, h, 2, 0, seed=5), "%s scene %dx%d" % (which, w, h))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["reference", "general"])
@pytest.mark.parametrize("w,h,slots,dense", [(170, 99, 16, True), (1034, 771, 64, False)], ids=["dense", "sparse"])
def test_cost_ordered_compacting_launches(rpt, oracle, torch_cuda, which, w, h, slots, dense):
    """rpt_set_dispatch's unit_slots stands for the device's workgroup slots, so that launches of at least 3 x slots tiles run cost-ordered
    whatever the device's partitioning: 77 tiles against 16 slots (dense and cost-ordered, as on a partitioned device), 3 185 against 64
    (sparse).  Nine one-sample launches: the order is learned at launches 1, 2, 4 and 8, and the ninth runs the eighth's."""
    from test_gpu_parity import assert_bit_identical
    n_tiles = _tiles(w, h)
    assert n_tiles >= 3 * slots and (n_tiles <= 3072) == dense
    scene = {"reference": _reference, "general": _general}[which](rpt)
    frame, choice, t = _render(rpt, torch_cuda, scene, w, h, (1,) * 9, 0, seed=6, dispatch=(1, 12, 64, slots), keep=True)
    try:
        _assert_compact(choice, which, dense)
        _assert_learned_order(rpt, t, n_tiles)
    finally:
        t.close()
    assert_bit_identical(frame, _want(rpt, oracle, scene, w, h, 9, 0, seed=6), "%s scene %dx%d, cost-ordered" % (which, w, h))


@pytest.mark.gpu
def test_the_reference_redraw_loop_at_1080p(rpt, oracle, torch_cuda):
    """renderer/src/main.rs's loop at 1920 x 1080 with the default dispatch: nine x {render(); convert_to_u8()} on the resident buffer.
    8 160 workgroups (67.5 tile rows): the sparse form, cost-ordered.  The whole f32 frame and the u8 frame are the oracle's."""
    from test_gpu_parity import assert_bit_identical
    w, h, n = 1920, 1080, 9
    t = rpt.Tracer(rpt.AnalyticalScene(), device=0, seed=1)
    try:
        t.resident_reset()
        for _ in range(n):
            t.render_resident(w, h)                                   # pt.render(&mut buffer)
            frame = t.resident_to_u8(w, h).copy()                     # buffer.convert_to_u8(frame)
        assert t.resident_frames() == n
        _assert_compact(_choice(rpt, t), "reference", False)
        _assert_learned_order(rpt, t, _tiles(w, h))
        got = t.resident_to_host(w, h).image()
    finally:
        t.close()
    want = oracle.render(oracle.scene_analytical(), w, h, n, seed=1)
    assert_bit_identical(got, want, "1920x1080, %d redraws" % n)
    assert np.array_equal(frame, oracle.convert_to_u8(want, w, h)), "the u8 frame differs from the oracle's"


@pytest.mark.gpu
def test_a_rank_tile_at_one_sample_per_launch(rpt, oracle, torch_cuda):
    """configs[2]'s geometry (3 840 x 2 160, 8 virtual ranks, 2-row tiles), one sample per launch: rank 3's 270 rows are 240 x 17
    workgroups (the last tile row holds 14 rows), sparse and cost-ordered.  Rows at both ends of the tile and within it, from the
    oracle's full frame."""
    from rust_pathtracer_amd import tiling
    from test_gpu_parity import assert_bit_identical
    torch = torch_cuda
    w, h, world, tile_rows, rank, n = 3840, 2160, 8, 2, 3, 9
    rows = tiling.tile_global_rows(h, tile_rows, rank, world)
    assert len(rows) == 270 and _tiles(w, len(rows)) == 4080
    t = rpt.Tracer(rpt.AnalyticalScene(), device=0, seed=1)
    try:
        tile = torch.zeros(len(rows), w, 4, dtype=torch.float32, device="cuda")
        for k in range(n):
            t.render_tile(tile, w, h, k, 1, tile_rows, rank, world)
        torch.cuda.synchronize()
        _assert_compact(_choice(rpt, t), "reference", False)
        _assert_learned_order(rpt, t, 4080)
        got = tile.cpu().numpy()
    finally:
        t.close()
    local = [0, 1, 100, 255, 256, 268, 269]
    want = oracle.render_rows(oracle.scene_analytical(), w, h, n, [rows[lr] for lr in local], seed=1)
    for lr in local:
        assert_bit_identical(got[lr], want[rows[lr]], "rank %d local row %d (global %d)" % (rank, lr, rows[lr]))


# ---- the aimed-at check has teeth ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_without_the_material_table_another_kernel_runs(rpt, oracle, torch_cuda, monkeypatch):
    """RPT_NO_MATERIAL_TABLE=1 turns the table off: a table case then runs another kernel (which the matrix above would report), and the
    frame is still the oracle's."""
    from test_gpu_parity import assert_bit_identical
    kernel = "render_small_compact_sized_table_kernel"
    klass, make, w, h, launches, flags = CASES[kernel]
    monkeypatch.setenv("RPT_NO_MATERIAL_TABLE", "1")
    rpt.lib().rpt_debug_reload_knobs()
    scene = make(rpt)
    frame, choice = _render(rpt, torch_cuda, scene, w, h, launches, flags, seed=3)
    assert kernel_of(choice, klass) != kernel and kernel_of(choice, klass) == "render_small_compact_sized_kernel", hex(choice)
    assert_bit_identical(frame, _want(rpt, oracle, scene, w, h, sum(launches), flags, seed=3), "%s without the table" % kernel)
