"""The device held to tests/pt_f64.py, the float64 restatement of one pixel-sample, with no oracle/rpt_oracle.hpp in the loop (needs
an MI355X).  A one-sample render into a fresh buffer (frames = 0) is the sample itself (mix_color with v = 1, tracer.rs:115; a
non-finite sample blended as black), so per-sample values come from one-sample renders at several seeds:

  * the reference's scene at 800 x 600: six whole rows (the first, the last, the middle two and two more) and 2 000 random pixels, at
    two seeds through the compacting kernel (what a one-sample launch takes) and one through the sized-table megakernel;
  * the fuzzed small scenes of tests/test_path_f64.py at 64 x 48, alternately through the compacting kernel and the megakernel, the
    light-types and occluder scenes, and a scene of eight primitives that takes the per-hit general megakernel;
  * one large-class scene (1 000 spheres, 16 lights), which the restatement brute-forces with numpy over the sphere table (held to
    the large-scene margin TAU_LARGE: its coordinates are ~100).
The kernel that ran is asserted (rpt_debug_kernel_choice, tests/kernel_census.py).  Samples are split at the branch margin
test_path_f64.TAU: clean samples must be within REL_CLEAN of the restatement, near-tie ones at most NEAR_TIE_MAX of all — the
bounds the CPU leg calibrated on the f32 oracle, the device's twin.  The device probes (rpt_probe_fn) of disney_eval, disney_sample
and sample_light are held to the restatement's functions at the same bound.

The small scenes are also held to each sample's own f32 tolerance (Tally.add's spreads, tests/f32_spread.py).  There the device is
the f32 oracle's bit-identical twin and the bounds were calibrated on that oracle, so it passes by construction: a failure would mean
that the harness is wrong, not the kernel.  Largest z seen on an MI355X over the 6 123 clean samples: 5.04, median 0.349 (the oracle's
own over tests/test_path_f64.py's set: 4.15 and 0.346) — a measurement, not a bound."""
import numpy as np
import pytest

import pt_f64 as P
from kernel_census import kernel_of
from scene_fuzz import random_small_scene
from test_path_f64 import (FUZZ_SEEDS, NEAR_TIE_MAX, NEAR_TIE_MAX_LARGE, REL_CLEAN, TAU, TAU_LARGE, light_types_scene, occluder_scene,
                           rel_distance)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _one_sample(rpt, torch, scene, w, h, seed, megakernel, monkeypatch, flags=0):
    """A one-sample render into a fresh buffer -> (frame, kernel choice).  megakernel: RPT_COMPACT_MAX_SPP=0, so that the launch takes
    the class's megakernel instead of the compacting kernel.  flags: render flags (RPT_RENDER_RUSSIAN_ROULETTE)."""
    from test_gpu_strict_kernels import _render
    if megakernel:
        monkeypatch.setenv("RPT_COMPACT_MAX_SPP", "0")
    else:
        monkeypatch.delenv("RPT_COMPACT_MAX_SPP", raising=False)
    rpt.lib().rpt_debug_reload_knobs()
    try:
        return _render(rpt, torch, scene, w, h, (1,), flags, seed=seed)
    finally:
        monkeypatch.delenv("RPT_COMPACT_MAX_SPP", raising=False)
        rpt.lib().rpt_debug_reload_knobs()


class Tally:
    def __init__(self, tau=TAU, near_max=NEAR_TIE_MAX):
        self.tau, self.near_max = tau, near_max
        self.n = self.near = 0
        self.worst = 0.0
        self.ran = set()
        self.held = None                                              # f32_spread.Statements, once an add() brought spreads

    def add(self, what, frame, restated, margins, pixels, spreads=None):
        """frame: the device's; restated [n, 3] f64 and margins for `pixels` [(col, row)].  spreads [n] (tests/f32_spread.py; NaN:
        none for that sample): a clean sample that has one must also be within its own tolerance, and check() holds the set to the
        median and bias statements.  Without spreads nothing changes."""
        got = np.where(np.isfinite(restated), restated, 0.0)           # blended as black
        dev = np.array([frame[r, c, :3] for c, r in pixels], dtype=np.float64)
        rel = rel_distance(got, dev)
        tie = margins <= self.tau
        self.n += len(rel)
        self.near += int(tie.sum())
        if (~tie).any():
            self.worst = max(self.worst, float(rel[~tie].max()))
        bad = np.nonzero((rel > REL_CLEAN) & ~tie)[0]
        assert not bad.size, "%s: %d clean samples beyond %g; first pixel %s: device %s, restated %s, margin %.3g" % (
            what, bad.size, REL_CLEAN, pixels[bad[0]], dev[bad[0]].tolist(), got[bad[0]].tolist(), margins[bad[0]])
        if spreads is not None:
            import f32_spread as S
            self.held = self.held or S.Statements()
            bad = self.held.add(got, dev, ~tie, spreads)
            z = S.z_of(rel, np.nan_to_num(np.asarray(spreads, np.float64)))
            assert not bad.size, "%s: %d clean samples beyond their own tolerance, worst first:\n%s" % (what, bad.size, "\n".join(
                "  pixel %s: device %s, restated %s, distance %.3g, spread %.3g, z %.3g, margin %.3g" % (
                    pixels[k], dev[k].tolist(), got[k].tolist(), rel[k], spreads[k], z[k], margins[k])
                for k in sorted(bad, key=lambda k: -z[k])[:8]))

    def check(self, what):
        print("%s: %d samples, %d near-tie (%.2f %%), largest clean relative distance %.3g, kernels %s" % (
            what, self.n, self.near, 100.0 * self.near / max(self.n, 1), self.worst, sorted(self.ran)))
        if self.held is not None:
            print("%s: %s" % (what, self.held.line()))
        assert self.near <= self.near_max * self.n
        if self.held is not None:
            assert not self.held.failures(), "%s: %s" % (what, "; ".join(self.held.failures()))


def _compare(rpt, torch, oracle, tally, what, scene, w, h, seed, megakernel, monkeypatch, pixels, klass="small", flags=0, restate=None,
             with_spreads=False):
    """restate(oracle, seed, items, w, h) -> (radiance, margins, ...): another restatement than pt_f64's of scene.describe()
    (tests/media_sdf_f64.py's); flags: render flags of the launch, which that restatement has to follow.  with_spreads: every sample
    is also held to its own f32 tolerance (tests/f32_spread.py)."""
    frame, choice = _one_sample(rpt, torch, scene, w, h, seed, megakernel, monkeypatch, flags)
    tally.ran.add(kernel_of(choice, klass))
    items = [(c, r, 0) for c, r in pixels]
    if restate is not None:
        restated, margins = restate(oracle, seed, items, w, h)[:2]
    else:
        assert flags == 0
        restated, margins, _ = P.sample_many(P.DescScene(scene.describe()), oracle, seed, items, w, h)
    spreads = None
    if with_spreads:
        import f32_spread as S
        assert restate is None
        sc = P.DescScene(scene.describe())
        spreads = S.spread(lambda: P.sample_many(sc, oracle, seed, items, w, h), plain=restated)
    tally.add("%s (seed %d, %s)" % (what, seed, kernel_of(choice, klass)), frame, restated, margins, pixels, spreads=spreads)
    return choice


def test_reference_scene_against_the_restatement(rpt, oracle, torch_cuda, monkeypatch):
    w, h = 800, 600
    rng = np.random.default_rng(31)
    rows = (0, 1, 299, 300, 451, 599)
    pixels = [(c, r) for r in rows for c in range(w)] + list(zip(rng.integers(0, w, 2000).tolist(), rng.integers(0, h, 2000).tolist()))
    t = Tally()
    for seed, mega in ((1, False), (2, False), (3, True)):
        _compare(rpt, torch_cuda, oracle, t, "reference scene", rpt.AnalyticalScene(), w, h, seed, mega, monkeypatch, pixels)
    t.check("reference scene")
    assert {"render_small_compact_dense_sized_table_kernel", "render_small_regen_sized_table_kernel"} <= t.ran


def test_small_scenes_against_the_restatement(rpt, oracle, torch_cuda, monkeypatch):
    from test_gpu_dispatch import _table_scene
    w, h = 64, 48
    rng = np.random.default_rng(32)
    t = Tally()
    scenes = [("fuzz seed %d" % s, random_small_scene(rpt, s, log2_scale=0)[0]) for s in FUZZ_SEEDS]
    scenes += [("light types", light_types_scene(rpt)), ("occluder behind the light", occluder_scene(rpt)),
               ("eight primitives", _table_scene(rpt, "eight primitives many classes")[0])]
    for k, (what, s) in enumerate(scenes):
        pixels = list(zip(rng.integers(0, w, 240).tolist(), rng.integers(0, h, 240).tolist()))
        mega = k % 2 == 1 or what == "eight primitives"
        _compare(rpt, torch_cuda, oracle, t, what, s, w, h, 40 + k, mega, monkeypatch, pixels, with_spreads=True)
    t.check("small scenes")
    assert "render_small_regen_kernel" in t.ran                       # the per-hit general megakernel
    assert any(k.startswith("render_small_compact_") for k in t.ran)
    assert any(k.startswith("render_small_regen_") and k != "render_small_regen_kernel" for k in t.ran)


def test_large_scene_against_the_restatement(rpt, oracle, torch_cuda, monkeypatch):
    from rust_pathtracer_amd import scenes
    s = scenes.random_spheres_scene(1000, 16)
    w, h = 96, 64
    rng = np.random.default_rng(33)
    pixels = list(zip(rng.integers(0, w, 400).tolist(), rng.integers(0, h, 400).tolist()))
    t = Tally(TAU_LARGE, NEAR_TIE_MAX_LARGE)
    choice = _compare(rpt, torch_cuda, oracle, t, "1 000 spheres, 16 lights", s, w, h, 5, False, monkeypatch, pixels, klass="large")
    t.check("large scene")
    assert kernel_of(choice, "large") == "render_large_regen_kernel"


# ---- device probes against the restatement's functions -----------------------------------------------------------------------
def _probe_tracer(rpt):
    return rpt.Tracer(rpt.AnalyticalScene(), device=0, seed=1)


# The probe records are edge-heavy by construction (tests/test_gpu_probes.py: 8 % grazing views, 10 % normals on the onb's switch,
# black dielectrics): the near-tie fraction measured through the f32 oracle's probes was 7 % (disney_eval) and 17 % (disney_sample).
PROBE_NEAR_TIE_MAX = 0.25


def _within(mine, dev, margin):
    mine = np.where(np.isfinite(mine), mine, 0.0)
    dev = np.where(np.isfinite(dev), dev, 0.0).astype(np.float64)
    rel = (np.abs(dev - mine) / np.maximum(np.abs(mine), 1e-3)).max()
    return margin <= TAU or rel <= REL_CLEAN, rel


def test_bsdf_and_light_probes_against_the_restatement(rpt, torch_cuda):
    from test_gpu_probes import _bsdf_records, device_probe, records, u32_as_f32, unit
    from test_path_f64 import pcg_stream, widen
    A = rpt._abi
    n = 3000
    tr = _probe_tracer(rpt)
    try:
        rng = np.random.default_rng(34)
        rec, _ = _bsdf_records(rng, n)
        rec[:, 24:27] = unit(rng, n)
        got = device_probe(rpt, torch_cuda, tr, A.RPT_PROBE_FN_DISNEY_EVAL, rec)
        near = 0
        for k in range(n):
            M = P.Margin()
            f, pdf = P.disney_eval(P.Material.from17(rec[k, :17]).finalize(), float(rec[k, 17]), widen(rec[k, 18:21]),
                                   widen(rec[k, 21:24]), widen(rec[k, 24:27]), M=M)
            ok, rel = _within(np.array(f + (pdf,)), got[k, :4], M.m)
            near += M.m <= TAU
            assert ok, ("disney_eval", k, rec[k].tolist(), got[k, :4], f, pdf, rel)
        assert near <= PROBE_NEAR_TIE_MAX * n, near

        rec, _ = _bsdf_records(rng, n)
        stale = unit(rng, n)
        stale[rng.uniform(size=n) < 0.4] = 0.0
        rec[:, 24:27] = stale
        rec[:, 27] = u32_as_f32(rng.integers(0, 2 ** 32, size=n, dtype=np.uint64))
        rec[:, 28] = u32_as_f32(rng.integers(0, 2 ** 22, size=n, dtype=np.uint64))
        got = device_probe(rpt, torch_cuda, tr, A.RPT_PROBE_FN_DISNEY_SAMPLE, rec)
        near = 0
        for k in range(n):
            M = P.Margin()
            dr = pcg_stream(int(rec[k, 27:28].view(np.uint32)[0]), int(rec[k, 28:29].view(np.uint32)[0]))
            calls = [0]

            def draw():
                calls[0] += 1
                return dr()
            f, lo, pdf = P.disney_sample(P.Material.from17(rec[k, :17]).finalize(), float(rec[k, 17]), widen(rec[k, 18:21]),
                                         widen(rec[k, 21:24]), widen(rec[k, 24:27]), draw, M=M)
            assert M.m <= TAU or got[k, 7] == calls[0], (k, got[k], calls[0], rec[k].tolist())      # the arm the draws took
            # a grazing view (|v.n| < 1e-3, the records' 8 %) puts the specular lobe's 1 / (4 l.z v.z) and the GGX sample's
            # v.z-scaled half vector at f32's resolution: such a record counts as a near tie as well
            grazing = abs(float(np.dot(rec[k, 18:21].astype(np.float64), rec[k, 21:24].astype(np.float64)))) < 1e-3
            ok, rel = _within(np.array(f + lo + (pdf,)), got[k, :7], 0.0 if grazing else M.m)
            near += M.m <= TAU or grazing
            assert ok, ("disney_sample", k, rec[k].tolist(), got[k, :7], f, lo, pdf, rel)
        assert near <= PROBE_NEAR_TIE_MAX * n, near

        rec = records(n)
        types = rng.choice([A.RPT_LIGHT_SPHERICAL, A.RPT_LIGHT_SPHERICAL, A.RPT_LIGHT_RECTANGULAR, A.RPT_LIGHT_DISTANT], size=n)
        rec[:, 0] = u32_as_f32(types)
        rec[:, 1:4] = rng.uniform(-4, 4, size=(n, 3))
        rec[:, 4:7] = rng.uniform(0, 5, size=(n, 3))
        rec[:, 7] = rng.choice([1.0, 0.25, 2.0], size=n)
        rec[:, 8] = (4.0 * np.pi * rec[:, 7] ** 2).astype(np.float32)
        rec[:, 9:15] = rng.uniform(-2, 2, size=(n, 6))
        rec[:, 15:18] = rng.uniform(-6, 6, size=(n, 3))
        rec[:, 18] = rng.choice([1.0, 3.0, 16.0], size=n)
        rec[:, 19] = u32_as_f32(rng.choice([0, A.RPT_SCENE_SAMPLE_ALL_LIGHT_TYPES], size=n))
        rec[:, 20] = u32_as_f32(rng.integers(0, 2 ** 32, size=n, dtype=np.uint64))
        rec[:, 21] = u32_as_f32(rng.integers(0, 2 ** 22, size=n, dtype=np.uint64))
        got = device_probe(rpt, torch_cuda, tr, A.RPT_PROBE_FN_SAMPLE_LIGHT, rec)
        for k in range(n):
            r = rec[k]

            class S:
                flags = int(r[19:20].view(np.uint32)[0])
                lights = [None] * int(r[18])
            light = (int(types[k]), widen(r[1:4]), widen(r[4:7]), widen(r[9:12]), widen(r[12:15]), float(r[7]), float(r[8]))
            dr = pcg_stream(int(r[20:21].view(np.uint32)[0]), int(r[21:22].view(np.uint32)[0]))
            M = P.Margin()
            ls = P.sample_light(S, light, widen(r[15:18]), dr, M)
            ok, rel = _within(np.array(ls.normal + ls.emission + ls.direction + (ls.dist, ls.pdf)), got[k, :11], M.m)
            assert ok, ("sample_light", k, r.tolist(), got[k, :11], rel)
    finally:
        tr.close()
