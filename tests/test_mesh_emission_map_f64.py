"""The float64 restatement of mesh emission maps (tests/mesh_emap_f64.py) on its own, CPU only: what
tests/test_gpu_mesh_emission_map_f64.py compares the eight emission-mapped kernel forms against.

* The near-tie count of every case's 400 samples stays within the cap the material-map cases observe (48 of 400): BELOW_TAU pins the
  counts, printed again on every run.
* Three planted faults, each counted on case A over test_gpu_mesh_compose_f64's grid of 552 pixels at seed 7 and pinned in MOVED:
  the sampler ignores the map, the sampler looks up at (bv, bu), the hit side ignores the map.  Each moves more than 10 clean samples
  beyond REL_CLEAN: a device with that fault would fail the GPU comparison.
* With all-255 emission maps the subclass gives the material-map restatement's samples bit for bit.

* spreads() computes each case's f32 spreads (tests/f32_spread.py) once, for the GPU comparison and for the conditions held here: at
  least 100 clean samples with a spread, at most 5 % of them with a tolerance above 1e-3 (at most 1.33 %).

The tolerances are test_path_f64's TAU / REL_CLEAN / NEAR_TIE_MAX: this file has none of its own."""
import functools

import numpy as np
import pytest

import f32_spread as S
import mesh_emap_f64 as ME
import mesh_mmap_f64 as MM
from mesh_compose_f64 import ComposedPath, sample_pixels
from test_gpu_mesh_compose_f64 import CASES, GRID, H, W, inputs
from test_path_f64 import REL_CLEAN, TAU, rel_distance

BELOW_TAU_CAP = 48                                                   # of 400: what the material-map cases observe
# test_the_near_tie_count_of_the_restatement prints them
BELOW_TAU = {"A": 20, "B": 16, "C": 12, "D": 15, "E": 17, "F": 12, "G": 22, "H": 21}
# fault -> clean samples moved beyond REL_CLEAN on case A (test_the_restatement_sees_each_fault prints them)
MOVED = {"sampler_ignores_map": 137, "sampler_swaps_uv": 120, "hit_ignores_map": 107}


def draws(case):
    """[(seed, pixels)]: 200 random pixels at each of two seeds, the case's own."""
    k = sorted(CASES).index(case)
    rng = np.random.default_rng([47, k])
    return [(510 + 10 * k + seed, list(zip(rng.integers(0, W, 200).tolist(), rng.integers(0, H, 200).tolist()))) for seed in (1, 2)]


def path_of(s, case, identity=False, scene_faults=None, path_faults=None):
    sc = ME.EmapMeshDescScene(s.describe(), s, emission_maps=ME.emission_maps(identity), material_maps=MM.material_maps(), **(scene_faults or {}),
                              **inputs(s, case))
    return ME.EmapPath(sc, **(path_faults or {}))


@functools.lru_cache(maxsize=None)
def restated(oracle, case):
    """The restatement of the case's draws, computed once for every test that needs it: [(seed, pixels, radiance, margins)]."""
    s = ME.scene()
    path = path_of(s, case)
    return [(seed, pixels) + sample_pixels(path, oracle, seed, pixels, W, H) for seed, pixels in draws(case)]


@functools.lru_cache(maxsize=None)
def spreads(oracle, case):
    """The f32 spreads (tests/f32_spread.py) of the case's first 150 clean samples, computed once beside restated() for the CPU and
    the GPU leg: ([spreads per seed, NaN where there is none], CPU seconds)."""
    return S.spreads_of_draws(path_of(ME.scene(), case), oracle, restated(oracle, case), W, H)


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_spreads_of_the_restatement(rpt, oracle, case):
    """The conditions of the comparison with spreads, on the restatement alone: at least 100 clean samples of the case have a spread,
    and at most 5 % of them a tolerance above 1e-3."""
    spr, seconds = spreads(oracle, case)
    S.case_conditions("case %s" % case, restated(oracle, case), spr, seconds)


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_near_tie_count_of_the_restatement(rpt, oracle, case):
    below = sum(int((margins <= TAU).sum()) for _, _, _, margins in restated(oracle, case))
    lit = sum(int(np.nan_to_num(radiance).any(axis=1).sum()) for _, _, radiance, _ in restated(oracle, case))
    print("case %s: %d of 400 samples at or below TAU, %d carry radiance" % (case, below, lit))
    assert below <= BELOW_TAU_CAP
    assert below == BELOW_TAU[case]
    assert lit > 200


FAULTS = {"sampler_ignores_map": dict(path_faults=dict(sampler_ignores_map=True)),
          "sampler_swaps_uv": dict(path_faults=dict(sampler_swaps_uv=True)),
          "hit_ignores_map": dict(scene_faults=dict(hit_ignores_map=True))}


@functools.lru_cache(maxsize=None)
def _grid_base(oracle):
    return sample_pixels(path_of(ME.scene(), "A"), oracle, 7, GRID, W, H)


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_the_restatement_sees_each_fault(rpt, oracle, fault):
    base, marg = _grid_base(oracle)
    moved, marg2 = sample_pixels(path_of(ME.scene(), "A", **FAULTS[fault]), oracle, 7, GRID, W, H)
    far = (rel_distance(np.nan_to_num(moved), np.nan_to_num(base)) > REL_CLEAN) & (marg > TAU) & (marg2 > TAU)
    print("%s (case A): %d clean samples beyond REL_CLEAN" % (fault, int(far.sum())))
    assert len(GRID) == 552
    assert far.sum() > 10
    assert int(far.sum()) == MOVED[fault]


@pytest.mark.parametrize("case", ["A", "H"])
def test_an_all_255_map_is_the_material_map_restatement(rpt, oracle, case):
    """E exactly 1 at the hit, at the emitter exit and in the sampler: the samples are the material-map restatement's, bit for bit
    (the sampler's normal_of hook returns the very normal the sampler computes itself).  The margins can only narrow: the object's
    NEAREST map adds its texel borders."""
    s = ME.scene()
    args = inputs(s, case)
    pixels = GRID[::6]
    want = sample_pixels(ComposedPath(MM.MmapMeshDescScene(s.describe(), s, material_maps=MM.material_maps(), **args)), oracle, 9, pixels, W, H)
    got = sample_pixels(path_of(s, case, identity=True), oracle, 9, pixels, W, H)
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.nan_to_num(want[0]).any()
    assert (got[1] <= want[1]).all(), "the map's NEAREST lookup can only add margins"
    assert not np.array_equal(sample_pixels(path_of(s, case), oracle, 9, pixels, W, H)[0], want[0], equal_nan=True), "the cases' maps are no identity"
