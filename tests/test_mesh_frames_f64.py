"""The float64 restatement of a launch of several samples (tests/mesh_frames_f64.py: frame_f64) on its own, CPU only: the draws
tests/test_gpu_mesh_frames_f64.py holds the device to, their near-tie counts, what the planted faults move, and the other side.

Draws.  Nine cases: A .. H, the emission-mapped scene stack (mesh_emap_f64.scene(), EmapMeshDescScene / EmapPath under
mesh_mmap_f64.material_maps(), mesh_emap_f64.emission_maps() and test_gpu_mesh_compose_f64.inputs(s, case): forms 20 .. 27), and
"flat", through test_gpu_mesh_f64's MeshDescScene and pt_f64.sample_many (form 11) — on test_gpu_mesh_compose_f64's scene with
nothing set, not on test_gpu_mesh_f64's own: those sit at 10 to 14 % near ties per SAMPLE (127 of 1 200 in its file, a mirror-like
icosphere and a clearcoat torus of 2 304 triangles), which puts about 40 of 200 two-sample pixels at or below TAU whatever the
generator's key, and coarser meshes of the same builder no lower (measured: 29 to 70 of 200).  Per case 200 random pixels at
64 x 48 and then 200 at 50 x 37 (which fills no tile in either direction), both from ONE np.random.default_rng([55, ord(case)]) — "f"
for the flat case — the columns before the rows; seed 501; frames 0, 1, 2, 3, 5 and 1000.

The near-tie condition (test_the_near_tie_counts_of_the_restatement: a cap that keeps the GPU comparison from hiding a failure, not a
measurement).  By the restatement alone, for exactly those draws: per frame at most NEAR_TIE_MAX (24 of 200) of the samples at or
below TAU; for a two-sample launch — frames 0-1 from a fresh buffer, frames 1-2 on top of one earlier frame — at most 24 of 200
pixels with either sample at or below TAU; in every frame more than a quarter of the samples with radiance.  COUNTS pins every figure,
printed and counted again on every run.  Of 200, 64 x 48 / 50 x 37:

  case   frames 0-1   frames 1-2   largest single frame (0, 1, 2, 3, 5, 1000)   fewest lit
    A         13 / 15      20 / 12      15 /  9                                      126 / 118
    B          9 / 13       8 / 10       7 /  8                                      196 / 196
    C         16 / 21      16 / 19      11 / 17                                      121 / 124
    D         13 / 14      19 / 12      15 /  9                                      198 / 199
    E         13 / 19      11 / 17       8 / 13                                      115 / 114
    F         15 / 10      13 / 10      11 /  6                                      197 / 197
    G         20 / 23      19 / 20      14 / 16                                      133 / 129
    H          7 / 16       8 / 10       7 / 12                                      197 / 199
    flat       8 /  6       5 /  7       6 /  5                                      105 /  99
Every entry is under 24; G at 50 x 37 is close.

One case's draws had to be changed: C draws from default_rng([55, ord("C"), 1]), the first other key tried, because under
[55, ord("C")] 25 of its 200 two-sample pixels at 50 x 37 lie at or below TAU (KEYS).  Pixels with any of four samples near a tie pass
the cap on these draws (A 27, C 27 / 37, D 25, E 33 at 50 x 37, F 28, G 29 / 33; with three samples C 28 and G 27 at 50 x 37), which is
why the direct comparison of a mean stops at two samples; larger launches are reached through bit equality
(test_gpu_mesh_frames_f64.py, test_one_launch_is_its_one_sample_launches).

Mutations (test_the_restatement_sees_each_fault).  Each of frame_f64's planted faults moves more than 10 clean pixels beyond REL_CLEAN
on the two-sample mean that exercises it, over test_gpu_mesh_compose_f64's GRID of 552 pixels at seed 7 — MOVED, counted again on
every run:
  frame_ignored             case A, frames_done = 0   300   every sample draws frame 0's stream
  weight_off_by_one         case A, frames_done = 0   300   v = 1 / frame, and 1 at frame 0
  key_without_frames_done   case B, frames_done = 1   273   sample s draws stream s (test_a_fault_in_the_key_needs_earlier_frames: from
                                                            frames_done = 0 it changes nothing)
A device with one of them would fail the GPU comparison.

The other side (test_one_sample_from_a_fresh_buffer_is_the_sample): frame_f64(frames_done=0, n=1) is sample_pixels' sample and margin
bit for bit with alpha exactly 1, and a launch of three samples is a launch of one and a launch of two on top of it, bit for bit.

The spreads (tests/f32_spread.py), at 64 x 48.  noisy_samples restates the first 150 clean samples of a frame in eight noisy runs,
once; sample_spreads and launch_spreads turn them into the tolerances the GPU file's comparisons (a), (c) and (e) use.
test_the_spreads_of_the_restatement holds the conditions per case and comparison — at least 100 clean samples or pixels with a
spread (139 to 150), at most 5 % of them with a tolerance above 1e-3 (at most 2.1 %: case G, whose frame 1 has two samples of spread
0.3 and 0.6) — and the near-tie cap of the launch at depth (DEEP_NEAR; case G launches from 998, deep_of).  The noisy runs of a
case's six frames take 10 to 18 s of CPU time.  test_the_spreads_see_a_weight_one_frame_off_at_depth: v = 1 / (f + 2) from frame
500 on moves case A's frame 1000 by a part in a thousand — no clean sample beyond REL_CLEAN, 94 of 150 beyond their own tolerance.
test_the_blend_keeps_its_bits_with_the_noise_mode_off: frame_f64's blend is the plain float64 running mean bit for bit, and moves
under the noise.

The tolerances are test_path_f64's TAU / REL_CLEAN / NEAR_TIE_MAX (and Z_MAX / Z_MEDIAN): this file has none of its own.  Measured on the CPU: 1.5 ms per
sample of cases A .. H, 1.2 ms of the flat case; one size of a case, 1 200 samples, takes 1.5 to 2.2 s, a mutation's passes over the
grid 1.7 to 2.4 s, this file 37 s."""
import functools
import time

import numpy as np
import pytest

import f32_spread as S
import mesh_emap_f64 as ME
import mesh_mmap_f64 as MM
import pt_f64 as P
from mesh_compose_f64 import sample_pixels
from mesh_frames_f64 import frame_f64
from test_gpu_mesh_compose_f64 import CASES, GRID, inputs
from test_path_f64 import NEAR_TIE_MAX, REL_CLEAN, TAU, rel_distance

SIZES = ((64, 48), (50, 37))
SEED = 501
FRAMES = (0, 1, 2, 3, 5, 1000)
LAUNCHES = ((0, 1), (1, 2))                                          # the frames of the two-sample launches compared on the device
FLAT = "flat"
ALL_CASES = sorted(CASES) + [FLAT]
N = 200
KEYS = {"C": [55, ord("C"), 1]}                                      # the generator's key where it is not [55, ord(case)]: see the docstring
# (case, width) -> (samples at or below TAU per frame of FRAMES, samples with radiance per frame, pixels with either sample at or below
# TAU per launch of LAUNCHES); test_the_near_tie_counts_of_the_restatement prints them
COUNTS = {
    ("A", 64): ((7, 8, 15, 7, 13, 7), (130, 126, 127, 126, 129, 132), (13, 20)),
    ("A", 50): ((8, 9, 4, 7, 8, 8), (127, 118, 120, 123, 126, 118), (15, 12)),
    ("B", 64): ((7, 2, 6, 2, 3, 7), (200, 200, 200, 196, 200, 199), (9, 8)),
    ("B", 50): ((8, 5, 5, 5, 2, 3), (200, 198, 198, 196, 199, 199), (13, 10)),
    ("C", 64): ((10, 8, 8, 11, 7, 8), (125, 121, 132, 128, 122, 127), (16, 16)),
    ("C", 50): ((11, 12, 12, 17, 12, 11), (130, 126, 128, 126, 128, 124), (21, 19)),
    ("D", 64): ((7, 8, 15, 4, 8, 9), (199, 200, 198, 200, 200, 200), (13, 19)),
    ("D", 50): ((6, 8, 5, 7, 9, 6), (200, 199, 200, 199, 200, 199), (14, 12)),
    ("E", 64): ((8, 6, 5, 5, 6, 4), (122, 126, 126, 124, 115, 127), (13, 11)),
    ("E", 50): ((11, 10, 7, 13, 10, 10), (121, 119, 120, 114, 119, 114), (19, 17)),
    ("F", 64): ((11, 4, 10, 6, 4, 5), (197, 200, 199, 199, 199, 198), (15, 13)),
    ("F", 50): ((5, 6, 4, 4, 5, 3), (200, 199, 199, 198, 200, 197), (10, 10)),
    ("G", 64): ((11, 12, 9, 12, 11, 14), (138, 139, 133, 135, 137, 134), (20, 19)),
    ("G", 50): ((14, 13, 11, 10, 10, 16), (135, 130, 130, 129, 136, 135), (23, 20)),
    ("H", 64): ((5, 3, 6, 5, 7, 3), (198, 200, 197, 199, 200, 200), (7, 8)),
    ("H", 50): ((12, 5, 6, 9, 4, 5), (199, 199, 199, 199, 200, 199), (16, 10)),
    (FLAT, 64): ((6, 3, 2, 3, 3, 4), (110, 118, 113, 115, 105, 113), (8, 5)),
    (FLAT, 50): ((1, 5, 2, 3, 2, 2), (102, 105, 100, 101, 102, 99), (6, 7)),
}
# case -> pixels of the two-sample launch at depth with either sample at or below TAU; test_the_spreads_of_the_restatement prints them
DEEP_NEAR = {"A": 14, "B": 11, "C": 16, "D": 11, "E": 9, "F": 14, "G": 18, "H": 9, FLAT: 5}
# fault -> (case, frames_done, clean pixels moved beyond REL_CLEAN); test_the_restatement_sees_each_fault prints them
MOVED = {"frame_ignored": ("A", 0, 300), "weight_off_by_one": ("A", 0, 300), "key_without_frames_done": ("B", 1, 273)}


@functools.lru_cache(maxsize=None)
def draws(case):
    """{(w, h): 200 pixels}: the first size's, then the second's, from one generator."""
    rng = np.random.default_rng(KEYS.get(case, [55, ord(case[0])]))
    return {(w, h): list(zip(rng.integers(0, w, N).tolist(), rng.integers(0, h, N).tolist())) for w, h in SIZES}


@functools.lru_cache(maxsize=None)
def flat_scene():
    from test_gpu_mesh_compose_f64 import _scene
    from test_gpu_mesh_f64 import MeshDescScene
    s = _scene()
    return s, MeshDescScene(s.describe(), s)


@functools.lru_cache(maxsize=None)
def path_of(case):
    s = ME.scene()
    sc = ME.EmapMeshDescScene(s.describe(), s, emission_maps=ME.emission_maps(), material_maps=MM.material_maps(), **inputs(s, case))
    return ME.EmapPath(sc)


def sample_frame_of(oracle, case, seed, pixels, w, h):
    """-> f(frame) -> (radiance [p, 3], margins [p]): the case's restatement of one sample of each pixel."""
    if case == FLAT:
        return lambda f: P.sample_many(flat_scene()[1], oracle, seed, [(c, r, f) for c, r in pixels], w, h)[:2]
    return lambda f: sample_pixels(path_of(case), oracle, seed, pixels, w, h, frame=f)


@functools.lru_cache(maxsize=None)
def restated(oracle, case, size, frame):
    """The restated samples of the case's draws at one size and frame, computed once for every test that needs them, CPU or GPU:
    (radiance [200, 3], margins [200]).  Nobody writes to them."""
    w, h = size
    rad, marg = sample_frame_of(oracle, case, SEED, draws(case)[size], w, h)(frame)
    rad.setflags(write=False)
    marg.setflags(write=False)
    return rad, marg


def launch_f64(oracle, case, size, frames_done, n, acc=None):
    """frame_f64 over restated()'s samples."""
    w, h = size
    return frame_f64(None, oracle, SEED, draws(case)[size], w, h, frames_done, n, acc=acc,
                     sample_frame=lambda f: restated(oracle, case, size, f))


# ---- the samples' and the launches' own f32 tolerances (tests/f32_spread.py), at 64 x 48 ------------------------------------------------
DEEP = 1000                                                          # frames_done of the two-sample launch at depth


def deep_of(case):
    """frames_done of the case's two-sample launch at depth: 1000, but 998 for G, 26 of whose 200 pixels have frame 1000 or 1001 at
    or below TAU (the cap is 24; 25 from 999, 22 from 1001, 18 from 998).  Its mean over a zeroed accumulator times frames_done + 2
    is the sum of the two samples, but for a part in a thousand."""
    return 998 if case == "G" else DEEP


@functools.lru_cache(maxsize=None)
def noisy_samples(oracle, case, size, frame):
    """The first MIN_CLEAN clean samples of restated(oracle, case, size, frame) restated again in f32_spread.RUNS noisy runs, once
    for every comparison that needs them, CPU or GPU -> (their indices, radiance [RUNS, n, 3] blended as black, CPU seconds)."""
    w, h = size
    idx = S.first_clean(restated(oracle, case, size, frame)[1], S.MIN_CLEAN)
    sf = sample_frame_of(oracle, case, SEED, [draws(case)[size][i] for i in idx], w, h)
    t0 = time.process_time()
    runs = []
    for run in range(S.RUNS):
        with P.perturbed(0, run):
            runs.append(S._radiance(sf(frame)[0]))
    out = np.stack(runs)
    out.setflags(write=False)
    return idx, out, time.process_time() - t0


def sample_spreads(oracle, case, size, frame):
    """The spreads of the frame's first MIN_CLEAN clean samples, NaN elsewhere: [N]."""
    idx, runs, _ = noisy_samples(oracle, case, size, frame)
    plain = S._radiance(restated(oracle, case, size, frame)[0])[idx]
    return S.subset_spreads(N, idx, np.max([rel_distance(plain, r) for r in runs], axis=0))


def launch_spreads(oracle, case, size, frames_done, n, acc=None, scale=1.0):
    """The spreads of a launch's means (times `scale`), for the pixels every one of whose samples has noisy runs, NaN elsewhere: the
    noisy samples of each run through frame_f64's noisy blend, against launch_f64's plain mean.  acc: the accumulator before the
    launch, as launch_f64 takes it; it is an input and carries no noise."""
    w, h = size
    frames = range(frames_done, frames_done + n)
    idx = functools.reduce(np.intersect1d, [noisy_samples(oracle, case, size, f)[0] for f in frames])
    at = {f: np.searchsorted(noisy_samples(oracle, case, size, f)[0], idx) for f in frames}
    pixels = [draws(case)[size][i] for i in idx]
    sub = None if acc is None else np.asarray(acc, np.float64)[idx]
    plain = launch_f64(oracle, case, size, frames_done, n, acc=acc)[0][idx, :3] * scale
    out = np.zeros(len(idx))
    for run in range(S.RUNS):
        with P.perturbed(0, run):
            P.noise_begin(SEED, frames_done, n)
            sf = lambda f: (noisy_samples(oracle, case, size, f)[1][run][at[f]], restated(oracle, case, size, f)[1][idx])      # noqa: E731
            mean = frame_f64(None, oracle, SEED, pixels, w, h, frames_done, n, acc=sub, sample_frame=sf)[0]
        out = np.maximum(out, rel_distance(plain, mean[:, :3] * scale))
    return S.subset_spreads(N, idx, out)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("case", ALL_CASES)
def test_the_near_tie_counts_of_the_restatement(rpt, oracle, case, size):
    cap = NEAR_TIE_MAX * N
    below = tuple(int((restated(oracle, case, size, f)[1] <= TAU).sum()) for f in FRAMES)
    lit = tuple(int(np.nan_to_num(restated(oracle, case, size, f)[0]).any(axis=1).sum()) for f in FRAMES)
    pairs = tuple(int(((restated(oracle, case, size, a)[1] <= TAU) | (restated(oracle, case, size, b)[1] <= TAU)).sum()) for a, b in LAUNCHES)
    more = tuple(int((np.min([restated(oracle, case, size, f)[1] for f in range(k)], axis=0) <= TAU).sum()) for k in (3, 4))
    print("COUNTS[(%r, %d)] = (%s, %s, %s)    # three / four samples: %s" % (case, size[0], below, lit, pairs, more))
    assert len(draws(case)[size]) == N and cap == 24
    assert max(below) <= cap and max(pairs) <= cap
    assert min(lit) > N // 4
    for a, b in LAUNCHES:                                             # the margin frame_f64 hands the comparison is the samples' smallest
        _, margins, _ = launch_f64(oracle, case, size, a, 2)
        assert int((margins <= TAU).sum()) == pairs[LAUNCHES.index((a, b))]
    assert (below, lit, pairs) == COUNTS[(case, size[0])]


@functools.lru_cache(maxsize=None)
def _grid_samples(oracle, case, frame):
    return sample_pixels(path_of(case), oracle, 7, GRID, 64, 48, frame=frame)


@pytest.mark.parametrize("fault", sorted(MOVED))
def test_the_restatement_sees_each_fault(rpt, oracle, fault):
    case, frames_done, count = MOVED[fault]
    launch = lambda **kw: frame_f64(None, oracle, 7, GRID, 64, 48, frames_done, 2,          # noqa: E731
                                    sample_frame=lambda f: _grid_samples(oracle, case, f), **kw)
    base, marg, _ = launch()
    moved, marg2, _ = launch(**{fault: True})
    far = (rel_distance(moved[:, :3], base[:, :3]) > REL_CLEAN) & (marg > TAU) & (marg2 > TAU)
    print("%s (case %s, two samples from frames_done = %d): %d clean pixels beyond REL_CLEAN" % (fault, case, frames_done, int(far.sum())))
    assert len(GRID) == 552
    assert far.sum() > 10
    assert int(far.sum()) == count


def test_a_fault_in_the_key_needs_earlier_frames(rpt, oracle):
    """key_without_frames_done changes nothing from frames_done = 0: why its comparison starts from one earlier frame."""
    pixels = GRID[::6]
    sf = lambda f: tuple(x[::6] for x in _grid_samples(oracle, "B", f))                      # noqa: E731
    base = frame_f64(None, oracle, 7, pixels, 64, 48, 0, 2, sample_frame=sf)
    same = frame_f64(None, oracle, 7, pixels, 64, 48, 0, 2, sample_frame=sf, key_without_frames_done=True)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(base, same))


@pytest.mark.parametrize("case", ["A", "H", FLAT])
def test_one_sample_from_a_fresh_buffer_is_the_sample(rpt, oracle, case):
    pixels = GRID[::6]
    sf = sample_frame_of(oracle, case, 9, pixels, 64, 48)
    want, margins = sf(0)
    path = None if case == FLAT else path_of(case)
    mean, marg, samples = frame_f64(path, oracle, 9, pixels, 64, 48, 0, 1, sample_frame=sf if case == FLAT else None)
    assert np.array_equal(mean[:, :3], np.where(np.isfinite(want).all(axis=1, keepdims=True), want, 0.0)) and np.nan_to_num(want).any()
    assert np.array_equal(samples[:, 0], want, equal_nan=True) and np.array_equal(marg, margins)
    assert (mean[:, 3] == 1.0).all()
    # three samples are one sample and two on top of it
    whole = frame_f64(path, oracle, 9, pixels, 64, 48, 0, 3, sample_frame=sf)
    rest = frame_f64(path, oracle, 9, pixels, 64, 48, 1, 2, acc=mean, sample_frame=sf)
    assert np.array_equal(whole[0], rest[0]) and np.array_equal(whole[1], np.minimum(marg, rest[1]))
    assert np.array_equal(whole[2][:, 1:], rest[2]) and not np.array_equal(whole[2][:, 0], whole[2][:, 1], equal_nan=True)


# ---- the spreads: conditions, teeth, and the blend's bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES)
def test_the_spreads_of_the_restatement(rpt, oracle, case):
    """The conditions of the GPU file's comparisons with spreads (64 x 48), on the restatement alone: in each of them at least 100
    clean samples or pixels have a spread and at most 5 % of those a tolerance above 1e-3 — the later frames of (a), the two
    launches of (c) (the second on top of the restated first frame, where the device test has the device's) and the launch at
    depth, whose near ties stay under the cap as well (DEEP_NEAR pins the count)."""
    size = SIZES[0]
    seconds = 0.0
    for k in (1, 5, DEEP):
        S.case_conditions("case %s, frame %d" % (case, k), [(None, None, None, restated(oracle, case, size, k)[1])], [sample_spreads(oracle, case, size, k)])
    for frames_done, _ in LAUNCHES:
        acc = launch_f64(oracle, case, size, 0, frames_done)[0] if frames_done else None
        _, margins, _ = launch_f64(oracle, case, size, frames_done, 2, acc=acc)
        S.case_conditions("case %s, two samples on %d earlier" % (case, frames_done), [(None, None, None, margins)],
                          [launch_spreads(oracle, case, size, frames_done, 2, acc=acc)])
    deep = deep_of(case)
    _, margins, _ = launch_f64(oracle, case, size, deep, 2)
    near = int((margins <= TAU).sum())
    print("DEEP_NEAR[%r] = %d" % (case, near))
    S.case_conditions("case %s, two samples on %d earlier" % (case, deep), [(None, None, None, margins)],
                      [launch_spreads(oracle, case, size, deep, 2, scale=float(deep + 2))])
    frames = sorted({0, 1, 2, 5, DEEP, deep, deep + 1})
    for f in frames:
        seconds += noisy_samples(oracle, case, size, f)[2]
    print("case %s: the noisy runs of %d frames took %.2f s of CPU time" % (case, len(frames), seconds))
    assert near <= NEAR_TIE_MAX * N and near == DEEP_NEAR[case]


def test_the_spreads_see_a_weight_one_frame_off_at_depth(rpt, oracle):
    """v = 1 / (f + 2) from frame 500 on, rounded to f32, as a device's frame 1000 of case A scaled as the GPU comparison (a) scales
    it: a part in a thousand, within REL_CLEAN on every clean sample — the blind spot that comparison had — and beyond their own
    tolerance on at least 10.  At frame 5 the fault is not there and nothing moves."""
    size = SIZES[0]
    pixels = draws("A")[size]
    for k, sees in ((DEEP, True), (5, False)):
        rad, marg = restated(oracle, "A", size, k)
        mean = frame_f64(None, oracle, SEED, pixels, 64, 48, k, 1, sample_frame=lambda f: restated(oracle, "A", size, f), weight_late_from=500)[0]
        entries, spreads, faulty = [(SEED, pixels, rad, marg)], [sample_spreads(oracle, "A", size, k)], [(mean[:, :3] * float(k + 1), marg)]
        if sees:
            S.teeth("v = 1 / (f + 2) from frame 500 (case A, frame %d)" % k, entries, spreads, faulty)
        else:
            assert np.array_equal(faulty[0][0], S._radiance(rad) * (1.0 / (k + 1)) * float(k + 1))


def test_the_blend_keeps_its_bits_with_the_noise_mode_off(rpt, oracle):
    """frame_f64's blend with the noise mode off is the plain float64 running mean, bit for bit; with it on, it moves."""
    pixels = GRID[::6]
    sf = sample_frame_of(oracle, FLAT, 9, pixels, 64, 48)
    samples = {f: sf(f) for f in (DEEP, DEEP + 1, DEEP + 2)}
    acc = np.random.default_rng(5).uniform(0.0, 2.0, (len(pixels), 4))
    want = acc.copy()
    for f in sorted(samples):
        v = 1.0 / (f + 1)
        c = np.concatenate([np.nan_to_num(samples[f][0]), np.ones((len(pixels), 1))], axis=1)
        want = (1.0 - v) * want + c * v
    assert np.isfinite(np.concatenate([r for r, _ in samples.values()])).all()
    got = frame_f64(None, oracle, 9, pixels, 64, 48, DEEP, 3, acc=acc, sample_frame=lambda f: samples[f])[0]
    assert np.array_equal(got, want)
    with P.perturbed(0, 0):
        moved = frame_f64(None, oracle, 9, pixels, 64, 48, DEEP, 3, acc=acc, sample_frame=lambda f: samples[f])[0]
    assert not np.array_equal(moved, want) and np.abs(moved / want - 1.0).max() < 16 * P.NOISE_EPS
