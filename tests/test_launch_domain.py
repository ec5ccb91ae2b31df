"""The ends of the launch domain on the CPU: what a 64-bit frames_done, a 64-bit seed and the frame's weight are held to before
tests/test_gpu_launch_domain.py holds the device to the oracle there.  Needs no GPU.

The key.  frame_key (oracle/rpt_oracle.hpp, csrc/dev_scene.h frame_key_hd) folds seed >> 32, seed, frame >> 32 and frame, in that
order, twice (the second chain starts from the seed's high word xor 0x85EBCA6B); Rng::init hashes the pixel index into both.  Both
are restated here in Python integers from that text and oracle.rng_u32 is held to the restatement over every combination of zero and
non-zero high and low words of seed and frame (KEYS), at pixels 0 and 2^32 - 1.  tests/test_oracle_kat.py does this for frame 0 and
seed 1 alone, where both high words and the frame's low word fold in as zeros.

The weight.  The blend's v is 1 / f32(frames + 1): a u64 -> f32 conversion, exact below 2^24 and rounded to nearest even from there
on (2^24 + 1 is a tie).  f32_of is that rounding in integer arithmetic on the exact Python integer — never through a Python float,
which would round twice (2^53 + 1 + 2^29, say).  The oracle's multi-sample render (compiled by the host compiler, whose conversion
is therefore held to the integer rounding here) equals oracle.sample_pixels per frame blended with those weights in numpy float32,
word for word, at 1 x 1 and 5 x 3 from zeroed and 0.37-filled buffers, from every start of STARTS.

The float64 restatement at depth.  tests/test_gpu_launch_domain.py compares two-sample mesh launches from DEEP_STARTS with frame_f64
through Tally; the condition that keeps that comparison from hiding a failure is counted here, on every run, by the restatement
alone: of test_mesh_frames_f64's 200 draws at 64 x 48, the pixels with either sample at or below TAU stay under NEAR_TIE_MAX (24):
                    from 2^24 - 1   2^32 - 1   2^64 - 4        lit samples, fewest
    flat                  4            3          3             113
    B                     9           10          6             196
(case G gives 20 / 20 / 20, too near the cap, and is not used.)  DEEP_COUNTS pins them.

Planted faults.  frame_f64's frame_ignored and key_without_frames_done, and one more, frame_low_word_only (the key taken from
frame & 0xFFFFFFFF: a counter truncated to 32 bits anywhere between the caller and the kernel), on case B's two-sample launch from
frames_done = 2^32 - 1 over test_gpu_mesh_compose_f64's GRID at seed 7: each moves more than 10 clean pixels beyond REL_CLEAN
on the mean times frames_done + 2, as the GPU comparison scales both sides (DEEP_MOVED: 333, 318 and 270 of 552).
frame_low_word_only changes the launch's second sample alone: frame 2^32 draws frame 0's stream.

The tolerances are test_path_f64's TAU / REL_CLEAN / NEAR_TIE_MAX: this file has none of its own.  Measured on the CPU: the key
0.1 s, the blends 1 s, a case and start of the counts about 0.8 s, a fault about 2 s."""
import functools

import numpy as np
import pytest

import test_mesh_frames_f64 as TF
from kernel_census import render_kernels
from mesh_frames_f64 import frame_f64
from test_gpu_mesh_compose_f64 import GRID
from test_path_f64 import NEAR_TIE_MAX, REL_CLEAN, TAU, rel_distance

M32 = 0xFFFFFFFF
BIG_SEED = 0xDEADBEEF12345
# frames_done of the oracle's blends: both sides of 2^24 (where the weight's conversion starts to round), of 2^32 (the key's high word),
# a tie beyond a double's integers, the top bit, and the last start four samples fit behind
STARTS = (0, 2 ** 24 - 2, 2 ** 24, 2 ** 25 + 1, 2 ** 32 - 2, 2 ** 32 + 5, 2 ** 53 + 1, 2 ** 63, 2 ** 64 - 6)
# (seed, frame): every combination of a zero and a non-zero high and low word of either
SEEDS = (0, 1, 2 ** 32, 2 ** 32 + 1, BIG_SEED, 2 ** 64 - 1)
FRAMES = (0, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 63, 2 ** 64 - 1)
KEYS = tuple((s, f) for s in SEEDS for f in FRAMES)
PIXELS = (0, 2 ** 32 - 1)
# the starts of the two-sample mesh launches, and case -> pixels with either sample at or below TAU per start, fewest lit samples
DEEP_STARTS = (2 ** 24 - 1, 2 ** 32 - 1, 2 ** 64 - 4)
DEEP_CASES = (TF.FLAT, "B")
DEEP_COUNTS = {TF.FLAT: ((4, 3, 3), 113), "B": ((9, 10, 6), 196)}
# fault -> clean pixels moved beyond REL_CLEAN: case B, two samples from frames_done = 2^32 - 1
DEEP_FAULT_START = 2 ** 32 - 1
DEEP_MOVED = {"frame_ignored": 333, "key_without_frames_done": 318, "frame_low_word_only": 270}


# ---- the key -------------------------------------------------------------------------------------------------------------------------
def pcg(v):
    """pcg_hash (Jarzynski & Olano 2020), as oracle/rpt_oracle.hpp and csrc/dev_scene.h spell it."""
    state = (v * 747796405 + 2891336453) & M32
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & M32
    return ((word >> 22) ^ word) & M32


def frame_key(seed, frame):
    k = pcg((seed >> 32) & M32)
    k = pcg(k ^ (seed & M32))
    k = pcg(k ^ ((frame >> 32) & M32))
    k0 = pcg(k ^ (frame & M32))
    j = pcg(((seed >> 32) & M32) ^ 0x85EBCA6B)
    j = pcg(j ^ (seed & M32))
    j = pcg(j ^ ((frame >> 32) & M32))
    k1 = pcg(j ^ (frame & M32))
    return k0, k1


def stream(seed, frame, pixel, n):
    """The first n draws of Rng::init(frame_key(seed, frame), pixel): PCG-RXS-M-XS-32 with the path's own increment."""
    k0, k1 = frame_key(seed, frame)
    a = pcg(pixel)
    b = pcg(a)
    state, inc = pcg(a ^ k0), pcg(b ^ k1) | 1
    out = []
    for _ in range(n):
        state = (state * 747796405 + inc) & M32
        word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & M32
        out.append(((word >> 22) ^ word) & M32)
    return out


def test_the_key_list_has_every_combination_of_words():
    words = lambda x: (bool(x >> 32), bool(x & M32))                  # noqa: E731
    assert {words(s) + words(f) for s, f in KEYS} == {(a, b, c, d) for a in (False, True) for b in (False, True) for c in (False, True) for d in (False, True)}
    assert {2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 63, 2 ** 64 - 1} <= set(FRAMES) and {1, 2 ** 32 + 1, 2 ** 64 - 1} <= set(SEEDS)


def test_the_oracle_s_stream_is_the_restated_key_and_generator(oracle):
    for seed, frame in KEYS:
        for pixel in PIXELS:
            got = oracle.rng_u32(seed, frame, pixel, 16)
            assert [int(x) for x in got] == stream(seed, frame, pixel, 16), "seed %#x, frame %#x, pixel %#x" % (seed, frame, pixel)
            f = oracle.rng_f32(seed, frame, pixel, 16)
            assert np.array_equal(f, (got >> 8).astype(np.float32) * np.float32(2.0 ** -24))


def test_the_high_words_select_other_streams(oracle):
    """Frame 5 and frame 2^32 + 5 differ in the frame's high word alone, seed 1 and seed 2^32 + 1 in the seed's."""
    a, b, c = (tuple(oracle.rng_u32(s, f, 0, 16).tolist()) for s, f in ((1, 5), (1, 2 ** 32 + 5), (2 ** 32 + 1, 5)))
    assert len({a, b, c}) == 3
    assert not set(a) & set(b) and not set(a) & set(c) and not set(b) & set(c), "no draw in common"


# ---- the weight ----------------------------------------------------------------------------------------------------------------------
def f32_of(n):
    """The float32 nearest to the integer n >= 0, ties to even, in integer arithmetic: what `as f32` and a conforming (float) give."""
    bits = n.bit_length()
    if bits <= 24:
        return np.float32(n)
    shift = bits - 24
    m, rem, half = n >> shift, n & ((1 << shift) - 1), 1 << (shift - 1)
    if rem > half or (rem == half and m & 1):
        m += 1
    out = np.float32(np.ldexp(float(m), shift))                       # m <= 2^24 and a power of two: exact in both formats
    assert int(out) == m << shift
    return out


def weight(frame):
    """v of frame `frame`: 1 / f32(frame + 1), the division rounded once."""
    return np.float32(1.0) / f32_of(frame + 1)


def test_the_integer_rounding():
    assert f32_of(2 ** 24) == 2.0 ** 24 and f32_of(2 ** 24 - 1) == 2.0 ** 24 - 1
    assert f32_of(2 ** 24 + 1) == 2.0 ** 24, "a tie: to even, down"
    assert f32_of(2 ** 24 + 3) == 2.0 ** 24 + 4, "a tie: to even, up"
    assert f32_of(2 ** 25 + 2) == 2.0 ** 25 and f32_of(2 ** 25 + 3) == 2.0 ** 25 + 4
    assert f32_of(2 ** 64 - 1) == 2.0 ** 64 and f32_of(2 ** 32 - 1) == 2.0 ** 32
    n = 2 ** 53 + 2 ** 29 + 1                                        # through a double this rounds twice: first onto the tie, then down
    assert f32_of(n) == 2.0 ** 53 + 2.0 ** 30 and np.float32(float(n)) == 2.0 ** 53
    rng = np.random.default_rng(3)
    for bits in range(25, 54):                                       # below 2^53 a double holds n exactly and numpy rounds it once
        for n in rng.integers(2 ** (bits - 1), 2 ** bits, 50).tolist():
            assert f32_of(n) == np.float32(n)


def blend(samples, frames_done, acc):
    """acc [p, 4] f32 after samples[s] [p, 3] enter it as frames frames_done + s: tracer.rs:105-117 in numpy float32, every operation
    rounded once, a sample that is not finite blended as black."""
    one = np.float32(1.0)
    acc = acc.astype(np.float32).copy()
    for s, rad in enumerate(samples):
        v = weight(frames_done + s)
        rad = np.where(np.isfinite(rad).all(axis=1, keepdims=True), rad, np.float32(0.0)).astype(np.float32)
        color = np.concatenate([rad, np.ones((len(rad), 1), np.float32)], axis=1)
        acc = (((one - v) * acc).astype(np.float32) + (color * v).astype(np.float32)).astype(np.float32)
    return acc


@pytest.mark.parametrize("fill", [0.0, 0.37], ids=["zeroed", "filled"])
@pytest.mark.parametrize("size", [(1, 1), (5, 3)], ids=["1x1", "5x3"])
def test_the_oracle_s_render_is_its_samples_blended_with_the_rounded_weights(oracle, size, fill):
    w, h = size
    spp = 4
    desc = oracle.scene_analytical()
    rows, cols = (a.reshape(-1) for a in np.divmod(np.arange(w * h), w))
    for start in STARTS:
        assert start + spp <= 2 ** 64 - 1
        samples = [oracle.sample_pixels(desc, cols, rows, np.full(w * h, start + s, np.uint64), w, h, seed=BIG_SEED) for s in range(spp)]
        want = blend(samples, start, np.full((w * h, 4), fill, np.float32))
        got = oracle.render(desc, w, h, spp, seed=BIG_SEED, frames_done=start, pixels=np.full((h, w, 4), fill, np.float32)).reshape(w * h, 4)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%d x %d from %d: %s against %s" % (w, h, start, got[0], want[0])
        assert got[:, :3].view(np.uint32).any() and got[:, 3].view(np.uint32).all() and np.isfinite(got).all()


# ---- the float64 restatement at depth ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DEEP_CASES)
def test_the_near_tie_counts_at_depth(rpt, oracle, case):
    size = TF.SIZES[0]
    cap = NEAR_TIE_MAX * TF.N
    near, lit = [], []
    for start in DEEP_STARTS:
        a, b = TF.restated(oracle, case, size, start), TF.restated(oracle, case, size, start + 1)
        near.append(int(((a[1] <= TAU) | (b[1] <= TAU)).sum()))
        lit += [int(np.nan_to_num(x[0]).any(axis=1).sum()) for x in (a, b)]
        _, margins, _ = TF.launch_f64(oracle, case, size, start, 2)
        assert int((margins <= TAU).sum()) == near[-1], "the margin frame_f64 hands the comparison is the samples' smallest"
    print("DEEP_COUNTS[%r] = (%s, %d)    # lit per frame: %s" % (case, tuple(near), min(lit), lit))
    assert cap == 24 and max(near) <= cap and min(lit) > TF.N // 4
    assert (tuple(near), min(lit)) == DEEP_COUNTS[case]


@functools.lru_cache(maxsize=None)
def _grid_samples(oracle, frame):
    return TF.sample_pixels(TF.path_of("B"), oracle, 7, GRID, 64, 48, frame=frame)


@pytest.mark.parametrize("fault", sorted(DEEP_MOVED))
def test_the_restatement_sees_each_fault_at_depth(rpt, oracle, fault):
    launch = lambda **kw: frame_f64(None, oracle, 7, GRID, 64, 48, DEEP_FAULT_START, 2,     # noqa: E731
                                    sample_frame=lambda f: _grid_samples(oracle, f), **kw)
    base, marg, _ = launch()
    moved, marg2, _ = launch(**{fault: True})
    scale = float(DEEP_FAULT_START + 2)                               # as the GPU comparison scales both sides: the sum of the two samples
    far = (rel_distance(moved[:, :3] * scale, base[:, :3] * scale) > REL_CLEAN) & (marg > TAU) & (marg2 > TAU)
    print("DEEP_MOVED[%r] = %d    # case B, two samples from frames_done = 2^32 - 1" % (fault, int(far.sum())))
    assert len(GRID) == 552 and far.sum() > 10
    assert int(far.sum()) == DEEP_MOVED[fault]


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------
def test_the_gpu_file_s_kernels_are_the_library_s_strict_kernels(rpt):
    """tests/test_gpu_launch_domain.py's (a) runs one case per strict render_* kernel of the loaded library's gfx950 code object."""
    import test_gpu_launch_domain as G
    from test_gpu_strict_kernels import CASES
    names = render_kernels(rpt._lib.LIB_PATH, relaxed=False)
    assert len(names) == 29 and names == set(CASES) == set(G.KERNELS) == set(G.SIZES)
    assert {G.start_of(k) for k in G.KERNELS} == set(G.STARTS), "the rotation reaches every start"
    classes = {CASES[k][0] + (" media" if "media" in k else "") for k in G.ALL_STARTS}
    assert len(G.ALL_STARTS) == 4 and classes == {"small", "sdf", "large", "small media"}
