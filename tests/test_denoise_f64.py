"""The denoiser's specification (include/rpt.h "denoiser") checked by an independent statement of it: the f32 oracle
(oracle/rpt_oracle.hpp, denoise()) against tests/dn_f64.py, a float64 restatement written from the header's text.  CPU only.

- the oracle is within dn_f64's calibrated bound of the restatement, NaN and -inf in the same places, over rendered frames
  and synthetic images, at every iteration count and over edge_k from 1e-6 to 1e3;
- the comparison has teeth: six wrong restatements (k, step, H, border rule, alpha, iteration count) each fail it;
- a finite input pixel never makes another finite input pixel's output non-finite (an input of exactly -1 once did: its
  compressed colour is -inf, and 0 * inf spread NaN over its whole footprint), and fixing that changed no other pixel: the
  oracle's frames of inputs without a -1 are those of the specification before the fix (tests/golden/denoise_before_confinement.json);
- the u8 conversion of the oracle against float64 truncation at every step boundary."""
import hashlib
import json
import os

import numpy as np
import pytest

import dn_f64

HERE = os.path.dirname(os.path.abspath(__file__))
EDGE_KS = (1e-6, 0.5, 2.0, 8.0, 1e3)
# finite values at which a kernel or the specification could go wrong: the pole of c / (1 + c) (-1), its sign changes, the
# saturation of c' = 1 (c >= 2^24), the largest f32, subnormals, -0
FINITE_SPECIALS = (-1.0, -0.5, -2.0, 1e30, 3.4e38, 1.4e-45, 1e-40, -1e-40, -0.0)


def synthetic(w, h, seed, specials=(np.nan, np.inf, -np.inf) + FINITE_SPECIALS, alpha=False):
    """Random colours in [0, 3), a hard edge down the middle, 2 % fireflies and three of each special value."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0, 3, (h, w, 4)).astype(np.float32)
    if not alpha:
        img[..., 3] = 1.0
    img[:, w // 2:, :3] = (3.0, 0.1, 0.0)
    img[rng.random((h, w)) < 0.02, 0] = 4000.0
    for v in specials:
        for _ in range(3):
            img[rng.integers(0, h), rng.integers(0, w), rng.integers(0, 3)] = v
    return img


@pytest.fixture(scope="module")
def frames(oracle):
    """Rendered frames at 1, 4 and 16 spp, and synthetic images with every special value."""
    out = [("%d spp" % spp, oracle.render(oracle.scene_analytical(), 160, 90, spp, seed=5)) for spp in (1, 4, 16)]
    return out + [("synthetic 97x61", synthetic(97, 61, 1)), ("synthetic 64x64", synthetic(64, 64, 2, alpha=True))]


def test_the_oracle_is_within_the_bound_of_the_float64_restatement(oracle, frames):
    worst = 0.0
    for name, img in frames:
        h, w = img.shape[:2]
        for k in EDGE_KS:
            for it in range(1, 7):
                d = dn_f64.check(oracle.denoise(img, w, h, it, k), dn_f64.denoise(img, it, k), it, "%s, edge_k %g, x%d" % (name, k, it))
                worst = max(worst, d / it)
    assert worst > 0.0                                                 # (the comparison measures something)


@pytest.mark.parametrize("it", [1, 6])
@pytest.mark.parametrize("k", [1.4e-45, 3e38])
def test_edge_k_where_k_underflows_or_overflows(oracle, frames, k, it):
    """edge_k = the smallest subnormal (every weight is 1) and 3e38 (k_1 = inf: every weight is 0 from the second iteration)."""
    for name, img in frames[::2]:
        h, w = img.shape[:2]
        dn_f64.check(oracle.denoise(img, w, h, it, k), dn_f64.denoise(img, it, k), it, "%s, edge_k %g, x%d" % (name, k, it))


MISTAKES = {
    "k scaled by 2^i": dict(k_scale=2.0),
    "step 2^i + 1": dict(step=lambda i: (1 << i) + 1),
    "H = 1/3, 1/3, 1/3": dict(h=(1.0 / 3.0,) * 3),
    "taps clamped to the border": dict(clamp=True),
    "alpha filtered": dict(filter_alpha=True),
    "one iteration fewer": dict(fewer=1),
}


@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_a_wrong_restatement_fails(oracle, mistake):
    """Each mistake, on its own, takes the restatement out of the bound (or moves a NaN, or changes alpha)."""
    img = oracle.render(oracle.scene_analytical(), 96, 64, 2, seed=5)
    img[..., 3] = np.random.default_rng(3).uniform(0, 1, img.shape[:2])
    h, w = img.shape[:2]
    got = oracle.denoise(img, w, h, 3, 2.0)
    dn_f64.check(got, dn_f64.denoise(img, 3, 2.0), 3, "the restatement itself")
    with pytest.raises(AssertionError):
        dn_f64.check(got, dn_f64.denoise(img, 3, 2.0, **MISTAKES[mistake]), 3, mistake)


@pytest.mark.parametrize("value", FINITE_SPECIALS)
def test_a_finite_pixel_never_makes_another_one_non_finite(oracle, value):
    """Confinement (include/rpt.h): a pixel whose compressed colour is not finite is copied through and takes no part in its
    neighbours' sums.  For a finite input that is exactly one value, -1; every other finite value must filter like any colour."""
    w, h = 40, 40
    img = np.random.default_rng(11).uniform(0, 1, (h, w, 4)).astype(np.float32)
    img[..., 3] = 1.0
    spots = [(0, 0), (20, 20), (39, 5), (7, 39)]
    for i, (y, x) in enumerate(spots):
        if i < 3:
            img[y, x, i] = value                                           # one channel
        else:
            img[y, x, :3] = value                                          # all three
    for it in range(1, 7):
        for k in (1e-6, 2.0):
            out = oracle.denoise(img, w, h, it, k)
            bad = ~np.isfinite(out[..., :3]).all(-1)
            for y, x in spots:
                bad[y, x] = False                                          # (1e30 and up saturate c' = 1: their own output is +inf)
            assert not bad.any(), "input %r, x%d, edge_k %g: %d pixels non-finite, at %s" % (value, it, k, bad.sum(), np.argwhere(bad)[:4].tolist())
            if value == -1.0:
                for y, x in spots:                                         # copied through
                    assert np.array_equal(out[y, x], img[y, x])
            dn_f64.check(out, dn_f64.denoise(img, it, k), it, "input %r, x%d, edge_k %g" % (value, it, k))


# ---- the fix changed nothing else -----------------------------------------------------------------------------------------------
GOLDEN = os.path.join(HERE, "golden", "denoise_before_confinement.json")


def golden_cases(oracle):
    """Inputs without an exact -1: (name, image, iterations, edge_k).  Rendered frames, and synthetic images with every other
    special value, over iterations 1-6 and every edge_k."""
    no_pole = tuple(v for v in (np.nan, np.inf, -np.inf) + FINITE_SPECIALS if v != -1.0)
    imgs = [("render 2 spp", oracle.render(oracle.scene_analytical(), 96, 64, 2, seed=3)),
            ("synthetic", synthetic(70, 45, 21, specials=no_pole * 3, alpha=True))]
    cases = []
    for name, img in imgs:
        for it in range(1, 7):
            for k in EDGE_KS + (1.4e-45, 3e38):
                cases.append(("%s x%d edge_k %g" % (name, it, k), img, it, k))
    return cases


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def test_the_fix_changed_no_frame_without_a_pole(oracle):
    """The frames of the specification before confinement (d2 skipped only when NaN, copy-through only of non-finite inputs),
    recorded from that oracle: the same inputs give the same bits today.  (For a finite compressed colour |c'| <= 1.7e7 and so
    d2 <= ~4e15: d2 = +inf needs an infinite endpoint, and such a tap had weight 0 already.)"""
    want = json.load(open(GOLDEN))
    cases = golden_cases(oracle)
    assert len(cases) == len(want)
    for name, img, it, k in cases:
        h, w = img.shape[:2]
        rec = want[name]
        assert _digest(img) == rec["input"], "%s: the input is not the recorded one" % name
        assert _digest(oracle.denoise(img, w, h, it, k)) == rec["output"], "%s: the frame differs from the one before the fix" % name


# ---- u8 ------------------------------------------------------------------------------------------------------------------------
GAMMA = float(np.float32(0.4545))


def u8_boundary_values(span=2048):
    """For every k in 1..255: every f32 within +-span ulp of the f64 preimage of k under pow(x, f32(0.4545)) * 255 (colour) and
    under x * 255 (alpha)."""
    ks = np.arange(1, 256, dtype=np.float64)
    off = np.arange(-span, span + 1, dtype=np.int64)
    out = []
    for pre in ((ks / 255.0) ** (1.0 / GAMMA), ks / 255.0):
        base = pre.astype(np.float32).view(np.int32).astype(np.int64)
        out.append((base[:, None] + off[None, :]).reshape(-1).astype(np.int32).view(np.float32))
    return out


def u8_specials():
    one = np.float32(1.0)
    v = [0.0, -0.0, 1.4e-45, 1e-40, 1.17549435e-38, np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(2)), 1e30,
         np.inf, -np.inf, -1e-40, -0.5, -1.0, -3e38, 255.0, 254.0, 255.0 / 254.0, 3.4e38]
    v = np.array(v, np.float32)
    nans = np.array([0x7FC00000, 0x7F800001, 0xFFC00000, 0x7FFFFFFF, 0xFFBADBAD, 0x7FC0FFEE], np.uint32).view(np.float32)
    near = np.array([1.0, 255.0 / 256.0, (254.0 / 255.0) ** (1.0 / GAMMA), 254.0 / 255.0], np.float32)
    near = (near.view(np.int32)[:, None] + np.arange(-4, 5)[None, :]).reshape(-1).astype(np.int32).view(np.float32)
    return np.concatenate([v, nans, near])


def u8_frame(colour, alpha, specials, w, h):
    """A w x h frame: r = the colour values, g and b = the same rotated, alpha = the alpha values; the rest specials."""
    n = w * h
    assert n >= max(len(colour), len(alpha))
    px = np.resize(specials, (n, 4)).astype(np.float32)
    px[:len(colour), 0] = colour
    px[:len(colour), 1] = np.roll(colour, 4097)
    px[:len(colour), 2] = np.roll(colour, -12345)
    px[:len(alpha), 3] = alpha
    return px.reshape(h, w, 4)


def u8_f64(img):
    """(u8 per channel, exception mask): Rust's `as u8` of the float64 products; an exception is a product within 2 ulp(f32)
    of an integer, where the f32 product may round across it."""
    with np.errstate(all="ignore"):
        x = np.asarray(img, np.float64)
        p = np.concatenate([np.power(x[..., :3], GAMMA), x[..., 3:]], -1) * 255.0
        ulp = np.spacing(np.abs(p).astype(np.float32)).astype(np.float64)
        near = np.abs(p - np.round(p)) <= 2.0 * ulp
        q = np.where(np.isnan(p), 0.0, np.clip(np.trunc(np.nan_to_num(p, posinf=255.0, neginf=0.0)), 0.0, 255.0))
    exc = near & np.isfinite(p) & (p > 0.0) & (p < 256.0)
    return q.astype(np.uint8), exc


# Of all values.  Measured on the boundary frame below: 12 019 of 4 194 268 values (0.29 %), nearly all of them from the +-2048 ulp
# windows around the step boundaries, 4-12 per window and channel; 937 of them differ from the f64 truncation (the f32 product
# rounds across the integer).
U8_MAX_EXCEPTIONS = 5e-3


def assert_u8_is_truncation(got, img, what, limit=True):
    """limit: the boundary frame's bound on the exceptions (frames of special values alone are mostly exceptions: 1.0, 255 / 254 ...)."""
    want, exc = u8_f64(img)
    got = np.asarray(got).reshape(want.shape)
    bad = (got != want) & ~exc
    assert not bad.any(), "%s: %d bytes are not the float64 truncation, first %s" % (what, bad.sum(), np.argwhere(bad)[:3].tolist())
    assert not limit or exc.sum() <= U8_MAX_EXCEPTIONS * exc.size, "%s: %d values within 2 ulp of an integer" % (what, exc.sum())
    return int(exc.sum()), int((got != want).sum())


def test_the_oracle_u8_is_f64_truncation(oracle):
    colour, alpha = u8_boundary_values()
    w, h = 1021, 1027
    img = u8_frame(colour, alpha, u8_specials(), w, h)
    n_exc, n_diff = assert_u8_is_truncation(oracle.convert_to_u8(img, w, h), img, "oracle")
    print("u8: %d of %d values within 2 ulp(f32) of an integer; %d of them differ from the f64 truncation" % (n_exc, img.size, n_diff))
