"""A frame against the f64 oracle's frame of the same scene, seed, spp and flags (liboracle_f64.so, RPT_ORACLE_F64): the distance
statements a frame that is not bit-identical to the f32 oracle — the relaxed-arithmetic kernels (RPT_RENDER_FAST_MATH) — is held to.

The f64 frame runs the reference's statements, draws and operation order in double.  An f32 frame of the same scene rounds every
pixel of it, except where an f32 rounding flipped a branch and one sample took another path (tests/test_oracle_f64.py).  Five figures
describe how far a frame sits from it:

  finite        every pixel's colour is finite
  median        the median |delta| over the channels of the pixels with no flipped branch: the rounding error of the arithmetic
  flip          the fraction of "flipped" pixels, whose largest channel |delta| is above `flip_threshold`
  max_samples   the largest |delta| in samples' worth (spp * |delta|): a flip moves one sample by O(1), never a pixel by more
  bias          the signed mean delta over the frame, and its standard error (over pixels): a systematic error that flips no single
                pixel far shows here

Bounds are not fixed numbers: `calibrated_bounds` takes them from the strict f32 frame of the same case against the same f64 frame (the
GPU's strict frame is bit-identical to the f32 oracle's, so the CPU oracle gives that calibration), times stated factors.  Test
infrastructure; no GPU needed."""
import numpy as np

FLIP_THRESHOLD = 1e-4


class Distance:
    """The figures of one frame against the f64 frame."""

    def __init__(self, frame, ref64, spp, flip_threshold=FLIP_THRESHOLD):
        frame = np.asarray(frame, dtype=np.float32)
        ref64 = np.asarray(ref64, dtype=np.float32)
        assert frame.shape == ref64.shape and frame.ndim == 3 and frame.shape[2] >= 3, (frame.shape, ref64.shape)
        c = frame[..., :3].astype(np.float64)
        self.n_pixels = c.shape[0] * c.shape[1]
        self.spp = spp
        self.n_nonfinite = int((~np.isfinite(c).all(axis=-1)).sum())
        self.finite = self.n_nonfinite == 0
        d = np.where(np.isfinite(c), c, 0.0) - ref64[..., :3].astype(np.float64)
        a = np.abs(d)
        flipped = a.max(axis=-1) > flip_threshold
        self.n_flipped = int(flipped.sum())
        self.flip = self.n_flipped / self.n_pixels
        self.median = float(np.median(a[~flipped])) if (~flipped).any() else float("inf")
        self.max_samples = float(spp * a.max())
        per_pixel = d.mean(axis=-1).ravel()
        self.bias = float(per_pixel.mean())
        self.bias_se = float(per_pixel.std(ddof=1) / np.sqrt(per_pixel.size))

    def __repr__(self):
        return ("finite %s (%d not), median %.3g, flipped %.4f %% (%d px), max %.3g samples, bias %.3g (se %.3g)" %
                (self.finite, self.n_nonfinite, self.median, 100.0 * self.flip, self.n_flipped, self.max_samples, self.bias, self.bias_se))


class Bounds:
    """What a frame must stay within: median <= median, flip <= flip (a fraction), max_samples <= max_samples, and
    |bias| <= bias_sigmas * (the frame's own standard error) + bias_floor."""

    def __init__(self, median, flip, max_samples, bias_sigmas=4.0, bias_floor=1e-6):
        self.median, self.flip, self.max_samples = median, flip, max_samples
        self.bias_sigmas, self.bias_floor = bias_sigmas, bias_floor

    def __repr__(self):
        return "median <= %.3g, flipped <= %.4f %%, max <= %.3g samples, |bias| <= %g se + %g" % (
            self.median, 100.0 * self.flip, self.max_samples, self.bias_sigmas, self.bias_floor)

    def failures(self, dist):
        """The statements `dist` breaks (empty: within bounds)."""
        out = []
        if not dist.finite:
            out.append("%d pixels not finite" % dist.n_nonfinite)
        if not dist.median <= self.median:
            out.append("median |delta| %.3g > %.3g" % (dist.median, self.median))
        if not dist.flip <= self.flip:
            out.append("flipped pixels %.4f %% > %.4f %%" % (100.0 * dist.flip, 100.0 * self.flip))
        if not dist.max_samples <= self.max_samples:
            out.append("largest |delta| %.3g samples > %.3g" % (dist.max_samples, self.max_samples))
        if not abs(dist.bias) <= self.bias_sigmas * dist.bias_se + self.bias_floor:
            out.append("bias %.3g beyond %g standard errors (%.3g) + %g" % (dist.bias, self.bias_sigmas, dist.bias_se, self.bias_floor))
        return out


# The factors over the strict f32 frame's own distance from the f64 frame (tests/test_gpu_relaxed.py states what they were set from).
FLIP_FACTOR = 2.5
FLIP_FLOOR_PIXELS = 6
MEDIAN_FACTOR = 4.0
MEDIAN_FLOOR = 1e-8
MAX_SAMPLES_FACTOR = 2.0
MAX_SAMPLES_FLOOR = 8.0


def calibrated_bounds(strict, flip_factor=FLIP_FACTOR, flip_floor_pixels=FLIP_FLOOR_PIXELS, median_factor=MEDIAN_FACTOR,
                      median_floor=MEDIAN_FLOOR, max_samples_factor=MAX_SAMPLES_FACTOR, max_samples_floor=MAX_SAMPLES_FLOOR):
    """Bounds from the strict frame's Distance of the same case: flip <= flip_factor x strict + a floor of a few pixels (frames with very
    few flips), median <= median_factor x strict + a floor, max <= max(max_samples_factor x strict, max_samples_floor) samples."""
    assert strict.finite, "the strict frame itself has non-finite pixels: %r" % (strict,)
    return Bounds(median=median_factor * strict.median + median_floor,
                  flip=flip_factor * strict.flip + flip_floor_pixels / strict.n_pixels,
                  max_samples=max(max_samples_factor * strict.max_samples, max_samples_floor))


def compare(frame, ref64, spp, bounds, what="", flip_threshold=FLIP_THRESHOLD):
    """Assert that `frame` is within `bounds` of the f64 frame; -> its Distance."""
    dist = Distance(frame, ref64, spp, flip_threshold)
    bad = bounds.failures(dist)
    assert not bad, "%s: %s\n  frame:  %r\n  bounds: %r" % (what, "; ".join(bad), dist, bounds)
    return dist


class Calibrated:
    """One case's f64 frame and the strict f32 oracle's calibration: `check(frame)` holds a frame of the same scene, seed, spp and
    flags to the bounds.  `oracle` is the f32 oracle (liboracle.so), `oracle_f64` the f64 one; `desc` the scene's rpt_scene_desc."""

    def __init__(self, oracle, oracle_f64, desc, width, height, spp, seed=1, render_flags=0, **factors):
        self.spp = spp
        self.ref64 = oracle_f64.render(desc, width, height, spp, seed=seed, render_flags=render_flags)
        self.strict_frame = oracle.render(desc, width, height, spp, seed=seed, render_flags=render_flags)
        self.strict = Distance(self.strict_frame, self.ref64, spp)
        self.bounds = calibrated_bounds(self.strict, **factors)
        # the strict frame is within its own bounds (bias included): a calibration that fails that would test nothing
        compare(self.strict_frame, self.ref64, spp, self.bounds, "strict f32 frame against its own calibration")

    def distance(self, frame):
        return Distance(frame, self.ref64, self.spp)

    def check(self, frame, what=""):
        return compare(frame, self.ref64, self.spp, self.bounds, what)

    def ratios(self, dist):
        """(flip, median) of `dist` over the strict frame's: what the factors are set from."""
        return (dist.flip / self.strict.flip if self.strict.flip else float("inf") if dist.flip else 1.0,
                dist.median / self.strict.median if self.strict.median else float("inf") if dist.median else 1.0)
