"""The denoiser of include/rpt.h ("denoiser") restated in float64 from the header's text, not from oracle/rpt_oracle.hpp: an
independent statement of the specification that the f32 oracle and the device kernels are measured against
(tests/test_denoise_f64.py, tests/test_gpu_image_kernels.py).  numpy only; every pixel of an iteration at once, by array shifts.

The keyword arguments of denoise() are deliberate mistakes (tests/test_denoise_f64.py shows that each one is caught)."""
import numpy as np

H = (0.25, 0.5, 0.25)

# The largest distance distance() may report between the f32 oracle and this restatement, per iteration, in units of 2^-23 (one
# ulp of 1.0 in f32).  Basis (tests/test_denoise_f64.py): over rendered frames at 1, 4 and 16 spp and synthetic images of random
# colours with fireflies, hard edges and special values, at edge_k 1e-6, 0.5, 2, 8, 1e3 and iterations 1-6, the largest distance
# per iteration was 1.84 (1.17 on the rendered frames).  The bound keeps a margin of about 2x.
ULP_PER_ITERATION = 4.0
EPS = 2.0 ** -23


def _tap(a, oy, ox, clamp):
    """a shifted by (oy, ox): out[y, x] = a[y + oy, x + ox], and where that lies inside the image.  clamp: the border pixel
    instead (a mistake: the specification skips such taps)."""
    h, w = a.shape[:2]
    if clamp:
        yi = np.clip(np.arange(h) + oy, 0, h - 1)
        xi = np.clip(np.arange(w) + ox, 0, w - 1)
        return a[yi][:, xi], np.ones((h, w), bool)
    q = np.full_like(a, np.nan)
    valid = np.zeros((h, w), bool)
    y0, y1 = max(0, -oy), min(h, h - oy)
    x0, x1 = max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        q[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        valid[y0:y1, x0:x1] = True
    return q, valid


def denoise(img, iterations, edge_k, k_scale=4.0, step=None, h=H, clamp=False, filter_alpha=False, fewer=0):
    """img: (height, width, 4) float32.  Returns the denoised image in float64.

    Mistakes, for tests that show the comparison has teeth: k_scale (k_i = edge_k * k_scale^i), step (i -> the step of
    iteration i), h (the 1-D kernel), clamp (border taps clamped instead of skipped), filter_alpha (alpha filtered like a
    colour), fewer (iterations left out)."""
    img = np.asarray(img, np.float32)
    nc = 4 if filter_alpha else 3
    c = img[..., :nc].astype(np.float64)
    with np.errstate(all="ignore"):
        a = c / (1.0 + c)                                           # c' = c / (1 + c); exactly -1 -> -inf, +-inf -> NaN
        k = np.float32(edge_k)                                      # k_i is the f32 value edge_k * 4^i: inf where that overflows
        for i in range(iterations - fewer):
            s = (1 << i) if step is None else step(i)
            acc = np.zeros_like(a)
            wsum = np.zeros(a.shape[:2])
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    q, inside = _tap(a, dy * s, dx * s, clamp)
                    d2 = ((a - q) ** 2).sum(-1)
                    use = inside & (d2 < np.inf)                    # a tap outside the image, or whose d2 is not < inf, is skipped
                    t = 1.0 - d2 * np.float64(k)
                    g = np.where(t > 0.0, t, 0.0)                   # (NaN when d2 = 0 and k = inf: no weight)
                    wt = np.where(use, h[dy + 1] * h[dx + 1] * g * g, 0.0)
                    acc += np.where(use[..., None], q * wt[..., None], 0.0)
                    wsum += wt
            a = np.where((wsum > 0.0)[..., None], acc / np.where(wsum > 0.0, wsum, 1.0)[..., None], a)     # out of place
            k = np.float32(k * np.float32(k_scale))
        out = img.astype(np.float64)
        comp = c / (1.0 + c)
        keep = np.isfinite(comp).all(-1)                            # pixels whose compressed colour is finite are expanded
        out[..., :nc] = np.where(keep[..., None], a / (1.0 - a), img[..., :nc])
    return out


def compress(x):
    """x / (1 + x) in float64, +inf -> 1: the space the comparison is made in."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.isposinf(x), 1.0, x / (1.0 + x))


def distance(got, want):
    """Per pixel and channel (r, g, b), how far the f32 image `got` is from the float64 image `want`, in units of 2^-23: the
    difference in compressed space, relative to max(1, |c'|) (so that the 1 / (1 - c') expansion cannot inflate it), or, where
    smaller, the relative difference of the outputs themselves (an output near -1 is an input near -1, whose compressed colour
    is steep in the output).  0 where both are NaN or both are the same infinity."""
    g = np.asarray(got, np.float64)[..., :3]
    w = np.asarray(want, np.float64)[..., :3]
    cg, cw = compress(g), compress(w)
    with np.errstate(all="ignore"):
        dc = np.abs(cg - cw) / np.maximum(1.0, np.abs(cw))
        do = np.abs(g - w) / np.maximum(np.abs(w), np.finfo(np.float32).tiny)
        d = np.fmin(dc, do) / EPS
    same = (np.isnan(g) & np.isnan(w)) | (np.isneginf(g) & np.isneginf(w)) | (cg == cw)
    return np.where(same, 0.0, np.where(np.isnan(d), np.inf, d))


def check(got, want, iterations, what=""):
    """got (f32) equals want (float64) within the calibrated bound: NaN and -inf in the same places, alpha equal, every other
    value within ULP_PER_ITERATION * iterations."""
    got = np.asarray(got)
    want = np.asarray(want)
    g3, w3 = np.asarray(got[..., :3], np.float64), want[..., :3]
    assert np.array_equal(np.isnan(g3), np.isnan(w3)), "%s: NaN in different places" % what
    assert np.array_equal(np.isneginf(g3), np.isneginf(w3)), "%s: -inf in different places" % what
    assert np.array_equal(np.asarray(got[..., 3], np.float64), want[..., 3]) or \
        np.array_equal(np.isnan(got[..., 3]), np.isnan(want[..., 3])) and \
        np.array_equal(np.nan_to_num(np.asarray(got[..., 3], np.float64)), np.nan_to_num(want[..., 3])), "%s: alpha differs" % what
    d = distance(got, want)
    worst = float(d.max()) if d.size else 0.0
    assert worst <= ULP_PER_ITERATION * iterations, "%s: %.3g ulp from the float64 restatement at %s (bound %g)" % (
        what, worst, np.unravel_index(int(d.argmax()), d.shape), ULP_PER_ITERATION * iterations)
    return worst
