"""Inputs of the temporal accumulation tests (tests/test_temporal.py on the CPU, tests/test_gpu_temporal.py on the GPU): analytic
first-hit guides of a small world — a ground plane cut into three key regions, a sphere, the sky — as a camera sees it (float64 camera
maths, rounded to float32 rpt_guide records), camera pairs, and the fuzz laid over them as tests/gdn_fuzz.py lays it over its frames:
zero and NaN normals, position jumps, NaN positions, special depths, a history with every kind of n and non-finite colours, and
pixels with -1, NaN and 3.4e38."""
import numpy as np

import tacc_f64
from gdn_np import ALBEDO, F, KEY, KIND, NG, NS, POS, T, neutral_guides
from tacc_np import camera

SPHERE_C, SPHERE_R = np.array([0.3, 0.6, 0.0]), 0.6
CAM_A = camera((0.0, 1.5, 4.0), (0.0, 0.4, 0.0), 60.0)
# (n_max, normal_min, plane_k) of the fuzz: the defaults, every test off, a loose set, a plane test nothing but the point itself passes
PARAMS = ((32.0, 0.9, 1000.0), (1.0, -1.0, 0.0), (64.0, 0.5, 10.0), (8.0, 0.0, 1e30))


def analytic_guides(cam, w, h):
    """[h * w, 16] float32: the world seen through `cam`.  Keys: sky 0, sphere (1 << 28), the plane (2 << 28) | region."""
    C = tacc_f64.Camera(cam, w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    d = C.ray(xs.reshape(-1), ys.reshape(-1))
    n = w * h
    with np.errstate(all="ignore"):
        t_plane = np.where(d[:, 1] < 0, -C.o[1] / d[:, 1], np.inf)
        oc = C.o - SPHERE_C
        a, b, c = (d * d).sum(-1), (d * oc).sum(-1), (oc * oc).sum() - SPHERE_R ** 2
        disc = b * b - a * c
        t_sph = np.where(disc > 0, (-b - np.sqrt(np.abs(disc))) / a, np.inf)
        t_sph = np.where(t_sph > 0, t_sph, np.inf)
    t = np.minimum(t_plane, t_sph)
    hit = np.isfinite(t)
    p = C.o + d * np.where(hit, t, 0.0)[:, None]
    is_sph = hit & (t_sph <= t_plane)
    nrm = np.where(is_sph[:, None], (p - SPHERE_C) / SPHERE_R, np.array([0.0, 1.0, 0.0]))
    region = (p[:, 0] > 0.4).astype(np.uint32) + (p[:, 0] + p[:, 2] > 1.5).astype(np.uint32)
    g = neutral_guides(n)
    gu = g.view(np.uint32)
    g[:, POS], g[:, NS], g[:, NG] = p, nrm, nrm
    g[:, T] = t * np.sqrt((d * d).sum(-1))                              # the distance along the normalised ray
    gu[:, KEY] = np.where(is_sph, np.uint32(1 << 28), np.uint32(2 << 28) | region)
    gu[:, KIND] = np.where(is_sph, 1, 2)
    g[:, ALBEDO] = 0.5
    g[~hit] = neutral_guides(int((~hit).sum()))
    return g


def pan(cam, w, h, pixels):
    """`cam` moved sideways (origin and center alike) so that the image at the center's depth shifts by about `pixels`."""
    C = tacc_f64.Camera(cam, w, h)
    dist = np.sqrt(((C.o - np.asarray(cam[3:6], np.float64)) ** 2).sum())
    step = C.u / np.sqrt((C.u * C.u).sum()) * (pixels * 2.0 * C.half_width * dist / w)
    return camera(C.o + step, np.asarray(cam[3:6], np.float64) + step, cam[6])


def yaw(cam, w, h, fraction_of_fov):
    """`cam` turned about the vertical through its origin by `fraction_of_fov` of the horizontal field of view."""
    ang = np.radians(float(cam[6])) * fraction_of_fov
    o, c = np.asarray(cam[0:3], np.float64), np.asarray(cam[3:6], np.float64)
    v = c - o
    rot = np.array([v[0] * np.cos(ang) + v[2] * np.sin(ang), v[1], -v[0] * np.sin(ang) + v[2] * np.cos(ang)])
    return camera(o, o + rot, cam[6])


def dolly(cam, fraction):
    """`cam` moved towards its center by `fraction` of the distance."""
    o, c = np.asarray(cam[0:3], np.float64), np.asarray(cam[3:6], np.float64)
    return camera(o + (c - o) * fraction, c, cam[6])


def facing_away(cam):
    o, c = np.asarray(cam[0:3], np.float64), np.asarray(cam[3:6], np.float64)
    return camera(o, o - (c - o), cam[6])


def camera_pairs(w, h, turn=(0.0, 0.0, 0.0)):
    """name -> (previous camera, current camera): the current camera is CAM_A throughout.  `turn` is added to the center of every
    previous camera but the identical one.  Under a pure translation the sky, and under a sideways one every row, reprojects onto
    exact pixel centres: an edge the kernels are held to bit for bit, and one where float32 and float64 must be expected to pick
    different tap cells — a comparison between the two passes a small `turn`."""
    pairs = {"pan 0.3 px": pan(CAM_A, w, h, 0.3), "pan 1.3 px": pan(CAM_A, w, h, 1.3), "pan 5.7 px": pan(CAM_A, w, h, 5.7),
             "yaw a quarter of the fov": yaw(CAM_A, w, h, 0.25), "yaw a third": yaw(CAM_A, w, h, 1.0 / 3.0), "dolly 10 %": dolly(CAM_A, 0.1),
             "facing away": facing_away(CAM_A)}
    out = {"identical": (CAM_A, CAM_A)}
    for name, prev in pairs.items():
        prev = prev.copy()
        prev[3:6] += np.asarray(turn, F)
        out[name] = (prev, CAM_A)
    return out


def _fuzz_guides(g, rng):
    """gdn_fuzz's sprinkles over analytic guides, in place."""
    n = g.shape[0]

    def some(frac):
        return rng.random(n) < frac
    surface = g.view(np.uint32)[:, KIND] != 0
    with np.errstate(all="ignore"):                                     # a bent shading normal: ns != ng
        bent = g[:, NS] + rng.normal(0, 0.05, (n, 3))
        g[surface, NS] = (bent / np.sqrt((bent * bent).sum(-1, keepdims=True)))[surface].astype(F)
    g[some(0.03), NS] = 0.0
    g[some(0.03), NG] = 0.0
    g[some(0.02), NS.start + int(rng.integers(0, 3))] = np.nan
    g[some(0.02), NG.start + int(rng.integers(0, 3))] = np.nan
    g[some(0.01), POS.start + int(rng.integers(0, 3))] = np.nan
    jump = some(0.03)
    g[jump, POS] = g[jump, POS] + rng.uniform(-3, 3, (int(jump.sum()), 3)).astype(F)
    for v in (0.0, 1e-40, 1e19, np.inf, np.nan):
        g[some(0.015), T] = v
    flip = some(0.03)
    g.view(np.uint32)[flip, KEY] ^= np.uint32(1)
    return g


def fuzz_case(w, h, seed, prev_cam, cam, n_max, with_prev_positions=False):
    """One frame pair: dict(pixels [h, w, 4], guides, prev_guides, prev_history [h * w, 8], prev_positions or None)."""
    rng = np.random.default_rng(seed)
    n = w * h
    guides = _fuzz_guides(analytic_guides(cam, w, h), rng)
    prev_guides = _fuzz_guides(analytic_guides(prev_cam, w, h), rng)
    hist = np.zeros((n, 8), F)
    hist[:, 0:3] = rng.uniform(0, 2, (n, 3))
    hist[:, 3] = rng.uniform(1.0, 25.0, n)
    for v, frac in ((0.0, 0.05), (1.0, 0.1), (31.5, 0.1), (n_max, 0.1), (np.nan, 0.02)):
        hist[rng.random(n) < frac, 3] = v
    lum = hist[:, 0:3] @ np.array([0.2126, 0.7152, 0.0722], F)
    hist[:, 4] = lum
    hist[:, 5] = lum * lum + rng.uniform(0, 0.3, n)
    for v in (np.nan, np.inf, -np.inf):
        hist[rng.random(n) < 0.01, int(rng.integers(0, 3))] = v
    hist[rng.random(n) < 0.005, 4] = np.nan
    hist[rng.random(n) < 0.005, 5] = np.inf
    pixels = rng.uniform(0, 2, (h, w, 4)).astype(F)
    for v in (-1.0, np.nan, 3.4e38, np.inf):
        for _ in range(max(1, n // 300)):
            pixels[rng.integers(0, h), rng.integers(0, w), rng.integers(0, 3)] = v
    prev_positions = None
    if with_prev_positions:
        # a small rigid step between the frames that the previous guides do not share: every plane test on the ground meets a distance of
        # 0.05 from the tangent plane, which passes under plane_k 1000 at this world's distances (kx about 50) and would not without them
        prev_positions = np.zeros((n, 4), F)
        prev_positions[:, 0:3] = guides[:, POS] - np.array([0.02, 0.05, -0.03], F)
        prev_positions[:, 3] = rng.uniform(-9, 9, n)                    # ignored
    return dict(pixels=pixels, guides=guides, prev_guides=prev_guides, prev_history=hist, prev_positions=prev_positions)
