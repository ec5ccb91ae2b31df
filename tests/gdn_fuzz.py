"""Inputs of the guided denoiser's tests (tests/test_denoise_guided.py on the CPU, tests/test_gpu_denoise_guided.py on the GPU): fuzzed
frames with guides that reach every branch of the specification (include/rpt.h, "guided denoiser"), and the synthetic scene of the
quality check — a checkered floor, a striped wall and a sphere with analytic guides and gamma noise."""
import numpy as np

from gdn_np import ALBEDO, F, KEY, KIND, NG, NS, POS, T, neutral_guides

# (normal_k, plane_k, edge_k) triples of the fuzz: the defaults, each term off, each term large, an edge_k whose k_i overflows
PARAMS = ((4.0, 1000.0, 0.25), (0.0, 0.0, 2.0), (1e30, 0.0, 1e-6), (0.0, 1e30, 8.0), (4.0, 1000.0, 3e37), (0.5, 10.0, 1e3))


def _unit(v):
    with np.errstate(all="ignore"):
        return (v / np.sqrt((v * v).sum(-1, keepdims=True))).astype(F)


def fuzz_frame(w, h, seed):
    """(img [h, w, 4], guides [h * w, 16]): 3-5 key regions split by random lines, positions smooth inside a region with jumps between
    them, unit / zero / NaN normals, t among ordinary depths, 0, a subnormal, 1e19, +inf and NaN, albedo among textures, 0, below FLOOR,
    FLOOR itself, above 1 and NaN, colours with fireflies, NaN, -1, +-inf and 3.4e38."""
    rng = np.random.default_rng(seed)
    n = w * h
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    region = np.zeros((h, w), np.int64)
    for _ in range(int(rng.integers(2, 5))):                           # 2-4 lines: 3-5 regions at most sizes
        a, b = rng.normal(size=2)
        region = region * 2 + ((a * (xx - rng.uniform(0, w)) + b * (yy - rng.uniform(0, h))) > 0)
    ids = {v: i for i, v in enumerate(np.unique(region))}
    region = np.vectorize(ids.get)(region) % 5
    g = neutral_guides(n)
    gu = g.view(np.uint32)
    kinds = np.array([3, 3, 1, 2, 0], np.uint32)[region]
    base = rng.uniform(-1000, 1000, (5, 3))[region]                    # the jump between regions
    slope = rng.uniform(-0.05, 0.05, (5, 2, 3))[region]
    pos = base + slope[..., 0, :] * xx[..., None] + slope[..., 1, :] * yy[..., None] + rng.normal(0, 1e-3, (h, w, 3))
    nrm = _unit(rng.normal(size=(5, 3)))[region]
    g[:, POS] = pos.reshape(n, 3)
    gu[:, KEY] = ((kinds.astype(np.uint32) << 28) | (region.astype(np.uint32) + 7)).reshape(n)
    g[:, NG] = nrm.reshape(n, 3)
    g[:, NS] = _unit(nrm + rng.normal(0, 0.05, (h, w, 3))).reshape(n, 3)
    g[:, T] = rng.uniform(1.0, 20.0, n)
    gu[:, KIND] = kinds.reshape(n)
    g[:, ALBEDO] = rng.uniform(0.05, 1.0, (n, 3)) * np.where(((xx // 3 + yy // 3) % 2).reshape(n, 1) > 0, 1.0, 0.3)
    miss = (kinds == 0).reshape(n)
    g[miss] = neutral_guides(int(miss.sum()))

    def some(frac=0.03):
        return rng.random(n) < frac
    g[some(), NS] = 0.0
    g[some(), NG] = 0.0
    g[some(0.02), NS.start + int(rng.integers(0, 3))] = np.nan
    g[some(0.02), NG.start + int(rng.integers(0, 3))] = np.nan
    g[some(0.01), POS.start + int(rng.integers(0, 3))] = np.nan
    for v in (0.0, 1e-40, 1e19, np.inf, np.nan):
        g[some(0.015), T] = v
    for v in (0.0, 1e-3, 1.0 / 64.0, 2.5, np.nan):
        g[some(0.02), ALBEDO.start + int(rng.integers(0, 3))] = v
    img = rng.uniform(0, 1, (h, w, 4)).astype(F)
    img[..., :3] *= g[:, ALBEDO].reshape(h, w, 3) * 2.0
    img[rng.random((h, w)) < 0.02, int(rng.integers(0, 3))] = 4000.0   # fireflies
    for v in (np.nan, -1.0, np.inf, -np.inf, 3.4e38, -0.5, 1e-40):
        for _ in range(max(1, n // 400)):
            img[rng.integers(0, h), rng.integers(0, w), rng.integers(0, 3)] = v
    return img, g


def quality_scene(w, h, spp_like, seed):
    """(clean [h, w, 4], noisy, guides): a checkered floor below the horizon, a striped wall above it, a sphere in front; the radiance
    is albedo x a smooth shading, the noise a gamma distribution of shape `spp_like` and mean 1 per channel (1 spp: heavy-tailed)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = (xx + 0.5) / w - 0.5, 0.5 - (yy + 0.5) / h
    d = np.stack([u, v, -np.ones_like(u)], -1)                          # a pinhole at the origin looking down -z
    n = w * h
    g = neutral_guides(n).reshape(h, w, 16)
    gu = g.view(np.uint32)
    with np.errstate(all="ignore"):
        t_floor = np.where(d[..., 1] < 0, -0.5 / d[..., 1], np.inf)     # the plane y = -0.5
    t_wall = 6.0 / 1.0 * np.ones_like(u)                                # the plane z = -6
    centre, rad = np.array([0.1, -0.1, -3.0]), 0.4
    b = (d * centre).sum(-1)
    dd = (d * d).sum(-1)
    disc = b * b - dd * ((centre * centre).sum() - rad * rad)
    with np.errstate(all="ignore"):
        t_sph = np.where(disc > 0, (b - np.sqrt(disc)) / dd, np.inf)
    t = np.minimum(np.minimum(t_floor, t_wall), t_sph)
    p = d * t[..., None]
    is_sph, is_floor = t == t_sph, (t == t_floor) & (t != t_sph)
    nrm = np.where(is_sph[..., None], (p - centre) / rad, np.where(is_floor[..., None], (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)))
    checker = ((np.floor(p[..., 0] * 3) + np.floor(p[..., 2] * 3)) % 2)[..., None]
    stripes = (np.floor(p[..., 0] * 2.5) % 2)[..., None]
    albedo = np.where(is_sph[..., None], (0.8, 0.3, 0.2),
                      np.where(is_floor[..., None], 0.15 + 0.7 * checker * np.ones(3), np.array([0.2, 0.3, 0.7]) + 0.25 * stripes))
    light = _unit(np.array([0.4, 0.8, 0.45]))
    shade = 0.25 + 0.9 * np.clip((nrm * light).sum(-1), 0, 1)[..., None]
    clean = np.ones((h, w, 4), F)
    clean[..., :3] = albedo * shade
    noisy = clean.copy()
    noisy[..., :3] *= rng.gamma(spp_like, 1.0 / spp_like, (h, w, 3))
    g[..., POS], g[..., NS], g[..., NG], g[..., T], g[..., ALBEDO] = p, nrm, nrm, t, albedo
    gu[..., KEY] = np.where(is_sph, (1 << 28) | 0, np.where(is_floor, (2 << 28) | 0, (2 << 28) | 1))
    gu[..., KIND] = np.where(is_sph, 1, 2)
    return clean, noisy, np.ascontiguousarray(g.reshape(n, 16))


def rmse_compressed(a, b):
    """RMSE over r, g, b in the compressed space c / (1 + c)."""
    a, b = (np.asarray(x, np.float64)[..., :3] for x in (a, b))
    return float(np.sqrt(np.mean((a / (1 + a) - b / (1 + b)) ** 2)))
