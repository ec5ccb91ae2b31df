"""Environment lighting on the host (include/rpt.h, "environment lighting"; CPU only): csrc/host_env.h's checks answer in their
order, and its table, lookup and sampler equal a numpy float32 / integer restatement bit for bit (under g++'s address and
undefined-behaviour sanitizers: tests/env_harness.cpp); a sampled direction looks up the texel it was sampled in; the pdf equals an
independent float64 Jacobian of the octahedral map; rpt_environment has C's layout; the entry points reject what they can without a
GPU; scenes.octahedral_from_equirect keeps a constant image and the six axes; and the meshenv_* kernels live in a code object
library of their own, none of which uses scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from kernel_census import code_object_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rust-pathtracer_amd")
F = np.float32
FMAX = F(3.40282347e+38)
NONE = 0xFFFFFFFF
SIZES = (1, 2, 3, 5, 16, 17)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("env") / "env_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "env_harness.cpp"), "-o", exe], check=True)
    return exe


# ---- the restatements (tests/test_gpu_mesh_env.py and tests/test_gpu_mesh_env_f64.py import them) -----------------------------------
def restate_table(image, sampled=True):
    """[S, S, 3] f32 -> (texels [S*S, 4] f32 {r, g, b, (float)q_k}, C_k [S*S] uint64, E): include/rpt.h, "Table"."""
    rgb = np.ascontiguousarray(image, F).reshape(-1, 3)
    n = len(rgb)
    texels = np.zeros((n, 4), F)
    texels[:, :3] = rgb
    cdf = np.zeros(n, np.uint64)
    if not sampled:
        return texels, cdf, 0
    w = (rgb[:, 0] + rgb[:, 1]) + rgb[:, 2]
    assert w.dtype == F
    w_max = w.max()
    if not w_max > 0:
        return texels, cdf, 0
    e = int(np.frexp(w_max)[1])                                      # W_max = f * 2^E, f in [0.5, 1): subnormal values included
    q = np.floor(np.ldexp(w.astype(np.float64), 36 - e)).astype(np.uint64)
    texels[:, 3] = q.astype(F)                                      # uint64 -> f32: to nearest, ties to even
    return texels, np.cumsum(q, dtype=np.uint64), e


def _sgn(x):
    return np.where(x >= 0, F(1), F(-1)).astype(F)


def _pdf(q_f, q_total_f, size, p):
    s_f = F(size)
    l2 = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    length = np.sqrt(l2)
    sel = q_f / q_total_f
    return (sel * ((s_f * s_f) * F(0.25))) * (l2 * length), length


def restate_lookup(texels, size, q_total, scale, d):
    """Lookup of directions d [n, 3] f32 -> (k [n] int64, 0xFFFFFFFF: none; p [n, 3] BEFORE the fold; radiance [n, 3]; lp [n])."""
    d = np.ascontiguousarray(d, F).reshape(-1, 3)
    s_f, scale = F(size), F(scale)
    with np.errstate(all="ignore"):
        l1 = (np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2])
        ok = (l1 > 0) & (l1 <= FMAX)
        l1s = np.where(ok, l1, F(1))
        px, py, pz = d[:, 0] / l1s, d[:, 1] / l1s, d[:, 2] / l1s
        p = np.stack([px, py, pz], 1)
        low = d[:, 1] < 0
        fx = np.where(low, (F(1) - np.abs(pz)) * _sgn(px), px)
        fz = np.where(low, (F(1) - np.abs(px)) * _sgn(pz), pz)
        s, t = fx * F(0.5) + F(0.5), fz * F(0.5) + F(0.5)
        assert s.dtype == F and l1.dtype == F
        i = np.minimum(np.floor(np.where(ok, s, F(0)) * s_f).astype(np.int64), size - 1)
        j = np.minimum(np.floor(np.where(ok, t, F(0)) * s_f).astype(np.int64), size - 1)
        k = j * size + i
        c = texels[k]
        rad = c[:, :3] * scale
        lp = np.zeros(len(d), F)
        if q_total:
            full, _ = _pdf(c[:, 3], F(np.uint64(q_total)), size, p)
            lp = np.where(c[:, 3] != 0, full, F(0)).astype(F)
    k = np.where(ok, k, NONE)
    p = np.where(ok[:, None], p, F(0)).astype(F)
    rad = np.where(ok[:, None], rad, F(0)).astype(F)
    lp = np.where(ok, lp, F(0)).astype(F)
    return k, p, rad, lp


def restate_pick(cdf, r0a, r0b):
    """J, T and the binary search of "mesh lights": the first k with C_k > T."""
    q_total = int(cdf[-1])
    out = np.empty(len(r0a), np.int64)
    for n, (a, b) in enumerate(zip(r0a, r0b)):
        j = (int(F(a) * F(16777216.0)) << 24) | int(F(b) * F(16777216.0))
        out[n] = np.searchsorted(cdf, np.uint64((j * q_total) >> 48), side="right")
    return out


def restate_sample_point(k, size, r1, r2):
    """The point p of the octahedron (after the fold, py from before it) in texel k with the draws r1, r2."""
    s_f = F(size)
    i, j = (k % size).astype(F), (k // size).astype(F)
    s, t = (i + np.asarray(r1, F)) / s_f, (j + np.asarray(r2, F)) / s_f
    px, pz = s * F(2) - F(1), t * F(2) - F(1)
    py = (F(1) - np.abs(px)) - np.abs(pz)
    low = py < 0
    fx = np.where(low, (F(1) - np.abs(pz)) * _sgn(px), px)
    fz = np.where(low, (F(1) - np.abs(px)) * _sgn(pz), pz)
    p = np.stack([fx, py, fz], 1)
    assert p.dtype == F
    return p


def restate_sample(texels, cdf, size, scale, n_f, draws):
    """The sampler on draws [n, 4] = r0a, r0b, r1, r2 -> (k [n] (0xFFFFFFFF: dark), direction [n, 3], pdf [n], emission [n, 3])."""
    draws = np.ascontiguousarray(draws, F).reshape(-1, 4)
    n = len(draws)
    if int(cdf[-1]) == 0:
        return np.full(n, NONE, np.int64), np.zeros((n, 3), F), np.zeros(n, F), np.zeros((n, 3), F)
    k = restate_pick(cdf, draws[:, 0], draws[:, 1])
    p = restate_sample_point(k, size, draws[:, 2], draws[:, 3])
    c = texels[k]
    pdf, length = _pdf(c[:, 3], F(np.uint64(cdf[-1])), size, p)
    direction = p / length[:, None]
    emission = F(n_f) * (c[:, :3] * F(scale))
    assert direction.dtype == F and emission.dtype == F and pdf.dtype == F
    return k, direction, pdf, emission


def random_image(size, seed, kind="random"):
    """The images of the table tests: random over six decades with some zero texels, all-equal, one bright texel in a zero image."""
    rng = np.random.default_rng(seed)
    if kind == "equal":
        return np.full((size, size, 3), F(0.37), F)
    if kind == "one":
        img = np.zeros((size, size, 3), F)
        img[(size * 2) // 3, size // 3] = (F(5.0), F(3.0), F(1.5))
        return img
    img = (rng.random((size, size, 3)) * 10.0 ** rng.uniform(-4, 2, (size, size, 1))).astype(F)
    img[rng.random((size, size)) < 0.1] = 0
    return img


def draws_24(rng, shape):
    """Draws as the kernel's own: multiples of 2^-24 in [0, 1)."""
    return (rng.integers(0, 1 << 24, shape).astype(np.float64) / (1 << 24)).astype(F)


def directions(rng, n):
    """Unit directions, and beside them the cases the statement names: the six axes, d.y = +-0, unnormalised, NaN, zero, infinite."""
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    special = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
                        [0.6, 0.0, 0.8], [0.6, -0.0, 0.8], [-0.6, 0.0, -0.8], [-0.6, -0.0, 0.8], [0.0, -0.0, 1.0], [-0.0, -1.0, -0.0],
                        [3.0, 4.0, -5.0], [1e-30, -2e-30, 1e-30], [np.nan, 0.5, 0.5], [0.5, np.nan, 0.5], [0, 0, 0], [np.inf, 1, 0],
                        [3e38, 3e38, 3e38]], dtype=F)
    return np.concatenate([special, d])


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the harness against the restatement ---------------------------------------------------------------------------------------------
def run_table(harness, tmp_path, image, sampled):
    size = image.shape[0]
    inp, out = str(tmp_path / "t.in"), str(tmp_path / "t.out")
    with open(inp, "wb") as f:
        f.write(np.array([size, 1 if sampled else 0], np.uint32).tobytes() + np.ascontiguousarray(image, F).tobytes())
    subprocess.run([harness, "table", inp, out], check=True, capture_output=True)
    raw = open(out, "rb").read()
    n = size * size
    return (np.frombuffer(raw[:16 * n], F).reshape(n, 4), np.frombuffer(raw[16 * n:24 * n], np.uint64), int(np.frombuffer(raw[24 * n:], np.int32)[0]))


@pytest.mark.parametrize("size", SIZES)
def test_table_lookup_and_sampler_equal_the_restatement_bit_for_bit(harness, tmp_path, size):
    rng = np.random.default_rng(0xE57 + size)
    for kind in ("random", "equal", "one"):
        image = random_image(size, 100 + size, kind)
        for sampled in (True, False):
            texels, cdf, e = run_table(harness, tmp_path, image, sampled)
            r_texels, r_cdf, r_e = restate_table(image, sampled)
            assert np.array_equal(bits(texels), bits(r_texels)) and np.array_equal(cdf, r_cdf) and e == r_e, (kind, sampled)
            if sampled:
                assert cdf[-1] >= 1 << 35 and np.all(np.diff(cdf.astype(np.int64)) >= 0)
            # lookup
            d = directions(rng, 400)
            scale = F(1.7)
            inp, out = str(tmp_path / "l.in"), str(tmp_path / "l.out")
            with open(inp, "wb") as f:
                f.write(np.array([size, 1 if sampled else 0, len(d)], np.uint32).tobytes() + scale.tobytes() + image.tobytes() + d.tobytes())
            subprocess.run([harness, "lookup", inp, out], check=True, capture_output=True)
            got = np.frombuffer(open(out, "rb").read(), np.uint32).reshape(len(d), 8)
            k, p, rad, lp = restate_lookup(r_texels, size, int(r_cdf[-1]), scale, d)
            assert np.array_equal(got[:, 0], k.astype(np.uint32)), (kind, sampled)
            assert np.array_equal(got[:, 1:4], bits(p)) and np.array_equal(got[:, 4:7], bits(rad)) and np.array_equal(got[:, 7], bits(lp)), (kind, sampled)
            if not sampled:
                assert not got[:, 7].any()
        # sampler
        draws = draws_24(rng, (600, 4))
        draws[:8, :2] = [[0, 0], [1 - 2.0 ** -24, 1 - 2.0 ** -24], [0.5, 0], [0, 2.0 ** -24], [0.25, 0.75], [0, 0.5], [2.0 ** -24, 0], [0.75, 0]]
        draws[:4, 2:] = [[0, 0], [1 - 2.0 ** -24, 1 - 2.0 ** -24], [0, 1 - 2.0 ** -24], [0.5, 0.5]]
        inp, out = str(tmp_path / "s.in"), str(tmp_path / "s.out")
        with open(inp, "wb") as f:
            f.write(np.array([size, len(draws)], np.uint32).tobytes() + np.array([0.9, 3.0], F).tobytes() + image.tobytes() + draws.tobytes())
        subprocess.run([harness, "sample", inp, out], check=True, capture_output=True)
        got = np.frombuffer(open(out, "rb").read(), np.uint32).reshape(len(draws), 8)
        r_texels, r_cdf, _ = restate_table(image, True)
        k, direction, pdf, emission = restate_sample(r_texels, r_cdf, size, 0.9, 3.0, draws)
        assert np.array_equal(got[:, 0], k.astype(np.uint32)), kind
        assert np.array_equal(got[:, 1:4], bits(direction)) and np.array_equal(got[:, 4], bits(pdf)) and np.array_equal(got[:, 5:8], bits(emission)), kind
        w = (image[..., 0] + image[..., 1]) + image[..., 2]
        assert np.all(w.reshape(-1)[k] > 0), "a texel of weight zero is never picked"


def test_the_all_zero_image_is_dark(harness, tmp_path):
    image = np.zeros((3, 3, 3), F)
    texels, cdf, e = run_table(harness, tmp_path, image, True)
    assert not texels.any() and not cdf.any() and e == 0
    k, direction, pdf, emission = restate_sample(*restate_table(image)[:2], 3, 1.0, 1.0, np.full((2, 4), 0.5, F))
    assert np.all(k == NONE) and not direction.any() and not pdf.any() and not emission.any()
    inp, out = str(tmp_path / "s.in"), str(tmp_path / "s.out")
    with open(inp, "wb") as f:
        f.write(np.array([3, 2], np.uint32).tobytes() + np.array([1, 1], F).tobytes() + image.tobytes() + np.full((2, 4), 0.5, F).tobytes())
    subprocess.run([harness, "sample", inp, out], check=True, capture_output=True)
    got = np.frombuffer(open(out, "rb").read(), np.uint32).reshape(2, 8)
    assert np.all(got[:, 0] == NONE) and not got[:, 1:].any()


@pytest.mark.parametrize("size", SIZES)
def test_a_sampled_direction_looks_up_its_own_texel(size):
    """For picks (k, r1, r2) with r1, r2 at least 2^-10 from 0 and 1 the lookup of the sampled direction returns k: the normalisation
    and the division by l1 move s * S by a few 2^-24 S, far less than 2^-10."""
    rng = np.random.default_rng(0xD1 + size)
    n = size * size
    k = np.concatenate([np.arange(n), rng.integers(0, n, 2000)])
    lo = 2.0 ** -10
    r = (lo + rng.random((len(k), 2)) * (1 - 2 * lo)).astype(F)
    r[:n] = np.array([[lo, 1 - lo]], F)
    p = restate_sample_point(k, size, r[:, 0], r[:, 1])
    _, length = _pdf(F(1), F(1), size, p)
    d = p / length[:, None]
    texels = np.zeros((n, 4), F)
    got, p_back, _, _ = restate_lookup(texels, size, 0, 1.0, d)
    assert np.array_equal(got, k)
    assert np.allclose(p_back, p, atol=1e-6), "the lookup's p is the sampler's point"


def test_axes_and_signed_zero_land_where_the_statement_says():
    for size in (1, 2, 3, 5, 16):
        texels = np.zeros((size * size, 4), F)
        mid, last = size // 2, size - 1
        look = lambda d: int(restate_lookup(texels, size, 0, 1.0, np.array([d], F))[0][0])      # noqa: E731
        at = lambda i, j: j * size + i                                                           # noqa: E731
        assert look([0, 1, 0]) == at(mid, mid), "+y is the centre"
        assert look([1, 0, 0]) == at(last, mid) and look([-1, 0, 0]) == at(0, mid)
        assert look([0, 0, 1]) == at(mid, last) and look([0, 0, -1]) == at(mid, 0)
        assert look([0, -1, 0]) == at(last, last), "-y folds to (1, 1) with sgn(0) = 1: the last corner"
        assert look([-1e-3, -1, -1e-3]) == at(0, 0) and look([1e-3, -1, -1e-3]) == at(last, 0)
        # d.y = -0 does not fold; a tiny negative d.y does, and lands in the same texel away from borders
        a, b = look([0.3, 0.0, 0.7]), look([0.3, -0.0, 0.7])
        assert a == b
        k, p, rad, lp = restate_lookup(texels, size, 0, 1.0, np.array([[np.nan, 0, 1], [0, 0, 0]], F))
        assert np.all(k == NONE) and not rad.any() and not p.any() and not lp.any(), "a NaN direction gives black"


# ---- the pdf against an independent float64 statement ---------------------------------------------------------------------------------
def _direction64(s, t):
    """The normalised inverse map in float64: (s, t) in [0, 1]^2 -> unit direction."""
    px, pz = 2.0 * s - 1.0, 2.0 * t - 1.0
    py = 1.0 - np.abs(px) - np.abs(pz)
    low = py < 0
    fx = np.where(low, (1.0 - np.abs(pz)) * np.where(px >= 0, 1.0, -1.0), px)
    fz = np.where(low, (1.0 - np.abs(px)) * np.where(pz >= 0, 1.0, -1.0), pz)
    p = np.stack([fx, py, fz], -1)
    return p / np.linalg.norm(p, axis=-1, keepdims=True)


def _jacobian_central(s, t, h):
    ds = (_direction64(s + h, t) - _direction64(s - h, t)) / (2 * h)
    dt = (_direction64(s, t + h) - _direction64(s, t - h)) / (2 * h)
    return np.linalg.norm(np.cross(ds, dt), axis=-1)


def _jacobian_one_sided(s, t, h, sign):
    """|dd/ds x dd/dt| from second-order one-sided differences, both stepping away from the image's centre (sign = 1) or both towards
    it (sign = -1): the three nodes of each difference then stay inside one smooth piece of the map even when (s, t) lies on a kink
    (px = 0, pz = 0 or the fold's diagonal |px| + |pz| = 1)."""
    es = sign * h * np.where(s >= 0.5, 1.0, -1.0)
    et = sign * h * np.where(t >= 0.5, 1.0, -1.0)
    f0 = _direction64(s, t)
    ds = (-3 * f0 + 4 * _direction64(s + es, t) - _direction64(s + 2 * es, t)) / (2 * es)[..., None]
    dt = (-3 * f0 + 4 * _direction64(s, t + et) - _direction64(s, t + 2 * et)) / (2 * et)[..., None]
    return np.linalg.norm(np.cross(ds, dt), axis=-1)


def _solid_angles(size, m, h=1e-6):
    """Every texel's solid angle by the midpoint rule over m x m cells of |dd/ds x dd/dt| (central differences)."""
    c = (np.arange(size * m) + 0.5) / (size * m)
    s, t = np.meshgrid(c, c, indexing="xy")
    jac = _jacobian_central(s, t, h) / (size * m) ** 2
    return jac.reshape(size, m, size, m).sum(axis=(1, 3)).reshape(-1)


PDF_SIZES = (2, 3, 8)
QUAD_CELLS = 96
SUM_TOL = 1e-7           # 4 x the quadrature's own error of the sum, below, rounded up
PDF_TOL = 1.1e-6         # 4 x the finite differences' own error, below, + 16 * 2^-24 for the f32 side


@pytest.mark.parametrize("size", PDF_SIZES)
def test_the_pdf_is_the_inverse_solid_angle_density_of_an_independent_float64_map(size):
    """Independent of the closed form |p|^3: the solid angle of a patch of the image is the integral of |dd/ds x dd/dt| over it, d
    the normalised inverse map, the derivatives by finite differences in float64.

    (a) The texels' solid angles, by the midpoint rule with QUAD_CELLS^2 cells each, sum to 4 pi.  The quadrature's own error,
    measured by halving its step (48 -> 96 cells per texel side): the sum moves by 2.1e-8, 1.4e-8 and 5.0e-9 of 4 pi at sizes 2, 3
    and 8 (a single texel that a kink cuts by up to 5.6e-5 of itself: those errors cancel across the kink).  SUM_TOL = 1e-7; measured
    sum / 4 pi - 1: 2.0e-8, 1.3e-8, 5.0e-9.
    (b) At every texel centre, sel / Omega with Omega = |dd/ds x dd/dt| / S^2 — the solid angle per unit of texel area AT the centre:
    the pdf varies inside a texel, so it is the limit of sel / Omega over a small patch that the f32 pdf states — equals the f32
    pdf.  Centres lie on kinks of the map (odd sizes: the centre and the axes; 8: the fold's diagonals), so the differences are
    one-sided, second order, once both away from the image's centre and once both towards it, and both must agree with the pdf.
    Their own error, measured by halving the step (2e-5 -> 1e-5): at most 1.5e-8 relative.  The f32 side: the point's three
    coordinates, dot's five roundings, the root, the two conversions, the divide and four products, 16 * 2^-24 = 9.5e-7 to be
    safe.  PDF_TOL = 1.1e-6; measured worst: 7.0e-8, 1.7e-7, 1.6e-7."""
    full = _solid_angles(size, QUAD_CELLS)
    half = _solid_angles(size, QUAD_CELLS // 2)
    quad_err = abs(full.sum() - half.sum()) / (4 * np.pi)
    texel_err = (np.abs(full - half) / full).max()
    total = full.sum()
    print("size %d: sum / 4 pi - 1 = %.3e, the sum's own error by halving %.3e (one texel's: %.3e)" % (size, total / (4 * np.pi) - 1, quad_err, texel_err))
    assert quad_err * 4 <= SUM_TOL
    assert abs(total / (4 * np.pi) - 1) <= SUM_TOL
    # (b)
    image = random_image(size, 7 + size)
    image[image.sum(-1) == 0] = F(0.01)
    texels, cdf, _ = restate_table(image)
    k = np.arange(size * size)
    half_draw = np.full(len(k), 0.5, F)
    p = restate_sample_point(k, size, half_draw, half_draw)
    pdf, _ = _pdf(texels[:, 3], F(np.uint64(cdf[-1])), size, p)
    c = (np.arange(size) + 0.5) / size
    s, t = (a.reshape(-1) for a in np.meshgrid(c, c, indexing="xy"))
    sel = texels[:, 3].astype(np.float64) / float(F(np.uint64(cdf[-1])))
    worst = fd_err = 0.0
    for sign in (1.0, -1.0):
        jac = _jacobian_one_sided(s, t, 1e-5, sign)
        fd_err = max(fd_err, np.abs(_jacobian_one_sided(s, t, 2e-5, sign) / jac - 1).max())
        want = sel / (jac / size ** 2)
        worst = max(worst, np.abs(pdf.astype(np.float64) / want - 1).max())
    print("size %d: pdf against sel / Omega: worst %.3e, finite differences' own error by halving %.3e" % (size, worst, fd_err))
    assert fd_err * 4 + 16 * 2.0 ** -24 <= PDF_TOL
    assert worst <= PDF_TOL


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def test_every_rejection_in_its_order(harness):
    out = subprocess.run([harness, "checks"], capture_output=True, text=True)
    assert out.returncode == 0 and "checks OK" in out.stdout, out.stdout + out.stderr


def test_struct_layout_and_abi(rpt, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rpt.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %u\\n", '
                   'sizeof(rpt_environment), offsetof(rpt_environment, texels), offsetof(rpt_environment, scale), '
                   'offsetof(rpt_environment, mode), offsetof(rpt_environment, size), RPT_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A = rpt._abi
    E = A.rpt_environment
    assert got == [C.sizeof(E), E.texels.offset, E.scale.offset, E.mode.offset, E.size.offset, 5]
    assert (A.RPT_ENV_BACKGROUND_ONLY, A.RPT_ENV_SAMPLED) == (0, 1)


def test_entry_points_reject_what_they_can_without_a_gpu(rpt):
    """NULL ctx first, for both calls (no context can be made without a GPU: the rest of the order is the harness's)."""
    A = rpt._abi
    lib = rpt._lib.lib()
    env = A.rpt_environment()
    assert lib.rpt_set_environment(None, C.byref(env)) == A.RPT_ERR_INVALID_ARG
    assert b"rpt_set_environment: ctx is NULL" in lib.rpt_last_error(None)
    assert lib.rpt_set_environment(None, None) == A.RPT_ERR_INVALID_ARG
    e = C.c_int32(0)
    assert lib.rpt_download_environment_table(None, None, 0, C.byref(e)) == A.RPT_ERR_INVALID_ARG
    assert b"rpt_download_environment_table: ctx is NULL" in lib.rpt_last_error(None)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def test_octahedral_from_equirect_keeps_a_constant_image_and_the_axes(rpt):
    from rust_pathtracer_amd import scenes
    const = np.full((8, 16, 3), 0.25, F)
    out = scenes.octahedral_from_equirect(const, 5)
    assert out.shape == (5, 5, 3) and out.dtype == F and np.all(out == F(0.25))
    # a source whose six axis directions have six colours: top rows +y, bottom rows -y, the equator's four quarters around +-x, +-z
    h, w = 32, 64
    src = np.zeros((h, w, 3), F)
    src[:4] = (0, 1, 0)
    src[-4:] = (0, 0.5, 0)
    col = lambda u: int(u * w)                                      # noqa: E731  s = atan2(z, x) / 2 pi + 0.5
    for u, colour in ((0.5, (1, 0, 0)), (0.0, (0.5, 0, 0)), (0.999, (0.5, 0, 0)), (0.75, (0, 0, 1)), (0.25, (0, 0, 0.5))):
        src[12:20, max(col(u) - 3, 0):col(u) + 4] = colour
    size = 9
    out = scenes.octahedral_from_equirect(src, size)
    mid, last = size // 2, size - 1
    assert tuple(out[mid, mid]) == (0, 1, 0), "+y: the centre"
    assert tuple(out[mid, last]) == (1, 0, 0) and tuple(out[mid, 0]) == (0.5, 0, 0), "+x: row mid, the last column; -x: the first"
    assert tuple(out[last, mid]) == (0, 0, 1) and tuple(out[0, mid]) == (0, 0, 0.5), "+z: the last row; -z: the first"
    for j, i in ((0, 0), (0, last), (last, 0), (last, last)):
        assert tuple(out[j, i]) == (0, 0.5, 0), "-y: the four corners"
    # ... and the library's own lookup agrees with octahedral_directions about which texel a direction is
    d = scenes.octahedral_directions(size).reshape(-1, 3)
    k = restate_lookup(np.zeros((size * size, 4), F), size, 0, 1.0, d.astype(F))[0]
    assert np.array_equal(k, np.arange(size * size))


def test_mesh_env_scene(rpt):
    from rust_pathtracer_amd import scenes
    s, image = scenes.mesh_env_scene()
    assert image.shape == (64, 64, 3) and image.dtype == F and len(s.meshes) == 1 and not s.lights
    w = image.sum(-1)
    sun = w > 100
    assert 4 <= sun.sum() <= 40, "a sun a few texels wide"
    assert w[sun].sum() > 10 * w[~sun].sum(), "nearly all of the power is the sun's"


# ---- the code object library ----------------------------------------------------------------------------------------------------------
ENV_KERNELS = ["meshenv_block_kernel", "meshenv_cdf_kernel", "meshenv_quantise_kernel", "meshenv_query_kernel", "meshenv_regen_kernel",
               "meshenv_sample_kernel", "meshenv_weight_kernel"]
OTHER_LIBS = ("librpt_hip.so", "librpt_hip_test.so", "librpt_hip_mesh.so", "librpt_hip_refit.so", "librpt_hip_build.so", "librpt_hip_move.so",
              "librpt_hip_smooth.so", "librpt_hip_light.so", "librpt_hip_tex.so")


def test_the_environment_kernels_have_a_code_object_of_their_own():
    """librpt_hip_env.so (build.py, ENV_LIB) holds exactly the meshenv_* kernels and exports exactly its four launch functions; both
    libraries load it through their run path, and no other library holds a meshenv_ kernel."""
    assert sorted(code_object_kernels(os.path.join(PKG, "librpt_hip_env.so"))) == ENV_KERNELS
    for lib in OTHER_LIBS:
        assert not [n for n in code_object_kernels(os.path.join(PKG, lib)) if n.startswith("meshenv_")], lib
    for lib in ("librpt_hip.so", "librpt_hip_test.so"):
        dyn = subprocess.run(["readelf", "-d", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        assert "librpt_hip_env.so" in dyn and "$ORIGIN" in dyn, lib
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(PKG, "librpt_hip_env.so")], check=True, capture_output=True, text=True).stdout
    fns = sorted(line.split(" T ", 1)[1].split("(")[0] for line in out.splitlines() if " T " in line)
    assert fns == ["rptlaunch::env_query", "rptlaunch::env_sample", "rptlaunch::env_tables", "rptlaunch::render_mesh_env"], out
    for lib, hook in (("librpt_hip.so", False), ("librpt_hip_test.so", True)):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        for name in ("rpt_set_environment", "rpt_download_environment_table"):
            assert re.search(r" T %s$" % name, out, re.M), name
        for name in ("rpt_debug_env_query", "rpt_debug_env_sample"):
            assert bool(re.search(r" T %s$" % name, out, re.M)) == hook, lib


def test_build_py_names_the_environment_library(rpt):
    """build.py: env_lib_of beside the other eight, and needs_build's earlier positional parameters still mean what they meant."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_rpt_build_for_env_test", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.ENV_LIB == b.env_lib_of(b.LIB) == os.path.join(PKG, "librpt_hip_env.so")
    assert b.env_lib_of("/x/y/libz.so") == "/x/y/libz_env.so"
    assert any(o[0] == "k_env" and o[1] == "k_env.hip" and o[2] == b.PEROP and o[3] == "env" for o in b.OBJECTS)
    missing = os.path.join(PKG, "no_such_library.so")
    assert b.needs_build(b.LIB, b.MESH_LIB, b.REFIT_LIB, b.BUILD_LIB, b.MOVE_LIB, b.SMOOTH_LIB, b.LIGHT_LIB, missing) is True      # (the eighth is still tex_lib)
    assert b.needs_build(b.LIB, b.MESH_LIB, b.REFIT_LIB, b.BUILD_LIB, b.MOVE_LIB, b.SMOOTH_LIB, b.LIGHT_LIB, b.TEX_LIB, missing) is True
    assert b.needs_build(b.LIB, env_lib=missing) is True


def test_the_environment_kernels_use_no_scratch(tmp_path):
    """The kernels' metadata, read the way tools/kernel_meta.py reads it: no kernel of the library has a private segment or a spilled
    vector register; the table kernels spill nothing; the render kernel has mesh_regen_kernel's launch bounds."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
    fat, co = str(tmp_path / "fatbin"), str(tmp_path / "co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", os.path.join(PKG, "librpt_hip_env.so"), fat], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
    txt = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    blocks = txt.split("  - .agpr_count:")[1:]
    assert len(blocks) == len(ENV_KERNELS)
    seen = []
    for blk in blocks:
        g = lambda k: int(re.search(r"\.%s:\s*(\d+)" % k, blk).group(1))      # noqa: E731
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        seen.append(name)
        assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0, name
        if "regen" in name:
            assert g("max_flat_workgroup_size") == 256 and g("vgpr_count") <= 128, name      # 256 lanes, 4 waves per SIMD
        else:
            assert g("sgpr_spill_count") == 0, name
    assert sorted(n for s in seen for n in ENV_KERNELS if n in s) == ENV_KERNELS
