"""Mesh normal maps on the host (include/rpt.h, "mesh normal maps"; CPU only): csrc/host_nrm.h's checks answer in their order, its
decode and its bend equal a numpy float32 restatement bit for bit, every fall-back returns N's very bits, the bend agrees with an
independent float64 evaluation on well-conditioned inputs and has the geometry a normal map promises (tests/nrm_harness.cpp, a
stand-alone program built under g++'s address and undefined-behaviour sanitizers); rpt_mesh_normal_map has C's layout and the ABI
version did not move; the entry points reject what they can without a GPU; and the meshnrm_* kernels live in a code object library
of their own, none of which uses scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from kernel_census import code_object_kernels
from test_mesh_smooth_host import _cross, _dot
from test_mesh_texture_host import BILINEAR, CLAMP, NEAREST, REPEAT, restate_lookup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rust-pathtracer_amd")
F = np.float32
F32_MAX = F(3.40282347e+38)
STRENGTHS = (0.0, 1.0, 2.5)
# The largest angle between nrm_bend's float32 result and bend_f64 over test_the_bend_agrees_with_float64's well-conditioned inputs,
# measured with the numpy float32 restatement (not the harness): 2.88e-7 rad.  The test allows 4 x that for platform libm differences.
F64_ANGLE_MEASURED = 2.88e-7
F64_ANGLE_TOL = 4 * F64_ANGLE_MEASURED


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nrm") / "nrm_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "nrm_harness.cpp"), "-o", exe], check=True)
    return exe


# ---- the restatements (tests/test_gpu_mesh_normal_map.py imports them) -------------------------------------------------------------
def restate_decode(rgba, strength, flip):
    """include/rpt.h, "decode", on float32 arrays: [h, w, 4] uint8 -> [h, w, 4] f32 {sx*c(R), sy*c(G), c(B), 0}."""
    rgba = np.asarray(rgba, np.uint8)
    c = np.maximum((rgba[..., :3].astype(F) - F(128)) / F(127), F(-1))
    assert c.dtype == F
    sx = F(strength)
    sy = -sx if flip else sx
    out = np.zeros(rgba.shape[:2] + (4,), F)
    out[..., 0], out[..., 1], out[..., 2] = sx * c[..., 0], sy * c[..., 1], c[..., 2]
    return out


def restate_bend(N, e1, e2, uva, uvb, uvc, xyz):
    """include/rpt.h, "bend", per row of float32 arrays ([n, 3]; the UVs [n, 2] or [2]), one rounding per operation.
    -> (normals [n, 3] f32, which rows fell back to N, D, dot(B, B0))."""
    N, e1, e2, xyz = (np.ascontiguousarray(a, F).reshape(-1, 3) for a in (N, e1, e2, xyz))
    n = len(N)
    uva, uvb, uvc = (np.broadcast_to(np.ascontiguousarray(a, F), (n, 2)) for a in (uva, uvb, uvc))
    x, y, z = xyz[:, 0:1], xyz[:, 1:2], xyz[:, 2:3]
    with np.errstate(all="ignore"):
        du1, dv1 = uvb[:, 0] - uva[:, 0], uvb[:, 1] - uva[:, 1]
        du2, dv2 = uvc[:, 0] - uva[:, 0], uvc[:, 1] - uva[:, 1]
        D = du1 * dv2 - du2 * dv1
        g = np.where(D > 0, F(1), F(-1))[:, None]
        T0 = g * (e1 * dv2[:, None] - e2 * dv1[:, None])
        B0 = g * (e2 * du1[:, None] - e1 * du2[:, None])
        k = _dot(N, T0)
        T1 = T0 - N * k[:, None]
        t2 = _dot(T1, T1)
        T = T1 / np.sqrt(t2)[:, None]
        B = _cross(N, T)
        side = _dot(B, B0)
        B = np.where((side < 0)[:, None], -B, B)
        m = (x * T + y * B) + z * N
        m2 = _dot(m, m)
        out = m / np.sqrt(m2)[:, None]
    assert out.dtype == F and D.dtype == F and t2.dtype == F and m2.dtype == F
    ok = ~((xyz[:, 0] == 0) & (xyz[:, 1] == 0)) & ((D < 0) | (D > 0)) & (t2 > 0) & (t2 <= F32_MAX) & (m2 > 0) & (m2 <= F32_MAX)
    return np.where(ok[:, None], out, N), ~ok, D, side


def restate_shade(N, e1, e2, u, v, uva, uvb, uvc, texels, wrap, filt):
    """"lookup at the hit" and "bend": tex_interp with the triangle test's u and v, the lookup over the DECODED texels, the bend."""
    u, v = np.ascontiguousarray(u, F), np.ascontiguousarray(v, F)
    n = len(u)
    uva, uvb, uvc = (np.broadcast_to(np.ascontiguousarray(a, F), (n, 2)) for a in (uva, uvb, uvc))
    with np.errstate(all="ignore"):
        w = (F(1.0) - u) - v
        st = (w[:, None] * uva + u[:, None] * uvb) + v[:, None] * uvc
        assert st.dtype == F
        xyz = restate_lookup(texels, wrap, filt, st[:, 0], st[:, 1])
    return restate_bend(N, e1, e2, uva, uvb, uvc, xyz)


def bend_f64(N, e1, e2, uva, uvb, uvc, xyz):
    """The bend written independently in float64: the tangent is the surface's derivative by s — the solution of the 2 x 2 system,
    DIVIDED by its determinant, no sign select — made perpendicular to N; the bitangent is N x T on the side of the derivative by t."""
    N, e1, e2, xyz = (np.asarray(a, np.float64).reshape(-1, 3) for a in (N, e1, e2, xyz))
    n = len(N)
    uva, uvb, uvc = (np.broadcast_to(np.asarray(a, np.float64), (n, 2)) for a in (uva, uvb, uvc))
    d1, d2 = uvb - uva, uvc - uva
    det = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
    dPds = (e1 * d2[:, 1:2] - e2 * d1[:, 1:2]) / det[:, None]
    dPdt = (e2 * d1[:, 0:1] - e1 * d2[:, 0:1]) / det[:, None]
    T = dPds - N * (N * dPds).sum(1, keepdims=True)
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    B = np.cross(N, T)
    B *= np.sign((B * dPdt).sum(1, keepdims=True))
    m = xyz[:, 0:1] * T + xyz[:, 1:2] * B + xyz[:, 2:3] * N
    return m / np.linalg.norm(m, axis=1, keepdims=True), T, B


def random_bend_inputs(n, seed, mirrored=None):
    """n random (N, e1, e2, UVs, texel): N a unit normal within about 35 degrees of the facet's (as a smooth normal is), UVs in
    [-2, 2], texels of a decoded map.  `mirrored`: force the sign of D (None: both occur)."""
    rng = np.random.default_rng(seed)
    e1, e2 = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    g = np.cross(e1, e2)
    Nv = g / np.linalg.norm(g, axis=1, keepdims=True) + rng.normal(size=(n, 3)) * 0.25
    Nv /= np.linalg.norm(Nv, axis=1, keepdims=True)
    uv = rng.uniform(-2.0, 2.0, (n, 3, 2))
    if mirrored is not None:
        d1, d2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
        D = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
        swap = (D < 0) != mirrored
        uv[swap, 1], uv[swap, 2] = uv[swap, 2].copy(), uv[swap, 1].copy()
    xyz = restate_decode(rng.integers(0, 256, (n, 1, 4), dtype=np.uint8), 1.0, False)[:, 0, :3] * F(rng.choice([0.5, 1.0, 2.5]))
    return tuple(np.ascontiguousarray(a, F) for a in (Nv, e1, e2, uv[:, 0], uv[:, 1], uv[:, 2], xyz))


def _run(harness, mode, tmp_path, head, *blobs):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.uint32(head).tobytes())
        for b in blobs:
            f.write(np.ascontiguousarray(b).tobytes())
    r = subprocess.run([harness, mode, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == mode + " OK", r.stdout + r.stderr
    return np.fromfile(dst, F)


def _run_bend(harness, tmp_path, N, e1, e2, uva, uvb, uvc, xyz):
    n = len(N)
    rows = np.concatenate([np.asarray(a, F).reshape(n, -1) for a in (N, e1, e2, uva, uvb, uvc, xyz)], 1)
    assert rows.shape == (n, 18)
    return _run(harness, "bend", tmp_path, [n], rows).reshape(n, 3)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the tests ---------------------------------------------------------------------------------------------------------------------
def test_host_checks_in_their_order(harness):
    r = subprocess.run([harness, "checks"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "checks OK", r.stdout + r.stderr


def test_host_decode_equals_the_numpy_restatement(harness, tmp_path):
    """All 256 bytes in every channel x {strength 0, 1, 2.5} x flip, bit for bit; and the stated exact values."""
    every = np.zeros((1, 256, 4), np.uint8)
    every[0, :, 0], every[0, :, 1], every[0, :, 2], every[0, :, 3] = np.arange(256), np.arange(256)[::-1], np.roll(np.arange(256), 77), 9
    for strength in STRENGTHS:
        for flip in (False, True):
            got = _run(harness, "decode", tmp_path, [256, 1 if flip else 0], F(strength), every).reshape(1, 256, 4)
            want = restate_decode(every, strength, flip)
            assert np.array_equal(_bits(got), _bits(want)), (strength, flip, int((_bits(got) != _bits(want)).sum()))
            assert not got[..., 3].any()
    one = restate_decode(every, 1.0, False)[0]
    assert one[128, 0] == 0 and one[255, 0] == 1 and one[0, 0] == -1 and one[1, 0] == -1 and one[2, 0] > -1
    assert np.array_equal(restate_decode(every, 1.0, True)[0, :, 1], -one[:, 1]) and np.array_equal(restate_decode(every, 1.0, True)[0, :, 0], one[:, 0])
    assert np.array_equal(restate_decode(every, 2.5, False)[0, :, 2], one[:, 2]), "z is not scaled"
    assert not restate_decode(every, 0.0, True)[0, :, :2].any(), "strength 0: x == y == 0 everywhere"


def test_host_bend_equals_the_numpy_restatement(harness, tmp_path):
    """6000 random inputs, D of both signs, bit for bit; no random input falls back."""
    ins = [np.concatenate(p) for p in zip(random_bend_inputs(3000, 41, mirrored=False), random_bend_inputs(3000, 42, mirrored=True))]
    got = _run_bend(harness, tmp_path, *ins)
    want, fell, D, side = restate_bend(*ins)
    bad = np.nonzero((_bits(got) != _bits(want)).any(axis=1))[0]
    assert len(bad) == 0, "%d rows differ, first %s: got %s want %s" % (len(bad), bad[:3], got[bad[:3]], want[bad[:3]])
    assert (D[:3000] > 0).all() and (D[3000:] < 0).all() and (fell.mean() < 0.01), "mirrored UVs occur and the rows are bent"
    assert np.allclose(np.linalg.norm(want[~fell].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert (np.abs(want - ins[0]).max(axis=1) > 1e-3).mean() > 0.9


@pytest.mark.parametrize("wrap", [REPEAT, CLAMP])
@pytest.mark.parametrize("filt", [NEAREST, BILINEAR])
def test_host_shade_equals_the_numpy_restatement(harness, tmp_path, wrap, filt):
    """The whole of lookup and bend through nrm_shade, over a 5 x 3 decoded map, bit for bit."""
    n = 2000
    N, e1, e2, uva, uvb, uvc, _ = random_bend_inputs(n, 50 + 2 * wrap + filt)
    texels = restate_decode(np.random.default_rng(7).integers(0, 256, (3, 5, 4), dtype=np.uint8), 2.5, True)
    bary = np.random.default_rng(8).dirichlet([1, 1, 1], n).astype(F)
    u, v = bary[:, 1].copy(), bary[:, 2].copy()
    rows = np.concatenate([N, e1, e2, u[:, None], v[:, None], uva, uvb, uvc], 1).astype(F)
    got = _run(harness, "shade", tmp_path, [5, 3, wrap, filt, n], texels, rows).reshape(n, 3)
    want = restate_shade(N, e1, e2, u, v, uva, uvb, uvc, texels, wrap, filt)[0]
    assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).any(axis=1).sum())


def test_every_fall_back_returns_ns_very_bits(harness, tmp_path):
    """x == y == 0 (with either zero's sign); D == 0; collinear UVs; T0 parallel to N; overflowing edges (NaN); a zero m."""
    N0 = np.array([0.6, 0.0, 0.8], F)                                # unit in float32 up to rounding; its bits are what must come back
    flat_e1, flat_e2 = np.array([1, 0, 0], F), np.array([0, 1, 0], F)
    uv = np.array([[0, 0], [1, 0], [0, 1]], F)
    big = F(3e38)
    cases = [
        ("x == y == 0", N0, flat_e1, flat_e2, uv, [0.0, 0.0, 1.0]),
        ("x == y == -0", N0, flat_e1, flat_e2, uv, [-0.0, -0.0, 0.5]),
        ("x == +0, y == -0, z == 0", N0, flat_e1, flat_e2, uv, [0.0, -0.0, 0.0]),
        ("D == 0: two corners share a UV", N0, flat_e1, flat_e2, np.array([[0.25, 0.5], [0.25, 0.5], [1, 1]], F), [0.5, 0.5, 1.0]),
        ("D == 0: all corners share a UV", N0, flat_e1, flat_e2, np.array([[0.25, 0.5]] * 3, F), [0.5, 0.5, 1.0]),
        ("collinear UVs", N0, flat_e1, flat_e2, np.array([[0, 0], [0.5, 0.25], [1, 0.5]], F), [0.5, 0.5, 1.0]),
        ("T0 parallel to N", np.array([1, 0, 0], F), flat_e1, flat_e2, uv, [0.5, 0.5, 1.0]),
        ("overflowing edges: T0 is inf - inf", N0, np.array([big, big, 0], F), np.array([big, 0, big], F), np.array([[0, 0], [2, 2], [-2, 2]], F), [0.5, 0.5, 1.0]),
        ("NaN UV", N0, flat_e1, flat_e2, np.array([[0, 0], [np.nan, 0], [0, 1]], F), [0.5, 0.5, 1.0]),
        ("a zero m", np.array([0, 0, 1], F), flat_e1, flat_e2, uv, [1e-30, 0.0, 0.0]),
        ("an overflowing m", np.array([0, 0, 1], F), flat_e1, flat_e2, uv, [2e19, 2e19, 2e19]),
    ]
    rows = [np.concatenate([np.asarray(c[1], F), c[2], c[3], np.asarray(c[4], F).reshape(-1), np.asarray(c[5], F)]) for c in cases]
    cols = np.stack(rows)
    args = (cols[:, 0:3], cols[:, 3:6], cols[:, 6:9], cols[:, 9:11], cols[:, 11:13], cols[:, 13:15], cols[:, 15:18])
    got = _run_bend(harness, tmp_path, *args)
    want, fell, _, _ = restate_bend(*args)
    for k, c in enumerate(cases):
        assert fell[k], c[0] + ": the restatement falls back"
        assert np.array_equal(_bits(got[k]), _bits(c[1])), "%s: got %s, N is %s" % (c[0], got[k], c[1])
    assert np.array_equal(_bits(got), _bits(want))
    # and next to each: the smallest change that bends
    ok = _run_bend(harness, tmp_path, N0[None], flat_e1[None], flat_e2[None], uv[0][None], uv[1][None], uv[2][None], np.array([[1e-30, 0.0, 1.0]], F))
    assert np.array_equal(_bits(ok), _bits(restate_bend(N0, flat_e1, flat_e2, uv[0], uv[1], uv[2], np.array([[1e-30, 0.0, 1.0]], F))[0]))


def _well_conditioned(N, e1, e2, uva, uvb, uvc, xyz):
    """The rows the float64 comparison keeps.  In float64: |D| at least 0.1 of the sum of its two terms' magnitudes (the subtraction
    loses at most 3.4 bits); |T1|^2 at least 0.1 of |T0|^2 (the tangent lies at least 18 degrees off N); |dot(B, B0)| at least 0.1 of
    |B0| (the handedness is not a near tie); and x or y above 2^-7 (the texel is not flat)."""
    N, e1, e2, uva, uvb, uvc, xyz = (np.asarray(a, np.float64) for a in (N, e1, e2, uva, uvb, uvc, xyz))
    d1, d2 = uvb - uva, uvc - uva
    a, b = d1[:, 0] * d2[:, 1], d2[:, 0] * d1[:, 1]
    D = a - b
    T0 = e1 * d2[:, 1:2] - e2 * d1[:, 1:2]
    B0 = (e2 * d1[:, 0:1] - e1 * d2[:, 0:1]) * np.sign(D)[:, None]
    T1 = T0 - N * (N * T0).sum(1, keepdims=True)
    t2 = (T1 * T1).sum(1)
    B = np.cross(N, T1 / np.sqrt(np.maximum(t2, 1e-300))[:, None] * np.sign(D)[:, None])
    return ((np.abs(D) >= 0.1 * (np.abs(a) + np.abs(b))) & (t2 >= 0.1 * (T0 * T0).sum(1)) &
            (np.abs((B * B0).sum(1)) >= 0.1 * np.linalg.norm(B0, axis=1)) & (np.abs(xyz[:, :2]).max(1) > 2.0 ** -7))


def test_the_bend_agrees_with_float64(harness, tmp_path):
    """Against bend_f64 on the well-conditioned rows of 8000 random inputs (see _well_conditioned).  The largest angle between the
    numpy float32 restatement and the float64 evaluation measures 2.88e-7 rad (F64_ANGLE_MEASURED: about 2.4 float32 ulps of a unit
    vector's component); the harness is allowed 4 x that."""
    ins = [np.concatenate(p) for p in zip(random_bend_inputs(4000, 61), random_bend_inputs(4000, 62))]
    keep = _well_conditioned(*ins)
    assert 0.4 < keep.mean() < 0.95, keep.mean()
    ins = [a[keep] for a in ins]
    want = bend_f64(*ins)[0]

    def angle(a):
        a = np.asarray(a, np.float64)
        return np.arctan2(np.linalg.norm(np.cross(a, want), axis=1), (a * want).sum(1))

    restated, fell, _, _ = restate_bend(*ins)
    assert not fell.any()
    measured = angle(restated).max()
    print("largest angle between the float32 restatement and float64: %.3g rad over %d rows" % (measured, len(want)))
    assert measured <= F64_ANGLE_MEASURED * 1.001, "the recorded measurement is the restatement's on these inputs"
    got = _run_bend(harness, tmp_path, *ins)
    assert angle(got).max() <= F64_ANGLE_TOL, angle(got).max()


def test_the_bend_has_a_normal_maps_geometry():
    """In float64, and for the float32 restatement within 1e-5: T is perpendicular to N; (0, 0, 1) texels give N; a pure +x texel tilts
    the normal toward increasing s; FLIP_GREEN mirrors the tilt in t."""
    N, e1, e2, uva, uvb, uvc, xyz = random_bend_inputs(3000, 71)
    keep = _well_conditioned(N, e1, e2, uva, uvb, uvc, np.ones_like(xyz))
    N, e1, e2, uva, uvb, uvc = (a[keep] for a in (N, e1, e2, uva, uvb, uvc))
    n = len(N)
    N64 = N.astype(np.float64)
    N64 /= np.linalg.norm(N64, axis=1, keepdims=True)

    def both(texel):
        t = np.tile(np.asarray(texel, F), (n, 1))
        r64, T, B = bend_f64(N64, e1, e2, uva, uvb, uvc, t)
        r32 = restate_bend(N, e1, e2, uva, uvb, uvc, t)[0]
        assert np.abs(r32 - r64).max() < 1e-5
        return r64, T, B

    up, T, B = both([0.0, 0.0, 1.0])
    assert np.abs((T * N64).sum(1)).max() < 1e-12 and np.abs((B * N64).sum(1)).max() < 1e-12 and np.abs((T * B).sum(1)).max() < 1e-12
    assert np.abs(up - N64).max() < 1e-12
    assert np.array_equal(_bits(restate_bend(N, e1, e2, uva, uvb, uvc, np.tile(F([0, 0, 1]), (n, 1)))[0]), _bits(N)), "bit for bit in float32"
    # the surface point as a function of (s, t): P = a + dPds * (s - sa) + dPdt * (t - ta); the tilt's component along dPds is positive
    d1, d2 = (uvb - uva).astype(np.float64), (uvc - uva).astype(np.float64)
    det = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
    dPds = (e1 * d2[:, 1:2] - e2 * d1[:, 1:2]) / det[:, None]
    dPdt = (e2 * d1[:, 0:1] - e1 * d2[:, 0:1]) / det[:, None]

    def tilt(r):                                                     # the part of the bent normal that lies in N's plane
        return r - N64 * (r * N64).sum(1, keepdims=True)

    px = both([0.5, 0.0, 1.0])[0]
    assert ((tilt(px) * dPds).sum(1) > 0).all() and np.abs((tilt(px) * B).sum(1)).max() < 1e-12, "+x tilts toward increasing s, and only so"
    py = both([0.0, 0.5, 1.0])[0]
    assert ((tilt(py) * dPdt).sum(1) > 0).all() and np.abs((tilt(py) * T).sum(1)).max() < 1e-12, "+y tilts toward increasing t"
    flipped = both(restate_decode(np.array([[[128, 192, 255, 0]]], np.uint8), 1.0, True)[0, 0, :3])[0]
    plain = both(restate_decode(np.array([[[128, 192, 255, 0]]], np.uint8), 1.0, False)[0, 0, :3])[0]
    assert ((tilt(plain) * dPdt).sum(1) > 0).all() and ((tilt(flipped) * dPdt).sum(1) < 0).all(), "FLIP_GREEN mirrors the tilt in t"
    assert np.abs(tilt(plain) + tilt(flipped)).max() < 1e-12


def test_rpt_mesh_normal_map_layout_matches_c(rpt, tmp_path):
    prog = tmp_path / "nrm_layout.c"
    fields = ("mesh", "mode", "width", "height", "texels", "filter", "flags", "strength")
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "rpt.h"
int main(void) {
  printf("size %zu\n", sizeof(rpt_mesh_normal_map)); printf("abi %u\n", RPT_ABI_VERSION); printf("desc %zu\n", sizeof(rpt_scene_desc));
  printf("tex %zu\n", sizeof(rpt_mesh_texture)); printf("cut %zu\n", sizeof(rpt_mesh_cutout));
  printf("consts %d\n", RPT_MESH_NORMAL_MAP_OFF * 100 + RPT_MESH_NORMAL_MAP_ON * 10 + RPT_NORMAL_MAP_FLIP_GREEN);
''' + "".join('  printf("%s %%zu\\n", offsetof(rpt_mesh_normal_map, %s));\n' % (f, f) for f in fields) + "  return 0; }")
    exe = tmp_path / "nrm_layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    A = rpt._abi
    assert C.sizeof(A.rpt_mesh_normal_map) == int(out["size"]) == 40
    for f in fields:
        assert getattr(A.rpt_mesh_normal_map, f).offset == int(out[f]), f
    assert int(out["consts"]) == 11 and (A.RPT_MESH_NORMAL_MAP_OFF, A.RPT_MESH_NORMAL_MAP_ON, A.RPT_NORMAL_MAP_FLIP_GREEN) == (0, 1, 1)
    assert int(out["abi"]) == A.RPT_ABI_VERSION == 5                  # additive: the ABI version did not move
    assert int(out["desc"]) == C.sizeof(A.rpt_scene_desc) == rpt.lib().rpt_sizeof_scene_desc()
    assert int(out["tex"]) == C.sizeof(A.rpt_mesh_texture) == 48 and int(out["cut"]) == C.sizeof(A.rpt_mesh_cutout) == 32


def test_the_normal_map_calls_are_declared_exported_and_mirrored(rpt):
    A = rpt._abi
    header = open(os.path.join(ROOT, "include", "rpt.h")).read()
    hooks = open(os.path.join(ROOT, "include", "rpt_test.h")).read()
    for name in ("rpt_set_mesh_normal_maps", "rpt_download_mesh_normal_map"):
        assert re.search(r"^int %s\(rpt_ctx\*" % name, header, re.M) and name in A.SYMBOLS and name not in A.TEST_SYMBOLS, name
    assert re.search(r"^int rpt_debug_mesh_normal_map_query\(rpt_ctx\*", hooks, re.M) and "rpt_debug_mesh_normal_map_query" not in header
    assert "rpt_debug_mesh_normal_map_query" in A.TEST_SYMBOLS and "rpt_debug_mesh_normal_map_query" not in A.SYMBOLS
    assert "mesh normal maps — PROJECT-DEFINED" in header and "csrc/host_nrm.h" in header
    assert header.index("mesh cutouts — PROJECT-DEFINED") < header.index("mesh normal maps — PROJECT-DEFINED") < header.index("Tracer::render (tracer.rs")
    for lib, hook in (("librpt_hip.so", False), ("librpt_hip_test.so", True)):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        for name in ("rpt_set_mesh_normal_maps", "rpt_download_mesh_normal_map"):
            assert re.search(r" T %s$" % name, out, re.M), (lib, name)
        assert bool(re.search(r" T rpt_debug_mesh_normal_map_query$", out, re.M)) == hook, lib
        assert len(re.findall(r"normal_map", out)) == (3 if hook else 2), lib
    hpp = open(os.path.join(ROOT, "include", "rpt.hpp")).read()
    assert "rpt_set_mesh_normal_maps(ctx_" in hpp and "rpt_download_mesh_normal_map(ctx_" in hpp
    assert hasattr(rpt.Tracer, "set_mesh_normal_maps") and hasattr(rpt.Tracer, "mesh_normal_map")


def test_the_normal_map_calls_validate_without_gpu(rpt):
    """The NULL context answers before anything else, and says which call it was."""
    lib, A = rpt.lib(), rpt._abi
    items = (A.rpt_mesh_normal_map * 1)()
    out = np.zeros(4, F)
    for name, call in (("rpt_set_mesh_normal_maps", lambda: lib.rpt_set_mesh_normal_maps(None, items, 1)),
                       ("rpt_download_mesh_normal_map", lambda: lib.rpt_download_mesh_normal_map(None, 0, out.ctypes.data, 1, 1))):
        assert call() == A.RPT_ERR_INVALID_ARG, name
        assert lib.rpt_last_error(None).startswith(name.encode() + b": "), name
    assert lib.rpt_set_mesh_normal_maps(None, None, 0) == A.RPT_ERR_INVALID_ARG      # the NULL context comes before n_items == 0
    assert lib.rpt_debug_mesh_normal_map_query(None, None, 0, None, 0, None) == A.RPT_ERR_INVALID_ARG


def test_the_python_wrapper_checks_its_arguments(rpt):
    with pytest.raises(ValueError):
        rpt.Tracer.set_mesh_normal_maps(object(), {0: np.zeros((2, 2), np.uint8)})       # a height field, not an RGBA map
    with pytest.raises(ValueError):
        rpt.Tracer.set_mesh_normal_maps(object(), {0: np.zeros((2, 2, 3), np.uint8)})
    with pytest.raises(ValueError):
        rpt.Tracer.set_mesh_normal_maps(object(), {0: dict(texels=np.zeros((2, 2, 4), np.uint8), filter="trilinear")})


def test_the_scene_helpers_are_what_the_tests_need(rpt):
    from rust_pathtracer_amd import scenes
    flat = scenes.height_to_normal_map(np.zeros((3, 5), F), 1.0)
    assert flat.shape == (3, 5, 4) and flat.dtype == np.uint8 and (flat == np.array([128, 128, 255, 255], np.uint8)).all()
    ramp = scenes.height_to_normal_map(np.tile(np.arange(8, dtype=F) / 8, (4, 1)), 2.0)     # the height rises with s
    d = restate_decode(ramp, 1.0, False)
    assert (d[:, 1:-1, 0] < 0).all() and (d[..., 1] == 0).all() and (d[..., 2] > 0).all(), "the normal leans against the slope"
    assert np.allclose(np.linalg.norm(d[:, 1:-1, :3].astype(np.float64), axis=2), 1.0, atol=0.02)
    steeper = restate_decode(scenes.height_to_normal_map(np.tile(np.arange(8, dtype=F) / 8, (4, 1)), 8.0), 1.0, False)
    assert (steeper[:, 1:-1, 0] < d[:, 1:-1, 0]).all()
    s, uvs, nmap = scenes.mesh_normal_map_scene()
    base, base_uvs = scenes.mesh_texture_scene()
    assert len(s.meshes) == len(base.meshes) == len(uvs) == 2 and all(np.array_equal(a, b) for a, b in zip(uvs, base_uvs))
    assert nmap.ndim == 3 and nmap.shape[2] == 4 and nmap.dtype == np.uint8
    dd = restate_decode(nmap, 1.0, False).astype(np.float64)
    tilt = np.degrees(np.arctan2(np.hypot(dd[..., 0], dd[..., 1]), dd[..., 2]))
    assert 5.0 < tilt.max() < 40.0 and (dd[..., 2] > 0).all(), "a bump map: tilted, never past the horizon"


NRM_KERNELS = ["meshnrm_cut_env_regen_kernel", "meshnrm_cut_regen_kernel", "meshnrm_decode_kernel", "meshnrm_env_regen_kernel", "meshnrm_query_kernel",
               "meshnrm_regen_kernel"]
OTHER_LIBS = ("librpt_hip.so", "librpt_hip_test.so", "librpt_hip_mesh.so", "librpt_hip_refit.so", "librpt_hip_build.so", "librpt_hip_move.so",
              "librpt_hip_smooth.so", "librpt_hip_light.so", "librpt_hip_tex.so", "librpt_hip_env.so", "librpt_hip_cut.so")


def test_the_normal_map_kernels_have_a_code_object_of_their_own():
    """librpt_hip_nrm.so (build.py, NRM_LIB) holds exactly the meshnrm_* kernels and exports exactly its six launch functions; both
    libraries load it through their run path, and no other library holds a meshnrm_ kernel."""
    assert sorted(code_object_kernels(os.path.join(PKG, "librpt_hip_nrm.so"))) == NRM_KERNELS
    for lib in OTHER_LIBS:
        assert not [n for n in code_object_kernels(os.path.join(PKG, lib)) if n.startswith("meshnrm_")], lib
    for lib in ("librpt_hip.so", "librpt_hip_test.so"):
        dyn = subprocess.run(["readelf", "-d", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        assert "librpt_hip_nrm.so" in dyn and "$ORIGIN" in dyn, lib
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(PKG, "librpt_hip_nrm.so")], check=True, capture_output=True, text=True).stdout
    fns = sorted(line.split(" T ", 1)[1].split("(")[0] for line in out.splitlines() if " T " in line)
    assert fns == ["rptlaunch::mesh_normal_map_query", "rptlaunch::nrm_decode", "rptlaunch::render_mesh_nrm", "rptlaunch::render_mesh_nrm_cut",
                   "rptlaunch::render_mesh_nrm_cut_env", "rptlaunch::render_mesh_nrm_env"], out


def test_build_py_names_the_normal_map_library(rpt):
    """build.py: nrm_lib_of beside the other ten, and needs_build's earlier positional parameters still mean what they meant."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_rpt_build_for_nrm_test", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.NRM_LIB == b.nrm_lib_of(b.LIB) == os.path.join(PKG, "librpt_hip_nrm.so")
    assert b.nrm_lib_of("/x/y/libz.so") == "/x/y/libz_nrm.so"
    assert any(o[0] == "k_nrm" and o[1] == "k_nrm.hip" and o[2] == b.PEROP and o[3] == "nrm" for o in b.OBJECTS)
    missing = os.path.join(PKG, "no_such_library.so")
    assert b.needs_build(b.LIB, b.MESH_LIB, b.REFIT_LIB, b.BUILD_LIB, b.MOVE_LIB, b.SMOOTH_LIB, b.LIGHT_LIB, b.TEX_LIB, b.ENV_LIB, missing) is True     # (the tenth is still cut_lib)
    assert b.needs_build(b.LIB, b.MESH_LIB, b.REFIT_LIB, b.BUILD_LIB, b.MOVE_LIB, b.SMOOTH_LIB, b.LIGHT_LIB, b.TEX_LIB, b.ENV_LIB, b.CUT_LIB, missing) is True
    assert b.needs_build(b.LIB, nrm_lib=missing) is True


def test_the_normal_map_kernels_use_no_scratch(tmp_path):
    """The kernels' metadata, read the way tools/kernel_meta.py reads it: no kernel of the library has a private segment or a spilled
    vector register; the decode kernel needs no LDS and spills nothing; the four render kernels have mesh_regen_kernel's launch bounds
    and fit four waves per SIMD."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
    fat, co = str(tmp_path / "fatbin"), str(tmp_path / "co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", os.path.join(PKG, "librpt_hip_nrm.so"), fat], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
    txt = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    blocks = txt.split("  - .agpr_count:")[1:]
    assert len(blocks) == len(NRM_KERNELS)
    seen, regen = [], 0
    for blk in blocks:
        g = lambda k: int(re.search(r"\.%s:\s*(\d+)" % k, blk).group(1))      # noqa: E731
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        seen.append(name)
        assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0, name
        if "regen" in name:
            regen += 1
            assert g("max_flat_workgroup_size") == 256 and g("vgpr_count") <= 128, name      # 256 lanes, 4 waves per SIMD
        elif "decode" in name:
            assert g("sgpr_spill_count") == 0 and g("group_segment_fixed_size") == 0, name
    assert regen == 4 and sorted(n for s in seen for n in NRM_KERNELS if n in s.split("N8rptscene")[0]) == NRM_KERNELS
