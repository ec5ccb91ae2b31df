"""Smooth mesh shading on the host (include/rpt.h, "smooth mesh shading"; CPU only): csrc/host_smooth.h's adjacency and its reference of
both normal statements equal a numpy float32 restatement bit for bit, and its checks answer in their order (under g++'s address and
undefined-behaviour sanitizers: tests/smooth_harness.cpp); rpt_mesh_shading has C's layout and the ABI version did not move; the
two entry points reject what they can without a GPU; and the meshsmooth_* kernels live in a code object library of their own, whose
two table passes use no scratch."""
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
F32_MAX = F(3.40282347e38)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("smooth") / "smooth_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "smooth_harness.cpp"), "-o", exe], check=True)
    return exe


# ---- the numpy float32 restatement (tests/test_gpu_mesh_smooth.py imports it) ------------------------------------------------------
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def incidence(idx, n_vertices):
    """-> (vertex, triangle) of every pair "triangle names vertex at one or more corners", each once, sorted by vertex, then
    triangle; and each pair's rank within its vertex's list."""
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    m = max(len(idx), 1)
    key = np.unique(idx.ravel() * m + np.repeat(np.arange(len(idx)), 3))
    vert, tri = key // m, key % m
    first = np.searchsorted(vert, np.arange(n_vertices))
    return vert, tri, np.arange(len(vert)) - first[vert]


def restate_vertex_normals(v, idx):
    """include/rpt.h's vertex normals of one SMOOTH mesh on float32 arrays, one rounding per operation: [n, 3] f32."""
    v = np.ascontiguousarray(v, F).reshape(-1, 3)
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    s = np.zeros((len(v), 3), F)
    with np.errstate(all="ignore"):
        if len(idx):
            a, b, c = v[idx[:, 0]], v[idx[:, 1]], v[idx[:, 2]]
            g = _cross(b - a, c - a)
            vert, tri, rank = incidence(idx, len(v))
            for r in range(int(rank.max()) + 1):                      # left to right, starting with the first term
                sel = rank == r
                s[vert[sel]] = g[tri[sel]] if r == 0 else s[vert[sel]] + g[tri[sel]]
        l2 = _dot(s, s)
        ok = (l2 > 0) & (l2 <= F32_MAX)
        n = s / np.sqrt(l2)[:, None]
    assert n.dtype == F
    return np.where(ok[:, None], n, F(0))


def restate_hit_normals(o, d, a, e1, e2, na, nb, nc):
    """include/rpt.h's normal of a winning triangle of a SMOOTH mesh, per row of the [n, 3] f32 arrays: u and v of the triangle
    test, the interpolation, the fall-back to the flat normal.  -> (normals [n, 3] f32, which rows fell back)."""
    o, d, a, e1, e2, na, nb, nc = (np.ascontiguousarray(x, F) for x in (o, d, a, e1, e2, na, nb, nc))
    with np.errstate(all="ignore"):
        p = _cross(d, e2)
        inv = F(1.0) / _dot(e1, p)
        sv = o - a
        u = _dot(sv, p) * inv
        v = _dot(d, _cross(sv, e1)) * inv
        w = (F(1.0) - u) - v
        m = (w[:, None] * na + u[:, None] * nb) + v[:, None] * nc
        l2 = _dot(m, m)
        ok = (l2 > 0) & (l2 <= F32_MAX)
        smooth = m / np.sqrt(l2)[:, None]
        g = _cross(e1, e2)
        flat = g / np.sqrt(_dot(g, g))[:, None]
    assert smooth.dtype == F and flat.dtype == F
    return np.where(ok[:, None], smooth, flat), ~ok


# ---- the meshes both test files use ---------------------------------------------------------------------------------------------------
def fan(valence=300):
    """A fan around a hub (vertex 0) of `valence` triangles, not flat: the hub's list is longer than a wave and a workgroup."""
    k = np.arange(valence + 1)
    ang = k * (2.0 * np.pi / (valence + 1)) * 0.9
    rim = np.stack([np.cos(ang), np.sin(ang), 0.1 * np.sin(5.0 * ang) - 0.3], 1)
    v = np.concatenate([[[0.0, 0.0, 0.0]], rim]).astype(F)
    t = np.stack([np.zeros(valence, np.int64), 1 + k[:-1], 2 + k[:-1]], 1).astype(np.uint32)
    return v, t


def grid(n_vertices, seed):
    """A bumpy strip of exactly `n_vertices` vertices (two rows; an odd count leaves the last vertex unused by the strip's quads and
    closes with one more triangle)."""
    rng = np.random.default_rng(seed)
    cols = n_vertices // 2
    x = np.arange(cols) * 0.05
    v = np.concatenate([np.stack([x, np.zeros(cols), rng.uniform(-0.02, 0.02, cols)], 1),
                        np.stack([x, np.full(cols, 0.07), rng.uniform(-0.02, 0.02, cols)], 1)])
    i = np.arange(cols - 1)
    t = np.concatenate([np.stack([i, i + 1, cols + i], 1), np.stack([i + 1, cols + i + 1, cols + i], 1)])
    if n_vertices % 2:
        v = np.concatenate([v, [[x[-1] + 0.05, 0.035, 0.01]]])
        t = np.concatenate([t, [[cols - 1, n_vertices - 1, 2 * cols - 1]]])
    assert len(v) == n_vertices
    return v.astype(F), t.astype(np.uint32)


def edge_meshes():
    """[(what, vertices, indices)]: the cases include/rpt.h's statement has to get right beyond a closed surface."""
    out = [("a fan whose hub has valence 300",) + fan(300)]
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], F)
    out.append(("a vertex no triangle names", v, np.array([[0, 1, 2]], np.uint32)))
    v = np.array([[0.25, 0.5, 0.125], [1.5, 0.5, 0.25], [0.25, 1.75, 0.5]], F)
    out.append(("two coincident triangles of opposite winding", v, np.array([[0, 1, 2], [0, 2, 1]], np.uint32)))
    v = np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, 0.25], [1, 1, 0]], F)
    out.append(("a triangle naming one vertex twice", v, np.array([[0, 1, 2], [1, 1, 3], [3, 2, 3], [1, 3, 2]], np.uint32)))
    out.append(("exactly 256 vertices",) + grid(256, 11))
    out.append(("257 vertices",) + grid(257, 12))
    return out


def _base_meshes():
    from test_gpu_mesh import _test_scene
    return [("base mesh %d" % k, np.asarray(v, F), np.asarray(t, np.uint32)) for k, (v, t, _) in enumerate(_test_scene().meshes)]


def _run_normals(harness, tmp_path, meshes, modes):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.uint32([len(meshes)]).tobytes())
        for (v, t), mode in zip(meshes, modes):
            f.write(np.uint32([len(v), len(t), mode]).tobytes())
            f.write(np.ascontiguousarray(v, F).tobytes())
            f.write(np.ascontiguousarray(t, np.uint32).tobytes())
    r = subprocess.run([harness, "normals", src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "normals OK", r.stdout + r.stderr
    raw = np.fromfile(dst, np.uint32)
    n_faces, n_adj, n_vertices = (int(x) for x in raw[:3])
    at = 3
    parts = []
    for count in (3 * n_faces, n_vertices + 1, n_adj, (sum(len(t) for _, t in meshes) + 31) // 32, 4 * n_vertices):
        parts.append(raw[at:at + count])
        at += count
    assert at == len(raw)
    face_vertex, adj_first, adj, bits, normals = parts
    return face_vertex.reshape(3, n_faces), adj_first, adj, bits, normals.view(F).reshape(-1, 4)


@pytest.mark.parametrize("scale_exp", [0, -20, 20, -40, 40])
def test_adjacency_and_normals_equal_the_numpy_restatement(rpt, harness, tmp_path, scale_exp):
    """Every mesh of the GPU tests in one scene, every second one SMOOTH and then the others: the adjacency lists each vertex's
    triangles once, ascending; the normals are the restatement's words; FLAT meshes' vertices hold zeros."""
    scale = F(2.0 ** scale_exp)
    named = _base_meshes() + edge_meshes()
    meshes = [(v * scale, t) for _, v, t in named]
    for parity in (0, 1):
        modes = [1 if k % 2 == parity else 0 for k in range(len(meshes))]
        face_vertex, adj_first, adj, bits, normals = _run_normals(harness, tmp_path, meshes, modes)
        first_v = np.concatenate([[0], np.cumsum([len(v) for v, _ in meshes])])
        first_t = np.concatenate([[0], np.cumsum([len(t) for _, t in meshes])])
        assert np.array_equal(normals[:, 3].view(np.uint32), np.zeros(len(normals), np.uint32))
        face0 = 0
        for k, ((v, t), mode) in enumerate(zip(meshes, modes)):
            what = "%s at scale 2^%d" % (named[k][0], scale_exp)
            got = normals[first_v[k]:first_v[k + 1], :3]
            flag = [(int(bits[i >> 5]) >> (i & 31)) & 1 for i in range(first_t[k], first_t[k + 1])]
            assert flag == [mode] * len(t), what
            if not mode:
                assert not got.view(np.uint32).any() and (np.diff(adj_first[first_v[k]:first_v[k + 1] + 1]) == 0).all(), what
                continue
            want = restate_vertex_normals(v, t)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s: %d words differ" % (what, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
            # the adjacency: the mesh's triangles are faces face0 .. in order; each vertex's list is the restatement's incidence
            assert np.array_equal(face_vertex[:, face0:face0 + len(t)].T, t.astype(np.int64) + first_v[k]), what
            vert, tri, _ = incidence(t, len(v))
            lo, hi = adj_first[first_v[k]], adj_first[first_v[k + 1]]
            assert np.array_equal(adj[lo:hi], tri + face0), what
            assert np.array_equal(np.diff(adj_first[first_v[k]:first_v[k + 1] + 1]), np.bincount(vert, minlength=len(v))), what
            face0 += len(t)
            if abs(scale_exp) == 40:
                assert not got.view(np.uint32).any(), "%s: l2 under- or overflows: every normal is (0, 0, 0)" % what
            elif what.startswith(("base mesh 0", "base mesh 1", "a fan", "exactly", "257")):
                live = np.bincount(vert, minlength=len(v)) > 0
                assert np.allclose(np.linalg.norm(got[live].astype(np.float64), axis=1), 1.0, atol=1e-6), what
        assert face0 == face_vertex.shape[1]
    # the cases by name, at scale 1
    if scale_exp == 0:
        by = {what: restate_vertex_normals(v, t) for what, v, t in edge_meshes()}
        assert not by["a vertex no triangle names"][3].any() and by["a vertex no triangle names"][0, 2] == 1.0
        assert not by["two coincident triangles of opposite winding"].any(), "the exact cancellation"
        hub = by["a fan whose hub has valence 300"][0]
        assert abs(float(np.linalg.norm(hub.astype(np.float64))) - 1.0) < 1e-6 and hub[2] > 0.9
        twice = by["a triangle naming one vertex twice"]
        assert np.isfinite(twice).all() and twice.any(axis=1).all()


def test_hit_normal_reference_equals_the_numpy_restatement(harness, tmp_path):
    """Random hits on random triangles with unit and zero vertex normals among them, at scales where the interpolation lives and where
    it falls back to the flat normal."""
    rng = np.random.default_rng(7)
    n = 6000
    a = rng.uniform(-1, 1, (n, 3))
    e1, e2 = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    bary = rng.dirichlet([1, 1, 1], n)
    point = a + bary[:, 1:2] * e1 + bary[:, 2:3] * e2
    d = rng.normal(size=(n, 3))
    o = point - d * rng.uniform(0.5, 3, (n, 1))
    nrm = rng.normal(size=(3, n, 3))
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    nrm[:, 0::5] = 0.0                                               # every corner's normal zero: the fall-back
    nrm[1, 1::5] = -nrm[0, 1::5]                                     # cancelling corners
    nrm[2, 1::5] = 0.0
    scale = np.ones((n, 1))
    scale[2::7] = 2.0 ** -40                                         # the flat normal of a tiny triangle divides by zero: as today's
    rec = np.concatenate([o * scale, d, a * scale, e1 * scale, e2 * scale, nrm[0], nrm[1], nrm[2]], 1).astype(F)
    src, dst = str(tmp_path / "hits.bin"), str(tmp_path / "hits_out.bin")
    with open(src, "wb") as f:
        f.write(np.uint32([n]).tobytes())
        f.write(rec.tobytes())
    r = subprocess.run([harness, "hits", src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "hits OK", r.stdout + r.stderr
    got = np.fromfile(dst, np.uint32).reshape(n, 3)
    want, fell_back = restate_hit_normals(*(rec[:, 3 * k:3 * k + 3] for k in range(8)))
    same = (got == want.view(np.uint32)) | (np.isnan(got.view(F)) & np.isnan(want))
    assert same.all(), "%d words differ" % int((~same).sum())
    assert fell_back[0::5].all() and 0.15 < fell_back.mean() < 0.6 and (~np.isfinite(want)).any()


def test_host_checks_in_their_order(harness):
    r = subprocess.run([harness, "checks"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "checks OK", r.stdout + r.stderr


def test_rpt_mesh_shading_layout_matches_c(rpt, tmp_path):
    prog = tmp_path / "shading_layout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "rpt.h"
int main(void) {
  printf("size %zu\n", sizeof(rpt_mesh_shading)); printf("mesh %zu\n", offsetof(rpt_mesh_shading, mesh));
  printf("mode %zu\n", offsetof(rpt_mesh_shading, mode)); printf("abi %u\n", RPT_ABI_VERSION);
  printf("flat %d\n", RPT_MESH_SHADING_FLAT); printf("smooth %d\n", RPT_MESH_SHADING_SMOOTH);
  return 0; }''')
    exe = tmp_path / "shading_layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    A = rpt._abi
    assert C.sizeof(A.rpt_mesh_shading) == int(out["size"]) == 8
    for f in ("mesh", "mode"):
        assert getattr(A.rpt_mesh_shading, f).offset == int(out[f]), f
    assert (int(out["flat"]), int(out["smooth"])) == (A.RPT_MESH_SHADING_FLAT, A.RPT_MESH_SHADING_SMOOTH) == (0, 1)
    assert int(out["abi"]) == A.RPT_ABI_VERSION == 5                  # additive: the ABI version did not move


def test_the_shading_calls_validate_without_gpu(rpt):
    lib, A = rpt.lib(), rpt._abi
    items = (A.rpt_mesh_shading * 1)()
    items[0].mesh, items[0].mode = 0, A.RPT_MESH_SHADING_SMOOTH
    out = np.zeros(3, F)
    for name, call in (("rpt_set_mesh_shading", lambda: lib.rpt_set_mesh_shading(None, items, 1)),
                       ("rpt_download_mesh_normals", lambda: lib.rpt_download_mesh_normals(None, 0, out.ctypes.data, 1))):
        assert call() == A.RPT_ERR_INVALID_ARG, name
        assert name.encode() in lib.rpt_last_error(None), name
    assert lib.rpt_set_mesh_shading(None, None, 0) == A.RPT_ERR_INVALID_ARG       # the NULL context comes before n_items == 0
    assert lib.rpt_set_mesh_shading(None, None, 1) == A.RPT_ERR_INVALID_ARG
    assert lib.rpt_debug_mesh_normal_query(None, None, 0, None, 0, None) == A.RPT_ERR_INVALID_ARG


SMOOTH_KERNELS = ["meshsmooth_face_kernel", "meshsmooth_query_kernel", "meshsmooth_regen_kernel", "meshsmooth_vertex_kernel"]


def test_the_smooth_kernels_have_a_code_object_of_their_own():
    """librpt_hip_smooth.so (build.py, SMOOTH_LIB) holds exactly the meshsmooth_* kernels and exports exactly its three launch
    functions; both libraries load it through their run path, and no other library holds a meshsmooth_ kernel."""
    assert sorted(code_object_kernels(os.path.join(PKG, "librpt_hip_smooth.so"))) == SMOOTH_KERNELS
    for lib in ("librpt_hip.so", "librpt_hip_test.so", "librpt_hip_mesh.so", "librpt_hip_refit.so", "librpt_hip_build.so", "librpt_hip_move.so"):
        assert not [n for n in code_object_kernels(os.path.join(PKG, lib)) if n.startswith("meshsmooth_")], lib
    for lib in ("librpt_hip.so", "librpt_hip_test.so"):
        dyn = subprocess.run(["readelf", "-d", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        assert "librpt_hip_smooth.so" in dyn and "$ORIGIN" in dyn, lib
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(PKG, "librpt_hip_smooth.so")], check=True, capture_output=True, text=True).stdout
    fns = sorted(line.split(" T ", 1)[1].split("(")[0] for line in out.splitlines() if " T " in line)
    assert fns == ["rptlaunch::mesh_normal_query", "rptlaunch::render_mesh_smooth", "rptlaunch::smooth_normals"], out
    # the product exports the two new entry points, and the hook only in the test build
    for lib, hook in (("librpt_hip.so", False), ("librpt_hip_test.so", True)):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        for name in ("rpt_set_mesh_shading", "rpt_download_mesh_normals"):
            assert re.search(r" T %s$" % name, out, re.M), name
        assert bool(re.search(r" T rpt_debug_mesh_normal_query$", out, re.M)) == hook, lib


def test_build_py_names_the_smooth_library(rpt):
    """build.py: smooth_lib_of beside the other four, and needs_build's earlier positional parameters still mean what they meant."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_rpt_build_for_test", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.SMOOTH_LIB == b.smooth_lib_of(b.LIB) == os.path.join(PKG, "librpt_hip_smooth.so")
    assert b.smooth_lib_of("/x/y/libz.so") == "/x/y/libz_smooth.so"
    assert any(o[0] == "k_smooth" and o[1] == "k_smooth.hip" and o[2] == b.PEROP and o[3] == "smooth" for o in b.OBJECTS)
    assert "-ffp-contract=off" in b.BASE_FLAGS                      # no contraction: a fused multiply-add in cross changes bits
    missing = os.path.join(PKG, "no_such_library.so")
    assert b.needs_build(b.LIB, b.MESH_LIB, b.REFIT_LIB, b.BUILD_LIB, missing) is True       # (the fifth positional parameter is still move_lib)
    assert b.needs_build(b.LIB, b.MESH_LIB, b.REFIT_LIB, b.BUILD_LIB, b.MOVE_LIB, missing) is True
    assert b.needs_build(b.LIB, smooth_lib=missing) is True


def test_the_table_kernels_use_no_scratch(tmp_path):
    """The kernels' metadata, read the way tools/kernel_meta.py reads it: the face and vertex passes have no private segment, no
    spilled register and no LDS; the render kernel has mesh_regen_kernel's launch bounds and no private segment either."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
    fat, co = str(tmp_path / "fatbin"), str(tmp_path / "co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", os.path.join(PKG, "librpt_hip_smooth.so"), fat], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
    txt = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    blocks = txt.split("  - .agpr_count:")[1:]
    assert len(blocks) == 4
    seen = []
    for blk in blocks:
        g = lambda k: int(re.search(r"\.%s:\s*(\d+)" % k, blk).group(1))      # noqa: E731
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        seen.append(name)
        assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0, name
        if "face" in name or "vertex" in name:
            assert g("sgpr_spill_count") == 0 and g("group_segment_fixed_size") == 0 and g("vgpr_count") <= 32, name
        if "regen" in name:
            assert g("max_flat_workgroup_size") == 256 and g("vgpr_count") <= 128, name      # 256 lanes, 4 waves per SIMD
    assert sorted(n for s in seen for n in SMOOTH_KERNELS if n in s) == SMOOTH_KERNELS
