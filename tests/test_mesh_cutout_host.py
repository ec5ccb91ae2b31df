"""Mesh cutouts on the host (include/rpt.h, "mesh cutouts"; CPU only): csrc/host_cut.h's checks answer in their order, its plain-loop
mask equals numpy's packed bits, and its cut lookup equals a numpy float32 restatement bit for bit and a plain float64 evaluation
away from texel borders (under g++'s address and undefined-behaviour sanitizers: tests/cut_harness.cpp); rpt_mesh_cutout has C's
layout and the ABI version did not move; the entry points reject what they can without a GPU; and the meshcut_* kernels live in a
code object library of their own, none of which uses scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from kernel_census import code_object_kernels
from test_mesh_texture_host import CLAMP, REPEAT, _nearest, _wrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rust-pathtracer_amd")
F = np.float32
MASK_SIZES = ((1, 1), (5, 3), (33, 7), (64, 64))                     # (width, height); 33 x 7 ends in a ragged word
THRESHOLDS = (1, 128, 255)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cut") / "cut_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cut_harness.cpp"), "-o", exe], check=True)
    return exe


# ---- the restatements (tests/test_gpu_mesh_cutout.py imports them) -----------------------------------------------------------------
def random_alpha(w, h, seed):
    """[h, w] uint8 with every special value present where there is room: 0, threshold neighbours, 255."""
    a = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    special = np.array([0, 1, 127, 128, 129, 254, 255], np.uint8)
    a.reshape(-1)[:min(a.size, len(special))] = special[:min(a.size, len(special))]
    return a


def restate_mask_bits(alpha, threshold):
    """[h, w] uint8 -> bool [h * w]: bit k = alpha[k] >= threshold, an integer compare."""
    return np.asarray(alpha, np.uint8).reshape(-1).astype(np.int64) >= int(threshold)


def restate_mask_words(alpha, threshold, pad=32):
    """The mask as words: texel k in bit k % 32 of word k / 32 (numpy packbits, little bit order), zero-padded to `pad` texels."""
    bits = restate_mask_bits(alpha, threshold)
    bits = np.concatenate([bits, np.zeros((-len(bits)) % pad, bool)])
    return np.packbits(bits, bitorder="little").view(np.uint32).copy()


def restate_cut_texel(u, v, uva, uvb, uvc, width, height, wrap):
    """The texel of include/rpt.h, "cut test", on float32 arrays, one rounding per operation: u, v [n]; uva, uvb, uvc [2] or [n, 2]."""
    u, v = np.ascontiguousarray(u, F), np.ascontiguousarray(v, F)
    uva, uvb, uvc = (np.ascontiguousarray(x, F) for x in (uva, uvb, uvc))
    w = (F(1.0) - u) - v
    st = (w[:, None] * uva + u[:, None] * uvb) + v[:, None] * uvc
    assert st.dtype == F
    x, y = _wrap(st[:, 0], wrap), _wrap(st[:, 1], wrap)
    assert x.dtype == F and y.dtype == F
    return _nearest(y, height, wrap) * width + _nearest(x, width, wrap)


def cut_texel_f64(u, v, uva, uvb, uvc, width, height, wrap):
    """The same texel written plainly in float64, and the distance of x*W, y*H to the next integer, in texels (inf where a clamped
    coordinate makes both sides the edge texel)."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    uva, uvb, uvc = (np.asarray(x, np.float64) for x in (uva, uvb, uvc))
    st = (1.0 - u - v)[:, None] * uva + u[:, None] * uvb + v[:, None] * uvc

    def axis(c, n):
        x = np.clip(c, 0.0, 1.0) if wrap == CLAMP else c - np.floor(c)
        p = x * n
        i = np.floor(p).astype(np.int64)
        i = np.minimum(i, n - 1) if wrap == CLAMP else i % n
        away = np.where((wrap == CLAMP) & ((c <= 0) | (c >= 1)), np.inf, np.abs(p - np.round(p)))
        return i, away

    i, ai = axis(st[:, 0], width)
    j, aj = axis(st[:, 1], height)
    return j * width + i, np.minimum(ai, aj)


def _run(harness, mode, tmp_path, head, *blobs):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.uint32(head).tobytes())
        for b in blobs:
            f.write(np.ascontiguousarray(b).tobytes())
    r = subprocess.run([harness, mode, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == mode + " OK", r.stdout + r.stderr
    return np.fromfile(dst, np.uint32)


# ---- the tests ---------------------------------------------------------------------------------------------------------------------
def test_host_checks_in_their_order(harness):
    r = subprocess.run([harness, "checks"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "checks OK", r.stdout + r.stderr


@pytest.mark.parametrize("size", MASK_SIZES, ids=lambda wh: "%dx%d" % wh)
def test_host_mask_equals_packed_bits(harness, tmp_path, size):
    w, h = size
    for threshold in THRESHOLDS:
        alpha = random_alpha(w, h, 100 * w + h)
        got = _run(harness, "mask", tmp_path, [w, h, threshold], alpha)
        want = restate_mask_words(alpha, threshold, pad=128)
        assert len(got) == len(want) == 4 * ((w * h + 127) // 128) and np.array_equal(got, want), (size, threshold)
        n_words = (w * h + 31) // 32
        assert np.array_equal(got[:n_words], restate_mask_words(alpha, threshold)) and not got[n_words:].any()
    assert np.array_equal(restate_mask_words(np.array([[0, 1, 127, 128, 255]], np.uint8), 128), [0b11000])
    assert np.array_equal(restate_mask_words(np.array([[0, 1, 127, 128, 255]], np.uint8), 1), [0b11110])
    assert np.array_equal(restate_mask_words(np.array([[0, 1, 127, 128, 255]], np.uint8), 255), [0b10000])


@pytest.mark.parametrize("wrap", [REPEAT, CLAMP])
def test_host_cut_lookup_equals_the_numpy_restatement_and_float64(harness, tmp_path, wrap):
    """Bit for bit against the float32 restatement, UVs in [-1, 2].  Against float64 where x*W and y*H lie at least 1e-3 of a texel
    from an integer (the float32 values are within a few 2^-20 of those: s and t are below 2 in magnitude, W at most 64); every
    other point is counted."""
    compared = 0
    for k, (w, h) in enumerate(MASK_SIZES):
        rng = np.random.default_rng(300 + 10 * k + wrap)
        uv = rng.uniform(-1.0, 2.0, (3, 2)).astype(F)
        if k == 1:
            uv = np.array([[-1.0, -1.0], [2.0, -1.0], [-1.0, 2.0]], F)    # texel borders at representable places
        bary = rng.dirichlet([1, 1, 1], 3000).astype(F)
        u, v = bary[:, 1].copy(), bary[:, 2].copy()
        grid = np.arange(0, 33, dtype=F) / F(32)                    # and the corners, the edges and a lattice that meets borders
        gu, gv = np.meshgrid(grid, grid, indexing="ij")
        keep = gu + gv <= 1
        u, v = np.concatenate([u, gu[keep]]), np.concatenate([v, gv[keep]])
        got = _run(harness, "lookup", tmp_path, [w, h, wrap, len(u)], uv.reshape(-1), np.stack([u, v], 1).astype(F))
        want = restate_cut_texel(u, v, uv[0], uv[1], uv[2], w, h, wrap)
        assert np.array_equal(got.astype(np.int64), want), "%dx%d: %d lookups differ" % (w, h, int((got != want).sum()))
        plain, margin = cut_texel_f64(u, v, uv[0], uv[1], uv[2], w, h, wrap)
        sel = margin >= 1e-3
        compared += int(sel.sum())
        assert np.array_equal(got[sel].astype(np.int64), plain[sel]), (w, h)
        assert len(np.unique(got)) >= min(w * h, 8), "the points spread over the mask (a triangle covers half of its UV square)"
    assert compared >= 9000, "most points lie away from a texel border"


def test_rpt_mesh_cutout_layout_matches_c(rpt, tmp_path):
    prog = tmp_path / "cut_layout.c"
    fields = ("mesh", "mode", "width", "height", "alpha", "threshold")
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "rpt.h"
int main(void) {
  printf("size %zu\n", sizeof(rpt_mesh_cutout)); printf("abi %u\n", RPT_ABI_VERSION); printf("desc %zu\n", sizeof(rpt_scene_desc));
  printf("tex %zu\n", sizeof(rpt_mesh_texture)); printf("consts %d\n", RPT_MESH_CUTOUT_OFF * 10 + RPT_MESH_CUTOUT_ON);
''' + "".join('  printf("%s %%zu\\n", offsetof(rpt_mesh_cutout, %s));\n' % (f, f) for f in fields) + "  return 0; }")
    exe = tmp_path / "cut_layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    A = rpt._abi
    assert C.sizeof(A.rpt_mesh_cutout) == int(out["size"]) == 32
    for f in fields:
        assert getattr(A.rpt_mesh_cutout, f).offset == int(out[f]), f
    assert int(out["consts"]) == 1 and (A.RPT_MESH_CUTOUT_OFF, A.RPT_MESH_CUTOUT_ON) == (0, 1)
    assert int(out["abi"]) == A.RPT_ABI_VERSION == 5                  # additive: the ABI version did not move
    assert int(out["desc"]) == C.sizeof(A.rpt_scene_desc) == rpt.lib().rpt_sizeof_scene_desc()
    assert int(out["tex"]) == C.sizeof(A.rpt_mesh_texture) == 48      # rpt_mesh_texture is what it was


def test_the_cutout_calls_are_declared_exported_and_mirrored(rpt):
    A = rpt._abi
    header = open(os.path.join(ROOT, "include", "rpt.h")).read()
    hooks = open(os.path.join(ROOT, "include", "rpt_test.h")).read()
    for name in ("rpt_set_mesh_cutouts", "rpt_download_mesh_cutout"):
        assert re.search(r"^int %s\(rpt_ctx\*" % name, header, re.M) and name in A.SYMBOLS and name not in A.TEST_SYMBOLS, name
    assert re.search(r"^int rpt_debug_mesh_cutout_query\(rpt_ctx\*", hooks, re.M) and "rpt_debug_mesh_cutout_query" not in header
    assert "rpt_debug_mesh_cutout_query" in A.TEST_SYMBOLS and "rpt_debug_mesh_cutout_query" not in A.SYMBOLS
    assert "mesh cutouts — PROJECT-DEFINED" in header and "csrc/host_cut.h" in header
    for lib, hook in (("librpt_hip.so", False), ("librpt_hip_test.so", True)):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        for name in ("rpt_set_mesh_cutouts", "rpt_download_mesh_cutout"):
            assert re.search(r" T %s$" % name, out, re.M), (lib, name)
        assert bool(re.search(r" T rpt_debug_mesh_cutout_query$", out, re.M)) == hook, lib
        assert len(re.findall(r"cutout", out)) == (3 if hook else 2), lib


def test_the_cutout_calls_validate_without_gpu(rpt):
    """The NULL context answers before anything else, and says which call it was."""
    lib, A = rpt.lib(), rpt._abi
    items = (A.rpt_mesh_cutout * 1)()
    out = np.zeros(4, np.uint32)
    for name, call in (("rpt_set_mesh_cutouts", lambda: lib.rpt_set_mesh_cutouts(None, items, 1)),
                       ("rpt_download_mesh_cutout", lambda: lib.rpt_download_mesh_cutout(None, 0, out.ctypes.data, 1))):
        assert call() == A.RPT_ERR_INVALID_ARG, name
        assert lib.rpt_last_error(None).startswith(name.encode() + b": "), name
    assert lib.rpt_set_mesh_cutouts(None, None, 0) == A.RPT_ERR_INVALID_ARG           # the NULL context comes before n_items == 0
    assert lib.rpt_debug_mesh_cutout_query(None, None, 0, None, 0, None) == A.RPT_ERR_INVALID_ARG


def test_the_python_wrapper_checks_its_arguments(rpt):
    with pytest.raises(ValueError):
        rpt.Tracer.set_mesh_cutouts(object(), {0: np.zeros((2, 2, 4), np.uint8)})        # the whole RGBA image, not its alpha
    with pytest.raises(ValueError):
        rpt.Tracer.set_mesh_cutouts(object(), {0: np.zeros((2, 2), np.float32)})
    with pytest.raises(ValueError):
        rpt.Tracer.set_mesh_cutouts(object(), {0: dict(alpha=np.zeros(4, np.uint8), threshold=3)})


def test_the_scene_helpers_are_what_the_tests_need(rpt):
    from rust_pathtracer_amd import scenes
    m = scenes.checker_mask(6, 4, cells=2)
    assert m.shape == (4, 6) and m.dtype == np.uint8 and m[0, 0] == 255 and m[0, 3] == 0 and m[2, 3] == 255 and set(np.unique(m)) == {0, 255}
    assert np.array_equal(m == 255, (scenes.checker_texture(6, 4, (255,) * 3, (0,) * 3, cells=2)[..., 0] == 255))
    s, uvs, mask = scenes.mesh_cutout_scene()
    base, base_uvs = scenes.mesh_texture_scene()
    assert [len(np.asarray(t).reshape(-1, 3)) for _, t, _ in s.meshes] == [80, 2, 2] and len(uvs) == 3 and len(base.meshes) == 2
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(s.meshes, base.meshes)) and all(np.array_equal(a, b) for a, b in zip(uvs, base_uvs))
    assert uvs[2].shape == (4, 2) and uvs[2].min() == 0 and uvs[2].max() == 1 and mask.ndim == 2 and mask.dtype == np.uint8
    assert 0.4 < (mask == 255).mean() < 0.6 and s.describe().n_meshes == 3
    screen = np.asarray(s.meshes[2][0])
    assert screen[:, 2].min() > max(np.asarray(v)[:, 2].max() for v, _, _ in base.meshes), "the screen stands in front of the rest"


CUT_KERNELS = ["meshcut_env_regen_kernel", "meshcut_mask_kernel", "meshcut_query_kernel", "meshcut_regen_kernel"]
OTHER_LIBS = ("librpt_hip.so", "librpt_hip_test.so", "librpt_hip_mesh.so", "librpt_hip_refit.so", "librpt_hip_build.so", "librpt_hip_move.so",
              "librpt_hip_smooth.so", "librpt_hip_light.so", "librpt_hip_tex.so", "librpt_hip_env.so")


def test_the_cutout_kernels_have_a_code_object_of_their_own():
    """librpt_hip_cut.so (build.py, CUT_LIB) holds exactly the meshcut_* kernels and exports exactly its four launch functions; both
    libraries load it through their run path, and no other library holds a meshcut_ kernel."""
    assert sorted(code_object_kernels(os.path.join(PKG, "librpt_hip_cut.so"))) == CUT_KERNELS
    for lib in OTHER_LIBS:
        assert not [n for n in code_object_kernels(os.path.join(PKG, lib)) if n.startswith("meshcut_")], lib
    for lib in ("librpt_hip.so", "librpt_hip_test.so"):
        dyn = subprocess.run(["readelf", "-d", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        assert "librpt_hip_cut.so" in dyn and "$ORIGIN" in dyn, lib
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(PKG, "librpt_hip_cut.so")], check=True, capture_output=True, text=True).stdout
    fns = sorted(line.split(" T ", 1)[1].split("(")[0] for line in out.splitlines() if " T " in line)
    assert fns == ["rptlaunch::cut_mask", "rptlaunch::mesh_cutout_query", "rptlaunch::render_mesh_cut", "rptlaunch::render_mesh_cut_env"], out


def test_build_py_names_the_cutout_library(rpt):
    """build.py: cut_lib_of beside the other nine, and needs_build's earlier positional parameters still mean what they meant."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_rpt_build_for_cut_test", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.CUT_LIB == b.cut_lib_of(b.LIB) == os.path.join(PKG, "librpt_hip_cut.so")
    assert b.cut_lib_of("/x/y/libz.so") == "/x/y/libz_cut.so"
    assert any(o[0] == "k_cut" and o[1] == "k_cut.hip" and o[2] == b.PEROP and o[3] == "cut" for o in b.OBJECTS)
    missing = os.path.join(PKG, "no_such_library.so")
    assert b.needs_build(b.LIB, b.MESH_LIB, b.REFIT_LIB, b.BUILD_LIB, b.MOVE_LIB, b.SMOOTH_LIB, b.LIGHT_LIB, b.TEX_LIB, missing) is True      # (the ninth is still env_lib)
    assert b.needs_build(b.LIB, b.MESH_LIB, b.REFIT_LIB, b.BUILD_LIB, b.MOVE_LIB, b.SMOOTH_LIB, b.LIGHT_LIB, b.TEX_LIB, b.ENV_LIB, missing) is True
    assert b.needs_build(b.LIB, cut_lib=missing) is True


def test_the_cutout_kernels_use_no_scratch(tmp_path):
    """The kernels' metadata, read the way tools/kernel_meta.py reads it: no kernel of the library has a private segment or a spilled
    vector register; the mask kernel needs no LDS and spills nothing; the render kernels have mesh_regen_kernel's launch bounds."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
    fat, co = str(tmp_path / "fatbin"), str(tmp_path / "co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", os.path.join(PKG, "librpt_hip_cut.so"), fat], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
    txt = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    blocks = txt.split("  - .agpr_count:")[1:]
    assert len(blocks) == len(CUT_KERNELS)
    seen = []
    for blk in blocks:
        g = lambda k: int(re.search(r"\.%s:\s*(\d+)" % k, blk).group(1))      # noqa: E731
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        seen.append(name)
        assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0, name
        if "regen" in name:
            assert g("max_flat_workgroup_size") == 256 and g("vgpr_count") <= 128, name      # 256 lanes, 4 waves per SIMD
        elif "mask" in name:
            assert g("sgpr_spill_count") == 0 and g("group_segment_fixed_size") == 0, name
    assert sorted(n for s in seen for n in CUT_KERNELS if n in s) == CUT_KERNELS
