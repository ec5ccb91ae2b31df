"""rpt_update_meshes on the host (include/rpt.h, "moving meshes"; CPU only): the host reference of the refit keeps the build's bytes
and, after a move, the hierarchy's invariants, the level order is one, every error case answers its code (csrc/host_refit.h under
g++'s address and undefined-behaviour sanitizers: tests/refit_harness.cpp); rpt_mesh_vertices has C's layout; the entry point rejects
a NULL context without a GPU; and the refit kernels live in a code object library of their own and use no scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from kernel_census import code_object_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rust-pathtracer_amd")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("refit") / "refit_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "refit_harness.cpp"), "-o", exe], check=True)
    return exe


def test_refit_reference_under_sanitizers(harness):
    """tests/bvh_harness.cpp's families and 10^5 random triangles: the same vertices give the build's rows and nodes byte for byte;
    moved ones (displaced, collapsed to a point, scaled by 2^61) give every box as the union of its children's and its leaves'
    triangle_box, with the .w words, the child words and the empty children untouched; the level order is one."""
    args = ["random", "1", "random", "9", "random", "5000", "same_centroid", "20000", "identical", "5000", "line", "40000",
            "strip", "6000", "random", "100000"]
    r = subprocess.run([harness, "families"] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(args) // 2 and all(line.endswith("OK") for line in lines), r.stdout
    levels = [int(re.search(r"levels (\d+)", line).group(1)) for line in lines]
    assert levels[0] == 1 and max(levels) <= 24, r.stdout


@pytest.mark.parametrize("mode", ["subnormal", "errors", "rule"])
def test_refit_host_checks(harness, mode):
    """subnormal: edges of subnormal length are kept; errors: every RPT_ERR_INVALID_ARG / RPT_ERR_NO_SCENE case of an update, its
    message naming mesh and vertex, a valid update accepted after each; rule: a coordinate beyond 2^60 turns the walk off, and an
    update that brings it back turns it on."""
    r = subprocess.run([harness, mode], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == mode + " OK", r.stdout + r.stderr


def test_rpt_mesh_vertices_layout_matches_c(rpt, tmp_path):
    prog = tmp_path / "update_layout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "rpt.h"
int main(void) {
  printf("size %zu\n", sizeof(rpt_mesh_vertices)); printf("mesh %zu\n", offsetof(rpt_mesh_vertices, mesh));
  printf("n_vertices %zu\n", offsetof(rpt_mesh_vertices, n_vertices)); printf("vertices %zu\n", offsetof(rpt_mesh_vertices, vertices));
  printf("abi %u\n", RPT_ABI_VERSION);
  return 0; }''')
    exe = tmp_path / "update_layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    A = rpt._abi
    assert C.sizeof(A.rpt_mesh_vertices) == int(out["size"]) == 16
    for f in ("mesh", "n_vertices", "vertices"):
        assert getattr(A.rpt_mesh_vertices, f).offset == int(out[f]), f
    assert int(out["abi"]) == A.RPT_ABI_VERSION == 5                  # additive: the ABI version did not move


def test_update_meshes_validates_without_gpu(rpt):
    lib, A = rpt.lib(), rpt._abi
    v = np.zeros(3, np.float32)
    up = (A.rpt_mesh_vertices * 1)()
    up[0].mesh, up[0].n_vertices, up[0].vertices = 0, 1, v.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.rpt_update_meshes(None, up, 1) == A.RPT_ERR_INVALID_ARG
    assert b"rpt_update_meshes" in lib.rpt_last_error(None)
    assert lib.rpt_update_meshes(None, None, 0) == A.RPT_ERR_INVALID_ARG
    assert lib.rpt_debug_mesh_tables(None, 0, None, 0, None) == A.RPT_ERR_INVALID_ARG


def test_mesh_scene_moved_is_seeded_and_starts_at_the_scene(rpt):
    from rust_pathtracer_amd import scenes
    s = scenes.mesh_scene(subdivisions=2, n_major=8, n_minor=4)
    still = scenes.mesh_scene_moved(s, 0)
    for (v, _, _), w in zip(s.meshes, still):
        assert w.dtype == np.float32 and np.array_equal(np.asarray(v, np.float32).view(np.uint32), w.view(np.uint32)) and w is not v
    small, large = scenes.mesh_scene_moved(s, 0.05), scenes.mesh_scene_moved(s, 2.0)
    again = scenes.mesh_scene_moved(s, 2.0)
    for k in range(2):
        assert small[k].shape == large[k].shape == s.meshes[k][0].shape and np.isfinite(large[k]).all()
        assert np.array_equal(large[k], again[k])
        d_small = np.abs(small[k] - s.meshes[k][0]).max()
        d_large = np.abs(large[k] - s.meshes[k][0]).max()
        assert 0 < d_small < d_large, (k, d_small, d_large)
    # the torus turns about its own axis: every vertex keeps its distance from it and its height
    c = 0.5 * (s.meshes[1][0].min(0) + s.meshes[1][0].max(0)).astype(np.float64)
    r0 = np.hypot(*(s.meshes[1][0][:, :2] - c[:2]).T)
    r1 = np.hypot(*(large[1][:, :2] - c[:2]).T)
    assert np.allclose(r0, r1, atol=1e-5) and np.allclose(s.meshes[1][0][:, 2], large[1][:, 2], atol=1e-6)


def test_the_refit_kernels_have_a_code_object_of_their_own():
    """librpt_hip_refit.so (build.py, REFIT_LIB) holds exactly the two refit kernels; both libraries load it through their run path and
    hold no refit_* kernel themselves."""
    assert sorted(code_object_kernels(os.path.join(PKG, "librpt_hip_refit.so"))) == ["refit_nodes_kernel", "refit_triangles_kernel"]
    for lib in ("librpt_hip.so", "librpt_hip_test.so", "librpt_hip_mesh.so"):
        assert not [n for n in code_object_kernels(os.path.join(PKG, lib)) if n.startswith("refit_")], lib
    for lib in ("librpt_hip.so", "librpt_hip_test.so"):
        dyn = subprocess.run(["readelf", "-d", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        assert "librpt_hip_refit.so" in dyn and "$ORIGIN" in dyn, lib
    # what the library that loads it calls: the two launch functions, and nothing else
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(PKG, "librpt_hip_refit.so")], check=True, capture_output=True, text=True).stdout
    fns = sorted(line.split(" T ", 1)[1].split("(")[0] for line in out.splitlines() if " T " in line)
    assert fns == ["rptlaunch::refit_nodes", "rptlaunch::refit_triangles"], out


def test_the_refit_kernels_use_no_scratch(tmp_path):
    """The kernels' metadata, read the way tools/kernel_meta.py reads it: no private segment, no spilled register."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
    fat, co = str(tmp_path / "fatbin"), str(tmp_path / "co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", os.path.join(PKG, "librpt_hip_refit.so"), fat], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
    txt = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    blocks = txt.split("  - .agpr_count:")[1:]
    assert len(blocks) == 2
    for blk in blocks:
        g = lambda k: int(re.search(r"\.%s:\s*(\d+)" % k, blk).group(1))      # noqa: E731
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        assert "refit_" in name
        assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0, name
        assert g("group_segment_fixed_size") == 0 and g("vgpr_count") <= 64, name
