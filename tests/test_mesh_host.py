"""Triangle meshes on the host (include/rpt.h, "triangle meshes"; CPU only): rpt_mesh and the new rpt_scene_desc fields have C's
layout, Scene.describe() fills them, the bounding volume hierarchy (csrc/host_bvh.h) keeps its invariants under g++'s address and
undefined-behaviour sanitizers, and the library's code object holds the mesh class's kernels."""
import ctypes as C
import os
import subprocess

import numpy as np

from kernel_census import code_object_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rpt_mesh_layout_matches_c(rpt, tmp_path):
    prog = tmp_path / "mesh_layout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "rpt.h"
int main(void) {
  printf("rpt_mesh %zu\n", sizeof(rpt_mesh)); printf("rpt_scene_desc %zu\n", sizeof(rpt_scene_desc));
  printf("rpt_mesh.vertices %zu\n", offsetof(rpt_mesh, vertices)); printf("rpt_mesh.n_triangles %zu\n", offsetof(rpt_mesh, n_triangles));
  printf("rpt_mesh.indices %zu\n", offsetof(rpt_mesh, indices)); printf("rpt_mesh.material %zu\n", offsetof(rpt_mesh, material));
  printf("rpt_scene_desc.n_meshes %zu\n", offsetof(rpt_scene_desc, n_meshes)); printf("rpt_scene_desc.meshes %zu\n", offsetof(rpt_scene_desc, meshes));
  printf("abi %u\n", RPT_ABI_VERSION); printf("max %u\n", RPT_MESH_MAX_TRIANGLES);
  return 0; }''')
    exe = tmp_path / "mesh_layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    A = rpt._abi
    assert C.sizeof(A.rpt_mesh) == int(out["rpt_mesh"]) and C.sizeof(A.rpt_scene_desc) == int(out["rpt_scene_desc"])
    for key in ("rpt_mesh.vertices", "rpt_mesh.n_triangles", "rpt_mesh.indices", "rpt_mesh.material", "rpt_scene_desc.n_meshes",
                "rpt_scene_desc.meshes"):
        t, f = key.split(".")
        assert getattr(getattr(A, t), f).offset == int(out[key]), key
    assert int(out["abi"]) == A.RPT_ABI_VERSION == 5 and int(out["max"]) == A.RPT_MESH_MAX_TRIANGLES
    assert rpt.lib().rpt_sizeof_scene_desc() == C.sizeof(A.rpt_scene_desc)


def test_analytical_scene_has_no_meshes(rpt):
    d = rpt._abi.rpt_scene_desc()
    d.n_meshes = 7
    assert rpt.lib().rpt_scene_analytical(C.byref(d)) == 0
    assert d.n_meshes == 0 and not d.meshes


def test_describe_fills_the_meshes(rpt):
    from rust_pathtracer_amd import scenes
    s = scenes.mesh_scene(subdivisions=2, n_major=8, n_minor=4)
    d = s.describe()
    assert d.n_meshes == 2 and d.abi_version == rpt._abi.RPT_ABI_VERSION
    for i, (v, t, m) in enumerate(s.meshes):
        me = d.meshes[i]
        assert (me.n_vertices, me.n_triangles, me.material) == (len(v), len(t), m)
        assert np.array_equal(np.ctypeslib.as_array(me.vertices, (len(v) * 3,)), np.asarray(v, np.float32).ravel())
        assert np.array_equal(np.ctypeslib.as_array(me.indices, (len(t) * 3,)), np.asarray(t, np.uint32).ravel())
    assert d.meshes[0].n_triangles == 20 * 4 ** 2 and d.meshes[1].n_triangles == 2 * 8 * 4
    big = scenes.mesh_scene()
    n = sum(len(t) for _, t, _ in big.meshes)
    assert 1e5 <= n <= 1e6
    for v, t, _ in big.meshes:
        assert t.max() < len(v) and np.isfinite(v).all()


def test_bvh_invariants_under_sanitizers(tmp_path):
    """Each triangle in exactly one leaf, leaves of at most 8, no leaf deeper than the device stack (24), every box containing its
    children and its triangles' vertices, the same bytes from the same input — on random triangles, identical centroids, one
    triangle repeated, every triangle on one line, exponentially spaced slivers, and 10^6 triangles."""
    exe = str(tmp_path / "bvh_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "bvh_harness.cpp"), "-o", exe], check=True)
    args = ["random", "1", "random", "9", "random", "5000", "same_centroid", "20000", "identical", "5000", "line", "40000",
            "strip", "6000", "random", "1000000"]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(args) // 2 and all(line.endswith("OK") for line in lines), r.stdout


MESH_KERNELS = ["mesh_query_kernel", "mesh_regen_kernel"]


def test_the_code_object_holds_the_mesh_kernels():
    """The mesh class's kernels are named mesh_* and live in librpt_hip_mesh.so (build.py, MESH_LIB): the megakernel and the test hook's
    query kernel, nothing else; both libraries load it through their run path."""
    pkg = os.path.join(ROOT, "rust-pathtracer_amd")
    assert sorted(code_object_kernels(os.path.join(pkg, "librpt_hip_mesh.so"))) == MESH_KERNELS
    for lib in ("librpt_hip.so", "librpt_hip_test.so"):
        assert not [n for n in code_object_kernels(os.path.join(pkg, lib)) if n.startswith("mesh_")], lib
        dyn = subprocess.run(["readelf", "-d", os.path.join(pkg, lib)], check=True, capture_output=True, text=True).stdout
        assert "librpt_hip_mesh.so" in dyn and "$ORIGIN" in dyn, lib
