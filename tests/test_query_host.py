"""Ray queries on the host (include/rpt.h, "ray queries"; CPU only): the five entry points are declared in the product header, exported
by librpt_hip.so and absent from the test header; rpt_ray, rpt_hit and rpt_surface are 32, 32 and 64 bytes with the header's field
offsets in C and in the ctypes mirror, and the ABI version did not move; each entry point answers RPT_ERR_INVALID_ARG for a NULL
context without touching a device; the lookup from a flattened triangle to its mesh equals a linear search over offsets with empty
meshes, one-triangle meshes and the first and last triangle of each, and the composer lends the query's empty tables exactly while
the feature each stands for is absent (tests/query_harness.cpp, a stand-alone program built under g++'s address and
undefined-behaviour sanitizers); the query_* kernels live in a code object library of their own, use no scratch and at most the 80
VGPRs that leave the walks' LDS stack, not the registers, as what bounds their occupancy; and the numpy restatement the GPU test
holds the kernels to meets that test's caps on the CPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import query_np as Q
from kernel_census import code_object_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rust-pathtracer_amd")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
ENTRY_POINTS = ["rpt_camera_rays_device", "rpt_occluded", "rpt_occluded_device", "rpt_trace_rays", "rpt_trace_rays_device"]
QUERY_KERNELS = ["query_camera_rays_kernel", "query_closest_cut_kernel", "query_closest_kernel", "query_occluded_cut_kernel", "query_occluded_kernel",
                 "query_surface_cut_kernel", "query_surface_kernel", "query_surface_nrm_cut_kernel", "query_surface_nrm_kernel"]
OTHER_LIBS = ("librpt_hip.so", "librpt_hip_test.so", "librpt_hip_mesh.so", "librpt_hip_refit.so", "librpt_hip_build.so", "librpt_hip_move.so",
              "librpt_hip_smooth.so", "librpt_hip_light.so", "librpt_hip_tex.so", "librpt_hip_env.so", "librpt_hip_cut.so", "librpt_hip_nrm.so",
              "librpt_hip_mmap.so", "librpt_hip_emap.so", "librpt_hip_med.so")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("query") / "query_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), os.path.join(ROOT, "tests", "query_harness.cpp"), "-o", exe], check=True)
    return exe


def _run(harness, *args):
    r = subprocess.run([harness] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr
    return r.stdout


# ---- the interface --------------------------------------------------------------------------------------------------------------------
def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(rpt_[a-z0-9_]+)\s*\(", src))


def test_the_entry_points_are_product_symbols(rpt):
    """This test fails without the feature: the header declares none of the five."""
    assert set(ENTRY_POINTS) <= _declared("rpt.h")
    assert not set(ENTRY_POINTS) & _declared("rpt_test.h")
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "librpt_hip.so")], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(ENTRY_POINTS) <= exported
    assert set(ENTRY_POINTS) <= set(rpt._abi.SYMBOLS) and not set(ENTRY_POINTS) & set(rpt._abi.TEST_SYMBOLS)
    assert rpt._abi.RPT_ABI_VERSION == 5 and rpt.lib().rpt_abi_version() == 5
    hpp = open(os.path.join(ROOT, "include", "rpt.hpp")).read()
    for name in ENTRY_POINTS:
        assert name + "(ctx_" in hpp, name


def test_record_layouts_match_c(rpt, tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "rpt.h"
#define S(t) printf(#t " %zu\n", sizeof(t))
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void) {
  S(rpt_ray); S(rpt_hit); S(rpt_surface);
  O(rpt_ray, origin); O(rpt_ray, max_dist); O(rpt_ray, direction); O(rpt_ray, reserved);
  O(rpt_hit, t); O(rpt_hit, kind); O(rpt_hit, primitive); O(rpt_hit, mesh); O(rpt_hit, triangle); O(rpt_hit, u); O(rpt_hit, v); O(rpt_hit, reserved);
  O(rpt_surface, ng); O(rpt_surface, ns); O(rpt_surface, rgb); O(rpt_surface, emission); O(rpt_surface, roughness); O(rpt_surface, metallic);
  O(rpt_surface, material); O(rpt_surface, reserved);
  printf("kinds %d %d %d %d\n", RPT_HIT_NONE, RPT_HIT_SPHERE, RPT_HIT_PLANE, RPT_HIT_TRIANGLE);
  return 0; }''')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)      # (C11: the header's _Static_assert is live)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert lines[-1] == "kinds 0 1 2 3"
    A = rpt._abi
    assert (A.RPT_HIT_NONE, A.RPT_HIT_SPHERE, A.RPT_HIT_PLANE, A.RPT_HIT_TRIANGLE) == (0, 1, 2, 3)
    out = dict(line.rsplit(" ", 1) for line in lines[:-1])
    assert (int(out["rpt_ray"]), int(out["rpt_hit"]), int(out["rpt_surface"])) == (32, 32, 64)
    for name in ("rpt_ray", "rpt_hit", "rpt_surface"):
        assert C.sizeof(getattr(A, name)) == int(out[name]), name
    n = 0
    for key, val in out.items():
        if "." in key:
            t, f = key.split(".")
            assert getattr(getattr(A, t), f).offset == int(val), key
            n += 1
    assert n == 20
    # the words the Python wrappers slice (api.py, Tracer._hit_views): 4 bytes each, in the header's order
    assert [getattr(A.rpt_hit, f).offset // 4 for f in ("t", "kind", "primitive", "mesh", "triangle", "u", "v")] == list(range(7))
    assert [getattr(A.rpt_surface, f).offset // 4 for f in ("ng", "ns", "rgb", "emission", "roughness", "metallic", "material")] == [0, 3, 6, 9, 12, 13, 14]
    assert [getattr(A.rpt_ray, f).offset // 4 for f in ("origin", "max_dist", "direction", "reserved")] == [0, 3, 4, 7]


def test_a_null_context_is_rejected_without_a_device(rpt):
    lib, bad = rpt.lib(), rpt._abi.RPT_ERR_INVALID_ARG
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert lib.rpt_trace_rays_device(None, p, 1, p, None, 0, None) == bad and b"ctx is NULL" in lib.rpt_last_error(None)
    assert lib.rpt_occluded_device(None, p, 1, p, 0, None) == bad and b"rpt_occluded_device" in lib.rpt_last_error(None)
    assert lib.rpt_camera_rays_device(None, 4, 4, p, None) == bad and b"rpt_camera_rays_device" in lib.rpt_last_error(None)
    assert lib.rpt_trace_rays(None, p, 1, p, p, 0) == bad and b"rpt_trace_rays" in lib.rpt_last_error(None)
    assert lib.rpt_occluded(None, p, 1, p, 0) == bad and b"rpt_occluded" in lib.rpt_last_error(None)
    assert lib.rpt_trace_rays(None, None, 0, None, None, 0) == bad, "also with nothing to do"
    assert not any(buf), "nothing was written"


# ---- the lookup and the composer ------------------------------------------------------------------------------------------------------
def test_the_mesh_lookup_equals_a_linear_search(harness):
    out = _run(harness, "lookup")
    assert re.search(r"lookup OK (\d+)", out) and int(re.search(r"lookup OK (\d+)", out).group(1)) > 300


def test_the_composer_lends_the_empty_tables_exactly_while_a_feature_is_absent(harness):
    out = _run(harness, "compose")
    assert out.rstrip().endswith("compose OK")
    lines = [l for l in out.splitlines() if l.startswith("surface")]
    assert len(lines) == 4 * 1 + 16 * 4, "without a texture one kernel, with one all four"      # 4 untextured combinations, 16 textured
    assert sum("emap lent" in l for l in lines) > 0 and sum("emap own" in l for l in lines) > 0
    assert "surface emap lent mmap lent tex lent lights lent smooth lent" in lines, "a scene with nothing ON"
    assert "surface_nrm_cut emap own mmap own tex own lights own smooth own" in lines, "a scene with everything ON"


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_the_query_kernels_have_a_code_object_of_their_own():
    """librpt_hip_query.so (build.py, QUERY_LIB) holds exactly the nine kernels and exports exactly its nine launch functions; both
    libraries load it through their run path, and no other library holds a query_ kernel."""
    assert sorted(code_object_kernels(os.path.join(PKG, "librpt_hip_query.so"))) == QUERY_KERNELS
    for lib in OTHER_LIBS:
        assert not [n for n in code_object_kernels(os.path.join(PKG, lib)) if n.startswith("query_")], lib
    for lib in ("librpt_hip.so", "librpt_hip_test.so"):
        dyn = subprocess.run(["readelf", "-d", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        assert "librpt_hip_query.so" in dyn and "$ORIGIN" in dyn, lib
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(PKG, "librpt_hip_query.so")], check=True, capture_output=True, text=True).stdout
    fns = sorted(line.split(" T ", 1)[1].split("(")[0] for line in out.splitlines() if " T " in line)
    assert fns == ["rptlaunch::query_camera_rays", "rptlaunch::query_closest", "rptlaunch::query_closest_cut", "rptlaunch::query_occluded",
                   "rptlaunch::query_occluded_cut", "rptlaunch::query_surface", "rptlaunch::query_surface_cut", "rptlaunch::query_surface_nrm",
                   "rptlaunch::query_surface_nrm_cut"], out


def test_build_py_names_the_query_library(rpt):
    import importlib.util
    spec = importlib.util.spec_from_file_location("_rpt_build_for_query_test", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.QUERY_LIB == b.query_lib_of(b.LIB) == os.path.join(PKG, "librpt_hip_query.so")
    assert b.query_lib_of("/x/y/libz.so") == "/x/y/libz_query.so"
    parts = [o for o in b.OBJECTS if o[3] == "query"]
    assert [(o[0], o[1]) for o in parts] == [("k_query", "k_query.hip")] and parts[0][2] == b.PEROP, "strict arithmetic, as k_med.hip"
    assert "-ffp-contract=off" in b.BASE_FLAGS
    assert b.needs_build(b.LIB, query_lib=os.path.join(PKG, "no_such_library.so")) is True


def test_the_query_kernels_use_no_scratch_and_at_most_80_vgprs(tmp_path):
    """The kernels' metadata, read the way tools/kernel_meta.py reads it: no private segment, no spilled register, 256 lanes; the eight
    that walk the hierarchy hold its 24 KiB LDS stack — six workgroups per CU — and at most 80 VGPRs, which six workgroups of four
    waves leave each lane (512 / 6): the stack, not the registers, bounds their occupancy.  The camera's kernel has no stack."""
    llvm = os.path.join(ROCM, "lib", "llvm", "bin")
    fat, co = str(tmp_path / "fatbin"), str(tmp_path / "co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", os.path.join(PKG, "librpt_hip_query.so"), fat], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
    txt = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    blocks = txt.split("  - .agpr_count:")[1:]
    assert len(blocks) == len(QUERY_KERNELS)
    walkers = 0
    for blk in blocks:
        g = lambda k: int(re.search(r"\.%s:\s*(\d+)" % k, blk).group(1))      # noqa: E731
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0, name
        assert g("max_flat_workgroup_size") == 256, name
        if "camera" in name:
            assert g("group_segment_fixed_size") == 0, name
        else:
            walkers += 1
            assert g("group_segment_fixed_size") == 24 * 1024 and g("vgpr_count") <= 80, name
    assert walkers == 8


# ---- the restatement's own sample ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_exp", [0, 20])
def test_the_restatement_meets_the_gpu_tests_caps(rpt, scale_exp):
    """The caps of tests/test_gpu_query.py's first test, on a fifth of its rays (the same generator and seed): the spheres and the
    plane are chosen so that the restatement alone answers triangles, spheres, planes and misses in quantity."""
    s, r7, unit = Q.big_case(scale_exp, 8000)
    hits, occluded = Q.restate(s, r7)
    kind = hits[:, 1]
    finite = np.isfinite(hits[:, 0].view(np.float32))
    assert unit.mean() > 0.6 and (~unit).sum() > 2000, "three rays in four have a unit direction"
    k = kind[unit]
    assert (k == Q.HIT_TRIANGLE).mean() > 0.2 and ((k == Q.HIT_SPHERE) & finite[unit]).mean() > 0.02 and (k == Q.HIT_PLANE).mean() > 0.02
    assert occluded[unit].mean() > 0.05 and (k == Q.HIT_NONE).mean() > 0.05
    assert (kind[~unit] == Q.HIT_TRIANGLE).mean() > 0.05 and (kind[~unit] == Q.HIT_SPHERE).mean() > 0.05, "the rays that keep their lengths hit things too"
    spheres = hits[kind == Q.HIT_SPHERE, 2]
    assert (spheres == 0).any() and (spheres == 1).any(), "both spheres win somewhere"
    tri = kind == Q.HIT_TRIANGLE
    first = np.cumsum([0] + [len(t) for _, t, _ in s.meshes])
    assert np.array_equal(first[hits[tri, 3]] + hits[tri, 4], hits[tri, 2]), "mesh and triangle name the flattened index"
    assert len(np.unique(hits[tri, 3])) == len(s.meshes), "every mesh wins somewhere"
    assert (hits[~tri, 3:5] == Q.NONE).all() and not hits[~tri, 5:7].any() and not hits[:, 7].any()
    assert (hits[kind == Q.HIT_NONE, 0] == Q.INF_BITS).all() and (hits[kind == Q.HIT_NONE, 2] == Q.NONE).all()
