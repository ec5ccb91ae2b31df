"""rpt_rebuild_meshes on the host (include/rpt.h, "rebuilding a moved mesh's hierarchy"; CPU only): the symbol is declared, exported
and mirrored; the build's kernels live in a code object library of their own, named bvhbuild_*, beside rocPRIM's, and use no
scratch; the split rule and the topology step the device runs (csrc/host_build.h, the text k_build.hip compiles) keep the
hierarchy's invariants — no leaf deeper than the walk's 24-entry stack above all — over key arrays made to press on them, under
g++'s address and undefined-behaviour sanitizers (tests/build_harness.cpp); the entry point answers without a GPU as
rpt_update_meshes does."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from kernel_census import code_object_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rust-pathtracer_amd")
BUILD_LIB = os.path.join(PKG, "librpt_hip_build.so")


# ---- exports and mirror -----------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_mirrored(rpt):
    header = open(os.path.join(ROOT, "include", "rpt.h")).read()
    assert re.search(r"^int rpt_rebuild_meshes\(rpt_ctx\* ctx, const rpt_mesh_vertices\* updates, uint32_t n_updates\);", header, re.M)
    assert re.search(r"#define RPT_ABI_VERSION 5u", header), "additive: the ABI version did not move"
    for lib in ("librpt_hip.so", "librpt_hip_test.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        assert re.search(r" T rpt_rebuild_meshes$", out, re.M), lib
    A = rpt._abi
    assert A.SYMBOLS["rpt_rebuild_meshes"] == A.SYMBOLS["rpt_update_meshes"]
    assert rpt.lib().rpt_rebuild_meshes.argtypes == [C.c_void_p, C.POINTER(A.rpt_mesh_vertices), C.c_uint32]
    assert callable(rpt.Tracer.rebuild_meshes)
    for path, needle in (("include/rpt.hpp", "rpt_rebuild_meshes(ctx_"), ("rust/gpu_tracer.rs", "pub fn rebuild_meshes(&mut self"),
                         ("rust/gpu_tracer.rs", "fn rpt_rebuild_meshes(ctx: *mut RptCtx, updates: *const RptMeshVertices, n_updates: u32) -> c_int;"),
                         ("INTEGRATION.md", "rpt_rebuild_meshes")):
        assert needle in open(os.path.join(ROOT, path)).read(), (path, needle)


def test_a_call_without_a_device_answers_as_an_update_does(rpt):
    lib, A = rpt.lib(), rpt._abi
    v = np.zeros(3, np.float32)
    up = (A.rpt_mesh_vertices * 1)()
    up[0].mesh, up[0].n_vertices, up[0].vertices = 0, 1, v.ctypes.data_as(C.POINTER(C.c_float))
    for args in ((None, up, 1), (None, None, 0)):
        assert lib.rpt_rebuild_meshes(*args) == lib.rpt_update_meshes(*args) == A.RPT_ERR_INVALID_ARG
        assert lib.rpt_rebuild_meshes(*args) == A.RPT_ERR_INVALID_ARG
        assert b"rpt_rebuild_meshes" in lib.rpt_last_error(None)


# ---- census -----------------------------------------------------------------------------------------------------------------------
def _kernel_notes(lib, tmp_path):
    """[(mangled name, metadata block)] of the gfx950 code object of a one-translation-unit library, read the way
    tools/kernel_meta.py reads it."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
    fat, co = str(tmp_path / "fatbin"), str(tmp_path / "co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
    txt = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    blocks = txt.split("  - .agpr_count:")[1:]
    return [(re.search(r"\.name:\s*(\S+)", blk).group(1), blk) for blk in blocks]


OWN = ["bvhbuild_bounds_kernel", "bvhbuild_emit_kernel", "bvhbuild_gather_kernel", "bvhbuild_init_kernel", "bvhbuild_iota_kernel",
       "bvhbuild_keys_kernel", "bvhbuild_scatter_kernel", "bvhbuild_split_kernel"]


def test_the_build_kernels_have_a_code_object_of_their_own(tmp_path):
    """librpt_hip_build.so (build.py, BUILD_LIB) holds the bvhbuild_* kernels and rocPRIM's, nothing else; no other library holds a
    bvhbuild_* kernel; both libraries load it through their run path; it exports its three launch functions and nothing else."""
    notes = _kernel_notes(BUILD_LIB, tmp_path)
    names = [n for n, _ in notes]
    own = [n for n in names if "bvhbuild_" in n]
    assert sorted(re.match(r"_Z\d+(bvhbuild_\w+_kernel)P", n).group(1) for n in own) == OWN, own
    others = [n for n in names if "bvhbuild_" not in n]
    assert others and all(n.startswith("_ZN7rocprim") for n in others), [n for n in others if not n.startswith("_ZN7rocprim")]
    assert sorted(n for n in code_object_kernels(BUILD_LIB) if n.startswith("bvhbuild_")) == OWN
    for lib in ("librpt_hip.so", "librpt_hip_test.so", "librpt_hip_mesh.so", "librpt_hip_refit.so"):
        assert not [n for n in code_object_kernels(os.path.join(PKG, lib)) if "bvhbuild" in n or "rocprim" in n], lib
    for lib in ("librpt_hip.so", "librpt_hip_test.so"):
        dyn = subprocess.run(["readelf", "-d", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        assert "librpt_hip_build.so" in dyn and "$ORIGIN" in dyn, lib
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", BUILD_LIB], check=True, capture_output=True, text=True).stdout
    fns = sorted(line.split(" T ", 1)[1].split("(")[0] for line in out.splitlines() if " T " in line)
    assert fns == ["rptlaunch::build_order", "rptlaunch::build_shape", "rptlaunch::build_temp_bytes"], out


def test_the_build_kernels_use_no_scratch(tmp_path):
    """No private segment, no spilled register, in any bvhbuild_* kernel; LDS only in the bounds' reduction."""
    seen = 0
    for name, blk in _kernel_notes(BUILD_LIB, tmp_path):
        if "bvhbuild_" not in name:
            continue
        seen += 1
        g = lambda k: int(re.search(r"\.%s:\s*(\d+)" % k, blk).group(1))      # noqa: E731
        assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0, name
        assert g("group_segment_fixed_size") == (96 if "bounds" in name else 0) and g("vgpr_count") <= 64, name
        assert not re.search(r"\.uses_dynamic_stack:\s*true", blk), name
    assert seen == len(OWN)


def test_the_refit_and_mesh_sources_are_not_the_build_s(tmp_path):
    """The build reuses the refit's launch functions as they are: k_build.hip defines no refit_* or mesh kernel, and the seam it adds
    is a header of its own, which the other kernel translation units do not include."""
    csrc = os.path.join(PKG, "csrc")
    for name in os.listdir(csrc):
        if name.endswith(".hip") and name not in ("k_build.hip", "capi.hip"):
            text = open(os.path.join(csrc, name)).read()
            assert "launch_build.h" not in text and "host_build.h" not in text, name
    text = open(os.path.join(csrc, "k_build.hip")).read()
    assert not re.search(r"__global__[^;{]*\b(?!bvhbuild_)\w+_kernel\(", text), "a kernel of k_build.hip is not named bvhbuild_*"


# ---- the split rule under the sanitizers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("build") / "build_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "build_harness.cpp"), "-o", exe], check=True)
    return exe


def test_the_topology_step_under_sanitizers(harness):
    """10^6 random keys; all-equal Morton parts; the diagonal exponential chain; a chain over every key bit (56 levels without the
    capacity rule); sparse index bits inside one cell; n = 1, 8, 9 — for leaf targets 2, 4 and 8.  The harness checks for each: every
    slot in exactly one leaf of 1-8, the root an interior node (one leaf beside an empty child up to 8 triangles), a parent below
    its children, levels contiguous and within their bounds, no leaf deeper than 24, two runs alike."""
    cases = [("random", 1000000), ("clustered", 300000), ("equal_morton", 100000), ("diagonal_chain", 20000), ("bit_chain", 5000),
             ("sparse_index", 5000), ("random", 1), ("random", 8), ("random", 9), ("equal_morton", 17), ("bit_chain", 57)]
    args = []
    for leaf in (2, 4, 8):
        for what, n in cases:
            if n == 1000000 and leaf != 4:
                continue
            args += [what, str(n), str(leaf)]
    r = subprocess.run([harness, "topology"] + args, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(args) // 3 and all(line.endswith("OK") for line in lines), r.stdout
    got = {}
    for line in lines:
        m = re.match(r"(\w+) (\d+) leaf (\d+): nodes (\d+) levels (\d+) deepest (\d+) leaves (\d+) OK", line)
        got[(m.group(1), int(m.group(2)), int(m.group(3)))] = tuple(int(x) for x in m.groups()[3:])
    assert all(levels <= 24 and deepest == levels for _, levels, deepest, _ in got.values()), r.stdout
    assert got[("bit_chain", 5000, 4)][1] == 24 and got[("bit_chain", 5000, 8)][1] == 24, "the chain presses on the rule"
    for leaf in (2, 4, 8):
        assert got[("random", 1, leaf)] == (1, 1, 1, 1) and got[("random", 8, leaf)] == (1, 1, 1, 1)
        assert got[("random", 9, leaf)][0] >= 1 and got[("random", 9, leaf)][3] >= 2


def test_the_key_and_the_split_rule_under_sanitizers(harness):
    """The quantisation gives a cell for every f32 input, NaN and infinite bounds included (nothing else reaches the conversion: the
    undefined-behaviour sanitizer watches it); zero and overflowing extents, 2^60; the key's bit layout; the split's two rules."""
    r = subprocess.run([harness, "keys"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "keys OK", r.stdout + r.stderr
