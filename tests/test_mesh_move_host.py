"""rpt_update_meshes_device / rpt_rebuild_meshes_device on the host (include/rpt.h, "moving meshes from device memory"; CPU only):
csrc/host_move.h's transform and check, which k_move.hip compiles for the device, equal a numpy float32 restatement bit for bit and
its host checks answer in their order (under g++'s address and undefined-behaviour sanitizers: tests/move_harness.cpp);
rpt_mesh_source has C's layout; the three entry points reject a NULL context without a GPU; and the meshmove_* kernels live in a code
object library of their own and use no scratch."""
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


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("move") / "move_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "move_harness.cpp"), "-o", exe], check=True)
    return exe


# ---- the numpy float32 restatement (tests/test_gpu_mesh_move.py imports it) --------------------------------------------------------
def restate_move(v, transform):
    """include/rpt.h's statement on float32 arrays, one rounding per operation: out[c] = ((t[4c]*x + t[4c+1]*y) + t[4c+2]*z) + t[4c+3];
    no transform: the words as they are."""
    v = np.ascontiguousarray(v, F).reshape(-1, 3)
    if transform is None:
        return v.copy()
    t = np.asarray(transform, F).reshape(12)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([((t[4 * c] * x + t[4 * c + 1] * y) + t[4 * c + 2] * z) + t[4 * c + 3] for c in range(3)], axis=1).astype(F)


def restate_check(p, referenced):
    """-> (the largest |coordinate| over referenced vertices as bits, 0xFFFFFFFF - the lowest vertex that is not finite or 0)"""
    mag = p.view(np.uint32) & np.uint32(0x7FFFFFFF)
    ref = mag[np.asarray(referenced, bool)]
    big = int(ref.max()) if ref.size else 0
    bad = np.nonzero((mag >= 0x7F800000).any(axis=1))[0]
    return big, (0xFFFFFFFF - int(bad[0])) if len(bad) else 0


IDENTITY = F([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])


def transforms():
    c, s = np.cos(0.7), np.sin(0.7)
    return [("NULL", None),
            ("identity", IDENTITY),
            ("rotation with translation", F([c, -s, 0, 0.25, s, c, 0, -1.5, 0, 0, 1, 3.0])),
            ("shear with scales 2^+-20", F([2.0 ** 20, 0.5, 0, 1, 0, 2.0 ** -20, 0.25, -2, 0.125, 0, 1, 2.0 ** -20])),
            ("overflow", F([2.0 ** 100, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]))]


OVERFLOW_AT = (1234, 2999)            # the vertices whose x = 2^30 overflows under the last transform (2^130)
UNREFERENCED = (7, 1234, 3500)


def move_inputs(n=4001, seed=3):
    """A few thousand vertices with zeros of both signs and subnormals among them; the vertices of UNREFERENCED are used by no
    triangle, and 3500 — one of them — holds the largest coordinate."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-2, 2, (n, 3)).astype(F)
    v[0] = [-0.0, 0.0, -0.0]
    v[1] = [2.0 ** -140, -2.0 ** -149, 1.0]
    v[3500] = [1000.0, -3.0, 0.5]
    for k in OVERFLOW_AT:
        v[k, 0] = F(2.0 ** 30)
    referenced = np.ones(n, np.uint8)
    referenced[list(UNREFERENCED)] = 0
    return v, referenced


def _run(harness, tmp_path, v, referenced, transform):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.uint32([len(v), 0 if transform is None else 1]).tobytes())
        f.write((np.zeros(12, F) if transform is None else np.asarray(transform, F)).tobytes())
        f.write(np.ascontiguousarray(v, F).tobytes())
        f.write(np.ascontiguousarray(referenced, np.uint8).tobytes())
    r = subprocess.run([harness, "run", src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "run OK", r.stdout + r.stderr
    raw = np.fromfile(dst, np.uint32)
    return raw[:-2].view(F).reshape(-1, 3), int(raw[-2]), int(raw[-1])


@pytest.mark.parametrize("which", range(5))
def test_transform_and_check_equal_the_numpy_restatement(harness, tmp_path, which):
    what, t = transforms()[which]
    v, referenced = move_inputs()
    got, big, bad = _run(harness, tmp_path, v, referenced, t)
    want = restate_move(v, t)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s: %d words differ" % (what, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    assert (big, bad) == restate_check(want, referenced), what
    if what == "NULL":
        assert np.array_equal(got.view(np.uint32), v.view(np.uint32)) and got.view(np.uint32)[0, 0] == 0x80000000      # -0 stays -0
        assert bad == 0 and big == F(2.0 ** 30).view(np.uint32), "the largest REFERENCED coordinate: vertex 2999's, not 3500's or 1234's"
    if what == "identity":
        assert np.array_equal(got, v) and list(got.view(np.uint32)[0]) == [0, 0, 0]                                   # ... and an identity loses it
        assert got.view(np.uint32)[1, 1] == 0x80000001, "subnormals pass through"
    if what == "overflow":
        assert bad == 0xFFFFFFFF - OVERFLOW_AT[0], "the lowest offending vertex, referenced or not"
        assert np.isinf(got[list(OVERFLOW_AT), 0]).all() and np.isfinite(np.delete(got, OVERFLOW_AT, axis=0)).all()
    else:
        assert bad == 0 and np.isfinite(got).all()
    if what == "rotation with translation":
        assert not np.array_equal(got, v)


def test_the_check_ignores_unreferenced_vertices_for_the_maximum_only(harness, tmp_path):
    v, referenced = move_inputs()
    v[list(OVERFLOW_AT), 0] = 1.0
    _, big, bad = _run(harness, tmp_path, v, referenced, None)
    assert bad == 0 and 0 < big < int(F(2.0).view(np.uint32)), "vertex 3500's 1000 is referenced by no triangle"
    referenced[3500] = 1
    _, big, bad = _run(harness, tmp_path, v, referenced, None)
    assert big == F(1000.0).view(np.uint32)
    v[7, 2], v[9, 0] = np.nan, -np.inf                               # vertex 7 is unreferenced and still checked; it is the lowest
    _, _, bad = _run(harness, tmp_path, v, referenced, None)
    assert bad == 0xFFFFFFFF - 7
    _, _, bad = _run(harness, tmp_path, v, referenced, IDENTITY)
    assert bad == 0xFFFFFFFF - 7
    _, big, bad = _run(harness, tmp_path, v[:0], referenced[:0], IDENTITY)      # no vertices: nothing
    assert (big, bad) == (0, 0)


def test_host_checks_in_their_order(harness):
    r = subprocess.run([harness, "checks"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "checks OK", r.stdout + r.stderr


def test_rpt_mesh_source_layout_matches_c(rpt, tmp_path):
    prog = tmp_path / "source_layout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "rpt.h"
int main(void) {
  printf("size %zu\n", sizeof(rpt_mesh_source)); printf("mesh %zu\n", offsetof(rpt_mesh_source, mesh));
  printf("n_vertices %zu\n", offsetof(rpt_mesh_source, n_vertices)); printf("vertices_dev %zu\n", offsetof(rpt_mesh_source, vertices_dev));
  printf("transform %zu\n", offsetof(rpt_mesh_source, transform)); printf("abi %u\n", RPT_ABI_VERSION);
  return 0; }''')
    exe = tmp_path / "source_layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    A = rpt._abi
    assert C.sizeof(A.rpt_mesh_source) == int(out["size"]) == 24
    for f in ("mesh", "n_vertices", "vertices_dev", "transform"):
        assert getattr(A.rpt_mesh_source, f).offset == int(out[f]), f
    assert int(out["abi"]) == A.RPT_ABI_VERSION == 5                  # additive: the ABI version did not move


def test_the_device_source_calls_validate_without_gpu(rpt):
    lib, A = rpt.lib(), rpt._abi
    src = (A.rpt_mesh_source * 1)()
    src[0].mesh, src[0].n_vertices = 0, 1
    out = np.zeros(3, F)
    for name, call in (("rpt_update_meshes_device", lambda: lib.rpt_update_meshes_device(None, src, 1)),
                       ("rpt_rebuild_meshes_device", lambda: lib.rpt_rebuild_meshes_device(None, src, 1)),
                       ("rpt_download_mesh_vertices", lambda: lib.rpt_download_mesh_vertices(None, 0, out.ctypes.data, 1))):
        assert call() == A.RPT_ERR_INVALID_ARG, name
        assert name.encode() in lib.rpt_last_error(None), name
    assert lib.rpt_update_meshes_device(None, None, 0) == A.RPT_ERR_INVALID_ARG
    assert lib.rpt_rebuild_meshes_device(None, None, 0) == A.RPT_ERR_INVALID_ARG


def test_the_move_kernels_have_a_code_object_of_their_own():
    """librpt_hip_move.so (build.py, MOVE_LIB) holds exactly the two meshmove_* kernels and exports exactly its two launch functions;
    both libraries load it through their run path, and no other library holds a meshmove_ kernel."""
    assert sorted(code_object_kernels(os.path.join(PKG, "librpt_hip_move.so"))) == ["meshmove_apply_kernel", "meshmove_check_kernel"]
    for lib in ("librpt_hip.so", "librpt_hip_test.so", "librpt_hip_mesh.so", "librpt_hip_refit.so", "librpt_hip_build.so"):
        assert not [n for n in code_object_kernels(os.path.join(PKG, lib)) if n.startswith("meshmove_")], lib
    for lib in ("librpt_hip.so", "librpt_hip_test.so"):
        dyn = subprocess.run(["readelf", "-d", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        assert "librpt_hip_move.so" in dyn and "$ORIGIN" in dyn, lib
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(PKG, "librpt_hip_move.so")], check=True, capture_output=True, text=True).stdout
    fns = sorted(line.split(" T ", 1)[1].split("(")[0] for line in out.splitlines() if " T " in line)
    assert fns == ["rptlaunch::move_apply", "rptlaunch::move_check"], out
    # the product exports the three new entry points
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "librpt_hip.so")], check=True, capture_output=True, text=True).stdout
    for name in ("rpt_update_meshes_device", "rpt_rebuild_meshes_device", "rpt_download_mesh_vertices"):
        assert re.search(r" T %s$" % name, out, re.M), name


def test_build_py_names_the_move_library(rpt):
    """build.py: move_lib_of beside the other three, and needs_build's earlier positional parameters still mean what they meant."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_rpt_build_for_test", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.MOVE_LIB == b.move_lib_of(b.LIB) == os.path.join(PKG, "librpt_hip_move.so")
    assert b.move_lib_of("/x/y/libz.so") == "/x/y/libz_move.so"
    assert any(o[0] == "k_move" and o[1] == "k_move.hip" and o[3] == "move" for o in b.OBJECTS)
    missing = os.path.join(PKG, "no_such_library.so")
    assert b.needs_build(b.LIB, b.MESH_LIB, b.REFIT_LIB, missing) is True            # (the fourth positional parameter is still build_lib)
    assert b.needs_build(b.LIB, b.MESH_LIB, b.REFIT_LIB, b.BUILD_LIB, missing) is True


def test_the_move_kernels_use_no_scratch(tmp_path):
    """The kernels' metadata, read the way tools/kernel_meta.py reads it: no private segment, no spilled register, no LDS beyond the
    check's reduction (4 waves x 2 words)."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
    fat, co = str(tmp_path / "fatbin"), str(tmp_path / "co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", os.path.join(PKG, "librpt_hip_move.so"), fat], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
    txt = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    blocks = txt.split("  - .agpr_count:")[1:]
    assert len(blocks) == 2
    for blk in blocks:
        g = lambda k: int(re.search(r"\.%s:\s*(\d+)" % k, blk).group(1))      # noqa: E731
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        assert "meshmove_" in name
        assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0, name
        assert g("group_segment_fixed_size") == (32 if "check" in name else 0) and g("vgpr_count") <= 64, name
    # every global write is a vector store or a vector atomic
    asm = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    writes = set(re.findall(r"^\s*(\w*(?:store|atomic)\w*)", asm, re.M))
    assert writes and all(w.startswith("global_") for w in writes), writes
