"""Mesh media on the host (include/rpt.h, "mesh media"; CPU only): csrc/host_med.h's checks answer in their order and a rejected call
leaves the table as it was, the anisotropy is clamped as Material::finalize clamps it, a three-mesh scene whose middle mesh carries
the medium gets that mesh's triangles and no other into tri_medium, mesh_form_med_of gives 28 .. 35 for exactly the (normal maps,
cutouts, environment) triples and is mesh_form_emit_of's value without a medium, and the composer lends its empty tables exactly
while the feature each stands for is absent (tests/med_harness.cpp, a stand-alone program built under g++'s address and
undefined-behaviour sanitizers); rpt_mesh_medium has C's layout and the ABI version did not move; the entry points reject what they
can without a GPU; the meshmed_* kernels live in a code object library of their own, use no scratch and at most 128 VGPRs; and the
numpy float32 restatement of the side test that tests/test_gpu_mesh_media.py holds the probe to."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from kernel_census import code_object_kernels
from test_mesh_emission_map_host import EMAP_KERNELS
from test_mesh_emission_map_host import OTHER_LIBS as EMAP_OTHER_LIBS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rust-pathtracer_amd")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
F = np.float32
MED_FORM_FIRST = 28
NO_MEDIUM = 0xFFFF
INVALID, NO_SCENE, UNSUPPORTED = -1, -4, -5


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("med") / "med_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), os.path.join(ROOT, "tests", "med_harness.cpp"), "-o", exe], check=True)
    return exe


def _run(harness, *args):
    r = subprocess.run([harness] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr
    return r.stdout


# ---- the restatement (tests/test_gpu_mesh_media.py imports it) ---------------------------------------------------------------------
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def flat_normal(tris, index):
    """G = normalize(cross(e1, e2)) of the flattened triangles `index`, float32, one rounding per operation: three divides by the
    correctly rounded root of dot(g, g)."""
    tris = np.ascontiguousarray(tris, F)
    e1, e2 = tris[index, 1] - tris[index, 0], tris[index, 2] - tris[index, 0]
    with np.errstate(all="ignore"):
        g = _cross(e1, e2)
        n = g / np.sqrt(_dot(g, g))[:, None]
    assert n.dtype == F
    return n


def restate_side(scene, tris, rays9, index):
    """-> (dot(l, G) per ray as float32, 0 where nothing is hit; the fraction of mesh 0's hits whose SMOOTH normal differs from G).
    `rays9`: [n, 9] f32 {o, d, l}; `index`: the winning triangle per ray or -1."""
    from test_gpu_mesh_smooth import _restate_query
    rays9 = np.ascontiguousarray(rays9, F)
    hit = index >= 0
    side = np.zeros(len(rays9), F)
    g = flat_normal(tris, index[hit])
    side[hit] = _dot(rays9[hit, 6:9], g)
    assert side.dtype == F
    rays7 = np.concatenate([rays9[:, :6], np.full((len(rays9), 1), 3.0e38, F)], 1)
    _, smooth, _ = _restate_query(scene, (0,), rays7)
    on0 = hit & (index < len(np.asarray(scene.meshes[0][1]).reshape(-1, 3)))
    differs = (smooth[on0] != flat_normal(tris, index[on0])).any(axis=1).mean() if on0.any() else 0.0
    return side, float(differs)


def test_the_flat_normal_restatement_is_a_unit_vector_across_the_plane():
    rng = np.random.default_rng(12)
    tris = rng.normal(size=(64, 3, 3)).astype(F)
    n = flat_normal(tris, np.arange(64)).astype(np.float64)
    e1, e2 = (tris[:, 1] - tris[:, 0]).astype(np.float64), (tris[:, 2] - tris[:, 0]).astype(np.float64)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)
    assert np.abs((n * e1).sum(1)).max() < 1e-5 and np.abs((n * e2).sum(1)).max() < 1e-5
    assert ((n * np.cross(e1, e2)).sum(1) > 0).all(), "not turned: along cross(e1, e2)"


# ---- the checks, the clamp, the tables --------------------------------------------------------------------------------------------------
def test_every_check_answers_in_its_order_and_a_rejected_call_changes_nothing(harness):
    """This test fails without the feature: there is no csrc/host_med.h to build the harness from.  The harness itself holds that
    every rejected call leaves both the current table and the output untouched; here are the codes, the messages and their order —
    each case carries the next check's fault as well."""
    out = _run(harness, "checks")
    assert "checks OK" in out
    want = [("no scene", NO_SCENE, "needs an uploaded scene with meshes"),
            ("2^32 vertices", UNSUPPORTED, "2^32 vertices"),
            ("NULL items", INVALID, "items is NULL"),
            ("mesh out of range", INVALID, "item 0: mesh 3 out of range (the scene has 3)"),
            ("named twice", INVALID, "item 1: mesh 0 is named twice"),
            ("type", INVALID, "medium_type 4"),
            ("negative density", INVALID, "density -1"),
            ("infinite density", INVALID, "density inf"),
            ("nan density", INVALID, "density"),
            ("colour", INVALID, "the colour is not finite"),
            ("anisotropy", INVALID, "the anisotropy is not finite"),
            ("a later item", INVALID, "item 1: mesh 0: the anisotropy"),
            ("too many", UNSUPPORTED, "32767 meshes would carry a medium: a path can remember 32766")]
    lines = [l for l in out.splitlines() if ": " in l and not l.startswith(("clamp", "tri_medium"))]
    assert len(lines) == len(want)
    for line, (what, code, says) in zip(lines, want):
        head, rest = line.split(": ", 1)
        assert head == what and int(rest.split()[0]) == code, line
        assert rest.split(" ", 1)[1].startswith("rpt_set_mesh_media: ") and says in rest, line


def test_the_clamp_is_material_finalizes(harness):
    """f32::clamp(-0.9, 0.9) on the bits: numpy's float32 clip gives the same words, -0 stays -0, the neighbours of +-0.9 are cut."""
    out = _run(harness, "checks")
    rows = [l.split()[1:] for l in out.splitlines() if l.startswith("clamp ")]
    assert len(rows) == 12
    g = np.array([int(a, 16) for a, _ in rows], np.uint32).view(F)
    got = np.array([int(b, 16) for _, b in rows], np.uint32)
    assert np.array_equal(got, np.clip(g, F(-0.9), F(0.9)).view(np.uint32))
    assert got[1] == 0x80000000 and got[4] == got[2] and got[5] == got[3] and got[2] != np.array([g[4]]).view(np.uint32)[0]


def test_tri_medium_of_a_three_mesh_scene_whose_middle_mesh_carries_the_medium(harness):
    out = _run(harness, "checks")
    line, = [l for l in out.splitlines() if l.startswith("tri_medium")]
    assert [int(x) for x in line.split()[1:]] == [NO_MEDIUM, NO_MEDIUM, 0, 0, 0, NO_MEDIUM]      # meshes of 2, 3 and 1 triangles


def test_the_form_is_28_to_35_with_a_medium_and_unchanged_without(harness):
    """Bits from the lowest up: smooth, lights, textured, environment, cutouts, normal_maps, material_maps, emission_maps, media.
    Cutouts and normal maps need a texture; maps need one too: only such combinations are held."""
    seen = set()
    for line in _run(harness, "forms").splitlines():
        b, emit, med = (int(x) for x in line.split())
        smooth, lights, tex, env, cut, nrm, mmap, emap, media = ((b >> k) & 1 for k in range(9))
        if (cut or nrm or mmap or emap) and not tex:
            continue
        if not media:
            assert med == emit and med < 28, line
            continue
        assert med == MED_FORM_FIRST + 4 * nrm + 2 * cut + env, line
        if emap:
            assert med == emit + 8, line                             # over the emission-mapped form that ran before
        seen.add(med)
    assert seen == set(range(28, 36))


def test_the_composer_lends_each_empty_table_exactly_while_its_feature_is_absent(harness):
    """Under the sanitizers every lent table is read through the argument's own pointers over a real allocation filled as the device's
    is.  Every base field equals the emission-mapped composer's over the same inputs but for the three lent pointers."""
    out = _run(harness, "compose")
    assert "compose OK" in out
    head, n = None, {}
    for line in out.splitlines():
        if line.startswith("bits "):
            head = [int(x) for x in line.split()[1::2]]
            continue
        w = line.split()
        if len(w) != 9:
            continue
        bits = head[0]
        emaps, lights, tex, smooth = bits & 1, bits & 4, bits & 8, bits & 16
        assert w[2] == ("own" if emaps else "lent") and w[4] == ("own" if tex else "lent"), (head, line)
        assert w[6] == ("own" if lights else "lent") and w[8] == ("own" if smooth else "lent"), (head, line)
        assert (w[0] in ("env", "cut_env", "nrm_env", "nrm_cut_env")) == (head[1] > 0)
        n[w[0]] = n.get(w[0], 0) + 1
    assert sorted(n) == sorted(["light_tex", "env", "cut", "cut_env", "nrm", "nrm_env", "nrm_cut", "nrm_cut_env"])
    assert n["light_tex"] == 20 and n["env"] == 40 and n["cut"] == n["nrm"] == n["nrm_cut"] == 16 and n["cut_env"] == 32


# ---- the interface -------------------------------------------------------------------------------------------------------------------
def test_rpt_mesh_medium_layout_matches_c(rpt, tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "rpt.h"
#define O(f) printf(#f " %zu\n", offsetof(rpt_mesh_medium, f))
int main(void) {
  printf("size %zu\n", sizeof(rpt_mesh_medium));
  O(mesh); O(medium_type); O(density); O(color); O(anisotropy);
  printf("abi %u\nnone %d\nemissive %d\n", (unsigned)RPT_ABI_VERSION, RPT_MEDIUM_NONE, RPT_MEDIUM_EMISSIVE);
  return 0; }''')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    A = rpt._abi
    assert C.sizeof(A.rpt_mesh_medium) == int(out.pop("size")) == 28
    assert int(out.pop("abi")) == A.RPT_ABI_VERSION == 5
    assert (int(out.pop("none")), int(out.pop("emissive"))) == (A.RPT_MEDIUM_NONE, A.RPT_MEDIUM_EMISSIVE) == (0, 3)
    for f, off in out.items():
        assert getattr(A.rpt_mesh_medium, f).offset == int(off), f


def test_the_media_calls_validate_without_gpu(rpt):
    lib, A = rpt.lib(), rpt._abi
    it = A.rpt_mesh_medium()
    assert lib.rpt_set_mesh_media(None, C.byref(it), 1) == A.RPT_ERR_INVALID_ARG
    assert lib.rpt_last_error(None).startswith(b"rpt_set_mesh_media: ")
    assert lib.rpt_download_mesh_medium(None, 0, C.byref(it)) == A.RPT_ERR_INVALID_ARG
    assert lib.rpt_last_error(None).startswith(b"rpt_download_mesh_medium: ")
    assert lib.rpt_debug_mesh_media_query(None, None, 0, None, 0, None) == A.RPT_ERR_INVALID_ARG
    assert hasattr(rpt.Tracer, "set_mesh_media") and hasattr(rpt.Tracer, "download_mesh_medium")
    with pytest.raises(ValueError):
        rpt.Tracer.set_mesh_media(object(), {0: dict(type="fog", density=1.0, color=(1, 1, 1))})
    with pytest.raises(ValueError):
        rpt.Tracer.set_mesh_media(object(), {0: dict(type="absorb", density=1.0, color=(1, 1))})
    for name in ("rpt_set_mesh_media", "rpt_download_mesh_medium"):
        assert name in open(os.path.join(ROOT, "include", "rpt.h")).read()
        assert hasattr(C.CDLL(os.path.join(PKG, "librpt_hip.so")), name), "the product library exports it"
    assert "set_mesh_media" in open(os.path.join(ROOT, "include", "rpt.hpp")).read()
    assert not hasattr(C.CDLL(os.path.join(PKG, "librpt_hip.so")), "rpt_debug_mesh_media_query"), "the probe is the test library's only"


def test_the_media_scene_is_the_light_scene_with_a_glass_object(rpt):
    from rust_pathtracer_amd import scenes
    base = scenes.mesh_light_scene(sphere_light=True)
    for kind in ("absorb", "scatter", "emissive", None):
        s, media = scenes.mesh_media_scene(kind)
        assert len(s.meshes) == 2 and sum(len(np.asarray(t).reshape(-1, 3)) for _, t, _ in s.meshes) == 82
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] for a, b in zip(s.meshes, base.meshes))
        assert s.any_hit_uses_max_dist and len(s.lights) == 1
        glass = s.materials[s.meshes[0][2]].fields
        assert glass["spec_trans"] == 1.0 and glass["ior"] == 1.45 and glass["roughness"] <= 0.1
        assert s.materials[1].fields == base.materials[1].fields, "the lamp is the light scene's"
        assert list(media) == [0] and (media[0] is None) == (kind is None)
        if kind:
            assert media[0]["type"] == kind and media[0]["density"] > 0 and len(media[0]["color"]) == 3
    with pytest.raises(ValueError):
        scenes.mesh_media_scene("smoke")


# ---- the library ---------------------------------------------------------------------------------------------------------------------
MED_KERNELS = ["meshmed_cut_env_regen_kernel", "meshmed_cut_regen_kernel", "meshmed_env_regen_kernel", "meshmed_nrm_cut_env_regen_kernel",
               "meshmed_nrm_cut_regen_kernel", "meshmed_nrm_env_regen_kernel", "meshmed_nrm_regen_kernel", "meshmed_query_kernel",
               "meshmed_regen_kernel"]
OTHER_LIBS = EMAP_OTHER_LIBS + ("librpt_hip_emap.so",)


def test_the_media_kernels_have_a_code_object_of_their_own():
    """librpt_hip_med.so (build.py, MED_LIB) holds exactly the eight forms and the probe and exports exactly its nine launch functions;
    both libraries load it through their run path, no other library holds a meshmed_ kernel, and the emission maps' library is what
    its own test says."""
    assert sorted(code_object_kernels(os.path.join(PKG, "librpt_hip_med.so"))) == MED_KERNELS
    for lib in OTHER_LIBS:
        assert not [n for n in code_object_kernels(os.path.join(PKG, lib)) if n.startswith("meshmed_")], lib
    assert sorted(code_object_kernels(os.path.join(PKG, "librpt_hip_emap.so"))) == EMAP_KERNELS
    for lib in ("librpt_hip.so", "librpt_hip_test.so"):
        dyn = subprocess.run(["readelf", "-d", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        assert "librpt_hip_med.so" in dyn and "$ORIGIN" in dyn, lib
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(PKG, "librpt_hip_med.so")], check=True, capture_output=True, text=True).stdout
    fns = sorted(line.split(" T ", 1)[1].split("(")[0] for line in out.splitlines() if " T " in line)
    assert fns == ["rptlaunch::mesh_media_query", "rptlaunch::render_mesh_med", "rptlaunch::render_mesh_med_cut", "rptlaunch::render_mesh_med_cut_env",
                   "rptlaunch::render_mesh_med_env", "rptlaunch::render_mesh_med_nrm", "rptlaunch::render_mesh_med_nrm_cut",
                   "rptlaunch::render_mesh_med_nrm_cut_env", "rptlaunch::render_mesh_med_nrm_env"], out


def test_build_py_names_the_media_library(rpt):
    import importlib.util
    spec = importlib.util.spec_from_file_location("_rpt_build_for_med_test", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.MED_LIB == b.med_lib_of(b.LIB) == os.path.join(PKG, "librpt_hip_med.so")
    assert b.med_lib_of("/x/y/libz.so") == "/x/y/libz_med.so"
    parts = [o for o in b.OBJECTS if o[3] == "med"]
    assert [o[0] for o in parts] == ["k_med", "k_med_nrm"] and all(o[1] == "k_med.hip" and o[2][:len(b.PEROP)] == b.PEROP for o in parts)
    assert [o[2][len(b.PEROP):] for o in parts] == [["-DRPT_MED_PART=0"], ["-DRPT_MED_PART=1"]]
    assert "-ffp-contract=off" in b.BASE_FLAGS
    assert b.needs_build(b.LIB, med_lib=os.path.join(PKG, "no_such_library.so")) is True


def test_the_media_kernels_use_no_scratch_and_at_most_128_vgprs(tmp_path):
    """The kernels' metadata, read the way tools/kernel_meta.py reads it: no private segment, no spilled vector register; the render
    forms have mesh_regen_kernel's launch bounds (256 lanes, 4 waves per SIMD: 512 / 4 = 128 VGPRs)."""
    llvm = os.path.join(ROCM, "lib", "llvm", "bin")
    fat, co = str(tmp_path / "fatbin"), str(tmp_path / "co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", os.path.join(PKG, "librpt_hip_med.so"), fat], check=True)
    data = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), data)] + [len(data)]
    assert len(starts) == 3, "one offload bundle per translation unit: k_med and k_med_nrm"
    blocks = []
    for i, (lo, hi) in enumerate(zip(starts, starts[1:])):
        part = "%s.%d" % (fat, i)
        open(part, "wb").write(data[lo:hi])
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + part,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
        txt = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        blocks += txt.split("  - .agpr_count:")[1:]
    assert len(blocks) == len(MED_KERNELS)
    regen = 0
    for blk in blocks:
        g = lambda k: int(re.search(r"\.%s:\s*(\d+)" % k, blk).group(1))      # noqa: E731
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0, name
        if "regen" in name:
            regen += 1
            assert g("max_flat_workgroup_size") == 256 and g("vgpr_count") <= 128, name
    assert regen == 8
