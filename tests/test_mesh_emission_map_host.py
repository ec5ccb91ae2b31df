"""Mesh emission maps on the host (include/rpt.h, "mesh emission maps"; CPU only): csrc/host_emap.h's checks answer in their order,
its decode equals numpy float32 with the oracle's strict pow, its lookup-and-apply and its sampler line equal a numpy float32
restatement bit for bit, mesh_form_emit_of gives 20 .. 27 for exactly the (normal maps, cutouts, environment) triples that give
12 .. 19 and is unchanged below 20, and the composer lends the all-zero material-map table exactly when no material map is ON
(tests/emap_harness.cpp, a stand-alone program built under g++'s address and undefined-behaviour sanitizers);
rpt_mesh_emission_map has C's layout and the ABI version did not move; the entry points reject what they can without a GPU; the
meshemit_* kernels live in a code object library of their own, use no scratch and at most 128 VGPRs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from kernel_census import code_object_kernels
from test_mesh_material_map_host import MAP_FORM_FIRST, MMAP_KERNELS
from test_mesh_material_map_host import OTHER_LIBS as MMAP_OTHER_LIBS
from test_mesh_texture_host import BILINEAR, CLAMP, NEAREST, REPEAT, coordinates, random_texels, restate_decode, restate_lookup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rust-pathtracer_amd")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
F = np.float32
EMIT_FORM_FIRST = 20


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emap") / "emap_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), os.path.join(ROOT, "tests", "emap_harness.cpp"), "-o", exe], check=True)
    return exe


def _run(harness, *args):
    r = subprocess.run([harness] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr
    return r.stdout


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the restatements (tests/test_gpu_mesh_emission_map.py imports them) -----------------------------------------------------------
def restate_st(u, v, uva, uvb, uvc):
    """"lookup": w = (1 - u) - v, then (w*sa + u*sb) + v*sc for s and for t, float32, one rounding per operation."""
    u, v, uva, uvb, uvc = (np.ascontiguousarray(x, F) for x in (u, v, uva, uvb, uvc))
    w = (F(1) - u) - v
    s = (w * uva[..., 0] + u * uvb[..., 0]) + v * uvc[..., 0]
    t = (w * uva[..., 1] + u * uvb[..., 1]) + v * uvc[..., 1]
    assert s.dtype == F and t.dtype == F
    return s, t


def restate_apply(emission, texels, wrap, filt, s, t):
    """"hit side": e.c * E.c over DECODED texels [h, w, 4] f32, for the (s, t) of the hits -> [n, 3] f32."""
    E = restate_lookup(texels, wrap, filt, s, t)
    out = np.asarray(emission, F)[None, :] * E[:, :3]
    assert out.dtype == F
    return out


def restate_sample_uv(r1, r2):
    """"sampler side": su = sqrt(r1), bu = 1 - su, bv = r2 * su, float32 (numpy's float32 root is correctly rounded)."""
    r1, r2 = np.ascontiguousarray(r1, F), np.ascontiguousarray(r2, F)
    su = np.sqrt(r1)
    assert su.dtype == F
    return F(1) - su, r2 * su


def restate_sample_emission(m_emission, n_f, texels, wrap, filt, s, t):
    """"sampler side": e.c = m.emission[c] * E.c, then N_f * e.c — the products in this order."""
    e = restate_apply(m_emission, texels, wrap, filt, s, t)
    out = F(n_f) * e
    assert out.dtype == F
    return out


# ---- decode, lookup, apply ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", (1.0, 2.2, 0.4545))
def test_host_decode_equals_numpy_and_the_oracles_pow(harness, oracle, tmp_path, gamma):
    """All 256 bytes in every channel (a 256-texel ramp whose four bytes differ): k / 255 at gamma 1, the oracle's strict pow otherwise,
    0 and 1 at the ends by definition, alpha ignored."""
    k = np.arange(256, dtype=np.uint32)
    ramp = np.stack([k, 255 - k, k ^ 0x55, (7 * k) % 256], 1).astype(np.uint8).reshape(1, 256, 4)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([256], np.uint32).tobytes() + np.array([gamma], F).tobytes() + ramp.tobytes())
    assert "decode OK" in _run(harness, "decode", src, dst)
    got = np.fromfile(dst, F).reshape(1, 256, 4)
    want = restate_decode(oracle, ramp, gamma)
    assert np.array_equal(_bits(got), _bits(want))
    assert got[0, 0, 0] == 0 and got[0, 255, 0] == 1 and not got[..., 3].any()
    if gamma == 1.0:
        assert np.array_equal(_bits(got[0, :, 0]), _bits(k.astype(F) / F(255)))


@pytest.mark.parametrize("wrap", (REPEAT, CLAMP))
@pytest.mark.parametrize("filt", (NEAREST, BILINEAR))
def test_host_lookup_and_apply_equal_the_numpy_restatement(harness, oracle, tmp_path, wrap, filt):
    """emap_reference (decode + lookup + apply) over a 3 x 5 map at gamma 2.2, at the texture test's coordinates pushed through a
    skewed UV triangle, so that tex_interp's three products all act."""
    w, h = 3, 5
    img = random_texels(w, h, 21)
    s0, t0 = coordinates(w, h, 22)
    s0, t0 = np.clip(s0, -3, 3), np.clip(t0, -3, 3)
    rows = np.zeros((len(s0), 11), F)
    rows[:, 0], rows[:, 1] = s0, t0
    rows[:, 2:8] = (0.25, -0.5, 1.5, 0.125, -0.75, 2.0)
    rows[:, 8:11] = (4.0, 2.5, 0.7)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([w, h, wrap, filt, len(s0)], np.uint32).tobytes() + np.array([2.2], F).tobytes() + img.tobytes() + rows.tobytes())
    assert "apply OK" in _run(harness, "apply", src, dst)
    got = np.fromfile(dst, F).reshape(-1, 3)
    s, t = restate_st(rows[:, 0], rows[:, 1], rows[:, 2:4], rows[:, 4:6], rows[:, 6:8])
    want = restate_apply((4.0, 2.5, 0.7), restate_decode(oracle, img, 2.2), wrap, filt, s, t)
    assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())
    assert len(np.unique(got[:, 0])) > 10


@pytest.mark.parametrize("wrap,filt", ((REPEAT, BILINEAR), (CLAMP, NEAREST)))
def test_host_sampler_line_equals_the_numpy_restatement(harness, oracle, tmp_path, wrap, filt):
    """bu, bv from r1, r2 (multiples of 2^-24, the ends included), the lookup at them, then N_f * (m.emission * E)."""
    w, h = 16, 16
    texels = restate_decode(oracle, random_texels(w, h, 31), 1.0)
    rng = np.random.default_rng(32)
    n = 2048
    r = (rng.integers(0, 1 << 24, (n, 2)).astype(np.float64) / (1 << 24)).astype(F)
    r[:4] = ((0, 0), (0, F(1) - F(2.0 ** -24)), (F(1) - F(2.0 ** -24), 0), (F(2.0 ** -24), F(2.0 ** -24)))
    rows = np.zeros((n, 12), F)
    rows[:, 0:2] = r
    rows[:, 2:8] = (0.1, 0.2, 1.3, -0.4, 0.6, 1.7)
    rows[:, 8:11] = (12.0, 7.5, 3.25)
    rows[:, 11] = 3.0
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([w, h, wrap, filt, n], np.uint32).tobytes() + texels.tobytes() + rows.tobytes())
    assert "sample OK" in _run(harness, "sample", src, dst)
    got = np.fromfile(dst, F).reshape(-1, 5)
    bu, bv = restate_sample_uv(r[:, 0], r[:, 1])
    assert np.array_equal(_bits(got[:, 0]), _bits(bu)) and np.array_equal(_bits(got[:, 1]), _bits(bv))
    s, t = restate_st(bu, bv, rows[:, 2:4], rows[:, 4:6], rows[:, 6:8])
    want = restate_sample_emission((12.0, 7.5, 3.25), 3.0, texels, wrap, filt, s, t)
    assert np.array_equal(_bits(got[:, 2:]), _bits(want))
    # the order of the products matters: N_f * (m * E) is not (N_f * m) * E everywhere
    other = (F(3.0) * np.array((12.0, 7.5, 3.25), F))[None, :] * restate_lookup(texels, wrap, filt, s, t)[:, :3]
    assert (_bits(other) != _bits(want)).any()


def test_host_checks_plan_layout_and_descriptors(harness):
    assert "checks OK" in _run(harness, "checks")


# ---- the forms and the composer ------------------------------------------------------------------------------------------------------
def test_the_emission_form_over_all_256_states(harness):
    """Without an emission map: mesh_form_ext_of's value, unchanged (all below 20).  With one: 20 + (form - 12) of the material-mapped
    form the same (normal maps, cutouts, environment) triple gives — whether a material map is ON or not; all of 20 .. 27 occur."""
    rows = [tuple(int(x) for x in line.split()) for line in _run(harness, "forms").splitlines()]
    assert [r[0] for r in rows] == list(range(256))
    seen = set()
    for bits, ext, emit in rows:
        smooth, lights, tex, env, cut, nrm, maps, emaps = ((bits >> i) & 1 for i in range(8))
        assert ext == rows[bits & 127][1] and ext < EMIT_FORM_FIRST
        if not emaps:
            assert emit == ext
            continue
        over = rows[(bits & 63) | 64][1]                              # the form a material map would take in this state
        if over < MAP_FORM_FIRST:
            assert emit == over and not (tex or env or cut or nrm)    # (unreachable: a map needs a texture)
            continue
        assert emit == over + 8 == EMIT_FORM_FIRST + (4 if nrm else 0) + (2 if cut else 0) + (1 if env else 0)
        assert emit == rows[bits ^ 64][2], "with or without a material map"
        seen.add(emit)
    assert seen == set(range(20, 28))


def test_the_composer_lends_the_zero_table_exactly_without_a_material_map(harness):
    out = _run(harness, "compose")
    assert "compose OK" in out
    head = None
    n = {"zero": 0, "own": 0}
    for line in out.splitlines():
        if line.startswith("maps "):
            head = line
        elif line.split()[-1] in n:
            assert (line.split()[-1] == "zero") == head.startswith("maps 0"), (head, line)
            n[line.split()[-1]] += 1
    assert n["zero"] == n["own"] == 24
    for form in ("light_tex", "env", "cut", "cut_env", "nrm", "nrm_env", "nrm_cut", "nrm_cut_env"):
        assert any(l.split()[0] == form for l in out.splitlines()), form


# ---- the interface -------------------------------------------------------------------------------------------------------------------
def test_rpt_mesh_emission_map_layout_matches_c(rpt, tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "rpt.h"
#define O(f) printf(#f " %zu\n", offsetof(rpt_mesh_emission_map, f))
int main(void) {
  printf("size %zu\n", sizeof(rpt_mesh_emission_map));
  O(mesh); O(mode); O(width); O(height); O(texels); O(filter); O(gamma);
  printf("abi %u\non %d\noff %d\n", (unsigned)RPT_ABI_VERSION, RPT_MESH_EMISSION_MAP_ON, RPT_MESH_EMISSION_MAP_OFF);
  return 0; }''')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    A = rpt._abi
    assert C.sizeof(A.rpt_mesh_emission_map) == int(out.pop("size"))
    assert int(out.pop("abi")) == A.RPT_ABI_VERSION == 5
    assert (int(out.pop("on")), int(out.pop("off"))) == (A.RPT_MESH_EMISSION_MAP_ON, A.RPT_MESH_EMISSION_MAP_OFF) == (1, 0)
    for f, off in out.items():
        assert getattr(A.rpt_mesh_emission_map, f).offset == int(off), f


def test_the_emission_map_calls_validate_without_gpu(rpt):
    lib, A = rpt.lib(), rpt._abi
    it = A.rpt_mesh_emission_map()
    assert lib.rpt_set_mesh_emission_maps(None, C.byref(it), 1) == A.RPT_ERR_INVALID_ARG
    assert lib.rpt_last_error(None).startswith(b"rpt_set_mesh_emission_maps: ")
    assert lib.rpt_download_mesh_emission_map(None, 0, None, 1, 1) == A.RPT_ERR_INVALID_ARG
    assert lib.rpt_last_error(None).startswith(b"rpt_download_mesh_emission_map: ")
    assert lib.rpt_debug_mesh_emission_map_query(None, None, 0, None, 0, None) == A.RPT_ERR_INVALID_ARG
    assert lib.rpt_debug_mesh_emission_map_sample(None, None, 0, None, None) == A.RPT_ERR_INVALID_ARG
    assert hasattr(rpt.Tracer, "set_mesh_emission_maps") and hasattr(rpt.Tracer, "download_mesh_emission_map")
    with pytest.raises(ValueError):
        rpt.Tracer.set_mesh_emission_maps(object(), {0: dict(texels=np.zeros((2, 2, 4), np.uint8), filter="cubic")})
    with pytest.raises(ValueError):
        rpt.Tracer.set_mesh_emission_maps(object(), {0: np.zeros((2, 2, 3), np.uint8)})


def test_the_emission_scene_is_the_light_scene_with_a_striped_lamp(rpt):
    from rust_pathtracer_amd import scenes
    s, textures, maps = scenes.mesh_emission_scene()
    base = scenes.mesh_light_scene()
    assert len(s.meshes) == len(base.meshes) and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(s.meshes, base.meshes))
    assert list(maps) == [1] and list(textures) == [1]
    img = maps[1]["texels"]
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 4 and img.shape[0] * img.shape[1] <= 64
    assert len(np.unique(img[..., 0])) >= 2, "stripes"
    assert len(textures[1]["uvs"]) == len(s.meshes[1][0])
    assert max(s.materials[s.meshes[1][2]].fields["emission"]) > 0


# ---- the library ---------------------------------------------------------------------------------------------------------------------
EMAP_KERNELS = ["meshemit_cut_env_regen_kernel", "meshemit_cut_regen_kernel", "meshemit_env_regen_kernel", "meshemit_nrm_cut_env_regen_kernel",
                "meshemit_nrm_cut_regen_kernel", "meshemit_nrm_env_regen_kernel", "meshemit_nrm_regen_kernel", "meshemit_query_kernel",
                "meshemit_regen_kernel", "meshemit_sample_kernel"]
OTHER_LIBS = MMAP_OTHER_LIBS + ("librpt_hip_mmap.so",)


def test_the_emission_map_kernels_have_a_code_object_of_their_own():
    """librpt_hip_emap.so (build.py, EMAP_LIB) holds exactly the ten meshemit_* kernels — no decode kernel: the decode is the texture
    library's — and exports exactly its ten launch functions; both libraries load it through their run path, no other library holds
    a meshemit_ kernel, and the material maps' library is what its own test says."""
    assert sorted(code_object_kernels(os.path.join(PKG, "librpt_hip_emap.so"))) == EMAP_KERNELS
    for lib in OTHER_LIBS:
        assert not [n for n in code_object_kernels(os.path.join(PKG, lib)) if n.startswith("meshemit_")], lib
    assert sorted(code_object_kernels(os.path.join(PKG, "librpt_hip_mmap.so"))) == MMAP_KERNELS
    for lib in ("librpt_hip.so", "librpt_hip_test.so"):
        dyn = subprocess.run(["readelf", "-d", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        assert "librpt_hip_emap.so" in dyn and "$ORIGIN" in dyn, lib
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(PKG, "librpt_hip_emap.so")], check=True, capture_output=True, text=True).stdout
    fns = sorted(line.split(" T ", 1)[1].split("(")[0] for line in out.splitlines() if " T " in line)
    assert fns == ["rptlaunch::mesh_emission_map_query", "rptlaunch::mesh_emission_map_sample", "rptlaunch::render_mesh_emit", "rptlaunch::render_mesh_emit_cut",
                   "rptlaunch::render_mesh_emit_cut_env", "rptlaunch::render_mesh_emit_env", "rptlaunch::render_mesh_emit_nrm", "rptlaunch::render_mesh_emit_nrm_cut",
                   "rptlaunch::render_mesh_emit_nrm_cut_env", "rptlaunch::render_mesh_emit_nrm_env"], out


def test_build_py_names_the_emission_map_library(rpt):
    import importlib.util
    spec = importlib.util.spec_from_file_location("_rpt_build_for_emap_test", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.EMAP_LIB == b.emap_lib_of(b.LIB) == os.path.join(PKG, "librpt_hip_emap.so")
    assert b.emap_lib_of("/x/y/libz.so") == "/x/y/libz_emap.so"
    parts = [o for o in b.OBJECTS if o[3] == "emap"]
    assert [o[0] for o in parts] == ["k_emap", "k_emap_nrm"] and all(o[1] == "k_emap.hip" and o[2][:len(b.PEROP)] == b.PEROP for o in parts)
    assert [o[2][len(b.PEROP):] for o in parts] == [["-DRPT_EMAP_PART=0"], ["-DRPT_EMAP_PART=1"]]
    assert "-ffp-contract=off" in b.BASE_FLAGS
    missing = os.path.join(PKG, "no_such_library.so")
    assert b.needs_build(b.LIB, b.MESH_LIB, b.REFIT_LIB, b.BUILD_LIB, b.MOVE_LIB, b.SMOOTH_LIB, b.LIGHT_LIB, b.TEX_LIB, b.ENV_LIB, b.CUT_LIB, b.NRM_LIB, missing) is True     # (the twelfth is still mmap_lib)
    assert b.needs_build(b.LIB, emap_lib=missing) is True


def test_the_emission_map_kernels_use_no_scratch_and_at_most_128_vgprs(tmp_path):
    """The kernels' metadata, read the way tools/kernel_meta.py reads it: no private segment, no spilled vector register; the render
    forms have mesh_regen_kernel's launch bounds (256 lanes, 4 waves per SIMD: 512 / 4 = 128 VGPRs)."""
    llvm = os.path.join(ROCM, "lib", "llvm", "bin")
    fat, co = str(tmp_path / "fatbin"), str(tmp_path / "co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", os.path.join(PKG, "librpt_hip_emap.so"), fat], check=True)
    data = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), data)] + [len(data)]
    assert len(starts) == 3, "one offload bundle per translation unit: k_emap and k_emap_nrm"
    blocks = []
    for i, (lo, hi) in enumerate(zip(starts, starts[1:])):
        part = "%s.%d" % (fat, i)
        open(part, "wb").write(data[lo:hi])
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + part,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
        txt = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        blocks += txt.split("  - .agpr_count:")[1:]
    assert len(blocks) == len(EMAP_KERNELS)
    regen = 0
    for blk in blocks:
        g = lambda k: int(re.search(r"\.%s:\s*(\d+)" % k, blk).group(1))      # noqa: E731
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0, name
        if "regen" in name:
            regen += 1
            assert g("max_flat_workgroup_size") == 256 and g("vgpr_count") <= 128, name
    assert regen == 8
