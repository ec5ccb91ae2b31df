"""Mesh material maps on the host (include/rpt.h, "mesh material maps"; CPU only): csrc/host_mmap.h's checks answer in their order,
its decode and its lookup-and-apply equal a numpy float32 restatement bit for bit, BILINEAR over factors in [0, 1] never leaves
[0, 1] and returns a constant image exactly only for the bytes 0 and 255, mesh_form_ext_of picks the twenty forms as stated and the
composer binds every base part as mesh_scene_of<Base> does (tests/mmap_harness.cpp, a stand-alone program built under g++'s address
and undefined-behaviour sanitizers); rpt_mesh_material_map has C's layout and the ABI version did not move; the entry points reject
what they can without a GPU; and the meshmap_* kernels live in a code object library of their own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from kernel_census import MESH_RENDER_KERNELS, code_object_kernels
from test_mesh_normal_map_host import NRM_KERNELS
from test_mesh_normal_map_host import OTHER_LIBS as NRM_OTHER_LIBS
from test_mesh_texture_host import BILINEAR, CLAMP, NEAREST, REPEAT, coordinates, random_texels, restate_lookup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rust-pathtracer_amd")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
F = np.float32
NONE = 0xFFFFFFFF
CHANNELS = (0, 1, 2, 3, NONE)
# What `mmap_harness bilinear` settled (include/rpt.h, "lookup at the hit"): BILINEAR never exceeds 1, and a constant image comes back
# exactly only when its byte is 0 or 255.  tests/test_gpu_mesh_material_map.py reads this: it repeats "a constant map is a material
# edit" under BILINEAR for those two bytes alone.
BILINEAR_CONSTANT_EXACT_BYTES = (0, 255)
# the eight textured forms a material map sits over, in mesh_form_ext_of's order: form 12 + i is the map over TEXTURED_FORMS[i]
TEXTURED_FORMS = ["meshtex_light_regen_kernel", "meshenv_regen_kernel", "meshcut_regen_kernel", "meshcut_env_regen_kernel", "meshnrm_regen_kernel",
                  "meshnrm_env_regen_kernel", "meshnrm_cut_regen_kernel", "meshnrm_cut_env_regen_kernel"]
MAP_FORM_FIRST = 12


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mmap") / "mmap_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), os.path.join(ROOT, "tests", "mmap_harness.cpp"), "-o", exe], check=True)
    return exe


def _run(harness, *args):
    r = subprocess.run([harness] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr
    return r.stdout


# ---- the restatements (tests/test_gpu_mesh_material_map.py imports them) -----------------------------------------------------------
def restate_value(k):
    """c(k) of include/rpt.h, "decode", in float32."""
    c = np.asarray(k).astype(F) / F(255)
    assert c.dtype == F
    return c


def restate_decode(rgba, roughness_channel, metallic_channel):
    """include/rpt.h, "decode": [h, w, 4] uint8 -> [h, w, 4] f32 {fr, fm, 0, 0}; a channel None or NONE gives exactly 1."""
    rgba = np.asarray(rgba, np.uint8)
    out = np.zeros(rgba.shape[:2] + (4,), F)
    for i, ch in enumerate((roughness_channel, metallic_channel)):
        out[..., i] = F(1) if ch is None or ch == NONE else restate_value(rgba[..., ch])
    return out


def restate_apply(roughness, metallic, texels, wrap, filt, s, t):
    """"lookup at the hit" and "apply" on float32 arrays: (roughness * fr, metallic * fm) for s, t of the hit, over DECODED texels."""
    f = restate_lookup(texels, wrap, filt, s, t)
    r, m = F(roughness) * f[:, 0], F(metallic) * f[:, 1]
    assert r.dtype == F and m.dtype == F
    return r, m


# ---- decode --------------------------------------------------------------------------------------------------------------------------
def test_host_decode_equals_numpy_for_every_byte_and_channel_choice(harness, tmp_path):
    """All 256 bytes x the five choices of each channel: a 256-texel ramp whose four bytes differ (k, 255 - k, k ^ 0x55, (7 k) mod 256)."""
    k = np.arange(256, dtype=np.uint32)
    ramp = np.stack([k, 255 - k, k ^ 0x55, (7 * k) % 256], 1).astype(np.uint8).reshape(1, 256, 4)
    for rc in CHANNELS:
        for mc in CHANNELS:
            src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
            with open(src, "wb") as f:
                f.write(np.array([256, rc, mc], np.uint32).tobytes() + ramp.tobytes())
            assert "decode OK" in _run(harness, "decode", src, dst)
            got = np.fromfile(dst, F).reshape(1, 256, 4)
            want = restate_decode(ramp, rc, mc)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rc, mc)
            if rc != NONE:
                assert set(np.unique(ramp[..., rc])) == set(range(256))
    assert restate_value(0) == 0 and restate_value(255) == 1
    assert np.all(np.diff(restate_value(np.arange(256))) > 0), "c is strictly increasing"


@pytest.mark.parametrize("wrap", (REPEAT, CLAMP))
@pytest.mark.parametrize("filt", (NEAREST, BILINEAR))
def test_host_factors_and_apply_equal_the_numpy_restatement(harness, tmp_path, wrap, filt):
    """mmap_factors + mmap_apply against restate_apply over a 3 x 5 map and the texture test's coordinates: u = s, v = t over the
    unit UV triangle {(0, 0), (1, 0), (0, 1)} make tex_interp return them through its own three products."""
    w, h = 3, 5
    texels = restate_decode(random_texels(w, h, 11), 1, 2)
    s, t = coordinates(w, h, 12)
    rows = np.zeros((len(s), 10), F)
    rows[:, 0], rows[:, 1] = s, t
    rows[:, 4], rows[:, 7] = 1, 1                                     # (sb, tb) = (1, 0), (sc, tc) = (0, 1)
    rows[:, 8], rows[:, 9] = F(0.7), F(0.9)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([w, h, wrap, filt, len(s)], np.uint32).tobytes() + texels.tobytes() + rows.tobytes())
    assert "factors OK" in _run(harness, "factors", src, dst)
    got = np.fromfile(dst, F).reshape(-1, 2)
    wgt = (F(1) - s) - t
    ss, tt = (wgt * F(0) + s * F(1)) + t * F(0), (wgt * F(0) + s * F(0)) + t * F(1)
    want_r, want_m = restate_apply(0.7, 0.9, texels, wrap, filt, ss, tt)
    assert np.array_equal(got[:, 0].view(np.uint32), want_r.view(np.uint32)) and np.array_equal(got[:, 1].view(np.uint32), want_m.view(np.uint32))
    assert len(np.unique(got[:, 0])) > 10


def test_bilinear_stays_in_range_and_is_exact_only_for_0_and_255(harness):
    """The two questions of include/rpt.h, over all 256 x 256 byte pairs x 65 weights x both blends of tex_lookup: no value above 1 or
    below 0 (so the statement has no clamp); a constant image is NOT returned exactly in general, but the all-0 and the all-255 one are."""
    out = dict(line.split() for line in _run(harness, "bilinear").splitlines())
    out = {k: int(v) for k, v in out.items()}
    assert out["taps"] == 256 * 256 * 65 * 2
    assert out["above_one"] == 0 and out["below_zero"] == 0
    assert out["constant_inexact"] > 0, "were BILINEAR constant-exact, include/rpt.h and the GPU test's BILINEAR cases would say so"
    assert out["constant_inexact_0_255"] == 0
    assert BILINEAR_CONSTANT_EXACT_BYTES == (0, 255)


def test_host_checks_plan_layout_and_descriptors(harness):
    assert "checks OK" in _run(harness, "checks")


# ---- the forms and the composer ----------------------------------------------------------------------------------------------------------
def test_the_extended_form_over_all_128_states(harness):
    """mesh_form_ext_of equals mesh_form_of whenever no map is ON or the scene is untextured; with a map, 12 + the index of the textured
    form that would have run, the plain textured form counting as the textured mesh-light one; all of 12 .. 19 occur, picked by (normal
    maps, cutouts, environment)."""
    rows = [tuple(int(x) for x in line.split()) for line in _run(harness, "forms").splitlines()]
    assert [r[0] for r in rows] == list(range(128))
    seen = set()
    for bits, base, ext in rows:
        smooth, lights, tex, env, cut, nrm, maps = ((bits >> i) & 1 for i in range(7))
        assert base == rows[bits & 63][1]
        if not maps:
            assert ext == base
            continue
        name = MESH_RENDER_KERNELS[base]
        if name == "meshtex_regen_kernel":
            name = "meshtex_light_regen_kernel"                       # empty light tables, as normal maps do it
        if name not in TEXTURED_FORMS:
            assert ext == base and not (tex or env or cut or nrm)      # (unreachable: a map needs a texture)
            continue
        assert ext == MAP_FORM_FIRST + TEXTURED_FORMS.index(name)
        assert ext == MAP_FORM_FIRST + (4 if nrm else 0) + (2 if cut else 0) + (1 if env else 0)
        seen.add(ext)
    assert seen == set(range(12, 20))
    assert len(MESH_RENDER_KERNELS) == MAP_FORM_FIRST


def test_the_composer_binds_the_base_as_mesh_scene_of_does(harness):
    """The eight forms, with and without mesh lights, SMOOTH meshes and an environment of either mode: every base field equals
    mesh_scene_of<Base>'s, the map's pointers lie in its allocation at its layout's offsets, and the one table the map's allocation
    lends — tri_light of the form over the textured mesh-light tables while no mesh is ON — is lent exactly then."""
    out = _run(harness, "compose")
    assert "compose OK" in out
    lines = out.splitlines()
    lent = [(h, l) for h, l in zip(lines, lines[1:]) if l.endswith(" lent")]
    assert lent and all(l == "light_tex lent" and h.startswith("lights 0 env 0") for h, l in lent)
    for form in ("light_tex", "env", "cut", "cut_env", "nrm", "nrm_env", "nrm_cut", "nrm_cut_env"):
        assert any(l.split()[0] == form for l in lines), form


# ---- the interface -------------------------------------------------------------------------------------------------------------------
def test_rpt_mesh_material_map_layout_matches_c(rpt, tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "rpt.h"
#define O(f) printf(#f " %zu\n", offsetof(rpt_mesh_material_map, f))
int main(void) {
  printf("size %zu\n", sizeof(rpt_mesh_material_map));
  O(mesh); O(mode); O(width); O(height); O(texels); O(filter); O(roughness_channel); O(metallic_channel);
  printf("abi %u\nnone %u\non %d\noff %d\n", (unsigned)RPT_ABI_VERSION, (unsigned)RPT_MATERIAL_MAP_CHANNEL_NONE, RPT_MESH_MATERIAL_MAP_ON, RPT_MESH_MATERIAL_MAP_OFF);
  return 0; }''')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    A = rpt._abi
    assert C.sizeof(A.rpt_mesh_material_map) == int(out.pop("size"))
    assert int(out.pop("abi")) == A.RPT_ABI_VERSION == 5
    assert int(out.pop("none")) == A.RPT_MATERIAL_MAP_CHANNEL_NONE == NONE
    assert (int(out.pop("on")), int(out.pop("off"))) == (A.RPT_MESH_MATERIAL_MAP_ON, A.RPT_MESH_MATERIAL_MAP_OFF) == (1, 0)
    for f, off in out.items():
        assert getattr(A.rpt_mesh_material_map, f).offset == int(off), f


def test_the_material_map_calls_validate_without_gpu(rpt):
    lib, A = rpt.lib(), rpt._abi
    it = A.rpt_mesh_material_map()
    assert lib.rpt_set_mesh_material_maps(None, C.byref(it), 1) == A.RPT_ERR_INVALID_ARG
    assert lib.rpt_last_error(None).startswith(b"rpt_set_mesh_material_maps: ")
    assert lib.rpt_download_mesh_material_map(None, 0, None, 1, 1) == A.RPT_ERR_INVALID_ARG
    assert lib.rpt_last_error(None).startswith(b"rpt_download_mesh_material_map: ")
    assert lib.rpt_debug_mesh_material_map_query(None, None, 0, None, 0, None) == A.RPT_ERR_INVALID_ARG
    assert lib.rpt_debug_mesh_form(None, None) == A.RPT_ERR_INVALID_ARG
    assert hasattr(rpt.Tracer, "set_mesh_material_maps") and hasattr(rpt.Tracer, "mesh_material_map")


# ---- the library -----------------------------------------------------------------------------------------------------------------------
MMAP_KERNELS = ["meshmap_cut_env_regen_kernel", "meshmap_cut_regen_kernel", "meshmap_decode_kernel", "meshmap_env_regen_kernel",
                "meshmap_nrm_cut_env_regen_kernel", "meshmap_nrm_cut_regen_kernel", "meshmap_nrm_env_regen_kernel", "meshmap_nrm_regen_kernel",
                "meshmap_query_kernel", "meshmap_regen_kernel"]
OTHER_LIBS = NRM_OTHER_LIBS + ("librpt_hip_nrm.so",)


def test_the_material_map_kernels_have_a_code_object_of_their_own():
    """librpt_hip_mmap.so (build.py, MMAP_LIB) holds exactly the ten meshmap_* kernels and exports exactly its ten launch functions;
    both libraries load it through their run path, no other library holds a meshmap_ kernel, and the normal maps' library is what its
    own test says."""
    assert sorted(code_object_kernels(os.path.join(PKG, "librpt_hip_mmap.so"))) == MMAP_KERNELS
    for lib in OTHER_LIBS:
        assert not [n for n in code_object_kernels(os.path.join(PKG, lib)) if n.startswith("meshmap_")], lib
    assert sorted(code_object_kernels(os.path.join(PKG, "librpt_hip_nrm.so"))) == NRM_KERNELS
    for lib in ("librpt_hip.so", "librpt_hip_test.so"):
        dyn = subprocess.run(["readelf", "-d", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        assert "librpt_hip_mmap.so" in dyn and "$ORIGIN" in dyn, lib
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(PKG, "librpt_hip_mmap.so")], check=True, capture_output=True, text=True).stdout
    fns = sorted(line.split(" T ", 1)[1].split("(")[0] for line in out.splitlines() if " T " in line)
    assert fns == ["rptlaunch::mesh_material_map_query", "rptlaunch::mmap_decode", "rptlaunch::render_mesh_map", "rptlaunch::render_mesh_map_cut",
                   "rptlaunch::render_mesh_map_cut_env", "rptlaunch::render_mesh_map_env", "rptlaunch::render_mesh_map_nrm", "rptlaunch::render_mesh_map_nrm_cut",
                   "rptlaunch::render_mesh_map_nrm_cut_env", "rptlaunch::render_mesh_map_nrm_env"], out


def test_build_py_names_the_material_map_library(rpt):
    """build.py: mmap_lib_of beside the other eleven, one source built as two objects, and needs_build's earlier positional parameters
    still mean what they meant."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_rpt_build_for_mmap_test", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.MMAP_LIB == b.mmap_lib_of(b.LIB) == os.path.join(PKG, "librpt_hip_mmap.so")
    assert b.mmap_lib_of("/x/y/libz.so") == "/x/y/libz_mmap.so"
    parts = [o for o in b.OBJECTS if o[3] == "mmap"]
    assert [o[0] for o in parts] == ["k_mmap", "k_mmap_nrm"] and all(o[1] == "k_mmap.hip" and o[2][:len(b.PEROP)] == b.PEROP for o in parts)
    assert [o[2][len(b.PEROP):] for o in parts] == [["-DRPT_MMAP_PART=0"], ["-DRPT_MMAP_PART=1"]]
    missing = os.path.join(PKG, "no_such_library.so")
    assert b.needs_build(b.LIB, b.MESH_LIB, b.REFIT_LIB, b.BUILD_LIB, b.MOVE_LIB, b.SMOOTH_LIB, b.LIGHT_LIB, b.TEX_LIB, b.ENV_LIB, b.CUT_LIB, missing) is True     # (the eleventh is still nrm_lib)
    assert b.needs_build(b.LIB, b.MESH_LIB, b.REFIT_LIB, b.BUILD_LIB, b.MOVE_LIB, b.SMOOTH_LIB, b.LIGHT_LIB, b.TEX_LIB, b.ENV_LIB, b.CUT_LIB, b.NRM_LIB, missing) is True
    assert b.needs_build(b.LIB, mmap_lib=missing) is True
