"""Radiance queries on the CPU (include/rpt.h, "radiance queries"): the float64 restatement of a sample along a ray no camera sends
(tests/radiance_f64.py), the near-tie condition of the rays tests/test_gpu_radiance_f64.py compares on an MI355X, the planted faults,
the census of the kernels' library, and the host-side form choice and argument composition (tests/rad_harness.cpp, a stand-alone
program built under g++'s address and undefined-behaviour sanitizers).

Seventeen cases, 200 rays each (radiance_f64.probe_rays: origins uniform in the box of the scene's mesh vertices grown by half its
size on every side, directions uniform on the sphere and normalised in float32; the generator's key is [61, k] for case k), one sample
per ray of frame FRAME on the stream of index FIRST_INDEX + i:
  media A .. H        scenes.mesh_media_scene at four bounces under the composed file's inputs, the medium of
                      tests/test_mesh_media_f64.py's MEDIA on the glass icosphere (the render's forms 28 .. 35) — MediaMeshPath
  both maps A .. H    the composed scene with material and emission maps ON (forms 20 .. 27) — EmapPath
  flat                the composed file's scene with nothing set (form 11) — pt_f64.Path over the mesh scene

The near-tie condition (test_the_near_tie_count_of_the_restatement): of each case's 200 samples, those at or below TAU by the
restatement's own margins / those that carry radiance, counted again on every run; the cap is test_path_f64's NEAR_TIE_MAX (24 of
200) and is a condition, not a measurement.  No case's ray seed had to be changed to stay under it:
  media      A 5 / 66   B 3 / 192   C 5 / 59   D 5 / 197   E 5 / 69   F 2 / 193   G 5 / 61   H 1 / 195
  both maps  A 6 / 84   B 3 / 198   C 7 / 74   D 5 / 200   E 4 / 80   F 6 / 194   G 2 / 66   H 3 / 198
  flat       2 / 53

Planted faults (test_the_restatement_sees_each_fault), each a single line of tests/radiance_f64.py, clean samples moved beyond
REL_CLEAN against the unfaulted restatement, counted again on every run (FAULT_MOVES below): draws_not_discarded 70 and
key_without_first_index 75 of media B's 200, starts_inside_medium 12 on media A.  starts_inside_medium runs on rays whose origins
lie in the icosphere's own box, so that a good part of them start inside the medium.

The spreads (tests/f32_spread.py; test_the_spreads_of_the_restatement): every ray of every case has one, cached beside the restated
values for both legs (2 to 2.8 s of CPU time per case); every sample that carries radiance has a non-zero one; at most 0.52 % of a
case's clean samples have a tolerance above 1e-3; the 99th percentile is 2e-6 to 3e-5, the largest 1.1e-3 on a clean sample (media
E) and 0.43 on one of both maps B, which REL_CLEAN caps."""
import os
import re
import subprocess

import numpy as np
import pytest

import f32_spread as S
import radiance_f64 as R
import test_mesh_frames_f64 as TF
from kernel_census import code_object_kernels
from mesh_media_f64 import MediaMeshDescScene, MediaMeshPath
from test_gpu_mesh_compose_f64 import CASES, inputs
from test_mesh_media_f64 import MEDIA
from test_mesh_media_f64 import scene as media_scene
from test_path_f64 import NEAR_TIE_MAX, REL_CLEAN, TAU, rel_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rust-pathtracer_amd")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SEED, FRAME, FIRST_INDEX, N_RAYS = 601, 3, 1000, 200
ALL_CASES = [("media", c) for c in sorted(CASES)] + [("both maps", c) for c in sorted(CASES)] + [("flat", TF.FLAT)]
CASE_IDS = ["%s-%s" % k for k in ALL_CASES]
ENTRY_POINTS = ["rpt_camera_sample_rays_device", "rpt_radiance", "rpt_radiance_device"]
RAD_KERNELS = ["radiance_camera_rays_kernel", "radiance_cut_env_kernel", "radiance_cut_kernel", "radiance_env_kernel", "radiance_kernel",
               "radiance_nrm_cut_env_kernel", "radiance_nrm_cut_kernel", "radiance_nrm_env_kernel", "radiance_nrm_kernel"]
# kernels per code object of every other library, as the commit before radiance queries built them
OTHER_LIBS = {"librpt_hip.so": 63, "librpt_hip_test.so": 67, "librpt_hip_mesh.so": 2, "librpt_hip_refit.so": 2, "librpt_hip_build.so": 350,
              "librpt_hip_move.so": 2, "librpt_hip_smooth.so": 4, "librpt_hip_light.so": 7, "librpt_hip_tex.so": 5, "librpt_hip_env.so": 7,
              "librpt_hip_cut.so": 4, "librpt_hip_nrm.so": 6, "librpt_hip_mmap.so": 10, "librpt_hip_emap.so": 10, "librpt_hip_med.so": 9,
              "librpt_hip_query.so": 9}
# Counted on the CPU (test_the_near_tie_count_of_the_restatement prints the figures): (samples at or below TAU, samples with radiance).
COUNTS = {
    ('media', 'A'): (5, 66),
    ('media', 'B'): (3, 192),
    ('media', 'C'): (5, 59),
    ('media', 'D'): (5, 197),
    ('media', 'E'): (5, 69),
    ('media', 'F'): (2, 193),
    ('media', 'G'): (5, 61),
    ('media', 'H'): (1, 195),
    ('both maps', 'A'): (6, 84),
    ('both maps', 'B'): (3, 198),
    ('both maps', 'C'): (7, 74),
    ('both maps', 'D'): (5, 200),
    ('both maps', 'E'): (4, 80),
    ('both maps', 'F'): (6, 194),
    ('both maps', 'G'): (2, 66),
    ('both maps', 'H'): (3, 198),
    ('flat', 'flat'): (2, 53),
}
# fault -> (stack, case, clean samples moved beyond REL_CLEAN)
FAULT_MOVES = {"draws_not_discarded": ("media", "B", 70), "key_without_first_index": ("media", "B", 75), "starts_inside_medium": ("media", "A", 12)}


def scene_of(stack, case):
    """The scene of a case, as the GPU leg uploads it."""
    if stack == "media":
        return media_scene()
    if stack == "both maps":
        return TF.ME.scene()
    return TF.flat_scene()[0]


def path_of(stack, case):
    if stack == "media":
        s = media_scene()
        return MediaMeshPath(MediaMeshDescScene(s.describe(), s, media={0: MEDIA[case]}, **inputs(s, case)))
    if stack == "both maps":
        return TF.path_of(case)
    return TF.P.Path(TF.flat_scene()[1], (), False)


def rays_of(stack, case):
    """The case's 200 rays [200, 8] f32: the same words on both sides of the GPU comparison."""
    k = ALL_CASES.index((stack, case))
    return R.probe_rays(scene_of(stack, case), N_RAYS, [61, k])


_RESTATED = {}


def restated(oracle, stack, case):
    """The restatement of the case's rays, computed once for every test that needs it, CPU or GPU: (radiance [200, 3], margins [200]).
    Nobody writes to them."""
    key = (stack, case)
    if key not in _RESTATED:
        rad, marg = R.sample_rays(path_of(stack, case), oracle, SEED, FRAME, rays_of(stack, case), first_index=FIRST_INDEX)
        rad.setflags(write=False)
        marg.setflags(write=False)
        _RESTATED[key] = (rad, marg)
    return _RESTATED[key]


_SPREADS = {}


def spreads(oracle, stack, case):
    """The f32 spreads (tests/f32_spread.py) of all 200 rays of the case, cached beside _RESTATED for the CPU and the GPU leg:
    (spreads [200], CPU seconds)."""
    key = (stack, case)
    if key not in _SPREADS:
        path, rays = path_of(stack, case), rays_of(stack, case)
        s, seconds = S.timed_spread(lambda: R.sample_rays(path, oracle, SEED, FRAME, rays, first_index=FIRST_INDEX), plain=restated(oracle, stack, case)[0])
        s.setflags(write=False)
        _SPREADS[key] = (s, seconds)
    return _SPREADS[key]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_the_rays_are_what_the_file_says():
    for stack, case in (("media", "A"), ("flat", TF.FLAT)):
        r = rays_of(stack, case)
        assert r.shape == (N_RAYS, 8) and r.dtype == np.float32 and np.array_equal(r.view(np.uint32), rays_of(stack, case).view(np.uint32))
        assert np.isinf(r[:, 3]).all() and not r[:, 7].any()
        assert np.abs(np.sqrt((r[:, 4:7].astype(np.float64) ** 2).sum(1)) - 1.0).max() < 1e-6
        verts = np.concatenate([np.asarray(v, np.float64).reshape(-1, 3) for v, _, _ in scene_of(stack, case).meshes])
        lo, hi = verts.min(0), verts.max(0)
        assert (r[:, 0:3] >= lo - 0.5 * (hi - lo) - 1e-5).all() and (r[:, 0:3] <= hi + 0.5 * (hi - lo) + 1e-5).all()
        outside = ((r[:, 0:3] < lo) | (r[:, 0:3] > hi)).any(axis=1)
        assert 0.5 < outside.mean() < 1.0, "most origins lie outside the meshes' own box, some inside"


def test_the_helper_puts_the_camera_back(oracle):
    """first_segment swaps pt_f64.gen_ray for the length of a call only, also when the call raises; a camera sample afterwards is
    what it was before."""
    path = path_of("flat", TF.FLAT)
    dr = oracle.rng_f32(5, 0, 7, R.N_DRAWS)
    before = path.sample(3, 2, 8, 6, dr)
    gen_ray, state = R.P.gen_ray, R.MS.PathState
    R.sample(path, (0.0, 1.0, 3.0), (0.0, 0.0, -1.0), dr)
    with pytest.raises(StopIteration):
        R.sample(path, (0.0, 1.0, 3.0), (0.0, 0.0, -1.0), dr[:1])
    assert R.P.gen_ray is gen_ray and R.MS.PathState is state
    after = path.sample(3, 2, 8, 6, dr)
    assert before[0] == after[0] and before[2] == after[2]
    # and along the camera's own ray the helper gives the camera sample: the same draws, the two first spent on the jitter
    o, d = gen_ray(path.scene.cam, (3.0 / 8.0, 1.0 - (6.0 - 3.0) / 6.0), (float(dr[0]), float(dr[1])), 8.0, 6.0)
    along = R.sample(path, o, d, dr)
    assert along[0] == before[0] and along[2] == before[2]


@pytest.mark.parametrize("stack,case", ALL_CASES, ids=CASE_IDS)
def test_the_near_tie_count_of_the_restatement(rpt, oracle, stack, case):
    """The restatement alone over exactly the rays of the GPU comparison: no more than the project's 12 % of the samples lie at or
    below TAU, more than a quarter carry radiance, and both counts are the ones in this file."""
    radiance, margins = restated(oracle, stack, case)
    below, lit = int((margins <= TAU).sum()), int((radiance.max(axis=1) > 0).sum())
    print("%s %s: %d of %d samples below TAU (%.2f %%), %d with radiance" % (stack, case, below, len(margins), 100.0 * below / len(margins), lit))
    assert len(margins) == N_RAYS and below <= NEAR_TIE_MAX * N_RAYS and lit > N_RAYS // 4
    assert (below, lit) == COUNTS[(stack, case)]


@pytest.mark.parametrize("stack,case", ALL_CASES, ids=CASE_IDS)
def test_the_spreads_of_the_restatement(rpt, oracle, stack, case):
    """The conditions of the comparison with spreads, on the restatement alone: every ray has a spread, at least 100 of the case's
    clean samples among them, and at most 5 % of the clean samples have a tolerance above 1e-3."""
    radiance, margins = restated(oracle, stack, case)
    s, seconds = spreads(oracle, stack, case)
    assert len(s) == N_RAYS and not np.isnan(s).any()
    S.case_conditions("%s %s" % (stack, case), [(SEED, None, radiance, margins)], [s], seconds)
    hit = radiance.max(axis=1) > 0
    print("%s %s: %d of the %d samples with radiance have a non-zero spread" % (stack, case, int((s[hit] > 0).sum()), int(hit.sum())))


def fault_rays(fault, stack, case):
    """The rays a fault is held to: the case's own; for starts_inside_medium with the origins moved into the icosphere's own box."""
    r = rays_of(stack, case).copy()
    if fault == "starts_inside_medium":
        v = np.asarray(scene_of(stack, case).meshes[0][0], np.float64).reshape(-1, 3)
        lo, hi = v.min(0), v.max(0)
        r[:, 0:3] = (lo + np.random.default_rng(62).uniform(size=(N_RAYS, 3)) * (hi - lo)).astype(np.float32)
    return r


@pytest.mark.parametrize("fault", R.FAULTS)
def test_the_restatement_sees_each_fault(rpt, oracle, fault):
    """A restatement with one line of the section wrong moves clean samples beyond REL_CLEAN: a device with that fault would fail the
    comparison on the GPU."""
    stack, case, count = FAULT_MOVES[fault]
    path, rays = path_of(stack, case), fault_rays(fault, stack, case)
    base, marg = R.sample_rays(path, oracle, SEED, FRAME, rays, first_index=FIRST_INDEX)
    moved, marg2 = R.sample_rays(path, oracle, SEED, FRAME, rays, first_index=FIRST_INDEX, fault=fault)
    far = (rel_distance(np.nan_to_num(moved), np.nan_to_num(base)) > REL_CLEAN) & (marg > TAU) & (marg2 > TAU)
    print("%s (%s %s): %d clean samples beyond REL_CLEAN" % (fault, stack, case, int(far.sum())))
    assert far.sum() >= 1, fault
    assert int(far.sum()) == count
    if fault == "starts_inside_medium":
        inside = sum(R.medium_around(path.scene, tuple(float(x) for x in r[0:3])) is not None for r in rays)
        assert N_RAYS // 8 < inside < N_RAYS, "%d origins inside the medium" % inside


# ---- the interface and the library ------------------------------------------------------------------------------------------------------
def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(rpt_[a-z0-9_]+)\s*\(", src))


def test_the_entry_points_are_product_symbols(rpt):
    """This test fails without the feature: the header declares none of the three."""
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
    lib, bad = rpt.lib(), rpt._abi.RPT_ERR_INVALID_ARG
    assert lib.rpt_radiance_device(None, None, 0, None, 0, 1, 1, 0, 0, None) == bad and b"ctx is NULL" in lib.rpt_last_error(None)
    assert lib.rpt_radiance(None, None, 0, None, 0, 1, 1, 0, 0) == bad and lib.rpt_camera_sample_rays_device(None, 4, 4, 0, 1, None, None) == bad


def test_the_radiance_kernels_have_a_code_object_of_their_own():
    """librpt_hip_rad.so (build.py, RAD_LIB) holds exactly the nine radiance_* kernels; both libraries load it through their run
    path; no other library holds a radiance_ kernel, and none gained or lost a kernel."""
    assert sorted(code_object_kernels(os.path.join(PKG, "librpt_hip_rad.so"))) == RAD_KERNELS
    for lib, count in OTHER_LIBS.items():
        names = code_object_kernels(os.path.join(PKG, lib))
        assert not [n for n in names if n.startswith("radiance_")], lib
        assert len(names) == count, "%s: %d kernels, not %d" % (lib, len(names), count)
    assert sorted(f for f in os.listdir(PKG) if f.endswith(".so")) == sorted(list(OTHER_LIBS) + ["librpt_hip_rad.so"])
    for lib in ("librpt_hip.so", "librpt_hip_test.so"):
        dyn = subprocess.run(["readelf", "-d", os.path.join(PKG, lib)], check=True, capture_output=True, text=True).stdout
        assert "librpt_hip_rad.so" in dyn and "$ORIGIN" in dyn, lib
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", os.path.join(PKG, "librpt_hip_rad.so")], check=True, capture_output=True, text=True).stdout
    fns = sorted(line.split(" T ", 1)[1].split("(")[0] for line in out.splitlines() if " T " in line)
    assert fns == ["rptlaunch::radiance", "rptlaunch::radiance_camera_rays", "rptlaunch::radiance_cut", "rptlaunch::radiance_cut_env", "rptlaunch::radiance_env",
                   "rptlaunch::radiance_max_spp", "rptlaunch::radiance_nrm", "rptlaunch::radiance_nrm_cut", "rptlaunch::radiance_nrm_cut_env",
                   "rptlaunch::radiance_nrm_env"], out


def test_build_py_names_the_radiance_library(rpt):
    import importlib.util
    spec = importlib.util.spec_from_file_location("_rpt_build_for_radiance_test", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.RAD_LIB == b.rad_lib_of(b.LIB) == os.path.join(PKG, "librpt_hip_rad.so")
    assert b.rad_lib_of("/x/y/libz.so") == "/x/y/libz_rad.so"
    parts = [o for o in b.OBJECTS if o[3] == "rad"]
    assert [(o[0], o[1]) for o in parts] == [("k_rad", "k_rad.hip"), ("k_rad_nrm", "k_rad.hip")]
    assert [o[2] for o in parts] == [b.PEROP + ["-DRPT_RAD_PART=0"], b.PEROP + ["-DRPT_RAD_PART=1"]], "strict arithmetic, as k_med.hip"
    assert "-ffp-contract=off" in b.BASE_FLAGS
    assert b.needs_build(b.LIB, rad_lib=os.path.join(PKG, "no_such_library.so")) is True


def test_the_radiance_forms_run_four_workgroups_per_cu(tmp_path):
    """The kernels' metadata, read the way tools/kernel_meta.py reads it: no private segment, no spilled vector register, 256 lanes; the
    eight forms hold at most 40 KiB of LDS — the walk's 24 KiB stack and the lane tables — and at most 128 VGPRs: four workgroups of
    four waves per CU, the media forms' occupancy (160 KiB / 4, 512 / 4).  The camera's kernel has no LDS."""
    llvm = os.path.join(ROCM, "lib", "llvm", "bin")
    fat, co = str(tmp_path / "fatbin"), str(tmp_path / "co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", os.path.join(PKG, "librpt_hip_rad.so"), fat], check=True)
    data = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), data)] + [len(data)]
    assert len(starts) == 3, "one offload bundle per translation unit: k_rad and k_rad_nrm"
    blocks = []
    for i, (lo, hi) in enumerate(zip(starts, starts[1:])):
        part = "%s.%d" % (fat, i)
        open(part, "wb").write(data[lo:hi])
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + part,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
        txt = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        blocks += txt.split("  - .agpr_count:")[1:]
    assert len(blocks) == len(RAD_KERNELS)
    forms = 0
    for blk in blocks:
        g = lambda k: int(re.search(r"\.%s:\s*(\d+)" % k, blk).group(1))      # noqa: E731
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0, name      # (no scratch: the cut forms park 8 SGPRs in VGPR lanes)
        assert g("max_flat_workgroup_size") == 256, name
        if "camera" in name:
            assert g("group_segment_fixed_size") == 0, name
        else:
            forms += 1
            agprs = int(blk.split()[0])                               # (the block starts behind its .agpr_count key)
            assert 24 * 1024 < g("group_segment_fixed_size") <= 40 * 1024 and g("vgpr_count") + agprs <= 128, name
    assert forms == 8


# ---- the form choice and the composer ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rad") / "rad_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), os.path.join(ROOT, "tests", "rad_harness.cpp"), "-o", exe], check=True)
    return exe


def _run(harness, *args):
    r = subprocess.run([harness] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr
    return r.stdout


def test_the_form_choice_and_the_cut_into_launches(harness):
    out = _run(harness, "forms")
    assert re.search(r"forms OK (\d+)", out) and int(re.search(r"forms OK (\d+)", out).group(1)) == 40


def test_the_composer_binds_the_media_s_tables_or_the_query_s_own(harness):
    out = _run(harness, "compose")
    assert out.rstrip().endswith("compose OK")
    lines = [l for l in out.splitlines() if l.startswith("radiance")]
    assert len(lines) == 2 * (4 * 2 + 16 * 5), "without a texture two forms, with one five; with and without media"
    assert "radiance media lent emap lent mmap lent tex lent lights lent smooth lent" in lines, "a scene with nothing ON"
    assert "radiance_nrm_cut_env media own emap own mmap own tex own lights own smooth own" in lines, "a scene with everything ON"
    assert sum("media lent" in l for l in lines) == sum("media own" in l for l in lines)
