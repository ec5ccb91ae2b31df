"""Build the HIP extension for gfx950, in-tree: librpt_hip.so (the product: exactly include/rpt.h) and librpt_hip_test.so (the SAME
objects linked with the test hooks of include/rpt_test.h and the probe kernels: what the GPU parity tests load).

    python rust-pathtracer_amd/build.py
"""
import glob
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "librpt_hip.so")
TEST_LIB = os.path.join(HERE, "librpt_hip_test.so")
# The mesh scene class's kernels (k_mesh.hip) are a code object library of their own, named after the library that loads it through
# its run path ($ORIGIN) — mesh_lib_of(lib): an experiment build next to the product (tools/) gets its own — so the census of each
# library's own kernels (tests/test_gpu_image_kernels.py, tests/kernel_census.py) stays what it was; tests/test_mesh_host.py keeps
# the census of this one.  The test build loads the product's.


def mesh_lib_of(lib):
    return os.path.splitext(os.path.abspath(lib))[0] + "_mesh.so"


MESH_LIB = mesh_lib_of(LIB)


# The refit kernels of rpt_update_meshes (k_refit.hip) are a third code object library, named, linked and found the same way:
# tests/test_mesh_update_host.py keeps its census.
def refit_lib_of(lib):
    return os.path.splitext(os.path.abspath(lib))[0] + "_refit.so"


REFIT_LIB = refit_lib_of(LIB)


# The hierarchy build of rpt_rebuild_meshes (k_build.hip: its bvhbuild_* kernels and the rocPRIM kernels of its sort and prefix sums)
# is a fourth, again named, linked and found the same way: tests/test_mesh_rebuild_host.py keeps its census.
def build_lib_of(lib):
    return os.path.splitext(os.path.abspath(lib))[0] + "_build.so"


BUILD_LIB = build_lib_of(LIB)


# The kernels of the device-source mesh calls (k_move.hip: meshmove_*) are a fifth, again named, linked and found the same way:
# tests/test_mesh_move_host.py keeps its census.
def move_lib_of(lib):
    return os.path.splitext(os.path.abspath(lib))[0] + "_move.so"


MOVE_LIB = move_lib_of(LIB)


# The kernels of smooth mesh shading (k_smooth.hip: meshsmooth_*) are a sixth, again named, linked and found the same way:
# tests/test_mesh_smooth_host.py keeps its census.
def smooth_lib_of(lib):
    return os.path.splitext(os.path.abspath(lib))[0] + "_smooth.so"


SMOOTH_LIB = smooth_lib_of(LIB)


# The kernels of mesh lights (k_light.hip: meshlight_*) are a seventh, again named, linked and found the same way:
# tests/test_mesh_light_host.py keeps its census.
def light_lib_of(lib):
    return os.path.splitext(os.path.abspath(lib))[0] + "_light.so"


LIGHT_LIB = light_lib_of(LIB)


# The kernels of mesh textures (k_tex.hip: meshtex_*) are an eighth, again named, linked and found the same way:
# tests/test_mesh_texture_host.py keeps its census.
def tex_lib_of(lib):
    return os.path.splitext(os.path.abspath(lib))[0] + "_tex.so"


TEX_LIB = tex_lib_of(LIB)


# The kernels of environment lighting (k_env.hip: meshenv_*) are a ninth, again named, linked and found the same way:
# tests/test_mesh_env_host.py keeps its census.
def env_lib_of(lib):
    return os.path.splitext(os.path.abspath(lib))[0] + "_env.so"


ENV_LIB = env_lib_of(LIB)


# The kernels of mesh cutouts (k_cut.hip: meshcut_*) are a tenth, again named, linked and found the same way:
# tests/test_mesh_cutout_host.py keeps its census.
def cut_lib_of(lib):
    return os.path.splitext(os.path.abspath(lib))[0] + "_cut.so"


CUT_LIB = cut_lib_of(LIB)


# The kernels of mesh normal maps (k_nrm.hip: meshnrm_*) are an eleventh, again named, linked and found the same way:
# tests/test_mesh_normal_map_host.py keeps its census.
def nrm_lib_of(lib):
    return os.path.splitext(os.path.abspath(lib))[0] + "_nrm.so"


NRM_LIB = nrm_lib_of(LIB)


# The kernels of mesh material maps (k_mmap.hip: meshmap_*) are a twelfth, again named, linked and found the same way:
# tests/test_mesh_material_map_host.py keeps its census.
def mmap_lib_of(lib):
    return os.path.splitext(os.path.abspath(lib))[0] + "_mmap.so"


MMAP_LIB = mmap_lib_of(LIB)


# The kernels of mesh emission maps (k_emap.hip: meshemit_*) are a thirteenth, again named, linked and found the same way:
# tests/test_mesh_emission_map_host.py keeps its census.
def emap_lib_of(lib):
    return os.path.splitext(os.path.abspath(lib))[0] + "_emap.so"


EMAP_LIB = emap_lib_of(LIB)


# The kernels of mesh media (k_med.hip: meshmed_*) are a fourteenth, again named, linked and found the same way:
# tests/test_mesh_media_host.py keeps its census.
def med_lib_of(lib):
    return os.path.splitext(os.path.abspath(lib))[0] + "_med.so"


MED_LIB = med_lib_of(LIB)


# The kernels of ray queries (k_query.hip: query_*) are a fifteenth, again named, linked and found the same way:
# tests/test_query_host.py keeps its census.
def query_lib_of(lib):
    return os.path.splitext(os.path.abspath(lib))[0] + "_query.so"


QUERY_LIB = query_lib_of(LIB)


# The kernels of radiance queries (k_rad.hip: radiance_*) are a sixteenth, again named, linked and found the same way:
# tests/test_radiance_f64.py keeps its census.
def rad_lib_of(lib):
    return os.path.splitext(os.path.abspath(lib))[0] + "_rad.so"


RAD_LIB = rad_lib_of(LIB)


# The kernels of the guided denoiser (k_gdn.hip: gdn_*) are a seventeenth, again named and linked the same way and found through the
# run path: tests/test_denoise_guided.py keeps its census.  It lies one directory down, in gdn/ ($ORIGIN/gdn is on the run path of the
# libraries that load it): tests/test_radiance_f64.py holds the package directory itself to the seventeen libraries it counts.
def gdn_lib_of(lib):
    d, base = os.path.split(os.path.abspath(lib))
    return os.path.join(d, "gdn", os.path.splitext(base)[0] + "_gdn.so")


GDN_LIB = gdn_lib_of(LIB)


# The kernels of temporal accumulation (k_tacc.hip: tacc_*) are an eighteenth, named, linked and found like the guided denoiser's and
# for the same reason one directory down, in tacc/ ($ORIGIN/tacc is on the run path of the libraries that load it):
# tests/test_temporal.py keeps its census.
def tacc_lib_of(lib):
    d, base = os.path.split(os.path.abspath(lib))
    return os.path.join(d, "tacc", os.path.splitext(base)[0] + "_tacc.so")


TACC_LIB = tacc_lib_of(LIB)

# One translation unit per kernel class (csrc/kernel_common.h says what each build of them is):
#   strict    k_small tracks the range tests of the short divide / sqrt; k_compact, k_sdf, k_large, k_mesh test next to every operation
#   relaxed   the four render TUs once more with hipcc's fast divide / sqrt and FMA contraction: what RPT_RENDER_FAST_MATH selects
PEROP = ["-DRPT_GUARD_PER_OP"]
RELAXED = ["-DRPT_RELAXED_BUILD", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-ffp-contract=fast"]
# (object, source, extra flags, which library: "both" | "product" | "test")
OBJECTS = [
    ("k_small", "k_small.hip", [], "both"),
    ("k_compact", "k_compact.hip", PEROP, "both"),
    ("k_sdf", "k_sdf.hip", PEROP, "both"),
    ("k_large", "k_large.hip", PEROP, "both"),
    ("k_mesh", "k_mesh.hip", PEROP, "mesh"),                       # mesh scenes: strict only (include/rpt.h, "triangle meshes"); MESH_LIB
    ("k_refit", "k_refit.hip", [], "refit"),                       # rpt_update_meshes' refit of a mesh scene's tables; REFIT_LIB
    ("k_build", "k_build.hip", [], "bvhbuild"),                    # rpt_rebuild_meshes' new slot order and shape; BUILD_LIB
    ("k_move", "k_move.hip", [], "move"),                          # the device-source calls' check and apply of new positions; MOVE_LIB
    ("k_smooth", "k_smooth.hip", PEROP, "smooth"),                 # smooth mesh shading: the normals' two passes and the mesh kernel's smooth form; SMOOTH_LIB
    ("k_light", "k_light.hip", PEROP, "light"),                    # mesh lights: the ON meshes' tables and the mesh kernel's form that samples them; LIGHT_LIB
    ("k_tex", "k_tex.hip", PEROP, "tex"),                          # mesh textures: the decode and the mesh kernel's two textured forms; TEX_LIB
    ("k_env", "k_env.hip", PEROP, "env"),                          # environment lighting: the table kernels and the mesh kernel's one form under a sky; ENV_LIB
    ("k_cut", "k_cut.hip", PEROP, "cut"),                          # mesh cutouts: the mask kernel and the mesh kernel's two forms whose walks test the mask; CUT_LIB
    ("k_nrm", "k_nrm.hip", PEROP, "nrm"),                          # mesh normal maps: the decode and the mesh kernel's four forms whose hit normal is bent; NRM_LIB
    # mesh material maps: the decode and the mesh kernel's eight forms whose roughness and metallic are scaled; MMAP_LIB.  One file,
    # two translation units (the forms over the normal-mapped forms are the second): the build's longest step is halved
    ("k_mmap", "k_mmap.hip", PEROP + ["-DRPT_MMAP_PART=0"], "mmap"),
    ("k_mmap_nrm", "k_mmap.hip", PEROP + ["-DRPT_MMAP_PART=1"], "mmap"),
    # mesh emission maps: the mesh kernel's eight forms whose emission is looked up at the hit, at the emitter exit and in the
    # mesh-light sampler, and their two probes; EMAP_LIB.  One file, two translation units, as k_mmap.hip
    ("k_emap", "k_emap.hip", PEROP + ["-DRPT_EMAP_PART=0"], "emap"),
    ("k_emap_nrm", "k_emap.hip", PEROP + ["-DRPT_EMAP_PART=1"], "emap"),
    # mesh media: the mesh kernel's eight forms whose paths carry the medium they are in, and their probe; MED_LIB.  One file, two
    # translation units, as k_emap.hip
    ("k_med", "k_med.hip", PEROP + ["-DRPT_MED_PART=0"], "med"),
    ("k_med_nrm", "k_med.hip", PEROP + ["-DRPT_MED_PART=1"], "med"),
    ("k_query", "k_query.hip", PEROP, "query"),                    # ray queries: closest, occluded, surfaces and the camera's rays; QUERY_LIB
    # radiance queries: the integrator over rays the caller brings, eight forms, and the camera's sample rays; RAD_LIB.  One file, two
    # translation units, as k_med.hip
    ("k_rad", "k_rad.hip", PEROP + ["-DRPT_RAD_PART=0"], "rad"),
    ("k_rad_nrm", "k_rad.hip", PEROP + ["-DRPT_RAD_PART=1"], "rad"),
    ("k_small_fast", "k_small.hip", RELAXED, "both"),
    ("k_compact_fast", "k_compact.hip", RELAXED, "both"),
    ("k_sdf_fast", "k_sdf.hip", RELAXED, "both"),
    ("k_large_fast", "k_large.hip", RELAXED, "both"),
    ("k_util", "k_util.hip", [], "both"),
    # the denoiser's taps are independent multiply / add sequences: packed f32 instructions halve their issue slots there
    # (the path kernels lose from SLP: it pins register pairs).  PEROP: its divides test their operands next to the operation —
    # the default form only records them for a render kernel's per-sample recomputation, which the denoiser does not have
    ("denoise", "denoise.hip", ["-fslp-vectorize"] + PEROP, "both"),
    # the guided denoiser: the pack kernel and the filter's fused and step kernels; GDN_LIB.  Built like denoise.hip
    ("k_gdn", "k_gdn.hip", ["-fslp-vectorize"] + PEROP, "gdn"),
    # temporal accumulation: one kernel in three forms (first frame, identity, reprojecting); TACC_LIB.  Built like denoise.hip
    ("k_tacc", "k_tacc.hip", ["-fslp-vectorize"] + PEROP, "tacc"),
    ("capi", "capi.hip", [], "product"),
    ("capi_test", "capi.hip", ["-DRPT_TEST_HOOKS"], "test"),
    ("k_probes", "k_probes.hip", [], "test"),
    ("k_probes_fast", "k_probes.hip", RELAXED, "test"),            # the math probes of the relaxed build (include/rpt_test.h, RPT_PROBE_RELAXED)
]
# -ffp-contract=off: results are compared bit for bit with a CPU restatement, the only
# fused operations are the explicit fma calls of rpt_strict_math.h.
# -mllvm -disable-machine-licm: MachineLICM hoists the materialisation of ~70 literal constants (the
#   f64 polynomial coefficients of rpt_strict_math.h, two VGPRs each) out of the sample loop, where
#   they stay live for the whole kernel: 183 VGPRs (2 waves/SIMD) with it, 115 without.
# -fno-slp-vectorize: SLP packs scalar f32 ops into v_pk_mul/add_f32, which issue at half rate on
#   gfx950 and need paired registers: 115 -> 95 VGPRs and +6 % throughput without it.
# -mllvm -amdgpu-sched-strategy=max-ilp: the machine scheduler interleaves independent chains (the three divides of a
#   normalize, the three pow of the background) instead of minimising register pressure first: +2 % on configs[1]
#   and [3] at the same 96 VGPRs (iterative-ilp / iterative-minreg: no gain).
# -fvisibility=hidden: the library exports what include/rpt.h declares (capi.hip pushes default visibility around it) and nothing else.
BASE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-fvisibility=hidden"]
# The two -mllvm options are tuning only (they change instruction order / register use, never a result); a toolchain that
# does not know them still builds the library without them (probed once, on an empty translation unit).
TUNING_FLAGS = ["-mllvm", "-disable-machine-licm", "-mllvm", "-amdgpu-sched-strategy=max-ilp"]

_tuning_ok = None


def _hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _tuning_flags():
    """TUNING_FLAGS if this hipcc accepts them, else []."""
    global _tuning_ok
    if _tuning_ok is None:
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, "empty.hip")
            open(src, "w").write("#include <hip/hip_runtime.h>\n__global__ void k() {}\n")
            r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3"] + TUNING_FLAGS + ["-c", src, "-o", os.path.join(d, "empty.o")],
                               capture_output=True)
            _tuning_ok = r.returncode == 0
            if not _tuning_ok:
                print("build.py: this hipcc rejects the -mllvm tuning options; building without them")
    if os.environ.get("RPT_TUNING_FLAGS") is not None:               # experiments (tools/build_variants.py): replace the tuning options
        return os.environ["RPT_TUNING_FLAGS"].split()
    return TUNING_FLAGS if _tuning_ok else []


def _deps():
    """Every file a change of which means a rebuild: all sources and headers under csrc/ and include/."""
    inc = os.path.join(HERE, "..", "include")
    return (glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(inc, "*.h")) +
            [os.path.abspath(__file__)])


def needs_build(lib=LIB, mesh_lib=None, refit_lib=None, build_lib=None, move_lib=None, smooth_lib=None, light_lib=None, tex_lib=None, env_lib=None,
                cut_lib=None, nrm_lib=None, mmap_lib=None, emap_lib=None, med_lib=None, query_lib=None, rad_lib=None, gdn_lib=None, tacc_lib=None):
    """`mesh_lib`, `refit_lib`, `build_lib`, `move_lib`, `smooth_lib`, `light_lib`, `tex_lib`, `env_lib`, `cut_lib`, `nrm_lib`, `mmap_lib`, `emap_lib`, `med_lib`, `query_lib`, `rad_lib`, `gdn_lib`, `tacc_lib`: the
    code object libraries `lib` loads (default mesh_lib_of(lib), refit_lib_of(lib), build_lib_of(lib), move_lib_of(lib), smooth_lib_of(lib), light_lib_of(lib),
    tex_lib_of(lib), env_lib_of(lib), cut_lib_of(lib), nrm_lib_of(lib), mmap_lib_of(lib), emap_lib_of(lib), med_lib_of(lib), query_lib_of(lib), rad_lib_of(lib), gdn_lib_of(lib), tacc_lib_of(lib); the test build loads the product's)."""
    parts = [lib, mesh_lib or mesh_lib_of(lib), refit_lib or refit_lib_of(lib), build_lib or build_lib_of(lib), move_lib or move_lib_of(lib),
             smooth_lib or smooth_lib_of(lib), light_lib or light_lib_of(lib), tex_lib or tex_lib_of(lib), env_lib or env_lib_of(lib),
             cut_lib or cut_lib_of(lib), nrm_lib or nrm_lib_of(lib), mmap_lib or mmap_lib_of(lib), emap_lib or emap_lib_of(lib), med_lib or med_lib_of(lib), query_lib or query_lib_of(lib),
             rad_lib or rad_lib_of(lib), gdn_lib or gdn_lib_of(lib), tacc_lib or tacc_lib_of(lib)]
    if not all(os.path.exists(p) for p in parts):
        return True
    t = min(os.path.getmtime(p) for p in parts)
    return any(os.path.getmtime(d) > t for d in _deps())


def build(force=False, verbose=False, extra_flags=(), lib=LIB, objdir_name="build", test_lib=None, only=None, jobs=None):
    """Compile csrc/*.hip -> `lib` (and, when `test_lib` is given, the test build beside it).  hipcc cross-compiles gfx950 without a GPU.
    `extra_flags` / `lib` / `objdir_name`: experiment builds next to the product library (tools/); `only`: recompile just these
    objects (the others are taken from `objdir_name`/ as they are — or, if missing there, from the product's build/)."""
    if not force and not needs_build(lib) and (test_lib is None or not needs_build(test_lib, mesh_lib_of(lib), refit_lib_of(lib), build_lib_of(lib), move_lib_of(lib),
                                                                         smooth_lib_of(lib), light_lib_of(lib), tex_lib_of(lib), env_lib_of(lib), cut_lib_of(lib),
                                                                         nrm_lib_of(lib), mmap_lib_of(lib), emap_lib_of(lib), med_lib_of(lib), query_lib_of(lib), rad_lib_of(lib),
                                                                         gdn_lib_of(lib), tacc_lib_of(lib))):
        return lib
    objdir = os.path.join(HERE, objdir_name)
    os.makedirs(objdir, exist_ok=True)
    flags = BASE_FLAGS + _tuning_flags()
    jobs = jobs or max(1, min(8, os.cpu_count() or 1))
    pending, objs = [], {}
    for name, src, extra, where in OBJECTS:
        if where == "test" and test_lib is None:
            continue
        obj = os.path.join(objdir, name + ".o")
        objs[name] = (obj, where)
        if only is not None and name not in only:
            if not os.path.exists(obj):
                shutil.copy(os.path.join(HERE, "build", name + ".o"), obj)
            continue
        pending.append([_hipcc()] + flags + extra + list(extra_flags) + ["-c", os.path.join(CSRC, src), "-o", obj])
    running, failed = [], []
    while pending or running:
        while pending and len(running) < jobs:
            cmd = pending.pop(0)
            if verbose:
                print(" ".join(cmd))
            running.append((cmd, subprocess.Popen(cmd, cwd=CSRC)))
        cmd, p = running.pop(0)
        if p.wait() != 0:
            failed.append(" ".join(cmd))
    if failed:
        raise RuntimeError("build.py: compilation failed:\n" + "\n".join(failed))
    mesh_lib, refit_lib, build_lib, move_lib, smooth_lib = mesh_lib_of(lib), refit_lib_of(lib), build_lib_of(lib), move_lib_of(lib), smooth_lib_of(lib)
    light_lib, tex_lib, env_lib, cut_lib, nrm_lib = light_lib_of(lib), tex_lib_of(lib), env_lib_of(lib), cut_lib_of(lib), nrm_lib_of(lib)
    mmap_lib, emap_lib, med_lib, query_lib = mmap_lib_of(lib), emap_lib_of(lib), med_lib_of(lib), query_lib_of(lib)
    rad_lib, gdn_lib, tacc_lib = rad_lib_of(lib), gdn_lib_of(lib), tacc_lib_of(lib)
    os.makedirs(os.path.dirname(gdn_lib), exist_ok=True)
    os.makedirs(os.path.dirname(tacc_lib), exist_ok=True)
    for part, kind in ((mesh_lib, "mesh"), (refit_lib, "refit"), (build_lib, "bvhbuild"), (move_lib, "move"), (smooth_lib, "smooth"), (light_lib, "light"),
                       (tex_lib, "tex"), (env_lib, "env"), (cut_lib, "cut"), (nrm_lib, "nrm"), (mmap_lib, "mmap"), (emap_lib, "emap"), (med_lib, "med"), (query_lib, "query"),
                       (rad_lib, "rad"), (gdn_lib, "gdn"), (tacc_lib, "tacc")):
        link = [_hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared"] + [o for o, w in objs.values() if w == kind] + [
            "-Wl,-soname," + os.path.basename(part), "-o", part]
        if verbose:
            print(" ".join(link))
        subprocess.run(link, check=True, cwd=CSRC)
    for out, kinds in ((lib, ("both", "product")), (test_lib, ("both", "test"))):
        if out is None:
            continue
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        link = [_hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared"] + [o for o, w in objs.values() if w in kinds] + [
            mesh_lib, refit_lib, build_lib, move_lib, smooth_lib, light_lib, tex_lib, env_lib, cut_lib, nrm_lib, mmap_lib, emap_lib, med_lib, query_lib, rad_lib, gdn_lib,
            tacc_lib, "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,$ORIGIN/gdn", "-Wl,-rpath,$ORIGIN/tacc", "-ldl", "-o", out]
        if verbose:
            print(" ".join(link))
        subprocess.run(link, check=True, cwd=CSRC)
    return lib


if __name__ == "__main__":
    print(build(force=True, verbose=True, test_lib=TEST_LIB))
