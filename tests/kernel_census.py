"""Which render kernels there are, and which one ran: the kernels of a library's gfx950 code object, and the kernel a launch took
according to rpt_debug_kernel_choice (include/rpt_test.h).  Shared by the strict and the relaxed kernel matrices
(tests/test_gpu_strict_kernels.py, tests/test_gpu_relaxed.py) and, for mesh scenes, by the float64 comparisons
(tests/test_gpu_mesh_*_f64.py).  Reading the code object needs no GPU."""
import os
import re
import struct
import subprocess
import tempfile

# ---- which kernel ran (include/rpt_test.h, rpt_debug_kernel_choice) -------------------------------------------------------------------
RELAXED_BIT, COMPACT_BIT, DENSE_BIT, NESTED_BIT, MEDIA_BIT = 1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24


def kernel_of(choice, klass):
    """The kernel the launchers (k_small / k_compact / k_sdf / k_large.hip) take for rpt_debug_kernel_choice's bits, in the build the bits
    name (the relaxed one's kernels end in _fast, before a template argument); klass is "small", "sdf" or "large"."""
    fast = "_fast" if choice & RELAXED_BIT else ""
    sized, table, wide, mapped = choice & 1, choice & 2, choice & 4, choice & 8
    if choice & MEDIA_BIT:                                            # (one form per class; no relaxed one)
        if klass == "large":
            return "render_large_regen_media_kernel" + fast
        if klass == "sdf":
            return "render_sdf_march2_media_kernel" + fast
        return ("render_small_compact_media_kernel" if choice & COMPACT_BIT else "render_small_regen_media_kernel") + fast
    if klass == "large":
        return "render_large_regen_kernel" + fast
    if klass == "sdf":
        n = (choice >> 16) & 0xF
        if n:
            return "render_sdf_march2_sized%s_kernel%s<%d>" % ("_table" if table else "", fast, n)
        return ("render_sdf_march2_table_kernel" if table else "render_sdf_march2_kernel") + fast
    if choice & NESTED_BIT:
        return "render_small_nested_kernel" + fast
    if choice & COMPACT_BIT:
        dense = "dense_" if choice & DENSE_BIT else ""
        form = "sized_table_" if sized and table else "sized_" if sized else "table_" if table else ""
        return "render_small_compact_%s%skernel%s" % (dense, form, fast)
    if sized and table:
        return "render_small_regen_sized_table_kernel" + fast
    if sized:
        return "render_small_regen_sized_kernel" + fast
    if table or wide:
        return "render_small_regen_table_kernel" + fast
    if mapped:
        return "render_small_regen_maptable_kernel" + fast
    return "render_small_regen_kernel" + fast


MESH_BIT, SMOOTH_BIT, LIGHT_BIT, TEX_BIT, ENV_BIT, CUT_BIT, NRM_BIT = (1 << b for b in range(25, 32))
MESH_FORM_BITS = 0x7F << 25
# every name mesh_kernel_of can return, in the order of csrc/mesh_args.h's MeshForm (tests/test_mesh_args_host.py)
MESH_RENDER_KERNELS = ["meshnrm_cut_env_regen_kernel", "meshnrm_cut_regen_kernel", "meshnrm_env_regen_kernel", "meshnrm_regen_kernel",
                       "meshcut_env_regen_kernel", "meshcut_regen_kernel", "meshenv_regen_kernel", "meshtex_light_regen_kernel",
                       "meshtex_regen_kernel", "meshlight_regen_kernel", "meshsmooth_regen_kernel", "mesh_regen_kernel"]


def mesh_kernel_of(choice):
    """The kernel launch_render (csrc/capi.hip) takes for a mesh scene with rpt_debug_kernel_choice's bits 25-31 (MESH, SMOOTH, LIGHT,
    TEX, ENV, CUT, NRM), restating mesh_form_of (csrc/mesh_args.h): normal maps first, picked by (cutouts, environment), then cutouts,
    picked by the environment, then the environment's one form, then textures over the lights' tables or the smooth ones', lights,
    smooth, flat."""
    assert choice & MESH_BIT, "not a mesh scene's launch: 0x%x" % choice
    smooth, lights, textured = choice & SMOOTH_BIT, choice & LIGHT_BIT, choice & TEX_BIT
    environment, cutouts, normal_maps = choice & ENV_BIT, choice & CUT_BIT, choice & NRM_BIT
    if normal_maps and cutouts and environment:
        return "meshnrm_cut_env_regen_kernel"
    if normal_maps and cutouts:
        return "meshnrm_cut_regen_kernel"
    if normal_maps and environment:
        return "meshnrm_env_regen_kernel"
    if normal_maps:
        return "meshnrm_regen_kernel"
    if cutouts and environment:
        return "meshcut_env_regen_kernel"
    if cutouts:
        return "meshcut_regen_kernel"
    if environment:
        return "meshenv_regen_kernel"
    if textured and lights:
        return "meshtex_light_regen_kernel"
    if textured:
        return "meshtex_regen_kernel"
    if lights:
        return "meshlight_regen_kernel"
    if smooth:
        return "meshsmooth_regen_kernel"
    return "mesh_regen_kernel"


# ---- which kernels there are ------------------------------------------------------------------------------------------------------
def code_object_kernels(lib_path):
    """Kernel names (demangled to name or name<N>) of every gfx950 code object in `lib_path`'s .hip_fatbin section: one offload bundle
    per translation unit, each unbundled by its header; llvm-readelf --notes reads the kernels' metadata (tools/kernel_meta.py).
    (The code object's metadata, not the host symbol table: the library is built with -fvisibility=hidden.)"""
    data = open(lib_path, "rb").read()
    # the ELF section .hip_fatbin
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    sec = lambda i: struct.unpack_from("<IIQQQQ", data, shoff + i * shentsize)      # noqa: E731  (name, type, flags, addr, offset, size)
    strtab = sec(shstrndx)
    fat = None
    for i in range(shnum):
        name_off, _, _, _, off, size = sec(i)
        name = data[strtab[4] + name_off:data.index(b"\0", strtab[4] + name_off)]
        if name == b".hip_fatbin":
            fat = data[off:off + size]
    assert fat is not None, "no .hip_fatbin in %s" % lib_path
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    names = []
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf")
    with tempfile.TemporaryDirectory() as d:
        for start in [m.start() for m in re.finditer(re.escape(magic), fat)]:
            n_entries, = struct.unpack_from("<Q", fat, start + len(magic))
            p = start + len(magic) + 8
            for _ in range(n_entries):
                off, size, tlen = struct.unpack_from("<QQQ", fat, p)
                triple = fat[p + 24:p + 24 + tlen].decode()
                p += 24 + tlen
                if triple.endswith("gfx950") and size:
                    co = os.path.join(d, "co")
                    open(co, "wb").write(fat[start + off:start + off + size])
                    txt = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
                    names += re.findall(r"^\s+\.name:\s+(\S+)\s*$", txt, re.M)
    return [_demangle(n) for n in names]


def _demangle(n):
    """name or name<N[,true|false]> of a kernel's mangled name: _Z<len><name>, or _ZN<len><scope>...<len><name>E (an anonymous
    namespace, for one), then integral and bool template arguments."""
    m = re.match(r"_ZN?", n)
    if not m:
        return n
    p, base = m.end(), None
    while True:
        d = re.match(r"\d+", n[p:])
        if not d:
            break
        base = n[p + d.end():p + d.end() + int(d.group())]
        p += d.end() + int(d.group())
        if not n.startswith("_ZN"):
            break
    if base is None:
        return n
    t = re.match(r"I((?:L[ijb]\d+E)+)E", n[p:])
    if not t:
        return base
    args = re.findall(r"L([ijb])(\d+)E", t.group(1))
    return base + "<%s>" % ",".join(("true" if v == "1" else "false") if c == "b" else v for c, v in args)


def render_kernels(lib_path, relaxed):
    """The render_* kernels of the library's code object: the relaxed build's (_fast) or the strict build's."""
    return set(k for k in code_object_kernels(lib_path) if k.startswith("render_") and ("_fast" in k) == relaxed)
