"""A mesh scene's kernel arguments on the host (csrc/mesh_args.h; CPU only): mesh_form_of picks, for every combination of
rpt_debug_kernel_choice's bits 26-31, the form whose kernel kernel_census.mesh_kernel_of names; and mesh_scene_of, for the form picked in
every reachable state, binds a present feature's pointers to its own allocation at its plan's own layout(), leaves null what the kernel
does not read, takes every empty table from a live allocation that carries one of the right kind and extent, derives nothing from a
null base, and counts the pickable lights as include/rpt.h does (tests/args_harness.cpp, a stand-alone program built under g++'s
address and undefined-behaviour sanitizers).  The tests state these properties; they do not restate which allocation lends which table."""
import json
import os
import subprocess

import pytest

from kernel_census import MESH_BIT, MESH_RENDER_KERNELS, mesh_kernel_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
N_TRIS, N_LIGHTS, NONE = 37, 3, 0xFFFFFFFF
ALLOCS = ("refit_a", "smooth_a", "light_a", "tex_a", "env_a", "cut_a", "nrm_a")
# field -> (the allocation, the offset of the plan's layout()) while its feature is present
PRESENT = {
    "smooth": {"vnormals": ("smooth_a", "off_normals"), "smooth_bits": ("smooth_a", "off_bits")},
    "lights": {"face_vertex": ("light_a", "off_face_vertex"), "light_desc": ("light_a", "off_desc"), "light_cdf": ("light_a", "off_cdf"),
               "tri_light": ("light_a", "off_tri_light")},
    "tex": {"tex_desc": ("tex_a", "off_desc"), "tri_tex": ("tex_a", "off_tri_tex"), "uvs": ("tex_a", "off_uvs"), "texels": ("tex_a", "off_texels")},
    "env": {"env_texels": ("env_a", "off_texels")},
    "cut": {"cut_desc": ("cut_a", "off_desc"), "cut_bits": ("cut_a", "off_bits")},
    "nrm": {"nrm_desc": ("nrm_a", "off_desc"), "nrm_texels": ("nrm_a", "off_texels")},
}
# ... and while it is absent: null where the binder's comment says "not read", else an empty table of this kind and at least these bytes
NOT_READ = {"smooth": ("vnormals",), "lights": ("face_vertex", "light_desc", "light_cdf"), "tex": ("tex_desc", "uvs", "texels")}
EMPTY = {"smooth": {"smooth_bits": ("zeros", 4 * ((N_TRIS + 31) // 32))}, "lights": {"tri_light": ("ones", 4 * N_TRIS)}, "tex": {"tri_tex": ("ones", 4 * N_TRIS)}}
REFIT = {"slot_vertex": "off_slot_vertex", "vertices": "off_vertices"}
POINTERS = sorted(set(REFIT) | {f for part in PRESENT.values() for f in part} | {"env_cdf"})


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("args") / "args_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROCM, "include"), os.path.join(ROOT, "tests", "args_harness.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def states(harness):
    r = subprocess.run([harness, "states"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    for s in out:
        s["empties"] = [e for e in s["empties"] if e]
    return out


def _label(s):
    return {k: s[k] for k in ("smooth", "lights", "tex", "env", "cut", "nrm", "form")}


def test_the_form_is_the_one_the_census_names(harness):
    """All 64 values of bits 26-31: MESH_RENDER_KERNELS[mesh_form_of(...)] is kernel_census.mesh_kernel_of's name for the same bits (the
    enum's order is that list's), and all twelve forms occur."""
    r = subprocess.run([harness, "forms"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert [b for b, _ in rows] == list(range(64))
    for bits, form in rows:
        assert MESH_RENDER_KERNELS[form] == mesh_kernel_of(MESH_BIT | bits << 26), (bits, form)
    assert sorted({form for _, form in rows}) == list(range(12)) == list(range(len(MESH_RENDER_KERNELS)))


def test_the_states_are_the_reachable_ones(states):
    """smooth, lights and textures free, the environment absent, BACKGROUND_ONLY or SAMPLED, cutouts and normal maps only with textures:
    2 x 2 x 3 x 5 = 60 states (40 by which features are present), and between them they take all twelve forms."""
    keys = {(s["smooth"], s["lights"], s["tex"], s["env"], s["cut"], s["nrm"]) for s in states}
    assert len(states) == len(keys) == 60 and len({k[:3] + (min(k[3], 1),) + k[4:] for k in keys}) == 40
    assert all(s["tex"] or not (s["cut"] or s["nrm"]) for s in states)
    assert sorted({s["form"] for s in states}) == list(range(12))
    for s in states:
        live = [a for a in ALLOCS if s[a]["base"]]
        assert live == ["refit_a"] + [a for a, k in zip(ALLOCS[1:], ("smooth", "lights", "tex", "env", "cut", "nrm")) if s[k]], _label(s)
        assert len({s[a]["base"] for a in live}) == len(live) and all(s[a]["base"] >= 1 << 40 and s[a]["total"] < 1 << 32 for a in live)


def test_a_present_features_pointers_are_its_own_tables(states):
    """base + the offset of the plan's own layout(), for every field of every part the form has; the refit's two tables always."""
    n = 0
    for s in states:
        arg = s["arg"]
        for field, off in REFIT.items():
            if field in arg:
                assert arg[field] == s["refit_a"]["base"] + s["refit_a"][off], (_label(s), field)
        for feature, part in PRESENT.items():
            for field, (alloc, off) in part.items():
                if s[feature] and field in arg:
                    assert s[alloc]["base"] and arg[field] == s[alloc]["base"] + s[alloc][off], (_label(s), field)
                    n += 1
        if "env_cdf" in arg:
            assert arg["env_cdf"] == (s["env_a"]["base"] + s["env_a"]["off_cdf"] if s["env"] == 2 else 0), _label(s)
        # the form picked never lacks the part of a present feature
        for feature, part in PRESENT.items():
            if s[feature]:
                assert all(f in arg for f in part), (_label(s), feature)
    assert n > 300


def test_an_absent_features_pointers_are_null_or_an_empty_table(states):
    """What the kernel does not read is null; what it reads is a table of zeros (smooth bits) or of 0xFFFFFFFF (tri_light, tri_tex) that
    a LIVE allocation carries, whole: at that allocation's offset for a table of that kind, long enough for the scene's triangles."""
    seen = set()
    for s in states:
        arg = s["arg"]
        for feature in NOT_READ:
            if s[feature]:
                continue
            for field in NOT_READ[feature]:
                if field in arg:
                    assert arg[field] == 0, (_label(s), field)
            for field, (kind, need) in EMPTY[feature].items():
                if field not in arg:
                    continue
                lenders = [(a, off, size) for k, a, off, size in s["empties"] if k == kind and s[a]["base"] and arg[field] == s[a]["base"] + off]
                assert len(lenders) == 1, (_label(s), field, arg[field], s["empties"])
                a, off, size = lenders[0]
                assert size >= need and off + size <= s[a]["total"], (_label(s), field, lenders)
                seen.add((field, a))
    # every kind of loan occurs: the states are not vacuous
    assert {f for f, _ in seen} == {"smooth_bits", "tri_light", "tri_tex"} and len(seen) >= 6, seen


def test_no_pointer_is_made_from_a_null_base(states):
    """Every pointer the binders set is null or lies inside a live allocation (absent allocations have base 0, live ones lie 2^40
    apart: base 0 plus an offset lies in none)."""
    for s in states:
        live = [(s[a]["base"], s[a]["total"]) for a in ALLOCS if s[a]["base"]]
        for field in POINTERS:
            p = s["arg"].get(field, 0)
            assert p == 0 or any(base <= p < base + total for base, total in live), (_label(s), field, p)


def test_the_pickable_lights_are_counted(states):
    """include/rpt.h, "pickable lights": N = the scene's lights + the ON meshes + a SAMPLED environment, N_f = (float)N, and the
    environment is the last of them or 0xFFFFFFFF."""
    for s in states:
        arg = s["arg"]
        sampled = 1 if s["env"] == 2 else 0
        assert arg["n_lights"] == N_LIGHTS and s["n_on"] == (1 if s["lights"] else 0)
        if "n_pick" in arg:
            assert arg["n_pick"] == N_LIGHTS + s["n_on"] + sampled, _label(s)
            assert arg["n_lights_f"] == float(arg["n_pick"]), _label(s)
            assert arg["n_faces"] == (17 if s["lights"] else 0), _label(s)
        else:
            assert not s["lights"] and not s["env"] and arg["n_lights_f"] == float(N_LIGHTS), _label(s)
        if "env_pick" in arg:
            assert arg["env_pick"] == (arg["n_pick"] - 1 if sampled else NONE), _label(s)
            assert arg["env_size"] == 4 and arg["env_scale"] == 1.5 and arg["env_q"] == (12345 if sampled else 0) == arg["env_q_f"], _label(s)
        else:
            assert not s["env"], _label(s)
