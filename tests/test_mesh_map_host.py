"""The image-map setters' shared host path (csrc/host_map.h; CPU only): the recipe of one device's part of rpt_set_mesh_cutouts,
rpt_set_mesh_normal_maps, rpt_set_mesh_material_maps and rpt_set_mesh_emission_maps, executed on host buffers with memset and memcpy
for the HIP calls and the headers' plain-loop references for the decode launches (tests/map_harness.cpp, a stand-alone program built
under g++'s address and undefined-behaviour sanitizers).  After every call of a sequence (set two meshes, replace one by another
size, set one OFF, name a third only, set all OFF) a feature's tables equal, byte for byte, those one call that names every ON mesh
builds from nothing; the stage's parts are multiples of 16 bytes, an image's bytes lie 1024 past its L table where the decode has
one, a kept mesh the device holds nothing for is an error and no step, and the emission tables' zero block is what it must be."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("map") / "map_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), os.path.join(ROOT, "tests", "map_harness.cpp"), "-o", exe], check=True)
    return exe


def _run(harness, *args):
    r = subprocess.run([harness] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr
    return r.stdout


@pytest.mark.parametrize("feature", ("cut", "nrm", "mmap", "emap"))
def test_a_sequence_of_calls_builds_the_tables_one_call_builds_from_nothing(harness, feature):
    out = _run(harness, feature)
    assert feature + " OK" in out
    sizes = [int(line.split()[2]) for line in out.splitlines() if line.startswith("call ")]
    assert len(sizes) == 5 and sizes[4] == 0 and all(s > 0 and s % 16 == 0 for s in sizes[:4])
    assert sizes[2] < sizes[0], "with mesh 0 OFF the tables hold one small image"


def test_the_recipes_own_rules(harness):
    assert "recipe OK" in _run(harness, "recipe")
