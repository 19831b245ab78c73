"""pack_layout (csrc/rtx_scene.hip): the storage order of a walk on the device, checked without a GPU.

tests/pack_layout_check.cpp builds three scenes, packs them and checks the order itself (a permutation that ends in
the sentinel; start and every stored next walk the input's pre-order; escapes recoded; primitives first by rank for a
scene in the LDS copy; the chosen entries first for a big one; the quad table after the halves).  It is built here with
the host compiler from the host-only unit rtx_scene.hip alone, as plain C++: no HIP, no Python extension, nothing
preloaded.  (The link keeps only what main reaches, so the planner's glue in that unit, which calls rtx_topology.hip
and rtx_collapse.hip, is dropped and those units are not needed.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer-go_amd", "csrc")
SCENES = ["spheres and a quad", "a sphere referenced twice", "1025 spheres, by reads", "1025 spheres, top levels"]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pack_layout") / "pack_layout_check")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-ffunction-sections", "-Wl,--gc-sections", "-o", exe,
           os.path.join(ROOT, "tests", "pack_layout_check.cpp"), "-x", "c++", os.path.join(CSRC, "rtx_scene.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_pack_layout_orders(checker):
    r = subprocess.run([checker], capture_output=True, text=True, env={})
    assert r.returncode == 0, r.stdout + r.stderr
    for name in SCENES:
        assert f"{name}: ok" in r.stdout, r.stdout
