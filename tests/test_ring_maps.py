"""The index maps of k_conv6r's ring exchange (csrc/conv6r_ring.h), checked on the CPU: a small host program (tests/ring_maps_check.cpp) built from
the header the kernel includes walks every tile of a tiling as the kernel's threads do."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("ring") / "ring_maps_check")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc"), os.path.join(ROOT, "tests", "ring_maps_check.cpp"), "-o", exe]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("tiles", [(1, 1), (2, 2), (3, 3), (4, 6)])
def test_ring_index_maps(checker, tiles):
    """Every ring entry of every chunk of every tile is written by exactly one fetched triple, from the matching interior entry of the right
    neighbour; border tiles fetch nothing across the image edge; every publish slot has exactly one writer; padding is never stored."""
    r = subprocess.run([checker, str(tiles[0]), str(tiles[1])], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok")
