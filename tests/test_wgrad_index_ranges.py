"""CPU: the LDS index arithmetic of the weight-gradient kernels (3d-playground_amd/csrc/conv_wgrad_geom.h, the header the
kernels themselves compile) is enumerated on the host for every tile instance the launchers use -- pixel-table reads,
direct-to-LDS fill blocks, fragment reads, the bf16 kernel's transposing reads -- and every index must stay inside the
structure it addresses (DESIGN.md "Rules": the grouped-wgrad experiment of round 1 faulted the GPU exactly there).  The same
program enumerates the pieces the three kernels share: workgroup id -> (K slice, tile), the slices' pixel ranges, the pixel-table
entries and the tap decode."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wgrad_index") / "wgrad_index_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(REPO, "3d-playground_amd", "csrc"),
                           os.path.join(REPO, "tests", "wgrad_index_check.cpp"), "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_wgrad_lds_indices_stay_in_range(check_run):
    r = check_run
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.count("ok ") == 8, r.stdout


def test_wgrad_shared_pieces(check_run):
    """Placement under both id types, the K slices and pixel tables of both element sizes, taps and packed words."""
    r = check_run
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.count("shared pass ") == 5, r.stdout
