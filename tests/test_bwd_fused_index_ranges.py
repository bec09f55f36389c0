"""CPU: the LDS index arithmetic of the fused 1x1 backward kernel (3d-playground_amd/csrc/conv_bwd_1x1_geom.h, the header the kernel
itself compiles) enumerated on the host: the stores of a K-step tile their plane images exactly once, every read stays inside its
image and finds the element the MFMA operand layout wants, and no lane group the LDS serves together meets a bank twice."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bwd_fused_lds_indices():
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "bwd_fused_index_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(REPO, "3d-playground_amd", "csrc"),
                               os.path.join(REPO, "tests", "bwd_fused_index_check.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.startswith("ok "), r.stdout
