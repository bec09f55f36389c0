"""The committed golden vectors are what the REFERENCE produces today: tools/make_golden.py (which imports /root/reference
behind the three harness shims of SURVEY.md 8c) is run into a scratch directory and every array is compared with the
committed tests/golden/ set.

CPU only, build container only: skipped where /root/reference does not exist (the GPU box).  Integer arrays, strings
(sha256 digests), the CSV row fixtures and every float array except the whole-model gradient summaries must regenerate
bit for bit; the float outputs of whole-model backward passes (``*_gsum_*``: sum / abs-sum / norm of a parameter gradient,
``*_g_*``: the gradient itself, ``*_losses``) may move by the CPU thread order of torch's backward reductions -- measured
1e-8 relative on one entry of 637 -- and are held to 1e-6 of the array's largest magnitude.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
REF = "/root/reference"

pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference checkout only exists in the build container")

FLOAT_TOL = 1e-6            # relative to the array's largest magnitude; only for whole-model backward outputs (see above)


def _thread_order_dependent(fname, key):
    return fname in ("model.npz", "model_deep.npz", "model_deep101.npz") and ("_gsum_" in key or "_g_" in key or key.endswith("_losses"))


@pytest.fixture(scope="module")
def regenerated(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("golden_regen"))
    env = dict(os.environ, OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "8"))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "make_golden.py"), "--out", out], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return out


@pytest.mark.timeout(1200)
def test_every_committed_fixture_regenerates(regenerated):
    committed = sorted(f for f in os.listdir(GOLDEN) if f.endswith((".npz", ".csv")))
    fresh = sorted(f for f in os.listdir(regenerated) if f.endswith((".npz", ".csv")))
    assert committed == fresh, (committed, fresh)
    moved = []
    for fname in committed:
        a_path, b_path = os.path.join(GOLDEN, fname), os.path.join(regenerated, fname)
        if fname.endswith(".csv"):
            assert open(a_path, "rb").read() == open(b_path, "rb").read(), fname
            continue
        a, b = np.load(a_path), np.load(b_path)                       # allow_pickle=False (the default): data only
        assert sorted(a.files) == sorted(b.files), fname
        for key in a.files:
            x, y = a[key], b[key]
            assert x.shape == y.shape and x.dtype == y.dtype, (fname, key)
            if np.array_equal(x, y, equal_nan=x.dtype.kind == "f"):
                continue
            assert x.dtype.kind == "f" and _thread_order_dependent(fname, key), "%s:%s is not bit-identical" % (fname, key)
            err = np.abs(x.astype(np.float64) - y.astype(np.float64)).max() / (np.abs(x).max() + 1e-300)
            assert err <= FLOAT_TOL, "%s:%s moved by %.2e" % (fname, key, err)
            moved.append((fname, key, float(err)))
    print("arrays that are not bit-identical (thread order of the CPU backward):", moved)
