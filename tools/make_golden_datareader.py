#!/usr/bin/env python3
"""Generate tests/golden/datareader.npz by running the REFERENCE's own Data_Reader (datareader.py) -- build container only.

The reference is imported unmodified from its checkout (never copied) behind the cv2 / matplotlib stand-ins of
tools/make_golden.py; its Homography / Homography_Wrapper get their ``correspondence`` filled by hand with the fixture
matrices, as gen_homography does.  For every case of tests/datareader_cases.py:GOLDEN_CASES the reference loads the input
file, resamples it (``reinterpolate(frequency, save=None)``) and writes it (``write_to_file``).  The file holds the input CSV
bytes, the matrices, the reference's output CSV bytes and a dump of its ``data`` (instant, id, timestamp, six fp64 fields).
This script refuses to run without the reference and is never executed on the GPU box.

    python tools/make_golden_datareader.py [--out DIR]
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import make_golden as mg                    # noqa: E402  (REF, the stand-ins; puts the package and tests/ on sys.path)
import datareader_cases as dc               # noqa: E402  (tests/datareader_cases.py)


def import_reference():
    if not os.path.isfile(os.path.join(mg.REF, "datareader.py")):
        raise SystemExit("the reference checkout (%s) is needed to write this fixture" % mg.REF)
    import types
    sys.modules["cv2"] = types.ModuleType("cv2")
    mg.matplotlib_stub()
    for k in ("homography", "datareader", "timestamp_utilities"):
        sys.modules.pop(k, None)
    sys.path.insert(0, mg.REF)
    try:
        import datareader as ref
        import homography as hgmod
    finally:
        sys.path.remove(mg.REF)
    for m in (ref, hgmod):
        assert os.path.realpath(m.__file__).startswith(os.path.realpath(mg.REF) + os.sep), m.__file__
    for k in ("homography", "datareader", "timestamp_utilities"):
        sys.modules.pop(k, None)            # later imports of these names are not to find the reference's
    return ref, hgmod


def inputs():
    with open(os.path.join(mg.REF, "working_3D_tracking_data.csv"), newline="") as f:
        working = f.read()
    return {"irregular": dc.tracking_csv(seed=11, n_frames=20, n_objs=6, edges=True),
            "metres": dc.tracking_csv(seed=12, n_frames=12, n_objs=5, scale=3.281),
            "working": working}


def main(out_dir):
    ref, hgmod = import_reference()
    names, P, P2 = dc.cameras()

    def make_hg(M):
        hg = hgmod.Homography()
        hg.correspondence = {n: {"P": M[i]} for i, n in enumerate(names[:len(M)])}
        hg.default_correspondence = names[0]
        return hg
    texts = inputs()
    out = {"names": np.array(names), "P": P, "P2": P2}
    # the shipped file names its own six cameras: each gets the fixture matrix that sees its rows best
    _, loaded = dc.load(texts["working"])
    items, st, _ = dc.states(loaded)
    order = []
    for n in names[:6]:
        rows = st[[o["camera"] == n for o in items]]
        order.append(int(np.argmax([dc.divisors(rows, [names[c]] * len(rows), names, P).min() for c in range(len(names))])))
    out["working_P"] = P[order]
    for key, text in texts.items():
        out["in_" + key] = np.frombuffer(text.encode(), np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        for case, (key, kw, freq, wrapper) in dc.GOLDEN_CASES.items():
            src, dst = os.path.join(tmp, key + ".csv"), os.path.join(tmp, case + "_out.csv")
            with open(src, "w", newline="") as f:
                f.write(texts[key])
            P = out["working_P"] if case == "working" else out["P"]
            hg = hgmod.Homography_Wrapper(hg1=make_hg(P), hg2=make_hg(P2)) if wrapper else make_hg(P)
            with contextlib.redirect_stdout(io.StringIO()):
                dr = ref.Data_Reader(src, hg, **kw)
                if freq is not None:
                    dr.reinterpolate(frequency=freq, save=None)
                dump = dc.dump(dr.data)
                dr.write_to_file(save_file=dst)
            with open(dst, newline="") as f:
                written = f.read()
            items, st, keep = dc.states(dr.data)
            w = dc.divisors(st[keep], [o["camera"] for o, k in zip(items, keep) if k], names, P, P2 if wrapper else None)
            assert w.min() > dc.MIN_DIVISOR, (case, float(w.min()))
            rows = len(dc.parse(written)) - 1
            assert 0 < rows <= 600, (case, rows)
            print("%-8s %4d data, %4d rows written, smallest divisor %.3f" % (case, len(dump), rows, w.min()))
            out[case + "_out"] = np.frombuffer(written.encode(), np.uint8)
            out[case + "_dump"] = dump
    np.savez_compressed(os.path.join(out_dir, "datareader.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else mg.OUT)
