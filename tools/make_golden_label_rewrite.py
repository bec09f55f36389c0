#!/usr/bin/env python3
"""Generate tests/golden/label_rewrite.npz by running the REFERENCE's own annotator methods (seems_to_be_working.py) -- build
container only.

The reference module is loaded unmodified from its checkout (never copied) under a private name, behind the stand-ins of
tools/make_golden.py, as tools/make_golden_labels.py does.  For every scene of tests/label_rewrite_cases.py:golden_scenes() its
methods replace_homgraphy (scenes whose every datum has a "gen"), replace_y (both values of reverse), offset_box_y,
replace_timestamps and interpolate run UNBOUND on a stand-in ``self``; plot_all_trajectories is stubbed to nothing.  The
homographies are the REFERENCE's Homography / Homography_Wrapper objects filled from the scene's matrices; replace_homgraphy
unpickles its replacement from the working directory, so the scene's ``hg_new`` is pickled into a temporary one.
replace_homgraphy keeps its errors and indices to itself: a line tracer reads the locals ``error`` and ``min_idx`` once per
round (it depends on these two names, :1701-1704).

Fixture condition, enforced here: in every round of every box the smallest and the second smallest of the reference's own
errors are apart by (e2 - e1) >= 1e-6 * e2.  The matrix product of torch.matmul and the kernel's agree to a few fp64 ulps on a
pixel coordinate, so a gap of 1e-6 cannot flip and the winning indices are comparable exactly.

The file holds arrays only, outputs only; the inputs are scripted in tests/label_rewrite_cases.py.  This script refuses to run
without the reference and is never executed on the GPU box.

    python tools/make_golden_label_rewrite.py [--out DIR]
"""
import contextlib
import copy
import io
import os
import pickle
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import make_golden as mg                    # noqa: E402  (REF, the stand-ins; puts the package and tests/ on sys.path)
import label_rewrite_cases as rc            # noqa: E402  (tests/label_rewrite_cases.py)

METHODS = ("safe", "get_unused_id", "interpolate", "replace_homgraphy", "replace_y", "offset_box_y", "replace_timestamps")
MIN_GAP = 1e-6
SHADOWED = ("homography", "datareader", "timestamp_utilities")


def _forget():
    found = {}
    for k in [k for k in sys.modules if k in SHADOWED or k == "retinanet" or k.startswith("retinanet.")]:
        found[k] = sys.modules.pop(k)
    return found


def import_reference():
    """-> (the annotator module, the reference's homography module)."""
    if not os.path.isfile(os.path.join(mg.REF, "seems_to_be_working.py")):
        raise SystemExit("the reference checkout (%s) is needed to write this fixture" % mg.REF)
    mg.install_shims()
    mg.tracker_import_shims()
    _forget()
    sys.path.insert(0, mg.REF)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            ref = mg.ref_module_from_file("_reference_annotator", "seems_to_be_working.py")
    finally:
        sys.path.remove(mg.REF)
    hgmod = _forget()["homography"]         # later imports of these names are not to find the reference's
    assert os.path.realpath(hgmod.__file__).startswith(os.path.realpath(mg.REF) + os.sep)
    return ref, hgmod


@contextlib.contextmanager
def reference_homography_importable(hgmod):
    """pickle names a class by its module: while the reference's objects are pickled and unpickled, ``homography`` is its."""
    mine = sys.modules.get("homography")
    sys.modules["homography"] = hgmod
    try:
        yield
    finally:
        del sys.modules["homography"]
        if mine is not None:
            sys.modules["homography"] = mine


def stand_in(ref, hgmod, scene):
    """rc.Labels with the reference's methods as its own and the reference's homography objects as ``hg``."""
    members = {name: getattr(ref.Annotator, name) for name in METHODS}
    members["plot_all_trajectories"] = lambda self: None
    cls = type("StandIn", (rc.Labels,), members)
    return cls(scene, hgmod.Homography, hgmod.Homography_Wrapper)


@contextlib.contextmanager
def setitem_casts():
    """One more stand-in, for the torch the reference was written against: its i24_state_to_space assigns the float64 sums of
    replace_homgraphy's candidates into a float32 ``torch.zeros`` through an index list (homography.py:307-318).  That torch
    converted the source to the destination's dtype on the way in; today's ``index_put_`` raises "requires the source and
    destination dtypes match" instead, so the method cannot run at all.  While the reference runs, ``Tensor.__setitem__``
    converts a tensor source first -- one rounding to float32, which is what the kernel's mixed corner rule restates."""
    import torch
    plain = torch.Tensor.__setitem__

    def setitem(self, index, value):
        if isinstance(value, torch.Tensor) and value.dtype != self.dtype:
            value = value.to(self.dtype)
        return plain(self, index, value)
    torch.Tensor.__setitem__ = setitem
    try:
        yield
    finally:
        torch.Tensor.__setitem__ = plain


def traced_rounds(me):
    """Runs me.replace_homgraphy() under a line tracer -> [(errors of the round's candidates, winning index)] per round."""
    code = type(me).replace_homgraphy.__code__
    got, last = [], [None]

    def local(frame, event, arg):
        m = frame.f_locals.get("min_idx")
        if m is not None and m is not last[0]:                  # a new argmin: ``error`` is still the round's own
            last[0] = m
            got.append((frame.f_locals["error"].numpy().copy(), int(m)))
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code is code else None
    sys.settrace(tracer)
    try:
        with setitem_casts():
            me.replace_homgraphy()
    finally:
        sys.settrace(None)
    return got


def run_rebase(ref, hgmod, scene, out):
    names = scene["names"]
    me = stand_in(ref, hgmod, scene)
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp, reference_homography_importable(hgmod):
        new = rc.build_hg(scene["hg_new"], hgmod.Homography, hgmod.Homography_Wrapper)
        for side, hg in (("EB", new.hg1), ("WB", new.hg2)):
            with open(os.path.join(tmp, "{}_homography5.cpkl".format(side)), "wb") as f:
                pickle.dump(hg, f)
        os.chdir(tmp)
        try:
            rounds = traced_rounds(me)
        finally:
            os.chdir(here)
    per_box = len(rc.radii())
    assert len(rounds) % per_box == 0 and len(rounds) > 0
    worst = np.inf
    for e, i in rounds:
        e1, e2 = np.sort(e)[:2]
        assert int(np.argmin(e)) == i
        worst = min(worst, (e2 - e1) / e2)
        if not (e2 - e1) >= MIN_GAP * e2:
            raise SystemExit("fixture condition: a round's two smallest errors are %r and %r" % (e1, e2))
    win = np.array([i for _, i in rounds], np.int64).reshape(-1, per_box)
    boxes = [o for f, key, o in rc.visit(rc.Labels(scene), scene["last_frame"] + 1) if o["gen"] == "Manual"]
    assert len(boxes) == len(win)
    out["rebase_win"] = win
    out["rebase_err"] = np.array([e[i] for e, i in rounds[per_box - 1::per_box]], np.float64)
    kept = [me.data[f][key] for f, key, o in rc.visit(rc.Labels(scene), scene["last_frame"] + 1) if o["gen"] == "Manual"]
    assert all(type(b["x"]) is float and type(b["y"]) is float for b in kept)
    out["rebase_xy"] = np.array([[b["x"], b["y"]] for b in kept], np.float64).reshape(-1, 2)
    rc.dumped(out, "hg", me, names)
    return worst


def run_scene(ref, hgmod, name, scene):
    out, names, worst = {}, scene["names"], None
    if rc.all_have_gen(scene):
        worst = run_rebase(ref, hgmod, scene, out)
    for tag, reverse in (("y0", False), ("y1", True)):
        me = stand_in(ref, hgmod, scene)
        me.replace_y(reverse=reverse)
        rc.dumped(out, tag, me, names)
    me = stand_in(ref, hgmod, scene)
    boxes = [me.offset_box_y(copy.deepcopy(o), reverse=rev) for rev in (False, True) for _, _, o in rc.visit(me, len(me.data))]
    out["box_y"] = np.array([b["y"] for b in boxes], np.float64).reshape(-1)
    me = stand_in(ref, hgmod, scene)
    me.replace_timestamps()
    rc.dumped(out, "ts", me, names)
    out["ts_table"] = rc.lc.ts_table(me.all_ts, names)
    return {name + "_" + k: v for k, v in out.items()}, worst


def main(out_dir):
    ref, hgmod = import_reference()
    out = {}
    for name, scene in rc.golden_scenes().items():
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            got, worst = run_scene(ref, hgmod, name, scene)
        out.update(got)
        print("%-7s %d arrays, %d re-based boxes (smallest relative gap %s), %d boxes after replace_y, %d printed lines"
              % (name, len(got), len(got.get(name + "_rebase_win", ())), "-" if worst is None else "%.3g" % worst,
                 len(got[name + "_y0_idx"]), log.getvalue().count("\n")))
    save_npz(os.path.join(out_dir, "label_rewrite.npz"), out)


def save_npz(path, arrays):
    """np.savez_compressed with a fixed date on every member: the same arrays give the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, value in arrays.items():
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else mg.OUT)
