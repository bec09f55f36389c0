#!/usr/bin/env python3
"""Generate tests/golden/label_assist.npz by running the REFERENCE's own annotator methods (manual_annotator_state_v3.py) --
build container only.

The reference module is loaded unmodified from its checkout (never copied) under a private name, behind the stand-ins of
tools/make_golden.py, as tools/make_golden_label_rewrite.py does.  For every scene of tests/label_assist_cases.py:golden_scenes()
its methods box_to_state, find_box, copy_paste, paste_in_2D_bbox and automate run UNBOUND on a stand-in ``self`` built on
``label_assist_cases.Labels`` and replay the scene's script (``golden_script``).  crop_detect is replaced by the script's 2D
box (torchvision's roi_align, to_tensor and normalize are absent here: that half stays "parity unpinned", as crop_refine is);
plot and the cv2 calls are stubbed to nothing.  The homographies are the REFERENCE's Homography / Homography_Wrapper objects
filled from the scene's matrices.  paste_in_2D_bbox keeps its errors and indices to itself and automate its crop box: a line
tracer reads the locals ``error`` and ``min_idx`` once per round and ``crop_box`` (it depends on these three names, :627-630,
:669).

Fixture condition, enforced here.  The tool replays the same script with the numpy restatement of label_assist_cases.py and
compares the errors of EVERY candidate of every round of every search with the reference's traced ones.  Measured on this
container (numpy 2.2.6, torch 2.10): they are BIT-EQUAL on every candidate of every scene (20 searches, 7 260 candidates,
largest relative difference 0.0), so MIN_GAP = 16 x 0.0 = 0.0 and indices, errors and centres are compared exactly; the smallest
relative gap between a round's two smallest reference errors is 5.68e-3.  The tool measures both again on every run.  Were they not
bit-equal, MIN_GAP would be 16 times the largest relative difference (both of a round's two smallest errors may move towards
each other, with margin) and the tool refuses, with SystemExit, any round whose two smallest reference errors are closer than
that; it also refuses when the restatement's winner, centre or written datum differs from the reference's.  No case is skipped.

The file holds arrays only, outputs only; the inputs are scripted in tests/label_assist_cases.py.  This script refuses to run
without the reference and is never executed on the GPU box.

    python tools/make_golden_label_assist.py [--out DIR]
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import make_golden as mg                    # noqa: E402  (REF, the stand-ins; puts the package and tests/ on sys.path)
import make_golden_label_rewrite as mr      # noqa: E402  (_forget, save_npz)
import label_assist_cases as ac             # noqa: E402  (tests/label_assist_cases.py)

SOURCE = "manual_annotator_state_v3.py"
METHODS = ("safe", "box_to_state", "find_box", "copy_paste", "paste_in_2D_bbox", "automate")
GAP_FACTOR = 16


def import_reference():
    """-> (the annotator module, the reference's homography module)."""
    if not os.path.isfile(os.path.join(mg.REF, SOURCE)):
        raise SystemExit("the reference checkout (%s) is needed to write this fixture" % mg.REF)
    mg.install_shims()
    mg.tracker_import_shims()
    lines = types.ModuleType("matplotlib.collections")      # one more name the v3 annotator imports at the top and never
    lines.LineCollection = object                           # uses on this path
    sys.modules["matplotlib"].collections = sys.modules["matplotlib.collections"] = lines
    mr._forget()
    sys.path.insert(0, mg.REF)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            ref = mg.ref_module_from_file("_reference_annotator_v3", SOURCE)
    finally:
        sys.path.remove(mg.REF)
    hgmod = mr._forget()["homography"]      # later imports of these names are not to find the reference's
    assert os.path.realpath(hgmod.__file__).startswith(os.path.realpath(mg.REF) + os.sep)
    return ref, hgmod


class _Nothing():
    """cv2 of the reference module while automate runs: every call does nothing."""

    def __getattr__(self, name):
        return lambda *a, **k: None


def stand_in(ref, hgmod, scene):
    """ac.Labels with the reference's methods as its own, the reference's homography objects as ``hg``, and the scripted
    crop_detect: ``self.scripted(c_idx, crop) -> float32 [4]``."""
    import torch
    members = {name: getattr(ref.Annotator, name) for name in METHODS}
    members["plot"] = lambda self: None

    def crop_detect(self, frame, crop, ber=1.2, cs=112):
        assert crop.dtype == torch.float32 and tuple(crop.shape) == (4,)
        self.seen_box = torch.from_numpy(np.asarray(self.scripted(None, crop.numpy().copy()), np.float32).copy())
        return self.seen_box
    members["crop_detect"] = crop_detect
    cls = type("StandIn", (ac.Labels,), members)
    me = cls(scene, hgmod.Homography, hgmod.Homography_Wrapper)
    me.plot_frame = None
    return me


def reference_ops(ref, rounds_out):
    """The functions ``ac.replay`` calls, on the reference's methods under a line tracer."""
    paste_code, auto_code = ref.Annotator.paste_in_2D_bbox.__code__, ref.Annotator.automate.__code__

    def traced(call, me):
        got, last, crop = [], [None], [None]

        def local_paste(frame, event, arg):
            m = frame.f_locals.get("min_idx")
            if m is not None and m is not last[0]:              # a new argmin: ``error`` is still the round's own
                last[0] = m
                e = frame.f_locals["error"]
                assert str(e.dtype) == "torch.float32" and str(frame.f_locals["boxes_new"].dtype) == "torch.float32"
                got.append((e.numpy().copy(), int(m)))
            return local_paste

        def local_auto(frame, event, arg):
            c = frame.f_locals.get("crop_box")
            if c is not None:
                crop[0] = c
            return local_auto

        def tracer(frame, event, arg):
            return local_paste if frame.f_code is paste_code else (local_auto if frame.f_code is auto_code else None)
        sys.settrace(tracer)
        try:
            call()
        finally:
            sys.settrace(None)
        return got, crop[0]

    def paste2d(me, box):
        got, _ = traced(lambda: me.paste_in_2D_bbox(box), me)
        rounds_out.append(got)
        return got

    def automate(me, oid, detect):
        me.scripted, me.seen_box = detect, None
        cv2, ref.cv2 = getattr(ref, "cv2", None), _Nothing()
        try:
            got, crop = traced(lambda: me.automate(oid), me)
        finally:
            ref.cv2 = cv2
        if me.seen_box is None:
            assert not got
            return {"crop_box": crop.numpy().copy(), "box_2D": None, "skipped": True}
        rounds_out.append(got)
        return {"crop_box": crop.numpy().copy(), "box_2D": me.seen_box.numpy().copy(), "skipped": False}

    def box_to_state(me, point):
        got = me.box_to_state(point)
        assert str(got.dtype) == "torch.float32" and str(got.mean(dim=0).dtype) == "torch.float32"
        return got.numpy()
    return {"box_to_state": box_to_state, "find_box": lambda me, p: me.find_box(p), "copy_paste": lambda me, p: me.copy_paste(p),
            "paste2d": paste2d, "automate": automate}


def restated_ops(rounds_out):
    plain = ac.ref_paste_in_2D_bbox

    def paste2d(me, box):
        got = plain(me, box)
        rounds_out.append(got)
        return got

    def automate(me, oid, detect):
        before = len(rounds_out)
        ac.ref_paste_in_2D_bbox = paste2d                       # ref_automate's own search is recorded too
        try:
            got = ac.ref_automate(me, oid, detect)
        finally:
            ac.ref_paste_in_2D_bbox = plain
        assert len(rounds_out) == before + (0 if got["skipped"] else 1)
        return got
    return dict(ac.RESTATED, paste2d=paste2d, automate=automate)


def run_scene(ref, hgmod, name, scene):
    steps = ac.golden_script(scene)
    ref_rounds, my_rounds = [], []
    theirs = ac.replay(stand_in(ref, hgmod, scene), steps, reference_ops(ref, ref_rounds))
    mine = ac.replay(ac.Labels(scene), steps, restated_ops(my_rounds))
    assert len(ref_rounds) == len(my_rounds) and len(ref_rounds) > 0
    worst_diff, worst_gap, n_cand = 0.0, np.inf, 0
    for a, b in zip(ref_rounds, my_rounds):
        assert len(a) == len(b) == len(ac.radii())
        for (e, i), (f, j) in zip(a, b):
            assert e.shape == f.shape and e.dtype == f.dtype == np.float32 and int(np.argmin(e)) == i
            n_cand += len(e)
            if i != j:
                raise SystemExit("fixture condition: the restatement's winner %d is not the reference's %d" % (j, i))
            diff = np.abs(e.astype(np.float64) - f.astype(np.float64)) / np.maximum(np.abs(e.astype(np.float64)), 1e-300)
            worst_diff = max(worst_diff, float(diff.max()))
            e1, e2 = np.sort(e)[:2].astype(np.float64)
            worst_gap = min(worst_gap, (e2 - e1) / e2)
    min_gap = GAP_FACTOR * worst_diff
    if not worst_gap >= min_gap:
        raise SystemExit("fixture condition: a round's two smallest errors are %.3g apart (relative), MIN_GAP is %.3g"
                         % (worst_gap, min_gap))
    for key in theirs:
        same = theirs[key].shape == mine[key].shape and theirs[key].dtype == mine[key].dtype and \
            np.array_equal(theirs[key], mine[key], equal_nan=theirs[key].dtype.kind == "f")
        if not same:
            raise SystemExit("fixture condition: the restatement's %s differs from the reference's" % key)
    assert theirs["data_idx"][:, 5:].all()                      # every x and y a Python float
    return {name + "_" + k: v for k, v in theirs.items()}, (worst_diff, worst_gap, n_cand, len(ref_rounds))


def main(out_dir):
    ref, hgmod = import_reference()
    out = {}
    for name, scene in ac.golden_scenes().items():
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            got, (diff, gap, n_cand, n_search) = run_scene(ref, hgmod, name, scene)
        out.update(got)
        print("%-7s %d arrays, %d searches, %d candidates: largest relative difference %.3g (bit-equal: %s), smallest relative gap "
              "%.3g, %d automate calls (%d skipped), %d printed lines"
              % (name, len(got), n_search, n_cand, diff, diff == 0.0, gap, len(got[name + "_auto_skip"]),
                 int(got[name + "_auto_skip"].sum()), log.getvalue().count("\n")))
    mr.save_npz(os.path.join(out_dir, "label_assist.npz"), out)


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else mg.OUT)
