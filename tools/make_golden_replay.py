#!/usr/bin/env python3
"""Generate tests/golden/replay.npz by running the REFERENCE's own Data_Reader.plot_in (datareader.py:294-399) -- build
container only.

The reference is imported unmodified from its checkout (never copied), as tools/make_golden_datareader.py does it.  plot_in
runs on a file of tests/datareader_cases.py (three cameras, six objects) with
  * its Camera_Wrapper replaced by a scripted stand-in: ``name``, ``ts`` from tests/replay_cases.py:script, a zero
    1080x1920x3 frame whose first byte carries the camera's number (so that the tile it lands in can be read back);
  * a recording cv2 stand-in: line / rectangle / putText note their integers and strings and draw nothing, getTextSize
    returns (6 * len, 8), addWeighted returns its first argument, waitKey returns -1, imshow closes an output frame.
The stamps are floats of a subclass that notes every ``cam_ts + bias - ts`` the loop forms, so dt is the reference's own.
The file holds data only: per output frame the label instant, the camera stamps, dt, the shifted boxes and state_to_im's
corners; every draw call; the tile of every camera.  This script refuses to run without the reference.

    python tools/make_golden_replay.py [--out DIR]
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import make_golden as mg                    # noqa: E402
import make_golden_datareader as mgd        # noqa: E402
import datareader_cases as dc               # noqa: E402
import replay_cases as rp                   # noqa: E402

FRAME_H, FRAME_W = 1080, 1920


class Stamp(float):
    """A camera stamp that notes the dt the loop forms from it (``cam_ts + bias - ts``) without changing a value or a type
    the loop sees further on."""
    noted = []

    def __add__(self, other):
        return Stamp(float(self) + other)

    def __sub__(self, other):
        r = float(self) - other
        Stamp.noted.append(r)
        return r


def main(out_dir):
    ref, hgmod = mgd.import_reference()
    cv2 = ref.cv2
    assert cv2 is hgmod.cv2
    names_all, P, P2 = dc.cameras()
    names = list(rp.GOLDEN_CAMERAS)
    text = dc.tracking_csv(**rp.GOLDEN_CSV)
    _, data = dc.load(text)
    stamps = rp.script(data)

    state = dict(frame=0, cam=-1, inside=False)
    rec = dict(lines=[], rects=[], texts=[], strings=[], inst=[], stamps=[], dt=[], n=[], views=[], corners=[], tiles=[])
    cams = []

    class Scripted:
        def __init__(self, sequence, ds=2):
            self.name, self.k, self.ts = sequence, 0, None
            self.frame = np.zeros((FRAME_H, FRAME_W, 3), np.uint8)
            self.frame[0, 0, 0] = names.index(sequence) + 1
            cams.append(self)

        def __next__(self):
            self.ts = Stamp(stamps[names.index(self.name), self.k])
            self.k += 1

        def release(self):
            pass

    def make_hg(M):
        hg = hgmod.Homography()
        hg.correspondence = {n: {"P": M[i]} for i, n in enumerate(names_all)}
        hg.default_correspondence = names_all[0]
        return hg
    hg = hgmod.Homography_Wrapper(hg1=make_hg(P), hg2=make_hg(P2))
    inner_to_im, inner_plot = hg.state_to_im, hg.plot_state_boxes

    def state_to_im(boxes, name=None):
        out = inner_to_im(boxes, name=name)
        if not state["inside"]:                                # plot_in's own call (:348): every object of the instant
            rec["views"].append(boxes.detach().clone().numpy().astype(np.float32))
            rec["corners"].append(out.detach().clone().numpy().astype(np.float64))
        return out

    def plot_state_boxes(im, boxes, name=None, **kw):
        state["cam"], state["inside"] = names.index(name), True
        try:
            return inner_plot(im, boxes, name=name, **kw)
        finally:
            state["inside"] = False
    hg.state_to_im, hg.plot_state_boxes = state_to_im, plot_state_boxes

    def line(im, a, b, color, thickness):
        rec["lines"].append([state["frame"], state["cam"], a[0], a[1], b[0], b[1], color[0], color[1], color[2], thickness])
        return im

    def rectangle(im, c1, c2, color, thickness):
        rec["rects"].append([state["frame"], state["cam"], c1[0], c1[1], c2[0], c2[1], color[0], color[1], color[2], thickness])
        return im

    def put_text(im, label, org, font, size, color, thickness):
        rec["texts"].append([state["frame"], state["cam"], org[0], org[1], color[0], color[1], color[2], thickness])
        rec["strings"].append(label)
        return im

    def imshow(title, cat_im):                                 # one output frame is complete
        rows, cols = cat_im.shape[0] // FRAME_H, cat_im.shape[1] // FRAME_W
        rec["tiles"].append([[int(round(cat_im[r * FRAME_H, c * FRAME_W, 0] * 255.0)) - 1 for c in range(cols)] for r in range(rows)])
        rec["inst"].append(dr.d_idx - 1)
        rec["stamps"].append([float(c.ts) for c in cams])
        rec["dt"].append(Stamp.noted[-len(cams):])
        rec["n"].append(len(rec["views"][-1]))
        state["frame"] += 1
    cv2.FONT_HERSHEY_PLAIN = 1
    cv2.line, cv2.rectangle, cv2.putText, cv2.imshow = line, rectangle, put_text, imshow
    cv2.getTextSize = lambda label, font, size, thickness: ((6 * len(label), 8), 0)
    cv2.addWeighted = lambda a, wa, b, wb, gamma: a
    cv2.setWindowTitle = lambda *a: None
    cv2.waitKey = lambda *a: -1
    cv2.destroyAllWindows = lambda: None
    ref.Camera_Wrapper = Scripted

    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "in.csv")
        with open(src, "w", newline="") as f:
            f.write(text)
        with contextlib.redirect_stdout(io.StringIO()):
            dr = ref.Data_Reader(src, hg)
            dr.plot_in(names)
    F = state["frame"]
    assert F >= 5 and dr.d_idx == len(dr.data), (F, dr.d_idx)                  # the labels ran out
    assert len(rec["views"]) == F * len(names) and len(Stamp.noted) == F * len(names)
    inst = np.asarray(rec["inst"], np.int64)
    assert (np.diff(inst) >= 2).any(), inst                                     # the jump over two label instants
    out = {"csv": np.frombuffer(text.encode(), np.uint8), "names": np.array(names), "script": stamps,
           "inst": inst, "stamps": np.asarray(rec["stamps"], np.float64), "dt": np.asarray(rec["dt"], np.float64),
           "n": np.asarray(rec["n"], np.int64), "views": np.concatenate(rec["views"]), "corners": np.concatenate(rec["corners"]),
           "lines": np.asarray(rec["lines"], np.int32), "rects": np.asarray(rec["rects"], np.int32),
           "texts": np.asarray(rec["texts"], np.int32), "strings": np.array(rec["strings"]),
           "tiles": np.asarray(rec["tiles"], np.int32)}
    path = os.path.join(out_dir, "replay.npz")
    np.savez_compressed(path, **out)
    print("replay: %d output frames, instants %s, %d lines, %d labels, %.1f KiB"
          % (F, inst.tolist(), len(out["lines"]), len(out["rects"]), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else mg.OUT)
