#!/usr/bin/env python3
"""Time the detector-assisted labelling (label_assist.py / csrc/label_assist.hip) on one instant of the full deployment -- 18
cameras of 1080p with 40 boxes each, 720 boxes -- against the numpy restatement (tests/label_assist_cases.py) on the CPU of the
same machine.  Device times come from HIP events around repeated launches, after a warm-up call; whole calls are timed by the
host clock around work that ends in a device synchronise.  Recorded: every launch of the chain apart, the whole
``automate_many`` with a stand-in detector (fixed LOCALIZE outputs: the chain without the network) and with the 2D ResNet-50
localiser at batch 720, and the number of device -> host copies of one call.  The launch of rn_label_fit_box2d is set beside the
operation floor of its projections: boxes x rounds x grid^2 candidates x 8 corners x the fp64 operations of one projection (18
multiplies and adds, 2 divides counted as one operation each) at the FP64 vector rate.  The feature is new: there is no earlier
timing to beat.  Reported, not a gate.

    python tools/bench_label_assist.py [--cameras 18] [--boxes 40] [--out profiles/label_assist.txt] [--no-resnet]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "3d-playground_amd"), os.path.join(REPO, "tools")):
    sys.path.insert(0, p)

import label_audit_cases as lc               # noqa: E402
import label_assist_cases as ac              # noqa: E402
import label_assist as la                    # noqa: E402
from bench_label_audit import events, wall   # noqa: E402
from datareader import _upload               # noqa: E402
from retinanet_mi355x import ops             # noqa: E402

FP64_OPS_PER_S = 157.3e12 / 2 / 2            # as tools/bench_label_rewrite.py: fp64 instructions x lanes per second, no fma
OPS_PER_CORNER = 3 * 6 + 2
H, W, CS, ANCHORS, CLASSES = 1080, 1920, 112, 2394, 8


def instant(n_cam, per_cam, seed=3):
    """One frame of ``per_cam`` boxes in each of ``n_cam`` cameras, all inside their camera's frame, both directions."""
    rng = np.random.RandomState(seed)
    s = lc.empty_scene(n_cam, 1, seed=seed)
    s["frame_idx"] = 0
    s["hg_old"] = ac.hg_spec(s["names"])
    for c in range(n_cam):
        for k in range(per_cam):
            east = k % 2 == 0
            y = rng.uniform(8.0, 45.0) if east else rng.uniform(68.0, 95.0)
            ac.put(s, 0, c, k, 60.0 * c + 35.0 + rng.uniform(-35.0, 20.0), y, rng.uniform(12.0, 30.0), rng.uniform(5.0, 8.0),
                   rng.uniform(4.0, 9.0), gen="Interpolation")
    return s


class Fixed():
    """A stand-in localiser: the same LOCALIZE outputs whatever the crops hold."""

    def __init__(self, n, dev, seed=9):
        cls, reg, _ = ac.fuzz_detector(n, ANCHORS, CLASSES, seed)
        self.cls, self.reg, self.training = torch.from_numpy(cls).to(dev), torch.from_numpy(reg).to(dev), False

    def eval(self):
        pass

    def __call__(self, crops, LOCALIZE=False):
        return self.reg[:crops.shape[0]], self.cls[:crops.shape[0]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=18)
    ap.add_argument("--boxes", type=int, default=40)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--restate", type=int, default=40, help="boxes the restatement is timed on (scaled to all)")
    ap.add_argument("--no-resnet", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out_file = open(args.out, "w") if args.out else None

    def say(s):
        print(s, flush=True)
        if out_file:
            out_file.write(s + "\n")
            out_file.flush()
    scene = instant(args.cameras, args.boxes)
    names = scene["names"]
    keys = list(scene["data"][0])
    n = len(keys)

    class Me(ac.Labels, la.LabelAssist):
        pass
    say("label assist on %s: %d cameras of %d x %d, %d boxes each, %d boxes in the instant"
        % (torch.cuda.get_device_name(0), args.cameras, W, H, args.boxes, n))
    frames = torch.randint(0, 256, (args.cameras, H, W, 3), dtype=torch.uint8, device=dev)

    # ---- the launches of the chain, apart
    me = Me(scene)
    state = np.array([[scene["data"][0][k][s] for s in ac.STATE_KEYS] for k in keys], np.float32)
    cam = np.array([names.index(scene["data"][0][k]["camera"]) for k in keys], np.int32)
    H1, H2 = la._tables(me.hg, names, "H")
    P1, P2 = la._tables(me.hg, names, "P")
    radii = np.array(ops.label_rebase_radii(la.SEARCH_RAD), np.float64)
    t_up, up = wall(lambda: _upload(dev, [state, cam, radii, H1, P1, H2, P2]))
    d_state, d_cam, d_rad = up[0], up[1], up[2]
    dP1, dP2, dH1, dH2 = la._mats(up[4], 4), la._mats(up[6], 4), up[3], up[5]
    fixed = Fixed(n, dev)
    say("upload of the boxes and camera tables, one copy: %.3f ms (host clock)" % t_up)
    say("launches (HIP events, mean of %d after a warm-up call):" % args.reps)
    ms, (crop, rois, win, skipped, status) = events(lambda: ops.label_crop_windows(d_state, d_cam, dP1, dP2), args.reps)
    say("  rn_label_crop_windows, %d boxes                                   : %9.4f ms   (%d skipped by the edge test)"
        % (n, ms, int(skipped.sum())))
    reps_big = max(3, args.reps // 4)
    ms, im = events(lambda: ops.frame_ingest(frames, swap_rb=False, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)), reps_big)
    say("  rn_frame_ingest (to_tensor), %d frames of 1080p, mean of %d        : %9.4f ms   (%.0f MB read, %.0f MB written)"
        % (args.cameras, reps_big, ms, frames.numel() / 1e6, im.numel() * 4 / 1e6))
    ms, crops = events(lambda: ops.roi_align(im, rois, (CS, CS)), args.reps)
    say("  rn_roi_align, %d crops of %d x %d                                : %9.4f ms" % (n, CS, CS, ms))
    mean = torch.tensor(la.MEAN, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(la.STD, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    ms, _ = events(lambda: crops.clone().sub_(mean).div_(std), args.reps)
    say("  normalize (clone, sub_, div_: three torch launches)                 : %9.4f ms" % ms)
    ms, (box, _, _, _) = events(lambda: ops.label_best_anchor(fixed.cls, fixed.reg, win, CS), args.reps)
    say("  rn_label_best_anchor, %d crops x %d anchors x %d classes          : %9.4f ms   (%.1f MB of scores)"
        % (n, ANCHORS, CLASSES, ms, fixed.cls.numel() * 4 / 1e6))
    ms, centre = events(lambda: la._centres(box.double(), d_cam, dH1, dH2), args.reps)
    say("  the starting centres (rn_im_to_state of %d points + torch glue)   : %9.4f ms" % (2 * n, ms))
    ms, fit = events(lambda: ops.label_fit_box2d(d_state[:, 2:].contiguous(), d_cam, centre, box, dP1, dP2, d_rad, la.GRID_SIZE,
                                                 skip=skipped), args.reps)
    rounds, grid = len(radii), la.GRID_SIZE
    live = n - int(skipped.sum())
    work = live * rounds * grid * grid * 8 * OPS_PER_CORNER
    floor = work / FP64_OPS_PER_S * 1e3
    say("  rn_label_fit_box2d, %d boxes x %d rounds x %d candidates         : %9.4f ms" % (live, rounds, grid * grid, ms))
    say("    operation floor: %.3g fp64 operations of the projections (%d per corner, 8 corners) at %.1f T/s = %.5f ms;"
        % (work, OPS_PER_CORNER, FP64_OPS_PER_S / 1e12, floor))
    say("    the launch is %.0fx that (%d boxes are %d waves, a few per CU: a launch this small is bound by latency, not by rate;"
        % (ms / floor, live, live))
    say("    the floor counts a divide as one operation and leaves out the corner sums, the extent, the error and the reduction)")

    # ---- the same stages in the numpy restatement, on this machine's CPU
    sub = min(args.restate, n)
    h_box, h_win = box.cpu().numpy(), win.cpu().numpy()
    t_win, _ = wall(lambda: ac.crop_windows(state, cam, P1, P2))
    t_anchor, _ = wall(lambda: ac.best_anchor(fixed.cls[:sub].cpu().numpy(), fixed.reg[:sub].cpu().numpy(), h_win[:sub], CS))
    keep = np.nonzero(skipped.cpu().numpy() == 0)[0][:sub]
    h_centre = centre.cpu().numpy()
    t_fit, _ = wall(lambda: ac.fit_boxes(state[keep, 2:], cam[keep], h_centre[keep], h_box[keep], P1, P2))
    say("the numpy restatement on the CPU (host clock): crop windows of %d boxes %.1f ms; best anchor of %d crops %.1f ms -> %.1f ms"
        % (n, t_win, sub, t_anchor, t_anchor / sub * n))
    say("  for %d; the search of %d boxes %.1f ms -> %.1f ms for %d (%.0fx the launch of rn_label_fit_box2d)"
        % (n, len(keep), t_fit, t_fit / len(keep) * live, live, t_fit / len(keep) * live / ms))

    # ---- whole calls
    copies = [0]
    plain = torch.Tensor.cpu

    def counting(self, *a, **k):
        copies[0] += 1
        return plain(self, *a, **k)

    def whole(detector, reps):
        me = Me(scene)
        me.detector = detector
        me.automate_many(keys, frames)                          # warm-up: code objects, the network's own set-up
        torch.Tensor.cpu, copies[0] = counting, 0
        try:
            one = Me(scene)
            one.detector = detector
            one.automate_many(keys, frames)
        finally:
            torch.Tensor.cpu = plain
        n_copies, total = copies[0], 0.0
        for _ in range(reps):
            m = Me(scene)
            m.detector = detector
            t, res = wall(lambda: m.automate_many(keys, frames))
            total += t
        return total / reps, n_copies, res, m
    t_fixed, n_copies, res, m = whole(fixed, 50)
    say("automate_many, %d keys, frames on the device, stand-in detector (host clock, mean of 50): %.2f ms, %d device -> host copy"
        % (n, t_fixed, n_copies))
    say("  (one pass over the dicts, one upload, one launch each of windows, ingest, roi_align, best anchor and fit, one copy back;")
    say("   %d of the %d boxes rewritten)" % (sum(not r["skipped"] for r in res.values()), n))
    want = ac.Labels(scene)
    t_ref = 0.0
    for key in keys[:sub]:
        o = want.data[0][key]
        want.active_cam, want.clicked_camera = names.index(o["camera"]), o["camera"]
        want.copied_box = (o["id"], o.copy(), [np.float32(0), np.float32(0)])
        i = keys.index(key)
        t, _ = wall(lambda: ac.ref_automate(want, o["id"], lambda c_idx, crop: h_box[i]))
        t_ref += t
    same = all(m.data[0][k] == want.data[0][k] for k in keys[:sub])
    say("  the restatement's automate without its detector, key by key, %d keys: %.1f ms -> %.1f ms for %d (%.0fx); same data: %s"
        % (sub, t_ref, t_ref / sub * n, n, t_ref / sub * n / t_fixed, same))
    if not args.no_resnet:
        from retinanet_mi355x import modules
        torch.manual_seed(0)
        net = modules.resnet50(num_classes=CLASSES, directional=False).to(dev)
        t_net, n_copies, res, _ = whole(net, 10)
        ms_net, _ = events(lambda: net(crops, LOCALIZE=True), 10)
        say("automate_many with the 2D ResNet-50 localiser at batch %d (untrained weights; host clock, mean of 10): %.1f ms, %d device"
            % (n, t_net, n_copies))
        say("  -> host copy; the network's forward alone (HIP events, mean of 10): %.1f ms = %.0f%% of the call" % (ms_net, 100 * ms_net / t_net))
    if out_file:
        out_file.close()


if __name__ == "__main__":
    main()
