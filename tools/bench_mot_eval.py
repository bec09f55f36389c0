"""Tracking evaluation (csrc/mot_eval.hip, mot_evaluator.evaluate_tracks) on a synthesised sequence -- 2 000 frames of
40 x 40 by default, seeded (tests/mot_cases.synth_sequence) -- beside the host restatement of the reference's loop
(tests/mot_cases.restated) on the same input.  The device part (upload, five launches, result block back) is timed with HIP
events: warm-up, then the median of several runs; the host packing (CSV rows -> flat arrays) and the restatement with the
wall clock.  Writes profiles/mot_eval_bench.txt.
    python tools/bench_mot_eval.py [frames] [objects]"""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "3d-playground_amd")):
    sys.path.insert(0, p)
import homography                                   # noqa: E402
import mot_cases as mc                              # noqa: E402
import mot_evaluator as me                          # noqa: E402


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    dev = torch.device("cuda:0")
    hg = homography.Homography(device="cuda:0")
    hg.correspondence = {"cam": {"H": mc.SYN_H, "P": mc.SYN_P}}
    hg.default_correspondence = "cam"
    gt, pred = mc.synth_sequence(frames, n, seed=0)
    t0 = time.perf_counter()
    pk = me.pack_tracks(gt, pred, hg, frames)
    t_pack = time.perf_counter() - t0
    for _ in range(3):
        out = me.run_packed(pk, hg, 0.51, dev)
    torch.cuda.synchronize()
    times = []
    for _ in range(9):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = me.run_packed(pk, hg, 0.51, dev)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    metrics, _ = me.metrics_from_result(out["result"], 0.51)
    t0 = time.perf_counter()
    want = mc.restated(gt, pred, mc.SYN_H, mc.SYN_P, 0.51, frames)
    t_ref = time.perf_counter() - t0
    keys = ("TP", "FP", "FN", "FP edge-case", "Fragmentations", "ID switches", "True unique objects", "Predicted unique objects")
    same = all(metrics[k] == want["metrics"][k] for k in keys)
    lines = ["tracking evaluation, %d frames of %d x %d, match_iou 0.51" % (frames, n, n),
             "  device (upload + 5 launches + result block): median %.2f ms, min %.2f, max %.2f over %d runs after 3 warm-ups"
             % (float(np.median(times)), min(times), max(times), len(times)),
             "  host packing of the rows (once per sequence): %.1f ms" % (t_pack * 1e3),
             "  host restatement of the reference's loop (numpy + scipy): %.1f ms" % (t_ref * 1e3),
             "  same integer metrics as the restatement: %s   %s" % (same, {k: metrics[k] for k in keys})]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "mot_eval_bench.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
