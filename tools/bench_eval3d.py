"""3D validation (csrc/eval_cuboid.hip, eval3d.evaluate_cuboids) on a validation set of 1 000 images x 100 detections x 10
annotations over 8 classes: projected cuboids in a 1920 x 1080 frame, seven detections in ten a jittered copy of an
annotation of their class.  Per launch the device time of one call (HIP events around the op: its memsets and launches),
the whole evaluate_cuboids call and the plain Python / numpy restatement on the CPU (tests/eval3d_cases.restated) with the
wall clock, and whether the results are identical.  Writes profiles/eval3d.txt.
    python tools/bench_eval3d.py [images] [detections] [annotations]"""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "3d-playground_amd")):
    sys.path.insert(0, p)
import eval3d_cases as e3                           # noqa: E402
from retinanet_mi355x import eval3d, ops            # noqa: E402

C = 8


def stat(times):
    return "%9.3f ms  (min %.3f, max %.3f, n = %d)" % (float(np.median(times)), min(times), max(times), len(times))


def timed(fn, n=20, warm=3):
    for _ in range(warm):
        out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return out, times


def wall(fn, n):
    times = []
    for _ in range(n):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def validation_set(images, K, N, seed=0):
    rng = np.random.RandomState(seed)
    dets, labels = [], []
    for _ in range(images):
        cls = rng.randint(0, C, N)
        anns = [np.asarray(e3.cuboid(rng.uniform(0, 1500), rng.uniform(0, 780), rng.uniform(20, 400), rng.uniform(20, 300)))
                for _ in range(N)]
        labels.append(e3.labels_of(*[e3.label(a, c) for a, c in zip(anns, cls)]))
        rows = []
        for k in range(K):
            if rng.rand() < 0.7:
                j = rng.randint(N)
                d, c = anns[j] + rng.normal(0, (0.5, 3.0, 10.0, 40.0)[k % 4], 16), cls[j]
            else:
                d = np.asarray(e3.cuboid(rng.uniform(0, 1500), rng.uniform(0, 780), rng.uniform(20, 400), rng.uniform(20, 300)))
                c = rng.randint(0, C)
            rows.append((rng.uniform(0.06, 1.0), c, d))
        dets.append(e3.det_rows(rows))
    return dets, labels


def main():
    images, K, N = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 1000), (2, 100), (3, 10)))
    dev = torch.device("cuda:0")
    dets, labels = validation_set(images, K, N)
    tdets = [tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in d) for d in dets]
    thr = (0.5, 0.7)
    rows = images * K
    ac, ao = e3.pack_labels(labels, C)
    M = len(ac)
    ac, ao = torch.from_numpy(ac).to(dev), torch.from_numpy(ao).to(dev)
    lines = ["3D validation on %s" % torch.cuda.get_device_name(0),
             "%d images x %d detections x %d annotations, %d classes: %d table rows, %d annotations, thresholds %s"
             % (images, K, N, C, rows, M, list(thr)), "  device time of one call (HIP events):"]

    def select(corners_too):
        table, img_rows, state = ops.eval_table(rows, images, dev)
        corners = torch.zeros((rows, 16), dtype=torch.float32, device=dev)
        for i, (s, l, b) in enumerate(tdets):
            ops.eval_select(s, l, b, table, img_rows, state, i, C, 0.05, 100, (16, 20))
            if corners_too:
                ops.eval_corners(b, table, img_rows, i, corners)
        return table, img_rows, state, corners
    _, t0 = timed(lambda: select(False), n=5, warm=1)
    (table, img_rows, state, corners), t1 = timed(lambda: select(True), n=5, warm=1)
    lines.append("    eval_select, %d launches                      : " % images + stat(t0))
    lines.append("    eval_select + eval_corners, %d launches each  : " % images + stat(t1))
    (best_iou, best_ann), t = timed(lambda: ops.eval_cuboid_overlap(table, img_rows, corners, ac, ao, C, "silhouette"))
    pairs = int(sum(int(np.sum(l[:, 20] == c)) * int(np.sum(d[1] == c)) for d, l in zip(dets, labels) for c in range(C)))
    lines.append("    eval_cuboid_overlap (%d pairs, one wave per group): " % pairs + stat(t))
    for name in ("base", "top"):
        _, t = timed(lambda: ops.eval_cuboid_overlap(table, img_rows, corners, ac, ao, C, name))
        lines.append("    eval_cuboid_overlap, overlap = %-5s             : " % name + stat(t))
    (tp, num, matched), t = timed(lambda: ops.eval_cuboid_assign(table, img_rows, best_iou, best_ann, ao, M, C, list(thr)))
    lines.append("    eval_cuboid_assign (2 thresholds)               : " + stat(t))
    _, t = timed(lambda: ops.eval_ap(table, state, tp[0], num))
    lines.append("    eval_ap, one threshold (sort + AP)              : " + stat(t))
    (terms, sums), t = timed(lambda: ops.eval_cuboid_errors(table, state, img_rows, corners, ac, ao, C, tp[0], matched, best_iou))
    lines.append("    eval_cuboid_errors (terms + ordered sums)       : " + stat(t))
    res, t = wall(lambda: eval3d.evaluate_cuboids(tdets, labels, C, iou_thresholds=thr), 5)
    lines.append("  evaluate_cuboids, whole call (pack + upload + %d + 6 launches-groups + copy back): " % (2 * images) + stat(t))
    _, t = wall(lambda: eval3d._pack_labels(eval3d.split_labels(labels), C), 3)
    lines.append("    of which packing the labels on the host         : " + stat(t))
    want, t = wall(lambda: e3.restated(dets, labels, C, iou_thresholds=thr), 1)
    lines.append("  CPU restatement (plain Python / numpy, tests/eval3d_cases.restated): " + stat(t))
    same = all(np.ascontiguousarray(x.cpu().numpy()).tobytes() == np.ascontiguousarray(want[k]).tobytes()
               for k, x in (("best_iou", best_iou), ("best_ann", best_ann), ("tp", tp), ("matched", matched), ("terms", terms),
                            ("sums", sums)))
    lines.append("  identical to the restatement (best_iou, best_ann, tp, matched, terms, sums bit for bit): %s" % same)
    lines.append("  errors equal the restatement's summary: %s" % (res["errors"] == e3.summary(want, thr)["errors"]))
    lines.append("  mAP " + "  ".join("@%.1f %.4f" % (k, v) for k, v in res["mAP"].items())
                 + "  true positives %d of %d rows" % (sum(v["tp"] for v in res["errors"].values()), rows)
                 + "  mean corner error %.3f px  reversed %d"
                 % (sum(v["corner_px"] * v["tp"] for v in res["errors"].values()) / max(1, sum(v["tp"] for v in res["errors"].values())),
                    sum(v["reversed"] for v in res["errors"].values())))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "eval3d.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
