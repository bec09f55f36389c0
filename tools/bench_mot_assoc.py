"""Identity and association scores (csrc/mot_assoc.hip, mot_evaluator.evaluate_association) on the tracking-evaluation
benchmark's sequence -- tests/mot_cases.synth_sequence at its own size, 2 000 frames of 40 objects -- and on a fragmented
variant with several times more predicted ids than true ones (tests/mot_assoc_cases.fragmented_sequence).  Per stage the device
time of one call (HIP events around the op: its memsets and launches), the whole evaluate_association call and the CPU
restatement (tests/mot_assoc_cases.restated, on the device's own IoU matrices) with the wall clock, the size of the id
workspace, and whether the results are identical.  Writes profiles/mot_assoc.txt.
    python tools/bench_mot_assoc.py [frames] [objects]"""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "3d-playground_amd")):
    sys.path.insert(0, p)
import homography                                   # noqa: E402
import mot_assoc_cases as ac                        # noqa: E402
import mot_cases as mc                              # noqa: E402
import mot_evaluator as me                          # noqa: E402
from retinanet_mi355x import _hip, ops              # noqa: E402


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
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def workload(name, gt, pred, hg, dev, frames):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    pk = me.pack_tracks(gt, pred, hg, frames)
    n_gid, n_pid = len(pk["gid"]), len(pk["pid"])
    offsets, totals = ops.mot_offsets(pk["n_gt"], pk["n_pred"], dev)
    cor = hg.correspondence[hg.default_correspondence]
    _, gt_box, pred_box, _ = ops.mot_prepare(up(pk["gt_im"]), up(pk["gt_h0"]), up(pk["gt_vel"]), up(pk["pred_state"]),
                                             up(np.asarray(cor["H"], np.float64)), up(np.asarray(cor["P"], np.float64)))
    iou = ops.mot_iou(gt_box, pred_box, offsets, totals)
    gt_id, pred_id, alphas = up(pk["gt_id"]), up(pk["pred_id"]), up(ops.mot_alphas())
    csr = tuple(up(a) for a in ops.mot_id_csr(pk["n_gt"], pk["n_pred"], pk["gt_id"], n_gid))
    lines = ["%s: %d frames, %d + %d objects, %d ground-truth ids x %d predicted ids, %d assignment slots"
             % (name, len(pk["frames"]), len(pk["gt_id"]), len(pk["pred_id"]), n_gid, n_pid, totals[3]),
             "  id workspace (fp64 copy of C, solver vectors, 19 layers of M): %.2f MB; C %.2f MB, pot %.2f MB"
             % (_hip.load().rn_mot_assoc_workspace_bytes(n_gid, n_pid) / 1e6, n_gid * n_pid * 4 / 1e6, n_gid * n_pid * 8 / 1e6),
             "  device time of one call (HIP events):"]
    (gc, pc, C, _), t = timed(lambda: ops.mot_id_counts(iou, offsets, totals, gt_id, pred_id, n_gid, n_pid, 0.5))
    lines.append("    mot_id_counts                                  : " + stat(t))
    _, t = timed(lambda: ops.mot_id_assign(C))
    lines.append("    mot_id_assign (one wave, %4d x %4d)           : " % (n_gid, n_pid) + stat(t))
    (pot, _), t = timed(lambda: ops.mot_hota_align(iou, offsets, totals, gt_id, pred_id, csr, n_gid, n_pid))
    lines.append("    mot_hota_align (row / column sums + pot)       : " + stat(t))
    assigned, t = timed(lambda: ops.mot_hota_assign(iou, offsets, totals, gt_id, pred_id, gc, pc, pot, alphas))
    lines.append("    mot_hota_assign (one wave per frame)           : " + stat(t))
    _, t = timed(lambda: ops.mot_hota_reduce(offsets, totals, assigned, gt_id, pred_id, gc, pc))
    lines.append("    mot_hota_reduce (histogram, suffix, 19 sums)   : " + stat(t))
    (m, out), t = wall(lambda: me.evaluate_association(gt, pred, hg, frames, collect=True), 5)
    lines.append("  evaluate_association, whole call (pack + upload + IoU + 5 stages + copy back): " + stat(t))
    _, t = wall(lambda: me.pack_tracks(gt, pred, hg, frames), 3)
    lines.append("    of which pack_tracks on the host             : " + stat(t))
    gi, pi = {v: k for k, v in pk["gid"].items()}, {v: k for k, v in pk["pid"].items()}
    g_ids, p_ids, mats, go, po, co = [], [], [], 0, 0, 0
    for ng, npr in zip(pk["n_gt"], pk["n_pred"]):
        g_ids.append([gi[v] for v in pk["gt_id"][go:go + ng]])
        p_ids.append([pi[v] for v in pk["pred_id"][po:po + npr]])
        mats.append(out["iou"][co:co + ng * npr].reshape(ng, npr) if ng and npr else None)
        go, po, co = go + ng, po + npr, co + ng * npr
    scene = dict(gt_ids=g_ids, pred_ids=p_ids, ious=mats)
    w, t = wall(lambda: ac.restated(scene, 0.5), 1)
    lines.append("  CPU restatement (numpy + scipy) on the same IoU matrices: " + stat(t))
    same = all(m[k] == w[k] for k in me.ASSOC_SCALARS) and out["pot"].tobytes() == w["pot"].tobytes() \
        and all(m["per_alpha"][k].tobytes() == w["per_alpha"][k].tobytes() for k in ac.FIGURES)
    lines.append("  identical to the restatement (every scalar, pot and the per-alpha figures bit for bit): %s" % same)
    lines.append("  " + "  ".join("%s %.4f" % (k, m[k]) for k in ("HOTA", "DetA", "AssA", "LocA", "IDF1", "IDP", "IDR"))
                 + "  IDTP %d IDFP %d IDFN %d" % (m["IDTP"], m["IDFP"], m["IDFN"]))
    return lines


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    dev = torch.device("cuda:0")
    hg = homography.Homography(device="cuda:0")
    hg.correspondence = {"cam": {"H": mc.SYN_H, "P": mc.SYN_P}}
    hg.default_correspondence = "cam"
    lines = ["identity and association scores on %s" % torch.cuda.get_device_name(0)]
    lines += workload("synth_sequence", *mc.synth_sequence(frames, n, seed=0), hg, dev, frames)
    lines += workload("fragmented", *ac.fragmented_sequence(frames, n, seed=0), hg, dev, frames)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "mot_assoc.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
