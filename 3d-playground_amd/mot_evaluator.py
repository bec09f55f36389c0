"""Drop-in for the reference's ``mot_evaluator.py``: ``MOT_Evaluator(gt_path, pred_path, homography, params).evaluate()``
scores a tracking CSV against a ground-truth CSV -- TP / FP / FN, recall, precision, false-alarm rate, fragmentations, ID
switches, the three MOTA figures, the IoU / state / pixel precision figures and the class confusion matrix -- with the same
``params`` keys, ``metrics`` keys, ``confusion``, ``units`` and ``print_metrics`` table.

The reference walks the frames in Python (six homography calls, a double loop over ``self.iou`` and scipy per frame).  Here
the host parses both files once, maps ids and class strings to dense indices, packs all frames into flat arrays with
per-frame offsets and uploads them in one go; five kernels of csrc/mot_eval.hip score the sequence (ops.mot_*), and one
result block of ops.MOT_RESULT doubles comes back.  The per-match lists of ``self.m`` are copied back only when asked for
(``evaluate(collect=True)`` / ``evaluate_tracks(..., collect=True)``); ``evaluate`` goes through ``evaluate_tracks``.
There is no CPU path.

Beyond the reference: ``evaluate_association`` / ``params["association"]`` add the identity scores (IDF1 / IDP / IDR) and
the HOTA family from the same packed frames (csrc/mot_assoc.hip, ops.mot_id_* / ops.mot_hota_*); with the key absent or
False ``evaluate`` is unchanged.

Differences a caller can see, all stated in INTEGRATION.md: ``params["sequence"]`` (plotting through cv2) raises
NotImplementedError; the (mean, deviation) figures are summed in fp64 in a fixed order, where the reference sums the fp32
stack in fp32 -- they agree to the reference's own summation error; a frame with more than ops.MOT_MAX objects on a side
raises; a NaN coordinate raises ValueError with scipy's wording, as the reference does through scipy.
"""
import numpy as np
import torch

from homography import load_i24_csv
from retinanet_mi355x import ops

STATE_COLS = (39, 40, 43, 42, 44, 35, 38)           # mot_evaluator.py:189
FIGURES = ("Pre-threshold IOU", "Match IOU", "X precision", "Y precision", "Length precision", "Width precision",
           "Height precision", None, "Velocity precision", "Bottom im precision", "Top im precision")   # result order; None: direction


class _Dense:
    """Values -> dense indices in first-seen order."""
    def __init__(self):
        self.index = {}

    def __call__(self, v):
        return self.index.setdefault(v, len(self.index))


def pack_tracks(gt_rows, pred_rows, hg, cutoff_frame):
    """The frames in [0, cutoff_frame) that either side holds, in increasing order, as flat host arrays."""
    frames = sorted(f for f in set(gt_rows) | set(pred_rows) if 0 <= f < cutoff_frame)
    gid, pid = _Dense(), _Dense()

    def cls_index(c):
        try:
            v = hg.class_dict[c]
        except (KeyError, TypeError):
            return -1
        return v if isinstance(v, (int, np.integer)) and 0 <= v < 10 else -1
    g_im, g_vel, g_id, g_cls, p_state, p_id, p_cls, n_gt, n_pred = [], [], [], [], [], [], [], [], []
    scored, scored_cls = [], []                                          # rows of frames that both sides hold, and their classes
    for f in frames:
        g, p = gt_rows.get(f, ()), pred_rows.get(f, ())
        n_gt.append(len(g))
        n_pred.append(len(p))
        for box in g:
            g_id.append(gid(int(box[2])))
            if p:                                                        # a frame without predictions only counts ids
                scored.append(len(g_im))
                scored_cls.append(box[3])
                g_im.append(np.array(box[11:27]).astype(float))
                g_vel.append(float(box[38]) if len(box[38]) > 0 else 0)
            else:
                g_im.append(np.zeros(16))
                g_vel.append(0.0)
            g_cls.append(cls_index(box[3]))
        for box in p:
            p_id.append(pid(int(box[2])))
            if g:
                row = list(box) + [2] if len(box) == 44 else box         # no height column (:186-187)
                p_state.append(np.array([row[c] for c in STATE_COLS]).astype(float))
            else:
                p_state.append(np.zeros(7))
            p_cls.append(cls_index(box[3]))
    h0 = np.ones(len(g_im), np.float32)                                  # the reference guesses heights only where it scores
    if scored:
        h0[scored] = hg.guess_heights(scored_cls).numpy().astype(np.float32)
    return dict(frames=frames, n_gt=n_gt, n_pred=n_pred, gt_im=np.asarray(g_im, np.float64).reshape(-1, 8, 2), gt_h0=h0,
                gt_vel=np.asarray(g_vel, np.float64).astype(np.float32), gt_id=np.asarray(g_id, np.int32),
                gt_cls=np.asarray(g_cls, np.int32), pred_state=np.asarray(p_state, np.float64).reshape(-1, 7).astype(np.float32),
                pred_id=np.asarray(p_id, np.int32), pred_cls=np.asarray(p_cls, np.int32), gid=gid.index, pid=pid.index)


def run_packed(pk, hg, match_iou, device, ious=None, collect=False):
    """Upload once, five launches, one result block back.  ious: a flat fp64 device tensor replacing rn_mot_iou's output."""
    dev = torch.device(device)
    cor = hg.correspondence[hg.default_correspondence]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    H, P = up(np.asarray(cor["H"], np.float64)), up(np.asarray(cor["P"], np.float64))
    offsets, totals = ops.mot_offsets(pk["n_gt"], pk["n_pred"], dev)      # raises above ops.MOT_MAX, before any launch
    gt_im, gt_h0, gt_vel, pred_state = up(pk["gt_im"]), up(pk["gt_h0"]), up(pk["gt_vel"]), up(pk["pred_state"])
    gt_id, pred_id, gt_cls, pred_cls = up(pk["gt_id"]), up(pk["pred_id"]), up(pk["gt_cls"]), up(pk["pred_cls"])
    gt_state, gt_box, pred_box, pred_im = ops.mot_prepare(gt_im, gt_h0, gt_vel, pred_state, H, P)
    iou = ops.mot_iou(gt_box, pred_box, offsets, totals) if ious is None else ious
    assigned = ops.mot_assign(iou, offsets, totals, pred_id.numel())
    per_slot = ops.mot_frame_metrics(iou, offsets, totals, assigned, match_iou, gt_state, pred_state, gt_im, pred_im, gt_cls,
                                     pred_cls, gt_id, pred_id)
    result = ops.mot_reduce(offsets, totals, assigned, per_slot, gt_id, pred_id, len(pk["gid"]), len(pk["pid"]))
    out = dict(result=result.cpu().numpy())
    if collect:
        out.update(iou=iou.cpu().numpy(), slot_row=assigned[0].cpu().numpy(), slot_col=assigned[1].cpu().numpy(),
                   slot_iou=per_slot[0].cpu().numpy(), slot_gid=per_slot[1].cpu().numpy(), slot_pid=per_slot[2].cpu().numpy(),
                   state_err=per_slot[3].cpu().numpy(), bot=per_slot[4].cpu().numpy(), top=per_slot[5].cpu().numpy(),
                   gt_state=gt_state.cpu().numpy(), pred_im=pred_im.cpu().numpy())
    return out


def metrics_from_result(res, match_iou):
    """The reference's ``metrics`` dict (mot_evaluator.py:348-408) from the result block."""
    if res[11] != 0:
        frame = int(res[12])
        if int(res[11]) == ops.MOT_INVALID:
            raise ValueError("matrix contains invalid numeric entries (frame slot %d)" % frame)
        if int(res[11]) == ops.MOT_INFEASIBLE:
            raise ValueError("cost matrix is infeasible (frame slot %d)" % frame)
        raise RuntimeError("frame slot %d holds more than %d objects on a side" % (frame, ops.MOT_MAX))
    TP, FP, FN, edge, FP02, FN02, n_gt, n_pred, frag, sw = (int(v) for v in res[:10])
    m = {"iou_threshold": match_iou, "True unique objects": n_gt, "Predicted unique objects": n_pred, "TP": TP, "FP": FP, "FN": FN,
         "FP edge-case": edge, "FP @ 0.2": FP02, "FN @ 0.2": FN02}
    m["Recall"] = TP / (TP + FN)                                        # TP = 0: ZeroDivisionError, as the reference
    m["Precision"] = TP / (TP + FP)
    m["False Alarm Rate"] = FP / TP
    m["Fragmentations"] = frag
    m["ID switches"] = sw
    m["MOTA"] = 1 - (FN + frag + sw + FP) / TP
    m["MOTA edge-case"] = 1 - (FN + frag + sw + FP - edge) / TP
    m["MOTA @ 0.2"] = 1 - (FN02 + frag + sw + FP02) / TP
    fig = {}
    with np.errstate(all="ignore"):
        for q, name in enumerate(FIGURES):
            if name is None:
                continue
            n, s1, s2 = res[16 + 3 * q:19 + 3 * q]
            if q < 2:                                                   # np.mean / np.std: population, fp64
                fig[name] = (np.float64(s1 / n), np.float64(np.sqrt(s2 / n)))
            else:                                                       # torch.mean / torch.std: sample
                dt = torch.float32 if q <= 8 else torch.float64         # the state stack is fp32, the image errors fp64
                fig[name] = (torch.tensor(s1 / n, dtype=dt), torch.tensor(np.sqrt(s2 / (n - 1)), dtype=dt))
    for name in ("Pre-threshold IOU", "Match IOU", "Width precision", "Height precision", "Length precision", "Velocity precision",
                 "X precision", "Y precision", "Bottom im precision", "Top im precision"):
        m[name] = fig[name]
    return m, res[52:152].astype(np.int64).reshape(10, 10)


def evaluate_tracks(gt_rows, pred_rows, homography, match_iou=0, cutoff_frame=10000, collect=False, m=None, pk=None):
    """For callers that already hold the per-frame dicts of load_i24_csv: -> (metrics, confusion), and with collect=True a
    third value, the per-pair arrays (IoU matrices, assignment slots, per-match vectors).  m: the evaluator's running dict;
    its counters and confusion matrix are set before the ratios are formed, so they outlive TP = 0 as in the reference."""
    if pk is None:                                                       # pk: pack_tracks' result, for a caller that packs once
        pk = pack_tracks(gt_rows, pred_rows, homography, cutoff_frame)
    out = run_packed(pk, homography, match_iou, getattr(homography, "device", "cuda:0"), collect=collect)
    res = out["result"]
    if m is not None and res[11] == 0:
        for k, key in enumerate(("TP", "FP", "FN", "FP edge-case", "FP @ 0.2", "FN @ 0.2")):
            m[key] = int(res[k])
        m["cls"] = res[52:152].astype(int).reshape(10, 10)
    metrics, confusion = metrics_from_result(res, match_iou)
    if collect:
        out["packed"] = pk
        return metrics, confusion, out
    return metrics, confusion


# ------------------------------------------------------------------------------------------------ identity and association
ASSOC_SCALARS = ("IDF1", "IDP", "IDR", "IDTP", "IDFP", "IDFN", "HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA",
                 "HOTA(0)")
ASSOC_FIGURES = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")
ASSOC_TAIL = 6                                                           # IDTP, its status, the two (code, where) status pairs


def run_association(pk, hg, id_iou, device, ious=None, collect=False):
    """Upload once, the five stages of csrc/mot_assoc.hip, one block back: ops.MOT_ASSOC_RESULT doubles of rn_mot_hota_reduce,
    then IDTP, the identity assignment's status, and (code, where) of rn_mot_id_counts and of rn_mot_hota_align."""
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    n_gid, n_pid = len(pk["gid"]), len(pk["pid"])
    offsets, totals = ops.mot_offsets(pk["n_gt"], pk["n_pred"], dev)      # raises above ops.MOT_MAX, before any launch
    ops.mot_assoc_dims("evaluate_association", n_gid, n_pid)              # ... and above the dense storage's cap
    gt_id, pred_id = up(pk["gt_id"]), up(pk["pred_id"])
    if ious is None:
        cor = hg.correspondence[hg.default_correspondence]
        H, P = up(np.asarray(cor["H"], np.float64)), up(np.asarray(cor["P"], np.float64))
        _, gt_box, pred_box, _ = ops.mot_prepare(up(pk["gt_im"]), up(pk["gt_h0"]), up(pk["gt_vel"]), up(pk["pred_state"]), H, P)
        ious = ops.mot_iou(gt_box, pred_box, offsets, totals)
    csr = tuple(up(a) for a in ops.mot_id_csr(pk["n_gt"], pk["n_pred"], pk["gt_id"], n_gid))
    alphas = up(ops.mot_alphas())
    gc, pc, C, st_counts = ops.mot_id_counts(ious, offsets, totals, gt_id, pred_id, n_gid, n_pid, id_iou)
    match, info = ops.mot_id_assign(C)
    pot, st_align = ops.mot_hota_align(ious, offsets, totals, gt_id, pred_id, csr, n_gid, n_pid)
    assigned = ops.mot_hota_assign(ious, offsets, totals, gt_id, pred_id, gc, pc, pot, alphas)
    result = ops.mot_hota_reduce(offsets, totals, assigned, gt_id, pred_id, gc, pc)
    block = torch.cat((result, info.double(), st_counts.double(), st_align.double()))
    out = dict(result=block.cpu().numpy())
    if collect:
        out.update(iou=ious.cpu().numpy(), gc=gc.cpu().numpy(), pc=pc.cpu().numpy(), C=C.cpu().numpy(), id_match=match.cpu().numpy(),
                   pot=pot.cpu().numpy(), slot_row=assigned[0].cpu().numpy(), slot_col=assigned[1].cpu().numpy(),
                   slot_s=assigned[2].cpu().numpy(), slot_n=assigned[3].cpu().numpy())
    return out


def association_from_result(res, n_gt_objects, n_pred_objects, alphas=None):
    """The identity and HOTA figures from run_association's block.  The ratios and the means over alpha are formed here."""
    R = ops.MOT_ASSOC_RESULT
    idtp, id_status, c_code, c_where, a_code, a_where = (int(v) for v in res[R:R + ASSOC_TAIL])
    for code, where, what in ((c_code, c_where, "frame slot"), (a_code, a_where, "ground-truth id index")):
        if code == ops.MOT_DUPLICATE_ID:
            raise ValueError("an id occurs twice in one frame on one side (%s %d); the identity and association scores need "
                             "ids that are unique within a frame" % (what, where))
        if code != 0:
            raise RuntimeError("association scores: an index outside the packed layout (code %d, %s %d)" % (code, what, where))
    status, frame = int(res[R - 2]), int(res[R - 1])
    if status == ops.MOT_INVALID:
        raise ValueError("matrix contains invalid numeric entries (frame slot %d)" % frame)
    if status == ops.MOT_INFEASIBLE or id_status == ops.MOT_INFEASIBLE:
        raise ValueError("cost matrix is infeasible (frame slot %d)" % frame)
    if status != 0:
        raise RuntimeError("association scores: frame slot %d has status %d" % (frame, status))
    idfn, idfp = n_gt_objects - idtp, n_pred_objects - idtp
    m = {"IDF1": idtp / max(1, idtp + 0.5 * idfp + 0.5 * idfn), "IDP": idtp / max(1, idtp + idfp), "IDR": idtp / max(1, idtp + idfn),
         "IDTP": idtp, "IDFP": idfp, "IDFN": idfn}
    blk = np.asarray(res[:ops.MOT_ALPHAS * 7], np.float64).reshape(ops.MOT_ALPHAS, 7)
    TP, FN, FP, loc, a_sum, re_sum, pr_sum = (blk[:, k] for k in range(7))
    per = {"TP": TP.astype(np.int64), "FN": FN.astype(np.int64), "FP": FP.astype(np.int64)}
    per["AssA"] = a_sum / np.maximum(1, TP)
    per["AssRe"] = re_sum / np.maximum(1, TP)
    per["AssPr"] = pr_sum / np.maximum(1, TP)
    per["DetRe"] = TP / np.maximum(1, TP + FN)
    per["DetPr"] = TP / np.maximum(1, TP + FP)
    per["DetA"] = TP / np.maximum(1, TP + FN + FP)
    per["HOTA"] = np.sqrt(per["DetA"] * per["AssA"])
    per["LocA"] = np.maximum(1e-10, loc) / np.maximum(1e-10, TP)
    for name in ASSOC_FIGURES:
        m[name] = float(np.mean(per[name]))
    m["HOTA(0)"] = float(per["HOTA"][0])
    m["alphas"] = ops.mot_alphas() if alphas is None else np.asarray(alphas, np.float64)
    m["per_alpha"] = per
    return m


def evaluate_association(gt_rows, pred_rows, homography, cutoff_frame=10000, id_iou=0.5, collect=False, ious=None):
    """IDF1 / IDP / IDR (Ristani et al. 2016) and the HOTA family (Luiten et al. 2021) of a tracking output, on the device.
    These go beyond the reference's evaluator.  -> a dict with IDF1, IDP, IDR, IDTP, IDFP, IDFN; HOTA, DetA, AssA, DetRe, DetPr,
    AssRe, AssPr, LocA (means over alpha); "HOTA(0)"; "alphas" and "per_alpha" (the arrays).  ious: a flat fp64 device tensor
    replacing rn_mot_iou's output, as in run_packed.  collect=True returns (dict, the per-stage arrays)."""
    return _association(pack_tracks(gt_rows, pred_rows, homography, cutoff_frame), homography, id_iou, collect, ious)


def _association(pk, homography, id_iou, collect=False, ious=None):
    out = run_association(pk, homography, id_iou, getattr(homography, "device", "cuda:0"), ious=ious, collect=collect)
    m = association_from_result(out["result"], int(np.sum(pk["n_gt"])), int(np.sum(pk["n_pred"])))
    if collect:
        out["packed"] = pk
        return m, out
    return m


class MOT_Evaluator():
    def __init__(self, gt_path, pred_path, homography, params=None):
        self.match_iou = 0
        self.cutoff_frame = 10000
        self.sequence = None
        self.association = False
        self.id_iou = 0.5
        self.gt_mode = "im"
        self.hg = homography
        _, self.gt = load_i24_csv(gt_path)
        _, self.pred = load_i24_csv(pred_path)
        if params is not None:
            self.match_iou = params.get("match_iou", self.match_iou)
            self.cutoff_frame = params.get("cutoff_frame", self.cutoff_frame)
            self.sequence = params.get("sequence", self.sequence)
            self.association = bool(params.get("association", self.association))
            self.id_iou = params.get("id_iou", self.id_iou)
        if self.sequence is not None:
            raise NotImplementedError("params['sequence'] plots every frame through cv2 (mot_evaluator.py:242-277); "
                                      "this evaluator scores only")
        n_classes = len(self.hg.class_heights.keys())
        self.m = {"FP": 0, "FP edge-case": 0, "FP @ 0.2": 0, "FN @ 0.2": 0, "FN": 0, "TP": 0, "pre_thresh_IOU": [], "match_IOU": [],
                  "state_err": [], "im_bot_err": [], "im_top_err": [], "cls": np.zeros([n_classes, n_classes]).astype(int), "ids": {},
                  "gt_ids": [], "pred_ids": []}
        self.units = {"Match IOU": "", "Pre-threshold IOU": "", "Width precision": "ft", "Height precision": "ft",
                      "Length precision": "ft", "Velocity precision": "ft/s", "X precision": "ft", "Y precision": "ft",
                      "Bottom im precision": "px", "Top im precision": "px"}

    def evaluate(self, collect=False):
        """collect=True also fills the per-match lists of ``self.m`` (one more copy from the device)."""
        pk = pack_tracks(self.gt, self.pred, self.hg, self.cutoff_frame) if self.association else None   # packed once for both
        got = evaluate_tracks(self.gt, self.pred, self.hg, self.match_iou, self.cutoff_frame, collect=collect, m=self.m, pk=pk)
        self.metrics, self.confusion = got[0], got[1]
        if collect:
            self._collect(got[2]["packed"], got[2])
        if self.association:                                             # after the reference's keys; absent or False: nothing changes
            assoc = self.association_metrics = _association(pk, self.hg, self.id_iou)
            for key in ASSOC_SCALARS:
                self.metrics[key] = assoc[key]
        self.print_metrics()

    def evaluate_association(self, collect=False):
        """Only the identity and association figures (IDF1, HOTA, ...): the dict of the module's evaluate_association, kept in
        ``self.association_metrics``."""
        got = evaluate_association(self.gt, self.pred, self.hg, self.cutoff_frame, self.id_iou, collect=collect)
        self.association_metrics = got[0] if collect else got
        return got

    def _collect(self, pk, out):
        """The reference's per-match lists, in its order: frames in increasing order, matches by ascending row."""
        ok = out["slot_gid"] >= 0
        gid = {v: k for k, v in pk["gid"].items()}
        pid = {v: k for k, v in pk["pid"].items()}
        self.m["pre_thresh_IOU"] = list(out["slot_iou"][out["slot_row"] >= 0])
        self.m["match_IOU"] = list(out["slot_iou"][ok])
        self.m["state_err"] = list(torch.from_numpy(out["state_err"][ok]))
        self.m["im_bot_err"] = list(torch.from_numpy(out["bot"][ok]))
        self.m["im_top_err"] = list(torch.from_numpy(out["top"][ok]))
        ids, gt_ids, pred_ids = {}, [], []
        gi, pi, k = 0, 0, 0                                              # first gt row, pred row and slot of the frame
        for ng, npr in zip(pk["n_gt"], pk["n_pred"]):
            if ng == 0:
                for j in range(pi, pi + npr):
                    if pid[pk["pred_id"][j]] not in pred_ids:
                        pred_ids.append(pid[pk["pred_id"][j]])
            elif npr == 0:
                for i in range(gi, gi + ng):
                    if gid[pk["gt_id"][i]] not in gt_ids:
                        gt_ids.append(gid[pk["gt_id"][i]])
            for s in range(k, k + min(ng, npr)):
                if ok[s]:
                    g, p = gid[out["slot_gid"][s]], pid[out["slot_pid"][s]]
                    if g not in ids:
                        ids[g] = [p]
                    elif ids[g][-1] != p:
                        ids[g].append(p)
                    if p not in pred_ids:
                        pred_ids.append(p)
                    if g not in gt_ids:
                        gt_ids.append(g)
            gi, pi, k = gi + ng, pi + npr, k + min(ng, npr)
        self.m["ids"], self.m["gt_ids"], self.m["pred_ids"] = ids, gt_ids, pred_ids

    def print_metrics(self):
        print("\n")
        for name in self.metrics:
            try:
                unit = self.units[name]
                print("{:<30}: {:.2f}{} avg., {:.2f}{} st.dev.".format(name, self.metrics[name][0], unit, self.metrics[name][1], unit))
            except (KeyError, TypeError, IndexError):
                print("{:<30}: {:.3f}".format(name, self.metrics[name]))
        print("Class confusion matrix:")
        print(self.confusion)
