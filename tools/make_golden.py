#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE itself (build container only).

The reference (/root/reference, read-only, never copied) is imported unmodified
behind three harness-side shims:

  1. a stub ``torchvision.ops.nms`` (torchvision is not installed) -- the build's own greedy NMS
     (oracle/boxes.py); NMS results are therefore "parity unpinned" and only the surrounding
     reference logic (threshold loops, per-class loops, offset trick) is pinned by these vectors;
  2. an empty stub ``cv2`` (only fitting/plotting code touches it);
  3. ``Tensor.cuda`` -> identity, except a leaf that requires grad returns a clone (a real ``.cuda()``
     returns a non-leaf copy; D/losses.py:310 writes into such a tensor in place).

The augmentation section (gen_augment) adds a fourth: ``torchvision.transforms`` / ``functional`` as the thin Pillow
wrappers of tools/tv_pillow_stub.py, so that the reference's own Detection_Dataset.__getitem__ and collate run; the
colour-jitter draws are therefore "parity unpinned" as well.

Inputs come from ``retinanet_mi355x.synth`` (portable integer-hash generators), so the fixtures
hold OUTPUTS (and the few inputs built with libm/LAPACK).  This script refuses to run without
/root/reference and is never executed on the GPU box.

    python tools/make_golden.py                     # writes tests/golden/*.npz
    python tools/make_golden.py --out DIR [names]   # elsewhere (tests/test_golden_regen.py compares with the committed set)
"""
import hashlib
import importlib
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "3d-playground_amd"))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from retinanet_mi355x import synth          # noqa: E402
from oracle import boxes as oboxes          # noqa: E402  (only its greedy_nms, as shim 1)


def install_shims():
    tv = types.ModuleType("torchvision")
    tv_ops = types.ModuleType("torchvision.ops")
    tv_ops.nms = oboxes.greedy_nms
    tv.ops = tv_ops
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.ops"] = tv_ops
    sys.modules["cv2"] = types.ModuleType("cv2")
    torch.Tensor.cuda = lambda self, *a, **k: self.clone() if (self.requires_grad and self.is_leaf) else self


def import_variant(which):
    """Import the reference's top-level ``retinanet`` package from D/ or R/ (same package name)."""
    for k in [k for k in sys.modules if k == "retinanet" or k.startswith("retinanet.")]:
        del sys.modules[k]
    root = os.path.join(REF, "pytorch_retinanet_detector_directional") if which == "dir" else REF
    sys.path.insert(0, root)
    try:
        model = importlib.import_module("retinanet.model")
        losses = importlib.import_module("retinanet.losses")
        utils = importlib.import_module("retinanet.utils")
        anchors = importlib.import_module("retinanet.anchors")
    finally:
        sys.path.remove(root)
    return model, losses, utils, anchors


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def t2n(t):
    return t.detach().cpu().numpy()


import golden_cases as gc                   # noqa: E402  (tests/golden_cases.py)


# ----------------------------------------------------------------------------- generators
def gen_anchors(anchors_mod):
    out = {}
    A = anchors_mod.Anchors()
    for (h, w) in [(64, 96), (72, 104), (112, 112), (96, 128), (512, 512)]:
        out["full_%dx%d" % (h, w)] = t2n(A(torch.zeros(1, 3, h, w)))
    for (h, w) in [(540, 960), (1080, 1920), (1081, 1917)]:
        a = t2n(A(torch.zeros(1, 3, h, w)))
        out["sha_%dx%d" % (h, w)] = np.array(sha(a))
        out["count_%dx%d" % (h, w)] = np.array(a.shape[1])
        out["sample_%dx%d" % (h, w)] = a[0, ::997].copy()
    np.savez_compressed(os.path.join(OUT, "anchors.npz"), **out)


def gen_losses(losses_dir_mod, losses_2d_mod, anchors_mod):
    H, W = gc.LOSS_HW
    anc = anchors_mod.Anchors()(torch.zeros(1, 3, H, W))
    out = {}
    # pairwise IoU + assignment (integers must be reproduced bit-exactly)
    ann = gc.loss_labels_dir()
    for j in range(ann.shape[0]):
        lab = ann[j][ann[j, :, 20] != -1]
        if lab.shape[0] == 0:
            continue
        xs, ys = lab[:, 0:16:2], lab[:, 1:16:2]
        env = torch.stack((xs.min(1).values, ys.min(1).values, xs.max(1).values, ys.max(1).values), 1)
        iou = losses_dir_mod.calc_iou(anc[0], env)
        m, a = torch.max(iou, dim=1)
        out["dir_iou_max_%d" % j] = t2n(m)
        out["dir_iou_arg_%d" % j] = t2n(a)
    # directional loss, forward + input gradients, all images and each image alone
    cls, reg = gc.loss_heads(12, 21)
    cls.requires_grad_(True)
    reg.requires_grad_(True)
    fl = losses_dir_mod.FocalLoss()
    l = fl(cls, reg, anc, ann.clone())
    (l[0] + 2.0 * l[1] + 3.0 * l[2]).sum().backward()
    out["dir_losses"] = np.array([float(x.detach()) for x in l], dtype=np.float32)
    out["dir_dcls"] = t2n(cls.grad)
    out["dir_dreg"] = t2n(reg.grad)
    for j in (0, 1, 3, 4):
        lj = fl(cls[j:j + 1].detach(), reg[j:j + 1].detach(), anc, ann[j:j + 1].clone())
        out["dir_losses_img%d" % j] = np.array([float(x) for x in lj], dtype=np.float32)
    # 2D loss
    ann2 = gc.loss_labels_2d()
    cls2, reg2 = gc.loss_heads(4, 31)
    cls2.requires_grad_(True)
    reg2.requires_grad_(True)
    fl2 = losses_2d_mod.FocalLoss()
    l2 = fl2(cls2, reg2, anc, ann2.clone())
    (l2[0] + 2.0 * l2[1]).sum().backward()
    out["2d_losses"] = np.array([float(x.detach()) for x in l2], dtype=np.float32)
    out["2d_dcls"] = t2n(cls2.grad)
    out["2d_dreg"] = t2n(reg2.grad)
    np.savez_compressed(os.path.join(OUT, "losses.npz"), **out)


class _Stub(torch.nn.Module):
    """Stands in for a head: returns preset per-level slices so the reference's own post-process code
    runs on designed inputs."""

    def __init__(self, full, level_counts):
        super().__init__()
        self.chunks = list(torch.split(full, level_counts, dim=1))
        self.i = 0

    def forward(self, x):
        c = self.chunks[self.i % len(self.chunks)]
        self.i += 1
        return c


def gen_boxes(model_dir, utils_dir, model_2d, utils_2d):
    out = {}
    H, W = gc.POST_HW
    counts = gc.level_counts(H, W)
    img = torch.zeros(1, 3, H, W)

    def pack(prefix, s, c, b, im=None):
        """scores/classes in full; boxes as sha + every 8th row (NMS itself is parity-unpinned: what these
        vectors pin is the reference's threshold loop, per-class loop, offset trick and gather order)."""
        out[prefix + "_scores"], out[prefix + "_classes"] = t2n(s), t2n(c)
        out[prefix + "_boxes_sha"] = np.array(sha(t2n(b)))
        out[prefix + "_boxes_sample"] = t2n(b)[::8].copy()
        if im is not None:
            out[prefix + "_im"] = t2n(im)
    # --- directional single-frame and LOCALIZE
    net = model_dir.resnet18(num_classes=2)
    net.eval()
    cls, reg = gc.post_single_inputs()
    net.regressionModel = _Stub(reg, counts)
    net.classificationModel = _Stub(cls, counts)
    with torch.no_grad():
        boxes, cls_back = net(img, LOCALIZE=True)
        s, c, b = net(img)
    out["dir_decode_sha"] = np.array(sha(t2n(boxes)))
    out["dir_decode_sample"] = t2n(boxes)[0, ::53].copy()
    pack("dir_single", s, c, b)
    # --- MULTI_FRAME, B = 3
    cls3, reg3 = gc.post_multi_inputs()
    net = model_dir.resnet18(num_classes=3)
    net.eval()
    net.regressionModel = _Stub(reg3, counts)
    net.classificationModel = _Stub(cls3, counts)
    with torch.no_grad():
        s, c, b, im = net(torch.zeros(3, 3, H, W), MULTI_FRAME=True)
    pack("dir_multi", s, c, b, im)
    # --- 2D: decode + clip + per-class 0.05 threshold + NMS
    net2 = model_2d.resnet18(num_classes=3)
    net2.eval()
    cls2, reg2 = gc.post_2d_inputs()
    net2.regressionModel = _Stub(reg2, counts)
    net2.classificationModel = _Stub(cls2, counts)
    with torch.no_grad():
        boxes2, _ = net2(img, LOCALIZE=True)
        s, c, b = net2(img)
    out["2d_decode_clip_sample"] = t2n(boxes2)[0, ::7].copy()
    out["2d_decode_clip_sha"] = np.array(sha(t2n(boxes2)))
    pack("2d", s, c, b)
    np.savez_compressed(os.path.join(OUT, "boxes.npz"), **out)


def _grad_summary(model, out, tag, full_limit=4096):
    for name, p in model.named_parameters():
        g = p.grad
        if g is None:
            continue
        g = t2n(g)
        out["%s_gsum_%s" % (tag, name)] = np.array([g.sum(dtype=np.float64), np.abs(g).sum(dtype=np.float64),
                                                    np.sqrt((g.astype(np.float64) ** 2).sum())])
        if g.size <= full_limit:
            out["%s_g_%s" % (tag, name)] = g


def gen_model(model_dir, model_2d):
    out = {}
    for arch in ("resnet18", "resnet50"):
        sd, img, ann = gc.model_inputs(arch, directional=True)
        net = getattr(model_dir, arch)(num_classes=4)
        net.load_state_dict(sd)
        net.train()
        net.freeze_bn()
        l = net([img, ann.clone()])
        (l[0] + l[1] + l[2]).sum().backward()
        out["%s_dir_losses" % arch] = np.array([float(x.detach()) for x in l], dtype=np.float32)
        _grad_summary(net, out, "%s_dir" % arch)
        net.eval()
        with torch.no_grad():
            boxes, cls = net(img, LOCALIZE=True)
        out["%s_dir_boxes" % arch] = t2n(boxes)
        out["%s_dir_cls" % arch] = t2n(cls)
    # 2D twin, cfg1-like plumbing at small size
    sd, img, ann = gc.model_inputs("resnet18", directional=False)
    net = model_2d.resnet18(num_classes=4)
    net.load_state_dict(sd)
    net.train()
    net.freeze_bn()
    l = net([img, ann.clone()])
    (l[0] + l[1]).sum().backward()
    out["resnet18_2d_losses"] = np.array([float(x.detach()) for x in l], dtype=np.float32)
    _grad_summary(net, out, "resnet18_2d")
    net.eval()
    with torch.no_grad():
        boxes, cls = net(img, LOCALIZE=True)
    out["resnet18_2d_boxes"] = t2n(boxes)
    out["resnet18_2d_cls"] = t2n(cls)
    np.savez_compressed(os.path.join(OUT, "model.npz"), **out)


def gen_model_deep(model_dir):
    """The other two architectures callers build: resnet34 = the tracker's crop detector (MC3D_crop_tracker.py:1535, at its
    112x112 crop size, batch 2) and resnet101 (BASELINE configs[4]).  Own files so that model.npz stays as it was, one per
    architecture so that each stays under the size limit of a committed file."""
    for arch, hw, batch in (("resnet34", gc.CROP_HW, 2), ("resnet101", gc.MODEL_HW, 1)):
        out = {}
        sd, img, ann = gc.model_inputs(arch, directional=True, hw=hw, batch=batch)
        net = getattr(model_dir, arch)(num_classes=4)
        net.load_state_dict(sd)
        net.train()
        net.freeze_bn()
        l = net([img, ann.clone()])
        (l[0] + l[1] + l[2]).sum().backward()
        out["%s_dir_losses" % arch] = np.array([float(x.detach()) for x in l], dtype=np.float32)
        _grad_summary(net, out, "%s_dir" % arch, full_limit=2048)
        net.eval()
        with torch.no_grad():
            boxes, cls = net(img, LOCALIZE=True)
        out["%s_dir_boxes" % arch] = t2n(boxes)
        out["%s_dir_cls" % arch] = t2n(cls)
        np.savez_compressed(os.path.join(OUT, gc.MODEL_CASES[arch][0] + ".npz"), **out)


def gen_homography():
    hgmod = ref_module_from_file("_reference_homography", "homography.py")
    out = {}
    names, state, cam_index, (Ps, Hs), (Ps2, Hs2) = gc.homography_inputs()
    out["P"], out["H"] = Ps, Hs

    def make_hg(P, H):
        hg = hgmod.Homography()
        hg.correspondence = {n: {"P": P[i], "H": H[i], "H_inv": np.linalg.inv(H[i])} for i, n in enumerate(names)}
        hg.default_correspondence = names[0]
        return hg
    hg = make_hg(Ps, Hs)
    cams = [names[i] for i in cam_index]
    out["state"] = t2n(state)
    out["cam_index"] = cam_index
    space = hg.state_to_space(state)
    out["space"] = t2n(space)
    out["space_to_state"] = t2n(hg.space_to_state(space))
    im_list = hg.state_to_im(state, name=cams)
    im_one = hg.state_to_im(state, name="p1c3")
    im_default = hg.state_to_im(state)
    out["im_list"], out["im_one"], out["im_default"] = t2n(im_list), t2n(im_one), t2n(im_default)
    heights = hg.guess_heights(["sedan", "semi", 3, "nonsense", "trailer", "truck (other)"])
    out["guess_heights"] = t2n(heights)
    h = state[:, 4]
    out["back_space_list"] = t2n(hg.im_to_space(im_list, name=cams, heights=h))
    out["back_state_list"] = t2n(hg.im_to_state(im_list, name=cams, heights=h))
    out["back_state_one"] = t2n(hg.im_to_state(im_one, name="p1c3", heights=h))
    out["height_from_template"] = t2n(hg.height_from_template(im_list, h, im_list * 1.07 + 3.0))
    # wrapper: second homography = perturbed cameras
    out["P2"], out["H2"] = Ps2, Hs2
    wr = hgmod.Homography_Wrapper(hg1=hg, hg2=make_hg(Ps2, Hs2))
    out["wr_im_list"] = t2n(wr.state_to_im(state, name=cams))
    out["wr_back_state_list"] = t2n(wr.im_to_state(t2n_t(out["wr_im_list"]), name=cams, heights=h))
    out["wr_im_one"] = t2n(wr.state_to_im(state, name="p2c4"))
    np.savez_compressed(os.path.join(OUT, "homography.npz"), **out)


def t2n_t(a):
    return torch.from_numpy(np.asarray(a))


def gen_csv_kat():
    """Known-answer rows from the reference's own result CSVs (data files): state columns ->
    space-corner columns (i24_state_to_space) and image-corner columns (space_to_im with the camera's P).
    A strided sample of rows is kept as a fixture; P is recovered per (camera, side of y=60) by DLT from the
    SAME rows inside the test (tests/test_homography_kat.py), so nothing but data is stored."""
    import csv
    rows = []
    for fi, fn in enumerate(("3D_tracking_results.csv", "working_3D_tracking_data.csv")):
        with open(os.path.join(REF, fn)) as f:
            rd = csv.reader(f)
            hdr = next(rd)
            col = {n: i for i, n in enumerate(hdr)}
            keep = ["fbrx", "fbry", "fblx", "fbly", "bbrx", "bbry", "bblx", "bbly", "ftrx", "ftry", "ftlx", "ftly",
                    "btrx", "btry", "btlx", "btly", "fbr_x", "fbr_y", "fbl_x", "fbl_y", "bbr_x", "bbr_y", "bbl_x",
                    "bbl_y", "direction", "veh rear x", "veh center y", "width", "length", "height"]
            n = 0
            for r in rd:
                if len(r) < len(hdr) - 1 or r[col["fbrx"]] == "":
                    continue
                n += 1
                if fn.startswith("3D_tracking") and n % 12:
                    continue
                cam = r[col["camera"]]
                rows.append([100.0 * fi + float(cam[1]) * 10 + float(cam[3])] + [float(r[col[k]]) for k in keep])
    arr = np.array(rows, dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, "csv_kat.npz"), rows=arr,
                        columns=np.array(["cam_code"] + keep))


def gen_csv_rows():
    """A strided sample of the reference's shipped result files AS TEXT (data files, not source): the byte-level fixture
    for the row formatting of write_results_csv (MC3D_crop_tracker.py:1318-1453).  One header + sample per file."""
    for fn, stride, out_name in (("3D_tracking_results.csv", 59, "results_rows_3D_tracking_results.csv"),
                                 ("working_3D_tracking_data.csv", 3, "results_rows_working_3D_tracking_data.csv")):
        with open(os.path.join(REF, fn), newline="") as f:
            lines = f.read().split("\r\n")
        keep = [lines[0]] + [l for i, l in enumerate(lines[1:]) if l and i % stride == 0]
        with open(os.path.join(OUT, out_name), "w", newline="") as f:
            f.write("\r\n".join(keep) + "\r\n")


def tracker_import_shims():
    """Two more stub attributes the tracker module needs at import time."""
    tv = sys.modules["torchvision"]
    tvt = types.ModuleType("torchvision.transforms")
    tvf = types.ModuleType("torchvision.transforms.functional")
    tvt.functional = tvf
    tv.transforms = tvt
    sys.modules["torchvision.transforms"] = tvt
    sys.modules["torchvision.transforms.functional"] = tvf

    def _no_roi_align(*a, **k):
        raise NotImplementedError("roi_align is not on this path")
    sys.modules["torchvision.ops"].roi_align = _no_roi_align
    matplotlib_stub()


def matplotlib_stub():
    """util_track/kf.py imports matplotlib.pyplot at the top (unused by the class, absent here)."""
    if "matplotlib" not in sys.modules:
        mpl = types.ModuleType("matplotlib")
        mpl.pyplot = types.ModuleType("matplotlib.pyplot")
        sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, mpl.pyplot


def gen_tracker_post():
    """MC_Crop_Tracker.parse_detections / im_nms / space_nms / md_iou (MC3D_crop_tracker.py:319-383, 592-636,
    1030-1049) run UNBOUND on a stand-in ``self`` that carries only the attributes those methods read (sigma_d,
    phi_nms_*, cameras, est_ts, hg = the reference's own Homography_Wrapper filled with the fixture's matrices).
    The module imports behind two more stub attributes (torchvision.transforms.functional, torchvision.ops.roi_align);
    constructing the tracker itself needs videos and checkpoints the reference does not ship."""
    trk, hgmod = import_reference_tracker()
    T = trk.MC_Crop_Tracker
    scores, labels, boxes, cams, names, (Ps, Hs), (Ps2, Hs2) = gc.tracker_post_inputs()

    def make_hg(P, H):
        hg = hgmod.Homography()
        hg.correspondence = {n: {"P": P[i], "H": H[i], "H_inv": np.linalg.inv(H[i])} for i, n in enumerate(names)}
        hg.default_correspondence = names[0]
        return hg
    me = types.SimpleNamespace(sigma_d=0.1, phi_nms_im=0.3, phi_nms_space=0.2, cameras=list(names), est_ts=False,
                               hg=hgmod.Homography_Wrapper(hg1=make_hg(Ps, Hs), hg2=make_hg(Ps2, Hs2)))
    me.im_nms = types.MethodType(T.im_nms, me)
    me.space_nms = types.MethodType(T.space_nms, me)
    out = {}
    for tag, kw in (("nms", dict(perform_nms=True, refine_height=False)),
                    ("nms_refine", dict(perform_nms=True, refine_height=True)),
                    ("plain", dict(perform_nms=False, refine_height=False))):
        st, lb, sc, cm = T.parse_detections(me, scores.clone(), labels.clone(), boxes.clone(), cams.clone(), **kw)
        out[tag + "_state"], out[tag + "_labels"] = t2n(st), t2n(lb)
        out[tag + "_scores"], out[tag + "_cams"] = t2n(sc), t2n(cm)
    keep = scores > 0.1
    det = boxes[keep].reshape(-1, 10, 2)[:, :8, :]
    out["im_nms_idx"] = t2n(T.im_nms(me, det, scores[keep], groups=cams[keep], threshold=0.3))
    out["im_nms_idx_nogroups"] = t2n(T.im_nms(me, det, scores[keep], threshold=0.3))
    st_plain = torch.from_numpy(out["plain_state"])
    out["space_nms_idx"] = t2n(T.space_nms(me, st_plain, torch.from_numpy(out["plain_scores"]), threshold=0.2))
    b4 = boxes[:64, 16:20].double()
    out["md_iou"] = t2n(T.md_iou(me, b4[None].repeat(64, 1, 1), b4[:, None].repeat(1, 64, 1)))
    empty = T.parse_detections(me, scores[:0], labels[:0], boxes[:0], cams[:0])
    low = T.parse_detections(me, scores * 0.01, labels, boxes, cams)
    out["empty_is_lists"] = np.array([all(isinstance(e, list) and len(e) == 0 for e in empty),
                                      all(isinstance(e, list) and len(e) == 0 for e in low)])
    np.savez_compressed(os.path.join(OUT, "tracker_post.npz"), **out)


def gen_crop_refine():
    """MC_Crop_Tracker.get_crop_boxes / local_to_global / select_best_box (MC3D_crop_tracker.py:920-1028) run unbound
    on a stand-in ``self`` (b, cs, W, device, hg, md_iou); same import shims as gen_tracker_post."""
    trk, hgmod = import_reference_tracker()
    T = trk.MC_Crop_Tracker
    from oracle import crop_refine as ocr          # only for the roi-free middle of the pipeline (top-k, homographies)
    pre_loc, cam, im_objs, names, (Ps, Hs), (Ps2, Hs2) = gc.crop_refine_inputs()

    def make_hg(P, H):
        hg = hgmod.Homography()
        hg.correspondence = {n: {"P": P[i], "H": H[i], "H_inv": np.linalg.inv(H[i])} for i, n in enumerate(names)}
        hg.default_correspondence = names[0]
        return hg
    me = types.SimpleNamespace(b=1.25, cs=112, W=0.5, device=torch.device("cpu"),
                               hg=hgmod.Homography_Wrapper(hg1=make_hg(Ps, Hs), hg2=make_hg(Ps2, Hs2)))
    me.md_iou = types.MethodType(T.md_iou, me)
    out = {}
    crop_boxes = T.get_crop_boxes(me, im_objs)
    out["crop_boxes"] = t2n(crop_boxes)
    reg_boxes, cls = gc.crop_detections(im_objs, crop_boxes)
    # as in track(): crop_boxes stays float64 (it comes from the float64 state_to_im), so the float32 detections are
    # promoted and the frame coordinates are float64 (MC3D_crop_tracker.py:1198, 1204)
    glob = T.local_to_global(me, reg_boxes.clone(), crop_boxes)
    out["local_to_global"] = t2n(glob)
    # the reference's own sequence between the detector and select_best_box (MC3D_crop_tracker.py:1188-1219), run with
    # the reference's Homography_Wrapper
    confs, classes = torch.max(cls, dim=2)
    top = torch.topk(confs, 50, dim=1)[1]
    rows = torch.arange(glob.shape[0]).unsqueeze(1).repeat(1, top.shape[1])
    g, confs, classes = glob[rows, top, :, :], confs[rows, top], classes[rows, top]
    n_objs = g.shape[0]
    cam_rep = [names[int(c)] for c in cam for _ in range(g.shape[1])]
    pts = g.reshape(-1, 8, 2)
    heights = me.hg.guess_heights(classes.reshape(-1))
    st = me.hg.im_to_state(pts, heights=heights, name=cam_rep)
    repro = me.hg.state_to_im(st, name=cam_rep)
    st = me.hg.im_to_state(pts, heights=me.hg.height_from_template(repro, heights, pts), name=cam_rep)
    out["cand_state"], out["cand_confs"], out["cand_classes"] = t2n(st), t2n(confs), t2n(classes)
    best, bcls, bconf = T.select_best_box(me, pre_loc.clone(), st.clone(), confs, classes, n_objs)
    out["best_state"], out["best_classes"], out["best_confs"] = t2n(best), t2n(bcls), t2n(bconf)
    np.savez_compressed(os.path.join(OUT, "crop_refine.npz"), **out)


def gen_datareader():
    """tests/golden/datareader.npz: the reference's Data_Reader on the cases of tests/datareader_cases.py.  Its own script
    (tools/make_golden_datareader.py), in a child process: it imports the reference's datareader and homography modules under
    their own names, which this process must not see."""
    import subprocess
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "make_golden_datareader.py"), "--out", OUT])


def gen_label_audit():
    """tests/golden/label_audit.npz: the batch passes of the reference's annotator (seems_to_be_working.py) on the scenes of
    tests/label_audit_cases.py.  Its own script (tools/make_golden_labels.py), in a child process, for the reason
    gen_datareader gives: the annotator imports the reference's homography, datareader and retinanet under their own names."""
    import subprocess
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "make_golden_labels.py"), "--out", OUT],
                          stdout=subprocess.DEVNULL)


def gen_label_rewrite():
    """tests/golden/label_rewrite.npz: replace_homgraphy, replace_y, offset_box_y and replace_timestamps of the reference's
    annotator on the scenes of tests/label_rewrite_cases.py.  Its own script (tools/make_golden_label_rewrite.py), in a child
    process, for the reason gen_label_audit gives."""
    import subprocess
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "make_golden_label_rewrite.py"), "--out", OUT],
                          stdout=subprocess.DEVNULL)


def gen_label_trajectory():
    """tests/golden/label_trajectory.npz: create_trajectory, get_splines, gen_trajectories and adjust_ts_with_trajectories of
    the reference's annotator and scipy's UnivariateSpline on the scenes of tests/label_trajectory_cases.py.  Its own script
    (tools/make_golden_label_trajectory.py), in a child process, for the reason gen_label_audit gives."""
    import subprocess
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "make_golden_label_trajectory.py"), "--out", OUT],
                          stdout=subprocess.DEVNULL)


def gen_label_quality():
    """tests/golden/label_quality.npz: calculate_total_variation, calculate_feasibility and annotator_rmse of the reference's
    later annotator on the scenes of tests/label_quality_cases.py.  Its own script (tools/make_golden_label_quality.py), in a
    child process, for the reason gen_label_audit gives."""
    import subprocess
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "make_golden_label_quality.py"), "--out", OUT],
                          stdout=subprocess.DEVNULL)


def gen_label_assist():
    """tests/golden/label_assist.npz: box_to_state, find_box, copy_paste, paste_in_2D_bbox and automate of the reference's v3
    annotator on the scripts of tests/label_assist_cases.py.  Its own script (tools/make_golden_label_assist.py), in a child
    process, for the reason gen_label_audit gives."""
    import subprocess
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "make_golden_label_assist.py"), "--out", OUT],
                          stdout=subprocess.DEVNULL)


def gen_track_stitch():
    """tests/golden/track_stitch.npz: the reference's shipped 3D_tracking_results.csv packed by tracklet, and the restatement of
    tests/stitch_cases.py on it.  Its own script (tools/make_golden_track_stitch.py), in a child process: it imports this
    repository's datareader under the name the reference's module takes above."""
    import subprocess
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "make_golden_track_stitch.py"), "--out", OUT],
                          stdout=subprocess.DEVNULL)


def gen_replay():
    """tests/golden/replay.npz: the reference's own Data_Reader.plot_in over scripted cameras behind a recording cv2 stand-in.
    Its own script (tools/make_golden_replay.py), in a child process, for the reason gen_datareader gives."""
    import subprocess
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "make_golden_replay.py"), "--out", OUT],
                          stdout=subprocess.DEVNULL)


def gen_tracker_run():
    """tests/golden/tracker_run.npz: the reference's own MC_Crop_Tracker.track() and write_results_csv() on the scene of
    tests/tracker_cases.py.  Its own script (tools/make_golden_tracker.py), in a child process: it patches module globals of
    the reference's tracker (nms, roi_align) and torch.cuda for the duration of the run."""
    import subprocess
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "make_golden_tracker.py"), "--out", OUT],
                          stdout=subprocess.DEVNULL)


def ref_module_from_file(alias, relpath):
    """A reference module loaded from its file, under a private name: this repository ships same-named drop-ins
    (util_track/kf.py, homography.py) that come first on sys.path, and a golden must come from the REFERENCE's code."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(alias, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert os.path.realpath(mod.__file__).startswith(os.path.realpath(REF) + os.sep)
    return mod


def import_reference_tracker():
    """MC3D_crop_tracker + homography with the reference checkout FIRST on sys.path, so that its own
    `from util_track.kf import ...` / `util_track.mp_loader` / `homography` resolve inside the reference (util_track is a
    namespace package there and a namespace portion here: whichever root comes first wins per submodule)."""
    for k in [k for k in sys.modules if k in ("homography", "MC3D_crop_tracker") or k == "util_track" or k.startswith("util_track.")]:
        del sys.modules[k]
    sys.path.insert(0, REF)
    try:
        trk = importlib.import_module("MC3D_crop_tracker")
        hgmod = importlib.import_module("homography")
    finally:
        sys.path.remove(REF)
    for m in (trk, hgmod, sys.modules["util_track.kf"]):
        assert os.path.realpath(m.__file__).startswith(os.path.realpath(REF) + os.sep), m.__file__
    for k in [k for k in sys.modules if k == "util_track" or k.startswith("util_track.") or k == "homography"]:
        del sys.modules[k]                          # later imports of these names are not to find the reference's
    return trk, hgmod


def gen_kf():
    """Torch_KF (util_track/kf.py) itself: add, predict with the default dt / a float dt / a per-object dt tensor, view,
    update.  The module imports matplotlib.pyplot at the top (unused by the class, absent here): stubbed."""
    matplotlib_stub()
    kfmod = ref_module_from_file("_reference_util_track_kf", "util_track/kf.py")
    INIT, det, directions, times, speed, upd_ids, z, dts = gc.kf_inputs()
    out = {}

    def snap(t):                                  # the class updates X, P and T in place: snapshots must be copies
        return t2n(t.clone())
    kf = kfmod.Torch_KF(torch.device("cpu"), INIT={k: v.clone() for k, v in INIT.items()}, ADD_MEAN_R=True)
    ids = list(range(100, 100 + len(det)))
    kf.add(det.clone(), ids, directions.clone(), times.clone())
    kf.X[:, 5] = speed
    out["X0"], out["P0"], out["T0"] = snap(kf.X), snap(kf.P), snap(kf.T)
    kf.predict()
    out["X1"], out["P1"], out["T1"] = snap(kf.X), snap(kf.P), snap(kf.T)
    kf.predict(dt=0.05)
    out["X2"], out["P2"], out["T2"] = snap(kf.X), snap(kf.P), snap(kf.T)
    kf.predict(dt=dts.clone())
    out["X3"], out["P3"], out["T3"] = snap(kf.X), snap(kf.P), snap(kf.T)
    _, v = kf.view(dt=dts.clone(), with_direction=True)
    out["view_dir"] = t2n(v)
    _, v = kf.view(dt=1 / 30.0)
    out["view_plain"] = t2n(v)
    kf.update(z.clone(), [ids[i] for i in upd_ids])
    out["X4"], out["P4"] = snap(kf.X), snap(kf.P)
    kf.remove([ids[0], ids[5]])
    out["X5"], out["T5"] = snap(kf.X), snap(kf.T)
    out["ids5"] = np.array(kf.view()[0])
    # the default constructor (diagonal matrices, H sees 4 of 5 measurements: kf.py:60-68)
    kd = kfmod.Torch_KF(torch.device("cpu"))
    kd.add(det.clone(), ids, directions.clone(), times.clone())
    kd.predict()
    kd.update(z.clone(), [ids[i] for i in upd_ids])
    out["Xd"], out["Pd"] = snap(kd.X), snap(kd.P)
    np.savez_compressed(os.path.join(OUT, "kf.npz"), **out)


def _run_sequence(T, kfmod, tc, hg, frames, ts_bias, out, before_frame=None, attrs=None, methods=()):
    """Detection frames through match_hungarian / manage_tracks / increment_fslds / remove_overlaps / remove_anomalies in
    track()'s order (MC3D_crop_tracker.py:1100-1137, 1259-1261, verbatim in substance) on a stand-in tracker with the
    reference's own Torch_KF; the state after every frame goes to out["seq<f>_*"].  ``before_frame(trkr, key, detections,
    labels, scores, camera_idxs)`` -> the four tensors to associate (the parse stage of the frame)."""
    trkr = types.SimpleNamespace(**{k: v for k, v in tc.PARAMS.items()})
    trkr.hg = hg
    trkr.class_dict = tc.class_dict()
    trkr.filter = kfmod.Torch_KF(torch.device("cpu"), INIT=tc.kf_init())
    trkr.fsld, trkr.all_classes, trkr.all_confs, trkr.all_cameras = {}, {}, {}, {}
    trkr.next_obj_id, trkr.updated_this_frame = 0, []
    trkr.time_metrics = {"add and remove": 0.0}
    trkr.ts_bias = list(ts_bias)
    for k, v in (attrs or {}).items():
        setattr(trkr, k, v)
    for meth in ("match_hungarian", "manage_tracks", "increment_fslds", "remove_overlaps", "remove_anomalies", "md_iou") + tuple(methods):
        setattr(trkr, meth, types.MethodType(getattr(T, meth), trkr))
    log = {}
    phase = ["none"]
    remove = trkr.filter.remove

    def logged_remove(ids):
        log[phase[0]] = sorted(int(i) for i in ids)
        remove(ids)
    trkr.filter.remove = logged_remove
    for f, fr in enumerate(frames):
        log.clear()
        key = "seq%d_" % f
        trkr.timestamps = list(fr["timestamps"])
        detections = torch.from_numpy(fr["detections"])
        labels, scores = torch.from_numpy(fr["labels"]), torch.from_numpy(fr["scores"])
        camera_idxs = torch.from_numpy(fr["cameras"])
        if before_frame is not None:
            detections, labels, scores, camera_idxs = before_frame(trkr, key, detections, labels, scores, camera_idxs)
        trkr.updated_this_frame = []
        avg_time = sum(trkr.timestamps) / len(trkr.timestamps)
        dts = trkr.filter.get_dt(avg_time)
        pre_ids, pre_loc = trkr.filter.view(with_direction=True, dt=dts)
        matchings = trkr.match_hungarian(pre_loc, detections)
        if len(matchings) > 0:
            assert len(trkr.filter.X) != 6, "see tests/track_cases.py:sequence (Q broadcast at 6 rows)"
            filter_idxs = [match[0] for match in matchings]
            match_times = [trkr.timestamps[camera_idxs[match[1]]] + trkr.ts_bias[camera_idxs[match[1]]] for match in matchings]
            dts = trkr.filter.get_dt(match_times, idxs=filter_idxs)
            trkr.filter.predict(dt=dts)
        detection_times = [trkr.timestamps[cam_idx] + trkr.ts_bias[cam_idx] for cam_idx in camera_idxs]
        trkr.manage_tracks(detections, matchings, pre_ids, labels, scores, camera_idxs, detection_times)
        updated = list(set(trkr.updated_this_frame))
        undetected = [i for i in pre_ids if i not in updated]
        phase[0] = "fsld"
        trkr.increment_fslds(pre_ids, undetected)
        phase[0] = "over"
        trkr.remove_overlaps()
        phase[0] = "anom"
        trkr.remove_anomalies(x_bounds=trkr.x_range)
        phase[0] = "none"
        out[key + "pre_ids"] = np.array(pre_ids, dtype=np.int64)
        out[key + "match"] = np.asarray(matchings, dtype=np.int64).reshape(-1, 2)
        fk = sorted(trkr.fsld)
        out[key + "fsld"] = np.array([[k, trkr.fsld[k]] for k in fk], dtype=np.int64).reshape(-1, 2)
        out[key + "next_obj_id"] = np.array(trkr.next_obj_id, dtype=np.int64)
        ids, _ = trkr.filter.view()
        out[key + "ids"] = np.array(ids, dtype=np.int64)
        out[key + "X"], out[key + "P"], out[key + "T"] = (t2n(trkr.filter.X.clone()), t2n(trkr.filter.P.clone()),
                                                            t2n(trkr.filter.T.clone()))     # predict works in place
        ck = sorted(trkr.all_classes)
        out[key + "classes"] = np.array([trkr.all_classes[k] for k in ck], dtype=np.float64).reshape(-1, 8)
        out[key + "class_ids"] = np.array(ck, dtype=np.int64)
        for ph in ("fsld", "over", "anom"):
            out[key + "rm_" + ph] = np.array(log.get(ph, []), dtype=np.int64)


def gen_tracker_assoc():
    """scipy.optimize.linear_sum_assignment on the matrices of tests/track_cases.py (indices only: both sides rebuild the
    matrices from seeds); MC_Crop_Tracker.match_hungarian run unbound on a stand-in ``self`` (hg, md_iou, phi_match);
    and a scripted 8-frame run of match_hungarian / manage_tracks / increment_fslds / remove_overlaps /
    remove_anomalies in track()'s order (MC3D_crop_tracker.py:1100-1137, 1259-1261) on the reference's own Torch_KF."""
    import track_cases as tc
    from scipy.optimize import linear_sum_assignment
    trk, hgmod = import_reference_tracker()
    T = trk.MC_Crop_Tracker
    kfmod = ref_module_from_file("_reference_util_track_kf", "util_track/kf.py")
    out = {}
    for name, c in tc.lsap_cases():
        r, k = linear_sum_assignment(c)
        out["lsap_%s_row" % name], out["lsap_%s_col" % name] = r.astype(np.int64), k.astype(np.int64)
    hg = hgmod.Homography()                                # state_to_space needs no camera: a bare wrapper
    me = types.SimpleNamespace(phi_match=tc.PHI_MATCH, hg=hgmod.Homography_Wrapper(hg1=hg, hg2=hgmod.Homography()))
    me.md_iou = types.MethodType(T.md_iou, me)
    for name, pre, det in tc.hungarian_cases():
        p, d = torch.from_numpy(pre), torch.from_numpy(det)
        if len(pre) and len(det):
            fp = me.hg.state_to_space(p.clone())
            fd = me.hg.state_to_space(d.clone())

            def env(s):
                b = torch.zeros([s.shape[0], 4])
                b[:, 0], b[:, 2] = torch.min(s[:, 0:4, 0], dim=1)[0], torch.max(s[:, 0:4, 0], dim=1)[0]
                b[:, 1], b[:, 3] = torch.min(s[:, 0:4, 1], dim=1)[0], torch.max(s[:, 0:4, 1], dim=1)[0]
                return b
            a, b = env(fp), env(fd)
            f, s = a.shape[0], b.shape[0]
            out["hung_%s_dist" % name] = t2n(1.0 - T.md_iou(me, a.unsqueeze(1).repeat(1, s, 1).double(),
                                                               b.unsqueeze(0).repeat(f, 1, 1).double()))
        m = T.match_hungarian(me, p.clone(), d.clone())
        out["hung_%s_is_list" % name] = np.array(isinstance(m, list))
        out["hung_%s_match" % name] = np.asarray(m, dtype=np.int64).reshape(-1, 2)
    _run_sequence(T, kfmod, tc, me.hg, tc.sequence(), tc.TS_BIAS, out)
    np.savez_compressed(os.path.join(OUT, "tracker_assoc.npz"), **out)


def _traced_ts_bias(T, me, boxes, cams):
    """The reference's estimate_ts_bias, unbound on ``me``, under a line tracer that reads its locals: the method keeps
    the entry list and time_error to itself.  It depends on the reference's local names x_offsets, i, j, time_error,
    EB_vel and WB_vel (MC3D_crop_tracker.py:260-303): if they are renamed there, rename them here.  -> (entries [e,4] i64 (cam1, cam2, i, j), time_error [e] f32, vel [2] f32)."""
    code = T.estimate_ts_bias.__code__
    got = {"ij": [], "te": np.zeros(0, np.float32), "vel": np.zeros(2, np.float32), "cams": []}

    def local(frame, event, arg):
        loc = frame.f_locals
        xo = loc.get("x_offsets")
        if xo is not None:
            while len(got["ij"]) < len(xo):                      # an append ran since the last line: i, j are still its own
                got["ij"].append((loc["i"], loc["j"]))
            if event == "return":
                got["cams"] = [(int(e[0]), int(e[1])) for e in xo]
                if "time_error" in loc:
                    got["te"] = t2n(loc["time_error"].float().reshape(-1))
                got["vel"] = np.array([float(loc["EB_vel"]), float(loc["WB_vel"])], dtype=np.float32)
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code is code else None
    sys.settrace(tracer)
    try:
        T.estimate_ts_bias(me, boxes, cams)
    finally:
        sys.settrace(None)
    ent = np.array([(c1, c2, i, j) for (c1, c2), (i, j) in zip(got["cams"], got["ij"])], dtype=np.int64).reshape(-1, 4)
    assert len(ent) == len(got["te"]) and len(got["cams"]) == len(got["ij"])
    return ent, got["te"], got["vel"]


def _ref_filter(kfmod, tc, objs):
    """The reference's Torch_KF holding the tracks objs [n,7] (x y l w h dir v)."""
    kf = kfmod.Torch_KF(torch.device("cpu"), INIT=tc.kf_init())
    if len(objs):
        o = torch.from_numpy(np.ascontiguousarray(objs))
        kf.add(o[:, :5].clone(), list(range(len(o))), o[:, 5].clone(), torch.zeros(len(o), dtype=torch.float64))
        kf.X[:, 5] = o[:, 6]
        assert np.array_equal(t2n(kf.view(with_direction=True)[1]), objs)
    return kf


def gen_ts_bias():
    """MC_Crop_Tracker.estimate_ts_bias (MC3D_crop_tracker.py:237-315) run unbound on a stand-in ``self`` (the reference's
    Torch_KF, a bare Homography_Wrapper, md_iou, timestamps, ts_bias, phi_nms_space, ts_alpha) on the scenes of
    tests/ts_bias_cases.py; the reference's parse_detections with est_ts=True and that method bound; and 8 frames of
    estimate_ts_bias -> space_nms -> association -> pruning in track()'s order on the reference's own filter.  Every
    case is checked here for the behaviour it is named after.  Outputs only."""
    import track_cases as tc
    import ts_bias_cases as tb
    trk, hgmod = import_reference_tracker()
    T = trk.MC_Crop_Tracker
    kfmod = ref_module_from_file("_reference_util_track_kf", "util_track/kf.py")
    bare = hgmod.Homography_Wrapper(hg1=hgmod.Homography(), hg2=hgmod.Homography())
    out = {}

    def stand_in(objs, timestamps, ts_bias, phi, hg=bare):
        me = types.SimpleNamespace(filter=_ref_filter(kfmod, tc, objs), hg=hg, timestamps=list(timestamps),
                                   ts_bias=list(ts_bias), phi_nms_space=phi, ts_alpha=tb.ALPHA)
        me.md_iou = types.MethodType(T.md_iou, me)
        return me
    for name, c in tb.cases().items():
        me = stand_in(c["objs"], c["timestamps"], c["ts_bias"], c["phi"])
        ent, te, vel = _traced_ts_bias(T, me, torch.from_numpy(c["boxes"]).clone(), torch.from_numpy(c["cams"]).clone())
        out[name + "_entries"], out[name + "_time_error"], out[name + "_vel"] = ent, te, vel
        out[name + "_ts_bias"] = np.array(me.ts_bias, dtype=np.float64)
        start = list(c["ts_bias"])
        assert all(float(np.float32(b)) == b for b, b0 in zip(me.ts_bias, start) if b != b0), name   # written biases are fp32 values
        if name == "overlap3":
            written, dependent = set(), False
            for c1, c2, _, _ in ent:
                dependent |= c1 != 0 and c2 in written
                written |= {c1} - {0}
            assert len(ent) >= 12 and dependent and set(ent[:, 0]) == {0, 1, 2} and me.ts_bias[0] == start[0]
            dirs = c["boxes"][ent[:, 2], 5]
            assert (dirs == 1).any() and (dirs == -1).any()
        elif name == "cam0_only":
            assert len(ent) >= 4 and all(0 in (c1, c2) for c1, c2, _, _ in ent) and me.ts_bias[0] == 0.0
            assert (ent[0::2, 0] == 0).any() and (ent[1::2, 0] == 0).any() and me.ts_bias[1] != start[1]
        elif name == "one_direction":
            assert vel[1] == -tb.MU_V and (c["boxes"][ent[:, 2], 5] == -1).any()
        elif name in ("same_camera", "no_tracks", "no_detections", "threshold_equal", "threshold_ulps_above"):
            assert len(ent) == 0 and me.ts_bias == start
        elif name in ("threshold", "threshold_ulps_below"):
            assert [tuple(e) for e in ent[:, 2:]] == [(0, 1), (0, 1)]
    c = tb.cases()["threshold"]                            # the reference's own md_iou puts the pairs where they are meant to be
    fp = torch.from_numpy(tb.footprints(c["boxes"])).double()
    iou = T.md_iou(stand_in(c["objs"], c["timestamps"], c["ts_bias"], c["phi"]), fp[[0, 2]][None], fp[[1, 3]][None]).reshape(-1)
    assert float(iou[0]) > tb.PHI > float(iou[1]) and float(iou[0]) - float(iou[1]) < 1e-5
    assert float(iou[0]) == tb.cases()["threshold_equal"]["phi"]
    # parse_detections with est_ts = True and the reference's own estimate_ts_bias bound
    scores, labels, boxes, cams, names, (Ps, Hs), (Ps2, Hs2) = gc.tracker_post_inputs()

    def make_hg(P, H):
        hg = hgmod.Homography()
        hg.correspondence = {n: {"P": P[i], "H": H[i], "H_inv": np.linalg.inv(H[i])} for i, n in enumerate(names)}
        hg.default_correspondence = names[0]
        return hg
    objs, ts, bias = tb.parse_scene()
    me = stand_in(objs, ts, bias, tb.PHI, hg=hgmod.Homography_Wrapper(hg1=make_hg(Ps, Hs), hg2=make_hg(Ps2, Hs2)))
    me.sigma_d, me.phi_nms_im, me.cameras, me.est_ts = 0.1, 0.3, list(names), True
    me.im_nms, me.space_nms = types.MethodType(T.im_nms, me), types.MethodType(T.space_nms, me)
    seen = {}

    def est(boxes_, cams_):
        seen["ent"], seen["te"], seen["vel"] = _traced_ts_bias(T, me, boxes_, cams_)
    me.estimate_ts_bias = est
    st, lb, sc, cm = T.parse_detections(me, scores.clone(), labels.clone(), boxes.clone(), cams.clone(), refine_height=True)
    k = "parse_est_ts_"
    out[k + "state"], out[k + "labels"], out[k + "scores"], out[k + "cams"] = t2n(st), t2n(lb), t2n(sc), t2n(cm)
    out[k + "entries"], out[k + "time_error"], out[k + "vel"] = seen["ent"], seen["te"], seen["vel"]
    out[k + "ts_bias"] = np.array(me.ts_bias, dtype=np.float64)
    assert len(seen["ent"]) >= 20 and me.ts_bias != list(bias)
    # the 8-frame sequence: MC3D_crop_tracker.py:373-381 in front of every frame of _run_sequence
    moved = [0]

    def parse_stage(trkr, key, detections, labels, scores, camera_idxs):
        before = list(trkr.ts_bias)
        ent, te, vel = _traced_ts_bias(T, trkr, detections.clone(), camera_idxs)
        moved[0] += trkr.ts_bias != before
        idxs = trkr.space_nms(detections, scores, threshold=trkr.phi_nms_space)
        out[key + "entries"], out[key + "time_error"], out[key + "vel"] = ent, te, vel
        out[key + "ts_bias"] = np.array(trkr.ts_bias, dtype=np.float64)
        out[key + "nms_idx"] = t2n(idxs).astype(np.int64)
        return detections[idxs], labels[idxs], scores[idxs], camera_idxs[idxs]
    _run_sequence(T, kfmod, tc, bare, tb.sequence(), tb.SEQ_TS_BIAS, out, before_frame=parse_stage,
                  attrs=dict(phi_nms_space=tb.PHI, ts_alpha=tb.ALPHA), methods=("space_nms",))
    moved = moved[0]
    assert moved >= 6, moved                                # the biases move from frame to frame
    np.savez_compressed(os.path.join(OUT, "ts_bias.npz"), **out)


def _script_iou(a, b):
    """The script's own iou (fit_filter_3D.py:30-61), restated: the file cannot be imported (it opens its dataset, its
    homography pickle and its checkpoint at import, :166-181)."""
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[2] - b[0]) * (b[3] - b[1])
    minx, maxx = max(a[0], b[0]), min(a[2], b[2])
    miny, maxy = max(a[1], b[1]), min(a[3], b[3])
    intersection = max(0, maxx - minx) * max(0, maxy - miny)
    union = area_a + area_b - intersection
    return intersection / union


def _script_moments(error_vectors):
    """:292-299 (and :377-384, :426-434, :471-478): torch.mean, then the serial fp32 sum of outer products."""
    k = error_vectors.shape[1]
    mean = torch.mean(error_vectors, dim=0)
    covariance = torch.zeros((k, k))
    for vec in error_vectors:
        covariance += torch.mm((vec - mean).unsqueeze(1), (vec - mean).unsqueeze(1).transpose(0, 1))
    return mean, covariance / error_vectors.shape[0]


def _script_footprint(hg, states):
    space = hg.state_to_space(states)
    box = torch.zeros([space.shape[0], 4])
    box[:, 0] = torch.min(space[:, 0:4, 0], dim=1)[0]
    box[:, 2] = torch.max(space[:, 0:4, 0], dim=1)[0]
    box[:, 1] = torch.min(space[:, 0:4, 1], dim=1)[0]
    box[:, 3] = torch.max(space[:, 0:4, 1], dim=1)[0]
    return box


def _script_nearest(hg, gt_state, detections):
    """:331-337 and :356-372 -> the chosen row or None."""
    gt_box = _script_footprint(hg, gt_state).squeeze(0)
    boxes_new = _script_footprint(hg, detections)
    min_dist, min_idx = np.inf, None
    for d_idx in range(len(boxes_new)):
        dist = 1.0 - _script_iou(boxes_new[d_idx], gt_box)
        if dist < min_dist:
            min_dist, min_idx = dist, d_idx
    return min_idx


def gen_fit_filter():
    """fit_filter_3D.py restated cell by cell (Q :242-304, R :306-389, class sizes :394-441, speed and P :444-485) around
    the reference's own Homography_Wrapper and Torch_KF, in the script's order and with its incremental add / predict
    loop, on the inputs of tests/fit_filter_cases.py.  The script's kf.add has no time argument and its kf.objs() is a
    dict by id (an older util_track/kf.py): here add gets zero times and the newest rows are read through obj_idxs, the
    rows the script's ids 0..3 name.  Arrays only."""
    import fit_filter_cases as fc
    matplotlib_stub()
    hgmod = ref_module_from_file("_reference_homography", "homography.py")
    kfmod = ref_module_from_file("_reference_util_track_kf", "util_track/kf.py")
    names, (Ps, Hs), (Ps2, Hs2) = fc.cameras()

    def make_hg(P, H):
        h = hgmod.Homography()
        h.correspondence = {n: {"P": P[i], "H": H[i], "H_inv": np.linalg.inv(H[i])} for i, n in enumerate(names)}
        h.default_correspondence = names[0]
        return h
    hg = hgmod.Homography_Wrapper(hg1=make_hg(Ps, Hs), hg2=make_hg(Ps2, Hs2))
    class_dict = {i: n for i, n in enumerate(fc.CLASS_NAMES)}
    out = {}

    def to_state(gt_im, classes, camera):                                   # :262-266
        heights = hg.guess_heights(classes)
        temp_boxes = hg.im_to_state(gt_im, heights=heights, name=camera)
        repro_boxes = hg.state_to_im(temp_boxes, name=camera)
        refined_heights = hg.height_from_template(repro_boxes, heights, gt_im)
        return hg.im_to_state(gt_im, heights=refined_heights, name=camera)

    # ---- Q
    kf_params = fc.kf_params()
    kf = kfmod.Torch_KF(torch.device("cpu"), INIT=kf_params)
    tr, tr_cls, tr_cam = fc.tracklets()
    tr_t = torch.from_numpy(tr)
    errors, preds, tgts, states = [], [], [], []
    for idx in range(len(tr) // 4):
        targets = []
        for b_idx in range(4):
            k = idx * 4 + b_idx
            gt_im = tr_t[k]
            classes = [class_dict[int(tr_cls[k])]] * 3
            gt_state = to_state(gt_im, classes, names[tr_cam[k]])
            states.append(gt_state)
            vel = (gt_state[1, 0] - gt_state[0, 0]) * 30
            init_state = torch.cat((gt_state[0, :5].unsqueeze(0), vel.unsqueeze(0).unsqueeze(1)), dim=1)
            direction = gt_state[0, 5].unsqueeze(0)
            kf.add(init_state, [b_idx], direction, torch.zeros(1, dtype=torch.float64))
            vel = (gt_state[2, 0] - gt_state[1, 0]) * 30
            targets.append(torch.cat((gt_state[1, :5].unsqueeze(0), vel.unsqueeze(0).unsqueeze(1)), dim=1).squeeze(0))
        kf.predict()
        pred = torch.stack([kf.X[kf.obj_idxs[i]].clone() for i in kf.obj_idxs.keys()])
        targets = torch.stack(targets)
        errors.append(pred - targets)
        preds.append(pred)
        tgts.append(targets)
    error_vectors = torch.cat(errors, dim=0)
    mean, covariance = _script_moments(error_vectors)
    out["q_states"] = t2n(torch.stack(states))
    out["q_pred"], out["q_target"], out["q_errors"] = t2n(torch.cat(preds)), t2n(torch.cat(tgts)), t2n(error_vectors)
    out["mu_Q"], out["Q"] = t2n(mean), t2n(covariance)
    kf_params["mu_Q"], kf_params["Q"] = mean, covariance
    assert abs(float(mean[5])) > 0.05 and len(kf.X) == len(tr)

    # ---- R
    gt_im_all, gt_cls, cam, scores, labels, boxes20, offsets = fc.detector_frames()
    errors, rows, gt_states, det_states = [], [], [], []
    for b in range(len(gt_im_all)):
        camera = names[cam[b]]
        gt_state = to_state(torch.from_numpy(gt_im_all[b]), [class_dict[int(gt_cls[b])]], camera)
        gt_states.append(gt_state[0])
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        if hi - lo == 0:                                                      # :343-344
            rows.append(-1)
            continue
        detections = torch.from_numpy(boxes20[lo:hi]).reshape(-1, 10, 2)
        detections = detections[:, :8, :]
        detections = to_state(detections, [class_dict[int(l)] for l in labels[lo:hi]], camera)      # :349-354
        det_states.append(detections)
        d_idx = _script_nearest(hg, gt_state, detections)
        assert d_idx is not None
        rows.append(lo + d_idx)
        error = detections[d_idx] - gt_state
        errors.append(error[0, :5])
    error_vectors = torch.stack(errors)
    mean, covariance = _script_moments(error_vectors)
    out["r_gt_states"], out["r_det_states"] = t2n(torch.stack(gt_states)), t2n(torch.cat(det_states))
    out["r_rows"], out["r_errors"] = np.array(rows, dtype=np.int32), t2n(error_vectors)
    out["mu_R"], out["R"] = t2n(mean), t2n(covariance)
    kf_params["mu_R"], kf_params["R"] = mean, covariance

    # ---- class sizes (:394-441): every frame of a tracklet under the tracklet's first class
    means = {}
    for k in range(len(tr)):
        means.setdefault(class_dict[int(tr_cls[k])], []).append(states[k])
    class_sizes, class_covariances = {}, {}
    for key in means.keys():
        vecs = torch.cat(means[key], dim=0)[:, 2:5]
        class_sizes[key], class_covariances[key] = _script_moments(vecs)
    assert sorted(class_sizes) == sorted(fc.CLASS_NAMES)
    out["class_size"] = np.stack([t2n(class_sizes[n]) for n in fc.CLASS_NAMES])
    out["class_covariance"] = np.stack([t2n(class_covariances[n]) for n in fc.CLASS_NAMES])
    kf_params["class_size"], kf_params["class_covariance"] = class_sizes, class_covariances

    # ---- mean speed and P (:444-485)
    vecs = []
    for gt_state in states:
        vel = torch.abs(gt_state[-1, 0] - gt_state[0, 0]) / ((len(gt_state) - 1) / 30.0)
        vecs.append(vel.clone().unsqueeze(0))
    vecs = torch.cat(vecs, dim=0).unsqueeze(1)
    mean, covariance = _script_moments(vecs)
    out["speeds"] = t2n(vecs)
    kf_params["P"] = torch.zeros([6, 6]).float()
    kf_params["mu_v"] = mean
    kf_params["P"][:5, :5] = kf_params["R"]
    kf_params["P"][5, 5] = covariance.item()
    out["mu_v"], out["var_v"], out["P"] = t2n(mean), t2n(covariance), t2n(kf_params["P"])

    # ---- the operator-level cases of the nearest-box search, through the script's loop
    bare = hgmod.Homography_Wrapper(hg1=hgmod.Homography(), hg2=hgmod.Homography())
    for name, (gt, det, off) in fc.nearest_cases().items():
        rows, resid = [], []
        for b in range(len(gt)):
            lo, hi = int(off[b]), int(off[b + 1])
            g = torch.from_numpy(gt[b:b + 1])
            d = torch.from_numpy(det[lo:hi])
            d_idx = _script_nearest(bare, g, d) if hi > lo else None
            rows.append(-1 if d_idx is None else lo + d_idx)
            if d_idx is not None:
                resid.append((d[d_idx] - g)[0, :5])
        out["nearest_%s_rows" % name] = np.array(rows, dtype=np.int32)
        out["nearest_%s_resid" % name] = t2n(torch.stack(resid))
    assert list(out["nearest_ties_rows"]) == [0, 70 + 3, 140 + 1] and list(out["nearest_nan_rows"]) == [1, -1, 4, -1]

    # ---- a filter built from the fitted dict: add with class sizes and the mean speed, predict, update
    st, classes, z = fc.filter_probe()
    kf = kfmod.Torch_KF(torch.device("cpu"), INIT=kf_params)
    s = torch.from_numpy(st)
    kf.add(s[:, :5].clone(), list(range(len(s))), s[:, 5].clone(), torch.zeros(len(s), dtype=torch.float64),
           init_speed=True, classes=classes)
    out["probe_X0"], out["probe_P0"] = t2n(kf.X.clone()), t2n(kf.P.clone())
    kf.predict()
    out["probe_X1"], out["probe_P1"] = t2n(kf.X.clone()), t2n(kf.P.clone())
    kf.update(torch.from_numpy(z), list(range(len(s))))
    out["probe_X2"], out["probe_P2"] = t2n(kf.X.clone()), t2n(kf.P.clone())
    np.savez_compressed(os.path.join(OUT, "fit_filter.npz"), **out)


class _EvalItem(dict):
    """What csv_eval._get_detections reads of a dataset item: data[0] (CHW, its GPU branch) or data['img'] (HWC, its CPU
    branch).  Pixel (0,0) of channel 0 carries the image index."""
    def __getitem__(self, k):
        return dict.__getitem__(self, "chw" if k == 0 else k)


class _EvalDataset:
    def __init__(self, anns, C):
        self.anns, self.C = anns, C

    def __len__(self):
        return len(self.anns)

    def num_classes(self):
        return self.C

    def __getitem__(self, i):
        chw = torch.zeros(3, 2, 2)
        chw[0, 0, 0] = float(i)
        return _EvalItem(chw=chw, img=chw.permute(1, 2, 0))

    def load_annotations(self, i):
        return self.anns[i]

    def label_to_name(self, label):
        return "class%d" % label


class _EvalNet:
    """Returns the stored detections of the image whose index the input carries."""
    def __init__(self, dets):
        self.dets = dets

    def eval(self):
        return self

    def __call__(self, x):
        s, l, b = self.dets[int(round(float(x[0, 0, 0, 0])))]
        return torch.from_numpy(s.copy()), torch.from_numpy(l.copy()), torch.from_numpy(b.copy())


def gen_csv_eval():
    """The reference's own csv_eval.evaluate (retinanet/csv_eval.py) on the stub dataset and network above."""
    import contextlib
    import io
    import eval_cases as ec
    ce = ref_module_from_file("ref_csv_eval", "retinanet/csv_eval.py")
    out = {}
    for name, g in ec.GOLDEN.items():
        dets, anns = ec.golden_inputs(name)
        C = g["classes"]
        with contextlib.redirect_stdout(io.StringIO()):
            res = ce.evaluate(_EvalDataset(anns, C), _EvalNet(dets), iou_threshold=g["iou"], score_threshold=g["score"],
                              max_detections=g["max_det"])
        for k, v in ec.pack_golden(dets, anns, C).items():
            out[name + "_" + k] = v
        out[name + "_params"] = np.array([g["iou"], g["score"], g["max_det"]], np.float64)
        out[name + "_ap"] = np.array([float(res[c][0]) for c in range(C)], np.float64)
        out[name + "_num_annotations"] = np.array([float(res[c][1]) for c in range(C)], np.float64)
    np.savez_compressed(os.path.join(OUT, "csv_eval.npz"), **out)


# ----------------------------------------------------------------------------- training-batch augmentation
class _Recorder:
    """Wraps np.random.normal / rand / randint and torch.rand for one __getitem__: what was drawn, in order."""
    def __init__(self):
        self.np_draws, self.randints, self.noise = [], [], []

    def __enter__(self):
        self.saved = (np.random.normal, np.random.rand, np.random.randint, torch.rand)

        def wrap(fn, kind):
            def inner(*a, **k):
                v = fn(*a, **k)
                self.np_draws.append(float(v))
                if kind == "randint":
                    self.randints.append((int(a[1]), int(v)))
                return v
            return inner

        def rand(*a, **k):
            v = self.saved[3](*a, **k)
            if v.dim() == 3:
                self.noise.append(v.clone())
            return v
        np.random.normal, np.random.rand = wrap(self.saved[0], "normal"), wrap(self.saved[1], "rand")
        np.random.randint, torch.rand = wrap(self.saved[2], "randint"), rand
        return self

    def __exit__(self, *exc):
        np.random.normal, np.random.rand, np.random.randint, torch.rand = self.saved


def augment_reference_dataset(tmp, cases, shapes=None, crop=0):
    """A temporary dataset in the reference's own format (PNG frames, labels.cpkl, camera_vps.cpkl) for the cases of
    tests/augment_cases.py (name, shape key, camera, boxes, seed), read by the reference's own Detection_Dataset.
    -> {name: (dataset, index)}"""
    import pickle
    import random
    from PIL import Image
    import augment_cases as ac
    import tv_pillow_stub
    tv_pillow_stub.install()
    ref = ref_module_from_file("_reference_corrected_3D_dataset", "corrected_3D_dataset.py")
    os.makedirs(os.path.join(tmp, "frames"), exist_ok=True)
    all_data, by_path = [], {}
    for i, (name, shape, camera, kind, seed) in enumerate(cases):
        W, H = (shapes or ac.SHAPES)[shape]
        path = os.path.join(tmp, "frames", "%s_0_%d.png" % (camera, i))
        Image.fromarray(ac.frame_bytes(name, W, H)).save(path)
        all_data.append([path, ac.boxes_rows(name, kind, W, H)])
        by_path[path] = (name, kind)
    with open(os.path.join(tmp, "labels.cpkl"), "wb") as f:
        pickle.dump(all_data, f)
    with open(os.path.join(tmp, "camera_vps.cpkl"), "wb") as f:
        pickle.dump(ac.VPS, f)
    found, cwd = {}, os.getcwd()
    os.chdir(tmp)                                             # the reference opens camera_vps.cpkl in the working directory
    try:
        for mode in ("train", "test"):                        # the two sides of its 90/10 split, from the same shuffle
            random.seed(0)
            ds = ref.Detection_Dataset(tmp, mode=mode, CROP=crop)
            for idx, path in enumerate(ds.data):
                name, kind = by_path[path]
                if kind == "empty":                           # a frame whose label tensor is empty: the no_labels path (:311-313)
                    ds.labels[idx] = torch.zeros([0, 21], dtype=torch.float64)
                found[name] = (ds, idx)
    finally:
        os.chdir(cwd)
    assert len(found) == len(cases)
    return ref, found


def augment_reference_item(ds, idx, seed):
    """The reference's __getitem__ under seeds, with every draw and every intermediate image recorded."""
    import random
    from PIL import Image
    import augment_cases as ac
    import tv_pillow_stub
    np.random.seed(seed)
    torch.manual_seed(seed)
    random.seed(seed)
    del tv_pillow_stub.LOG[:]
    with _Recorder() as rec:
        im_t, y = ds[idx]
    log = list(tv_pillow_stub.LOG)
    first = {}
    for k, v in log:
        first.setdefault(k, v)
    H, W = im_t.shape[1:]
    camera = ds.data[idx].split("/")[-1].split("_")[0]
    d = rec.np_draws
    scale, aspect, flip, angle, tile = max(1, d[0]), max(0.75, d[1]), d[2], d[3] * 40 - 20, d[4]
    assert first["rotate"][0] == angle and len(rec.noise) == 1 and ("hflip" in first) == (flip > 0.5)
    xs = [v for hi, v in rec.randints if hi == W]
    ys = [v for hi, v in rec.randints if hi == H]
    dx = xs[-1] if 0.25 < tile < 0.75 else 0
    dy = ys[-1] if tile > 0.5 and tile != 0.75 else 0
    (rh, rw), resized = first["resize"]
    apply = first["apply"]
    order, factors = first["jitter"] if apply else ([0, 1, 2, 3], [1.0, 1.0, 1.0])
    steps = [v for k, v in log if k == "jitter_step"]
    out = dict(frame=np.array(Image.open(ds.data[idx])), labels_in=t2n(ds.labels[idx]),
               camera=np.array(camera), vps=np.array(ac.VPS[camera], np.float64), seed=np.array(seed),
               np_draws=np.array(d, np.float64), xsplits=np.array(xs, np.int64), ysplits=np.array(ys, np.int64),
               scalars=np.array([scale, aspect, angle, tile], np.float64),
               draws=np.array([rh, rw, int(flip > 0.5), apply, dy, dx], np.int32),
               order=np.array(order, np.int32), factors=np.array(factors, np.float64),
               noise=ac.noise_bytes(t2n(rec.noise[0]).transpose(1, 2, 0)), resized=resized, padded=first["to_pil_image"],
               rotated=first["rotate"][1],
               jitter_steps=np.stack(steps) if steps else np.zeros((0, H, W, 3), np.uint8),
               im_t=t2n(im_t), y=t2n(y))
    assert np.array_equal(first["to_tensor"], steps[-1] if steps else out["rotated"])
    return out


def augment_features(name, kind, camera, o):
    """What one golden item covers of the list the set must contain."""
    rh, rw, flip, apply, dy, dx = (int(v) for v in o["draws"])
    scale, aspect, angle, tile = o["scalars"]
    f = {"flip%d" % flip, "tile_none" if tile <= 0.25 else "tile_x" if tile < 0.5 else "tile_xy" if tile < 0.75 else "tile_y",
         "aspect_below_1" if aspect < 1 else "aspect_above_1", "jitter_applied" if apply else "jitter_skipped"}
    if (0.25 < tile < 0.75 and dx == 0) or (tile > 0.5 and dy == 0):
        f.add("split_at_0")
    if scale == 1:
        f.add("scale_1")
    if apply:
        f.add("order_" + "".join(str(v) for v in o["order"]))
    if kind == "empty":
        f.add("label_less")
        if flip:
            f.add("label_less_flipped")
    if kind == "none":
        f.add("zero_row")
    if kind == "corner" and o["y"][0, 20] == -1:
        f.add("rotated_out")
    if camera == "p2c3":
        f.add("p2c3")
    return f


AUGMENT_MUST_COVER = {"flip0", "flip1", "tile_none", "tile_x", "tile_xy", "tile_y", "split_at_0", "aspect_below_1",
                      "aspect_above_1", "scale_1", "jitter_applied", "jitter_skipped", "label_less", "label_less_flipped",
                      "zero_row", "rotated_out", "p2c3"}


def gen_augment():
    """The reference's own Detection_Dataset.__getitem__ and collate (corrected_3D_dataset.py:296-498, 714-741, CROP == 0) on a
    temporary dataset, behind tools/tv_pillow_stub.py and an empty cv2; the inputs, every draw, the noise, the bytes at every
    step, im_t and y of every case of tests/augment_cases.py."""
    import tempfile
    import augment_cases as ac
    out, covered, items = {}, set(), {}
    with tempfile.TemporaryDirectory() as tmp:
        ref, found = augment_reference_dataset(tmp, ac.GOLDEN)
        for name, shape, camera, kind, seed in ac.GOLDEN:
            o = augment_reference_item(*found[name], seed)
            covered |= augment_features(name, kind, camera, o)
            items[name] = o
            for k, v in o.items():
                out["%s_%s" % (name, k)] = v
    assert AUGMENT_MUST_COVER <= covered, AUGMENT_MUST_COVER - covered
    assert len([c for c in covered if c.startswith("order_")]) >= 3, covered
    for shape in ac.SHAPES:
        names = [c[0] for c in ac.GOLDEN if c[1] == shape]
        ims, ys = ref.collate([(torch.from_numpy(items[n]["im_t"]), torch.from_numpy(items[n]["y"])) for n in names])
        assert len({len(items[n]["y"]) for n in names}) > 1 and np.array_equal(t2n(ims), np.stack([items[n]["im_t"] for n in names]))
        out["collate_%s_y" % shape] = t2n(ys)
    out["names"] = np.array([c[0] for c in ac.GOLDEN])
    np.savez_compressed(os.path.join(OUT, "augment.npz"), **out)


# ----------------------------------------------------------------------------- crop-detector training batches
class _CropRecorder(_Recorder):
    """... and np.random.normal(size=2) (an array: both values, in order) and torch.normal (the occlusion's values)."""
    def __enter__(self):
        _Recorder.__enter__(self)
        self.normals, self.saved_normal, normal = [], torch.normal, np.random.normal
        np_draws = self.np_draws

        def np_normal(*a, **k):
            if "size" not in k:
                return normal(*a, **k)
            v = self.saved[0](*a, **k)                    # the unwrapped function: the wrapper cannot take an array
            np_draws.extend(float(x) for x in v)
            return v

        def np_randint(*a, **k):                          # one argument or two, floats among them: as they are passed
            v = self.saved[2](*a, **k)
            np_draws.append(float(v))
            return v

        def t_normal(*a, **k):
            v = self.saved_normal(*a, **k)
            self.normals.append(v.clone())
            return v
        np.random.normal, np.random.randint, torch.normal = np_normal, np_randint, t_normal
        return self

    def __exit__(self, *exc):
        _Recorder.__exit__(self, *exc)
        torch.normal = self.saved_normal


def augment_crop_reference_item(ds, idx, seed, cs):
    """The reference's __getitem__ with CROP = cs under seeds: every draw, the locals that place the window, every
    intermediate image of the crop branch, the occlusion's region and values, im_t and y."""
    import random
    from PIL import Image
    import augment_cases as ac
    import tv_pillow_stub
    np.random.seed(seed)
    torch.manual_seed(seed)
    random.seed(seed)
    del tv_pillow_stub.LOG[:]
    ds.CROP = cs
    seen = {}

    def profile(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "__getitem__" and "centx" in frame.f_locals:
            seen.update(frame.f_locals)
    with _CropRecorder() as rec:
        sys.setprofile(profile)
        try:
            im_t, y = ds[idx]
        finally:
            sys.setprofile(None)
    log = list(tv_pillow_stub.LOG)
    first = {}
    for k, v in log:
        first.setdefault(k, v)
    camera = ds.data[idx].split("/")[-1].split("_")[0]
    frame = np.array(Image.open(ds.data[idx]))
    H, W = frame.shape[:2]
    d = rec.np_draws
    scale, aspect, flip, angle = max(1, d[0]), max(0.75, d[1]), d[2], d[3] * 40 - 20
    assert first["rotate"][0] == angle and len(rec.noise) == 1 and ("hflip" in first) == (flip > 0.5)
    resizes = [v for k, v in log if k == "resize"]
    assert len(resizes) == 2 and resizes[1][0] == (cs, cs)
    (rh, rw), _ = resizes[0]
    win, cropped = first["crop"]
    assert win == (seen["minx"], seen["miny"], seen["maxx"] - seen["minx"], seen["maxy"] - seen["miny"])
    apply = first["apply"]
    order, factors = first["jitter"] if apply else ([0, 1, 2, 3], [1.0, 1.0, 1.0])
    steps = [v for k, v in log if k == "jitter_step"]
    occlude_draw = float(seen["OCCLUDE"])
    occluded = occlude_draw > 0.9
    region, values = (0, 0, 0, 0), np.zeros((3, cs, cs), np.float32)
    assert len(rec.normals) == (3 if occluded else 0)
    if occluded:
        region = tuple(int(v) for v in seen["region"])
        x0, y0, x1, y1 = region
        values[:, y0:y1, x0:x1] = t2n(torch.stack(rec.normals))
        assert np.array_equal(t2n(im_t)[:, y0:y1, x0:x1], values[:, y0:y1, x0:x1])
    out = dict(frame=frame, labels_in=t2n(ds.labels[idx]), camera=np.array(camera), vps=np.array(ac.VPS[camera], np.float64),
               seed=np.array(seed), cs=np.array(cs), np_draws=np.array(d, np.float64),
               scalars=np.array([scale, aspect, angle, occlude_draw], np.float64),
               draws=np.array([rh, rw, int(flip > 0.5), apply, int(occluded)], np.int32),
               order=np.array(order, np.int32), factors=np.array(factors, np.float64),
               noise=ac.noise_bytes(t2n(rec.noise[0]).transpose(1, 2, 0)),
               center=np.array([float(seen["centx"]), float(seen["centy"])], np.float64), size=np.array(float(seen["size"]), np.float64),
               win=np.array(win, np.int64), window=cropped, second=resizes[1][1],
               jitter_steps=np.stack(steps) if steps else np.zeros((0, cs, cs, 3), np.uint8),
               region=np.array(region, np.int64), occlusion=values, im_t=t2n(im_t), y=t2n(y))
    assert np.array_equal(first["to_tensor"], steps[-1] if steps else out["second"])
    return out


def augment_crop_features(name, kind, camera, o):
    """What one golden item covers of the list the set must contain."""
    rh, rw, flip, apply, occluded = (int(v) for v in o["draws"])
    H, W = o["frame"].shape[:2]
    minx, miny, cw, ch = (int(v) for v in o["win"])
    cs = int(o["cs"])
    f = {"flip%d" % flip, "jitter_applied" if apply else "jitter_skipped", "occluded" if occluded else "not_occluded"}
    overlaps = minx < W and minx + cw > 0 and miny < H and miny + ch > 0
    if not overlaps:
        f.add("outside")
    elif minx >= 0 and miny >= 0 and minx + cw <= W and miny + ch <= H:
        f.add("inside")
    else:
        f |= {n for n, c in (("left", minx < 0), ("top", miny < 0), ("right", minx + cw > W), ("bottom", miny + ch > H)) if c}
    if cw != ch:
        f.add("non_square")
    if max(cw, ch) / cs > 3:
        f.add("shrink_above_3")
        if o["window"].any():
            f.add("shrink_above_3_of_content")
    if max(cw, ch) < cs:
        f.add("enlargement")
    if minx < 0 or miny < 0:
        f.add("negative_origin")
    if rh < H and overlaps and miny + ch > rh and o["window"].any():
        f.add("pad_noise")
    if kind == "empty":
        f.add("label_less_flipped" if flip else "label_less")
    if kind == "none":
        f.add("zero_row")
    n_in = len(o["labels_in"])
    kept = 0 if o["y"][0, 0] == -1 and o["y"][0, 20] == -1 else len(o["y"])
    if kind not in ("empty", "none") and 0 < kept < n_in:
        f.add("box_removed")
    if kind not in ("empty", "none") and kept == 0:
        f.add("all_removed")
    if o["y"].dtype == np.float64:
        f.add("y_fp64")
        if cw != ch:
            f.add("kept_in_non_square")
    else:
        f.add("y_fp32")
    if camera == "p2c3":
        f.add("p2c3")
    return f


AUGMENT_CROP_MUST_COVER = {"flip0", "flip1", "inside", "left", "top", "right", "bottom", "outside", "non_square", "shrink_above_3",
                           "enlargement", "pad_noise", "label_less", "label_less_flipped", "zero_row", "box_removed", "all_removed",
                           "jitter_applied", "jitter_skipped", "occluded", "not_occluded", "p2c3", "negative_origin", "y_fp64",
                           "y_fp32", "shrink_above_3_of_content", "kept_in_non_square"}


def gen_augment_crop():
    """The reference's own Detection_Dataset.__getitem__ with CROP > 0 and collate (corrected_3D_dataset.py:296-402, 501-594,
    714-741) on a temporary dataset, behind tools/tv_pillow_stub.py: the inputs, every draw, the window, the bytes at every
    step of the crop branch, the occlusion, im_t and y of every case of tests/augment_crop_cases.py."""
    import tempfile
    import augment_crop_cases as cc
    out, covered, items = {}, set(), {}
    with tempfile.TemporaryDirectory() as tmp:
        ref, found = augment_reference_dataset(tmp, [cc.case_golden(c) for c in cc.GOLDEN], cc.SHAPES, crop=24)
        for name, shape, camera, kind, seed, cs in cc.GOLDEN:
            o = augment_crop_reference_item(*found[name], seed, cs)
            covered |= augment_crop_features(name, kind, camera, o)
            items[name] = o
            for k, v in o.items():
                out["%s_%s" % (name, k)] = v
    assert AUGMENT_CROP_MUST_COVER <= covered, AUGMENT_CROP_MUST_COVER - covered
    for shape, cs in sorted({(c[1], c[5]) for c in cc.GOLDEN}):
        names = [c[0] for c in cc.GOLDEN if (c[1], c[5]) == (shape, cs)]
        ims, ys = ref.collate([(torch.from_numpy(items[n]["im_t"]), torch.from_numpy(items[n]["y"])) for n in names])
        assert np.array_equal(t2n(ims), np.stack([items[n]["im_t"] for n in names]))
        out["collate_%s%d_y" % (shape, cs)] = t2n(ys)
    out["names"] = np.array([c[0] for c in cc.GOLDEN])
    np.savez_compressed(os.path.join(OUT, "augment_crop.npz"), **out)

# ----------------------------------------------------------------------------- tracking evaluation (MOT metrics)
MOT_FRAMES = 100                    # the result files are cut to frames below this (959 frames, ~7 rows each, in full)
# name -> (prediction file, match_iou, cutoff_frame).  The 100-frame cases pin the restatement and feed the staged
# comparison; the trackers drift apart after the first frames (most pairs stop overlapping and scipy's tie rule decides),
# so the end-to-end comparison, which needs frames that stay decided under a last-bit change of the IoU, runs on the
# "_first" cases: the longest prefixes in which every frame is stable (tests/test_mot_eval_host.py asserts it).
MOT_CASES = {"p20_iou0": ("pred20", 0, MOT_FRAMES), "p20_iou51": ("pred20", 0.51, MOT_FRAMES),
             "p90_iou0": ("pred90", 0, MOT_FRAMES), "p90_iou51": ("pred90", 0.51, MOT_FRAMES),
             "p20_iou0_first": ("pred20", 0, 9), "p20_iou51_first": ("pred20", 0.51, 9),
             "p90_iou0_first": ("pred90", 0, 5), "p90_iou51_first": ("pred90", 0.51, 5)}


def _fit_projective(src, dst):
    """The [3, k+1] matrix M with dst ~ M [src; 1] (k = 2: a plane homography, k = 3: a camera matrix): normalised DLT on
    the normal equations.  Only elementwise numpy sums and a symmetric 9x9 / 12x12 eigenproblem, and the result is
    rounded to 15 digits, so that it regenerates bit for bit."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)

    def norm(x):
        T = np.eye(x.shape[1] + 1)
        s = float(np.round(x.std(0).mean(), 3))
        T[:-1, :-1] /= s
        T[:-1, -1] = -np.round(x.mean(0), 3) / s
        return T
    Ts, Td = norm(src), norm(dst)
    s = (Ts[None] * np.concatenate((src, np.ones((len(src), 1))), 1)[:, None, :]).sum(2)
    d = (Td[None] * np.concatenate((dst, np.ones((len(dst), 1))), 1)[:, None, :]).sum(2)
    z = np.zeros_like(s)
    A = np.concatenate((np.concatenate((s, z, -d[:, 0:1] * s), 1), np.concatenate((z, s, -d[:, 1:2] * s), 1)), 0)
    N = (A[:, :, None] * A[:, None, :]).sum(0)
    w, v = np.linalg.eigh((N + N.T) / 2)
    M = np.linalg.inv(Td) @ v[:, 0].reshape(3, -1) @ Ts
    M = M / M[2, -1]
    return np.array([[float("%.14e" % x) for x in row] for row in M])


def _fit_camera(rows):
    """H (image -> road plane) and P (space -> image) of the camera that wrote the result file, from the file's own state
    and image-corner columns.  The matrices of the homography fixture are synthetic: through them the file's image
    corners land nowhere near its states and nothing overlaps."""
    from oracle import homography as ohg
    st = np.array([[r[c] for c in (39, 40, 43, 42, 44, 35)] for r in rows]).astype(float).astype(np.float32)
    im = np.array([r[11:27] for r in rows]).astype(float).reshape(-1, 8, 2)
    sp = ohg.state_to_space(st).astype(np.float64)
    P = _fit_projective(sp.reshape(-1, 3), im.reshape(-1, 2))
    H = _fit_projective(im[:, 0:4].reshape(-1, 2), sp[:, 0:4, 0:2].reshape(-1, 2))
    assert np.abs(ohg.state_to_im(st, P) - im).max() < 0.05                                    # px; the file keeps fp32 states
    assert np.abs(ohg.im_to_space(im, H, np.zeros(len(im)))[:, 0:4, 0:2] - sp[:, 0:4, 0:2]).max() < 1e-3     # ft
    return H, P


def _cut_csv(fn, frames):
    """The header line and the rows of the first frames of one of the reference's result files, as bytes."""
    keep = []
    with open(os.path.join(REF, fn), newline="") as f:
        for k, line in enumerate(f):
            if k == 0 or (line.strip() and int(line.split(",", 1)[0]) < frames):
                keep.append(line)
    return np.frombuffer("".join(keep).encode(), np.uint8)


def gen_mot_eval():
    """The reference's MOT_Evaluator.evaluate on its own result files (data): 3D_tracking_results.csv as the ground truth
    against the _20 and _90 files, cut to their first frames, through a Homography holding the camera fitted to the
    ground-truth file itself (_fit_camera).  scipy's solver is wrapped to record each frame's IoU matrix and assignment."""
    import contextlib
    import io
    import tempfile
    for k in [k for k in sys.modules if k == "homography"]:
        del sys.modules[k]
    sys.path.insert(0, REF)
    try:
        hgmod = importlib.import_module("homography")
        ev_mod = ref_module_from_file("ref_mot_evaluator", "mot_evaluator.py")
    finally:
        sys.path.remove(REF)
    assert os.path.realpath(hgmod.__file__).startswith(os.path.realpath(REF) + os.sep)
    del sys.modules["homography"]
    hg = hgmod.Homography()
    out = {}
    files = {"gt": "3D_tracking_results.csv", "pred20": "3D_tracking_results_20.csv", "pred90": "3D_tracking_results_90.csv"}
    solve = ev_mod.linear_sum_assignment
    with tempfile.TemporaryDirectory() as tmp:
        for key, fn in files.items():
            out[key + "_csv"] = _cut_csv(fn, MOT_FRAMES)
            with open(os.path.join(tmp, key + ".csv"), "wb") as f:
                f.write(out[key + "_csv"].tobytes())
        gt_rows = [r for rows in hgmod.load_i24_csv(os.path.join(tmp, "gt.csv"))[1].values() for r in rows]
        H, P = _fit_camera(gt_rows)
        hg.correspondence = {gt_rows[0][36]: {"P": P, "H": H, "H_inv": np.linalg.inv(H)}}
        hg.default_correspondence = gt_rows[0][36]
        out["P"], out["H"] = P, H
        for case, (pkey, thr, frames) in MOT_CASES.items():
            rec = []

            def recording(ious, maximize=False):
                a, b = solve(ious, maximize=maximize)
                rec.append((ious.copy(), a.copy(), b.copy()))
                return a, b
            ev_mod.linear_sum_assignment = recording
            ev = ev_mod.MOT_Evaluator(os.path.join(tmp, "gt.csv"), os.path.join(tmp, pkey + ".csv"), hg,
                                      params={"match_iou": thr, "cutoff_frame": frames})
            text = io.StringIO()
            raised = False
            with contextlib.redirect_stdout(text):
                try:
                    ev.evaluate()
                except ZeroDivisionError:                   # TP = 0 (:360): the bookkeeping in ev.m is complete by then
                    raised = True
            ev_mod.linear_sum_assignment = solve
            out[case + "_raises_zero_division"] = np.array(raised)
            both = [f for f in range(frames) if f in ev.gt and f in ev.pred]
            assert len(both) == len(rec)
            out[case + "_iou_frames"] = np.array([[f, r[0].shape[0], r[0].shape[1]] for f, r in zip(both, rec)], np.int64)
            out[case + "_iou"] = np.concatenate([r[0].reshape(-1) for r in rec])
            out[case + "_assign"] = np.array([[f, i, j] for f, r in zip(both, rec) for i, j in zip(r[1], r[2])], np.int64)
            m = ev.m
            out[case + "_pre_thresh_iou"] = np.array(m["pre_thresh_IOU"], np.float64)
            out[case + "_match_iou"] = np.array(m["match_IOU"], np.float64)
            out[case + "_counters"] = np.array([m[k] for k in ("TP", "FP", "FN", "FP edge-case", "FP @ 0.2", "FN @ 0.2")], np.int64)
            out[case + "_state_err"] = torch.stack(m["state_err"]).numpy() if m["state_err"] else np.zeros((0, 7), np.float32)
            out[case + "_bot_err"] = torch.stack(m["im_bot_err"]).numpy() if m["im_bot_err"] else np.zeros(0, np.float64)
            out[case + "_top_err"] = torch.stack(m["im_top_err"]).numpy() if m["im_top_err"] else np.zeros(0, np.float64)
            assert out[case + "_state_err"].dtype == np.float32 and out[case + "_bot_err"].dtype == np.float64
            out[case + "_ids"] = np.array([[g, p] for g, v in m["ids"].items() for p in v], np.int64).reshape(-1, 2)
            out[case + "_gt_ids"] = np.array(m["gt_ids"], np.int64)
            out[case + "_pred_ids"] = np.array(m["pred_ids"], np.int64)
            out[case + "_confusion"] = np.asarray(m["cls"], np.int64)
            if raised:
                continue
            scalar = [k for k, v in ev.metrics.items() if not isinstance(v, tuple)]
            pair = [k for k, v in ev.metrics.items() if isinstance(v, tuple)]
            out[case + "_metric_names"] = np.array(scalar)
            out[case + "_metric_values"] = np.array([float(ev.metrics[k]) for k in scalar], np.float64)
            out[case + "_figure_names"] = np.array(pair)
            out[case + "_figure_values"] = np.array([[float(ev.metrics[k][0]), float(ev.metrics[k][1])] for k in pair], np.float64)
            out[case + "_figure_is_f32"] = np.array([isinstance(ev.metrics[k][0], torch.Tensor) and ev.metrics[k][0].dtype == torch.float32
                                                    for k in pair])
            table = text.getvalue()
            out[case + "_table"] = np.frombuffer(table[table.index("\n\n"):].encode(), np.uint8)
    np.savez_compressed(os.path.join(OUT, "mot_eval.npz"), **out)


def gen_calibration():
    """The reference's own find_vanishing_point, test_transformation and scale_Z (homography.py:96-154, 554-666) on the
    synthetic cases of tests/calib_cases.py, behind the empty cv2.  The module's ``np`` is wrapped to record every
    np.arange / np.linspace call, and the instance's test_transformation to record P's third column and the error of
    every evaluation.  Data only: inputs, outputs, the recorded calls."""
    import contextlib
    import io
    import warnings
    import calib_cases as cc
    hgmod = ref_module_from_file("_reference_homography_calib", "homography.py")

    class Recorder:
        def __init__(self):
            self.aranges, self.linspaces = [], []

        def __getattr__(self, k):
            return getattr(np, k)

        def arange(self, a, b, step):
            r = np.arange(a, b, step)
            self.aranges.append((float(a), float(b), float(step), float(len(r)), float(r[0]) if len(r) else np.nan,
                                 float(r[-1]) if len(r) else np.nan))
            return r

        def linspace(self, a, b, num=50):
            r = np.linspace(a, b, num=num)
            self.linspaces.append(r.copy())
            return r
    out = {}
    for name in cc.VP_GOLDEN:
        rec = Recorder()
        hgmod.np = rec
        lines = cc.vp_lines(name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            vp = hgmod.find_vanishing_point([row for row in lines])
        out["vp_%s_lines" % name] = lines
        out["vp_%s_point" % name] = np.array([float(vp[0]), float(vp[1])])
        out["vp_%s_arange" % name] = np.array(rec.aranges, np.float64).reshape(16, 2, 6)
    names, _, _, (Ps, Hs), _ = gc.homography_inputs()
    for cam, d in enumerate(cc.SZ_D):
        rec = Recorder()
        hgmod.np = rec
        H, P_true = Hs[cam], Ps[cam]
        st, heights, P0 = cc.sz_case(d, P_true, H)
        hg = hgmod.Homography()
        hg.correspondence = {"true": {"H": H, "P": P_true, "H_inv": np.linalg.inv(H)}, "cam": {"H": H, "P": P0.copy(), "H_inv": np.linalg.inv(H)}}
        hg.default_correspondence = "cam"
        boxes = hg.state_to_im(torch.from_numpy(st), name="true")
        boxes = boxes + torch.from_numpy(synth.normal((d, 8, 2), 400 + d, std=0.7).astype(np.float64))
        hts = torch.from_numpy(heights)
        tag = "sz_d%d_" % d
        out[tag + "boxes"], out[tag + "heights"], out[tag + "H"], out[tag + "P0"] = t2n(boxes), heights, H, P0
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            err0 = hg.test_transformation(boxes, heights=hts)
        out[tag + "tt_text"] = np.frombuffer(text.getvalue().encode(), np.uint8)
        out[tag + "tt_error"] = np.array(float(err0))
        evals = []
        inner = hg.test_transformation

        def recording(points, **kw):
            e = inner(points, **kw)
            evals.append(np.concatenate((hg.correspondence["cam"]["P"][:, 2], [float(e)])))
            return e
        hg.test_transformation = recording
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            hg.scale_Z(boxes, hts)
        out[tag + "sz_text"] = np.frombuffer(text.getvalue().encode(), np.uint8)
        out[tag + "P_final"] = hg.correspondence["cam"]["P"]
        out[tag + "grids"] = np.stack(rec.linspaces)                           # [iterations + 1, 10]: the last is never evaluated
        out[tag + "evals"] = np.stack(evals)                                   # [iterations * 10, 4] = (P[:,2], error)
    hgmod.np = np
    np.savez_compressed(os.path.join(OUT, "calibration.npz"), **out)


def gen_frames4k():
    """The reference's own parse_frame_timestamp (timestamp_utilities.py:46-115) on tests/frames4k_cases.golden_cases().  Its
    two cv2 calls go to a stand-in that provides only cvtColor, threshold and the two constants, made of the restated gray
    rule (cv2 is not installed: that rule alone stays unpinned); the slicing, the six areas, the table search, the point at
    cell 10 and the literal are the reference's.  The empty cv2 stub is put back afterwards.  Data only: inputs, the
    returned time (NaN for None) and the returned error pixels."""
    import frames4k_cases as fc
    stand_in = types.ModuleType("cv2")
    stand_in.COLOR_BGR2GRAY, stand_in.THRESH_BINARY = 6, 0
    stand_in.cvtColor = lambda img, code: fc.gray(img).astype(np.uint8)
    stand_in.threshold = lambda g, thresh, maxval, kind: (float(thresh), np.where(g > thresh, maxval, 0).astype(np.uint8))
    empty = sys.modules["cv2"]
    sys.modules["cv2"] = stand_in
    try:
        tsu = ref_module_from_file("_reference_timestamp_utilities", "timestamp_utilities.py")
        results = [tsu.parse_frame_timestamp(c["geom"], c["table"], frame_pixels=c["frame"]) for c in fc.golden_cases()]
    finally:
        sys.modules["cv2"] = empty
    fc.save_golden(os.path.join(OUT, "frames4k.npz"), results)


def main():
    if not os.path.isdir(REF):
        sys.exit("make_golden.py needs the reference checkout at %s (build container only)" % REF)
    global OUT
    argv = sys.argv[1:]
    if "--out" in argv:
        i = argv.index("--out")
        OUT = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    os.makedirs(OUT, exist_ok=True)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    install_shims()
    m_dir, l_dir, u_dir, a_dir = import_variant("dir")
    dir_mods = (m_dir, l_dir, u_dir, a_dir)
    m_2d, l_2d, u_2d, a_2d = import_variant("2d")
    which = set(argv) or {"anchors", "losses", "boxes", "model", "model_deep", "homography", "csv", "csv_rows", "tracker_post", "crop_refine", "kf", "tracker_assoc", "ts_bias", "fit_filter", "csv_eval", "augment", "augment_crop", "mot_eval", "calibration", "frames4k", "datareader", "replay", "tracker_run", "label_audit", "label_rewrite", "label_trajectory", "label_quality", "label_assist", "track_stitch"}
    if "anchors" in which:
        gen_anchors(a_dir)
    if "losses" in which:
        gen_losses(l_dir, l_2d, a_dir)
    if "boxes" in which:
        gen_boxes(m_dir, u_dir, m_2d, u_2d)
    if "model" in which:
        gen_model(m_dir, m_2d)
    if "model_deep" in which:
        gen_model_deep(m_dir)
    if "homography" in which:
        gen_homography()
    if "csv" in which:
        gen_csv_kat()
    if "csv_rows" in which:
        gen_csv_rows()
    if "tracker_post" in which or "crop_refine" in which or "tracker_assoc" in which or "ts_bias" in which:
        tracker_import_shims()
    if "tracker_post" in which:
        gen_tracker_post()
    if "crop_refine" in which:
        gen_crop_refine()
    if "kf" in which:
        gen_kf()
    if "tracker_assoc" in which:
        gen_tracker_assoc()
    if "ts_bias" in which:
        gen_ts_bias()
    if "fit_filter" in which:
        gen_fit_filter()
    if "csv_eval" in which:
        gen_csv_eval()
    if "augment" in which:
        gen_augment()
    if "augment_crop" in which:
        gen_augment_crop()
    if "mot_eval" in which:
        gen_mot_eval()
    if "calibration" in which:
        gen_calibration()
    if "frames4k" in which:
        gen_frames4k()
    if "datareader" in which:
        gen_datareader()
    if "replay" in which:
        gen_replay()
    if "tracker_run" in which:
        gen_tracker_run()
    if "label_audit" in which:
        gen_label_audit()
    if "label_rewrite" in which:
        gen_label_rewrite()
    if "label_trajectory" in which:
        gen_label_trajectory()
    if "label_quality" in which:
        gen_label_quality()
    if "label_assist" in which:
        gen_label_assist()
    if "track_stitch" in which:
        gen_track_stitch()
    for fn in sorted(os.listdir(OUT)):
        print("%-20s %8.1f KiB" % (fn, os.path.getsize(os.path.join(OUT, fn)) / 1024))
    del dir_mods


if __name__ == "__main__":
    main()
