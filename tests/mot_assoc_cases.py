"""Identity and association scores (mot_evaluator.evaluate_association, csrc/mot_assoc.hip): a plain restatement of the
published definitions with the device's summation orders, the scenes, and builders that turn a scene into CSV rows.

A scene is a dict: ``gt_ids`` / ``pred_ids`` (per frame the raw ids, in row / column order; an empty list = the side lacks the
frame) and ``ious`` (per frame the fp64 matrix S_t [n_gt, n_pred], None unless both sides hold the frame).  The IoU matrices are
injected through ``ious=``, so thresholds can be hit exactly.  Ids become dense indices in first-seen order, ground truth and
predictions apart, frames in increasing order -- as mot_evaluator.pack_tracks does.

Definitions (Ristani et al., ECCV-W 2016; Luiten et al., IJCV 2021), eps = 2^-52, gc / pc = frames holding an id:
  C[g,p] = frames with S >= id_iou;  IDTP = max-weight one-to-one matching of ids on C (scipy, maximize);  IDFN = sum gc - IDTP,
  IDFP = sum pc - IDTP;  IDR = IDTP / max(1, IDTP + IDFN), IDP likewise, IDF1 = IDTP / max(1, IDTP + 0.5 IDFP + 0.5 IDFN)
  per scored frame den = (colsum[p] + rowsum[g]) - S, J = S / den where den > eps else 0, pot[g,p] += J
  ga = pot / ((gc[g] + pc[p]) - pot);  per scored frame ONE scipy assignment on -(ga * S)
  alpha_k = 0.05 + k 0.05 (np.arange(0.05, 0.99, 0.05));  a matched pair counts for k when S >= alpha_k - eps
  TP_k, FN_k, FP_k, Loc_k, M_k[g,p];  AssA_k = sum M (M / max(1, gc + pc - M)) / max(1, TP_k), AssRe with max(1, gc), AssPr with
  max(1, pc);  DetRe = TP / max(1, TP + FN), DetPr, DetA = TP / max(1, TP + FN + FP);  HOTA_k = sqrt(DetA AssA);
  LocA_k = max(1e-10, Loc) / max(1e-10, TP);  the reported scalars are np.mean over k.
Summation orders (the device's, so that it can be held to them bit for bit):
  rowsum[i] = ((S[i,0] + S[i,1]) + ...) and colsum[j] = ((S[0,j] + S[1,j]) + ...): sequential, ascending
  pot[g,p]: one add per scored frame holding both ids, frames ascending
  Loc_k over the slots (scored frames ascending, ground-truth row ascending inside a frame) and the three association sums over the
  cells g * P + p: entry e goes to partial e % 256, each partial in ascending e, the partials added in increasing order; an entry
  that does not count adds +0.0
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

import mot_cases as mc

LANES = 256
EPS = 2.0 ** -52
ALPHAS = np.arange(0.05, 0.99, 0.05)
N_ALPHA = 19
MAX_CELLS = 1 << 20                            # ops.MOT_ASSOC_MAX_CELLS
FIGURES = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")


def dense_ids(frames_ids):
    index, out = {}, []
    for ids in frames_ids:
        out.append(np.array([index.setdefault(int(v), len(index)) for v in ids], np.int64))
    return out, index


def fixed_sum(values):
    v = np.asarray(values, np.float64).reshape(-1)
    x = np.concatenate((v, np.zeros((-len(v)) % LANES))).reshape(-1, LANES)
    part = np.zeros(LANES)
    for row in x:
        part = part + row
    s = 0.0
    for p in part:
        s = s + p
    return float(s)


def ascending_sums(S):
    """(rowsum, colsum): sequential ascending sums, one column / row added at a time."""
    r, c = np.zeros(S.shape[0]), np.zeros(S.shape[1])
    for j in range(S.shape[1]):
        r = r + S[:, j]
    for i in range(S.shape[0]):
        c = c + S[i, :]
    return r, c


def prefix_length(s, alphas=ALPHAS):
    n = 0
    for a in alphas:
        if not s >= a - EPS:
            break
        n += 1
    return n


def figures(TP, FN, FP, loc, a_sum, re_sum, pr_sum):
    TP, FN, FP = (np.asarray(x, np.float64) for x in (TP, FN, FP))
    per = {"AssA": np.asarray(a_sum) / np.maximum(1, TP), "AssRe": np.asarray(re_sum) / np.maximum(1, TP),
           "AssPr": np.asarray(pr_sum) / np.maximum(1, TP), "DetRe": TP / np.maximum(1, TP + FN), "DetPr": TP / np.maximum(1, TP + FP),
           "DetA": TP / np.maximum(1, TP + FN + FP), "LocA": np.maximum(1e-10, np.asarray(loc)) / np.maximum(1e-10, TP)}
    per["HOTA"] = np.sqrt(per["DetA"] * per["AssA"])
    out = {k: float(np.mean(per[k])) for k in FIGURES}
    out["HOTA(0)"] = float(per["HOTA"][0])
    return out, per


def identity_scores(IDTP, n_gt, n_pred):
    IDFN, IDFP = n_gt - IDTP, n_pred - IDTP
    return {"IDTP": IDTP, "IDFN": IDFN, "IDFP": IDFP, "IDR": IDTP / max(1, IDTP + IDFN), "IDP": IDTP / max(1, IDTP + IDFP),
            "IDF1": IDTP / max(1, IDTP + 0.5 * IDFP + 0.5 * IDFN)}


def restated(scene, id_iou=0.5, alphas=ALPHAS):
    """-> dict: gc, pc, C, id_rows / id_cols (scipy's matching on C), the identity scores, pot, the slots (frame, row, col, S,
    prefix length), TP / FN / FP / Loc / the association sums per alpha, ``per_alpha`` and the mean figures."""
    gids, gmap = dense_ids(scene["gt_ids"])
    pids, pmap = dense_ids(scene["pred_ids"])
    G, P = len(gmap), len(pmap)
    for ids in gids + pids:
        if len(set(ids.tolist())) != len(ids):
            raise ValueError("an id occurs twice in one frame on one side")
    gc, pc = np.zeros(G, np.int64), np.zeros(P, np.int64)
    C, pot = np.zeros((G, P), np.int64), np.zeros((G, P))
    for t, (g, p) in enumerate(zip(gids, pids)):
        for v in g:
            gc[v] += 1
        for v in p:
            pc[v] += 1
        if len(g) and len(p):
            S = np.asarray(scene["ious"][t], np.float64)
            assert S.shape == (len(g), len(p))
            with np.errstate(invalid="ignore", divide="ignore"):
                C[np.ix_(g, p)] += S >= id_iou
                rs, cs = ascending_sums(S)
                den = (cs[None, :] + rs[:, None]) - S
                J = np.where(den > EPS, S / np.where(den > EPS, den, 1.0), 0.0)
            pot[np.ix_(g, p)] = pot[np.ix_(g, p)] + J                    # ids are unique in a frame: one add per cell
    id_rows, id_cols = linear_sum_assignment(C, maximize=True)
    IDTP = int(C[id_rows, id_cols].sum())
    n_gt, n_pred = int(gc.sum()), int(pc.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        ga = pot / ((gc[:, None] + pc[None, :]) - pot)
    slots = []
    for t, (g, p) in enumerate(zip(gids, pids)):
        if not (len(g) and len(p)):
            continue
        S = np.asarray(scene["ious"][t], np.float64)
        with np.errstate(invalid="ignore"):
            score = ga[np.ix_(g, p)] * S
        rows, cols = linear_sum_assignment(-score)
        for i, j in zip(rows, cols):
            slots.append((t, int(i), int(j), float(S[i, j]), prefix_length(S[i, j], alphas), int(g[i]), int(p[j])))
    n = np.array([s[4] for s in slots], np.int64)
    sv = np.array([s[3] for s in slots], np.float64)
    K = len(alphas)
    TP = np.array([int((n > k).sum()) for k in range(K)], np.int64)
    FN, FP = n_gt - TP, n_pred - TP
    loc = np.array([fixed_sum(np.where(n > k, sv, 0.0)) for k in range(K)])
    M = np.zeros((K, G, P), np.int64)
    for s in slots:
        M[:s[4], s[5], s[6]] += 1
    a_sum, re_sum, pr_sum = np.zeros(K), np.zeros(K), np.zeros(K)
    for k in range(K):
        m = M[k].astype(np.float64)
        a_sum[k] = fixed_sum(m * (m / np.maximum(1, gc[:, None] + pc[None, :] - M[k])))
        re_sum[k] = fixed_sum(m * (m / np.maximum(1, gc[:, None] + 0 * pc[None, :])))
        pr_sum[k] = fixed_sum(m * (m / np.maximum(1, 0 * gc[:, None] + pc[None, :])))
    fig, per = figures(TP, FN, FP, loc, a_sum, re_sum, pr_sum)
    out = dict(gc=gc, pc=pc, C=C, id_rows=id_rows, id_cols=id_cols, pot=pot, slots=slots, TP=TP, FN=FN, FP=FP, loc=loc, a_sum=a_sum,
               re_sum=re_sum, pr_sum=pr_sum, M=M, per_alpha=per, n_gt=n_gt, n_pred=n_pred)
    out.update(identity_scores(IDTP, n_gt, n_pred))
    out.update(fig)
    return out


# ------------------------------------------------------------------------------------------------ scenes -> rows
def scene_rows(scene):
    """-> (gt_rows, pred_rows, flat fp64 IoUs): rows with the scene's ids and counts; the boxes are placeholders, the IoU
    matrices travel through ``ious=``."""
    gt, pred, flat = {}, {}, []
    for t, (g, p) in enumerate(zip(scene["gt_ids"], scene["pred_ids"])):
        for i, v in enumerate(g):
            gt.setdefault(t, []).append(mc.gt_row(t, int(v), "sedan", mc.box_corners(32.0 * (i % 32), 16.0 * (i // 32), 16.0, 6.0, 4.0), 1.0))
        for j, v in enumerate(p):
            pred.setdefault(t, []).append(mc.pred_row(t, int(v), "sedan", (32.0 * (j % 32), 16.0 * (j // 32), 16.0, 6.0, 4.0, 1.0, 1.0)))
        if len(g) and len(p):
            flat.append(np.asarray(scene["ious"][t], np.float64).reshape(-1))
    return gt, pred, (np.concatenate(flat) if flat else np.zeros(0))


def _scene(frames):
    """frames: [(gt ids, pred ids, S or None)]."""
    return dict(gt_ids=[list(f[0]) for f in frames], pred_ids=[list(f[1]) for f in frames],
                ious=[None if f[2] is None else np.asarray(f[2], np.float64).reshape(len(f[0]), len(f[1])) for f in frames])


# ------------------------------------------------------------------------------------------------ closed forms
def closed_form_scenes(n=6):
    """name -> (scene, expected): the answers derived by hand from the definitions (2n frames each)."""
    one = dict(DetA=1.0, DetRe=1.0, DetPr=1.0)
    out = {}
    out["perfect"] = (_scene([([1], [10], [[1.0]])] * (2 * n)),
                      dict(one, HOTA=1.0, AssA=1.0, AssRe=1.0, AssPr=1.0, LocA=1.0, IDF1=1.0, IDP=1.0, IDR=1.0, IDTP=2 * n, IDFN=0, IDFP=0))
    # the prediction id changes at half time: M = n in two cells, gc = 2n, pc = n each
    out["split"] = (_scene([([1], [10], [[1.0]])] * n + [([1], [11], [[1.0]])] * n),
                    dict(one, AssA=0.5, AssRe=0.5, AssPr=1.0, HOTA=float(np.sqrt(0.5)), LocA=1.0, IDTP=n, IDFN=n, IDFP=n, IDF1=0.5))
    # two ids exchange their predictions at half time: four cells with M = n, gc = pc = 2n -> n (n / 3n) each
    eye = [[1.0, 0.0], [0.0, 1.0]]
    out["swap"] = (_scene([([1, 2], [10, 11], eye)] * n + [([1, 2], [11, 10], eye)] * n),
                   dict(one, AssA=1.0 / 3.0, AssRe=0.5, AssPr=0.5, HOTA=float(np.sqrt(1.0 / 3.0)), LocA=1.0, IDF1=0.5, IDTP=2 * n))
    # S = 0.5: alpha_9 = 0.05 + 9 * 0.05 is the alpha - eps edge; ten alphas pass
    out["half"] = (_scene([([1], [10], [[0.5]])] * (2 * n)),
                   dict(HOTA=10.0 / 19.0, DetA=10.0 / 19.0, AssA=10.0 / 19.0, LocA=14.0 / 19.0, IDF1=1.0, IDTP=2 * n))
    # nothing ever matches: S = 0 frames, frames only in the ground truth, frames only in the predictions
    out["misses"] = (_scene([([1], [10], [[0.0]])] * n + [([1, 2], [], None)] * 2 + [([], [10, 11, 12], None)] * 3),
                     dict(HOTA=0.0, DetA=0.0, AssA=0.0, DetRe=0.0, DetPr=0.0, AssRe=0.0, AssPr=0.0, LocA=1.0, IDF1=0.0, IDTP=0,
                          IDFN=n + 4, IDFP=n + 9))
    return out


def closed_form_per_alpha(name, n=6):
    """The per-alpha integers of the scenes where they are not the same for every alpha."""
    if name == "half":
        return dict(TP=np.array([2 * n] * 10 + [0] * 9), FN=np.array([0] * 10 + [2 * n] * 9), FP=np.array([0] * 10 + [2 * n] * 9))
    if name == "misses":
        return dict(TP=np.zeros(19, np.int64), FN=np.full(19, n + 4), FP=np.full(19, n + 9))
    return dict(TP=np.full(19, {"perfect": 2 * n, "split": 2 * n, "swap": 4 * n}[name]), FN=np.zeros(19, np.int64), FP=np.zeros(19, np.int64))


# ------------------------------------------------------------------------------------------------ edge and fuzz scenes
def fuzz_scene(seed, frames, n_gid, n_pid, win_g, win_p, step_g=1, step_p=1, density=0.35, levels=None, dup_cols=0, one_sided=()):
    """Frame t holds the ground-truth ids (t * step_g + i) % n_gid, i < win_g (win_g <= n_gid keeps them unique), shuffled, and
    the predictions likewise: an id leaves and, once the window wraps, comes back.  S: uniform in (0, 1) or drawn from
    ``levels``, zero outside a random ``density`` of the cells; dup_cols: that many columns copy their left neighbour (in every
    frame the two ids always meet, so their scores tie exactly).  one_sided: {frame: "gt" | "pred"} drops the other side."""
    rng = np.random.RandomState(seed)
    fr = []
    for t in range(frames):
        ng = win_g if np.isscalar(win_g) else win_g[t % len(win_g)]
        npr = win_p if np.isscalar(win_p) else win_p[t % len(win_p)]
        g = np.array([(t * step_g + i) % n_gid for i in range(ng)])
        p = np.array([(t * step_p + i) % n_pid for i in range(npr)])
        pg, pp = rng.permutation(ng), rng.permutation(npr)
        S = rng.uniform(0.0, 1.0, (ng, npr)) if levels is None else rng.choice(np.asarray(levels, np.float64), (ng, npr))
        S = S * (rng.uniform(0, 1, (ng, npr)) < density)
        base = np.argsort(p)                                             # columns by id, so that duplicates pair the same ids
        for d in range(min(dup_cols, npr // 2)):
            S[:, base[2 * d + 1]] = S[:, base[2 * d]]
        g, p, S = 1000 + g[pg], 5000 + p[pp], S[pg][:, pp]
        side = one_sided.get(t) if isinstance(one_sided, dict) else None
        if side == "gt":
            fr.append((g, [], None))
        elif side == "pred":
            fr.append(([], p, None))
        else:
            fr.append((g, p, S))
    return _scene(fr)


def edge_scenes():
    """name -> (scene, id_iou): the smallest sizes that reach each code path."""
    s = {}
    s["transpose"] = (fuzz_scene(1, 6, 7, 7, [3, 5], [5, 3], density=0.7), 0.5)                # n_gt < n_pred and n_gt > n_pred
    s["wide70"] = (fuzz_scene(2, 3, 72, 75, [70, 4, 66], [66, 5, 70], density=0.1), 0.5)      # past one wave's 64 lanes
    s["ids_tall"] = (fuzz_scene(3, 8, 80, 70, 24, 22, step_g=9, step_p=8, density=0.3), 0.3)  # G > P, more than 64 columns
    s["ids_wide"] = (fuzz_scene(4, 8, 70, 80, 22, 24, step_g=8, step_p=9, density=0.3), 0.3)  # P > G
    s["ids300"] = (fuzz_scene(5, 5, 300, 310, 100, 104, step_g=50, step_p=52, density=0.05), 0.4)  # past 256 ids a side
    s["absent"] = (fuzz_scene(6, 14, 6, 7, 3, 4, density=0.8, one_sided={4: "gt", 9: "pred"}), 0.5)   # ids leave and return
    s["ties"] = (fuzz_scene(7, 10, 8, 10, 5, 8, levels=[0.25, 0.5, 0.5, 0.75, 1.0], density=0.6, dup_cols=2), 0.5)   # C and ga S tie
    s["on_id_iou"] = (fuzz_scene(8, 9, 5, 5, 4, 4, levels=[0.5, 0.5 - 2.0 ** -54, 0.5 + 2.0 ** -52, 0.75], density=0.9), 0.5)
    s["long"] = (fuzz_scene(9, 60, 12, 15, 6, 7, density=0.5), 0.5)
    return s


def duplicate_scene():
    return _scene([([1, 2], [10, 11], [[0.9, 0.0], [0.0, 0.9]]), ([1, 2], [10, 10], [[0.9, 0.0], [0.0, 0.9]])])


def nan_scene():
    return _scene([([1], [10], [[0.9]]), ([1, 2], [10, 11], [[0.9, 0.1], [float("nan"), 0.8]])])


def fragmented_sequence(frames=2000, n=40, pieces=8, seed=0):
    """mot_cases.synth_sequence with every track's prediction id changing ``pieces`` times as often: several times more
    predicted ids than true ones (the benchmark's second workload)."""
    gt, pred = mc.synth_sequence(frames, n, seed)
    span = max(1, 500 // pieces)
    for f, rows in pred.items():
        for k, r in enumerate(rows):
            r[2] = str(k + 100 * ((f + k) // span))
    return gt, pred
