"""docs/MOTEVAL.md §1 restated on the CPU: HOTA and CLEAR MOT of one ground-truth / tracker pair, NumPy with explicit sequential
sums and scipy.optimize.linear_sum_assignment(-score).  Uses neither the device nor strongsort_yolo_amd.moteval; the GPU tests
compare the library's per-row record and every figure with this file by equality.

Rows are float64 [N, 8]: frame, id, x1, y1, x2, y2, conf, cls.  Every sum starts from 0.0 and adds in the written order
(`seq_sum`: np.cumsum is a sequential scan; np.sum is pairwise and is not used here)."""
from __future__ import annotations

import numpy as np
from scipy.optimize import linear_sum_assignment

EPS = 2.0 ** -52
ALPHAS = [0.05 + k * 0.05 for k in range(19)]
MAX_BOXES = 256
HOTA_FIELDS = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")


def seq_sum(x) -> float:
    x = np.asarray(x, np.float64).ravel()
    return float(np.cumsum(x)[-1]) if len(x) else 0.0


def check_rows(rows, what="rows") -> np.ndarray:
    """-> the rows by (frame, id); refuses duplicates, empty boxes, NaN and infinity"""
    r = np.array(rows, np.float64, copy=True).reshape(-1, 8)
    if not np.isfinite(r).all():
        raise ValueError(f"{what}: NaN or infinity")
    if len(r) and len(np.unique(r[:, :2], axis=0)) != len(r):
        raise ValueError(f"{what}: duplicate (frame, id)")
    if ((r[:, 4] <= r[:, 2]) | (r[:, 5] <= r[:, 3])).any():
        raise ValueError(f"{what}: a box with x2 <= x1 or y2 <= y1")
    return r[np.lexsort((r[:, 1], r[:, 0]))] if len(r) else r


class Pair:
    """One pair laid out as the specification names it: evaluated frames (the union, rising), per frame the row ranges of
    both sides, dense ids by np.unique per side."""

    def __init__(self, gt_rows, tr_rows):
        self.gt, self.tr = check_rows(gt_rows, "ground truth"), check_rows(tr_rows, "tracker")
        self.frames = np.unique(np.concatenate([self.gt[:, 0], self.tr[:, 0]]))
        self.gt_off = np.searchsorted(self.gt[:, 0], np.concatenate([self.frames, [np.inf]]), "left").astype(np.int64)
        self.tr_off = np.searchsorted(self.tr[:, 0], np.concatenate([self.frames, [np.inf]]), "left").astype(np.int64)
        self.gt_uid, self.gt_id = np.unique(self.gt[:, 1], return_inverse=True)
        self.tr_uid, self.tr_id = np.unique(self.tr[:, 1], return_inverse=True)
        self.gt_id, self.tr_id = self.gt_id.reshape(-1), self.tr_id.reshape(-1)
        self.n_gid, self.n_tid = len(self.gt_uid), len(self.tr_uid)
        self.cnt_g = np.bincount(self.gt_id, minlength=self.n_gid).astype(np.int64)
        self.cnt_t = np.bincount(self.tr_id, minlength=self.n_tid).astype(np.int64)

    def frame(self, f):
        a, b = slice(self.gt_off[f], self.gt_off[f + 1]), slice(self.tr_off[f], self.tr_off[f + 1])
        return a, b


def similarity(a, b) -> np.ndarray:
    """S [len(a), len(b)] of boxes x1 y1 x2 y2: each cell by the four written steps"""
    a, b = np.asarray(a, np.float64).reshape(-1, 4), np.asarray(b, np.float64).reshape(-1, 4)
    S = np.zeros((len(a), len(b)))
    for i in range(len(a)):
        ax1, ay1, ax2, ay2 = a[i]
        w = np.maximum(0.0, np.minimum(ax2, b[:, 2]) - np.maximum(ax1, b[:, 0]))
        h = np.maximum(0.0, np.minimum(ay2, b[:, 3]) - np.maximum(ay1, b[:, 1]))
        inter = w * h
        union = ((ax2 - ax1) * (ay2 - ay1) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) - inter
        S[i] = inter / union
    return S


def solve(score):
    """-> (rows, cols) of the assignment that minimises -score, SciPy's algorithm and tie order (it transposes a tall matrix itself)"""
    return linear_sum_assignment(-score)


def global_alignment(p: Pair, sims):
    pot = np.zeros((p.n_gid, p.n_tid))
    for f in range(len(p.frames)):
        a, b = p.frame(f)
        S = sims[f]
        if S.size == 0:
            continue
        R = np.cumsum(S, axis=1)[:, -1]                 # j rising
        Cc = np.cumsum(S, axis=0)[-1, :]                # i rising
        den = (Cc[None, :] + R[:, None]) - S
        si = np.where(den > EPS, S / np.where(den > EPS, den, 1.0), 0.0)
        pot[np.ix_(p.gt_id[a], p.tr_id[b])] += si       # ids are unique in a frame: one addend per cell and frame, frames rising
    return pot / ((p.cnt_g[:, None] + p.cnt_t[None, :]).astype(np.float64) - pot)


def hota_record(p: Pair, sims, GA):
    idx, s = np.full(len(p.gt), -1, np.int32), np.zeros(len(p.gt))
    for f in range(len(p.frames)):
        a, b = p.frame(f)
        S = sims[f]
        if S.size == 0:
            continue
        score = GA[np.ix_(p.gt_id[a], p.tr_id[b])] * S
        r, c = solve(score)
        idx[a.start + r], s[a.start + r] = c, S[r, c]
    return idx, s


def clear_record(p: Pair, sims, thr):
    """-> (idx, s, IDSW, n_g): the walk of §1 with both tables"""
    idx, s = np.full(len(p.gt), -1, np.int32), np.zeros(len(p.gt))
    prev, prev_t = np.full(p.n_gid, -1, np.int64), np.full(p.n_gid, -1, np.int64)
    idsw, n_g = 0, np.zeros(p.n_gid, np.int64)
    for f in range(len(p.frames)):
        a, b = p.frame(f)
        S = sims[f]
        if S.size == 0:
            continue
        g, t = p.gt_id[a], p.tr_id[b]
        score = np.where(t[None, :] == prev_t[g][:, None], 1000.0, 0.0) + S
        score[S < thr - EPS] = 0.0
        r, c = solve(score)
        m = score[r, c] > EPS
        r, c = r[m], c[m]
        idx[a.start + r], s[a.start + r] = c, S[r, c]
        gm, tm = g[r], t[c]
        idsw += int(((prev[gm] >= 0) & (prev[gm] != tm)).sum())
        n_g[gm[prev_t[gm] < 0]] += 1
        prev[gm] = tm
        prev_t[:] = -1
        prev_t[gm] = tm
    return idx, s, idsw, n_g


def hota_figures(p: Pair, idx, s) -> dict:
    n_gt, n_tr = len(p.gt), len(p.tr)
    frame_of = np.repeat(np.arange(len(p.frames)), np.diff(p.gt_off))
    g = p.gt_id
    t = p.tr_id[np.where(idx >= 0, p.tr_off[frame_of] + idx, 0)] if n_tr else np.zeros(n_gt, np.int64)
    out = {k: [] for k in HOTA_FIELDS}
    for alpha in ALPHAS:
        m = (idx >= 0) & (s >= alpha - EPS)
        tp = int(m.sum())
        fn, fp = n_gt - tp, n_tr - tp
        det_a, det_re, det_pr = tp / max(1, tp + fn + fp), tp / max(1, tp + fn), tp / max(1, tp + fp)
        loc_a = max(1e-10, seq_sum(s[m])) / max(1e-10, float(tp))
        key, c = np.unique(g[m].astype(np.int64) * max(p.n_tid, 1) + t[m], return_counts=True)      # rising (g, t)
        cg, ct = p.cnt_g[key // max(p.n_tid, 1)], p.cnt_t[key % max(p.n_tid, 1)]
        c = c.astype(np.float64)
        ass_a = seq_sum(c * (c / np.maximum(1, cg + ct - c))) / max(1, tp)
        ass_re = seq_sum(c * (c / np.maximum(1, cg))) / max(1, tp)
        ass_pr = seq_sum(c * (c / np.maximum(1, ct))) / max(1, tp)
        for k, v in zip(HOTA_FIELDS, (float(np.sqrt(det_a * ass_a)), det_a, ass_a, det_re, det_pr, ass_re, ass_pr, loc_a)):
            out[k].append(float(v))
    res = {}
    for k in HOTA_FIELDS:
        res[k] = seq_sum(out[k]) / 19.0
        res[k + "_alpha"] = out[k]
    res["HOTA(0)"], res["LocA(0)"] = out["HOTA"][0], out["LocA"][0]
    return res


def clear_figures(p: Pair, idx, s, idsw, n_g) -> dict:
    n_gt, n_tr = len(p.gt), len(p.tr)
    m = idx >= 0
    tp = int(m.sum())
    fn, fp = n_gt - tp, n_tr - tp
    share = np.bincount(p.gt_id[m], minlength=p.n_gid) / np.maximum(1, p.cnt_g)
    mt, ml = int((share > 0.8).sum()), int((share < 0.2).sum())
    return {"TP": tp, "FN": fn, "FP": fp, "IDSW": int(idsw), "MOTA": (tp - fp - idsw) / max(1, tp + fn), "MOTP": seq_sum(s[m]) / max(1, tp),
            "MT": mt, "PT": p.n_gid - mt - ml, "ML": ml, "Frag": int(np.maximum(0, n_g - 1).sum())}


def evaluate_full(gt_rows, tr_rows, thr: float = 0.5):
    """-> (metrics dict, record dict: hota_idx, hota_s, clear_idx, clear_s per ground-truth row by (frame, id), GA)"""
    p = Pair(gt_rows, tr_rows)
    for f in range(len(p.frames)):
        a, b = p.frame(f)
        if max(a.stop - a.start, b.stop - b.start) > MAX_BOXES:
            raise ValueError(f"frame {int(p.frames[f])}: more than {MAX_BOXES} boxes")
    sims = [similarity(p.gt[p.frame(f)[0], 2:6], p.tr[p.frame(f)[1], 2:6]) for f in range(len(p.frames))]
    GA = global_alignment(p, sims)
    hi, hs = hota_record(p, sims, GA)
    ci, cs, idsw, n_g = clear_record(p, sims, thr)
    metrics = {"gt_rows": len(p.gt), "tracker_rows": len(p.tr), "gt_ids": p.n_gid, "tracker_ids": p.n_tid, "frames": len(p.frames), "thr": float(thr)}
    metrics.update(hota_figures(p, hi, hs))
    metrics.update(clear_figures(p, ci, cs, idsw, n_g))
    return metrics, {"hota_idx": hi, "hota_s": hs, "clear_idx": ci, "clear_s": cs, "GA": GA, "pair": p}


def evaluate(gt_rows, tr_rows, thr: float = 0.5) -> dict:
    return evaluate_full(gt_rows, tr_rows, thr)[0]


# ---- seeded inputs: SynthStream ground truth and a perturbed copy as tracker output (tests/golden/make_moteval_golden.py) --------
def synth_gt(seed: int, n_ids: int, n_frames: int, width: int = 1280, height: int = 720) -> np.ndarray:
    from strongsort_yolo_amd.synth import make_stream
    st = make_stream(seed, width, height, n_ids)
    rows = []
    for k in range(n_frames):
        fr = st.next_frame()
        r = np.zeros((len(fr.dets), 8))
        r[:, 0], r[:, 1], r[:, 2:6], r[:, 6], r[:, 7] = k, fr.gt_ids + 1, fr.dets[:, :4], fr.dets[:, 4], fr.dets[:, 5]
        rows.append(r)
    return np.concatenate(rows, 0)


def perturb(gt, rng, swap_every: int = 0, drop: float = 0.0, jitter: float = 0.0, fp_rate: float = 0.0, width: int = 1280, height: int = 720):
    """Tracker rows from ground truth: two ids exchange every `swap_every` frames, a share `drop` of the rows is lost, the corners
    get Gaussian jitter (rounded to 1/8 px, sides kept >= 1 px), Poisson(fp_rate) false positives a frame with fresh ids."""
    r = np.array(gt, np.float64, copy=True)
    ids = np.unique(r[:, 1])
    name = {i: i for i in ids}
    frames = np.unique(r[:, 0])
    if swap_every:
        for f in frames:
            if f > 0 and int(f) % swap_every == 0 and len(ids) >= 2:
                a, b = rng.choice(ids, 2, replace=False)
                name[a], name[b] = name[b], name[a]
            sel = r[:, 0] == f
            r[sel, 1] = [name[i] for i in gt[sel, 1]]
    if drop:
        r = r[rng.random(len(r)) >= drop]
    if jitter:
        r[:, 2:6] = np.round((r[:, 2:6] + rng.normal(0, jitter, (len(r), 4))) * 8) / 8
        r[:, 4], r[:, 5] = np.maximum(r[:, 4], r[:, 2] + 1), np.maximum(r[:, 5], r[:, 3] + 1)
    fresh, extra = float(ids.max()) + 1000, []
    if fp_rate:
        for f in frames:
            for _ in range(int(rng.poisson(fp_rate))):
                w, h = rng.integers(40, 120), rng.integers(80, 240)
                x, y = rng.integers(0, width - w), rng.integers(0, height - h)
                extra.append([f, fresh, x, y, x + w, y + h, 0.5, 0])
                fresh += 1
    if extra:
        r = np.concatenate([r, np.array(extra, np.float64)], 0)
    return r[np.lexsort((r[:, 1], r[:, 0]))]


def random_frames(rng, counts, first_frame: int = 0, step: int = 1, width: int = 1280, height: int = 720, overlap: bool = True):
    """(gt, tracker) rows with the given per-frame (n_gt, n_tracker) box counts: boxes on a 1/4 px grid; the tracker boxes of a frame
    are jittered copies of its ground truth (cyclically) so that most pairs overlap; ids are persistent across frames."""
    gt, tr = [], []
    for k, (ng, nt) in enumerate(counts):
        f = first_frame + k * step
        w, h = rng.integers(160, 480, ng) / 4.0, rng.integers(320, 960, ng) / 4.0
        x, y = rng.integers(0, 4 * (width - 120), ng) / 4.0, rng.integers(0, 4 * (height - 240), ng) / 4.0
        g = np.zeros((ng, 8))
        g[:, 0], g[:, 1], g[:, 2], g[:, 3], g[:, 4], g[:, 5], g[:, 6] = f, rng.permutation(max(ng, 1))[:ng] + 1, x, y, x + w, y + h, 1.0
        gt.append(g)
        t = np.zeros((nt, 8))
        if nt:
            if ng and overlap:
                src = g[np.arange(nt) % ng, 2:6] + rng.integers(-60, 61, (nt, 4)) / 4.0
            else:
                src = np.stack([rng.integers(0, 3000, nt) / 4.0, rng.integers(0, 1500, nt) / 4.0, np.zeros(nt), np.zeros(nt)], 1)
                src[:, 2], src[:, 3] = src[:, 0] + 50, src[:, 1] + 100
            src[:, 2], src[:, 3] = np.maximum(src[:, 2], src[:, 0] + 1), np.maximum(src[:, 3], src[:, 1] + 1)
            t[:, 0], t[:, 1], t[:, 2:6], t[:, 6] = f, rng.permutation(nt) + 101, src, 0.5
        tr.append(t)
    return np.concatenate(gt, 0), np.concatenate(tr, 0)
