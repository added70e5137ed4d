"""Scoring tracks against ground truth: HOTA (Luiten et al. 2020) and CLEAR MOT (Bernardin & Stiefelhagen 2008), docs/MOTEVAL.md.

Rows are the float64 [N, 8] rows of `strongsort_yolo_amd.gsi`: frame, id, x1, y1, x2, y2, conf, cls.  A pair is one ground-truth row
set and one tracker row set of the same sequence.  The similarities, HOTA's global alignment, every per-frame assignment problem and
CLEAR's walk over the frames run on the device (csrc/ss_mot.hip), all pairs of a call in one device call; the host half here maps
ids to dense indices, packs the call and turns the per-row record that comes back into the figures, with sequential sums.  There is
no CPU fallback: without the library or a device `evaluate` raises as the rest of the package does.  tests/moteval_ref.py restates
the whole of it; the device's record and every figure equal it bit for bit.  Parity with TrackEval or motmetrics is unpinned.

The identity metrics IDF1, IDP and IDR (docs/MOTEVAL.md §1 "Identity") are a device call of their own, `identity` /
`identity_full`, or `evaluate(..., identity=True)`, which adds their six keys to every dict: the counts of the id pairs and one
maximum-weight matching of ground-truth ids to tracker ids, solved by a workgroup for up to 4096 ids a side.  They are not part of
the default call: `evaluate(..., metrics=("IDF1",))` still refuses by name and says which switch to use."""
from __future__ import annotations

import json

import numpy as np

from . import lib as _lib

EPS = 2.0 ** -52
ALPHAS = [0.05 + k * 0.05 for k in range(19)]
MAX_BOXES = 256                                         # ss_mot_max_boxes(); the other caps are the library's to refuse (docs/MOTEVAL.md §2)
LDS_CELLS = 20000                                       # a frame's matrix of up to this many cells is solved from LDS
HOTA_FIELDS = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")
REFUSED = ("IDF1", "IDP", "IDR")                        # not in `metrics=`: they come from identity=True or moteval.identity
IDENTITY_FIELDS = ("IDTP", "IDFN", "IDFP", "IDF1", "IDP", "IDR")


def _seq(x) -> float:
    x = np.asarray(x, np.float64).ravel()
    return float(np.cumsum(x)[-1]) if len(x) else 0.0


def _rows(rows, what: str, classes=None) -> np.ndarray:
    r = np.array(rows, np.float64, copy=True).reshape(-1, 8)
    if classes is not None:
        r = r[np.isin(r[:, 7], np.asarray(list(classes), np.float64))]
    if not np.isfinite(r).all():
        raise ValueError(f"{what}: NaN or infinity")
    if len(r) and len(np.unique(r[:, :2], axis=0)) != len(r):
        raise ValueError(f"{what}: duplicate (frame, id)")
    if ((r[:, 4] <= r[:, 2]) | (r[:, 5] <= r[:, 3])).any():
        raise ValueError(f"{what}: a box with x2 <= x1 or y2 <= y1")
    return r[np.lexsort((r[:, 1], r[:, 0]))] if len(r) else r


class _Pair:
    """The packed form of one pair: rows by (frame, id), the evaluated frames (union of both sides, rising), row offsets per
    frame and dense ids by np.unique per side."""

    def __init__(self, gt, tr):
        self.gt, self.tr = gt, tr
        self.frames = np.unique(np.concatenate([gt[:, 0], tr[:, 0]]))
        self.gt_off = np.searchsorted(gt[:, 0], self.frames, "left").tolist() + [len(gt)]
        self.tr_off = np.searchsorted(tr[:, 0], self.frames, "left").tolist() + [len(tr)]
        self.gt_off, self.tr_off = np.asarray(self.gt_off, np.int64), np.asarray(self.tr_off, np.int64)
        self.gt_id = np.unique(gt[:, 1], return_inverse=True)[1].reshape(-1).astype(np.int64)
        self.tr_id = np.unique(tr[:, 1], return_inverse=True)[1].reshape(-1).astype(np.int64)
        self.n_gid = int(self.gt_id.max()) + 1 if len(gt) else 0
        self.n_tid = int(self.tr_id.max()) + 1 if len(tr) else 0
        self.cnt_g = np.bincount(self.gt_id, minlength=self.n_gid).astype(np.int64)
        self.cnt_t = np.bincount(self.tr_id, minlength=self.n_tid).astype(np.int64)
        self.frame_of = np.repeat(np.arange(len(self.frames)), np.diff(self.gt_off))       # per ground-truth row


def _matched_ids(p: _Pair, idx):
    """dense tracker id of every ground-truth row's match (0 where there is none)"""
    if not len(p.tr):
        return np.zeros(len(p.gt), np.int64)
    return p.tr_id[np.where(idx >= 0, p.tr_off[p.frame_of] + idx, 0)]


def _hota(p: _Pair, idx, s) -> dict:
    n_gt, n_tr, nt1 = len(p.gt), len(p.tr), max(p.n_tid, 1)
    t = _matched_ids(p, idx)
    vec = {k: [] for k in HOTA_FIELDS}
    for alpha in ALPHAS:
        m = (idx >= 0) & (s >= alpha - EPS)
        tp = int(np.count_nonzero(m))
        fn, fp = n_gt - tp, n_tr - tp
        det_a, det_re, det_pr = tp / max(1, tp + fn + fp), tp / max(1, tp + fn), tp / max(1, tp + fp)
        loc_a = max(1e-10, _seq(s[m])) / max(1e-10, float(tp))
        key, c = np.unique(p.gt_id[m] * nt1 + t[m], return_counts=True)                  # the id pairs with matches, (g, t) rising
        c, cg, ct = c.astype(np.float64), p.cnt_g[key // nt1], p.cnt_t[key % nt1]
        ass_a = _seq(c * (c / np.maximum(1, cg + ct - c))) / max(1, tp)
        ass_re = _seq(c * (c / np.maximum(1, cg))) / max(1, tp)
        ass_pr = _seq(c * (c / np.maximum(1, ct))) / max(1, tp)
        for k, v in zip(HOTA_FIELDS, (np.sqrt(det_a * ass_a), det_a, ass_a, det_re, det_pr, ass_re, ass_pr, loc_a)):
            vec[k].append(float(v))
    out = {}
    for k in HOTA_FIELDS:
        out[k] = _seq(vec[k]) / 19.0
        out[k + "_alpha"] = vec[k]
    out["HOTA(0)"], out["LocA(0)"] = vec["HOTA"][0], vec["LocA"][0]
    return out


def _clear(p: _Pair, idx, s) -> dict:
    n_gt, n_tr = len(p.gt), len(p.tr)
    m = idx >= 0
    tp = int(np.count_nonzero(m))
    fn, fp = n_gt - tp, n_tr - tp
    # the walk's tables replayed from the record: the matched rows by (ground-truth id, frame)
    g, t = p.gt_id[m], _matched_ids(p, idx)[m]
    both = (np.diff(p.gt_off) > 0) & (np.diff(p.tr_off) > 0)
    proc = (np.cumsum(both) - 1)[p.frame_of[m]]                   # number of the processed frame of every matched row
    order = np.lexsort((proc, g))
    g, t, proc = g[order], t[order], proc[order]
    same = g[1:] == g[:-1]
    idsw = int(np.count_nonzero(same & (t[1:] != t[:-1])))        # prev: the last tracker id the ground-truth id was ever matched to
    starts = np.ones(len(g), bool)
    starts[1:] = ~(same & (proc[1:] == proc[:-1] + 1))            # prev_t was none: not matched in the processed frame before
    n_g = np.bincount(g[starts], minlength=p.n_gid)
    share = np.bincount(p.gt_id[m], minlength=p.n_gid) / np.maximum(1, p.cnt_g)
    mt, ml = int(np.count_nonzero(share > 0.8)), int(np.count_nonzero(share < 0.2))
    return {"TP": tp, "FN": fn, "FP": fp, "IDSW": idsw, "MOTA": (tp - fp - idsw) / max(1, tp + fn), "MOTP": _seq(s[m]) / max(1, tp),
            "MT": mt, "PT": p.n_gid - mt - ml, "ML": ml, "Frag": int(np.maximum(0, n_g - 1).sum())}


def pack(pairs):
    """The arguments of TrackerEngine.mot_eval for a list of _Pair."""
    cat = lambda parts, dt: np.concatenate([np.asarray(x, dt) for x in parts]) if parts else np.zeros(0, dt)
    frame_off, gt_off, tr_off, g_at, t_at = [0], [np.zeros(1, np.int64)], [np.zeros(1, np.int64)], 0, 0
    for p in pairs:
        frame_off.append(frame_off[-1] + len(p.frames))
        gt_off.append(p.gt_off[1:] + g_at)
        tr_off.append(p.tr_off[1:] + t_at)
        g_at, t_at = g_at + len(p.gt), t_at + len(p.tr)
    return (np.asarray(frame_off, np.int32), cat(gt_off, np.int32), cat(tr_off, np.int32), cat([p.gt_id for p in pairs], np.int32),
            cat([p.tr_id for p in pairs], np.int32), np.concatenate([p.gt[:, 2:6] for p in pairs], 0), np.concatenate([p.tr[:, 2:6] for p in pairs], 0),
            np.asarray([p.n_gid for p in pairs], np.int32), np.asarray([p.n_tid for p in pairs], np.int32))


def _pairs(gt_rows, tracker_rows, thr, classes):
    """-> the list of _Pair of a call: tracker_rows is one row set or a list of them, each scored against gt_rows"""
    if not (0.0 < float(thr) <= 1.0):
        raise ValueError("thr must be in (0, 1]")
    many = isinstance(tracker_rows, (list, tuple)) and (len(tracker_rows) == 0 or np.ndim(tracker_rows[0]) >= 2)
    sets = list(tracker_rows) if many else [tracker_rows]
    if not sets:
        return []
    gt = _rows(gt_rows, "ground truth", classes)
    return [_Pair(gt, _rows(t, f"tracker rows {k}", classes)) for k, t in enumerate(sets)]


def _identity_figures(idtp: int, n_gt: int, n_tr: int) -> dict:
    idfn, idfp = n_gt - idtp, n_tr - idtp
    return {"IDTP": int(idtp), "IDFN": int(idfn), "IDFP": int(idfp), "IDF1": idtp / max(1, idtp + 0.5 * idfp + 0.5 * idfn),
            "IDP": idtp / max(1, idtp + idfp), "IDR": idtp / max(1, idtp + idfn)}


def _identity(pairs, engine, thr, want_pot):
    """one engine call for all pairs -> (one dict of the six figures per pair, one record dict per pair or None)"""
    out = engine.mot_identity(*pack(pairs), thr=float(thr), want_pot=want_pot)
    idtp, match = out[:2]
    res, rec, g_at, c_at = [], [], 0, 0
    for k, p in enumerate(pairs):
        res.append(_identity_figures(int(idtp[k]), len(p.gt), len(p.tr)))
        if want_pot:
            m = np.asarray(match[g_at:g_at + p.n_gid])
            gid, tid = np.unique(p.gt[:, 1]), np.unique(p.tr[:, 1])
            rec.append({"gt_to_tr": {float(gid[g]): float(tid[m[g]]) for g in np.nonzero(m >= 0)[0]},
                        "pot": np.asarray(out[2][c_at:c_at + p.n_gid * p.n_tid]).reshape(p.n_gid, p.n_tid)})
        g_at, c_at = g_at + p.n_gid, c_at + p.n_gid * p.n_tid
    return res, rec


def identity_full(gt_rows, tracker_rows_or_list, engine, thr: float = 0.5, classes=None):
    """-> (one dict per pair as `identity` returns it, one record dict per pair: `gt_to_tr`, the reported matching as a dict
    original ground-truth id -> original tracker id (the matched ids only; ids whose pair never passes `thr` are left out), and
    `pot` [ground-truth ids, tracker ids] int32 in np.unique order of the ids)."""
    pairs = _pairs(gt_rows, tracker_rows_or_list, thr, classes)
    return _identity(pairs, engine, thr, True) if pairs else ([], [])


def identity(gt_rows, tracker_rows_or_list, engine, thr: float = 0.5, classes=None):
    """The identity metrics (docs/MOTEVAL.md §1 "Identity"): one dict per pair with IDTP, IDFN, IDFP (ints) and IDF1, IDP, IDR
    (floats), through a single device call.  A box pair counts where its similarity is at least `thr`."""
    pairs = _pairs(gt_rows, tracker_rows_or_list, thr, classes)
    return _identity(pairs, engine, thr, False)[0] if pairs else []


def evaluate_full(gt_rows, tracker_rows, engine, thr: float = 0.5, classes=None, metrics=None, want_ga: bool = False, identity: bool = False):
    """-> (one dict of metrics per pair, one record dict per pair: hota_idx, hota_s, clear_idx, clear_s per ground-truth row by
    (frame, id), and GA with want_ga).  tracker_rows: one row set or a list of them, each scored against gt_rows.  identity: a
    second engine call adds IDTP, IDFN, IDFP, IDF1, IDP, IDR to every dict."""
    for name in metrics or ():
        if name in REFUSED:
            raise ValueError(f"{name}: identity metrics are not selected with metrics=; pass identity=True or call moteval.identity (docs/MOTEVAL.md)")
    pairs = _pairs(gt_rows, tracker_rows, thr, classes)
    if not pairs:
        return [], []
    out = engine.mot_eval(*pack(pairs), thr=float(thr), want_ga=want_ga)
    hi, hs, ci, cs = out[:4]
    res, rec, at, ga_at = [], [], 0, 0
    for p in pairs:
        sl = slice(at, at + len(p.gt))
        at += len(p.gt)
        m = {"gt_rows": len(p.gt), "tracker_rows": len(p.tr), "gt_ids": p.n_gid, "tracker_ids": p.n_tid, "frames": len(p.frames), "thr": float(thr)}
        m.update(_hota(p, hi[sl], hs[sl]))
        m.update(_clear(p, ci[sl], cs[sl]))
        res.append(m)
        r = {"hota_idx": hi[sl], "hota_s": hs[sl], "clear_idx": ci[sl], "clear_s": cs[sl]}
        if want_ga:
            r["GA"] = out[4][ga_at:ga_at + p.n_gid * p.n_tid].reshape(p.n_gid, p.n_tid)
            ga_at += p.n_gid * p.n_tid
        rec.append(r)
    if identity:
        for m, more in zip(res, _identity(pairs, engine, thr, False)[0]):
            m.update(more)
    return res, rec


def evaluate(gt_rows, tracker_rows_or_list, engine, thr: float = 0.5, classes=None, metrics=None, identity: bool = False):
    """One dict of metrics per pair (a list, also for a single tracker row set), through a single device call: the 19-vectors
    `<name>_alpha` as lists, their means HOTA, DetA, AssA, DetRe, DetPr, AssRe, AssPr, LocA, HOTA(0), LocA(0), and CLEAR's TP, FN,
    FP, IDSW, MOTA, MOTP, MT, PT, ML, Frag at the similarity threshold `thr`.  classes: keep only the rows of these classes.
    identity: a second device call adds the identity metrics IDTP, IDFN, IDFP, IDF1, IDP, IDR at the same `thr`."""
    return evaluate_full(gt_rows, tracker_rows_or_list, engine, thr, classes, metrics, identity=identity)[0]


def read_labels(path: str) -> np.ndarray:
    """The rows of a labels file as cli.LabelsWriter and gsi.write_labels write it: `frame cls id conf x1 y1 x2 y2 -1 -1 -1 -1`."""
    out = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            v = line.split()
            if not v:
                continue
            if len(v) < 8:
                raise ValueError(f"{path}:{n}: expected `frame cls id conf x1 y1 x2 y2 ...`")
            out.append([float(v[0]), float(v[2]), float(v[4]), float(v[5]), float(v[6]), float(v[7]), float(v[3]), float(v[1])])
    return np.asarray(out, np.float64).reshape(-1, 8)


def write_metrics(path: str, metrics) -> None:
    with open(path, "w") as f:
        json.dump(metrics, f, indent=1)
        f.write("\n")


def max_boxes() -> int:
    return int(_lib.load().ss_mot_max_boxes())


def max_ids() -> int:
    """the most ids one side of a pair may have in `identity`"""
    return int(_lib.load().ss_mot_max_ids())
