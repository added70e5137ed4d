"""Scoring detections against ground truth: COCO's AP@[.50:.95], AP50, AP75, AP by object size and AR at 1 / 10 / 100 detections
(docs/DETEVAL.md).

Rows are the float64 [N, 8] rows of `strongsort_yolo_amd.gsi` / `moteval`: frame, id, x1, y1, x2, y2, conf, cls.  The frame number is
the image; a ground-truth row with id < 0 is a crowd region; of a detection row only conf (the score) is read.  With
similarity="probiou" rows are [N, 9]: frame, id, cx, cy, w, h, theta, conf, cls, as `<name>_labels_obb.txt` holds them.  The order of
every class's detections by score, the greedy matching per (image, class) cell, area range and threshold and the accumulation into
`precision` [T,R,K,A,M] and `recall` [T,K,A,M] run on the device (csrc/ss_ap.hip) in one call; the host half here packs the rows by
(class, image, input index) and takes the means.  There is no CPU fallback: without the library or a device `evaluate` raises as the
rest of the package does.  tests/deteval_ref.py restates the whole of it; the device's ranks, match record and arrays equal it bit
for bit.  Parity with pycocotools is unpinned (docs/DETEVAL.md §5)."""
from __future__ import annotations

import numpy as np

from . import lib as _lib
from .moteval import _seq, read_labels, write_metrics  # noqa: F401  (the labels reader and the JSON writer are moteval's)

FIGURES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0.0, 1.0, 101)
AREAS = np.array([[0.0, 1e10], [0.0, 32.0 ** 2], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]])


def _rows(rows, what: str, obb: bool, classes=None) -> np.ndarray:
    w = 9 if obb else 8
    r = np.array(rows, np.float64, copy=True).reshape(-1, w)
    if classes is not None:
        r = r[np.isin(r[:, w - 1], np.asarray(list(classes), np.float64))]
    if not np.isfinite(r).all():
        raise ValueError(f"{what}: NaN or infinity")
    if not obb and ((r[:, 4] <= r[:, 2]) | (r[:, 5] <= r[:, 3])).any():
        raise ValueError(f"{what}: a box with x2 <= x1 or y2 <= y1")
    if obb and ((r[:, 4] <= 0) | (r[:, 5] <= 0)).any():
        raise ValueError(f"{what}: a box with w <= 0 or h <= 0")
    return r


class _Pack:
    """Both row sets by (class, image, input index), the cells that hold a row of either side and the offsets ss_ap_eval takes."""

    def __init__(self, gt, dt, obb):
        w = 9 if obb else 8
        self.classes = np.unique(np.concatenate([gt[:, w - 1], dt[:, w - 1]]))
        self.images = np.unique(np.concatenate([gt[:, 0], dt[:, 0]]))
        n_img = max(len(self.images), 1)
        key = lambda r: np.searchsorted(self.classes, r[:, w - 1]).astype(np.int64) * n_img + np.searchsorted(self.images, r[:, 0])
        gkey, dkey = key(gt), key(dt)
        self.g_order, self.d_order = np.argsort(gkey, kind="stable"), np.argsort(dkey, kind="stable")
        gkey, dkey = gkey[self.g_order], dkey[self.d_order]
        cells = np.unique(np.concatenate([gkey, dkey]))
        self.cell_gt_off = np.concatenate([np.searchsorted(gkey, cells, "left"), [len(gkey)]]).astype(np.int32)
        self.cell_det_off = np.concatenate([np.searchsorted(dkey, cells, "left"), [len(dkey)]]).astype(np.int32)
        self.class_cell_off = np.searchsorted(cells // n_img, np.arange(len(self.classes) + 1), "left").astype(np.int32)
        self.cell_image = (cells % n_img).astype(np.int32)
        nb = 5 if obb else 4
        self.gt_boxes, self.det_boxes = np.ascontiguousarray(gt[self.g_order, 2:2 + nb]), np.ascontiguousarray(dt[self.d_order, 2:2 + nb])
        self.gt_crowd = (gt[self.g_order, 1] < 0).astype(np.int32)
        self.det_scores = np.ascontiguousarray(dt[self.d_order, w - 2])


def _mean(x) -> float:
    x = np.asarray(x, np.float64).ravel()
    x = x[x > -1]
    return _seq(x) / len(x) if len(x) else -1.0


def figures(precision, recall, iou_thrs) -> dict:
    """The twelve statistics and AP_class from the arrays (docs/DETEVAL.md §1 "Figures")."""
    n_areas, n_max = precision.shape[3], precision.shape[4]
    t75 = np.nonzero(np.asarray(iou_thrs) == 0.75)[0]
    ap = lambda a: _mean(precision[:, :, :, a, -1]) if a < n_areas else -1.0
    ar = lambda a, m: _mean(recall[:, :, a, m]) if a < n_areas and m < n_max else -1.0
    out = {"AP": ap(0), "AP50": _mean(precision[0, :, :, 0, -1]), "AP75": _mean(precision[t75, :, :, 0, -1]) if len(t75) else -1.0,
           "APs": ap(1), "APm": ap(2), "APl": ap(3), "AR1": ar(0, 0), "AR10": ar(0, 1), "AR100": ar(0, n_max - 1),
           "ARs": ar(1, n_max - 1), "ARm": ar(2, n_max - 1), "ARl": ar(3, n_max - 1)}
    out["AP_class"] = [_mean(precision[:, :, k, 0, -1]) for k in range(precision.shape[2])]
    return out


def _run(gt_rows, det_rows, engine, similarity, iou_thrs, rec_thrs, areas, max_dets, classes, full):
    """checks, packing, the device call, the figures -> (figures, record or None); the ranks and the match record are asked of the
    device only with `full`"""
    if similarity not in ("iou", "probiou"):
        raise ValueError("similarity must be 'iou' or 'probiou'")
    obb = similarity == "probiou"
    iou_thrs = IOU_THRS if iou_thrs is None else np.asarray(iou_thrs, np.float64).reshape(-1)
    rec_thrs = REC_THRS if rec_thrs is None else np.asarray(rec_thrs, np.float64).reshape(-1)
    areas = AREAS if areas is None else np.asarray(areas, np.float64).reshape(-1, 2)
    max_dets = np.asarray([int(m) for m in max_dets], np.int32)
    if not ((iou_thrs > 0.0) & (iou_thrs <= 1.0)).all():
        raise ValueError("iou_thrs must be in (0, 1]")
    gt, dt = _rows(gt_rows, "ground truth", obb, classes), _rows(det_rows, "detections", obb, classes)
    if obb and (gt[:, 1] < 0).any():
        raise ValueError("a crowd region cannot be scored with probiou")
    if not len(gt) and not len(dt):
        raise ValueError("nothing to score: no ground-truth row and no detection row")
    p = _Pack(gt, dt, obb)
    got = engine.ap_eval(1 if obb else 0, p.class_cell_off, p.cell_image, p.cell_gt_off, p.cell_det_off, p.gt_boxes, p.gt_crowd, p.det_boxes,
                         p.det_scores, iou_thrs, rec_thrs, areas, max_dets, want_rank=full, want_record=full)
    precision, recall = got[:2]
    out = figures(precision, recall, iou_thrs)
    out["classes"] = [float(c) for c in p.classes]
    if not full:
        return out, None
    rank, match, ignored = got[2:]
    rank_in = np.zeros(len(dt), np.int64)
    rank_in[p.d_order] = rank
    cell_of = np.repeat(np.arange(len(p.cell_image)), np.diff(p.cell_det_off))
    by = np.lexsort((rank, cell_of))                                       # packed detections by (cell, rank)
    first = p.cell_det_off[:-1][cell_of[by]]
    kept = by[np.arange(len(by)) - first < int(max_dets[-1])]
    return out, {"precision": precision, "recall": recall, "rank": rank_in, "kept_rows": p.d_order[kept].astype(np.int64), "match": match,
                 "ignored": ignored.astype(bool)}


def evaluate_full(gt_rows, det_rows, engine, similarity: str = "iou", iou_thrs=None, rec_thrs=None, areas=None, max_dets=(1, 10, 100), classes=None):
    """-> (the dict `evaluate` returns, a record dict: `precision` [T,R,K,A,M], `recall` [T,K,A,M], `rank` per detection row (after
    the class filter, in input order: its place in its class's order), `kept_rows` (the detection rows that are matched: cell after
    cell by (class, image), by position, cut at max_dets[-1]) and `match` / `ignored` [A,T,kept]: the matched ground-truth row's
    index within its cell in input order or -1, and the ignored bit)."""
    return _run(gt_rows, det_rows, engine, similarity, iou_thrs, rec_thrs, areas, max_dets, classes, True)


def evaluate(gt_rows, det_rows, engine, similarity: str = "iou", iou_thrs=None, rec_thrs=None, areas=None, max_dets=(1, 10, 100), classes=None) -> dict:
    """The twelve COCO figures (AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl; -1.0 where nothing qualifies),
    `AP_class` and `classes` (np.unique order), through a single device call.  classes: keep only the rows of these classes."""
    return _run(gt_rows, det_rows, engine, similarity, iou_thrs, rec_thrs, areas, max_dets, classes, False)[0]


def read_labels_obb(path: str) -> np.ndarray:
    """The rows of an oriented labels file as cli.LabelsWriter writes `<name>_labels_obb.txt`: `frame cls id conf cx cy w h theta`
    -> [N, 9] frame, id, cx, cy, w, h, theta, conf, cls."""
    out = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            v = line.split()
            if not v:
                continue
            if len(v) < 9:
                raise ValueError(f"{path}:{n}: expected `frame cls id conf cx cy w h theta`")
            out.append([float(v[0]), float(v[2]), float(v[4]), float(v[5]), float(v[6]), float(v[7]), float(v[8]), float(v[3]), float(v[1])])
    return np.asarray(out, np.float64).reshape(-1, 9)


def caps() -> dict:
    """the library's caps: ground-truth rows a cell, detections a cell, the largest max_dets entry, detections a call"""
    L = _lib.load()
    return {"gts": int(L.ss_ap_max_gts()), "cell_dets": int(L.ss_ap_max_cell_dets()), "keep": int(L.ss_ap_max_keep()), "dets": int(L.ss_ap_max_dets())}
