"""docs/MOTEVAL.md §1 "Identity" restated on the CPU: the counts `pot`, TrackEval's (G+T)² formulation of the Identity metric as this
project restates it (`full`), the reduction to a maximum-weight matching of G x T (`reduced`), and the six figures.  NumPy and
scipy.optimize.linear_sum_assignment; neither the device nor strongsort_yolo_amd.moteval.  Pair and similarity are
tests/moteval_ref.py's.

`crowd` makes dense, tie-heavy input: every frame draws `boxes` ids a side and places all of them as jittered copies of one base box
(80 x 160 px, corners moved by whole quarter pixels, uniformly within +-JITTER_Q quarter pixels = +-32 px).  Measured on the CPU
over 24 frames of 256 x 256 boxes (seed 0): 40.3 % of a frame's cells pass thr = 0.5 (between a third and a half, as intended);
with 1100 x 1030 ids the counts run from 0 to 7 and 43 % of them are positive, with 4096 x 3072 ids and 40 frames from 0 to 4."""
from __future__ import annotations

import numpy as np
from scipy.optimize import linear_sum_assignment

from tests.moteval_ref import EPS, Pair, similarity

JITTER_Q = 128                                          # quarter pixels: corners move by up to +-32 px


def pot_of(gt, tr, thr: float = 0.5):
    """-> (pot [n_gid, n_tid] int64: the frames in which both ids have a box with S >= thr - eps, the Pair)"""
    p = Pair(gt, tr)
    pot = np.zeros((p.n_gid, p.n_tid), np.int64)
    for f in range(len(p.frames)):
        a, b = p.frame(f)
        if a.stop > a.start and b.stop > b.start:
            S = similarity(p.gt[a, 2:6], p.tr[b, 2:6])
            pot[np.ix_(p.gt_id[a], p.tr_id[b])] += S >= thr - EPS       # ids are unique in a frame: one addend per cell and frame
    return pot, p


def full(pot, cnt_g, cnt_t):
    """TrackEval's Identity construction: a (G+T)² matrix of false negatives plus false positives with a dummy column per
    ground-truth id, a dummy row per tracker id and 1e10 walls -> (IDTP, IDFN, IDFP)"""
    pot, cnt_g, cnt_t = np.asarray(pot, np.float64), np.asarray(cnt_g, np.float64), np.asarray(cnt_t, np.float64)
    G, T = pot.shape
    fn, fp = np.zeros((G + T, G + T)), np.zeros((G + T, G + T))
    fp[G:, :T], fn[:G, T:] = 1e10, 1e10
    for g in range(G):
        fn[g, :T] = cnt_g[g]
        fn[g, T + g] = cnt_g[g]
    for t in range(T):
        fp[:G, t] = cnt_t[t]
        fp[G + t, t] = cnt_t[t]
    fn[:G, :T] -= pot
    fp[:G, :T] -= pot
    r, c = linear_sum_assignment(fn + fp)
    idfn, idfp = int(fn[r, c].sum()), int(fp[r, c].sum())
    return int(cnt_g.sum()) - idfn, idfn, idfp


def reduced(pot):
    """-> W, the maximum weight of a one-to-one matching of ground-truth ids to tracker ids under pot (SciPy on -pot)"""
    pot = np.asarray(pot, np.int64)
    if not pot.size:
        return 0
    r, c = linear_sum_assignment(-pot)
    return int(pot[r, c].sum())


def figures(idtp: int, n_gt: int, n_tr: int) -> dict:
    idfn, idfp = n_gt - idtp, n_tr - idtp
    return {"IDTP": int(idtp), "IDFN": int(idfn), "IDFP": int(idfp), "IDF1": idtp / max(1, idtp + 0.5 * idfp + 0.5 * idfn),
            "IDP": idtp / max(1, idtp + idfp), "IDR": idtp / max(1, idtp + idfn)}


def identity(gt, tr, thr: float = 0.5) -> dict:
    pot, p = pot_of(gt, tr, thr)
    return figures(reduced(pot), len(p.gt), len(p.tr))


def crowd(rng, n_gid: int, n_tid: int, frames: int, boxes: int = 256, meet: float = 1.0):
    """-> (gt, tracker) rows: `frames` frames, each with min(boxes, ids) ids a side drawn without replacement, every box a jittered
    copy of one base box on a quarter-pixel grid.  meet < 1: only the first share `meet` of each side's ids ever appears in a frame
    with the other side; the others get a frame of their own side each, so their rows and columns of pot are zero."""
    assert boxes <= 256
    mg, mt = max(1, int(n_gid * meet)), max(1, int(n_tid * meet))
    out = ([], [])
    for f in range(frames):
        for side, n in ((0, mg), (1, mt)):
            k = min(boxes, n)
            ids = rng.choice(n, k, replace=False)
            q = rng.integers(-JITTER_Q, JITTER_Q + 1, (k, 4)) / 4.0
            r = np.zeros((k, 8))
            r[:, 0], r[:, 1], r[:, 6] = f, ids + 1 + 10000 * side, 1.0
            r[:, 2], r[:, 3], r[:, 4], r[:, 5] = 400.0 + q[:, 0], 200.0 + q[:, 1], 480.0 + q[:, 2], 360.0 + q[:, 3]
            out[side].append(r)
    # every id exists: ids that no frame drew, and with meet < 1 the ones that never meet the other side, get one row in a frame
    # of their own side (the ground truth's after the sequence, the tracker's after those)
    for side, n in ((0, n_gid), (1, n_tid)):
        seen = np.unique(np.concatenate(out[side])[:, 1]) if out[side] else np.zeros(0)
        rest = np.setdiff1d(np.arange(n) + 1 + 10000 * side, seen)
        for k0 in range(0, len(rest), boxes):
            part = rest[k0:k0 + boxes]
            r = np.zeros((len(part), 8))
            r[:, 0], r[:, 1], r[:, 6] = frames + 1000 * (side + 1) + k0 // boxes, part, 1.0
            r[:, 2:6] = [400.0, 200.0, 480.0, 360.0]
            out[side].append(r)
    return np.concatenate(out[0], 0), np.concatenate(out[1], 0)
