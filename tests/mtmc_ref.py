"""Restatement of the multi-camera linking (docs/MTMC.md): the track bank, the distances, the conflicts and the constrained
average-linkage clustering, in NumPy, one rounded operation at a time.  These semantics are this project's own; the device code
(csrc/ss_mtmc.hip) is held to these bits.
"""
from __future__ import annotations

import numpy as np

FEAT_DIM, MAX_TRACKS, MAX_DETS = 512, 256, 128


def butterfly(p: np.ndarray) -> float:
    """Σ p over 512 f64 values in the device's order: lane l of 64 adds k = l, l + 64, ... in rising order, then the xor butterfly
    with offsets 32, 16, 8, 4, 2, 1."""
    m = np.asarray(p, np.float64).reshape(8, 64)
    v = m[0].copy()
    for j in range(1, 8):
        v = v + m[j]
    while len(v) > 1:
        h = len(v) // 2
        v = v[:h] + v[h:]
    return float(v[0])


def unit_row(f: np.ndarray):
    """The f64 unit row of a raw f32 feature, or None when its squared norm is zero or not finite."""
    d = np.asarray(f, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        s = butterfly(d * d)
    if not np.isfinite(s) or s == 0.0:
        return None
    return d / np.sqrt(s)


class Bank:
    """One stream's bank: per id the f64 sum of the unit rows, the count, first and last frame and the last class."""

    def __init__(self, max_ids: int):
        self.max_ids = int(max_ids)
        self.sum, self.n, self.first, self.last, self.cls = {}, {}, {}, {}, {}
        self.frame, self.err = 0, False

    def update(self, rows, feats):
        """One frame: rows [n, 8] (x1, y1, x2, y2, id, cls, conf, det_idx) as a tracker leaves them, feats [MAX_DETS, 512] raw f32.
        rows None: the stream sits the frame out."""
        if rows is None:
            return
        rows = np.asarray(rows, np.float32).reshape(-1, 8)[:MAX_TRACKS]
        for r in rows:
            det, tid = float(r[7]), float(r[4])
            if not (0.0 <= det < MAX_DETS) or not (1.0 <= tid < 2147483648.0):
                continue
            tid = int(tid)
            if tid > self.max_ids:
                self.err = True
                continue
            u = unit_row(feats[int(det)])
            if u is None:
                continue
            if tid not in self.n:
                self.sum[tid], self.n[tid], self.first[tid] = np.zeros(FEAT_DIM), 0, self.frame
            self.sum[tid] = self.sum[tid] + u
            self.n[tid] += 1
            self.last[tid] = self.frame
            self.cls[tid] = int(r[5])
        self.frame += 1

    def table(self) -> dict:
        ids = sorted(self.n)
        desc = np.zeros((len(ids), FEAT_DIM), np.float32)
        for i, t in enumerate(ids):
            s = self.sum[t]
            with np.errstate(invalid="ignore", divide="ignore"):
                desc[i] = (s / np.sqrt(butterfly(s * s))).astype(np.float32)
        col = lambda d: np.array([d[t] for t in ids], np.int32)
        return {"ids": np.array(ids, np.int32), "n": col(self.n), "first": col(self.first), "last": col(self.last), "cls": col(self.cls), "desc": desc}


def tracklets(tables):
    """The cameras' tables as one tracklet list in rising (camera, local id) order -> desc [T, 512], cam, ids, first, last, n [T]."""
    cam = np.concatenate([np.full(len(t["ids"]), c, np.int32) for c, t in enumerate(tables)]) if tables else np.zeros(0, np.int32)
    cat = lambda k, dt: np.concatenate([np.asarray(t[k], dt) for t in tables]) if tables else np.zeros(0, dt)
    desc = np.concatenate([np.asarray(t["desc"], np.float32).reshape(-1, FEAT_DIM) for t in tables]) if tables else np.zeros((0, FEAT_DIM), np.float32)
    return desc, cam, cat("ids", np.int32), cat("first", np.int32), cat("last", np.int32), cat("n", np.int32)


def dist64(desc) -> np.ndarray:
    """D[i][j] = 1 - desc_i . desc_j in f64, i < j; zero elsewhere."""
    d = np.asarray(desc, np.float32).astype(np.float64)
    return np.triu(1.0 - d @ d.T, 1)


def dist_exact(desc) -> np.ndarray:
    """The same with every product and partial sum carried out one at a time in f64 over rising k (for exact operands)."""
    d = np.asarray(desc, np.float32).astype(np.float64)
    acc = np.zeros((len(d), len(d)))
    for k in range(d.shape[1]):
        acc = acc + np.outer(d[:, k], d[:, k])
    return np.triu(1.0 - acc, 1)


def conflicts(cam, first, last, n, min_rows: int = 1) -> np.ndarray:
    cam, first, last, n = (np.asarray(v, np.int64) for v in (cam, first, last, n))
    c = (cam[:, None] == cam[None, :]) & (first[:, None] <= last[None, :]) & (first[None, :] <= last[:, None])
    small = n < min_rows
    c |= small[:, None] | small[None, :]
    np.fill_diagonal(c, False)
    return c


def cluster(D, cam, first, last, n, thr: float, min_rows: int = 1):
    """Constrained UPGMA on the f32 distances D [T, T] (i < j read) -> (global ids int32 [T], merges [(a, b, height)])."""
    T = len(cam)
    d = np.asarray(D, np.float32).astype(np.float64).copy()
    d = np.triu(d, 1)
    d = d + d.T
    conf = conflicts(cam, first, last, n, min_rows)
    live, size, root = np.ones(T, bool), np.ones(T, np.float64), np.arange(T)
    upper = np.triu(np.ones((T, T), bool), 1)
    merges = []
    while True:
        ok = upper & live[:, None] & live[None, :] & ~conf & (d < thr)
        if not ok.any():
            break
        m = np.where(ok, d, np.inf)
        a, b = divmod(int(np.argmin(m)), T)                    # the first minimum in row-major order: the smallest (d, a, b)
        merges.append((a, b, float(d[a, b])))
        new = (size[a] * d[a] + size[b] * d[b]) / (size[a] + size[b])
        keep = live.copy()
        keep[[a, b]] = False
        d[a, keep] = new[keep]
        d[keep, a] = new[keep]
        conf[a] |= conf[b]
        conf[:, a] |= conf[:, b]
        size[a] += size[b]
        live[b] = False
        root[root == b] = a
    order = {r: i + 1 for i, r in enumerate(sorted(set(root.tolist())))}
    return np.array([order[r] for r in root.tolist()], np.int32), merges


def link(tables, thr: float = 0.2, min_rows: int = 1, D=None):
    """One {local id: global id} dict per camera; D: the f32 distances to cluster on (default: f64 distances rounded to f32)."""
    desc, cam, ids, first, last, n = tracklets(tables)
    if D is None:
        D = dist64(desc).astype(np.float32)
    gid, merges = cluster(D, cam, first, last, n, thr, min_rows)
    return [{int(i): int(g) for i, g, c2 in zip(ids, gid, cam) if c2 == c} for c in range(len(tables))], merges
