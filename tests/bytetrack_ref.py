"""CPU reference of the BYTE tracker family (docs/BYTETRACK.md §1, decisions B-01..): a NumPy / float64 restatement of one
stream, written in the operation order of csrc/ss_byte.hip so that the device reproduces it bit for bit.

Not a conftest and not a test module: imported by tests/test_bytetrack_cpu.py and tests/test_gpu_bytetrack.py.

    ref = ByteTrackRef(ByteTrackConfig(kalman="xyah"))
    rows = ref.update(dets)      # dets [N,6] float32 x1,y1,x2,y2,score,cls -> float32 [M,8] x1,y1,x2,y2,id,cls,score,det_idx

The Kalman arithmetic mirrors ss_kf_initiate / ss_kf_predict / ss_kf_update (csrc/ss_kalman.h) with conf = 0 for "xyah" and with
the xywh noise model for "xywh" line by line; every fused multiply-add of the device is an exactly rounded fma here (`_fma`).
"""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np
from scipy.optimize import linear_sum_assignment

from strongsort_yolo_amd.config import ByteTrackConfig

TRACKED, LOST, REMOVED = 1, 2, 3


def _fma(a: float, b: float, c: float) -> float:
    """a * b + c rounded once (IEEE fma): exact rational arithmetic on the binary fractions, one correctly rounded division."""
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    nc, dc = c.as_integer_ratio()
    n, d = na * nb, da * db
    if n == 0 and nc == 0:
        return a * b + c                       # the sign of an exact zero as the hardware gives it
    if d >= dc:
        return (n + nc * (d // dc)) / d        # denominators are powers of two: d // dc is exact
    return (n * (dc // d) + nc) / dc


# ---- Kalman filters (8 states, f64) ------------------------------------------------------------------------------
def _initiate_sd(z, xywh, wp, wv):
    if xywh:
        w, h = z[2], z[3]
        return [2.0 * wp * w, 2.0 * wp * h, 2.0 * wp * w, 2.0 * wp * h, 10.0 * wv * w, 10.0 * wv * h, 10.0 * wv * w, 10.0 * wv * h]
    h = z[3]
    return [2.0 * wp * h, 2.0 * wp * h, 1e-2, 2.0 * wp * h, 10.0 * wv * h, 10.0 * wv * h, 1e-5, 10.0 * wv * h]


def kf_initiate(z, xywh, wp, wv):
    mean = [float(z[0]), float(z[1]), float(z[2]), float(z[3]), 0.0, 0.0, 0.0, 0.0]
    sd = _initiate_sd(mean, xywh, wp, wv)
    cov = [0.0] * 64
    for i in range(8):
        cov[i * 8 + i] = sd[i] * sd[i]
    return mean, cov


def kf_predict(mean, cov, xywh, wp, wv):
    if xywh:
        w, h = mean[2], mean[3]
        sd = [wp * w, wp * h, wp * w, wp * h, wv * w, wv * h, wv * w, wv * h]
    else:
        h = mean[3]
        sp, sv = wp * h, wv * h
        sd = [sp, sp, 1e-2, sp, sv, sv, 1e-5, sv]
    P = list(cov)
    for i in range(8):
        for j in range(4):
            P[i * 8 + j] = P[i * 8 + j] + P[i * 8 + j + 4]
    for i in range(4):
        for j in range(8):
            P[i * 8 + j] = P[i * 8 + j] + P[(i + 4) * 8 + j]
    for i in range(8):
        P[i * 8 + i] = P[i * 8 + i] + sd[i] * sd[i]
    m = list(mean)
    for i in range(4):
        m[i] = m[i] + m[i + 4]
    return m, P


def kf_project(mean, cov, xywh, wp):
    if xywh:
        w, h = mean[2], mean[3]
        sd = [wp * w, wp * h, wp * w, wp * h]
    else:
        h = mean[3]
        sd = [wp * h, wp * h, 1e-1, wp * h]
    m4 = list(mean[:4])
    S = [cov[i * 8 + j] for i in range(4) for j in range(4)]
    for i in range(4):
        s = (1.0 - 0.0) * sd[i] if not xywh else sd[i]          # ss_kf_project with conf = 0 (exact: (1 - 0) * x == x)
        S[i * 4 + i] = S[i * 4 + i] + s * s
    return m4, S


def _chol4(S):
    L = [0.0] * 16
    for i in range(4):
        for j in range(i + 1):
            s = S[i * 4 + j]
            for k in range(j):
                s = _fma(-L[i * 4 + k], L[j * 4 + k], s)
            L[i * 4 + j] = math.sqrt(s) if i == j else s / L[j * 4 + j]
    return L


def kf_update(mean, cov, z, xywh, wp):
    m4, S = kf_project(mean, cov, xywh, wp)
    L = _chol4(S)
    K = []
    for r in range(8):
        w = [0.0] * 4
        for i in range(4):
            s = cov[r * 8 + i]
            for k in range(i):
                s = _fma(-L[i * 4 + k], w[k], s)
            w[i] = s / L[i * 4 + i]
        x = [0.0] * 4
        for i in range(3, -1, -1):
            s = w[i]
            for k in range(3, i, -1):
                s = _fma(-L[k * 4 + i], x[k], s)
            x[i] = s / L[i * 4 + i]
        K.append(x)
    y = [float(z[i]) - m4[i] for i in range(4)]
    M = [[0.0] * 8 for _ in range(4)]
    for i in range(4):
        for c in range(8):
            acc = 0.0
            for k in range(4):
                acc = _fma(S[i * 4 + k], K[c][k], acc)
            M[i][c] = acc
    nm = []
    for r in range(8):
        acc = 0.0
        for k in range(4):
            acc = _fma(y[k], K[r][k], acc)
        nm.append(mean[r] + acc)
    nc = list(cov)
    for r in range(8):
        for c in range(8):
            acc = 0.0
            for k in range(4):
                acc = _fma(K[r][k], M[k][c], acc)
            nc[r * 8 + c] = cov[r * 8 + c] - acc
    return nm, nc


# ---- boxes and costs -------------------------------------------------------------------------------------------
def det_tlwh(d):
    """f32 xyxy -> f64 tlwh (differences of f32 values are exact in f64)."""
    x1, y1, x2, y2 = (float(np.float64(v)) for v in d[:4])
    return [x1, y1, x2 - x1, y2 - y1]


def det_measure(t, xywh):
    if xywh:
        return [t[0] + t[2] / 2, t[1] + t[3] / 2, t[2], t[3]]
    return [t[0] + t[2] / 2, t[1] + t[3] / 2, t[2] / t[3], t[3]]


def mean_tlwh(mean, xywh):
    if xywh:
        return [mean[0] - mean[2] / 2, mean[1] - mean[3] / 2, mean[2], mean[3]]
    w = mean[2] * mean[3]
    return [mean[0] - w / 2, mean[1] - mean[3] / 2, w, mean[3]]


def iou_cost(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """1 - IoU of tlwh rows a [T,4] x b [D,4] in ss_iou_cost's order (D-10; no threshold replacement, no epsilon)."""
    a = np.asarray(a, np.float64).reshape(-1, 4)
    b = np.asarray(b, np.float64).reshape(-1, 4)
    t, c = a[:, None, :], b[None, :, :]
    tbr0, tbr1, tarea = t[..., 0] + t[..., 2], t[..., 1] + t[..., 3], t[..., 2] * t[..., 3]
    cbr0, cbr1 = c[..., 0] + c[..., 2], c[..., 1] + c[..., 3]
    tl0, tl1 = np.maximum(t[..., 0], c[..., 0]), np.maximum(t[..., 1], c[..., 1])
    br0, br1 = np.minimum(tbr0, cbr0), np.minimum(tbr1, cbr1)
    w, h = np.maximum(0.0, br0 - tl0), np.maximum(0.0, br1 - tl1)
    inter, carea = w * h, c[..., 2] * c[..., 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = inter / (tarea + carea - inter)
    return 1.0 - iou


def fuse_score(cost: np.ndarray, scores) -> np.ndarray:
    """Ultralytics fuse_score: 1 - (1 - cost) * score, the score the detection's float32 value."""
    s = np.asarray(scores, np.float32).astype(np.float64)[None, :]
    return 1.0 - (1.0 - cost) * s


def assign(cost: np.ndarray, thresh: float):
    """SciPy's optimum of the raw rectangular matrix, then pairs above `thresh` rejected (B-05).
    -> (pairs in ascending row order, unmatched rows ascending, unmatched columns ascending)"""
    R, C = cost.shape
    if R == 0 or C == 0:
        return [], list(range(R)), list(range(C))
    rows, cols = linear_sum_assignment(cost)
    pairs = [(int(r), int(c)) for r, c in zip(rows, cols) if cost[r, c] <= thresh]
    mr, mc = {r for r, _ in pairs}, {c for _, c in pairs}
    return pairs, [r for r in range(R) if r not in mr], [c for c in range(C) if c not in mc]


class Track:
    __slots__ = ("mean", "cov", "state", "activated", "id", "start", "end", "tracklet_len", "score", "cls", "det", "tlwh")

    def __repr__(self):
        return f"Track(id={self.id}, state={self.state}, act={self.activated}, start={self.start}, end={self.end})"


class ByteTrackRef:
    """One stream of the BYTE tracker (docs/BYTETRACK.md §1)."""

    def __init__(self, cfg: Optional[ByteTrackConfig] = None):
        self.cfg = cfg or ByteTrackConfig()
        if self.cfg.kalman not in ("xyah", "xywh"):
            raise ValueError("kalman must be 'xyah' or 'xywh'")
        self.xywh = self.cfg.kalman == "xywh"
        self.max_time_lost = int(self.cfg.frame_rate / 30.0 * self.cfg.track_buffer)
        self.reset()

    def reset(self):
        self.tracked: List[Track] = []
        self.lost: List[Track] = []
        self.frame_id = 0
        self.next_id = 1
        self.capacity_error = False

    # -- Kalman steps on a track --
    def _set_mean(self, t, mean, cov):
        t.mean, t.cov = mean, cov
        t.tlwh = mean_tlwh(mean, self.xywh)

    def _update(self, t, d, reactivate=False):
        c = self.cfg
        m, P = kf_update(t.mean, t.cov, self._z[d], self.xywh, c.std_weight_position)
        self._set_mean(t, m, P)
        t.tracklet_len = 0 if reactivate else t.tracklet_len + 1
        t.state, t.activated, t.end = TRACKED, True, self.frame_id
        t.score, t.cls, t.det = self._score[d], self._cls[d], d

    def update(self, dets) -> np.ndarray:
        c = self.cfg
        dets = np.asarray(dets, np.float32).reshape(-1, 6)
        if dets.shape[0] > c.max_dets:
            self.capacity_error = True
            dets = dets[:c.max_dets]
        self.frame_id += 1
        fid = self.frame_id
        N = dets.shape[0]
        self._tl = [det_tlwh(dets[i]) for i in range(N)]
        self._z = [det_measure(t, self.xywh) for t in self._tl]
        self._score = [np.float32(dets[i, 4]) for i in range(N)]
        self._cls = [np.float32(dets[i, 5]) for i in range(N)]
        hi_t, lo_t = np.float32(c.track_high_thresh), np.float32(c.track_low_thresh)
        # 1. split the rows by score (float32 compares, B-04)
        high = [i for i in range(N) if self._score[i] >= hi_t]
        low = [i for i in range(N) if lo_t < self._score[i] < hi_t]
        # 2. unconfirmed / pool
        unconf = [t for t in self.tracked if not t.activated]
        pool = [t for t in self.tracked if t.activated] + list(self.lost)
        n_live = len(self.tracked) + len(self.lost)
        # 3. predict the pool (not the unconfirmed tracks)
        for t in pool:
            m = list(t.mean)
            if t.state != TRACKED:
                m[7] = 0.0
                if self.xywh:
                    m[6] = 0.0
            m, P = kf_predict(m, t.cov, self.xywh, c.std_weight_position, c.std_weight_velocity)
            self._set_mean(t, m, P)
        # 4. first association: pool x high, fused IoU cost
        refound = []
        cost = iou_cost([t.tlwh for t in pool], [self._tl[i] for i in high]) if pool and high else np.zeros((len(pool), len(high)))
        if c.fuse_score and cost.size:
            cost = fuse_score(cost, [self._score[i] for i in high])
        pairs, u_pool, u_high = assign(cost, c.match_thresh)
        for r, k in pairs:
            t = pool[r]
            if t.state == TRACKED:
                self._update(t, high[k])
            else:
                self._update(t, high[k], reactivate=True)
                refound.append(t)
        # 5. second association: the unmatched Tracked pool tracks x low rows, plain IoU
        r2 = [pool[r] for r in u_pool if pool[r].state == TRACKED]
        cost = iou_cost([t.tlwh for t in r2], [self._tl[i] for i in low]) if r2 and low else np.zeros((len(r2), len(low)))
        pairs, u_r2, _ = assign(cost, 0.5)
        for r, k in pairs:
            self._update(r2[r], low[k])
        new_lost = []
        for r in u_r2:
            if r2[r].state != LOST:
                r2[r].state = LOST
                new_lost.append(r2[r])
        # 6. unconfirmed x the high rows left over, fused cost, 0.7
        left = [high[k] for k in u_high]
        cost = iou_cost([t.tlwh for t in unconf], [self._tl[i] for i in left]) if unconf and left else np.zeros((len(unconf), len(left)))
        if c.fuse_score and cost.size:
            cost = fuse_score(cost, [self._score[i] for i in left])
        pairs, u_unc, u_left = assign(cost, 0.7)
        for r, k in pairs:
            self._update(unconf[r], left[k])
        for r in u_unc:
            unconf[r].state = REMOVED
        # 7. births
        births = []
        for k in u_left:
            d = left[k]
            if self._score[d] < np.float32(c.new_track_thresh):
                continue
            if n_live + len(births) >= c.max_tracks:
                self.capacity_error = True
                continue
            t = Track()
            t.id = self.next_id
            self.next_id += 1
            m, P = kf_initiate(self._z[d], self.xywh, c.std_weight_position, c.std_weight_velocity)
            self._set_mean(t, m, P)
            t.tracklet_len, t.state, t.activated = 0, TRACKED, fid == 1
            t.start = t.end = fid
            t.score, t.cls, t.det = self._score[d], self._cls[d], d
            births.append(t)
        # 8. lost tracks past max_time_lost
        for t in self.lost:
            if t.state == LOST and fid - t.end > self.max_time_lost:
                t.state = REMOVED
        # 9. the lists
        tracked = [t for t in self.tracked if t.state == TRACKED] + births + refound
        lost = [t for t in self.lost if t.state == LOST] + new_lost
        if tracked and lost:
            d = iou_cost([t.tlwh for t in tracked], [t.tlwh for t in lost])
            dup_a, dup_b = set(), set()
            for p, q in zip(*np.nonzero(d < 0.15)):
                tp, tq = tracked[p].end - tracked[p].start, lost[q].end - lost[q].start
                if tp > tq:
                    dup_b.add(int(q))
                else:
                    dup_a.add(int(p))
            tracked = [t for i, t in enumerate(tracked) if i not in dup_a]
            lost = [t for i, t in enumerate(lost) if i not in dup_b]
        self.tracked, self.lost = tracked, lost
        # 10. rows of the activated tracked tracks
        rows = []
        for t in self.tracked:
            if t.activated:
                tl = t.tlwh
                rows.append([tl[0], tl[1], tl[0] + tl[2], tl[1] + tl[3], t.id, t.cls, t.score, t.det])
        return np.asarray(rows, np.float32).reshape(-1, 8)

    def tracks(self):
        """The table in list order (tracked, then lost): ids, states, activated, means [n,8] — what ss_byte_get_tracks returns."""
        ts = self.tracked + self.lost
        return (np.array([t.id for t in ts], np.int32), np.array([t.state for t in ts], np.int32),
                np.array([int(t.activated) for t in ts], np.int32), np.array([t.mean for t in ts], np.float64).reshape(-1, 8))
