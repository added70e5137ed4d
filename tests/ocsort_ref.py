"""CPU reference of the OC-SORT tracker (docs/OCSORT.md, decisions O-01..): a float64 restatement of one stream, written in the
operation order of csrc/ss_ocsort.hip so that the device reproduces it bit for bit.

Not a conftest and not a test module: imported by tests/test_ocsort_cpu.py and tests/test_gpu_ocsort.py.

    ref = OCSortRef(OCSortConfig())
    rows = ref.update(dets)      # dets [N,6] float32 x1,y1,x2,y2,score,cls -> float32 [M,8] x1,y1,x2,y2,id,cls,score,det_idx

Every Kalman step is written element by element (no BLAS, no inverse, no `@`): the 4x4 solve mirrors ss_chol4 / ss_kf_gain_row
(csrc/ss_kalman.h, exactly rounded fma: `_fma`), everything else is one multiplication or one addition at a time, as the device
computes it under -ffp-contract=off.  `counters` counts the branches taken (the GPU tests assert that their inputs reach them).
"""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np
from scipy.optimize import linear_sum_assignment

from strongsort_yolo_amd.config import OCSortConfig
from tests.bytetrack_ref import _fma

NAN = float("nan")
PIO2 = 1.5707963267948966
PI = 3.141592653589793
ASIN_C = (1.0, 0.16666666666666666, 0.075, 0.044642857142857144, 0.030381944444444444, 0.022372159090909092,
          0.017352764423076924, 0.01396484375, 0.011551800896139705, 0.009761609529194078, 0.008390335809616815,
          0.0073125258735988454, 0.006447210311889649, 0.005740037670841924, 0.005153309682319905, 0.004660143486915096,
          0.004240907093679363, 0.003880964558837669, 0.0035692053938259347, 0.003297059503473485, 0.0030578216492580306,
          0.002846178401108942)
R_DIAG = (1.0, 1.0, 10.0, 10.0)
Q_DIAG = (1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 0.0001)
P0_DIAG = (10.0, 10.0, 10.0, 10.0, 1e4, 1e4, 1e4)


def ss_asin(c):
    """csrc/ss_asin.h on a float64 array (or scalar): elementwise, one rounding per operation."""
    c = np.asarray(c, np.float64)
    a = np.abs(c)
    big = a > 0.5
    with np.errstate(invalid="ignore"):
        x = np.where(big, np.sqrt((1.0 - a) / 2.0), a)
    z = x * x
    p = np.full_like(z, ASIN_C[-1])
    for k in range(len(ASIN_C) - 2, -1, -1):
        p = p * z
        p = p + ASIN_C[k]
    r = x * p
    r = np.where(big, PIO2 - 2.0 * r, r)
    return np.where(c < 0.0, -r, r)


def _div(a: float, b: float) -> float:
    """IEEE division (no ZeroDivisionError)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(a: float) -> float:
    """IEEE square root (NaN below zero)."""
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(a)))


# ---- the 7-state filter (x, y, s, r, vx, vy, vs), f64 ----------------------------------------------------------------------
def box_to_z(b):
    """xyxy -> (x, y, s, r) as upstream's convert_bbox_to_z."""
    w, h = b[2] - b[0], b[3] - b[1]
    return [b[0] + w / 2.0, b[1] + h / 2.0, w * h, _div(w, h + 1e-6)]


def x_to_box(x):
    """state -> xyxy as upstream's convert_x_to_bbox."""
    w = _sqrt(x[2] * x[3])
    h = _div(x[2], w)
    return [x[0] - w / 2.0, x[1] - h / 2.0, x[0] + w / 2.0, x[1] + h / 2.0]


def kf_init(z):
    x = [z[0], z[1], z[2], z[3], 0.0, 0.0, 0.0]
    P = [0.0] * 49
    for i in range(7):
        P[i * 7 + i] = P0_DIAG[i]
    return x, P


def kf_predict(x, P):
    """x = F x, P = F P F^T + Q: F adds the velocity of x, y, s; additions only."""
    P = list(P)
    for i in range(7):
        for j in range(3):
            P[i * 7 + j] = P[i * 7 + j] + P[i * 7 + j + 4]
    for i in range(3):
        for j in range(7):
            P[i * 7 + j] = P[i * 7 + j] + P[(i + 4) * 7 + j]
    for i in range(7):
        P[i * 7 + i] = P[i * 7 + i] + Q_DIAG[i]
    x = list(x)
    for i in range(3):
        x[i] = x[i] + x[i + 4]
    return x, P


def _chol4(S):
    L = [0.0] * 16
    for i in range(4):
        for j in range(i + 1):
            s = S[i * 4 + j]
            for k in range(j):
                s = _fma(-L[i * 4 + k], L[j * 4 + k], s)
            L[i * 4 + j] = _sqrt(s) if i == j else _div(s, L[j * 4 + j])
    return L


def _gain_row(L, p):
    w = [0.0] * 4
    for i in range(4):
        s = p[i]
        for k in range(i):
            s = _fma(-L[i * 4 + k], w[k], s)
        w[i] = _div(s, L[i * 4 + i])
    x = [0.0] * 4
    for i in range(3, -1, -1):
        s = w[i]
        for k in range(3, i, -1):
            s = _fma(-L[k * 4 + i], x[k], s)
        x[i] = _div(s, L[i * 4 + i])
    return x


def kf_update(x, P, z):
    """The Joseph-form update with H = [I4 0]: S = P[:4,:4] + R, K = P[:, :4] S^-1 by Cholesky solves, x += K (z - x[:4]),
    P = (I - K H) P (I - K H)^T + K R K^T as B = P - K P[:4, :], then B - B[:, :4] K^T, then + K R K^T."""
    if not all(math.isfinite(v) for v in x) or not all(math.isfinite(v) for v in P) or not all(math.isfinite(v) for v in z):
        return [NAN] * 7, [NAN] * 49                       # a non-finite filter stays non-finite (its bits are not compared)
    S = [P[i * 7 + j] for i in range(4) for j in range(4)]
    for i in range(4):
        S[i * 4 + i] = S[i * 4 + i] + R_DIAG[i]
    L = _chol4(S)
    K = [_gain_row(L, P[r * 7:r * 7 + 4]) for r in range(7)]
    y = [z[i] - x[i] for i in range(4)]
    nx = []
    for r in range(7):
        acc = 0.0
        for k in range(4):
            acc = acc + K[r][k] * y[k]
        nx.append(x[r] + acc)
    top = P[:28]
    B = [0.0] * 49
    for r in range(7):
        for c in range(7):
            acc = 0.0
            for k in range(4):
                acc = acc + K[r][k] * top[k * 7 + c]
            B[r * 7 + c] = P[r * 7 + c] - acc
    N = [0.0] * 49
    for r in range(7):
        for c in range(7):
            acc = 0.0
            for k in range(4):
                acc = acc + B[r * 7 + k] * K[c][k]
            t = B[r * 7 + c] - acc
            acc = 0.0
            for k in range(4):
                acc = acc + (K[r][k] * R_DIAG[k]) * K[c][k]
            N[r * 7 + c] = t + acc
    return nx, N


def kf_oru(xf, Pf, z1, z2, g, counters=None):
    """Observation-centric re-update: from the frozen filter, g virtual observations on the line z1 -> z2 (x, y, w, h
    interpolated), a predict between them; the caller's ordinary update with z2 follows."""
    x, P = list(xf), list(Pf)
    w1, h1 = _sqrt(z1[2] * z1[3]), _sqrt(_div(z1[2], z1[3]))
    w2, h2 = _sqrt(z2[2] * z2[3]), _sqrt(_div(z2[2], z2[3]))
    gf = float(g)
    dx, dy, dw, dh = (z2[0] - z1[0]) / gf, (z2[1] - z1[1]) / gf, (w2 - w1) / gf, (h2 - h1) / gf
    for i in range(1, g + 1):
        fi = float(i)
        vx, vy, vw, vh = z1[0] + fi * dx, z1[1] + fi * dy, w1 + fi * dw, h1 + fi * dh
        x, P = kf_update(x, P, [vx, vy, vw * vh, _div(vw, vh)])
        if i < g:
            x, P = kf_predict(x, P)
        if counters is not None:
            counters["oru"] += 1
    return x, P


# ---- boxes and costs ---------------------------------------------------------------------------------------------------------
def iou_matrix(d: np.ndarray, t: np.ndarray) -> np.ndarray:
    """IoU of xyxy rows d [D,4] x t [T,4] in oc_iou's order; 0 where the union is not positive (or not a number)."""
    d = np.asarray(d, np.float64).reshape(-1, 4)[:, None, :]
    t = np.asarray(t, np.float64).reshape(-1, 4)[None, :, :]
    with np.errstate(all="ignore"):
        w = np.minimum(d[..., 2], t[..., 2]) - np.maximum(d[..., 0], t[..., 0])
        h = np.minimum(d[..., 3], t[..., 3]) - np.maximum(d[..., 1], t[..., 1])
        w = np.where(w > 0.0, w, 0.0)
        h = np.where(h > 0.0, h, 0.0)
        inter = w * h
        u = (d[..., 2] - d[..., 0]) * (d[..., 3] - d[..., 1]) + (t[..., 2] - t[..., 0]) * (t[..., 3] - t[..., 1]) - inter
        return np.where(u > 0.0, inter / np.where(u > 0.0, u, 1.0), 0.0)


def direction(cx0, cy0, cx1, cy1):
    """unit vector (x, y) from (cx0, cy0) to (cx1, cy1), norm sqrt(dx^2 + dy^2) + 1e-6; arrays or scalars."""
    dx, dy = cx1 - cx0, cy1 - cy0
    n = np.sqrt(dx * dx + dy * dy) + 1e-6
    return dx / n, dy / n


def lsap(cost: np.ndarray):
    rows, cols = linear_sum_assignment(cost)
    return [(int(r), int(c)) for r, c in zip(rows, cols)]


class Track:
    __slots__ = ("x", "P", "xf", "Pf", "frozen", "observed", "id", "age", "tsu", "hits", "streak", "has_obs", "lobs", "obs",
                 "vel", "score", "cls", "det", "dead", "pbox", "kc", "mdet")


class OCSortRef:
    """One stream of OC-SORT (docs/OCSORT.md §1)."""

    def __init__(self, cfg: Optional[OCSortConfig] = None):
        self.cfg = cfg or OCSortConfig()
        self.reset()

    def reset(self):
        self.trackers: List[Track] = []
        self.frame_count = 0
        self.next_id = 1
        self.capacity_error = False
        self.counters = dict(oru=0, oru_tracks=0, lsap=0, shortcut=0, clamp=0, ocr=0, byte=0, match=0)

    def _k_obs(self, t):
        """the observation delta_t ages back, else the nearest later one, else the last (O-07); None without any."""
        if not t.has_obs:
            return None
        for dt in range(self.cfg.delta_t, 0, -1):
            if t.age - dt in t.obs:
                return t.obs[t.age - dt]
        return t.lobs

    def _matched(self, t, d):
        c = self.cfg
        box = self._box[d]
        if t.has_obs:
            k = t.kc                                               # centre of _k_obs (found after the predict, same age)
            vx, vy = direction(k[0], k[1], (box[0] + box[2]) / 2.0, (box[1] + box[3]) / 2.0)
            t.vel = (float(vx), float(vy))
        z1 = box_to_z(t.lobs) if t.has_obs else None
        t.lobs, t.has_obs = box, True
        t.obs[t.age] = box
        for a in [a for a in t.obs if a <= t.age - c.delta_t]:     # the ring forgets what no later frame can ask for
            del t.obs[a]
        g = t.tsu
        t.tsu = 0
        t.hits += 1
        t.streak += 1
        t.score, t.cls, t.det = self._score[d], self._cls[d], d
        z2 = box_to_z(box)
        if t.frozen:
            t.x, t.P = kf_oru(t.xf, t.Pf, z1, z2, g, self.counters)
            t.frozen = False
            self.counters["oru_tracks"] += 1
        t.x, t.P = kf_update(t.x, t.P, z2)
        t.observed = True
        self.counters["match"] += 1

    def update(self, dets) -> np.ndarray:
        c = self.cfg
        dets = np.asarray(dets, np.float32).reshape(-1, 6)
        if dets.shape[0] > c.max_dets:
            self.capacity_error = True
            dets = dets[:c.max_dets]
        self.frame_count += 1
        N = dets.shape[0]
        self._box = [[float(np.float64(v)) for v in dets[i, :4]] for i in range(N)]
        self._score = [np.float32(dets[i, 4]) for i in range(N)]
        self._cls = [np.float32(dets[i, 5]) for i in range(N)]
        hi_t, lo_t = np.float32(c.det_thresh), np.float32(c.low_thresh)
        # 1. split the rows by score (float32 compares)
        high = [i for i in range(N) if self._score[i] > hi_t]
        second = [i for i in range(N) if lo_t < self._score[i] < hi_t] if c.use_byte else []
        trks = self.trackers
        n_live = len(trks)
        # 2. predict every track
        for t in trks:
            if t.x[6] + t.x[2] <= 0.0:
                t.x[6] = 0.0
                self.counters["clamp"] += 1
            t.x, t.P = kf_predict(t.x, t.P)
            t.age += 1
            if t.tsu > 0:
                t.streak = 0
            t.tsu += 1
            t.pbox = x_to_box(t.x)
            t.dead = not all(math.isfinite(v) for v in t.pbox)     # O-10: leaves at the end of the frame, matches nothing
            k = self._k_obs(t)
            t.kc = None if k is None else ((k[0] + k[2]) / 2.0, (k[1] + k[3]) / 2.0)
            t.mdet = -1
        T, H = len(trks), len(high)
        used = [False] * H
        # 3. first association: high rows x all tracks
        if T and H:
            hb = np.array([self._box[i] for i in high], np.float64).reshape(-1, 4)
            iou = iou_matrix(hb, [t.pbox for t in trks])
            valid = np.array([0.0 if (t.kc is None or t.dead) else 1.0 for t in trks])
            kcx = np.array([0.0 if t.kc is None else t.kc[0] for t in trks])
            kcy = np.array([0.0 if t.kc is None else t.kc[1] for t in trks])
            vx = np.array([t.vel[0] for t in trks])
            vy = np.array([t.vel[1] for t in trks])
            dcx, dcy = (hb[:, 0] + hb[:, 2]) / 2.0, (hb[:, 1] + hb[:, 3]) / 2.0
            ux, uy = direction(kcx[None, :], kcy[None, :], dcx[:, None], dcy[:, None])
            cs = vx[None, :] * ux + vy[None, :] * uy
            cs = np.where(cs < -1.0, -1.0, np.where(cs > 1.0, 1.0, cs))
            term = ss_asin(cs) / PI
            term = term * c.inertia
            term = term * np.array([np.float64(self._score[i]) for i in high])[:, None]
            term = np.where(valid[None, :] > 0.0, term, 0.0)
            a = iou > c.iou_threshold
            if a.any() and a.sum(1).max() == 1 and a.sum(0).max() == 1:
                pairs = [(int(r), int(k)) for r, k in zip(*np.nonzero(a))]
                self.counters["shortcut"] += 1
            else:
                pairs = lsap(-(iou + term))
                self.counters["lsap"] += 1
            for r, k in pairs:
                if iou[r, k] < c.iou_threshold:
                    continue
                trks[k].mdet = high[r]
                used[r] = True
        # 4. BYTE stage: second rows x the unmatched tracks' predicted boxes
        ut = [k for k in range(T) if trks[k].mdet < 0 and not trks[k].dead]
        if second and ut:
            iou = iou_matrix([self._box[i] for i in second], [trks[k].pbox for k in ut])
            if (iou > c.iou_threshold).any():
                for r, k in lsap(-iou):
                    if iou[r, k] < c.iou_threshold:
                        continue
                    trks[ut[k]].mdet = second[r]
                    self.counters["byte"] += 1
        # 5. OCR: the high rows left x the remaining tracks' last observations
        ut = [k for k in range(T) if trks[k].mdet < 0 and not trks[k].dead]
        ud = [r for r in range(H) if not used[r]]
        if ud and ut:
            iou = iou_matrix([self._box[high[r]] for r in ud], [trks[k].lobs for k in ut])
            iou = np.where(np.array([trks[k].has_obs for k in ut])[None, :], iou, 0.0)
            if (iou > c.iou_threshold).any():
                for r, k in lsap(-iou):
                    if iou[r, k] < c.iou_threshold:
                        continue
                    trks[ut[k]].mdet = high[ud[r]]
                    used[ud[r]] = True
                    self.counters["ocr"] += 1
        # 6. update
        for t in trks:
            if t.mdet >= 0:
                self._matched(t, t.mdet)
            else:
                if t.observed:                                     # the first miss after an observation freezes the filter
                    t.xf, t.Pf, t.frozen = list(t.x), list(t.P), True
                t.observed = False
        # 7. births: the high rows still unmatched, ascending
        births = []
        for r in range(H):
            if used[r]:
                continue
            if n_live + len(births) >= c.max_tracks:
                self.capacity_error = True
                continue
            d = high[r]
            t = Track()
            t.x, t.P = kf_init(box_to_z(self._box[d]))
            t.xf, t.Pf, t.frozen, t.observed = None, None, False, False
            t.id = self.next_id
            self.next_id += 1
            t.age = t.tsu = t.hits = t.streak = 0
            t.has_obs, t.lobs, t.obs, t.vel = False, self._box[d], {}, (0.0, 0.0)     # O-06: the birth row is shown, not observed
            t.score, t.cls, t.det, t.dead = self._score[d], self._cls[d], d, False
            births.append(t)
        # 8. the list and the rows (newest first)
        self.trackers = [t for t in trks if not (t.tsu > c.max_age) and not t.dead] + births
        rows = []
        for t in reversed(self.trackers):
            if t.tsu < 1 and (t.streak >= c.min_hits or self.frame_count <= c.min_hits):
                rows.append([t.lobs[0], t.lobs[1], t.lobs[2], t.lobs[3], t.id, t.cls, t.score, t.det])
        return np.asarray(rows, np.float32).reshape(-1, 8)

    def tracks(self) -> dict:
        """The table in list order — what ss_ocsort_get_tracks returns."""
        ts = self.trackers
        i32 = lambda f: np.array([f(t) for t in ts], np.int32)
        return dict(track_id=i32(lambda t: t.id), age=i32(lambda t: t.age), time_since_update=i32(lambda t: t.tsu),
                    hits=i32(lambda t: t.hits), hit_streak=i32(lambda t: t.streak), frozen=i32(lambda t: int(t.frozen)),
                    x=np.array([t.x for t in ts], np.float64).reshape(-1, 7), P=np.array([t.P for t in ts], np.float64).reshape(-1, 49),
                    last_obs=np.array([t.lobs if t.has_obs else [-1.0] * 4 for t in ts], np.float32).reshape(-1, 4),
                    velocity=np.array([t.vel for t in ts], np.float64).reshape(-1, 2),
                    n_tracks=len(ts), next_id=self.next_id, frame_count=self.frame_count)
