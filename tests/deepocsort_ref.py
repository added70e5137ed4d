"""CPU reference of the Deep OC-SORT tracker (docs/DEEPOCSORT.md, decisions DO-01..): OCSortRef's frame procedure without the
BYTE stage, plus camera-motion compensation (step 1b), the tracks' features and the appearance cost of the first association,
written in the operation order of csrc/ss_deepoc.hip so that the device reproduces it bit for bit.

Not a conftest and not a test module: imported by tests/test_deepocsort_cpu.py and tests/test_gpu_deepocsort.py.

    ref = DeepOCSortRef(DeepOCSortConfig())
    rows = ref.update(dets, feats, warp=None)   # dets [N,6] f32, feats [N,512] raw features of the rows, warp [8] or None

The feature arithmetic goes through the exact-order oracle (oracle.cexact: so_normalize, so_ema, so_dot); everything else is one
float64 operation at a time.  `counters` counts the branches taken (the GPU tests assert that their inputs reach them).
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from oracle import cexact
from strongsort_yolo_amd.config import DeepOCSortConfig
from tests.ocsort_ref import (OCSortRef, Track, PI, ss_asin, box_to_z, x_to_box, kf_init, kf_predict, iou_matrix, direction, lsap)

FEAT = 512


def warp_point(w, px, py):
    """p' = R p + t with R = [[w0, w1], [w3, w4]], t = (w2, w5): two products and one add per coordinate, then + t."""
    return (w[0] * px + w[1] * py) + w[2], (w[3] * px + w[4] * py) + w[5]


def warp_box32(w, b):
    """both corners of an xyxy box moved as points, rounded to float32 once."""
    x1, y1 = warp_point(w, b[0], b[1])
    x2, y2 = warp_point(w, b[2], b[3])
    return [float(np.float32(v)) for v in (x1, y1, x2, y2)]


def warp_filter(w, x, P):
    """step 1b on a filter: x[0:2] = R x[0:2] + t, x[4:6] = R x[4:6], and the two diagonal 2x2 blocks of P at 0 and 4 become
    R B R^T (X = R B, then X R^T, in index order).  Nothing else moves (DO-03)."""
    r = ((w[0], w[1]), (w[3], w[4]))
    x, P = list(x), list(P)
    x[0], x[1] = warp_point(w, x[0], x[1])
    x[4], x[5] = r[0][0] * x[4] + r[0][1] * x[5], r[1][0] * x[4] + r[1][1] * x[5]
    for o in (0, 4):
        B = [[P[(o + i) * 7 + o + j] for j in range(2)] for i in range(2)]
        X = [[r[i][0] * B[0][j] + r[i][1] * B[1][j] for j in range(2)] for i in range(2)]
        for i in range(2):
            for j in range(2):
                P[(o + i) * 7 + o + j] = X[i][0] * r[j][0] + X[i][1] * r[j][1]
    return x, P


def top2(v):
    """the largest and the second largest value of a sequence of at least two (values: a tie gives m2 == m1)."""
    m1, m2 = (v[0], v[1]) if v[0] > v[1] else (v[1], v[0])
    for a in v[2:]:
        if a > m1:
            m1, m2 = a, m1
        elif a > m2:
            m2 = a
    return m1, m2


def aw_factor(m1, m2, aw):
    """the factor of one row or column (DO-07): 0 if m1 == 0, else 1 - max(m2 / m1 - aw, 0) / (1 - aw)."""
    if m1 == 0.0:
        return 0.0
    d = m2 / m1 - aw
    d = d if d > 0.0 else 0.0
    return 1.0 - d / (1.0 - aw)


def aw_weights(E, w, aw, counters=None):
    """adaptive weighting: W = w everywhere, every row with at least two columns multiplied by its factor, then every column with
    at least two rows by its factor, on top: W[r][k] = (w * rf[r]) * cf[k]."""
    H, T = E.shape
    rf = [aw_factor(*top2([float(v) for v in E[r]]), aw) if T >= 2 else 1.0 for r in range(H)]
    cf = [aw_factor(*top2([float(v) for v in E[:, k]]), aw) if H >= 2 else 1.0 for k in range(T)]
    if counters is not None:
        counters["aw_rows"] += sum(1 for f in rf if f < 1.0)
        counters["aw_cols"] += sum(1 for f in cf if f < 1.0)
    W = np.empty((H, T))
    for r in range(H):
        for k in range(T):
            W[r, k] = (w * rf[r]) * cf[k]
    return W


class DeepOCSortRef(OCSortRef):
    """One stream of Deep OC-SORT (docs/DEEPOCSORT.md §1)."""

    def __init__(self, cfg: Optional[DeepOCSortConfig] = None):
        self.cfg = cfg or DeepOCSortConfig()
        self.reset()

    def reset(self):
        super().reset()
        self.counters.update(lsap_emb=0, aw_rows=0, aw_cols=0, warp=0, warp_frozen=0, ema=0)
        self.last_E = self.last_W = None

    def _alpha(self, score) -> float:
        c = self.cfg
        if not c.dynamic_appearance:
            return c.alpha_fixed_emb
        trust = (float(np.float64(score)) - c.det_thresh) / (1.0 - c.det_thresh)
        return c.alpha_fixed_emb + (1.0 - c.alpha_fixed_emb) * (1.0 - trust)

    def _cmc(self, w):
        """step 1b, before the predict: every track of the list."""
        D = self.cfg.delta_t
        self.counters["warp"] += 1
        any_frozen = False
        for t in self.trackers:
            t.x, t.P = warp_filter(w, t.x, t.P)
            if t.frozen:
                t.xf, t.Pf = warp_filter(w, t.xf, t.Pf)
                any_frozen = True
            if t.has_obs:
                t.lobs = warp_box32(w, t.lobs)
            for a in list(t.obs):
                if t.age - D <= a <= t.age:
                    t.obs[a] = warp_box32(w, t.obs[a])
        if any_frozen:
            self.counters["warp_frozen"] += 1

    def update(self, dets, feats=None, warp=None) -> np.ndarray:
        c = self.cfg
        dets = np.asarray(dets, np.float32).reshape(-1, 6)
        raw = np.zeros((dets.shape[0], FEAT), np.float32) if feats is None else np.asarray(feats, np.float32).reshape(-1, FEAT)
        if dets.shape[0] > c.max_dets:
            self.capacity_error = True
            dets = dets[:c.max_dets]
        self.frame_count += 1
        N = dets.shape[0]
        self._box = [[float(np.float64(v)) for v in dets[i, :4]] for i in range(N)]
        self._score = [np.float32(dets[i, 4]) for i in range(N)]
        self._cls = [np.float32(dets[i, 5]) for i in range(N)]
        hi_t = np.float32(c.det_thresh)
        # 1. the high rows (float32 compare); only their features are read (DO-05)
        high = [i for i in range(N) if self._score[i] > hi_t]
        curr = {i: cexact.normalize(raw[i]) for i in high} if c.appearance else {}
        trks = self.trackers
        n_live = len(trks)
        # 1b. camera-motion compensation
        if warp is not None and float(warp[6]) >= 0.0:
            self._cmc([float(v) for v in np.asarray(warp, np.float64)[:6]])
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
            t.dead = not all(math.isfinite(v) for v in t.pbox)
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
                base = iou + term
                if c.appearance:
                    E = np.zeros((H, T))
                    for r, k in zip(*np.nonzero(iou > 0.0)):           # a dead track's IoU is 0 (O-10)
                        E[r, k] = float(np.float64(cexact.dot(curr[high[r]], trks[k].emb)))
                    W = aw_weights(E, c.w_association_emb, c.aw_param, self.counters) if c.adaptive_weighting \
                        else np.full((H, T), c.w_association_emb)
                    self.last_E, self.last_W = E, W
                    base = base + W * E
                    self.counters["lsap_emb"] += 1
                pairs = lsap(-base)
                self.counters["lsap"] += 1
            for r, k in pairs:
                if iou[r, k] < c.iou_threshold:
                    continue
                trks[k].mdet = high[r]
                used[r] = True
        # 5. OCR: the high rows left x the remaining tracks' last observations, on IoU alone
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
        # 6. update: the filter as OC-SORT (ORU, freeze), then the feature
        for t in trks:
            if t.mdet >= 0:
                self._matched(t, t.mdet)
                if c.appearance:
                    t.emb = cexact.ema(t.emb, curr[t.mdet], self._alpha(self._score[t.mdet]))   # (float)alpha, (float)(1.0 - alpha)
                    self.counters["ema"] += 1
            else:
                if t.observed:
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
            t = DeepTrack()
            t.x, t.P = kf_init(box_to_z(self._box[d]))
            t.xf, t.Pf, t.frozen, t.observed = None, None, False, False
            t.id = self.next_id
            self.next_id += 1
            t.age = t.tsu = t.hits = t.streak = 0
            t.has_obs, t.lobs, t.obs, t.vel = False, self._box[d], {}, (0.0, 0.0)
            t.score, t.cls, t.det, t.dead = self._score[d], self._cls[d], d, False
            t.emb = curr[d].copy() if c.appearance else np.zeros(FEAT, np.float32)
            births.append(t)
        # 8. the list and the rows (newest first)
        self.trackers = [t for t in trks if not (t.tsu > c.max_age) and not t.dead] + births
        rows = []
        for t in reversed(self.trackers):
            if t.tsu < 1 and (t.streak >= c.min_hits or self.frame_count <= c.min_hits):
                rows.append([t.lobs[0], t.lobs[1], t.lobs[2], t.lobs[3], t.id, t.cls, t.score, t.det])
        return np.asarray(rows, np.float32).reshape(-1, 8)

    def features(self) -> np.ndarray:
        """The tracks' features in tracks()' list order — what ss_deepoc_get_features returns."""
        return np.array([t.emb for t in self.trackers], np.float32).reshape(-1, FEAT)


class DeepTrack(Track):
    __slots__ = ("emb",)
