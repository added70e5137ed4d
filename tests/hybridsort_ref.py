"""CPU reference of the Hybrid-SORT tracker (docs/HYBRIDSORT.md, decisions H-01..): a float64 restatement of one stream, written in
the operation order of csrc/ss_hybrid.hip so that the device reproduces it bit for bit.

Not a conftest and not a test module: imported by tests/test_hybridsort_cpu.py and tests/test_gpu_hybridsort.py.

    ref = HybridSortRef(HybridSortConfig())
    rows = ref.update(dets)      # dets [N,6] float32 x1,y1,x2,y2,score,cls -> float32 [M,8] x1,y1,x2,y2,id,cls,score,det_idx

The 9-state filter is kept as what it is: four independent (position, velocity) filters for x, y, s and the confidence c, and one
scalar filter for r (H-02).  Every step is one multiplication, addition or division at a time, as the device computes it under
-ffp-contract=off.  `counters` counts the branches taken (the GPU tests assert that their inputs reach them).
"""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np

from strongsort_yolo_amd.config import HybridSortConfig
from tests.ocsort_ref import PI, _div, _sqrt, iou_matrix, lsap, ss_asin

# per component x, y, s, c: initial covariance, process noise (position, velocity) and measurement noise; then r's three
P0_PAIR = (10.0, 1e4)
Q_PAIR = ((1.0, 0.01), (1.0, 0.01), (1.0, 1e-4), (1.0, 1e-4))
R_PAIR = (1.0, 1.0, 10.0, 10.0)
P0_R, Q_R, R_R = 10.0, 1.0, 10.0
CORNERS = ((0, 1), (2, 1), (0, 3), (2, 3))          # lt, rt, lb, rb as (x index, y index) of an xyxy box: the order of every sum (H-05)


# ---- the filter: flt = [p, v, P00, P01, P10, P11] * 4 (x, y, s, c) + [r, Pr], 26 doubles -------------------------------------
def box_to_z5(b, score):
    """xyxy and the score -> the measurement (x, y, s, c, r)."""
    w, h = b[2] - b[0], b[3] - b[1]
    return [b[0] + w / 2.0, b[1] + h / 2.0, w * h, float(score), _div(w, h + 1e-6)]


def kf_init(z):
    f = []
    for i in range(4):
        f += [z[i], 0.0, P0_PAIR[0], 0.0, 0.0, P0_PAIR[1]]
    return f + [z[4], P0_R]


def kf_predict(f):
    """Each pair: p += v, P = F P F^T + Q by additions (columns, then rows, then the diagonal); r's variance grows by Q_R."""
    f = list(f)
    for i in range(4):
        o = i * 6
        f[o] = f[o] + f[o + 1]
        f[o + 2] = f[o + 2] + f[o + 3]
        f[o + 4] = f[o + 4] + f[o + 5]
        f[o + 2] = f[o + 2] + f[o + 4]
        f[o + 3] = f[o + 3] + f[o + 5]
        f[o + 2] = f[o + 2] + Q_PAIR[i][0]
        f[o + 5] = f[o + 5] + Q_PAIR[i][1]
    f[25] = f[25] + Q_R
    return f


def kf_update(f, z):
    """Every component on its own (H-03): k = P[:, 0] / (P00 + R), x += k (z - x0), then the Joseph form as B = P - k P[0, :],
    N = (B - B[:, 0] k^T) + (k R) k^T."""
    f = list(f)
    for i in range(4):
        o, R = i * 6, R_PAIR[i]
        p00, p01, p10, p11 = f[o + 2:o + 6]
        S = p00 + R
        k0, k1 = _div(p00, S), _div(p10, S)
        y = z[i] - f[o]
        f[o] = f[o] + k0 * y
        f[o + 1] = f[o + 1] + k1 * y
        b00, b01, b10, b11 = p00 - k0 * p00, p01 - k0 * p01, p10 - k1 * p00, p11 - k1 * p01
        r0, r1 = k0 * R, k1 * R
        f[o + 2] = (b00 - b00 * k0) + r0 * k0
        f[o + 3] = (b01 - b00 * k1) + r0 * k1
        f[o + 4] = (b10 - b10 * k0) + r1 * k0
        f[o + 5] = (b11 - b10 * k1) + r1 * k1
    P = f[25]
    k = _div(P, P + R_R)
    f[24] = f[24] + k * (z[4] - f[24])
    b = P - k * P
    f[25] = (b - b * k) + (k * R_R) * k
    return f


def kf_oru(ff, z1, z2, g, counters=None):
    """Observation-centric re-update: from the frozen filter, g virtual observations on the line z1 -> z2 (x, y, w, h and the
    confidence interpolated), a predict between them; the caller's ordinary update with z2 follows (O-02)."""
    f = list(ff)
    w1, h1 = _sqrt(z1[2] * z1[4]), _sqrt(_div(z1[2], z1[4]))
    w2, h2 = _sqrt(z2[2] * z2[4]), _sqrt(_div(z2[2], z2[4]))
    gf = float(g)
    dx, dy, dw, dh, dc = (z2[0] - z1[0]) / gf, (z2[1] - z1[1]) / gf, (w2 - w1) / gf, (h2 - h1) / gf, (z2[3] - z1[3]) / gf
    for i in range(1, g + 1):
        fi = float(i)
        vw, vh = w1 + fi * dw, h1 + fi * dh
        f = kf_update(f, [z1[0] + fi * dx, z1[1] + fi * dy, vw * vh, z1[3] + fi * dc, _div(vw, vh)])
        if i < g:
            f = kf_predict(f)
        if counters is not None:
            counters["oru"] += 1
    return f


def flt_to_dense(f):
    """flt -> upstream's x[9] = [x, y, s, c, r, vx, vy, vs, vc] and the dense P[81]; off-block entries +0.0."""
    x, P = [0.0] * 9, [0.0] * 81
    for i in range(4):
        o = i * 6
        x[i], x[5 + i] = f[o], f[o + 1]
        P[i * 9 + i], P[i * 9 + 5 + i], P[(5 + i) * 9 + i], P[(5 + i) * 9 + 5 + i] = f[o + 2:o + 6]
    x[4], P[4 * 9 + 4] = f[24], f[25]
    return x, P


def flt_to_box(f):
    """the filter's box: w = sqrt(s r), h = s / w."""
    w = _sqrt(f[12] * f[24])
    h = _div(f[12], w)
    return [f[0] - w / 2.0, f[6] - h / 2.0, f[0] + w / 2.0, f[6] + h / 2.0]


def _clip(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


# ---- costs ---------------------------------------------------------------------------------------------------------------------
def assoc_matrix(d, t, asso):
    """A of xyxy rows d [D,4] x t [T,4]: IoU (O-11), or with "hmiou" IoU times the height overlap ratio; 0 where IoU is 0 (H-04)."""
    iou = iou_matrix(d, t)
    if asso != "hmiou":
        return iou, iou
    d = np.asarray(d, np.float64).reshape(-1, 4)[:, None, :]
    t = np.asarray(t, np.float64).reshape(-1, 4)[None, :, :]
    with np.errstate(all="ignore"):
        num = np.minimum(d[..., 3], t[..., 3]) - np.maximum(d[..., 1], t[..., 1])
        den = np.maximum(d[..., 3], t[..., 3]) - np.minimum(d[..., 1], t[..., 1])
        ok = (iou > 0.0) & (den > 0.0)
        a = iou * (num / np.where(ok, den, 1.0))
    return np.where(ok, a, 0.0), iou


def corner_direction(b0, b1, k):
    """unit vector from corner k of box b0 to corner k of box b1, norm sqrt(dx^2 + dy^2) + 1e-6."""
    ix, iy = CORNERS[k]
    dx, dy = b1[ix] - b0[ix], b1[iy] - b0[iy]
    n = _sqrt(dx * dx + dy * dy) + 1e-6
    return dx / n, dy / n


class Track:
    __slots__ = ("f", "ff", "frozen", "observed", "id", "age", "tsu", "hits", "streak", "has_obs", "lobs", "obs", "vel",
                 "score", "cprev", "has_prev", "cls", "det", "dead", "pbox", "kobs", "ckal", "clin", "mdet")


class HybridSortRef:
    """One stream of Hybrid-SORT (docs/HYBRIDSORT.md §1)."""

    def __init__(self, cfg: Optional[HybridSortConfig] = None):
        self.cfg = cfg or HybridSortConfig()
        self.reset()

    def reset(self):
        self.trackers: List[Track] = []
        self.frame_count = 0
        self.next_id = 1
        self.capacity_error = False
        self.counters = dict(oru=0, oru_tracks=0, lsap=0, shortcut=0, clamp=0, ocr=0, byte=0, match=0, tcm=0, height=0,
                             byte_tcm_refused=0, vel_sum=0, vel_over_one=0)

    def _k_obs(self, t):
        if not t.has_obs:
            return None
        for dt in range(self.cfg.delta_t, 0, -1):
            if t.age - dt in t.obs:
                return t.obs[t.age - dt]
        return t.lobs

    def _matched(self, t, d):
        c = self.cfg
        box = self._box[d]
        z1 = None
        if t.has_obs:
            vel, found = [0.0] * 8, 0
            for dt in range(c.delta_t, 0, -1):                     # H-06: the sum over the stored observations, oldest first
                if t.age - dt in t.obs:
                    found += 1
                    for k in range(4):
                        ux, uy = corner_direction(t.obs[t.age - dt], box, k)
                        vel[2 * k], vel[2 * k + 1] = vel[2 * k] + ux, vel[2 * k + 1] + uy
            if not found:
                for k in range(4):
                    vel[2 * k], vel[2 * k + 1] = corner_direction(t.lobs, box, k)
            t.vel = vel
            self.counters["vel_sum"] += found > 1
            self.counters["vel_over_one"] += any(vel[2 * k] * vel[2 * k] + vel[2 * k + 1] * vel[2 * k + 1] > 1.0000001 for k in range(4))
            z1 = box_to_z5(t.lobs, t.score)
        t.lobs, t.has_obs = box, True
        t.obs[t.age] = box
        for a in [a for a in t.obs if a <= t.age - c.delta_t]:
            del t.obs[a]
        g = t.tsu
        t.tsu = 0
        t.hits += 1
        t.streak += 1
        t.cprev, t.has_prev = t.score, True                        # H-07: a flag, not upstream's truthiness
        t.score, t.cls, t.det = self._score[d], self._cls[d], d
        z2 = box_to_z5(box, t.score)
        if t.frozen:
            t.f = kf_oru(t.ff, z1, z2, g, self.counters)
            t.frozen = False
            self.counters["oru_tracks"] += 1
        t.f = kf_update(t.f, z2)
        t.observed = True
        self.counters["match"] += 1

    def _second(self, rows, ut, boxes, clin, weight, count):
        """BYTE stage / OCR: A (minus the TCM term with clin) of the rows x the tracks ut; solved when some entry exceeds the
        threshold, pairs at or above it are kept.  -> [(row position, position in ut)]"""
        c = self.cfg
        a, plain = assoc_matrix([self._box[i] for i in rows], boxes, c.asso)
        self.counters["height"] += int(((a != plain) & (plain > 0.0)).sum())
        b = a
        if clin is not None:
            sc = np.array([np.float64(self._score[i]) for i in rows])[:, None]
            b = a - np.abs(sc - np.array(clin)[None, :]) * weight
        if not (b > c.iou_threshold).any():
            if clin is not None and (a > c.iou_threshold).any():
                self.counters["byte_tcm_refused"] += 1
            return []
        out = []
        for r, k in lsap(-b):
            if b[r, k] < c.iou_threshold:
                if clin is not None and not a[r, k] < c.iou_threshold:
                    self.counters["byte_tcm_refused"] += 1
                continue
            out.append((r, k))
            self.counters[count] += 1
        return out

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
        high = [i for i in range(N) if self._score[i] > hi_t]
        second = [i for i in range(N) if lo_t < self._score[i] < hi_t] if c.use_byte else []
        trks = self.trackers
        n_live = len(trks)
        # 2. predict every track, its two confidences
        for t in trks:
            if t.f[13] + t.f[12] <= 0.0:
                t.f[13] = 0.0
                self.counters["clamp"] += 1
            t.f = kf_predict(t.f)
            t.age += 1
            if t.tsu > 0:
                t.streak = 0
            t.tsu += 1
            t.pbox = flt_to_box(t.f)
            t.dead = not (all(math.isfinite(v) for v in t.pbox) and math.isfinite(t.f[18]))      # O-10, and the confidence state
            t.ckal = _clip(t.f[18], float(c.det_thresh), 1.0)
            conf = float(np.float64(t.score))
            t.clin = _clip(conf + (conf - float(np.float64(t.cprev))) if t.has_prev else conf, float(c.low_thresh), float(c.det_thresh))
            t.kobs = self._k_obs(t)
            t.mdet = -1
        T, H = len(trks), len(high)
        used = [False] * H
        # 3. first association: high rows x all tracks
        if T and H:
            hb = np.array([self._box[i] for i in high], np.float64).reshape(-1, 4)
            a, plain = assoc_matrix(hb, [t.pbox for t in trks], c.asso)
            live = np.array([not t.dead for t in trks])
            a = np.where(live[None, :], a, 0.0)
            self.counters["height"] += int(((a != plain) & (plain > 0.0) & live[None, :]).sum())
            valid = np.array([t.kobs is not None and not t.dead for t in trks])
            sc = np.array([np.float64(self._score[i]) for i in high])[:, None]
            ssum = np.zeros((H, T))
            for k, (ix, iy) in enumerate(CORNERS):
                kx = np.array([0.0 if t.kobs is None else t.kobs[ix] for t in trks])
                ky = np.array([0.0 if t.kobs is None else t.kobs[iy] for t in trks])
                dx, dy = hb[:, ix][:, None] - kx[None, :], hb[:, iy][:, None] - ky[None, :]
                n = np.sqrt(dx * dx + dy * dy) + 1e-6
                cs = np.array([t.vel[2 * k] for t in trks])[None, :] * (dx / n) + np.array([t.vel[2 * k + 1] for t in trks])[None, :] * (dy / n)
                with np.errstate(invalid="ignore"):
                    cs = np.where(cs < -1.0, -1.0, np.where(cs > 1.0, 1.0, cs))
                cs = np.where(valid[None, :], cs, 0.0)
                ssum = ssum + ss_asin(cs)
            term = ssum / PI
            term = term * c.inertia
            term = term * sc
            term = np.where(valid[None, :], term, 0.0)
            with np.errstate(invalid="ignore"):
                tcm = np.abs(sc - np.array([t.ckal for t in trks])[None, :]) * c.tcm_first_weight
            tcm = np.where(live[None, :], tcm, 0.0)
            self.counters["tcm"] += int((tcm != 0.0).sum())
            above = a > c.iou_threshold
            if above.any() and above.sum(1).max() == 1 and above.sum(0).max() == 1:
                pairs = [(int(r), int(k)) for r, k in zip(*np.nonzero(above))]
                self.counters["shortcut"] += 1
            else:
                pairs = lsap(-((a + term) - tcm))
                self.counters["lsap"] += 1
            for r, k in pairs:
                if a[r, k] < c.iou_threshold or trks[k].dead:
                    continue
                trks[k].mdet = high[r]
                used[r] = True
        # 4. BYTE stage: second rows x the unmatched tracks' predicted boxes, A minus the TCM term on the linear confidence
        ut = [k for k in range(T) if trks[k].mdet < 0 and not trks[k].dead]
        if second and ut:
            for r, k in self._second(second, ut, [trks[k].pbox for k in ut], [trks[k].clin for k in ut], c.tcm_byte_weight, "byte"):
                trks[ut[k]].mdet = second[r]
        # 5. OCR: the high rows left x the remaining tracks' last observations
        ut = [k for k in range(T) if trks[k].mdet < 0 and not trks[k].dead]
        ud = [r for r in range(H) if not used[r]]
        if ud and ut:
            # a track without an observation: an empty box at the origin, whose A is 0 with every row (O-11)
            boxes = [trks[k].lobs if trks[k].has_obs else [0.0, 0.0, 0.0, 0.0] for k in ut]
            for r, k in self._second([high[r] for r in ud], ut, boxes, None, 0.0, "ocr"):
                trks[ut[k]].mdet = high[ud[r]]
                used[ud[r]] = True
        # 6. update
        for t in trks:
            if t.mdet >= 0:
                self._matched(t, t.mdet)
            else:
                if t.observed:
                    t.ff, t.frozen = list(t.f), True
                t.observed = False
        # 7. births
        births = []
        for r in range(H):
            if used[r]:
                continue
            if n_live + len(births) >= c.max_tracks:
                self.capacity_error = True
                continue
            d = high[r]
            t = Track()
            t.f = kf_init(box_to_z5(self._box[d], self._score[d]))
            t.ff, t.frozen, t.observed = None, False, False
            t.id = self.next_id
            self.next_id += 1
            t.age = t.tsu = t.hits = t.streak = 0
            t.has_obs, t.lobs, t.obs, t.vel = False, self._box[d], {}, [0.0] * 8
            t.score, t.cprev, t.has_prev, t.cls, t.det, t.dead = self._score[d], np.float32(0.0), False, self._cls[d], d, False
            births.append(t)
        # 8. the list and the rows (newest first)
        self.trackers = [t for t in trks if not (t.tsu > c.max_age) and not t.dead] + births
        rows = []
        for t in reversed(self.trackers):
            if t.tsu < 1 and (t.streak >= c.min_hits or self.frame_count <= c.min_hits):
                rows.append([t.lobs[0], t.lobs[1], t.lobs[2], t.lobs[3], t.id, t.cls, t.score, t.det])
        return np.asarray(rows, np.float32).reshape(-1, 8)

    def tracks(self) -> dict:
        """The table in list order — what ss_hybridsort_get_tracks returns."""
        ts = self.trackers
        i32 = lambda f: np.array([f(t) for t in ts], np.int32)
        dense = [flt_to_dense(t.f) for t in ts]
        return dict(track_id=i32(lambda t: t.id), age=i32(lambda t: t.age), time_since_update=i32(lambda t: t.tsu),
                    hits=i32(lambda t: t.hits), hit_streak=i32(lambda t: t.streak), frozen=i32(lambda t: int(t.frozen)),
                    x=np.array([d[0] for d in dense], np.float64).reshape(-1, 9), P=np.array([d[1] for d in dense], np.float64).reshape(-1, 81),
                    last_obs=np.array([t.lobs if t.has_obs else [-1.0] * 4 for t in ts], np.float32).reshape(-1, 4),
                    velocity=np.array([t.vel for t in ts], np.float64).reshape(-1, 8),
                    conf=np.array([t.score for t in ts], np.float32), conf_prev=np.array([t.cprev if t.has_prev else -1.0 for t in ts], np.float32),
                    n_tracks=len(ts), next_id=self.next_id, frame_count=self.frame_count)
