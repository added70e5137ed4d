"""Executable form of docs/OBB.md: ProbIoU as the fixed float64 sequence of csrc/ss_probiou.h (same constants, same order), the row
post-steps of the rotated NMS (scale, regularise, envelope) and nms_rotated itself (R-02: a candidate is removed by ANY higher-scored
overlapping candidate).  NumPy float64 element-wise operations round once each and never contract, so array arguments give the bits the
scalar sequence gives.  Recalled from Ultralytics 8.3.x; no Ultralytics checkout was consulted."""
import numpy as np

from tests.botsort_pose_ref import EXPNEG_C, EXPNEG_CUT, EXPNEG_LN2_HI, EXPNEG_LN2_LO, EXPNEG_LOG2E

EPS = 1e-7
SINCOS_MAX = 1048576.0
LOG_C = [1.0, 0.3333333333333333, 0.2, 0.14285714285714285, 0.1111111111111111, 0.09090909090909091, 0.07692307692307693,
         0.06666666666666667, 0.058823529411764705, 0.05263157894736842, 0.047619047619047616, 0.043478260869565216]
SIN_C = [1.0, -0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06, -2.505210838544172e-08,
         1.6059043836821613e-10, -7.647163731819816e-13, 2.8114572543455206e-15]
COS_C = [1.0, -0.5, 0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05, -2.755731922398589e-07,
         2.08767569878681e-09, -1.1470745597729725e-11, 4.779477332387385e-14, -1.5619206968586225e-16]
TWO_OVER_PI = 0.6366197723675814
PIO2_1, PIO2_2, PIO2_3, PIO2_3T = 1.57079632673412561417e+00, 6.07710050630396597660e-11, 2.02226624871116645580e-21, 8.47842766036889956997e-32
SQRT2 = 1.4142135623730951
F32_PI, F32_PI_2 = np.float32(3.14159274101257324), np.float32(1.57079637050628662)


def _f64(x):
    return np.atleast_1d(np.asarray(x, np.float64))


def ss_expneg(x):
    """tests/botsort_pose_ref.ss_expneg on arrays"""
    x = _f64(x)
    with np.errstate(all="ignore"):
        ok = x <= EXPNEG_CUT
        y = -np.where(ok, x, 0.0)
        k = np.floor(y * EXPNEG_LOG2E + 0.5)
        r = (y - k * EXPNEG_LN2_HI) - k * EXPNEG_LN2_LO
        p = np.full_like(r, EXPNEG_C[12])
        for i in range(11, -1, -1):
            p = p * r + EXPNEG_C[i]
        return np.where(ok, np.ldexp(p, k.astype(np.int32)), 0.0)


def ss_log(x):
    x = _f64(x)
    with np.errstate(all="ignore"):
        ok = (x >= 2.2250738585072014e-308) & (x <= 1.7976931348623157e308)
        m, e = np.frexp(np.where(ok, x, 1.0))            # m in [1/2, 1)
        m = m * 2.0
        e = e - 1
        big = m > SQRT2
        m = np.where(big, m * 0.5, m)
        e = np.where(big, e + 1, e)
        f = m - 1.0
        s = f / (2.0 + f)
        z = s * s
        p = np.full_like(z, LOG_C[-1])
        for k in range(len(LOG_C) - 2, -1, -1):
            p = p * z
            p = p + LOG_C[k]
        r = 2.0 * s
        r = r * p
        de = e.astype(np.float64)
        lo = de * EXPNEG_LN2_LO
        lo = r + lo
        hi = de * EXPNEG_LN2_HI
        return np.where(ok, hi + lo, np.nan)


def ss_sincos(t):
    t = _f64(t)
    with np.errstate(all="ignore"):
        ok = np.abs(t) <= SINCOS_MAX
        t = np.where(ok, t, 0.0)
        k = np.floor(t * TWO_OVER_PI + 0.5)
        r = t - k * PIO2_1
        r = r - k * PIO2_2
        r = r - k * PIO2_3
        r = r - k * PIO2_3T
        z = r * r
        ps = np.full_like(z, SIN_C[-1])
        for i in range(len(SIN_C) - 2, -1, -1):
            ps = ps * z
            ps = ps + SIN_C[i]
        pc = np.full_like(z, COS_C[-1])
        for i in range(len(COS_C) - 2, -1, -1):
            pc = pc * z
            pc = pc + COS_C[i]
        ps = r * ps
        q = k.astype(np.int64) & 3
        sn = np.select([q == 0, q == 1, q == 2], [ps, pc, -ps], -pc)
        cs = np.select([q == 0, q == 1, q == 2], [pc, -ps, -pc], ps)
        return np.where(ok, sn, np.nan), np.where(ok, cs, np.nan)


def box_terms(boxes):
    """float32 [n, 5] (cx, cy, w, h, theta) -> float64 [n, 6] (x, y, A, B, C, D); D = -1 marks a degenerate box (R-01)."""
    b = np.asarray(boxes, np.float32).reshape(-1, 5).astype(np.float64)
    with np.errstate(all="ignore"):
        x, y, w, h = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        s, c = ss_sincos(b[:, 4])
        bad = ~(np.abs(x) <= 3.5e38) | ~(np.abs(y) <= 3.5e38) | ~(np.abs(w) <= 3.5e38) | ~(np.abs(h) <= 3.5e38) | ~(w > 0.0) | ~(h > 0.0) | (s != s)
        a_, b_ = w * w / 12.0, h * h / 12.0
        cc, ss = c * c, s * s
        A = a_ * cc + b_ * ss
        B = a_ * ss + b_ * cc
        C = (a_ - b_) * c * s
        D = A * B - C * C
        D = np.where(D > 0.0, D, 0.0)
        out = np.stack([x, y, A, B, C, D], axis=1)
        out[bad, 2:5] = 0.0
        out[bad, 5] = -1.0
    return out


def probiou_terms(P, Q):
    """terms [n, 6] x [m, 6] -> float64 [n, m]"""
    P, Q = P[:, None, :], Q[None, :, :]
    with np.errstate(all="ignore"):
        sa, sb, sc = P[..., 2] + Q[..., 2], P[..., 3] + Q[..., 3], P[..., 4] + Q[..., 4]
        dx, dy = P[..., 0] - Q[..., 0], P[..., 1] - Q[..., 1]
        den = sa * sb - sc * sc
        de = den + EPS
        t1 = (sa * dy * dy + sb * dx * dx) / de * 0.25
        t2 = sc * (-dx) * dy / de * 0.5
        t3 = 0.5 * ss_log((den / (4.0 * np.sqrt(np.where(P[..., 5] * Q[..., 5] > 0, P[..., 5] * Q[..., 5], 0.0)) + EPS) + EPS).ravel()).reshape(den.shape)
        bd = t1 + t2 + t3
        nan = bd != bd
        bd = np.where(nan, EPS, bd)
        bd = np.where(bd < EPS, EPS, bd)
        bd = np.where(bd > 100.0, 100.0, bd)
        v = 1.0 - np.sqrt(1.0 - ss_expneg(bd.ravel()).reshape(bd.shape) + EPS)
        return np.where(nan | (P[..., 5] < 0.0) | (Q[..., 5] < 0.0), 0.0, v)


def probiou(a, b):
    """float32 [n, 5] x [m, 5] -> float64 [n, m]"""
    return probiou_terms(box_terms(a), box_terms(b))


# ---- row post-steps (docs/OBB.md §3: float32, one operation per step) ------------------------------------------------------------------
def scale_rbox(xywhr, gain, pad_x, pad_y):
    """network-input pixels -> original-image pixels, no clipping (R-04)"""
    b = np.asarray(xywhr, np.float32).reshape(-1, 5).copy()
    g, px, py = np.float32(gain), np.float32(pad_x), np.float32(pad_y)
    b[:, 0] = (b[:, 0] - px) / g
    b[:, 1] = (b[:, 1] - py) / g
    b[:, 2] = b[:, 2] / g
    b[:, 3] = b[:, 3] / g
    return b


def regularise(xywhr):
    """R-05: w > h keeps (w, h, theta); otherwise swap and theta += pi/2; then one +pi if theta < 0, or one -pi if theta >= pi (float32)."""
    b = np.asarray(xywhr, np.float32).reshape(-1, 5).copy()
    keep = b[:, 2] > b[:, 3]
    w = np.where(keep, b[:, 2], b[:, 3])
    h = np.where(keep, b[:, 3], b[:, 2])
    t = np.where(keep, b[:, 4], b[:, 4] + F32_PI_2).astype(np.float32)
    t = np.where(t < np.float32(0), t + F32_PI, np.where(t >= F32_PI, t - F32_PI, t)).astype(np.float32)
    b[:, 2], b[:, 3], b[:, 4] = w, h, t
    return b


def corners(xywhr):
    """float32 [n, 5] -> float64 [n, 4, 2]: ctr + v1 + v2, ctr + v1 - v2, ctr - v1 - v2, ctr - v1 + v2 with v1 = (w/2)(cos, sin),
    v2 = (h/2)(-sin, cos): upstream's corner order"""
    b = np.asarray(xywhr, np.float32).reshape(-1, 5).astype(np.float64)
    s, c = ss_sincos(b[:, 4])
    hw, hh = b[:, 2] / 2.0, b[:, 3] / 2.0
    vx, vy, ux, uy = hw * c, hw * s, hh * s, hh * c
    cx, cy = b[:, 0], b[:, 1]
    xs = np.stack([cx + vx - ux, cx + vx + ux, cx - vx + ux, cx - vx - ux], axis=1)
    ys = np.stack([cy + vy + uy, cy + vy - uy, cy - vy - uy, cy - vy + uy], axis=1)
    return np.stack([xs, ys], axis=2)


def envelope(xywhr, w0, h0):
    """axis-aligned envelope of the rotated box: min / max of the float64 corners, rounded to float32, clipped to the image"""
    p = corners(xywhr)
    lo, hi = p.min(axis=1).astype(np.float32), p.max(axis=1).astype(np.float32)
    w0, h0, z = np.float32(w0), np.float32(h0), np.float32(0)
    return np.stack([np.minimum(np.maximum(lo[:, 0], z), w0), np.minimum(np.maximum(lo[:, 1], z), h0),
                     np.minimum(np.maximum(hi[:, 0], z), w0), np.minimum(np.maximum(hi[:, 1], z), h0)], axis=1).astype(np.float32)


# ---- nms_rotated ----------------------------------------------------------------------------------------------------------------------
def candidates(pred, nc, conf, classes=None):
    """k_nms_filter: best class per anchor (first maximum), score > conf, classes mask; order: descending score, ties by anchor."""
    pred = np.asarray(pred, np.float32)
    sc = pred[4:4 + nc]
    cls = sc.argmax(axis=0)
    best = sc.max(axis=0)
    ok = best > np.float32(conf)
    if classes is not None:
        ok &= np.isin(cls, np.asarray(list(classes)))
    idx = np.nonzero(ok)[0]
    order = np.lexsort((idx, -best[idx].astype(np.float64)))
    return idx[order], best[idx][order], cls[idx][order]


def removed_mask(terms, cls, iou_thres, agnostic, block=256):
    """R-02 / R-03: removed[j] = some i < j has probiou(i, j) >= float32(iou_thres) (and, unless agnostic, the same class).  A candidate
    that is already removed needs no further rows: `any` is decided."""
    n = len(terms)
    removed = np.zeros(n, bool)
    thr = float(np.float32(iou_thres))
    for i0 in range(0, n, block):
        i1 = min(i0 + block, n)
        js = np.nonzero(~removed & (np.arange(n) > i0))[0]
        if len(js) == 0:
            continue
        v = probiou_terms(terms[i0:i1], terms[js])
        hit = (v >= thr) & (np.arange(i0, i1)[:, None] < js[None, :])
        if not agnostic:
            hit &= cls[i0:i1, None] == cls[None, js]
        removed[js[hit.any(axis=0)]] = True
    return removed


def nms_rotated(pred, nc, conf, iou_thres, agnostic, max_det, geom, classes=None, max_cand=8192):
    """pred float32 [4 + nc + 1][A] in network-input pixels, geom (gain, pad_x, pad_y, w0, h0) -> (keep anchors int32 [k],
    rows float32 [k, 11] = x1, y1, x2, y2, conf, cls, cx, cy, w, h, theta in original-image pixels)."""
    pred = np.asarray(pred, np.float32)
    idx, score, cls = candidates(pred, nc, conf, classes)
    if len(idx) > max_cand:
        return None
    boxes = np.stack([pred[0, idx], pred[1, idx], pred[2, idx], pred[3, idx], pred[4 + nc, idx]], axis=1).reshape(-1, 5)
    removed = removed_mask(box_terms(boxes), cls, iou_thres, agnostic)
    kept = np.nonzero(~removed)[0][:max_det]
    gain, pad_x, pad_y, w0, h0 = geom
    rb = regularise(scale_rbox(boxes[kept], gain, pad_x, pad_y))
    rows = np.zeros((len(kept), 11), np.float32)
    rows[:, :4] = envelope(rb, w0, h0)
    rows[:, 4], rows[:, 5] = score[kept], cls[kept].astype(np.float32)
    rows[:, 6:] = rb
    return idx[kept].astype(np.int32), rows


def greedy_nms(terms, cls, iou_thres, agnostic):
    """what R-02 is NOT: a sequential scan in which a removed candidate removes nothing (the tests pin the difference)"""
    n = len(terms)
    removed = np.zeros(n, bool)
    v = probiou_terms(terms, terms)
    for i in range(n):
        if removed[i]:
            continue
        for j in range(i + 1, n):
            if v[i, j] >= float(np.float32(iou_thres)) and (agnostic or cls[i] == cls[j]):
                removed[j] = True
    return removed


# ---- seeded candidate fields of the NMS tests ------------------------------------------------------------------------------------------
def field_shape(n_cand):
    """anchor count of the field with n_cand candidates: 84 (a 64 x 64 input), 1100, 9000"""
    return (84,) if n_cand <= 84 else (1100,) if n_cand <= 1100 else (9000,)


def probiou_boxes(n, seed):
    """float32 [n, 5]: rows 0..5 degenerate (R-01), then groups of near-copies, right-angle turns and far-apart boxes"""
    base, rng = np.random.default_rng(70), np.random.default_rng(seed)
    b = np.zeros((n, 5), np.float32)
    b[:, :2] = base.uniform(0, 300, (n, 2))
    b[:, 2], b[:, 3] = base.uniform(5, 120, n), base.uniform(5, 40, n)
    b[:, 4] = base.uniform(-np.pi / 4, np.pi, n)
    b[6::5, :4] += rng.uniform(-4, 4, b[6::5, :4].shape).astype(np.float32)          # the seed moves every fifth box: two lists overlap in part
    for i in range(8, n, 3):                                   # i: a near-copy of i - 1
        b[i] = b[i - 1] + np.float32(0.01) * rng.standard_normal(5).astype(np.float32)
    b[0, 2], b[1, 3], b[2, 0], b[3, 1], b[4, 4], b[5, 2] = 0.0, -3.0, np.nan, np.inf, np.float32(2.0e6), np.nan
    return b


def obb_field(n_cand, A, nc, seed, per=None, span=900.0):
    """float32 [4 + nc + 1][A] with exactly n_cand anchors above conf 0.25: clusters of `per` near-copies of an elongated box (jittered
    centre, size and angle; every third member turned by a right angle about the same centre: the envelopes then nearly coincide while
    the rotated overlap is small), class scores with one winner, a few exact score ties.  per: 6, and 64 for the large fields."""
    per = per or (6 if n_cand < 2000 else 64)
    rng = np.random.default_rng(seed)
    pred = np.zeros((4 + nc + 1, A), np.float32)
    pred[0], pred[1] = rng.uniform(0, span, A), rng.uniform(0, span, A)
    pred[2], pred[3] = rng.uniform(20, 60, A), rng.uniform(20, 60, A)
    pred[4:4 + nc] = rng.uniform(0.0, 0.2, (nc, A))
    pred[4 + nc] = rng.uniform(-np.pi / 4, 3 * np.pi / 4, A)
    anchors = rng.permutation(A)[:n_cand]
    ncl = max(1, (n_cand + per - 1) // per)
    ctr = rng.uniform(60, span, (ncl, 2))
    wh = np.stack([rng.uniform(60, 140, ncl), rng.uniform(8, 30, ncl)], axis=1)
    th = rng.uniform(-np.pi / 4, 3 * np.pi / 4, ncl)
    kc = rng.integers(0, nc, ncl)
    for q, a in enumerate(anchors):
        c, m = q // per, q % per
        pred[0, a], pred[1, a] = ctr[c] + rng.uniform(-3, 3, 2)
        pred[2, a], pred[3, a] = wh[c] * rng.uniform(0.9, 1.1, 2)
        t = th[c] + rng.uniform(-0.08, 0.08) + (np.pi / 2 if m % 3 == 2 else 0.0)
        pred[4 + nc, a] = t - np.pi if t >= 3 * np.pi / 4 else t
        k = kc[c] if m != per - 1 else (kc[c] + 1) % nc               # the last member of a cluster carries another class (when nc > 1)
        pred[4 + k, a] = np.float32(0.3) + np.float32(rng.integers(0, 1 << 20)) * np.float32(2.0 ** -21)      # a 2^-21 grid: ties occur
    return pred


# ---- BYTE tracking on rotated boxes (docs/OBB.md §4) ------------------------------------------------------------------------------------
from tests import bytetrack_ref as _bt                                                                            # noqa: E402


class ObbTrack(_bt.Track):
    __slots__ = ("box", "angle")


def envelope_open(xywhr):
    """the envelope without an image to clip to: min / max of the float64 corners, rounded to float32"""
    p = corners(xywhr)
    return np.concatenate([p.min(axis=1), p.max(axis=1)], axis=1).astype(np.float32)


class ByteTrackObbRef(_bt.ByteTrackRef):
    """tests/bytetrack_ref.ByteTrackRef with the cost of the three associations and of the duplicate test swapped for 1 - ProbIoU of the
    rotated boxes, every track carrying the angle of its last row (R-06).  The frame procedure below is ByteTrackRef.update's, step by
    step; what differs is marked OBB.

        rows, rbox = ref.update(dets)   # dets [N, 11] f32 x1, y1, x2, y2, score, cls, cx, cy, w, h, theta (ss_nms_obb_batch's rows)
                                        # -> f32 [M, 8] envelope, id, cls, score, det_idx and f32 [M, 5] cx, cy, w, h, theta
    """

    # OBB: the track's box is the Kalman mean's centre and size (xyah: w = a h), not a tlwh
    def _set_mean(self, t, mean, cov):
        t.mean, t.cov = mean, cov
        t.box = [mean[0], mean[1], mean[2] if self.xywh else mean[2] * mean[3], mean[3]]
        t.tlwh = None

    def _xywhr(self, ts):
        """the float32 boxes the device forms its ProbIoU terms from (and shows in d_out_rbox)"""
        return np.array([[*t.box, t.angle] for t in ts], np.float64).astype(np.float32).reshape(-1, 5)

    def _cost_td(self, ts, idx):
        if not ts or not idx:
            return np.zeros((len(ts), len(idx)))
        return 1.0 - probiou(self._xywhr(ts), self._rb[idx])

    def _update(self, t, d, reactivate=False):
        t.angle = self._rb[d, 4]                                   # R-06, before the box's terms
        super()._update(t, d, reactivate)

    def update(self, dets):
        c = self.cfg
        dets = np.asarray(dets, np.float32).reshape(-1, 11)
        if dets.shape[0] > c.max_dets:
            self.capacity_error = True
            dets = dets[:c.max_dets]
        self.frame_id += 1
        fid = self.frame_id
        N = dets.shape[0]
        self._rb = dets[:, 6:11].copy()
        b = self._rb.astype(np.float64)
        self._z = [[float(b[i, 0]), float(b[i, 1]), float(b[i, 2]) if self.xywh else float(b[i, 2]) / float(b[i, 3]), float(b[i, 3])]
                   for i in range(N)]
        self._score = [np.float32(dets[i, 4]) for i in range(N)]
        self._cls = [np.float32(dets[i, 5]) for i in range(N)]
        hi_t, lo_t = np.float32(c.track_high_thresh), np.float32(c.track_low_thresh)
        high = [i for i in range(N) if self._score[i] >= hi_t]
        low = [i for i in range(N) if lo_t < self._score[i] < hi_t]
        unconf = [t for t in self.tracked if not t.activated]
        pool = [t for t in self.tracked if t.activated] + list(self.lost)
        n_live = len(self.tracked) + len(self.lost)
        for t in pool:
            m = list(t.mean)
            if t.state != _bt.TRACKED:
                m[7] = 0.0
                if self.xywh:
                    m[6] = 0.0
            m, P = _bt.kf_predict(m, t.cov, self.xywh, c.std_weight_position, c.std_weight_velocity)
            self._set_mean(t, m, P)
        refound = []
        cost = self._cost_td(pool, high)
        if c.fuse_score and cost.size:
            cost = _bt.fuse_score(cost, [self._score[i] for i in high])
        pairs, u_pool, u_high = _bt.assign(cost, c.match_thresh)
        for r, k in pairs:
            t = pool[r]
            if t.state == _bt.TRACKED:
                self._update(t, high[k])
            else:
                self._update(t, high[k], reactivate=True)
                refound.append(t)
        r2 = [pool[r] for r in u_pool if pool[r].state == _bt.TRACKED]
        pairs, u_r2, _ = _bt.assign(self._cost_td(r2, low), 0.5)
        for r, k in pairs:
            self._update(r2[r], low[k])
        new_lost = []
        for r in u_r2:
            if r2[r].state != _bt.LOST:
                r2[r].state = _bt.LOST
                new_lost.append(r2[r])
        left = [high[k] for k in u_high]
        cost = self._cost_td(unconf, left)
        if c.fuse_score and cost.size:
            cost = _bt.fuse_score(cost, [self._score[i] for i in left])
        pairs, u_unc, u_left = _bt.assign(cost, 0.7)
        for r, k in pairs:
            self._update(unconf[r], left[k])
        for r in u_unc:
            unconf[r].state = _bt.REMOVED
        births = []
        for k in u_left:
            d = left[k]
            if self._score[d] < np.float32(c.new_track_thresh):
                continue
            if n_live + len(births) >= c.max_tracks:
                self.capacity_error = True
                continue
            t = ObbTrack()
            t.id = self.next_id
            self.next_id += 1
            t.angle = self._rb[d, 4]                               # R-06
            m, P = _bt.kf_initiate(self._z[d], self.xywh, c.std_weight_position, c.std_weight_velocity)
            self._set_mean(t, m, P)
            t.tracklet_len, t.state, t.activated = 0, _bt.TRACKED, fid == 1
            t.start = t.end = fid
            t.score, t.cls, t.det = self._score[d], self._cls[d], d
            births.append(t)
        for t in self.lost:
            if t.state == _bt.LOST and fid - t.end > self.max_time_lost:
                t.state = _bt.REMOVED
        tracked = [t for t in self.tracked if t.state == _bt.TRACKED] + births + refound
        lost = [t for t in self.lost if t.state == _bt.LOST] + new_lost
        self.n_duplicates = getattr(self, "n_duplicates", 0)
        if tracked and lost:
            d = 1.0 - probiou(self._xywhr(tracked), self._xywhr(lost))
            dup_a, dup_b = set(), set()
            for p, q in zip(*np.nonzero(d < 0.15)):
                tp, tq = tracked[p].end - tracked[p].start, lost[q].end - lost[q].start
                if tp > tq:
                    dup_b.add(int(q))
                else:
                    dup_a.add(int(p))
            self.n_duplicates += len(dup_a) + len(dup_b)
            tracked = [t for i, t in enumerate(tracked) if i not in dup_a]
            lost = [t for i, t in enumerate(lost) if i not in dup_b]
        self.n_refound = getattr(self, "n_refound", 0) + len(refound)
        self.tracked, self.lost = tracked, lost
        out = [t for t in self.tracked if t.activated]
        rbox = self._xywhr(out)
        env = envelope_open(rbox) if out else np.zeros((0, 4), np.float32)
        rows = np.zeros((len(out), 8), np.float32)
        rows[:, :4] = env
        for i, t in enumerate(out):
            rows[i, 4:] = [t.id, t.cls, t.score, t.det]
        return rows, rbox

    def angles(self):
        return np.array([t.angle for t in self.tracked + self.lost], np.float32)


def obb_rows(xywhr, score, cls, w0=1e6, h0=1e6):
    """[n, 11] rows as ss_nms_obb_batch writes them from regularised boxes: envelope, score, class, cx, cy, w, h, theta"""
    b = np.asarray(xywhr, np.float32).reshape(-1, 5)
    rows = np.zeros((b.shape[0], 11), np.float32)
    if b.shape[0]:
        rows[:, :4] = envelope(b, w0, h0)
    rows[:, 4], rows[:, 5], rows[:, 6:] = score, cls, b
    return rows


def rotating_scene(seed, frames=40, n=6, lane=18.0):
    """Seeded frames of elongated boxes that rotate and cross (docs/OBB.md §4): two lanes of long boxes that pass through one another
    at different angles (their envelopes overlap long before the boxes do), a box that vanishes for a few frames and comes back (lost,
    then re-found), and one whose score drops below the birth threshold so that a second, young track is born on it and then loses the
    duplicate test.  lane: the lanes' spacing (at 6 the boxes themselves overlap while they pass).  -> list of [n_f, 11] float32 rows"""
    rng = np.random.default_rng(seed)
    out = []
    x0 = rng.uniform(100.0, 200.0, n)
    y0 = 200.0 + lane * np.arange(n) + rng.uniform(-2.0, 2.0, n)
    vx = np.where(np.arange(n) % 2 == 0, 9.0, -9.0) + rng.uniform(-1.0, 1.0, n)
    x0 = np.where(np.arange(n) % 2 == 0, x0, x0 + 360.0)
    th0 = rng.uniform(0.0, np.pi, n)
    om = rng.uniform(-0.06, 0.06, n)
    for f in range(frames):
        boxes, sc = [], []
        for i in range(n):
            if i == 1 and 12 <= f < 17:                           # gone: lost, then re-found
                continue
            x, y = x0[i] + vx[i] * f, y0[i] + 3.0 * np.sin(0.3 * f + i)
            th = (th0[i] + om[i] * f) % np.pi
            s = 0.9 - 0.01 * i
            if i == 2 and 20 <= f < 24:                           # low score: second association only
                s = 0.3
            boxes.append([x, y, 90.0 + 2.0 * i, 14.0 + i, th])
            sc.append(s)
            if i == 3 and 22 <= f < 30:                           # a near copy: a young track on the same object
                boxes.append([x + 0.5, y + 0.25, 96.0, 17.0, th])
                sc.append(0.8)
        b = regularise(np.asarray(boxes, np.float32).reshape(-1, 5))
        out.append(obb_rows(b, np.asarray(sc, np.float32), np.zeros(len(sc), np.float32)))
    return out
