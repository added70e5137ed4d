"""CPU reference of BoT-SORT's keypoint term (docs/BYTETRACK.md §1e, decisions K-01..): the OKS entry of the first and third
associations and the tracks' stored poses, on top of tests/bytetrack_ref.py and tests/botsort_gmc_ref.py.

Not a conftest and not a test module: imported by tests/test_botsort_pose_cpu.py and tests/test_gpu_botsort_pose.py.

    ref = BotSortPoseRef()                       # ByteTrackConfig(kalman="xywh", with_pose=True) by default
    rows = ref.update(dets, kpts, warp=None)     # kpts [N,K,3] float32 (x, y, v) in the dets' pixels; warp as BotSortGmcRef.update

Every product, sum and quotient below is one rounded float64 operation (no fma), as the device computes it with
-ffp-contract=off; `ss_expneg` is the fixed operation sequence of §1e, which csrc/ss_byte.hip runs with the same constants.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from strongsort_yolo_amd.config import ByteTrackConfig
import tests.bytetrack_ref as _bt
from tests.botsort_gmc_ref import BotSortGmcRef

# ---- ss_expneg (§1e, K-06): exp(-x) for x >= 0 as one fixed sequence of float64 operations ----------------------------------
EXPNEG_CUT = 700.0                                    # above it (and for a NaN) the result is 0
EXPNEG_LOG2E = float.fromhex("0x1.71547652b82fep+0")  # 1 / ln 2
EXPNEG_LN2_HI = float.fromhex("0x1.62e42feep-1")      # ln 2, the upper 32 bits: k * LN2_HI is exact for |k| < 2^20
EXPNEG_LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
EXPNEG_C = tuple(1.0 / math.factorial(i) for i in range(13))          # 1 / i!, correctly rounded (i! is exact)


def ss_expneg(x: float) -> float:
    x = float(x)
    if not x <= EXPNEG_CUT:
        return 0.0
    y = -x
    k = math.floor(y * EXPNEG_LOG2E + 0.5)
    kf = float(k)
    r = (y - kf * EXPNEG_LN2_HI) - kf * EXPNEG_LN2_LO
    p = EXPNEG_C[12]
    for i in range(11, -1, -1):
        p = p * r + EXPNEG_C[i]
    return math.ldexp(p, k)


# ---- keypoints ----------------------------------------------------------------------------------------------------
def visible(kpts, vis_thresh) -> np.ndarray:
    """[.., K, 3] float32 -> bool [.., K]: v >= float32(kpt_vis_thresh), a float32 comparison (B-04)."""
    return np.asarray(kpts, np.float32)[..., 2] >= np.float32(vis_thresh)


def original_pixels(kpts, gain, pad_x, pad_y) -> np.ndarray:
    """k_byte_kpts' geometry path: network-input pixels -> original-frame pixels, (k - pad) / gain in float32 (the floats
    Results.keypoints shows); the visibility column is kept."""
    k = np.array(kpts, np.float32, copy=True)
    k[..., 0] = (k[..., 0] - np.float32(pad_x)) / np.float32(gain)
    k[..., 1] = (k[..., 1] - np.float32(pad_y)) / np.float32(gain)
    return k


def track_pose(z, kpts, vis):
    """The pose a track stores from its matched / birth detection: z = (cx, cy, w, h) of the detection (float64, the measurement
    of the xywh filter), kpts [K,3] f32, vis bool [K] -> (offsets [K][2] float64, visibility [K]); all invisible if w <= 0 or h <= 0."""
    cx, cy, w, h = (float(v) for v in z)
    K = len(vis)
    if w <= 0 or h <= 0:
        return [[0.0, 0.0] for _ in range(K)], [False] * K
    off = [[(float(np.float64(kpts[k][0])) - cx) / w, (float(np.float64(kpts[k][1])) - cy) / h] for k in range(K)]
    return off, [bool(v) for v in vis]


def oks_entry(cfg: ByteTrackConfig, mean, pose, pvis, dkp, dvis, dtlwh) -> float:
    """§1e steps 3-5 for one pair: the track's predicted mean (cx, cy, w, h), its stored pose, the detection's keypoints and box."""
    cx, cy, w, h = (float(v) for v in mean[:4])
    area = float(dtlwh[2]) * float(dtlwh[3])
    common = [k for k in range(len(pvis)) if pvis[k] and dvis[k]]
    if len(common) < cfg.min_common_kpts or not area > 0.0:
        return 1.0
    acc = 0.0
    for k in common:
        px, py = cx + pose[k][0] * w, cy + pose[k][1] * h
        dx, dy = px - float(np.float64(dkp[k][0])), py - float(np.float64(dkp[k][1]))
        d2 = dx * dx + dy * dy
        s2 = 2.0 * float(cfg.kpt_sigmas[k])
        acc = acc + ss_expneg(d2 / (2.0 * area * s2 * s2))
    oks = acc / float(len(common))
    e = (1.0 - oks) / 2.0
    return 1.0 if e > cfg.pose_thresh else e


class BotSortPoseRef(BotSortGmcRef):
    """BoT-SORT with the keypoint term (and optional GMC): BotSortGmcRef's frame procedure with
      - stage 4 (pool x high rows) and stage 6 (unconfirmed x leftover high rows) on min(fused 1 - IoU, OKS entry);
      - every track's pose: written at birth, replaced by every Kalman update of stages 4-6 (no smoothing, K-03); lost tracks
        keep theirs, a removed track forgets it.
    ByteTrackRef.update calls `assign` three times a frame (stages 4, 5, 6, empty matrices included); the cost of stages 4 and 6
    is replaced there, after checking that the one passed in is the fused IoU cost of the expected rows and columns."""

    def __init__(self, cfg: Optional[ByteTrackConfig] = None):
        cfg = cfg or ByteTrackConfig(kalman="xywh", with_pose=True)
        if not cfg.with_pose:
            raise ValueError("BotSortPoseRef needs cfg.with_pose")
        self.K = len(cfg.kpt_sigmas)
        super().__init__(cfg)

    def reset(self):
        super().reset()
        self.pose = {}                                # Track -> (offsets [K][2], visibility [K])

    def _update(self, t, d, reactivate=False):
        super()._update(t, d, reactivate)
        self.pose[t] = track_pose(self._z[d], self._kp[d], self._vis[d])

    def get_dists(self, rows, cols) -> np.ndarray:
        c = self.cfg
        tl, dl, sc = [t.tlwh for t in rows], [self._tl[i] for i in cols], [self._score[i] for i in cols]
        iou = _bt.iou_cost(tl, dl)
        mask = iou > c.proximity_thresh
        cost = _bt.fuse_score(iou, sc) if c.fuse_score else iou
        e = np.ones_like(iou)
        for r, k in zip(*np.nonzero(~mask)):
            t, d = rows[r], cols[k]
            e[r, k] = oks_entry(c, t.mean, self.pose[t][0], self.pose[t][1], self._kp[d], self._vis[d], self._tl[d])
        return iou, cost, np.minimum(cost, e)

    def _assign(self, cost, thresh):
        stage, self._stage = self._stage, self._stage + 1
        if stage == 1:                                # stage 5: plain IoU on the low rows
            return self._orig_assign(cost, thresh)
        rows, cols = (self._pool, self._high) if stage == 0 else (self._unconf, self._left)
        if len(rows) and len(cols):
            iou, fused, new = self.get_dists(rows, cols)
            assert np.array_equal(cost, fused, equal_nan=True)
            cost = new
        pairs, ur, uc = self._orig_assign(cost, thresh)
        if stage == 0:
            self._left = [self._high[k] for k in uc]
        return pairs, ur, uc

    def update(self, dets, kpts=None, warp=None) -> np.ndarray:
        c = self.cfg
        dets = np.asarray(dets, np.float32).reshape(-1, 6)
        n = min(dets.shape[0], c.max_dets)
        kp = np.zeros((dets.shape[0], self.K, 3), np.float32) if kpts is None else np.asarray(kpts, np.float32).reshape(-1, self.K, 3)
        self._kp = kp[:n]
        self._vis = visible(self._kp, c.kpt_vis_thresh)
        sc = dets[:n, 4].astype(np.float32)
        self._high = [i for i in range(n) if sc[i] >= np.float32(c.track_high_thresh)]
        self._pool = [t for t in self.tracked if t.activated] + list(self.lost)
        self._unconf = [t for t in self.tracked if not t.activated]
        self._left, self._stage = [], 0
        self._orig_assign = _bt.assign
        _bt.assign = self._assign
        try:
            rows = super().update(dets, warp)
        finally:
            _bt.assign = self._orig_assign
        assert self._stage == 3, "BotSortPoseRef: ByteTrackRef.update no longer calls assign once per stage"
        live = self.tracked + self.lost
        for t in live:
            if t not in self.pose:                    # a birth of this frame
                self.pose[t] = track_pose(self._z[t.det], self._kp[t.det], self._vis[t.det])
        self.pose = {t: self.pose[t] for t in live}
        return rows

    def keypoints(self):
        """The stored poses in tracks()' list order (tracked, then lost) — what ss_byte_get_keypoints returns:
        (offsets [n,K,2] float64, visibility words [n] uint32, bit k = keypoint k)."""
        ts = self.tracked + self.lost
        off = np.array([self.pose[t][0] for t in ts], np.float64).reshape(-1, self.K, 2)
        vis = np.array([sum(1 << k for k in range(self.K) if self.pose[t][1][k]) for t in ts], np.uint32)
        return off, vis
