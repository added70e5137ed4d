"""CPU reference of BoT-SORT's ReID branch (docs/BYTETRACK.md §1c, decisions R-01..): the appearance term of the first and
third associations and the tracks' smoothed features, on top of tests/bytetrack_ref.py and tests/botsort_gmc_ref.py.

Not a conftest and not a test module: imported by tests/test_botsort_reid_cpu.py and tests/test_gpu_botsort_reid.py.

    ref = BotSortReidRef()                       # ByteTrackConfig(kalman="xywh", with_reid=True) by default
    rows = ref.update(dets, feats, warp=None)    # feats [N,512] raw features of the rows; warp as BotSortGmcRef.update

The feature arithmetic goes through the exact-order oracle (oracle.cexact: so_normalize, so_ema, so_cosine_min), which the
device reproduces bit for bit; the IoU, fusion and threshold steps are float64 NumPy as in ByteTrackRef.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from oracle import cexact
from strongsort_yolo_amd.config import ByteTrackConfig
import tests.bytetrack_ref as _bt
from tests.botsort_gmc_ref import BotSortGmcRef

FEAT = 512


def appearance(smooth, curr) -> float:
    """§1c step 4 before the threshold: (double) max(0, 1 - so_dot(smooth, curr)) / 2 in float32, halved in float64."""
    d = cexact.cosine_min(np.asarray(smooth, np.float32)[None], np.asarray(curr, np.float32)[None])[0]
    return float(np.maximum(np.float32(0.0), d)) / 2.0


def get_dists(cfg: ByteTrackConfig, tracks_tlwh, dets_tlwh, scores, smooth, curr) -> np.ndarray:
    """§1c get_dists on tracks x rows: min(fused 1 - IoU, appearance entry); the appearance entry is 1 where 1 - IoU >
    proximity_thresh or where the halved cosine distance exceeds appearance_thresh.  smooth [T,512], curr [D,512] unit rows."""
    iou = _bt.iou_cost(tracks_tlwh, dets_tlwh)
    mask = iou > cfg.proximity_thresh
    c = _bt.fuse_score(iou, scores) if cfg.fuse_score else iou
    emb = np.ones_like(iou)
    for r, k in zip(*np.nonzero(~mask)):            # a masked entry needs no dot product
        e = appearance(smooth[r], curr[k])
        emb[r, k] = 1.0 if e > cfg.appearance_thresh else e
    return np.minimum(c, emb)


class BotSortReidRef(BotSortGmcRef):
    """BoT-SORT with ReID (and optional GMC): BotSortGmcRef's frame procedure with
      - stage 4 (pool x high rows) and stage 6 (unconfirmed x leftover high rows) on get_dists instead of the fused IoU cost;
      - every track's smoothed unit feature: a birth copies its row's unit feature, every Kalman update of stages 4-6 takes
        so_ema(smooth, curr, alpha, 1 - alpha); lost tracks keep theirs, a removed track forgets it.
    ByteTrackRef.update calls `assign` three times a frame (stages 4, 5, 6, empty matrices included); the cost of stages 4 and 6
    is replaced there, after checking that the one passed in is the fused IoU cost of the expected rows and columns."""

    def __init__(self, cfg: Optional[ByteTrackConfig] = None):
        cfg = cfg or ByteTrackConfig(kalman="xywh", with_reid=True)
        if not cfg.with_reid:
            raise ValueError("BotSortReidRef needs cfg.with_reid")
        super().__init__(cfg)

    def reset(self):
        super().reset()
        self.feat = {}                                # Track -> smoothed unit feature [512] f32

    def _update(self, t, d, reactivate=False):
        super()._update(t, d, reactivate)
        self.feat[t] = cexact.ema(self.feat[t], self._curr[d], self.cfg.feat_alpha)

    def _assign(self, cost, thresh):
        stage, self._stage = self._stage, self._stage + 1
        if stage == 1:                                # stage 5: plain IoU on the low rows
            return self._orig_assign(cost, thresh)
        if stage == 0:
            rows, cols = self._pool, self._high
        else:
            rows, cols = self._unconf, self._left
        if len(rows) and len(cols):
            tl, dl, sc = [t.tlwh for t in rows], [self._tl[i] for i in cols], [self._score[i] for i in cols]
            iou = _bt.iou_cost(tl, dl)
            assert np.array_equal(cost, _bt.fuse_score(iou, sc) if self.cfg.fuse_score else iou, equal_nan=True)
            cost = get_dists(self.cfg, tl, dl, sc, [self.feat[t] for t in rows], [self._curr[i] for i in cols])
        pairs, ur, uc = self._orig_assign(cost, thresh)
        if stage == 0:
            self._left = [self._high[k] for k in uc]
        return pairs, ur, uc

    def update(self, dets, feats=None, warp=None) -> np.ndarray:
        c = self.cfg
        dets = np.asarray(dets, np.float32).reshape(-1, 6)
        n = min(dets.shape[0], c.max_dets)
        raw = np.zeros((dets.shape[0], FEAT), np.float32) if feats is None else np.asarray(feats, np.float32).reshape(-1, FEAT)
        self._curr = [cexact.normalize(raw[i]) for i in range(n)]
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
        assert self._stage == 3, "BotSortReidRef: ByteTrackRef.update no longer calls assign once per stage"
        live = self.tracked + self.lost
        for t in live:
            if t not in self.feat:                    # a birth of this frame
                self.feat[t] = self._curr[t.det].copy()
        self.feat = {t: self.feat[t] for t in live}
        return rows

    def features(self) -> np.ndarray:
        """The smoothed features in tracks()' list order (tracked, then lost) — what ss_byte_get_features returns."""
        return np.array([self.feat[t] for t in self.tracked + self.lost], np.float32).reshape(-1, FEAT)
