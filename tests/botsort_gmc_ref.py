"""CPU reference of BoT-SORT's camera-motion step (docs/BYTETRACK.md §1b, decisions G-01..G-06): a float64 restatement of
Ultralytics' `STrack.multi_gmc` in the operation order of csrc/ss_byte.hip (`byte_gmc`), plugged into tests/bytetrack_ref.py.

Not a conftest and not a test module: imported by tests/test_botsort_gmc_cpu.py and tests/test_gpu_botsort_gmc.py.

    ref = BotSortGmcRef()                    # ByteTrackConfig(kalman="xywh") by default
    rows = ref.update(dets, warp)            # warp: 8 floats as ss_cmc_estimate writes them, or None (no warp)

Every product and sum below is one rounded float64 operation (no fma), as the device computes it with -ffp-contract=off.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from strongsort_yolo_amd.config import ByteTrackConfig
from tests.bytetrack_ref import ByteTrackRef, mean_tlwh


def gmc_apply(mean, cov, w):
    """Step 3b on one track: mean <- R8 mean + (t, 0, ...), cov <- R8 cov R8^T with R8 = kron(I4, R), R = [[w0, w1], [w3, w4]],
    t = (w2, w5); written as 2x2 blocks (G-02).  -> (new mean [8], new cov [64]) as lists of floats."""
    r00, r01, r10, r11 = float(w[0]), float(w[1]), float(w[3]), float(w[4])
    m = [float(v) for v in mean]
    for k in range(4):
        u, v = m[2 * k], m[2 * k + 1]
        m[2 * k] = r00 * u + r01 * v
        m[2 * k + 1] = r10 * u + r11 * v
    m[0] = m[0] + float(w[2])
    m[1] = m[1] + float(w[5])
    P = [float(v) for v in cov]
    for i in range(4):                           # X = R8 P: for row 2i+r, R[r][0] * P[2i][c] + R[r][1] * P[2i+1][c]
        for c in range(8):
            a, e = P[(2 * i) * 8 + c], P[(2 * i + 1) * 8 + c]
            P[(2 * i) * 8 + c] = r00 * a + r01 * e
            P[(2 * i + 1) * 8 + c] = r10 * a + r11 * e
    for r in range(8):                           # P' = X R8^T: for column 2j+q, X[r][2j] * R[q][0] + X[r][2j+1] * R[q][1]
        for j in range(4):
            a, e = P[r * 8 + 2 * j], P[r * 8 + 2 * j + 1]
            P[r * 8 + 2 * j] = a * r00 + e * r01
            P[r * 8 + 2 * j + 1] = a * r10 + e * r11
    return m, P


class BotSortGmcRef(ByteTrackRef):
    """BoT-SORT with GMC: ByteTrackRef's frame procedure (§1, xywh) with step 3b between the pool's prediction and the first
    association.  The unconfirmed tracks are not predicted and nothing reads them before step 6, so they are moved first;
    the pool tracks are moved as ByteTrackRef.update stores each predicted mean (its first `_set_mean` calls of a frame,
    one per pool track, in pool order)."""

    def __init__(self, cfg: Optional[ByteTrackConfig] = None):
        cfg = cfg or ByteTrackConfig(kalman="xywh")
        if cfg.kalman != "xywh":
            raise ValueError("BoT-SORT's GMC needs the xywh filter (G-05)")
        self._gmc_w, self._gmc_left = None, 0
        super().__init__(cfg)

    def _set_mean(self, t, mean, cov):
        if self._gmc_left > 0:                   # step 3: this is a pool track's predicted state
            self._gmc_left -= 1
            mean, cov = gmc_apply(mean, cov, self._gmc_w)
        super()._set_mean(t, mean, cov)

    def update(self, dets, warp=None) -> np.ndarray:
        w = None if warp is None else [float(v) for v in np.asarray(warp, np.float64).reshape(-1)[:8]]
        if w is not None and w[6] < 0:           # G-03: no warp (first frame, failed alignment, padding frame) skips 3b
            w = None
        if w is not None:
            for t in self.tracked:
                if not t.activated:              # unconfirmed: moved, not predicted
                    t.mean, t.cov = gmc_apply(t.mean, t.cov, w)
                    t.tlwh = mean_tlwh(t.mean, True)
            self._gmc_w = w
            self._gmc_left = sum(1 for t in self.tracked if t.activated) + len(self.lost)
        try:
            return super().update(dets)
        finally:
            left, self._gmc_left, self._gmc_w = self._gmc_left, 0, None
            assert left == 0, "BotSortGmcRef: the pool's prediction no longer comes first in ByteTrackRef.update"
