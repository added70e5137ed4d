"""Inputs and group bookkeeping for the ECC camera-motion tests (csrc/ss_cmc.hip against oracle.cexact; no GPU needed here).

    sc = scene(H, W, seed)                    # a BGR canvas with a margin of MARGIN pixels around the H x W view
    fr = warped(sc, theta, tx, ty)            # the view after the camera turned by theta about the image origin and moved by (tx, ty)
    ref = EccRef(S); ref.estimate(frames)     # what ss_cmc_estimate returns for a call, with its remembered frames

The estimator's warp maps the previous frame's coordinates to the current frame's: cur(R p + t) = prev(p).  So the frame after a
motion (theta, tx, ty) shows at q what the still view shows at R^T (q - t), which is what warped() samples.
"""
import numpy as np

from oracle import cexact
from tests.test_oracle_cmc import _texture

MARGIN = 100
IDENTITY = np.array([1.0, 0, 0, 0, 1.0, 0, -1.0, 0])

# the motions of the rotation tests: theta [rad], shift in SMALL-image pixels, gain, bias
MOTIONS = [(0.03, 1.5, -1.0, 1.0, 0.0), (-0.05, 0.0, 0.0, 1.0, 0.0), (0.02, 2.0, 1.0, 0.7, 20.0)]


def small_hw(H, W):
    return int(H * 0.1), int(W * 0.1)


def scene(h, w, seed):
    """BGR uint8 [h + 2 MARGIN, w + 2 MARGIN, 3]: the texture of test_oracle_cmc ten times enlarged (structure at the scale the
    0.1x grey images keep) plus pixel noise, as test_gpu_cmc._scene makes it."""
    from scipy.ndimage import zoom
    hh, ww = h + 2 * MARGIN, w + 2 * MARGIN
    small = np.stack([_texture(hh // 10 + 1, ww // 10 + 1, seed + c) for c in range(3)], axis=2)
    t = zoom(small, (10, 10, 1), order=1)[:hh, :ww]
    t = t + np.random.default_rng(seed).normal(0, 3, t.shape)
    return np.clip(t, 0, 255).astype(np.uint8)


def warped(sc, theta, tx, ty, gain=1.0, bias=0.0):
    """BGR uint8 [H, W, 3]: the scene's view after a rotation by theta about the image origin and a shift (tx, ty), full-frame
    pixels; v * gain + bias, clipped.  warped(sc, 0, 0, 0) is the still view sc[MARGIN:-MARGIN, MARGIN:-MARGIN]."""
    from scipy.ndimage import affine_transform
    H, W = sc.shape[0] - 2 * MARGIN, sc.shape[1] - 2 * MARGIN
    c, s = np.cos(theta), np.sin(theta)
    # (row, col) of the source for output (row, col): R^T (q - t) + MARGIN
    m = np.array([[c, -s], [s, c]])
    off = np.array([MARGIN - c * ty + s * tx, MARGIN - s * ty - c * tx])
    out = np.stack([affine_transform(sc[..., k].astype(np.float64), m, offset=off, output_shape=(H, W), order=1, mode="nearest")
                    for k in range(3)], axis=2)
    return np.clip(np.floor(out * gain + bias + 0.5), 0, 255).astype(np.uint8)


def small_motion(theta, tx, ty, sx=10.0, sy=10.0):
    """(theta, tx, ty) of the small images for a full-frame motion: small pixel x sits at full-frame sx * (x + 0.5) - 0.5, so the
    rotation about the full-frame origin is one about (0.5 / sx - 0.5, 0.5 / sy - 0.5) of the small image.  Exact for sx == sy."""
    c, s = np.cos(theta), np.sin(theta)
    ox, oy = 0.5 * sx - 0.5, 0.5 * sy - 0.5
    return theta, ((c - 1) * ox - s * oy + tx) / sx, (s * ox + (c - 1) * oy + ty) / sy


def blocks(small):
    """BGR uint8 [10 hs, 10 ws, 3] whose 0.1x grey image is `small` exactly: every value fills a 10 x 10 block of three equal
    channels; the down-scale reads inside one block (10 x + 4.5) and the grey of (v, v, v) is v."""
    b = np.kron(np.asarray(small, np.uint8), np.ones((10, 10), np.uint8))
    return np.ascontiguousarray(np.stack([b, b, b], axis=2))


def pair_warp(prev_small, cur_small, H, W):
    """The 8 numbers ss_cmc_estimate stores for one pair of small images of H x W frames."""
    hs, ws = cur_small.shape
    w, it = cexact.ecc(prev_small, cur_small)
    if it < 0:
        return IDENTITY.copy()
    out = np.zeros(8)
    w = w.copy(); w[0, 2] *= W / ws; w[1, 2] *= H / hs
    out[:6], out[6] = w.reshape(6), it
    return out


class EccRef:
    """ss_cmc_estimate's contract on the oracle: per stream the remembered small image (`prev[s]`, None: no predecessor) and the
    small images of the last call (`smalls[f][s]`)."""

    def __init__(self, S):
        self.S, self.hw = S, None
        self.prev = [None] * S
        self.smalls = []

    def reset(self, stream=-1):
        for s in (range(self.S) if stream < 0 else [stream]):
            self.prev[s] = None

    def estimate(self, frames, n_valid=None):
        F, S, H, W = frames.shape[:4]
        assert S == self.S and frames.shape[4] == 3
        if self.hw != (H, W):                                  # a new frame size: new buffers, every predecessor forgotten
            self.hw, self.prev = (H, W), [None] * S
        hs, ws = small_hw(H, W)
        n = F if n_valid is None else min(int(n_valid), F)
        out = np.tile(IDENTITY, (F, S, 1))
        self.smalls = [[cexact.gray_small(frames[f, s], hs, ws) for s in range(S)] for f in range(F)]
        for f in range(n):                                     # frames at or past n are stale: -1, and not remembered
            for s in range(S):
                cur = self.smalls[f][s]
                if self.prev[s] is not None:
                    out[f, s] = pair_warp(self.prev[s], cur, H, W)
                self.prev[s] = cur
        return out
