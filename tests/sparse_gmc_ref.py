"""CPU reference of the sparse-optical-flow camera-motion estimator (docs/BYTETRACK.md §1f, decisions S-01..): this project's
restatement of Ultralytics' `gmc_method: sparseOptFlow` (Shi-Tomasi corners on a half-size grey frame, pyramidal Lucas-Kanade
from the previous frame, a RANSAC similarity fit) in the operation order of csrc/ss_gmc.hip, vectorised over points.

Not a conftest and not a test module: imported by tests/test_sparse_gmc_cpu.py and tests/test_gpu_sparse_gmc.py.

    ref = SparseGmcRef(n_streams)
    warps = ref.estimate(frames)             # frames [F,S,H,W,3] BGR u8 -> [F,S,8] float64, ss_gmc_sparse_estimate's layout
    ref.last[(f, s)]                         # the stages of that pair (what ss_gmc_sparse_get returns)

Integer stages are exact.  Every float32 / float64 product, sum, quotient and square root below is one rounded operation (no
fma), as the device computes it with -ffp-contract=off; the sums over a window or over the matches run in the device's order.
"""
from __future__ import annotations

import numpy as np

MAX_CORNERS = 1000          # S-04
QUALITY = np.float32(0.01)
LEVELS = 4                  # pyramid levels 0..3 (S-03)
WIN, HALF_WIN = 21, 10      # S-06
WIN_N = WIN * WIN
MAX_ITER = 30
STEP2 = 1e-4                # 0.01^2
MIN_EIG = 1e-4
MIN_DET = 1.1920928955078125e-07
N_HYP = 1024                # S-09
INLIER2 = 9.0
MIN_MATCHES = 5
MIN_SIDE = 64               # smallest frame side ss_gmc_sparse_estimate accepts
_LANE = np.arange(64)


def grey(bgr):
    """cm_grey of csrc/ss_cmc.hip: integer BGR -> grey."""
    p = bgr.astype(np.int32)
    return ((p[..., 0] * 1868 + p[..., 1] * 9617 + p[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def half(g):
    """S-02: 2x2 mean with rounding; an odd last row or column is dropped."""
    hh, wh = g.shape[0] // 2, g.shape[1] // 2
    g = g[:2 * hh, :2 * wh].astype(np.int32)
    return ((g[0::2, 0::2] + g[0::2, 1::2] + g[1::2, 0::2] + g[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def pyr_down(a):
    """S-03: [1 4 6 4 1] x [1 4 6 4 1] / 256 with rounding at the even pixels, reflect-101 border, size (n + 1) // 2."""
    h, w = a.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    p = np.pad(a.astype(np.int32), 2, mode="reflect")
    k = (1, 4, 6, 4, 1)
    t = sum(k[j] * p[:, j:j + 2 * ow - 1:2] for j in range(5))
    o = sum(k[i] * t[i:i + 2 * oh - 1:2, :] for i in range(5))
    return ((o + 128) >> 8).astype(np.uint8)


def pyramid(bgr):
    lv = [half(grey(bgr))]
    for _ in range(LEVELS - 1):
        lv.append(pyr_down(lv[-1]))
    return lv


def min_eig_map(l0):
    """S-04: the smaller eigenvalue (float32, one stated formula) of the 3x3 box sums of the integer 3x3 Sobel products; the
    image is extended by two pixels (reflect-101), so every pixel has nine gradients."""
    p = np.pad(l0.astype(np.int32), 2, mode="reflect")
    gx = (p[:-2, 2:] - p[:-2, :-2]) + 2 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])
    gy = (p[2:, :-2] - p[:-2, :-2]) + 2 * (p[2:, 1:-1] - p[:-2, 1:-1]) + (p[2:, 2:] - p[:-2, 2:])
    h, w = l0.shape

    def box(a):
        return sum(a[i:i + h, j:j + w] for i in range(3) for j in range(3))
    sxx, sxy, syy = box(gx * gx), box(gx * gy), box(gy * gy)
    a = sxx.astype(np.float32) * np.float32(0.5)
    c = syy.astype(np.float32) * np.float32(0.5)
    b = sxy.astype(np.float32)
    d = a - c
    return (a + c) - np.sqrt(d * d + b * b)


def corners(l0):
    """S-04/S-05 -> (points [n,2] int32 (x, y), number of candidates before the cut to MAX_CORNERS)."""
    lam = min_eig_map(l0)
    mx = lam.max()
    if not mx > 0:
        return np.zeros((0, 2), np.int32), 0
    thr = QUALITY * mx
    h, w = lam.shape
    p = np.pad(lam, 1, constant_values=-np.inf)
    nb = np.max([p[i:i + h, j:j + w] for i in range(3) for j in range(3)], axis=0)
    idx = np.flatnonzero((lam > 0) & (lam >= thr) & (lam == nb))
    v = lam.ravel()[idx]
    order = np.lexsort((idx, -v))[:MAX_CORNERS]
    sel = idx[order]
    return np.stack([sel % w, sel // w], axis=1).astype(np.int32), len(idx)


def _wave_sum(v):
    """[n, 448] -> [n]: lane l adds its elements l, l + 64, ... in order from 0.0, then the xor butterfly 32, 16, .., 1."""
    a = v.reshape(len(v), 7, 64)
    acc = np.zeros((len(v), 64))
    for k in range(7):
        acc = acc + a[:, k, :]
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, _LANE ^ off]
    return acc[:, 0]


_PAD = 13
_E = np.arange(7 * 64)
_EI, _EJ, _EV = _E // WIN, _E % WIN, _E < WIN_N


def _bilerp(v00, v01, v10, v11, fx, fy):
    a = v00 + fx * (v01 - v00)
    b = v10 + fx * (v11 - v10)
    return a + fy * (b - a)


def _window(cx, cy, stride):
    """Window around the centres (cx, cy) [n] in an image replicate-padded by _PAD with `stride` columns -> (flat indices
    [n, 448] of each element's upper-left pixel, fx [n,1], fy [n,1])."""
    bx, by = cx - float(HALF_WIN), cy - float(HALF_WIN)
    ix, iy = np.floor(bx), np.floor(by)
    x = ix.astype(np.int64)[:, None] + (_EJ[None, :] + _PAD)
    y = iy.astype(np.int64)[:, None] + (_EI[None, :] + _PAD)
    return y * stride + x, (bx - ix)[:, None], (by - iy)[:, None]


def _sample(img, win):
    """img: the padded image, float64 -> the bilinear window values [n, 448], zero past the window's 441 elements."""
    idx, fx, fy = win
    f, stride = img.reshape(-1), img.shape[1]
    v = _bilerp(f.take(idx), f.take(idx + 1), f.take(idx + stride), f.take(idx + stride + 1), fx, fy)
    v[:, WIN_N:] = 0.0
    return v


def lk(prev_pyr, cur_pyr, pts):
    """S-06..S-08: pts [n,2] int (level-0 pixels of the previous image) -> (tracked [n,2] float64, status [n] u8)."""
    n = len(pts)
    status = np.ones(n, bool)
    nx, ny = np.zeros(n), np.zeros(n)
    h0, w0 = prev_pyr[0].shape
    for L in range(LEVELS - 1, -1, -1):
        I = np.pad(prev_pyr[L].astype(np.int64), _PAD, mode="edge")
        J = np.pad(cur_pyr[L].astype(np.float64), _PAD, mode="edge")
        xmax, ymax = (w0 - 1) * 0.5 ** L, (h0 - 1) * 0.5 ** L          # S-08: level 0's frame at this level's scale
        # integer Scharr of the replicate-extended previous level, scaled by 1/32 (exact)
        dxi = np.zeros_like(I)
        dyi = np.zeros_like(I)
        dxi[1:-1, 1:-1] = 3 * (I[:-2, 2:] - I[:-2, :-2]) + 10 * (I[1:-1, 2:] - I[1:-1, :-2]) + 3 * (I[2:, 2:] - I[2:, :-2])
        dyi[1:-1, 1:-1] = 3 * (I[2:, :-2] - I[:-2, :-2]) + 10 * (I[2:, 1:-1] - I[:-2, 1:-1]) + 3 * (I[2:, 2:] - I[:-2, 2:])
        If, Dxf, Dyf = I.astype(np.float64), dxi.astype(np.float64) * 0.03125, dyi.astype(np.float64) * 0.03125
        scale = 0.5 ** L
        px, py = pts[:, 0] * scale, pts[:, 1] * scale
        if L == LEVELS - 1:
            nx, ny = px.copy(), py.copy()
        else:
            nx, ny = nx * 2.0, ny * 2.0
        act = np.flatnonzero(status)
        if len(act) == 0:
            continue
        win = _window(px[act], py[act], If.shape[1])
        Iw, Dx, Dy = _sample(If, win), _sample(Dxf, win), _sample(Dyf, win)
        A11, A12, A22 = _wave_sum(Dx * Dx), _wave_sum(Dx * Dy), _wave_sum(Dy * Dy)
        dA = A11 - A22
        min_eig = ((A22 + A11) - np.sqrt(dA * dA + 4.0 * A12 * A12)) / 882.0
        D = A11 * A22 - A12 * A12
        ok = (min_eig >= MIN_EIG) & (D >= MIN_DET)
        if L == 0:
            status[act[~ok]] = False             # S-07: a window without texture fails the point at level 0 only
        sub = np.flatnonzero(ok)                 # rows of act still iterating
        for _ in range(MAX_ITER):
            if len(sub) == 0:
                break
            g = act[sub]
            inside = (nx[g] >= 0.0) & (nx[g] <= xmax) & (ny[g] >= 0.0) & (ny[g] <= ymax)
            status[g[~inside]] = False           # S-08: left the frame -> lost
            sub, g = sub[inside], g[inside]
            if len(sub) == 0:
                break
            diff = _sample(J, _window(nx[g], ny[g], J.shape[1])) - Iw[sub]
            b1, b2 = _wave_sum(diff * Dx[sub]), _wave_sum(diff * Dy[sub])
            ddx = (A12[sub] * b2 - A22[sub] * b1) / D[sub]
            ddy = (A12[sub] * b1 - A11[sub] * b2) / D[sub]
            nx[g] = nx[g] + ddx
            ny[g] = ny[g] + ddy
            sub = sub[~(ddx * ddx + ddy * ddy < STEP2)]
        g = np.flatnonzero(status)
        inside = (nx[g] >= 0.0) & (nx[g] <= xmax) & (ny[g] >= 0.0) & (ny[g] <= ymax)
        status[g[~inside]] = False               # the level's final position
    out = np.stack([nx, ny], axis=1)
    out[~status] = 0.0
    return out, status.astype(np.uint8)


def _mix32(u):
    """S-09: the counter-based generator (murmur3's 32-bit finaliser over counter * 0x9E3779B9 + 0x7F4A7C15)."""
    m = np.uint64(0xFFFFFFFF)
    u = (u.astype(np.uint64) * np.uint64(0x9E3779B9) + np.uint64(0x7F4A7C15)) & m
    u ^= u >> np.uint64(16)
    u = (u * np.uint64(0x85EBCA6B)) & m
    u ^= u >> np.uint64(13)
    u = (u * np.uint64(0xC2B2AE35)) & m
    u ^= u >> np.uint64(16)
    return u


def _block_sum(v):
    """[1024] -> scalar: 16 waves of 64 lanes, xor butterfly per wave, then the 16 wave sums added left to right."""
    a = v.reshape(16, 64)
    for off in (32, 16, 8, 4, 2, 1):
        a = a + a[:, _LANE ^ off]
    tot = a[0, 0]
    for g in range(1, 16):
        tot = tot + a[g, 0]
    return tot


def fit(src, dst, status):
    """S-09..S-11: src [n,2] int, dst [n,2] float64, status [n] -> (warp [8], inlier mask [n] u8); half-size pixels inside,
    translation doubled on the way out."""
    none = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0, 0.0])
    mask = np.zeros(len(src), np.uint8)
    m = np.flatnonzero(status)
    M = len(m)
    none[7] = M
    if M < MIN_MATCHES:
        return none, mask
    x, y = src[m, 0].astype(np.float64), src[m, 1].astype(np.float64)
    u, v = dst[m, 0], dst[m, 1]
    k = np.arange(N_HYP, dtype=np.uint64)
    i1 = ((_mix32(k * np.uint64(2)) * np.uint64(M)) >> np.uint64(32)).astype(np.int64)
    i2 = ((_mix32(k * np.uint64(2) + np.uint64(1)) * np.uint64(M - 1)) >> np.uint64(32)).astype(np.int64)
    i2 = i2 + (i2 >= i1)
    dx, dy, ex, ey = x[i2] - x[i1], y[i2] - y[i1], u[i2] - u[i1], v[i2] - v[i1]
    den = dx * dx + dy * dy
    good = den > 0.0
    den = np.where(good, den, 1.0)
    a = (dx * ex + dy * ey) / den
    b = (dx * ey - dy * ex) / den
    tx = u[i1] - (a * x[i1] - b * y[i1])
    ty = v[i1] - (b * x[i1] + a * y[i1])

    def inliers(a, b, tx, ty):
        rx = ((a * x - b * y) + tx) - u
        ry = ((b * x + a * y) + ty) - v
        return rx * rx + ry * ry <= INLIER2
    cnt = inliers(a[:, None], b[:, None], tx[:, None], ty[:, None]).sum(axis=1)
    cnt = np.where(good, cnt, 0)
    best = int(np.argmax(cnt))                   # most inliers, lowest index on a tie
    if cnt[best] < 2:
        return none, mask
    inl = inliers(a[best], b[best], tx[best], ty[best])
    n_in = float(inl.sum())

    def bsum(t):
        p = np.zeros(1024)
        p[:M] = np.where(inl, t, 0.0)
        return _block_sum(p)
    mx, my, mu, mv = bsum(x) / n_in, bsum(y) / n_in, bsum(u) / n_in, bsum(v) / n_in
    xc, yc, uc, vc = x - mx, y - my, u - mu, v - mv
    sxx = bsum(xc * xc + yc * yc)
    sa = bsum(xc * uc + yc * vc)
    sb = bsum(xc * vc - yc * uc)
    if not sxx > 0.0:
        return none, mask
    ra, rb = sa / sxx, sb / sxx
    rtx = mu - (ra * mx - rb * my)
    rty = mv - (rb * mx + ra * my)
    mask[m[inl]] = 1
    return np.array([ra, -rb, 2.0 * rtx, rb, ra, 2.0 * rty, n_in, float(M)]), mask


def estimate_pair(prev_bgr, cur_bgr):
    """One pair without state -> (warp [8], stages dict)."""
    r = SparseGmcRef(1)
    r.estimate(prev_bgr[None, None])
    w = r.estimate(cur_bgr[None, None])
    return w[0, 0], r.last[(0, 0)]


class SparseGmcRef:
    """The estimator with ss_gmc_sparse_estimate's memory: per stream the last real frame's pyramid and corner list."""

    def __init__(self, n_streams=1):
        self.S = n_streams
        self.prev = [None] * n_streams           # (pyramid, corners, n_candidates)
        self.last = {}

    def reset(self, stream=-1):
        for s in range(self.S) if stream < 0 else [stream]:
            self.prev[s] = None

    def estimate(self, frames, n_valid=None):
        F, S = frames.shape[:2]
        assert S == self.S and min(frames.shape[2:4]) >= MIN_SIDE
        n_valid = F if n_valid is None else min(int(n_valid), F)
        out = np.zeros((F, S, 8))
        out[..., 0] = out[..., 4] = 1.0
        out[..., 6] = -1.0
        self.last = {}
        for s in range(S):
            for f in range(F):
                if f >= n_valid:
                    continue
                pyr = pyramid(frames[f, s])
                c, n_cand = corners(pyr[0])
                cur = (pyr, c, n_cand)
                p = self.prev[s]
                if p is not None:
                    rec = dict(pyramid=pyr, corners=p[1], n_candidates=p[2])
                    if len(p[1]) and len(c):     # S-12: a pair with a cornerless image has no warp
                        pts, st = lk(p[0], pyr, p[1])
                        out[f, s], rec["inliers"] = fit(p[1], pts, st)
                        rec["points"], rec["status"] = pts, st
                    else:
                        n = len(p[1])
                        rec["points"], rec["status"], rec["inliers"] = np.zeros((n, 2)), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
                    self.last[(f, s)] = rec
                self.prev[s] = cur
        return out
