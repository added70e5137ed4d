"""CPU restatement of GSI, Gaussian-smoothed interpolation (docs/GSI.md): the gap filling and the Gaussian-process smoothing of
StrongSORT++ on tracked rows, in the operation order the device kernel csrc/ss_gsi.hip is held to bit for bit.

Not a conftest and not a test module: imported by tests/test_gsi_cpu.py, tests/test_gpu_gsi.py and tests/golden/make_gsi_golden.py.

    rows = interpolate(rows, interval=20)                    # [N, 8] float64: frame, id, x1, y1, x2, y2, conf, cls
    rows, status = smooth(rows, tau=10.0, alpha=1e-10)       # status: {id: 0 smoothed | 1 pivot | 2 too long}
    rows, status = gsi(rows, interval=20, tau=10.0)

Every product, sum, quotient and square root below is one rounded float64 operation (numpy's element-wise ufuncs do not fuse),
as the device computes it with -ffp-contract=off.  `solve_track` is the schedule used (right-looking, whole columns at a time);
`solve_track_scalar` is docs/GSI.md §3 to the letter, one element at a time, and gives the same bits (tests/test_gsi_cpu.py).
"""
from __future__ import annotations

import math

import numpy as np

from tests.botsort_pose_ref import EXPNEG_C, EXPNEG_CUT, EXPNEG_LN2_HI, EXPNEG_LN2_LO, EXPNEG_LOG2E, ss_expneg

MAX_LEN = 1024                  # ss_gsi_max_len()
INTERVAL, TAU, ALPHA = 20, 10.0, 1e-10


# ---- rows ------------------------------------------------------------------------------------------------------------------
def _rows(rows) -> np.ndarray:
    r = np.array(rows, np.float64, copy=True).reshape(-1, 8)
    key = r[:, :2]
    if len(r) and len(np.unique(key, axis=0)) != len(r):
        raise ValueError("duplicate (frame, id)")
    return r


def _sorted(r: np.ndarray) -> np.ndarray:
    """Rows by (frame, id)."""
    return r[np.lexsort((r[:, 1], r[:, 0]))] if len(r) else r


def tracks_of(r: np.ndarray):
    """[(id, rows of that id in rising frame order)] by rising id."""
    out = []
    for tid in np.unique(r[:, 1]):
        t = r[r[:, 1] == tid]
        out.append((float(tid), t[np.argsort(t[:, 0], kind="stable")]))
    return out


# ---- §1 interpolation ------------------------------------------------------------------------------------------------------
def interpolate(rows, interval: int = INTERVAL) -> np.ndarray:
    r = _rows(rows)
    new = []
    for tid, t in tracks_of(r):
        for a, b in zip(t[:-1], t[1:]):
            gap = int(b[0]) - int(a[0])
            if not 1 < gap < interval:
                continue
            fg = float(gap)
            for j in range(1, gap):
                row = np.empty(8)
                row[0], row[1] = a[0] + j, tid
                for c in range(2, 6):
                    step = (b[c] - a[c]) / fg
                    row[c] = a[c] + step * float(j)
                row[6], row[7] = 0.0, a[7]
                new.append(row)
    if new:
        r = np.concatenate([r, np.array(new)], 0)
    return _sorted(r)


# ---- §2 length scale and kernel ----------------------------------------------------------------------------------------------
def length_scale(n: int, tau: float = TAU) -> float:
    tau = float(tau)
    t3 = tau * tau * tau
    return float(np.clip(tau * np.log(t3 / float(n)), 1.0 / tau, tau * tau))


def expneg_array(x: np.ndarray) -> np.ndarray:
    """ss_expneg (docs/BYTETRACK.md §1e) element-wise: the same operations on whole arrays."""
    x = np.asarray(x, np.float64)
    ok = x <= EXPNEG_CUT
    y = -np.where(ok, x, 0.0)
    k = np.floor(y * EXPNEG_LOG2E + 0.5)
    r = (y - k * EXPNEG_LN2_HI) - k * EXPNEG_LN2_LO
    p = np.full(x.shape, EXPNEG_C[12])
    for i in range(11, -1, -1):
        p = p * r + EXPNEG_C[i]
    return np.where(ok, np.ldexp(p, k.astype(np.int64)), 0.0)


def kernel_matrix(frames, l: float) -> np.ndarray:
    t = np.asarray(frames, np.float64)
    d = t[:, None] - t[None, :]
    den = (2.0 * l) * l
    return expneg_array((d * d) / den)


# ---- §3 the solve ----------------------------------------------------------------------------------------------------------
def solve_track(frames, vals, l: float, alpha: float = ALPHA):
    """vals [n, 4] -> (posterior mean [n, 4], status).  Right-looking: after column k is final, every element behind it takes
    its k-th subtraction, so each element sees the products of k = 0, 1, .. in rising order, rounded one by one."""
    y = np.array(vals, np.float64, copy=True).reshape(-1, 4)
    n = len(y)
    K = kernel_matrix(frames, l)
    A = K.copy()
    A[np.diag_indices(n)] = A[np.diag_indices(n)] + alpha
    z = y.copy()
    for k in range(n):
        s = A[k, k]
        if not s > 0.0:
            return y, 1
        d = math.sqrt(s)
        A[k, k] = d
        A[k + 1:, k] = A[k + 1:, k] / d
        z[k] = z[k] / d
        col = A[k + 1:, k]
        A[k + 1:, k + 1:] -= col[:, None] * col[None, :]
        z[k + 1:] -= col[:, None] * z[k][None, :]
    a = z
    for k in range(n - 1, -1, -1):
        a[k] = a[k] / A[k, k]
        a[:k] -= A[k, :k][:, None] * a[k][None, :]
    m = np.zeros((n, 4))
    for k in range(n):
        m += K[:, k][:, None] * a[k][None, :]
    return m, 0


def solve_track_scalar(frames, vals, l: float, alpha: float = ALPHA):
    """docs/GSI.md §3 one element at a time (left-looking); for short tracks."""
    y = np.array(vals, np.float64, copy=True).reshape(-1, 4)
    n = len(y)
    den = (2.0 * l) * l
    K = [[ss_expneg((float(frames[i] - frames[j]) * float(frames[i] - frames[j])) / den) for j in range(n)] for i in range(n)]
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        for i in range(j, n):
            s = K[i][j] + alpha if i == j else K[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            if i == j:
                if not s > 0.0:
                    return y, 1
                L[j][j] = math.sqrt(s)
            else:
                L[i][j] = s / L[j][j]
    m = np.zeros((n, 4))
    for c in range(4):
        z = [0.0] * n
        for i in range(n):
            s = float(y[i, c])
            for k in range(i):
                s = s - L[i][k] * z[k]
            z[i] = s / L[i][i]
        a = [0.0] * n
        for i in range(n - 1, -1, -1):
            s = z[i]
            for k in range(n - 1, i, -1):
                s = s - L[k][i] * a[k]
            a[i] = s / L[i][i]
        for i in range(n):
            acc = 0.0
            for k in range(n):
                acc = acc + K[i][k] * a[k]
            m[i, c] = acc
    return m, 0


# ---- §2 smoothing of rows ----------------------------------------------------------------------------------------------------
def tlwh(t: np.ndarray) -> np.ndarray:
    return np.stack([t[:, 2], t[:, 3], t[:, 4] - t[:, 2], t[:, 5] - t[:, 3]], 1)


def put_tlwh(t: np.ndarray, m: np.ndarray) -> np.ndarray:
    t = t.copy()
    t[:, 2], t[:, 3] = m[:, 0], m[:, 1]
    t[:, 4], t[:, 5] = m[:, 0] + m[:, 2], m[:, 1] + m[:, 3]
    return t


def smooth(rows, tau: float = TAU, alpha: float = ALPHA):
    r = _rows(rows)
    out, status = [], {}
    for tid, t in tracks_of(r):
        n = len(t)
        if n > MAX_LEN:
            out.append(t)
            status[int(tid)] = 2
            continue
        m, st = solve_track(t[:, 0].astype(np.int64), tlwh(t), length_scale(n, tau), alpha)
        status[int(tid)] = st
        out.append(put_tlwh(t, m) if st == 0 else t)
    return _sorted(np.concatenate(out, 0) if out else r), status


def gsi(rows, interval: int = INTERVAL, tau: float = TAU, alpha: float = ALPHA):
    return smooth(interpolate(rows, interval), tau, alpha)


def label_lines(rows) -> str:
    """LabelsWriter's line format (strongsort_yolo_amd/cli.py): `frame cls id conf x1 y1 x2 y2 -1 -1 -1 -1` per row."""
    out = []
    for r in np.asarray(rows, np.float64).reshape(-1, 8):
        out.append(f"{int(r[0])} {int(r[7])} {int(r[1])} {round(float(r[6]), 3)} {int(r[2])} {int(r[3])} {int(r[4])} {int(r[5])} -1 -1 -1 -1\n")
    return "".join(out)


# ---- seeded tracks for the tests, the golden file and tools/gsi_time.py ----------------------------------------------------------
def trajectory(frames) -> np.ndarray:
    """A known path, [n, 4] corners: a box that drifts across a 1920 x 1080 frame on a slow curve while it grows."""
    t = np.asarray(frames, np.float64)
    cx = 300.0 + 1200.0 * (0.5 - 0.5 * np.cos(t / 700.0)) + 40.0 * np.sin(t / 45.0)
    cy = 500.0 + 300.0 * np.sin(t / 400.0) + 25.0 * np.cos(t / 60.0)
    w = 80.0 + 30.0 * np.sin(t / 300.0)
    h = 200.0 + 60.0 * np.sin(t / 350.0)
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)


def make_frames(rng, n: int, gaps: bool, start: int = 0) -> np.ndarray:
    """n rising frame numbers; gaps=True: a jump of 20 .. 60 frames after about every 25th row (at least one when n >= 2)."""
    step = np.ones(n, np.int64)
    if gaps and n >= 2:
        at = rng.choice(np.arange(1, n), size=max(1, n // 25), replace=False)
        step[at] = rng.integers(20, 61, len(at))
    step[0] = start
    return np.cumsum(step)


def make_track(rng, n: int, gaps: bool = False, tid: int = 1, sigma: float = 2.0, start: int = 0) -> np.ndarray:
    """Rows of one track: the trajectory plus N(0, sigma) px on every corner."""
    f = make_frames(rng, n, gaps, start)
    r = np.zeros((n, 8))
    r[:, 0], r[:, 1] = f, tid
    r[:, 2:6] = trajectory(f) + rng.normal(0.0, sigma, (n, 4))
    r[:, 6], r[:, 7] = np.round(rng.uniform(0.3, 0.95, n), 3), 0.0
    return r
