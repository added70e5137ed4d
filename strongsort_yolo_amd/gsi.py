"""GSI, Gaussian-smoothed interpolation: the weight-free half of StrongSORT++'s post-processing (docs/GSI.md).

Rows are a float64 array [N, 8]: frame, id, x1, y1, x2, y2, conf, cls (frame and id are integers held in float64).  A track is the
set of rows of one id in rising frame order.  `interpolate` fills short gaps on the host; `smooth` replaces x1, y1, w, h of every
track by the posterior mean of a Gaussian process over the frame number, on the device (csrc/ss_gsi.hip, one workgroup per track).
There is no CPU fallback: without the library or a device `smooth` raises as the rest of the package does.  tests/gsi_ref.py restates
both steps; the device's results equal it bit for bit.

AFLink, the other half of StrongSORT++, is strongsort_yolo_amd.aflink (docs/AFLINK.md).
"""
from __future__ import annotations

import numpy as np

from . import lib as _lib

INTERVAL, TAU, ALPHA = 20, 10.0, 1e-10
MAX_LEN = 1024      # ss_gsi_max_len(): longer tracks pass through with status 2 (docs/GSI.md G-07)
# the kernel's path boundaries (csrc/ss_gsi.hip): tracks up to LDS_MAX rows keep their triangle in LDS, longer ones in device memory;
# both factorise PANEL columns at a time and update the trailing matrix in TILE x TILE register tiles
LDS_MAX, PANEL, TILE = 192, 16, 4
BOUNDARIES = (TILE, PANEL, LDS_MAX, MAX_LEN)


def _rows(rows) -> np.ndarray:
    r = np.array(rows, np.float64, copy=True).reshape(-1, 8)
    if len(r) and len(np.unique(r[:, :2], axis=0)) != len(r):
        raise ValueError("duplicate (frame, id)")
    return r


def _sorted(r: np.ndarray) -> np.ndarray:
    return r[np.lexsort((r[:, 1], r[:, 0]))] if len(r) else r


def _tracks(r: np.ndarray):
    out = []
    for tid in np.unique(r[:, 1]):
        t = r[r[:, 1] == tid]
        out.append((float(tid), t[np.argsort(t[:, 0], kind="stable")]))
    return out


def interpolate(rows, interval: int = INTERVAL) -> np.ndarray:
    """Fill every gap of fewer than `interval` frames inside a track by linear interpolation (docs/GSI.md §1): per corner
    step = (v1 - v0) / (f1 - f0), v = v0 + step * j; conf 0.0 marks the inserted rows, cls is the earlier row's.  Host, float64."""
    r = _rows(rows)
    new = []
    for tid, t in _tracks(r):
        f = t[:, 0].astype(np.int64)
        for k in np.nonzero((np.diff(f) > 1) & (np.diff(f) < interval))[0]:
            a, b, gap = t[k], t[k + 1], int(f[k + 1] - f[k])
            j = np.arange(1, gap, dtype=np.float64)
            blk = np.empty((gap - 1, 8))
            blk[:, 0], blk[:, 1], blk[:, 6], blk[:, 7] = a[0] + j, tid, 0.0, a[7]
            for c in range(2, 6):
                blk[:, c] = a[c] + ((b[c] - a[c]) / float(gap)) * j
            new.append(blk)
    if new:
        r = np.concatenate([r] + new, 0)
    return _sorted(r)


def length_scale(n: int, tau: float = TAU) -> float:
    """The RBF length scale of a track of n rows: clip(tau ln(tau^3 / n), 1 / tau, tau^2), float64 on the host."""
    tau = float(tau)
    t3 = tau * tau * tau
    return float(np.clip(tau * np.log(t3 / float(n)), 1.0 / tau, tau * tau))


def smooth(rows, engine, tau: float = TAU, alpha: float = ALPHA):
    """-> (rows by (frame, id), {id: status}): x1, y1, w, h of every track smoothed on the device, x2 = x1 + w, y2 = y1 + h.
    Status 0 smoothed, 1 a pivot was not positive, 2 more than MAX_LEN rows; the rows of 1 and 2 pass through."""
    r = _rows(rows)
    tracks = _tracks(r)
    if not tracks:
        return r, {}
    t = np.concatenate([tr for _, tr in tracks], 0)
    lens = np.array([len(tr) for _, tr in tracks], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    vals = np.stack([t[:, 2], t[:, 3], t[:, 4] - t[:, 2], t[:, 5] - t[:, 3]], 1)
    ls = np.array([length_scale(int(n), tau) for n in lens], np.float64)
    out, status = engine.gsi_smooth(offsets, t[:, 0].astype(np.int32), vals, ls, alpha)
    ok = np.repeat(status == 0, lens)
    t[ok, 2], t[ok, 3] = out[ok, 0], out[ok, 1]
    t[ok, 4], t[ok, 5] = out[ok, 0] + out[ok, 2], out[ok, 1] + out[ok, 3]
    return _sorted(t), {int(tid): int(s) for (tid, _), s in zip(tracks, status)}


def gsi(rows, engine, interval: int = INTERVAL, tau: float = TAU):
    """Both steps: (rows, {id: status})."""
    return smooth(interpolate(rows, interval), engine, tau)


def rows_of(results, frame_id: int) -> np.ndarray:
    """The tracked boxes of one frame's Results as rows [n, 8], corners as the floats the tracker gave (not truncated)."""
    out = []
    for r in results:
        b = None if r is None else r.boxes if r.boxes is not None else getattr(r, "obb", None)    # an oriented-box result: its envelopes (docs/OBB.md §3)
        if b is None or b.id is None or len(b) == 0:
            continue
        f = [np.asarray(v.cpu() if hasattr(v, "cpu") else v, np.float64).reshape(len(b), -1) for v in (b.id, b.xyxy, b.conf, b.cls)]
        out.append(np.concatenate([np.full((len(b), 1), float(frame_id)), f[0], f[1], f[2], f[3]], 1))
    return np.concatenate(out, 0) if out else np.zeros((0, 8))


def label_lines(rows) -> str:
    return "".join(f"{int(r[0])} {int(r[7])} {int(r[1])} {round(float(r[6]), 3)} {int(r[2])} {int(r[3])} {int(r[4])} {int(r[5])} -1 -1 -1 -1\n"
                   for r in np.asarray(rows, np.float64).reshape(-1, 8))


def write_labels(path: str, rows) -> int:
    """LabelsWriter's line format (cli.py): `frame cls id conf x1 y1 x2 y2 -1 -1 -1 -1`, int() corners, round(conf, 3)."""
    rows = np.asarray(rows, np.float64).reshape(-1, 8)
    with open(path, "w") as f:
        f.write(label_lines(rows))
    return len(rows)


def max_len() -> int:
    return int(_lib.load().ss_gsi_max_len())
