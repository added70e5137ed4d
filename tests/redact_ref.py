"""NumPy int64 restatement of the redaction (docs/REDACT.md): the three effects, the three coverage rules and the region builder.
Written from the document, independent of strongsort_yolo_amd/redact.py and of the library: the GPU tests compare whole buffers with
what is computed here, byte for byte.

Regions: int32 rows {type, x0, y0, x1, y1, vertex offset, vertices, 0} and an int32 [m, 2] vertex array.
  RECT 0     inclusive corners in any order, clipped to the frame
  ELLIPSE 1  inscribed in that CLIPPED rectangle: a = x1-x0+1, b = y1-y0+1, (2x-x0-x1)^2 b^2 + (2y-y0-y1)^2 a^2 <= a^2 b^2
  POLY 2     even-odd interior (an edge is crossed when exactly one end has y <= the pixel's and the pixel is strictly left of the
             crossing) united with every closed edge's thickness-2 line coverage (4 d^2 <= 2^2, d the distance to the segment);
             fewer than 3 vertices cover nothing
Every output pixel is computed from the untouched input; only covered pixels change.
"""
import math

import numpy as np

RECT, ELLIPSE, POLY = 0, 1, 2
BLUR, PIXELATE, FILL = 0, 1, 2
EFFECTS = {"blur": BLUR, "pixelate": PIXELATE, "fill": FILL}
MAX_REGIONS, MAX_VERTICES, MAX_RADIUS = 1024, 4096, 31
VERT_MIN, VERT_MAX = -8192, 16383
LIM = 1 << 30


def reflect(i, n):
    """reflect-101 by repeated reflection: period 2 (n - 1); 0 when n == 1"""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    t = np.mod(i, p)
    return np.where(t < n, t, p - t)


def blur_sums(x, r):
    """x int [H, W(, C)] -> the (2r+1)^2 window sums, borders reflect-101"""
    x = np.asarray(x, np.int64)
    H, W = x.shape[:2]
    p = x[reflect(np.arange(-r, H + r), H)][:, reflect(np.arange(-r, W + r), W)]
    c = np.zeros((p.shape[0] + 1, p.shape[1] + 1) + p.shape[2:], np.int64)
    c[1:, 1:] = p.cumsum(0).cumsum(1)
    k = 2 * r + 1
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def blur(x, r):
    k2 = (2 * r + 1) ** 2
    return ((blur_sums(x, r) + k2 // 2) // k2).astype(np.uint8)


def pixelate(x, c):
    x = np.asarray(x, np.int64)
    H, W = x.shape[:2]
    out = np.empty(x.shape, np.uint8)
    for y in range(0, H, c):
        for xx in range(0, W, c):
            cell = x[y:y + c, xx:xx + c]
            n = cell.shape[0] * cell.shape[1]
            out[y:y + c, xx:xx + c] = (cell.reshape(n, -1).sum(0) + n // 2) // n
    return out


def polygon_interior(q, H, W):
    q = np.asarray(q, np.int64).reshape(-1, 2)
    out = np.zeros((H, W), bool)
    if len(q) < 3:
        return out
    xs, ys = np.arange(W, dtype=np.int64)[None, :], np.arange(H, dtype=np.int64)[:, None]
    cnt = np.zeros((H, W), np.int64)
    for (ax, ay), (bx, by) in zip(np.roll(q, 1, 0), q):
        if ay == by:
            continue
        straddle = (ay <= ys) != (by <= ys)
        dy = by - ay
        lhs, rhs = (xs - ax) * dy, (ys - ay) * (bx - ax)
        cnt += straddle & ((lhs < rhs) if dy > 0 else (lhs > rhs))
    return (cnt & 1).astype(bool)


def line_cover(ax, ay, bx, by, H, W, a=2):
    """thickness-a coverage of the segment: 4 d^2 <= a^2"""
    out = np.zeros((H, W), bool)
    o = (a + 1) >> 1
    x0, x1, y0, y1 = max(min(ax, bx) - o, 0), min(max(ax, bx) + o, W - 1), max(min(ay, by) - o, 0), min(max(ay, by) + o, H - 1)
    if x0 > x1 or y0 > y1:
        return out
    xs, ys = np.arange(x0, x1 + 1, dtype=np.int64)[None, :], np.arange(y0, y1 + 1, dtype=np.int64)[:, None]
    dx, dy, px, py = bx - ax, by - ay, xs - ax, ys - ay
    L, t, a2 = dx * dx + dy * dy, px * dx + py * dy, a * a
    qx, qy = xs - bx, ys - by
    cr = px * dy - py * dx
    out[y0:y1 + 1, x0:x1 + 1] = np.where(t <= 0, 4 * (px * px + py * py) <= a2, np.where(t >= L, 4 * (qx * qx + qy * qy) <= a2, 4 * cr * cr <= a2 * L))
    return out


def region_mask(row, verts, H, W):
    t, x0, y0, x1, y1, off, nv = (int(v) for v in row[:7])
    out = np.zeros((H, W), bool)
    if t == POLY:
        q = np.asarray(verts, np.int64).reshape(-1, 2)[off:off + nv]
        if nv < 3:
            return out
        out |= polygon_interior(q, H, W)
        for (ax, ay), (bx, by) in zip(np.roll(q, 1, 0), q):
            out |= line_cover(int(ax), int(ay), int(bx), int(by), H, W)
        return out
    if t not in (RECT, ELLIPSE):
        return out
    X0, X1, Y0, Y1 = max(min(x0, x1), 0), min(max(x0, x1), W - 1), max(min(y0, y1), 0), min(max(y0, y1), H - 1)
    if X0 > X1 or Y0 > Y1:
        return out
    if t == RECT:
        out[Y0:Y1 + 1, X0:X1 + 1] = True
        return out
    a, b = X1 - X0 + 1, Y1 - Y0 + 1
    xs, ys = np.arange(X0, X1 + 1, dtype=np.int64)[None, :], np.arange(Y0, Y1 + 1, dtype=np.int64)[:, None]
    out[Y0:Y1 + 1, X0:X1 + 1] = (2 * xs - X0 - X1) ** 2 * b * b + (2 * ys - Y0 - Y1) ** 2 * a * a <= a * a * b * b
    return out


def cover(rows, verts, H, W):
    m = np.zeros((H, W), bool)
    for row in np.asarray(rows).reshape(-1, 8):
        m |= region_mask(row, verts, H, W)
    return m


def redact(frame, rows, verts, effect, strength=0, fill_bgr=(0, 0, 0)):
    """frame uint8 [H, W, 3] -> a new array: the effect where a region covers, the input elsewhere"""
    frame = np.asarray(frame)
    H, W = frame.shape[:2]
    e = EFFECTS.get(effect, effect)
    if e == BLUR:
        new = blur(frame, strength)
    elif e == PIXELATE:
        new = pixelate(frame, strength)
    else:
        new = np.empty_like(frame)
        new[:] = np.asarray(fill_bgr, np.uint8)
    out = frame.copy()
    m = cover(rows, verts, H, W)
    out[m] = new[m]
    return out


# ---- the region builder --------------------------------------------------------------------------------------------------
def _clip(v):
    return int(min(max(v, -LIM), LIM))


def _poly_rows(rows, verts, q, max_vertices):
    q = np.asarray(q).astype(np.int32).reshape(-1, 2)
    if len(q) < 3:
        return
    if len(q) > max_vertices:
        raise ValueError(f"redact: a polygon of {len(q)} vertices is above the cap of {max_vertices}")
    if q.min() < VERT_MIN or q.max() > VERT_MAX:
        raise ValueError(f"redact: a polygon vertex lies outside {VERT_MIN} .. {VERT_MAX}")
    off = sum(len(v) for v in verts)
    rows.append((POLY, int(q[:, 0].min()), int(q[:, 1].min()), int(q[:, 0].max()), int(q[:, 1].max()), off, len(q), 0))
    verts.append(q)


def regions_of(results, region="box", classes=None, pad=0.0, head_scale=0.75, head_frac=0.2, max_regions=MAX_REGIONS, max_vertices=MAX_VERTICES):
    """-> (int32 [n, 8], int32 [m, 2]) of one frame's results"""
    rows, verts = [], []
    keep = None if classes is None else {int(c) for c in classes}
    for r in results:
        if r is None:
            continue
        if r.boxes is None and getattr(r, "obb", None) is not None:
            if region not in ("box", "ellipse"):
                raise ValueError(f"redact: region '{region}' is not available on an oriented-box model")
            for cls, pts in zip(r.obb.cls, r.obb.xyxyxyxy.tolist()):
                if keep is None or int(cls) in keep:
                    _poly_rows(rows, verts, np.int32(pts), max_vertices)
            continue
        if r.boxes is None:
            continue
        if region == "head" and r.keypoints is None:
            raise ValueError("redact: region 'head' needs keypoints: use a pose model")
        if region == "mask" and getattr(r, "masks", None) is None:
            raise ValueError("redact: region 'mask' needs masks: use a segmentation model")
        for i in range(len(r.boxes)):
            if keep is not None and int(r.boxes.cls[i]) not in keep:
                continue
            bx = [float(v) for v in r.boxes.xyxy[i]]
            x0, y0, x1, y1 = (int(v) for v in bx)
            if region in ("box", "ellipse"):
                px, py = int(math.floor(float(pad) * float(x1 - x0))), int(math.floor(float(pad) * float(y1 - y0)))
                rows.append((RECT if region == "box" else ELLIPSE, _clip(x0 - px), _clip(y0 - py), _clip(x1 + px), _clip(y1 + py), 0, 0, 0))
            elif region == "head":
                kp = [(float(x), float(y)) for x, y in np.asarray(r.keypoints.xy[i], np.float64)[:5].tolist()]
                kp = [p for p in kp if p != (0.0, 0.0)]
                if kp:
                    cx, cy = sum(p[0] for p in kp) / len(kp), sum(p[1] for p in kp) / len(kp)
                    d = max([math.sqrt((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2) for p in kp for q in kp] + [(bx[2] - bx[0]) / 6.0])
                    a = float(head_scale) * d
                    b = 1.25 * a
                    rows.append((ELLIPSE, _clip(math.floor(cx - a)), _clip(math.floor(cy - b)), _clip(math.floor(cx + a)), _clip(math.floor(cy + b)), 0, 0, 0))
                else:
                    rows.append((RECT, _clip(x0), _clip(y0), _clip(x1), _clip(y0 + int(math.floor(float(head_frac) * float(y1 - y0)))), 0, 0, 0))
            else:
                polys = r.masks.xy[i]
                for poly in (polys if isinstance(polys, (list, tuple)) else [polys]):
                    _poly_rows(rows, verts, np.int32(poly), max_vertices)
    if len(rows) > max_regions:
        raise ValueError(f"redact: {len(rows)} regions in one frame are above the cap of {max_regions}")
    return (np.asarray(rows, np.int32).reshape(-1, 8), np.concatenate(verts).astype(np.int32).reshape(-1, 2) if verts else np.zeros((0, 2), np.int32))
