"""The definition of the analytics stage (docs/ZONES.md) in plain Python and NumPy: line crossings, zones, dwell, heat and the blend.

Every floating-point step is one IEEE f64 add, sub or mul on Python floats (never fused), in the order written here; everything else
is integer arithmetic.  csrc/ss_zone.hip gives these bytes.  Nothing of the package is imported.
"""
import math

import numpy as np

MAX_LINES, MAX_ZONES, MAX_VERTICES, MAX_LIVE, MAX_CELLS, ROWS = 16, 16, 32, 1024, 65536, 256


def side(ax, ay, bx, by, px, py):
    """1 when P is on the non-negative side of a -> b (all doubled coordinates)."""
    return 1 if (bx - ax) * (py - ay) - (by - ay) * (px - ax) >= 0.0 else 0


def crosses(line2, p0, p1):
    """0: no crossing, 1: inward (P1 on side 1), 2: outward.  line2 = doubled ax, ay, bx, by."""
    ax, ay, bx, by = line2
    s0, s1 = side(ax, ay, bx, by, *p0), side(ax, ay, bx, by, *p1)
    if s0 == s1:
        return 0
    if side(p0[0], p0[1], p1[0], p1[1], ax, ay) == side(p0[0], p0[1], p1[0], p1[1], bx, by):
        return 0
    return 1 if s1 == 1 else 2


def inside(poly2, px, py):
    """Even-odd rule on doubled vertices [[x, y], ...]."""
    par, n = 0, len(poly2)
    for i in range(n):
        vix, viy = poly2[i]
        vjx, vjy = poly2[(i + 1) % n]
        if (viy > py) != (vjy > py):
            t = (vjx - vix) * (py - viy) - (px - vix) * (vjy - viy)
            par ^= int(t > 0.0 if vjy > viy else t < 0.0)
    return par


def counted_rows(rows, n):
    """Indices of the rows that count: id = int(row[4]) >= 1 (and below 2^31), finite corners, the lowest row of every id."""
    out, seen = [], set()
    for r in range(min(int(n), ROWS)):
        x1, y1, x2, y2, idf = (float(v) for v in rows[r, :5])
        if not (idf >= 1.0 and idf < 2147483648.0) or not all(math.isfinite(v) for v in (x1, y1, x2, y2)):
            continue
        if int(idf) in seen:
            continue
        seen.add(int(idf))
        out.append(r)
    return out


class ZoneRef:
    """lines [[ax, ay, bx, by], ...] and zones [[[x, y], ...], ...] in integer pixels; heat None / "anchor" / "box"."""

    def __init__(self, lines=(), zones=(), anchor="bottom", max_gap=30, n_classes=80, heat=None, cell=8, frame_hw=None, n_streams=1):
        assert anchor in ("centre", "bottom") and 1 <= max_gap <= 32 and 1 <= n_classes <= 128 and heat in (None, "anchor", "box")
        assert len(lines) <= MAX_LINES and len(zones) <= MAX_ZONES and all(3 <= len(z) <= MAX_VERTICES for z in zones)
        self.lines = [[2.0 * int(v) for v in l] for l in lines]
        self.zones = [[(2.0 * int(x), 2.0 * int(y)) for x, y in z] for z in zones]
        self.anchor, self.max_gap, self.nc, self.heat, self.S = anchor, max_gap, n_classes, heat, n_streams
        self.k = int(cell).bit_length() - 1
        assert 1 << self.k == cell and 0 <= self.k <= 6
        self.h, self.w = frame_hw if heat else (0, 0)
        self.gh, self.gw = ((self.h + cell - 1) // cell, (self.w + cell - 1) // cell) if heat else (1, 1)
        assert self.gh * self.gw <= MAX_CELLS
        self.reset()

    def reset(self, stream=-1):
        for s in range(self.S) if stream < 0 else [stream]:
            if not hasattr(self, "st"):
                self.st = [None] * self.S
            self.st[s] = dict(frame=0, tracks={}, line_class=np.zeros((MAX_LINES, 2, self.nc), np.int32), line_totals=np.zeros((MAX_LINES, 2), np.int32),
                              entries=np.zeros(MAX_ZONES, np.int32), exits=np.zeros(MAX_ZONES, np.int32), dwell_sum=np.zeros(MAX_ZONES, np.int64),
                              longest=np.zeros(MAX_ZONES, np.int32), peak=np.zeros(MAX_ZONES, np.int32), heat=np.zeros((self.gh, self.gw), np.int32), heat_max=0)

    def totals(self, stream=0):
        st = self.st[stream]
        return dict(frames=st["frame"], heat_max=int(st["heat_max"]),
                    **{k: st[k].copy() for k in ("line_class", "line_totals", "entries", "exits", "dwell_sum", "longest", "peak")})

    def heatmap(self, stream=0):
        return self.st[stream]["heat"].copy()

    def _frame(self, st, rows, n, out, f_idx, s):
        f = st["frame"]
        occ = np.zeros(MAX_ZONES, np.int32)
        for r in counted_rows(rows, n):
            x1, y1, x2, y2 = (float(v) for v in rows[r, :4])
            tid = int(float(rows[r, 4]))
            AX = x1 + x2
            AY = 2.0 * y2 if self.anchor == "bottom" else y1 + y2
            tr = st["tracks"].get(tid)
            if tr is not None and f - tr["last"] > self.max_gap:
                tr = None                                           # the state is lost: a first appearance
            ev = 0
            if tr is not None:
                for l, ln in enumerate(self.lines):
                    c = crosses(ln, (tr["ax"], tr["ay"]), (AX, AY))
                    if c:
                        d = c - 1
                        ev |= 1 << (16 * d + l)
                        st["line_totals"][l, d] += 1
                        cf = float(rows[r, 5])
                        if cf >= 0.0 and cf < float(self.nc):
                            st["line_class"][l, d, int(cf)] += 1
            cur = 0
            for z, poly in enumerate(self.zones):
                cur |= inside(poly, AX, AY) << z
            prev = tr["inside"] if tr is not None else 0
            entry = dict(tr["entry"]) if tr is not None else {}
            dw = 0
            for z in range(len(self.zones)):
                bit = 1 << z
                if prev & ~cur & bit:
                    d = tr["last"] - entry.pop(z) + 1
                    st["exits"][z] += 1
                    st["dwell_sum"][z] += d
                    st["longest"][z] = max(st["longest"][z], d)
                if cur & bit:
                    if not prev & bit:
                        entry[z] = f
                        st["entries"][z] += 1
                    dw = max(dw, f - entry[z] + 1)
                    occ[z] += 1
            st["tracks"][tid] = dict(last=f, ax=AX, ay=AY, inside=cur, entry=entry)
            if self.heat == "anchor":
                px, py = math.floor(AX * 0.5), math.floor(AY * 0.5)
                if 0 <= px < self.w and 0 <= py < self.h:
                    st["heat"][py >> self.k, px >> self.k] += 1
            elif self.heat == "box":
                xa, xb = max(0, math.floor(x1)), min(self.w - 1, math.ceil(x2) - 1)
                ya, yb = max(0, math.floor(y1)), min(self.h - 1, math.ceil(y2) - 1)
                if xa <= xb and ya <= yb:
                    st["heat"][ya >> self.k:(yb >> self.k) + 1, xa >> self.k:(xb >> self.k) + 1] += 1
            out["events"][f_idx, s, r], out["inside"][f_idx, s, r], out["dwell"][f_idx, s, r] = ev, cur, dw
        st["peak"] = np.maximum(st["peak"], occ)
        if self.heat:
            st["heat_max"] = max(st["heat_max"], int(st["heat"].max()))
        st["tracks"] = {t: v for t, v in st["tracks"].items() if f - v["last"] < self.max_gap}   # gone for every later frame
        st["frame"] = f + 1
        out["line_totals"][f_idx, s] = st["line_totals"]
        out["occupancy"][f_idx, s] = occ
        out["heat_frames"][f_idx, s] = st["heat"]
        out["heat_max"][f_idx, s] = st["heat_max"]

    def update_group(self, rows, counts):
        """rows [F, S, 256, 8] f32, counts [F, S] (negative: the stream sits the frame out, its outputs stay 0) -> dict of arrays."""
        rows, counts = np.asarray(rows, np.float32), np.asarray(counts, np.int64)
        F, S = counts.shape
        assert S == self.S and rows.shape == (F, S, ROWS, 8)
        out = dict(events=np.zeros((F, S, ROWS), np.uint32), inside=np.zeros((F, S, ROWS), np.uint32), dwell=np.zeros((F, S, ROWS), np.int32),
                   line_totals=np.zeros((F, S, MAX_LINES, 2), np.int32), occupancy=np.zeros((F, S, MAX_ZONES), np.int32),
                   heat_frames=np.zeros((F, S, self.gh, self.gw), np.int32), heat_max=np.zeros((F, S), np.int32))
        for fi in range(F):
            for s in range(S):
                if counts[fi, s] >= 0:
                    self._frame(self.st[s], rows[fi, s], counts[fi, s], out, fi, s)
        return out


def colormap():
    """The 256 x 3 BGR table zones.py ships, by its integer formula (a jet ramp): u = 4 t, channel = clip(382 - |u - centre|, 0, 255)
    with centres 255 (blue), 510 (green), 765 (red)."""
    t = np.arange(256, dtype=np.int64) * 4
    return np.stack([np.clip(382 - np.abs(t - c), 0, 255) for c in (255, 510, 765)], 1).astype(np.uint8)


def blend(frame, heat, m, k, lut, a):
    """frame u8 [h, w, 3] -> the blended copy: v = heat[y >> k][x >> k]; v <= 0 keeps the pixel; t = (min(v, m) * 255 + m // 2) // m with
    m = max(m, 1); out = (pix * (256 - a) + lut[t] * a + 128) >> 8."""
    h, w = frame.shape[:2]
    m = max(int(m), 1)
    v = np.asarray(heat, np.int64)[np.arange(h)[:, None] >> k, np.arange(w)[None, :] >> k]
    t = (np.minimum(np.maximum(v, 0), m) * 255 + m // 2) // m
    col = np.asarray(lut, np.int64)[t]
    out = (frame.astype(np.int64) * (256 - a) + col * a + 128) >> 8
    return np.where((v > 0)[..., None], out, frame).astype(np.uint8)
