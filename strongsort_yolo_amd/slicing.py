"""Sliced inference (SAHI, "slicing aided hyper inference"): the host side — the tile grid, the canvas all tiles share, the table
csrc/ss_slice.hip reads.  Semantics, decisions and kernels: docs/SLICE.md; the merge's reference: tests/slice_ref.py."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .engine import LetterboxGeom, letterbox_geometry, scale_geometry

MAX_TILES = 64              # ss_slice_max_tiles(): tiles of a frame, the full frame included
MAX_CANDIDATES = 8192       # ss_slice_max_candidates(): tiles x rows per tile
MERGES, METRICS = ("nms", "nmm"), ("iou", "ios")


def _pair(v, name):
    p = tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    if len(p) != 2:
        raise ValueError(f"{name}: one value or (height, width)")
    return p


@dataclass(frozen=True)
class SliceConfig:
    """slice_hw (sh, sw): tile size in frame pixels; overlap: one ratio or (oh, ow), each in [0, 1); full: the whole frame as one more
    tile (SAHI's standard prediction); merge "nmm" (GREEDYNMM) or "nms"; metric "ios" or "iou"; thr: the match threshold."""
    slice_hw: tuple
    overlap: tuple = (0.2, 0.2)
    full: bool = True
    merge: str = "nmm"
    metric: str = "ios"
    thr: float = 0.5

    def __post_init__(self):
        hw = _pair(self.slice_hw, "slice_hw")
        ov = _pair(self.overlap, "slice_overlap")
        if any(int(v) != v or int(v) < 1 for v in hw):
            raise ValueError(f"slice_hw {self.slice_hw}: positive integers")
        if not all(0.0 <= float(o) < 1.0 for o in ov):
            raise ValueError(f"slice_overlap {self.overlap}: each ratio in [0, 1)")
        if self.merge not in MERGES:
            raise ValueError(f"slice_merge {self.merge!r}: one of {MERGES}")
        if self.metric not in METRICS:
            raise ValueError(f"slice_metric {self.metric!r}: one of {METRICS}")
        if not np.isfinite(self.thr):
            raise ValueError("slice_thr must be finite")
        object.__setattr__(self, "slice_hw", (int(hw[0]), int(hw[1])))
        object.__setattr__(self, "overlap", (float(ov[0]), float(ov[1])))
        object.__setattr__(self, "full", bool(self.full))
        object.__setattr__(self, "thr", float(self.thr))

    def key(self):
        return (self.slice_hw, self.overlap, self.full, self.merge, self.metric, self.thr)


def _origins(n, s, ov, side):
    """Origins along one axis: windows of s at steps of s - int(ov * s) while the unshifted end is inside; the window that would pass
    the border is shifted back inside, not shrunk."""
    if s > n:
        raise ValueError(f"slice {side} {s} is larger than the frame's {n}")
    step_back, out, lo = int(ov * s), [], 0
    while True:
        hi = lo + s
        out.append(n - s if hi > n else lo)
        if hi >= n:
            return out
        lo = hi - step_back


def grid(H: int, W: int, slice_hw, overlap=(0.2, 0.2), full: bool = True):
    """-> [(x0, y0, tile_w, tile_h), ...] row-major, every cut tile exactly slice_hw, the whole frame last when `full`."""
    (sh, sw), (oh, ow) = _pair(slice_hw, "slice_hw"), _pair(overlap, "slice_overlap")
    ys, xs = _origins(H, sh, oh, "height"), _origins(W, sw, ow, "width")
    tiles = [(x, y, sw, sh) for y in ys for x in xs]
    if full:
        tiles.append((0, 0, W, H))
    if len(tiles) > MAX_TILES:
        raise ValueError(f"{len(tiles)} tiles (the full frame included), at most {MAX_TILES}")
    return tiles


def canvas(H: int, W: int, cfg: SliceConfig, imgsz: int = 640, stride: int = 32):
    """-> (canvas LetterboxGeom of a cut tile, int32 table [T][8] = x0, y0, tile_w, tile_h, new_w, new_h, pad_left, pad_top).
    The canvas is letterbox_geometry(sh, sw): a cut tile uses it as it is; the full-frame tile is letterboxed into the same canvas,
    pads centred with the round(x - 0.1) rule."""
    sh, sw = cfg.slice_hw
    g = letterbox_geometry(sh, sw, imgsz, stride)
    rows = []
    for x0, y0, tw, th in grid(H, W, cfg.slice_hw, cfg.overlap, cfg.full):
        if (tw, th) == (sw, sh):
            rows.append((x0, y0, tw, th, g.new_w, g.new_h, g.pad_left, g.pad_top))
        else:
            r = min(g.out_h / th, g.out_w / tw)
            nw, nh = max(int(round(tw * r)), 1), max(int(round(th * r)), 1)
            rows.append((x0, y0, tw, th, nw, nh, int(round((g.out_w - nw) / 2 - 0.1)), int(round((g.out_h - nh) / 2 - 0.1))))
    return g, np.asarray(rows, np.int32)


def nms_geometry(g: LetterboxGeom, table):
    """float32 [T][5]: ss_nms_batch's geometry rows {gain, pad_x, pad_y, tile_w, tile_h} (what ss_slice_nms_geom writes)."""
    return np.asarray([[*scale_geometry(g, int(t[3]), int(t[2])), float(t[2]), float(t[3])] for t in table], np.float32)


def rows_per_tile(pipeline_rows: int, n_tiles: int) -> int:
    return min(int(pipeline_rows), MAX_CANDIDATES // n_tiles)
