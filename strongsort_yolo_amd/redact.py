"""Redaction of the people a saved frame shows (docs/REDACT.md): blur, pixelate or fill regions of BGR u8 frames where they lie on
the device, before the overlay draws on them.  `regions_of` turns a frame's `Results` into regions (boxes, ellipses, heads from the
face keypoints of a pose model, silhouettes from the mask polygons of a segmentation model, rotated boxes of an OBB model);
`Redactor.apply_device` runs `ss_redact` (csrc/ss_redact.hip) over a batch in one call.  Everything is integer arithmetic on the
untouched frame: parity with tests/redact_ref.py is exact; parity with cv2.blur / cv2.GaussianBlur is not claimed (cv2 is not a
dependency, and the borders, the rounding and the cell alignment here are the project's own definition).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

RECT, ELLIPSE, POLY = 0, 1, 2
EFFECTS = ("blur", "pixelate", "fill")
REGIONS = ("box", "ellipse", "head", "mask")
CELLS = (4, 8, 16, 32)
DEFAULT_STRENGTH = {"blur": 15, "pixelate": 16, "fill": 0}
VERT_RANGE = (-8192, 16383)        # vertex coordinates the polygon tests take without overflow (include/strongsort_hip.h)
_LIM = 1 << 30


def caps() -> dict:
    """The library's caps, asked from it (no GPU needed)."""
    from . import lib
    L = lib.load()
    return {"regions": L.ss_redact_max_regions(), "vertices": L.ss_redact_max_vertices(), "radius": L.ss_redact_max_radius()}


@dataclass
class RedactConfig:
    effect: str = "blur"
    strength: Optional[int] = None              # blur: the radius r of the (2r+1)^2 box; pixelate: the cell side; None: 15 / 16
    region: str = "box"
    classes: Optional[Sequence[int]] = None     # None: every class
    pad: float = 0.0                            # box / ellipse: this fraction of the box side is added on each side
    fill_color: Tuple[int, int, int] = (0, 0, 0)     # B, G, R
    head_scale: float = 0.75
    head_frac: float = 0.2

    def __post_init__(self):
        if self.effect not in EFFECTS:
            raise ValueError(f"redact: effect '{self.effect}' is not one of {', '.join(EFFECTS)}")
        if self.region not in REGIONS:
            raise ValueError(f"redact: region '{self.region}' is not one of {', '.join(REGIONS)}")
        if self.strength is None:
            self.strength = DEFAULT_STRENGTH[self.effect]
        self.strength = int(self.strength)
        if self.effect == "blur" and not 1 <= self.strength <= 31:
            raise ValueError("redact: the blur radius must be 1 .. 31")
        if self.effect == "pixelate" and self.strength not in CELLS:
            raise ValueError("redact: the pixelate cell must be one of 4, 8, 16, 32")
        if not (0.0 <= float(self.pad) <= 4.0):
            raise ValueError("redact: pad must be 0 .. 4")
        if not (float(self.head_scale) > 0 and 0.0 < float(self.head_frac) <= 1.0):
            raise ValueError("redact: head_scale must be positive and head_frac in (0, 1]")
        col = tuple(int(v) for v in self.fill_color)
        if len(col) != 3 or any(not 0 <= v <= 255 for v in col):
            raise ValueError("redact: fill_color is three values B, G, R of 0 .. 255")
        self.fill_color = col
        if self.classes is not None:
            self.classes = tuple(int(c) for c in self.classes)


class _Builder:
    def __init__(self, max_regions, max_vertices):
        self.rows, self.verts, self.nv = [], [], 0
        self.max_regions, self.max_vertices = max_regions, max_vertices

    def shape(self, kind, x0, y0, x1, y1):
        c = lambda v: int(min(max(v, -_LIM), _LIM))
        self.rows.append((kind, c(x0), c(y0), c(x1), c(y1), 0, 0, 0))

    def poly(self, pts):
        q = np.ascontiguousarray(np.int32(pts)).reshape(-1, 2)        # np.int32(polygon): what the overlay draws
        n = len(q)
        if n < 3:
            return                                                     # a degenerate polygon covers nothing
        if n > self.max_vertices:
            raise ValueError(f"redact: a polygon of {n} vertices is above the cap of {self.max_vertices}")
        lo, hi = q.min(0), q.max(0)
        if min(lo) < VERT_RANGE[0] or max(hi) > VERT_RANGE[1]:
            raise ValueError(f"redact: a polygon vertex lies outside {VERT_RANGE[0]} .. {VERT_RANGE[1]}")
        self.rows.append((POLY, int(lo[0]), int(lo[1]), int(hi[0]), int(hi[1]), self.nv, n, 0))
        self.verts.append(q)
        self.nv += n

    def arrays(self):
        if len(self.rows) > self.max_regions:
            raise ValueError(f"redact: {len(self.rows)} regions in one frame are above the cap of {self.max_regions}")
        rows = np.array(self.rows, dtype=np.int32).reshape(-1, 8)
        return rows, (np.concatenate(self.verts) if self.verts else np.zeros((0, 2), np.int32))


def _head(b, xyxy, kpts, cfg):
    """The head of one pose row: an ellipse about the valid face keypoints (nose, eyes, ears: 0..4; valid by the reference's rule,
    (x, y) != (0, 0)); with none of them the top head_frac of the box, so that a head turned away stays covered."""
    face = [(float(p[0]), float(p[1])) for p in np.asarray(kpts, np.float64)[:5]]
    face = [p for p in face if not (p[0] == 0.0 and p[1] == 0.0)]
    x0, y0, x1, y1 = (int(v) for v in xyxy)
    if not face:
        b.shape(RECT, x0, y0, x1, y0 + int(math.floor(float(cfg.head_frac) * float(y1 - y0))))
        return
    sx = sy = 0.0
    for px, py in face:
        sx, sy = sx + px, sy + py
    cx, cy = sx / len(face), sy / len(face)
    d = (float(xyxy[2]) - float(xyxy[0])) / 6.0
    for i, (ax, ay) in enumerate(face):
        for bx, by in face[i + 1:]:
            d = max(d, math.sqrt((ax - bx) ** 2 + (ay - by) ** 2))
    a = float(cfg.head_scale) * d
    h = 1.25 * a
    b.shape(ELLIPSE, math.floor(cx - a), math.floor(cy - h), math.floor(cx + a), math.floor(cy + h))


def regions_of(results, cfg: RedactConfig, max_regions: Optional[int] = None, max_vertices: Optional[int] = None):
    """One frame's `Results` -> (int32 [n, 8] regions {type, x0, y0, x1, y1, vertex offset, vertices, 0}, int32 [m, 2] vertices).
    Box corners are truncated as Overlay._box truncates them: the redacted rectangle is the drawn rectangle.  More regions or
    vertices than the library takes raise — a dropped region would be a leaked face."""
    if max_regions is None or max_vertices is None:
        c = caps()
        max_regions = c["regions"] if max_regions is None else max_regions
        max_vertices = c["vertices"] if max_vertices is None else max_vertices
    b = _Builder(int(max_regions), int(max_vertices))
    want = None if cfg.classes is None else set(cfg.classes)
    for r in results:
        if r is None:
            continue
        obb = getattr(r, "obb", None)
        if r.boxes is None and obb is not None:
            if cfg.region not in ("box", "ellipse"):
                raise ValueError(f"redact: region '{cfg.region}' is not available on an oriented-box model")
            for cls, pts in zip(obb.cls, obb.xyxyxyxy.tolist()):
                if want is None or int(cls) in want:
                    b.poly(pts)
            continue
        if r.boxes is None:
            continue
        if cfg.region == "head" and r.keypoints is None:
            raise ValueError("redact: region 'head' needs keypoints: use a pose model")
        if cfg.region == "mask" and getattr(r, "masks", None) is None:
            raise ValueError("redact: region 'mask' needs masks: use a segmentation model")
        boxes = r.boxes.xyxy.tolist() if hasattr(r.boxes.xyxy, "tolist") else [list(v) for v in r.boxes.xyxy]
        for i, (xyxy, cls) in enumerate(zip(boxes, r.boxes.cls)):
            if want is not None and int(cls) not in want:
                continue
            if cfg.region == "head":
                _head(b, xyxy, r.keypoints.xy[i], cfg)
            elif cfg.region == "mask":
                polys = r.masks.xy[i]
                for poly in (polys if isinstance(polys, (list, tuple)) else [polys]):
                    b.poly(poly)
            else:
                x0, y0, x1, y1 = (int(v) for v in xyxy)
                gx, gy = int(math.floor(float(cfg.pad) * float(x1 - x0))), int(math.floor(float(cfg.pad) * float(y1 - y0)))
                b.shape(RECT if cfg.region == "box" else ELLIPSE, x0 - gx, y0 - gy, x1 + gx, y1 + gy)
    return b.arrays()


class Redactor:
    """The device launcher: regions of every frame of a batch uploaded once, ONE `ss_redact` call, in place."""

    def __init__(self, cfg: RedactConfig, engine):
        self.cfg, self.eng = cfg, engine
        L = engine.L
        self.max_regions, self.max_vertices = L.ss_redact_max_regions(), L.ss_redact_max_vertices()
        if cfg.effect == "blur" and cfg.strength > L.ss_redact_max_radius():
            raise ValueError(f"redact: the blur radius is at most {L.ss_redact_max_radius()}")
        self._scratch = self._frame = None
        self._keep = []

    def regions(self, results):
        return regions_of(results, self.cfg, self.max_regions, self.max_vertices)

    def apply_regions_device(self, frames, regions_per_frame, stream=None):
        """frames uint8 [B,H,W,3] (or [H,W,3]) on the device, in place; regions_per_frame: one (rows, vertices) pair per frame."""
        import torch
        e, cfg = self.eng, self.cfg
        fr = frames if frames.dim() == 4 else frames.unsqueeze(0)
        if fr.dtype != torch.uint8 or fr.shape[-1] != 3 or fr.stride(3) != 1 or fr.stride(2) != 3:
            raise ValueError("redact: frames must be uint8 [B,H,W,3] with packed pixels")
        if len(regions_per_frame) != fr.shape[0]:
            raise ValueError("redact: one region list per frame")
        off, voff, rows, verts = np.zeros(fr.shape[0] + 1, np.int32), 0, [], []
        for i, (rw, vt) in enumerate(regions_per_frame):
            rw = np.array(rw, dtype=np.int32).reshape(-1, 8)
            if len(rw) > self.max_regions:
                raise ValueError(f"redact: {len(rw)} regions in one frame are above the cap of {self.max_regions}")
            rw[rw[:, 0] == POLY, 5] += voff                              # vertex offsets into the concatenated array
            rows.append(rw)
            verts.append(np.asarray(vt, np.int32).reshape(-1, 2))
            off[i + 1] = off[i] + len(rw)
            voff += len(verts[-1])
        if off[-1] == 0:
            return frames                                               # nothing to hide in this batch: no launch
        rows, verts = np.concatenate(rows), np.concatenate(verts)
        if len(verts) == 0:
            verts = np.zeros((1, 2), np.int32)
        st = torch.cuda.current_stream(fr.device) if stream is None else stream
        B, H, W = fr.shape[:3]
        need = int(e.L.ss_redact_scratch_bytes(B, H, W))
        if need < 0:
            raise ValueError("redact: batch outside 1..65535 or a frame side outside 1..8192")
        with torch.cuda.stream(st):
            if self._scratch is None or self._scratch.numel() < need or self._scratch.device != fr.device:
                self._scratch = torch.empty(need, dtype=torch.uint8, device=fr.device)
            d_rows, d_off, d_verts = (torch.from_numpy(a).to(fr.device) for a in (rows, off, verts))
        col = cfg.fill_color[0] | cfg.fill_color[1] << 8 | cfg.fill_color[2] << 16
        e._ck(e.L.ss_redact(e.ctx, C.c_void_p(st.cuda_stream), C.c_void_p(fr.data_ptr()), B, fr.stride(0), H, W, fr.stride(1),
                            C.c_void_p(d_rows.data_ptr()), C.c_void_p(d_off.data_ptr()), C.c_void_p(d_verts.data_ptr()),
                            EFFECTS.index(cfg.effect), cfg.strength, col, C.c_void_p(self._scratch.data_ptr()), self._scratch.numel()))
        for t in (d_rows, d_off, d_verts, self._scratch):
            t.record_stream(st)
        self._keep = [d_rows, d_off, d_verts]                           # alive until the next call
        return frames

    def apply_device(self, frames, results_per_frame, stream=None):
        """frames uint8 [B,H,W,3] with one results list per frame, or [H,W,3] with the frame's results list: redacted in place, one
        call for the whole batch, enqueued on `stream` (default: the current torch stream)."""
        per = [results_per_frame] if frames.dim() == 3 else list(results_per_frame)
        return self.apply_regions_device(frames, [self.regions(r) for r in per], stream)

    def apply(self, frame: np.ndarray, results) -> np.ndarray:
        """Host frame in, redacted host frame out (upload -> ss_redact -> download)."""
        import torch
        e = self.eng
        if self._frame is None or self._frame.shape != frame.shape:
            self._frame = torch.empty(frame.shape, dtype=torch.uint8, device=e.device)
        e.upload(self._frame, frame)
        self.apply_device(self._frame, results)
        out = np.empty_like(frame)
        e.download(out, self._frame)
        return out
