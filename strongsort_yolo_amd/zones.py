"""Analytics behind the trackers (docs/ZONES.md): line crossings by direction and class, zone occupancy and dwell, a cumulative heat
map and its blend over resident frames, all on the device (csrc/ss_zone.hip).  tests/zones_ref.py is the definition; the device gives
its bytes.  There is no CPU fallback: without the library or a device the calls raise as the rest of the package does.

    cfg = ZoneConfig(lines=[parse_line("100,0,100,480")], zones=[parse_zone("0,0,200,0,200,200,0,200")], heat="box")
    zc = ZoneCounter(cfg, engine, frame_hw=(480, 640))
    zc.update_group_device(out, nout, n_frames)         # a tracker's rows, where they are
    zc.totals(), zc.heatmap()
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import lib as _lib

MAX_LINES, MAX_ZONES, MAX_VERTICES, MAX_LIVE, MAX_CELLS, MAX_COORD, ROWS, GROUP = 16, 16, 32, 1024, 65536, 32767, 256, 32
OUTPUTS = ("events", "inside", "dwell", "line_totals", "occupancy", "heat_frames", "heat_max")


def _ints(text: str, what: str) -> List[int]:
    try:
        v = [int(t) for t in text.split(",")]
    except ValueError:
        raise ValueError(f"{what} '{text}': integer pixel coordinates separated by commas") from None
    bad = [c for c in v if abs(c) > MAX_COORD]
    if bad:
        raise ValueError(f"{what} '{text}': coordinate {bad[0]} outside -{MAX_COORD}..{MAX_COORD}")
    return v


def parse_line(text: str) -> List[int]:
    """`x0,y0,x1,y1` -> [x0, y0, x1, y1], the directed segment a -> b."""
    v = _ints(text, "--line")
    if len(v) != 4:
        raise ValueError(f"--line '{text}': four numbers x0,y0,x1,y1")
    if v[:2] == v[2:]:
        raise ValueError(f"--line '{text}': both ends are the same point")
    return v


def parse_zone(text: str) -> List[List[int]]:
    """`x0,y0,x1,y1,...` -> [[x, y], ...], 3 to 32 vertices."""
    v = _ints(text, "--zone")
    if len(v) % 2 or not 3 <= len(v) // 2 <= MAX_VERTICES:
        raise ValueError(f"--zone '{text}': 3 to {MAX_VERTICES} vertices as x,y pairs")
    return [[v[i], v[i + 1]] for i in range(0, len(v), 2)]


def colormap() -> np.ndarray:
    """The blend's default table, uint8 [256, 3] BGR, a jet ramp by an integer formula: u = 4 t, channel = clip(382 - |u - centre|,
    0, 255) with the centres 255 (blue), 510 (green) and 765 (red)."""
    u = np.arange(256, dtype=np.int64) * 4
    return np.stack([np.clip(382 - np.abs(u - c), 0, 255) for c in (255, 510, 765)], 1).astype(np.uint8)


@dataclass
class ZoneConfig:
    lines: list = field(default_factory=list)        # [[ax, ay, bx, by], ...] integer pixels, directed a -> b
    zones: list = field(default_factory=list)        # [[[x, y], ...], ...] 3 to 32 vertices each, even-odd rule
    anchor: str = "bottom"                           # "bottom": middle of the box's bottom edge; "centre"
    max_gap: int = 30                                # a track unseen for more frames has lost its state (1..32)
    n_classes: int = 80
    heat: Optional[str] = None                       # None, "anchor" or "box"
    heat_cell: int = 8                               # pixels a side, a power of two up to 64
    heat_alpha: int = 128                            # the blend's weight of the heat colour, 0..256

    def validate(self, frame_hw=None):
        """ValueError naming the offending item; what the library refuses is refused here first."""
        if len(self.lines) > MAX_LINES:
            raise ValueError(f"{len(self.lines)} lines, at most {MAX_LINES}")
        if len(self.zones) > MAX_ZONES:
            raise ValueError(f"{len(self.zones)} zones, at most {MAX_ZONES}")
        for i, l in enumerate(self.lines):
            if len(l) != 4 or any(int(c) != c or abs(int(c)) > MAX_COORD for c in l):
                raise ValueError(f"line {i}: four integer coordinates within -{MAX_COORD}..{MAX_COORD}")
            if list(l[:2]) == list(l[2:]):
                raise ValueError(f"line {i}: both ends are the same point")
        for i, z in enumerate(self.zones):
            if not 3 <= len(z) <= MAX_VERTICES:
                raise ValueError(f"zone {i}: {len(z)} vertices, 3 to {MAX_VERTICES} allowed")
            if any(len(p) != 2 or int(p[0]) != p[0] or int(p[1]) != p[1] or max(abs(int(p[0])), abs(int(p[1]))) > MAX_COORD for p in z):
                raise ValueError(f"zone {i}: integer x, y pairs within -{MAX_COORD}..{MAX_COORD}")
        if self.anchor not in ("bottom", "centre"):
            raise ValueError("anchor must be 'bottom' or 'centre'")
        if not 1 <= self.max_gap <= 32:
            raise ValueError(f"max_gap {self.max_gap} outside 1..32")
        if not 1 <= self.n_classes <= 128:
            raise ValueError(f"n_classes {self.n_classes} outside 1..128")
        if self.heat not in (None, "anchor", "box"):
            raise ValueError("heat must be None, 'anchor' or 'box'")
        if self.heat_cell not in (1, 2, 4, 8, 16, 32, 64):
            raise ValueError(f"heat_cell {self.heat_cell}: a power of two from 1 to 64")
        if not 0 <= self.heat_alpha <= 256:
            raise ValueError(f"heat_alpha {self.heat_alpha} outside 0..256")
        if self.heat and frame_hw is not None:
            gh, gw = grid_shape(frame_hw, self.heat_cell)
            if gh * gw > MAX_CELLS:
                raise ValueError(f"heat grid of {gh * gw} cells is over the cap of {MAX_CELLS}: use a larger heat_cell")

    def struct(self, frame_hw=None):
        h, w = frame_hw if (self.heat and frame_hw is not None) else (0, 0)
        return _lib.ss_zone_config(int(self.anchor == "bottom"), int(self.max_gap), int(self.n_classes), (None, "anchor", "box").index(self.heat),
                                   int(self.heat_cell).bit_length() - 1, int(h), int(w))


def grid_shape(frame_hw, cell: int):
    return (int(frame_hw[0]) + cell - 1) // cell, (int(frame_hw[1]) + cell - 1) // cell


def rows_of(results) -> np.ndarray:
    """The tracked boxes of one frame's Results as device-layout rows [n, 8]: x1, y1, x2, y2, id, cls, conf, 0 (float32)."""
    out = []
    for r in results:
        b = None if r is None else r.boxes if r.boxes is not None else getattr(r, "obb", None)    # an oriented-box result: its envelopes (docs/OBB.md §3)
        if b is None or b.id is None or len(b) == 0:
            continue
        xyxy, tid, cls, conf = (np.asarray(v.cpu() if hasattr(v, "cpu") else v, np.float32).reshape(len(b), -1) for v in (b.xyxy, b.id, b.cls, b.conf))
        out.append(np.concatenate([xyxy, tid, cls, conf, np.zeros((len(b), 1), np.float32)], 1))
    return np.concatenate(out, 0) if out else np.zeros((0, 8), np.float32)


@dataclass
class ZoneFrame:
    """What one frame of one stream left: the rows' events / inside bits / dwell, the cumulative line totals [16, 2] (in, out) and
    the occupancy [16].  Overlay.commands(..., zones=this) draws it; `counter` blends the heat first."""
    cfg: ZoneConfig
    events: np.ndarray
    inside: np.ndarray
    dwell: np.ndarray
    line_totals: np.ndarray
    occupancy: np.ndarray
    counter: "ZoneCounter" = None
    stream: int = 0

    def blend_into(self, dev_frame, stream=None):
        if self.counter is not None and self.cfg.heat and self.cfg.heat_alpha:
            self.counter.blend(dev_frame, stream=self.stream, hip_stream=stream)
        return dev_frame


class ZoneCounter:
    """The analytics state of an engine's context: one table, one set of totals and one heat grid per stream, one configuration.
    `engine`: a TrackerEngine or any tracker engine on one (ByteTrackEngine, OCSortEngine, ...).  A context holds one state:
    a second ZoneCounter on the same engine replaces the first."""

    def __init__(self, cfg: ZoneConfig, engine, n_streams: Optional[int] = None, frame_hw=None):
        import torch
        self.cfg, self.eng = cfg, getattr(engine, "base", engine)
        self.S = self.eng.S if n_streams is None else int(n_streams)
        if self.S != self.eng.S:
            raise ValueError(f"ZoneCounter: the engine's context has {self.eng.S} streams, not {self.S}")
        if cfg.heat and frame_hw is None:
            raise ValueError("ZoneCounter: a heat map needs frame_hw=(height, width)")
        cfg.validate(frame_hw)
        self.frame_hw = tuple(int(v) for v in frame_hw) if frame_hw is not None else None
        self.grid = grid_shape(self.frame_hw, cfg.heat_cell) if cfg.heat else (1, 1)
        self.eng.zone_create(cfg.struct(self.frame_hw), cfg.lines, cfg.zones)
        if cfg.heat:
            self.eng.zone_set_colormap(colormap())
        self._torch, self._bufs, self._stage = torch, None, None
        self.last = None

    def close(self):
        if getattr(self.eng, "ctx", None) and self.eng.ctx.value:
            self.eng.zone_destroy()

    def reset(self, stream: int = -1):
        self.eng.zone_reset(stream)

    # ---- device path -------------------------------------------------------------------------------------------
    def _outputs(self, names):
        t, dev, S = self._torch, self.eng.device, self.S
        if self._bufs is None:
            gh, gw = self.grid
            shapes = dict(events=((GROUP, S, ROWS), t.int32), inside=((GROUP, S, ROWS), t.int32), dwell=((GROUP, S, ROWS), t.int32),
                          line_totals=((GROUP, S, MAX_LINES, 2), t.int32), occupancy=((GROUP, S, MAX_ZONES), t.int32),
                          heat_frames=((GROUP, S, gh, gw), t.int32), heat_max=((GROUP, S), t.int32))
            self._shapes, self._bufs = shapes, {}
        for n in names:
            if n not in self._bufs:
                shape, dt = self._shapes[n]
                self._bufs[n] = t.zeros(shape, dtype=dt, device=dev)
        return {n: self._bufs[n] for n in names}

    def update_group_device(self, d_out, d_nout, n_frames: int, outputs=("events", "inside", "dwell", "line_totals", "occupancy")):
        """A tracker's rows where they are: d_out [F,S,256,8] f32 and d_nout [F,S] i32 on the device, read in place, ONE launch, no
        copy.  -> {name: device tensor [F, S, ...]} for the names in `outputs` (OUTPUTS; events and inside hold u32 bits in int32
        tensors).  The tensors are the counter's own and are overwritten by the next call.  Asynchronous on the engine's stream."""
        if not 1 <= int(n_frames) <= GROUP:
            raise ValueError(f"update_group_device: 1 <= n_frames <= {GROUP}")
        bad = [n for n in outputs if n not in OUTPUTS]
        if bad or (not self.cfg.heat and any(n.startswith("heat") for n in outputs)):
            raise ValueError(f"update_group_device: outputs {bad or 'heat_*'} not available")
        if tuple(d_out.shape[1:]) != (self.S, ROWS, 8) or d_out.shape[0] < n_frames or d_out.dtype != self._torch.float32 or not d_out.is_contiguous() or \
                tuple(d_nout.shape[1:]) != (self.S,) or d_nout.shape[0] < n_frames or d_nout.dtype != self._torch.int32 or not d_nout.is_contiguous():
            raise ValueError(f"update_group_device: rows float32 [F, {self.S}, {ROWS}, 8] and counts int32 [F, {self.S}], contiguous")
        o = self._outputs(outputs)
        self.eng.zone_update_group(n_frames, d_out, d_nout, **o)
        return {n: v[:n_frames] for n, v in o.items()}

    # ---- host paths --------------------------------------------------------------------------------------------------
    def update_group(self, rows, counts) -> dict:
        """rows [F, S, 256, 8] float32 and counts [F, S] on the host (a negative count: the stream sits the frame out) -> every
        output as a NumPy array (events / inside uint32).  Synchronous."""
        t = self._torch
        rows, counts = np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(counts, np.int32)
        F = counts.shape[0]
        if rows.shape != (F, self.S, ROWS, 8) or counts.shape != (F, self.S):
            raise ValueError(f"update_group: rows [F, {self.S}, {ROWS}, 8] and counts [F, {self.S}]")
        names = OUTPUTS if self.cfg.heat else OUTPUTS[:5]
        d_rows, d_counts = t.from_numpy(rows).to(self.eng.device), t.from_numpy(counts).to(self.eng.device)
        for v in self._outputs(names).values():
            v[:F].zero_()                                   # a stream that sits a frame out leaves its part as it is
        out = self.update_group_device(d_rows, d_counts, F, names)
        host = {n: v.cpu().numpy() for n, v in out.items()}
        for n in ("events", "inside"):
            host[n] = host[n].view(np.uint32)
        return host

    def update(self, results_or_rows, stream: int = 0) -> ZoneFrame:
        """One frame of one stream: a list of Results (their tracked boxes) or rows [n, 8] = x1, y1, x2, y2, id, cls, conf, any.  The
        other streams sit the frame out.  More than 256 rows: the first 256 count."""
        r = results_or_rows if isinstance(results_or_rows, np.ndarray) else rows_of(results_or_rows)
        r = np.asarray(r, np.float32).reshape(-1, 8)[:ROWS]
        rows, counts = np.zeros((1, self.S, ROWS, 8), np.float32), np.full((1, self.S), -1, np.int32)
        rows[0, stream, :len(r)], counts[0, stream] = r, len(r)
        o = self.update_group(rows, counts)
        self.last = ZoneFrame(self.cfg, o["events"][0, stream, :len(r)], o["inside"][0, stream, :len(r)], o["dwell"][0, stream, :len(r)],
                              o["line_totals"][0, stream], o["occupancy"][0, stream], self, stream)
        return self.last

    def totals(self, stream: int = 0) -> dict:
        return self.eng.zone_totals(stream, self.cfg.n_classes)

    def heatmap(self, stream: int = 0) -> np.ndarray:
        return self.eng.zone_heat(stream)

    def blend(self, device_frames, heat=None, maxes=None, alpha: Optional[int] = None, stream: int = 0, hip_stream=None):
        """Blend the heat over BGR frames on the device, in place: uint8 [B,H,W,3] or [H,W,3].  heat None: the stream's cumulative
        grid as it stands, for every frame; or a device tensor int32 [gh, gw] (one grid for all) or [B, gh, gw] (update_group_device's
        heat_frames) with maxes int32 [1] or [B]."""
        a = self.cfg.heat_alpha if alpha is None else int(alpha)
        if heat is None:
            h_addr, m_addr = self.eng.zone_heat_device(stream)
            return self.eng.zone_heat_blend(device_frames, h_addr, 0, m_addr, 0, a, hip_stream)
        if maxes is None:
            raise ValueError("blend: a heat tensor needs its maxes")
        per_frame = heat.dim() == 3 and heat.shape[0] > 1
        return self.eng.zone_heat_blend(device_frames, heat, heat.stride(0) if per_frame else 0, maxes, 1 if per_frame else 0, a, hip_stream)


def label_rows(results) -> np.ndarray:
    """rows_of with the corners as the labels file records them (int(): truncated towards zero), so that `replay` of the file a run
    wrote gives the run's own totals."""
    r = rows_of(results)
    r[:, :4] = np.trunc(r[:, :4])
    return r


def replay(rows, cfg: ZoneConfig, engine, frame_hw=None):
    """A finished labels array (gsi.py's rows [N, 8]: frame, id, x1, y1, x2, y2, conf, cls) through the same device call, as stream 0
    from frame 0 to the last frame (frames without rows count as empty frames; of more than 256 rows in a frame the first 256
    count).  -> (totals, heat grid or None).  It makes a state of its own on the engine's context and drops it: a live ZoneCounter
    there is replaced."""
    r = np.asarray(rows, np.float64).reshape(-1, 8)
    zc = ZoneCounter(cfg, engine, None, frame_hw)
    try:
        t, dev, S = zc._torch, zc.eng.device, zc.S
        n_frames = int(r[:, 0].max()) + 1 if len(r) else 0
        fr = r[:, 0].astype(np.int64)
        order = np.argsort(fr, kind="stable")
        starts = np.searchsorted(fr[order], np.arange(n_frames + 1))
        for g0 in range(0, n_frames, GROUP):
            F = min(GROUP, n_frames - g0)
            buf, cnt = np.zeros((F, S, ROWS, 8), np.float32), np.full((F, S), -1, np.int32)
            for f in range(F):
                q = r[order[starts[g0 + f]:starts[g0 + f + 1]]][:ROWS]
                buf[f, 0, :len(q), :4], buf[f, 0, :len(q), 4], buf[f, 0, :len(q), 5], buf[f, 0, :len(q), 6] = q[:, 2:6], q[:, 1], q[:, 7], q[:, 6]
                cnt[f, 0] = len(q)
            zc.update_group_device(t.from_numpy(buf).to(dev), t.from_numpy(cnt).to(dev), F, ())
        return zc.totals(0), (zc.heatmap(0) if cfg.heat else None)
    finally:
        zc.close()


def summary(totals: dict, cfg: ZoneConfig, names=None) -> dict:
    """The `<name>_zones.json` document: per line in / out and their split by class name, per zone entries, exits, peak occupancy and
    the mean and longest dwell (frames) of the stays that ended with an exit (mean null when there was none)."""
    names = names or {}
    lines = []
    for i, l in enumerate(cfg.lines):
        by = [{str(names.get(c, c)): int(n) for c, n in enumerate(totals["line_class"][i, d]) if n} for d in (0, 1)]
        lines.append({"line": [int(v) for v in l], "in": int(totals["line_totals"][i, 0]), "out": int(totals["line_totals"][i, 1]),
                      "in_by_class": by[0], "out_by_class": by[1]})
    zones = []
    for i, z in enumerate(cfg.zones):
        ex = int(totals["exits"][i])
        zones.append({"polygon": [[int(p[0]), int(p[1])] for p in z], "entries": int(totals["entries"][i]), "exits": ex,
                      "peak_occupancy": int(totals["peak"][i]), "mean_dwell": (int(totals["dwell_sum"][i]) / ex if ex else None),
                      "longest_dwell": int(totals["longest"][i])})
    return {"frames": int(totals["frames"]), "anchor": cfg.anchor, "max_gap": int(cfg.max_gap), "lines": lines, "zones": zones}


def write_summary(path: str, totals: dict, cfg: ZoneConfig, names=None) -> dict:
    doc = summary(totals, cfg, names)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc
