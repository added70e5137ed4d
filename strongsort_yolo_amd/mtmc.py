"""Identities across cameras (docs/MTMC.md): a bank of one pooled appearance descriptor per track id, kept on the device while a
tracker runs, and the linking of several cameras' banks into global ids after the run, on the device (csrc/ss_mtmc.hip).
tests/mtmc_ref.py is the definition; the device gives its bits.  There is no CPU fallback: without the library or a device the
device calls raise as the rest of the package does.

    bank = TrackBank(engine)                                  # one table per stream of the engine's context
    bank.update_group_device(out, nout, feats, n_frames)      # a tracker's rows and the features it read, where they are
    tables = [bank.table(0), load_table("cam_b_bank.npz")]
    maps = link(tables, engine)                               # [{local id: global id}, ...]
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional

import numpy as np

from .config import FEAT_DIM, StrongSortConfig

ROWS, DETS, GROUP = 256, 128, 32
KEYS = ("ids", "n", "first", "last", "cls", "desc")
THR = StrongSortConfig.max_dist                              # the project's own cosine threshold
# the models that have features to pool (YOLO(track_bank=True), --mtmc)
NO_FEATURES = "no appearance features to pool: use tracker_type 'strongsort', 'deep_ocsort', or 'botsort' with with_reid=True and reid_model='osnet'"


def bank_refusal(tracker_type: str, with_reid: bool = False, reid_model: str = "osnet", obb: bool = False) -> Optional[str]:
    """Why a model of this kind cannot keep a track bank (None: it can)."""
    if obb:
        return f"an oriented-box model has {NO_FEATURES}"
    if tracker_type in ("bytetrack", "ocsort", "hybridsort"):
        return f"tracker_type {tracker_type!r} has {NO_FEATURES}"
    if tracker_type == "botsort" and not with_reid:
        return f"tracker_type 'botsort' without with_reid has {NO_FEATURES}"
    if reid_model == "auto":
        return f"reid_model='auto' reads the detector's own features, not OSNet's 512: {NO_FEATURES}"
    return None


class TrackBank:
    """The bank of an engine's context: per stream and track id the f64 sum of the unit features of the id's rows, their count,
    first and last frame and last class.  `engine`: a TrackerEngine or any tracker engine on one.  A context holds one bank: a
    second TrackBank on the same engine replaces the first."""

    def __init__(self, engine, max_ids: int = 4096):
        import torch
        self.eng = getattr(engine, "base", engine)
        self.S, self.max_ids, self._torch = self.eng.S, int(max_ids), torch
        self.eng.bank_create(self.max_ids)

    def close(self):
        if getattr(self.eng, "ctx", None) and self.eng.ctx.value:
            self.eng.bank_destroy()

    def reset(self, stream: int = -1):
        self.eng.bank_reset(stream)

    def update_group_device(self, d_rows, d_nrows, d_feats, n_frames: int):
        """A tracker's rows where they are: d_rows [F,S,256,8] f32, d_nrows [F,S] i32 and d_feats [F,S,128,512] f32 (the raw
        features that tracker call read) on the device, read in place, ONE launch, no copy.  Asynchronous on the engine's stream."""
        t, S = self._torch, self.S
        if not 1 <= int(n_frames) <= GROUP:
            raise ValueError(f"update_group_device: 1 <= n_frames <= {GROUP}")
        for v, tail, dt, what in ((d_rows, (ROWS, 8), t.float32, "rows float32 [F, S, 256, 8]"), (d_nrows, (), t.int32, "counts int32 [F, S]"),
                                  (d_feats, (DETS, FEAT_DIM), t.float32, "features float32 [F, S, 128, 512]")):
            if v.dtype != dt or not v.is_contiguous() or v.numel() < int(n_frames) * S * int(np.prod(tail, dtype=np.int64)) or v.numel() % (S * int(np.prod(tail, dtype=np.int64))):
                raise ValueError(f"update_group_device: {what}, contiguous, S = {S}")
        self.eng.bank_update_group(int(n_frames), d_rows, d_nrows, d_feats)

    def table(self, stream: int = 0) -> Dict[str, np.ndarray]:
        """Synchronous: ids, n, first, last, cls int32 [m] in rising id order and desc float32 [m, 512] (unit rows)."""
        return self.eng.bank_get(stream)


def save_table(path: str, table: dict):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:                              # (a file object: np.savez would add ".npz" to a path without it)
        np.savez(f, **{k: np.asarray(table[k]) for k in KEYS})


def load_table(path: str) -> Dict[str, np.ndarray]:
    with np.load(path) as z:
        t = {k: z[k] for k in KEYS}
    m = len(t["ids"])
    if t["desc"].shape != (m, FEAT_DIM) or any(t[k].shape != (m,) for k in KEYS[:5]):
        raise ValueError(f"{path}: not a track-bank table")
    return t


def tracklets(tables):
    """The cameras' tables as one list in rising (camera index, local id) order -> desc [T, 512], cam, ids, first, last, n [T]."""
    for c, t in enumerate(tables):
        ids = np.asarray(t["ids"])
        if len(ids) > 1 and not (np.diff(ids) > 0).all():
            raise ValueError(f"table {c}: ids must rise")
    cat = lambda k, dt: np.concatenate([np.asarray(t[k], dt).reshape(-1) for t in tables])
    cam = np.concatenate([np.full(len(t["ids"]), c, np.int32) for c, t in enumerate(tables)])
    desc = np.concatenate([np.asarray(t["desc"], np.float32).reshape(-1, FEAT_DIM) for t in tables])
    return desc, cam, cat("ids", np.int32), cat("first", np.int32), cat("last", np.int32), cat("n", np.int32)


def link(tables, engine, thr: float = THR, min_rows: int = 1, info: Optional[dict] = None) -> List[Dict[int, int]]:
    """The tables of C >= 2 cameras -> one {local id: global id} dict per camera, global ids 1.. in rising order of each cluster's
    smallest tracklet.  Two tracklets of one camera whose [first, last] overlap never share a global id, a tracklet with fewer than
    min_rows rows stays alone, and clusters merge by average linkage while the smallest distance is below thr (docs/MTMC.md).
    info, when given, receives tracklets, clusters, merges [(a, b, height)], cam, ids and (with info["want_dist"]) dist."""
    if len(tables) < 2:
        raise ValueError("link: the tables of at least two cameras")
    desc, cam, ids, first, last, n = tracklets(tables)
    eng = getattr(engine, "base", engine)
    want = bool(info and info.get("want_dist"))
    if len(cam) == 0:
        gid, merges, dist = np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 0), np.float32)
    else:
        out = eng.mtmc_link(desc, cam, first, last, n, thr, min_rows, want_dist=want)
        gid, merges, dist = out[0], out[1], (out[2] if want else None)
    if info is not None:
        info.update(tracklets=int(len(cam)), clusters=int(gid.max()) if len(gid) else 0, cam=cam, ids=ids, global_id=gid,
                    merges=[(int(a), int(b), float(h)) for a, b, h in merges], thr=float(thr), min_rows=int(min_rows))
        if want:
            info["dist"] = dist
    return [{int(i): int(g) for i, g in zip(ids[cam == c], gid[cam == c])} for c in range(len(tables))]


def relabel(rows: np.ndarray, mapping: Dict[int, int]) -> np.ndarray:
    """Label rows [N, 8] (frame, id, x1, y1, x2, y2, conf, cls: moteval.read_labels, gsi.rows_of) -> a copy with the ids replaced
    through one camera's mapping; an id the mapping lacks is a KeyError."""
    out = np.array(rows, np.float64, copy=True).reshape(-1, 8)
    if len(out):
        out[:, 1] = [mapping[int(i)] for i in out[:, 1]]
    return out


def concat(rows_per_camera) -> np.ndarray:
    """Label rows [n, 8] (frame first, as moteval.read_labels gives them) of several cameras as one sequence: each
    camera's frame numbers are offset past the previous camera's last frame, so that moteval.evaluate(..., identity=True) scores
    global ids as cross-camera IDF1."""
    out, base = [], 0
    for r in rows_per_camera:
        r = np.array(r, np.float64, copy=True).reshape(-1, 8)
        if len(r):
            r[:, 0] += base - r[:, 0].min()
            base = int(r[:, 0].max()) + 1
        out.append(r)
    return np.concatenate(out, 0) if out else np.zeros((0, 8))


def rewrite_labels(src: str, dst: str, mapping: Dict[int, int]) -> int:
    """The labels file `src` with the id column (the third) replaced through `mapping`, every other byte kept -> lines written.
    An id without a global id (a track that never had a feature) keeps its line with id 0."""
    n = 0
    with open(src, "r", newline="") as f, open(dst, "w", newline="") as g:
        for line in f:
            p = line.split(" ")
            if len(p) >= 3:
                p[2] = str(mapping.get(int(p[2]), 0))
                n += 1
            g.write(" ".join(p))
    return n


def write_summary(path: str, sources, tables, mappings, info: dict) -> dict:
    """mtmc.json: the cameras, tracklets, clusters, merges and thresholds, and per global id its (source, local id) members."""
    members: Dict[int, list] = {}
    for c, m in enumerate(mappings):
        for lid, g in sorted(m.items()):
            members.setdefault(g, []).append([str(sources[c]), int(lid)])
    s = {"cameras": [str(x) for x in sources], "tracklets": [int(len(t["ids"])) for t in tables], "clusters": len(members),
         "thr": float(info.get("thr", THR)), "min_rows": int(info.get("min_rows", 1)),
         "merges": [[int(a), int(b), float(h)] for a, b, h in info.get("merges", [])],
         "global_ids": {str(g): v for g, v in sorted(members.items())}}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(s, f, indent=1)
    return s
