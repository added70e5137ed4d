"""Per-tile detection fields for the merge of sliced inference: a scene of boxes in frame pixels, seen by every tile that holds enough
of each (clipped to the tile, in tile pixels, a little jitter), as a per-tile NMS would leave them: descending score, a count.
Shared by tests/test_slice_cpu.py (which checks, on the reference alone, that the fields are not vacuous) and tests/test_gpu_slice.py."""
import numpy as np

from strongsort_yolo_amd import slicing
from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry

F = np.float32

# name -> (frame H, W, slice, overlap, full, rows per tile, candidate total): the totals at which k_slice_merge changes path (one wave up
# to 64, the LDS sort and workspace above; 1025 = more than one candidate per thread; 8192 = the cap, T = 64 x 128 rows)
CASES = {
    "n0": (96, 160, (64, 64), 0.25, True, 128, 0), "n1": (96, 160, (64, 64), 0.25, True, 128, 1),
    "n63": (96, 160, (64, 64), 0.25, True, 128, 63), "n64": (96, 160, (64, 64), 0.25, True, 128, 64),
    "n65": (96, 160, (64, 64), 0.25, True, 128, 65), "n1025": (96, 160, (64, 64), 0.25, True, 160, 1025),
    "n8192": (288, 288, (64, 64), 0.5, False, 128, 8192),
}


def setup(name, imgsz=64):
    """-> dict(H, W, cfg, g canvas geometry, table [T][8], T, R, total, tile_geom [T][5], frame_geom)."""
    H, W, hw, ov, full, R, total = CASES[name]
    cfg = slicing.SliceConfig(hw, ov, full)
    g, table = slicing.canvas(H, W, cfg, imgsz=imgsz)
    gf = letterbox_geometry(H, W, imgsz)
    return dict(H=H, W=W, cfg=cfg, g=g, table=table, T=len(table), R=R, total=total, tile_geom=slicing.nms_geometry(g, table),
                frame_geom=scale_geometry(gf, H, W))


def field(su, seed, n_extra=0, n_cls=3, min_side=4.0):
    """-> (tile_rows [T, R, 6 + n_extra] f32, counts [T] i32, appearances: per scene object the number of tiles that hold it).
    Exactly su["total"] candidates: the tiles' quotas are as even as the total allows."""
    rng = np.random.default_rng(seed)
    T, R, total, tab = su["T"], su["R"], su["total"], su["table"]
    quota = np.full(T, total // T, np.int64)
    quota[: total - quota.sum()] += 1
    assert quota.max() <= R
    per = [[] for _ in range(T)]
    seen = []
    guard = 0
    while any(len(per[t]) < quota[t] for t in range(T)):
        guard += 1
        assert guard < 400000
        w, h = rng.uniform(8, 40), rng.uniform(8, 40)
        short = [t for t in range(T) if len(per[t]) < quota[t]]
        t0 = short[int(rng.integers(len(short)))]                      # centred in a tile that still has room, so the loop ends
        cx, cy = tab[t0][0] + rng.uniform(0, tab[t0][2]), tab[t0][1] + rng.uniform(0, tab[t0][3])
        x1, y1, x2, y2 = max(cx - w / 2, 0), max(cy - h / 2, 0), min(cx + w / 2, su["W"]), min(cy + h / 2, su["H"])
        score, cl = rng.uniform(0.3, 0.95), int(rng.integers(n_cls))
        same_score = rng.random() < 0.5                               # half the objects carry one score into every tile: ties across tiles
        hit = 0
        for t in range(T):
            tx, ty, tw, th = (int(v) for v in tab[t][:4])
            bx1, by1, bx2, by2 = max(x1, tx), max(y1, ty), min(x2, tx + tw), min(y2, ty + th)
            if bx2 - bx1 < min_side or by2 - by1 < min_side or len(per[t]) >= quota[t]:
                continue
            j = rng.uniform(-0.75, 0.75, 4)
            b = np.clip([bx1 - tx + j[0], by1 - ty + j[1], bx2 - tx + j[2], by2 - ty + j[3]], 0, [tw, th, tw, th])
            s = score if same_score else score + rng.uniform(-0.04, 0.04)
            per[t].append(np.concatenate([b, [s, cl], rng.uniform(0, 64, n_extra)]).astype(F))
            hit += 1
        if hit:
            seen.append(hit)
    rows = np.zeros((T, R, 6 + n_extra), F)
    counts = np.zeros(T, np.int32)
    for t in range(T):
        if per[t]:
            p = np.stack(per[t])
            p = p[np.argsort(-p[:, 4], kind="stable")]
            rows[t, :len(p)] = p
            counts[t] = len(p)
    rows[:, :, 4][np.arange(R)[None, :] >= counts[:, None]] = rng.uniform(0.96, 0.99)     # stale rows past the count: must never be read as candidates
    return rows, counts, np.asarray(seen)
