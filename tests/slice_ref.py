"""Reference of the cross-tile merge of sliced inference (docs/SLICE.md), in plain NumPy: every arithmetic step is one np.float32
operation, in the order the document gives.  The library is built with -ffp-contract=off and correctly rounded f32 division, so
csrc/ss_slice.hip must give these bits.  `sahi` itself is not a dependency: the semantics are this project's definition, restated from
SAHI's published behaviour (NMS / GREEDYNMM post-processing, IOU / IOS match metrics).

merge(): one frame.  Candidates are the rows r < min(max(count_t, 0), R) of every tile, corners shifted by the tile's origin; order =
ascending key (~score bits, tile * R + row), i.e. score descending, ties by tile then row, for the positive scores an NMS produces.
"""
import numpy as np

F = np.float32


def _metric(b, ab, B, aB, ios):
    """metric of box b (area ab) against the boxes B [m, 4] (areas aB); inter as k_nms_mask computes it."""
    xx1, yy1 = np.fmax(b[0], B[:, 0]), np.fmax(b[1], B[:, 1])
    xx2, yy2 = np.fmin(b[2], B[:, 2]), np.fmin(b[3], B[:, 3])
    iw, ih = np.fmax(F(0), xx2 - xx1), np.fmax(F(0), yy2 - yy1)
    inter = iw * ih
    with np.errstate(all="ignore"):
        return inter / np.fmin(ab, aB) if ios else inter / (ab + aB - inter)


def candidates(tile_rows, counts, origins, R):
    """-> (order keys' source indices [n] in candidate order, boxes [n, 4] f32 in frame pixels)."""
    tile_rows = np.asarray(tile_rows, F)
    T = tile_rows.shape[0]
    src, score = [], []
    for t in range(T):
        for r in range(min(max(int(counts[t]), 0), R)):
            src.append(t * R + r)
            score.append(tile_rows[t, r, 4])
    src = np.asarray(src, np.int64)
    bits = np.asarray(score, F).view(np.uint32).astype(np.uint64)
    keys = ((~bits & np.uint64(0xffffffff)) << np.uint64(32)) | src.astype(np.uint64)
    src = src[np.argsort(keys, kind="stable")]
    t, r = src // R, src % R
    org = np.asarray(origins, np.int64).reshape(T, 2)
    box = tile_rows[t, r, :4].copy() if len(src) else np.zeros((0, 4), F)
    ox, oy = org[t, 0].astype(F), org[t, 1].astype(F)
    box[:, 0] = box[:, 0] + ox
    box[:, 1] = box[:, 1] + oy
    box[:, 2] = box[:, 2] + ox
    box[:, 3] = box[:, 3] + oy
    return src, box


def merge(tile_rows, counts, origins, R, mode="nmm", metric="ios", thr=0.5, agnostic=False, out_cap=1024, n_kpt=0, tile_geom=None,
          frame_geom=None, want_stats=False):
    """tile_rows [T, >=R, ld] f32 (x1, y1, x2, y2 in tile pixels, score, class, extras), counts [T], origins [T][2] = (x0, y0).
    tile_geom [T][>=3] = (gain, pad_x, pad_y) of every tile's NMS, frame_geom = (gain, pad_x, pad_y) of the whole frame's letterbox
    (read when n_kpt > 0).  -> rows [m, ld] f32, m, source indices [m] (tile * R + row)."""
    tile_rows = np.asarray(tile_rows, F)
    ld, ios, thr = tile_rows.shape[2], metric == "ios", F(thr)
    src, box = candidates(tile_rows, counts, origins, R)
    n = len(src)
    t_of, r_of = src // R, src % R
    cls = tile_rows[t_of, r_of, 5] if n else np.zeros(0, F)
    area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
    removed, owner, kept = np.zeros(n, bool), np.full(n, -1, np.int64), []
    for i in range(n):
        if removed[i]:
            continue
        kept.append(i)
        m = _metric(box[i], area[i], box[i + 1:], area[i + 1:], ios) >= thr          # a NaN metric compares false
        if not agnostic:
            m &= cls[i + 1:] == cls[i]
        new = m & ~removed[i + 1:]
        owner[i + 1:][new] = i
        removed[i + 1:] |= m
    kept = kept[:out_cap]
    out = np.zeros((len(kept), ld), F)
    rechecks = 0                                                   # unions that the re-check against the GROWN box alone admits or refuses
    for kk, i in enumerate(kept):
        cur = box[i].copy()
        if mode == "nmm":
            for j in np.nonzero(owner == i)[0]:
                ac = (cur[2] - cur[0]) * (cur[3] - cur[1])
                hit = bool(_metric(cur, ac, box[j:j + 1], area[j:j + 1], ios)[0] > thr)
                if hit != bool(_metric(box[i], area[i], box[j:j + 1], area[j:j + 1], ios)[0] > thr):
                    rechecks += 1
                if hit:
                    cur = np.array([np.fmin(cur[0], box[j, 0]), np.fmin(cur[1], box[j, 1]), np.fmax(cur[2], box[j, 2]), np.fmax(cur[3], box[j, 3])], F)
        t, r = int(t_of[i]), int(r_of[i])
        out[kk] = tile_rows[t, r]
        out[kk, :4] = cur
        if n_kpt:
            gt, (gF, pxF, pyF) = np.asarray(tile_geom, F)[t], [F(v) for v in frame_geom]
            ox, oy = F(int(origins[t][0])), F(int(origins[t][1]))
            for q in range(n_kpt):
                out[kk, 6 + 3 * q] = ((tile_rows[t, r, 6 + 3 * q] - gt[1]) / gt[0] + ox) * gF + pxF
                out[kk, 7 + 3 * q] = ((tile_rows[t, r, 7 + 3 * q] - gt[2]) / gt[0] + oy) * gF + pyF
    res = (out, len(kept), src[kept].astype(np.int32) if kept else np.zeros(0, np.int32))
    return res + (dict(candidates=n, rechecks=rechecks),) if want_stats else res
