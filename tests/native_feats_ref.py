"""docs/BYTETRACK.md §1d (decisions N-01..N-04) in NumPy: BoT-SORT's `model: auto` raw feature of a kept detection, read from
the detector's head inputs at its anchor.  Also Ultralytics' own `get_obj_feats` expression in torch (restated from
Ultralytics 8.3.x), which the restatement is checked against.

    s = min(C_l) (or given), g_l = C_l / s;  raw[j] = (m[j*g] + m[j*g+1] + ... + m[j*g+g-1]) / (float)g   for j < s
    (f32: every element converted exactly, added in ascending channel order from the first term, correctly rounded divide)
    raw[s..512) = 0 (N-03);  anchors level by level (P3, P4, P5), row-major inside a level (the order of the NMS keep list)."""
import numpy as np

FEAT_DIM, MAX_DETS = 512, 128


def _np(x):
    import torch
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def anchor_pixel(shapes, a):
    """shapes: [(H_l, W_l)] of the three levels -> (level, y, x) of anchor index a."""
    for lv, (h, w) in enumerate(shapes):
        if a < h * w:
            return lv, a // w, a % w
        a -= h * w
    raise IndexError("anchor outside the maps")


def native_row(maps, b, a, s=None):
    """The §1d feature [512] f32 of image b's anchor a; maps: three arrays [B, C_l, H_l, W_l] (f16 or f32)."""
    maps = [_np(m) for m in maps]
    s = min(m.shape[1] for m in maps) if s is None else int(s)
    if s > FEAT_DIM or any(m.shape[1] % s for m in maps):
        raise ValueError("s <= 512 and C_l % s == 0 (N-03)")
    lv, y, x = anchor_pixel([m.shape[2:] for m in maps], int(a))
    m = maps[lv]
    g = m.shape[1] // s
    v = m[b, :, y, x].astype(np.float32).reshape(s, g)          # exact conversion of every element (f16 -> f32 is exact)
    acc = v[:, 0].copy()
    for k in range(1, g):                                       # ascending channel order from the first term, f32 adds
        acc = (acc + v[:, k]).astype(np.float32)
    out = np.zeros(FEAT_DIM, np.float32)
    out[:s] = acc / np.float32(g)                               # IEEE (correctly rounded) f32 divide
    return out


def native_feats(maps, keep, counts, s=None, out=None):
    """-> out [B, 128, 512] f32: rows r < min(count, 128) written, the others left as they are (zeros for a new array)."""
    maps, keep, counts = [_np(m) for m in maps], _np(keep), _np(counts)
    B = keep.shape[0]
    out = np.zeros((B, MAX_DETS, FEAT_DIM), np.float32) if out is None else out
    for b in range(B):
        for r in range(min(max(int(counts[b]), 0), MAX_DETS)):
            out[b, r] = native_row(maps, b, int(keep[b, r]), s)
    return out


def ultralytics_obj_feats(feat_maps, idxs):
    """Ultralytics' get_obj_feats (8.3.x, by recall): the rows at the kept anchors of every image, in the map's dtype."""
    import torch
    s = min(x.shape[1] for x in feat_maps)
    obj_feats = torch.cat([x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, s, x.shape[1] // s).mean(dim=-1) for x in feat_maps], dim=1)
    return [feats[idx] for feats, idx in zip(obj_feats, idxs)]
