"""Crowded scenes for the BYTE tracker family (docs/BYTETRACK.md §5): seeded NumPy generators whose frames push the three
associations of csrc/ss_byte.hip past 64 rows, past the LDS-resident cost matrix (SS_BYTE_COST_CAP = 2048 entries) and through
the transposed (more tracks than rows) orientation (two_crowds, three_crowds, boundary_pair), or make SciPy's tie order show in
the rows (dense_crowd, twin_crowds); the side inputs of the GMC / ReID / pose variants; and the CPU references' run of a scene
with the shape of every linear_sum_assignment call recorded.

Not a conftest and not a test module: imported by tests/test_byte_crowd_cpu.py and tests/test_gpu_byte_crowd.py.

    frames, ids = two_crowds(0, ids=True)        # frames: [N,6] float32 x1,y1,x2,y2,score,cls; ids: the lattice cell of every row
    run = reference("two_crowds", "reid")        # cached: .rows per frame, .ref (the reference after the last frame), .calls
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from strongsort_yolo_amd.config import ByteTrackConfig

COST_CAP = 2048                                   # SS_BYTE_COST_CAP: f64 cost entries that stay in LDS
VARIANTS = ("xyah", "xywh", "gmc", "reid", "pose")
# (n_tracks, n_rows) of boundary_pair: the last LDS-resident size, the first spilled ones, the 64-column edge of the solver's forms
# in both orientations, and the 128 edge
BOUNDARY_SIZES = ((32, 64), (33, 64), (64, 33), (45, 46), (64, 64), (65, 64), (64, 65), (127, 128), (128, 127), (128, 128))
SPILL_EDGE_SIZES = BOUNDARY_SIZES[:4]


def _lattice(nx, ny, px, py, ox=0.0, oy=0.0, n=None):
    gx, gy = np.meshgrid(np.arange(nx) * px + ox + 20.0, np.arange(ny) * py + oy + 20.0)
    return np.stack([gx.reshape(-1), gy.reshape(-1)], 1)[:n]


def _rows(xy, w, h, score):
    return np.column_stack([xy, xy + (w, h), score, np.zeros(len(xy))]).astype(np.float32)


def _crowds(rng, lattices, n_frames, turn, low_share, w=44.0, h=30.0):
    """The lattices shown in turn, `turn` frames each, rows permuted; ids: lattice index * len + cell."""
    n = len(lattices[0])
    frames, ids = [], []
    for f in range(n_frames):
        c = (f // turn) % len(lattices)
        xy = lattices[c] + rng.normal(0.0, 1.5, (n, 2))
        sc = rng.uniform(0.7, 0.95, n)
        if f % turn == turn - 1:                               # the turn's last frame: a share of the rows scores low
            low = rng.random(n) < low_share
            sc[low] = rng.uniform(0.12, 0.24, int(low.sum()))
        p = rng.permutation(n)
        frames.append(_rows(xy, w, h, sc)[p])
        ids.append(c * n + p)
    return frames, ids


def two_crowds(seed, n_frames=24, n=120, turn=3, low_share=0.5, ids=False):
    """Two interleaved lattices of n boxes (12 columns, pitch 100 x 70; B is A shifted by half a pitch; boxes 44 x 30, 1.5 px
    jitter: A and B never overlap), A for `turn` frames, then B, and so on.  While B is seen A is lost but kept: the pool is 2n
    tracks against n (or, on a turn's last frame, about n / 2) high rows — tall, spilled, 256-column solver form; B's first frame
    gives n unconfirmed x n left-over rows in the third association, the low-score frames a second association of about
    n / 2 x n / 2.  Every cost matrix between the crowds is the plateau 1.0."""
    a = _lattice(12, -(-n // 12), 100.0, 70.0, n=n)
    out = _crowds(np.random.default_rng(11000 + seed), [a, a + (50.0, 35.0)], n_frames, turn, low_share)
    return out if ids else out[0]


def three_crowds(seed, n_frames=12, n=100, turn=3, ids=False):
    """Three disjoint lattices of n boxes, `turn` frames each, then the first again: the third crowd pushes tracked + lost past
    max_tracks = 256 (births cut off, SS_ERR_CAPACITY), and the first crowd's return meets a pool of 256 tracks."""
    a = _lattice(10, -(-n // 10), 160.0, 70.0, n=n)
    out = _crowds(np.random.default_rng(12000 + seed), [a, a + (53.0, 35.0), a + (106.0, 0.0)], n_frames, turn, 0.0)
    return out if ids else out[0]


def twin_crowds(seed, n=120, ids=False):
    """two_crowds' lattices over six frames A*, B, B, A, A, B, where A* is A with eight rows duplicated exactly: both copies become
    tracks on frame 1 and are lost together, so they stay exact twins until A returns on frame 4.  That first association has
    2n + 8 pool tracks (transposed: the 256-column solver form, spilled) with eight pairs of exactly tied columns whose shared entry
    lies below match_thresh: SciPy's tie order decides which twin carries on, and the rows show its id."""
    rng = np.random.default_rng(18000 + seed)
    a = _lattice(12, -(-n // 12), 100.0, 70.0, n=n)
    frames, idl = [], []
    for f, c in enumerate((0, 1, 1, 0, 0, 1)):
        d, who = _rows((a, a + (50.0, 35.0))[c] + rng.normal(0.0, 1.5, (n, 2)), 44.0, 30.0, rng.uniform(0.7, 0.95, n)), c * n + np.arange(n)
        if f == 0:
            dup = rng.choice(n, 8, replace=False)
            d, who = np.concatenate([d, d[dup]]), np.concatenate([who, who[dup]])
        p = rng.permutation(len(d))
        frames.append(np.ascontiguousarray(d[p]))
        idl.append(who[p])
    return (frames, idl) if ids else frames


def dense_crowd(seed, n_frames=20, n=100, ids=False):
    """n people on a 20-column lattice whose columns, 30 px apart, are closer than a box is wide (44 x 100): every box overlaps its
    neighbours, so every cost row has several entries below 1.  They drift 4 px a frame with 3 px jitter; a quarter of the scores
    are low, a tenth of the sightings are dropped, and every fourth frame eight high rows are duplicated exactly (tied columns)."""
    rng = np.random.default_rng(13000 + seed)
    base = _lattice(20, -(-n // 20), 30.0, 130.0, n=n)
    frames, idl = [], []
    for f in range(n_frames):
        xy = base + (4.0 * f, 0.0) + rng.normal(0.0, 3.0, (n, 2))
        sc = rng.uniform(0.5, 0.95, n)
        low = rng.random(n) < 0.25
        sc[low] = rng.uniform(0.12, 0.24, int(low.sum()))
        keep = rng.random(n) >= 0.1
        d, who = _rows(xy, 44.0, 100.0, sc)[keep], np.arange(n)[keep]
        if f % 4 == 3:
            dup = rng.choice(np.nonzero(d[:, 4] >= 0.25)[0], 8, replace=False)
            d, who = np.concatenate([d, d[dup]]), np.concatenate([who, who[dup]])
        p = rng.permutation(len(d))
        frames.append(np.ascontiguousarray(d[p]))
        idl.append(who[p])
    return (frames, idl) if ids else frames


def boundary_pair(n_tracks, n_rows, ids=False):
    """Two frames: n_tracks separated boxes (all activate on frame 1), then n_rows high-score boxes over the first
    min(n_tracks, n_rows) of them, slightly moved, the others on cells of their own: a first association of exactly
    n_tracks x n_rows."""
    rng = np.random.default_rng(14000 + 131 * n_tracks + n_rows)
    cells = _lattice(16, 8, 70.0, 50.0)
    f1 = _rows(cells[:n_tracks], 44.0, 30.0, rng.uniform(0.5, 0.95, n_tracks))
    p = rng.permutation(n_rows)
    f2 = _rows(cells[:n_rows] + rng.normal(0.0, 1.5, (n_rows, 2)), 44.0, 30.0, rng.uniform(0.5, 0.95, n_rows))[p]
    out = [f1, f2], [np.arange(n_tracks), p]
    return out if ids else out[0]


# ---- side inputs of the variants ------------------------------------------------------------------------------------------
def _first_copy(d):
    """Per row the index of the first row with the same bytes (itself unless the row is an exact duplicate)."""
    seen, out = {}, []
    for i in range(len(d)):
        out.append(seen.setdefault(d[i].tobytes(), i))
    return out


def features(seed, frames, ids, noise=0.05):
    """Raw features [N,512] f32 per frame: a fixed unit vector per lattice cell plus `noise` Gaussian noise, at a random scale;
    an exactly duplicated row carries its original's feature."""
    base = np.random.default_rng(15000 + seed).standard_normal((int(max(i.max() for i in ids)) + 1, 512))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    rng, out = np.random.default_rng(15500 + seed), []
    for d, who in zip(frames, ids):
        f = ((base[who] + noise * rng.standard_normal((len(d), 512))) * rng.uniform(0.5, 3.0, (len(d), 1))).astype(np.float32)
        out.append(np.ascontiguousarray(f[_first_copy(d)]))
    return out


def keypoints(seed, frames, ids):
    """Keypoints [N,17,3] f32 per frame: every lattice cell's own skeleton on its box (tests/test_botsort_pose_cpu.skeleton /
    place); an exactly duplicated row carries its original's keypoints."""
    from tests.test_botsort_pose_cpu import K, place, skeleton
    sks, rng, out = {}, np.random.default_rng(16500 + seed), []
    for d, who in zip(frames, ids):
        kp = np.zeros((len(d), K, 3), np.float32)
        for i, c in enumerate(who):
            if int(c) not in sks:
                sks[int(c)] = skeleton(np.random.default_rng(16000 + 1009 * seed + int(c)))
            kp[i] = place(sks[int(c)], d[i, :4].astype(np.float64), rng)
        out.append(np.ascontiguousarray(kp[_first_copy(d)]))
    return out


def camera(seed, frames):
    """A moving camera over the scene: seeded warps [F,8] (ss_cmc_estimate's layout: rotation up to 0.01 rad, a shift of up to
    4 px, every fifth frame none, w6 = -1) and the frames with every box centre moved by the accumulated warp, the sizes kept.
    -> (warps float64 [F,8], moved frames)"""
    F = len(frames)
    rng = np.random.default_rng(17000 + seed)
    th = rng.uniform(-0.01, 0.01, F)
    w = np.zeros((F, 8))
    w[:, 0], w[:, 1], w[:, 3], w[:, 4] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    w[:, 2], w[:, 5] = rng.uniform(-4.0, 4.0, F), rng.uniform(-4.0, 4.0, F)
    w[:, 6] = rng.integers(1, 60, F)
    w[::5, 6] = -1.0
    A, t, moved = np.eye(2), np.zeros(2), []
    for k, d in enumerate(frames):
        if w[k, 6] >= 0:
            R = np.array([[w[k, 0], w[k, 1]], [w[k, 3], w[k, 4]]])
            A, t = R @ A, R @ t + (w[k, 2], w[k, 5])
        d64 = d.astype(np.float64)
        c, half = (d64[:, :2] + d64[:, 2:4]) / 2 @ A.T + t, (d64[:, 2:4] - d64[:, :2]) / 2
        moved.append(np.column_stack([c - half, c + half, d64[:, 4:]]).astype(np.float32))
    return w, moved


# ---- a scene on a variant, and the reference's run of it --------------------------------------------------------------------
def config(variant, **kw):
    return ByteTrackConfig(kalman="xyah" if variant == "xyah" else "xywh", with_reid=variant == "reid", with_pose=variant == "pose", **kw)


@functools.lru_cache(maxsize=None)
def scene(name, variant, seed=0, size=None, n_frames=None):
    """name: "two_crowds", "twin_crowds", "dense_crowd", "three_crowds" (n_frames: other than the generator's default) or "boundary_pair"
    (size = (n_tracks, n_rows)).
    -> namespace: cfg, frames (list of [N,6] f32), side (per frame the features / keypoints, or None), warps ([F,8] or None)."""
    if name == "boundary_pair":
        frames, ids = boundary_pair(*size, ids=True)
    else:
        kw = {} if n_frames is None else {"n_frames": n_frames}
        frames, ids = {"two_crowds": two_crowds, "dense_crowd": dense_crowd, "three_crowds": three_crowds, "twin_crowds": twin_crowds}[name](seed, ids=True, **kw)
    warps = side = None
    if variant == "gmc":
        warps, frames = camera(seed, frames)
    elif variant == "reid":
        side = features(seed, frames, ids)
    elif variant == "pose":
        side = keypoints(seed, frames, ids)
    return SimpleNamespace(name=name, variant=variant, cfg=config(variant), frames=frames, side=side, warps=warps)


def new_reference(variant, cfg):
    from tests.botsort_gmc_ref import BotSortGmcRef
    from tests.botsort_pose_ref import BotSortPoseRef
    from tests.botsort_reid_ref import BotSortReidRef
    from tests.bytetrack_ref import ByteTrackRef
    return {"xyah": ByteTrackRef, "xywh": ByteTrackRef, "gmc": BotSortGmcRef, "reid": BotSortReidRef, "pose": BotSortPoseRef}[variant](cfg)


def _tied(cost):
    """Rows of cost that repeat an earlier row exactly and hold an entry below 1.0 (rows off the plateau)."""
    off = cost[(cost < 1.0).any(1)]
    return len(off) - len(np.unique(off, axis=0))


@functools.lru_cache(maxsize=None)
def reference(name, variant, seed=0, size=None, n_frames=None):
    """The variant's CPU reference over the scene, computed once per process and shared (callers do not modify it).
    -> namespace: scene, ref (the reference object after the last frame), rows (per frame), calls: one (frame, stage, n_rows, n_cols,
    entries below 1.0, tied rows, tied columns) per linear_sum_assignment call, stage 0 / 1 / 2 = first / second / third association;
    a tied row (column) repeats an earlier one exactly and has an entry below 1.0.  The three botsort
    references reach SciPy through tests.bytetrack_ref.assign, so the name is patched there, where it is imported."""
    import tests.bytetrack_ref as bt
    sc = scene(name, variant, seed, size, n_frames)
    ref = new_reference(variant, sc.cfg)
    calls, state = [], {"frame": 0, "n": 0, "stage": 0}
    lsa, assign = bt.linear_sum_assignment, bt.assign

    def counted_assign(cost, thresh):                           # ByteTrackRef.update: one call per stage, empty matrices included
        state["stage"], state["n"] = state["n"] % 3, state["n"] + 1
        return assign(cost, thresh)

    def recorded_lsa(cost, *a, **kw):
        calls.append((state["frame"], state["stage"], cost.shape[0], cost.shape[1], int((cost < 1.0).sum()), _tied(cost), _tied(cost.T)))
        return lsa(cost, *a, **kw)

    bt.linear_sum_assignment, bt.assign = recorded_lsa, counted_assign
    try:
        rows = []
        for k, d in enumerate(sc.frames):
            state["frame"] = k
            if variant == "gmc":
                rows.append(ref.update(d, sc.warps[k]))
            elif variant in ("reid", "pose"):
                rows.append(ref.update(d, sc.side[k]))
            else:
                rows.append(ref.update(d))
    finally:
        bt.linear_sum_assignment, bt.assign = lsa, assign
    assert state["n"] == 3 * len(sc.frames), "ByteTrackRef.update no longer calls assign once per stage"
    return SimpleNamespace(scene=sc, ref=ref, rows=rows, calls=calls)
