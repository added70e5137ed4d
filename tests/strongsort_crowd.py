"""Crowded scenes for the StrongSORT chain (csrc/ss_track.hip: k_assoc, k_newrow, k_frame, k_post / k_postnew): seeded NumPy generators
whose frames fill the upper half of the track table (129 - 256 of SS_MAXT = 256 slots, 128 = SS_MAXD detections a frame), make both
stages of k_frame run the one-wave LSAP (ambiguous costs: twins) in each of its forms and orientations, on a cost matrix that is
resident in LDS or read back from the stream's cost_spill (more than COST_CAP entries), and reuse slots freed in the frame of the
births; and the oracle's cached run of a scene with, per frame and stage, the natural shape and whether the LSAP must run.

Not a conftest and not a test module: imported by tests/test_strongsort_crowd_cpu.py and tests/test_gpu_strongsort_crowd.py.

    frames = two_crowds(0)                        # list of (dets [N,6] float32 x1,y1,x2,y2,score,cls; feats [N,512] float32 unit rows)
    run = reference("two_crowds", 0)              # cached: .rows / .lasts / .stages / .n_tracks per frame, .orc (the oracle afterwards)

Every lattice cell owns a prototype feature; a sighting is the prototype plus 0.02 Gaussian noise, renormalised (synth.py).
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from strongsort_yolo_amd.config import StrongSortConfig

W, H = 1920, 1080
MAX_TRACKS, MAX_DETS = 256, 128                   # SS_MAXT, SS_MAXD
COST_CAP = 12288                                  # SS_COST_CAP: f64 cost entries that stay in LDS (more: the stream's cost_spill)
# (n_a + n_b, d) of edge_scene, from ss_lsap.h's lsap_wave (larger side <= 64: lsap_wave_small, <= 128: lsap_wave_regs<2>, <= 256:
# lsap_wave_regs<4>; more tracks than detections: transposed) and k_frame's `big` (nC * D > COST_CAP): the last resident and the first
# spilled size, the form edges in both orientations, the largest size, a small row side against the widest form
EDGE_SIZES = ((96, 128), (97, 128), (64, 64), (64, 63), (65, 64), (64, 65), (128, 128), (129, 128), (128, 65), (256, 128), (200, 3))


def edge_args(n_tracks, d):
    """edge_scene's arguments for a stage A of n_tracks x d: the tracks split over the two crowds."""
    return -(-n_tracks // 2), n_tracks // 2, d
SHIFTS = ((0.0, 0.0), (55.0, 62.0), (55.0, 0.0), (0.0, 62.0))


def solver_form(n_rows, n_cols):
    """The form lsap_wave takes for a natural n_rows x n_cols matrix: 1 (lsap_wave_small), 2 or 4 (lsap_wave_regs<2> / <4>)."""
    big = max(n_rows, n_cols)
    return 1 if big <= 64 else 2 if big <= 128 else 4


def _cells(shift=0):
    """128 lattice cells, 16 columns, pitch 110 x 125; the four SHIFTS give lattices whose 40 x 55 boxes are disjoint (the first two:
    40 x 90 boxes)."""
    gx, gy = np.meshgrid(np.arange(16) * 110.0 + 10.0, np.arange(8) * 125.0 + 10.0)
    return np.stack([gx.reshape(-1), gy.reshape(-1)], 1) + SHIFTS[shift]


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _protos(rng, n):
    return _unit(rng.standard_normal((n, 512)))


def _sight(rng, proto, sigma=0.02):
    return _unit(proto + sigma * rng.standard_normal(proto.shape)).astype(np.float32)


def _near(rng, feats, sigma=0.005):
    return _unit(feats + sigma * rng.standard_normal(feats.shape).astype(np.float32)).astype(np.float32)


def _boxes(xy, w, h, score):
    return np.column_stack([xy, xy + (w, h), score, np.zeros(len(xy))]).astype(np.float32)


def _twin(rng, d, f):
    """A second sighting of the same person: the box shifted by (3, 2, 3, 2), the score 0.01 lower, the feature 0.005 noise away."""
    t = d.copy()
    t[:, :4] += np.array([3, 2, 3, 2], np.float32)
    t[:, 4] -= np.float32(0.01)
    return t, _near(rng, f)


def _permuted(rng, d, f):
    p = rng.permutation(len(d))
    return np.ascontiguousarray(d[p]), np.ascontiguousarray(f[p])


def two_crowds(seed):
    """Two interleaved lattices A and B of 120 boxes 40 x 90 (B = A + (55, 62): no box of one overlaps a box of the other), 1 px jitter,
    in the order A A A B B B A A B; every frame adds twins of the crowd's first 8 cells (128 rows), exact copies of box and feature on
    the crowd's first frame (the two tracks are exact twins from birth: tied rows in the next frame's stage B), near copies afterwards;
    rows permuted.  The oracle: 128 tracks on frames 0 - 2, 256 from frame 3; stage A 128 x 128 unambiguous on frames 3 - 5 and
    256 x 128 ambiguous on frames 6 - 8 (transposed, spilled, lsap_wave_regs<4>); stage B 128 x 128 ambiguous on frames 1, 2, 4, 5
    (16384 entries: spilled, lsap_wave_regs<2>); no capacity error at exactly 256 live tracks."""
    rng = np.random.default_rng(21000 + seed)
    lat = [_cells(0)[:120], _cells(1)[:120]]
    proto = _protos(rng, 240)
    frames, seen = [], set()
    for c in (0, 0, 0, 1, 1, 1, 0, 0, 1):
        d = _boxes(lat[c] + rng.normal(0.0, 1.0, (120, 2)), 40.0, 90.0, rng.uniform(0.5, 0.95, 120))
        f = _sight(rng, proto[c * 120:(c + 1) * 120])
        if c in seen:
            td, tf = _twin(rng, d[:8], f[:8])
        else:
            td, tf = d[:8].copy(), f[:8].copy()
            td[:, 4] -= np.float32(0.01)
        seen.add(c)
        frames.append(_permuted(rng, np.concatenate([d, td]), np.concatenate([f, tf])))
    return frames


def edge_scene(n_a, n_b, d):
    """Crowd A (n_a rows) for three frames, crowd B (n_b rows) for three frames, then one frame of d rows: stage A of that frame is
    exactly (n_a + n_b) x d.  Crowd A's last row repeats the row of cell 0 exactly in all three frames, so cell 0 owns two tracks that
    are equal in every bit; the last frame holds two sightings of cell 0 (a twin pair, the later row the cleaner one: 0.01 noise): two
    identical cost rows with two entries under the threshold each, so the LSAP must run and meets an exact tie, and where the tracks
    are the solver's rows (n_a + n_b <= d) the first track takes the second column.  With d >= 4 and fewer than 256 tracks the last frame also holds B's cell 0 twice,
    exactly (tied columns; the copy that loses starts a track).  Its other rows: cells of B and A in turn, then cells that nobody has seen."""
    assert 2 <= n_a <= 128 and 1 <= n_b <= 128 and 2 <= d <= 128
    rng = np.random.default_rng(22000 + 1000 * (n_a + n_b) + d)
    ca, cb = _cells(0), _cells(1)
    pa, pb = _protos(rng, 128), _protos(rng, 128)
    frames = []
    ia = np.r_[np.arange(n_a - 1), 0]
    for _ in range(3):
        dd = _boxes(ca + rng.normal(0.0, 1.0, (128, 2)), 40.0, 90.0, rng.uniform(0.5, 0.95, 128))
        frames.append(_permuted(rng, dd[ia], _sight(rng, pa)[ia]))
    for _ in range(3):
        dd = _boxes(cb + rng.normal(0.0, 1.0, (128, 2)), 40.0, 90.0, rng.uniform(0.5, 0.95, 128))
        frames.append(_permuted(rng, dd[:n_b], _sight(rng, pb)[:n_b]))
    da = _boxes(ca + rng.normal(0.0, 1.0, (128, 2)), 40.0, 90.0, rng.uniform(0.5, 0.95, 128))
    db = _boxes(cb + rng.normal(0.0, 1.0, (128, 2)), 40.0, 90.0, rng.uniform(0.5, 0.95, 128))
    fa, fb = _sight(rng, pa), _sight(rng, pb)
    td, _ = _twin(rng, da[:1], fa[:1])
    tf = _sight(rng, pa[:1], 0.01)                       # the twin is the cleaner sighting: the cheaper column of both tracks
    rows, feats = [da[0], td[0]], [fa[0], tf[0]]
    if d >= 4 and n_a + n_b < MAX_TRACKS:
        rows += [db[0], db[0]]
        feats += [fb[0], fb[0]]
    rest = []                                            # B1, A1, B2, A2, ... over the cells that own a track, then unseen cells of A
    for i in range(1, 128):
        if i < n_b:
            rest.append((db[i], fb[i]))
        if i < n_a - 1:
            rest.append((da[i], fa[i]))
    rest += [(da[i], fa[i]) for i in range(n_a - 1, 128)]
    for r, f in rest[:d - len(rows)]:
        rows.append(r)
        feats.append(f)
    assert len(rows) == d
    p = rng.permutation(d)
    i0, i1 = int(np.nonzero(p == 0)[0][0]), int(np.nonzero(p == 1)[0][0])
    if i1 < i0:                                          # the cheaper twin comes second: the first track's column is not the first one
        p[i0], p[i1] = 1, 0
    frames.append((np.ascontiguousarray(np.stack(rows)[p]), np.ascontiguousarray(np.stack(feats)[p])))
    return frames


def dense_crowd(seed, n_frames=10):
    """128 people on a lattice of 32 columns 20 px apart, closer than a box is wide (44 x 100: neighbours overlap with IoU 0.375, so
    every stage B row over tentative tracks has several entries under max_iou_distance), drifting 2 px a frame with 1 px jitter.  From
    frame 1 on 12 sightings are dropped and 4 of the others are duplicated exactly (120 rows): stage B is ambiguous on the tentative
    frames 1 and 2, and after confirmation the duplicates make stage A ambiguous while the duplicates' left-over copies and the tracks
    that missed their sighting meet in a stage B of the same frame."""
    rng = np.random.default_rng(23000 + seed)
    gx, gy = np.meshgrid(np.arange(32) * 20.0 + 30.0, np.arange(4) * 130.0 + 20.0)
    base = np.stack([gx.reshape(-1), gy.reshape(-1)], 1)
    proto = _protos(rng, 128)
    frames = []
    for k in range(n_frames):
        d = _boxes(base + (2.0 * k, 0.0) + rng.normal(0.0, 1.0, (128, 2)), 44.0, 100.0, rng.uniform(0.5, 0.95, 128))
        f = _sight(rng, proto)
        if k:
            keep = np.sort(rng.permutation(128)[12:])
            dup = rng.choice(keep, 4, replace=False)
            d, f = np.concatenate([d[keep], d[dup]]), np.concatenate([f[keep], f[dup]])
        frames.append(_permuted(rng, d, f))
    return frames


def churn(seed, max_age):
    """Four disjoint crowds of 85 boxes 40 x 55, three frames each (12 frames), for a tracker with max_age 5 or 6: 255 tracks on
    frames 6 and 7; the first crowd's 85 tracks die on frame 8 (max_age 5: one frame before the fourth crowd is born, 170 tracks in
    between) or on frame 9 (max_age 6: in the frame of the 85 births, which take the slots freed in that frame: 255 -> 255).  No
    capacity error.  (The scene does not depend on max_age; the argument names the tracker it is meant for.)"""
    assert max_age in (5, 6)
    rng = np.random.default_rng(24000 + seed)
    proto = _protos(rng, 4 * 85)
    frames = []
    for k in range(12):
        c = k // 3
        d = _boxes(_cells(c)[:85] + rng.normal(0.0, 1.0, (85, 2)), 40.0, 55.0, rng.uniform(0.5, 0.95, 85))
        frames.append(_permuted(rng, d, _sight(rng, proto[c * 85:(c + 1) * 85])))
    return frames


def overflow(seed):
    """Three disjoint crowds of 100, three frames each: the third crowd meets 200 coasting tracks, so only the 56 unmatched detections
    of lowest index start a track (SS_ERR_CAPACITY), on each of its frames; those 56 are confirmed while the error is pending."""
    rng = np.random.default_rng(25000 + seed)
    proto = _protos(rng, 300)
    frames = []
    for k in range(9):
        c = k // 3
        d = _boxes(_cells(c)[:100] + rng.normal(0.0, 1.0, (100, 2)), 40.0, 55.0, rng.uniform(0.5, 0.95, 100))
        frames.append(_permuted(rng, d, _sight(rng, proto[c * 100:(c + 1) * 100])))
    return frames


def sparse(seed, n_frames=9):
    """A plain make_stream of 12 identities (the streams of tests/test_gpu_sequence.py), as a neighbour of a crowd."""
    from strongsort_yolo_amd.synth import make_stream
    st = make_stream(seed, W, H, 12)
    return [(fr.dets, fr.feats) for fr in (st.next_frame() for _ in range(n_frames))]


SCENES = {"two_crowds": two_crowds, "edge_scene": edge_scene, "dense_crowd": dense_crowd, "churn": churn, "overflow": overflow, "sparse": sparse}


def config(name, *args):
    return StrongSortConfig(max_age=args[1]) if name == "churn" else StrongSortConfig()


def needs_lsap(cost, thr):
    """The comment above frame_assign (ss_track.hip), restated: every entry above the threshold holds the replacement value, so the
    assignment can be read off the matrix unless some row or column has more than one entry not above the threshold.
    -> 0 (no matrix), 1 (shortcut) or 2 (LSAP): the value of debug()["path_a"] / ["path_b"]."""
    if cost.shape[0] == 0 or cost.shape[1] == 0:
        return 0
    ok = ~(cost > thr)
    return 2 if (ok.sum(1) > 1).any() or (ok.sum(0) > 1).any() else 1


@functools.lru_cache(maxsize=None)
def reference(name, *args, numerics="c"):
    """The oracle (with the device's capacity, max_tracks = 256) over SCENES[name](*args), computed once per process and shared; callers
    do not modify it.  -> namespace: cfg, frames, rows / lasts (OracleStrongSort.last) / n_tracks per frame, stages: per frame
    ((n_rows, n_cols, path) of stage A, the same of stage B) in the natural orientation (rows = tracks), orc (the oracle after the last
    frame: capacity_error, tracks), snapshot (its snapshot()), seconds (the oracle's time per frame)."""
    import time
    from oracle.strongsort_np import OracleStrongSort
    cfg, frames = config(name, *args), SCENES[name](*args)
    orc = OracleStrongSort(cfg, numerics, max_tracks=MAX_TRACKS)
    rows, lasts, stages, n_tracks, seconds = [], [], [], [], []
    for d, f in frames:
        t0 = time.perf_counter()
        rows.append(orc.update(d, f, (H, W)))
        seconds.append(time.perf_counter() - t0)
        last = orc.last
        lasts.append(last)
        stages.append(((*last["cost_a"].shape, needs_lsap(last["cost_a"], cfg.max_dist)),
                       (*last["cost_b"].shape, needs_lsap(last["cost_b"], cfg.max_iou_distance))))
        n_tracks.append(len(orc.tracks))
    return SimpleNamespace(name=name, args=args, cfg=cfg, frames=frames, rows=rows, lasts=lasts, stages=stages, n_tracks=n_tracks, orc=orc,
                           snapshot=orc.snapshot(), seconds=seconds)


def lsap_shapes(run):
    """The largest stage A and stage B shapes of the run that need the LSAP: ((n_rows, n_cols) or None, the same)."""
    out = []
    for st in (0, 1):
        s = [(r * c, (r, c)) for r, c, p in (fs[st] for fs in run.stages) if p == 2]
        out.append(max(s)[1] if s else None)
    return tuple(out)


def tie_flips(run):
    """Exact ties that the rows show.  Per frame and stage, for every pair of cost rows r1 < r2 that are equal in every bit and both
    matched (twin tracks: either pairing of their two columns costs the same), the naive choice gives the first row the first of the
    two columns.  -> (pairs seen, pairs where the oracle's LSAP chose the other way round)."""
    seen = flips = 0
    for last in run.lasts:
        for cost, pairs in ((last["cost_a"], last["pairs_a"]), (last["cost_b"], last["pairs_b"])):
            col = dict(pairs)
            first = {}
            for r in range(cost.shape[0]):
                if r not in col:
                    continue
                r1 = first.setdefault(cost[r].tobytes(), r)
                if r1 == r:
                    continue
                c1, c2 = col[r1], col[r]
                seen += 1
                flips += int(c1 > c2)
    return seen, flips
