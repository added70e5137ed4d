"""Scenes for the Deep OC-SORT tracker (docs/DEEPOCSORT.md §5): hand-built sequences with hand-derived outcomes, one branch each,
and the seeded streams (rows, identity features, warps) of the device tests.

Not a conftest and not a test module: imported by tests/test_deepocsort_cpu.py and tests/test_gpu_deepocsort.py.
A scene is (frames, feats, warps, cfg, check): per frame the rows [N,6] f32, their raw features [N,512] f32 and a warp [8] or
None; check(list of rows, reference after the last frame) asserts the outcome.
"""
from __future__ import annotations

import numpy as np

from strongsort_yolo_amd.config import DeepOCSortConfig
from strongsort_yolo_amd.synth import make_stream
from tests import byte_crowd
from tests.ocsort_scenes import E, F, box, crossing

FEAT = 512


def e(i, scale=1.0):
    """the i-th unit vector, at a scale (the tracker normalises)"""
    v = np.zeros(FEAT, np.float32)
    v[i] = scale
    return v


def mix(i, j, a=0.8, b=0.6):
    """a e_i + b e_j: a unit vector whose similarity with e_i is a"""
    return (a * e(i) + b * e(j)).astype(np.float32)


def FT(*vs):
    return np.asarray(vs, np.float32).reshape(-1, FEAT)


def _ids(rows):
    return {int(r[7]): int(r[4]) for r in rows}


def rot(theta, tx=0.0, ty=0.0, it=5.0):
    """a warp in ss_cmc_estimate's layout: rotation by theta about the origin, then a shift"""
    c, s = float(np.cos(theta)), float(np.sin(theta))
    return np.array([c, -s, tx, s, c, ty, it, 0.0])


# ---- hand-built scenes -----------------------------------------------------------------------------------------------------
def sc_appearance_keeps_ids_at_a_crossing():
    """tests/ocsort_scenes.crossing with the momentum term switched off: IoU alone swaps the ids on the last frame (the swapped
    pairing is ahead by .006).  A carries e_0 and B e_1 throughout: E is the identity, no factor is lowered, and the appearance
    cost puts 0.75 on the straight pairing."""
    frames, _ = crossing(inertia=0.0)
    feats = [FT(e(0, 2.0), e(1, 0.5)) for _ in frames]

    def check(rows, ref):
        assert all(_ids(rw) == {0: 1, 1: 2} for rw in rows)
        assert ref.counters["lsap_emb"] >= 1 and ref.counters["aw_rows"] == 0 and ref.counters["aw_cols"] == 0
    return frames, feats, [None] * len(frames), DeepOCSortConfig(inertia=0.0, min_hits=0), check


def _two_tracks_one_row(f_a, f_b, f_row):
    """two overlapping boxes born on frame 1 (x = 100 and 112), one row between them on frame 2: 1 x 2, an LSAP"""
    return [F(box(100), box(112)), F(box(106))], [FT(f_a, f_b), FT(f_row)], [None, None]


def sc_aw_one_row():
    """1 row x 2 tracks: the row has two columns (factor 1 - (0.8 - 0.5) / 0.5 = 0.4), the columns have one row each (no factor)."""
    frames, feats, warps = _two_tracks_one_row(e(0), mix(0, 1), e(0))

    def check(rows, ref):
        assert ref.counters["aw_rows"] == 1 and ref.counters["aw_cols"] == 0
        assert np.allclose(ref.last_E, [[1.0, 0.8]], atol=1e-6) and np.allclose(ref.last_W, 0.75 * 0.4, atol=1e-6)
        assert _ids(rows[1]) == {0: 1}
    return frames, feats, warps, DeepOCSortConfig(min_hits=0), check


def sc_aw_one_column():
    """2 rows x 1 track: the column has two rows (factor 0.4), the rows one column each."""
    frames = [F(box(100)), F(box(96), box(104))]
    feats = [FT(e(0)), FT(e(0), mix(0, 1))]

    def check(rows, ref):
        assert ref.counters["aw_rows"] == 0 and ref.counters["aw_cols"] == 1
        assert np.allclose(ref.last_W, 0.75 * 0.4, atol=1e-6) and _ids(rows[1])[0] == 1
    return frames, feats, [None, None], DeepOCSortConfig(min_hits=0), check


def sc_aw_m1_zero():
    """the row's feature is orthogonal to both tracks: m1 == 0, factor 0, the row's weights vanish and IoU decides."""
    frames, feats, warps = _two_tracks_one_row(e(0), e(1), e(5))

    def check(rows, ref):
        assert np.array_equal(ref.last_E, [[0.0, 0.0]]) and np.array_equal(ref.last_W, [[0.0, 0.0]])
        assert ref.counters["aw_rows"] == 1 and len(rows[1]) == 1
    return frames, feats, warps, DeepOCSortConfig(min_hits=0), check


def sc_aw_tie_gives_factor_zero():
    """both tracks carry the row's feature: m1 == m2, the factor is 1 - (1 - 0.5) / 0.5 = 0."""
    frames, feats, warps = _two_tracks_one_row(e(0), e(0), e(0))

    def check(rows, ref):
        assert np.array_equal(ref.last_E, [[1.0, 1.0]]) and np.array_equal(ref.last_W, [[0.0, 0.0]])
    return frames, feats, warps, DeepOCSortConfig(min_hits=0), check


def sc_similarity_is_zero_without_overlap():
    """a third track far away carries the first row's feature, and the far row the near tracks': no overlap, no similarity."""
    frames = [F(box(100), box(112), box(600)), F(box(106), box(600))]
    feats = [FT(e(0), e(1), e(0)), FT(e(0), e(1))]

    def check(rows, ref):
        assert ref.last_E.shape == (2, 3) and ref.last_E[0, 2] == 0.0 and ref.last_E[1, 0] == 0.0 and ref.last_E[1, 1] == 0.0
        assert ref.last_E[0, 0] == 1.0 and ref.last_E[1, 2] == 0.0 and _ids(rows[1]) == {0: 1, 1: 3}
    return frames, feats, [None, None], DeepOCSortConfig(min_hits=0), check


def sc_alpha_follows_the_score():
    """two tracks born with e_0 and e_1, matched (shortcut) by rows carrying e_2: at score 1.0 the trust is 1 and alpha =
    alpha_fixed_emb = 0.95; just above det_thresh the trust is about 0 and alpha about 1: the feature stays."""
    lowest = float(np.nextafter(np.float32(0.25), np.float32(1.0)))
    frames = [F(box(100), box(400)), F(box(101, score=1.0), box(401, score=lowest))]
    feats = [FT(e(0), e(1)), FT(e(2), e(2))]

    def check(rows, ref):
        f = ref.features()
        n = np.hypot(0.95, 0.05)
        assert ref.counters["shortcut"] == 1 and ref.counters["ema"] == 2
        assert abs(f[0, 0] - 0.95 / n) < 1e-6 and abs(f[0, 2] - 0.05 / n) < 1e-6
        assert abs(f[1, 1] - 1.0) < 1e-6 and 0.0 < f[1, 2] < 1e-6
    return frames, feats, [None, None], DeepOCSortConfig(min_hits=0), check


def sc_ocr_match_updates_the_feature():
    """tests/ocsort_scenes.sc_ocr_recovers_from_last_observation: the recovered row carries e_1 at score 1.0."""
    frames = [F(box(100 + 12 * k)) for k in range(5)] + [E] * 6 + [F(box(148, score=1.0))]
    feats = [FT(e(0))] * 5 + [np.zeros((0, FEAT), np.float32)] * 6 + [FT(e(1))]

    def check(rows, ref):
        f = ref.features()
        assert ref.counters["ocr"] == 1 and ref.counters["ema"] == 5 and f[0, 1] > 0.04 and list(ref.tracks()["hits"]) == [5]
    return frames, feats, [None] * 12, DeepOCSortConfig(), check


def sc_cmc_moves_a_frozen_track():
    """a box moves 10 px a frame for 4 frames and is missed for 3; the camera turns by 0.05 rad and shifts on the 2nd and 3rd
    missed frame (the track is frozen: x, P, xf, Pf, the last observation and the ring move), then the box is seen where the
    warps put it: the same id, re-updated from the moved frozen filter."""
    w = rot(0.05, 30.0, -12.0)
    frames = [F(box(100 + 10 * k, 200)) for k in range(4)] + [E, E, E]
    x, y = 170.0 + 20.0, 200.0 + 40.0                    # centre of the box at its 8th position, before the camera moved
    for _ in range(2):
        x, y = w[0] * x + w[1] * y + w[2], w[3] * x + w[4] * y + w[5]
    frames.append(F(box(x - 20.0, y - 40.0)))
    feats = [FT(e(0)) if len(d) else np.zeros((0, FEAT), np.float32) for d in frames]
    warps = [None, None, None, None, None, w, w, rot(0.0, it=-1.0)]

    def check(rows, ref):
        t = ref.tracks()
        assert ref.counters["warp"] == 2 and ref.counters["warp_frozen"] == 2 and ref.counters["oru_tracks"] == 1
        assert list(t["track_id"]) == [1] and list(t["hits"]) == [4] and _ids(rows[-1]) == {0: 1}
    return frames, feats, warps, DeepOCSortConfig(min_hits=0), check


def sc_negative_w6_is_no_warp():
    """a warp whose w6 is negative is skipped, whatever its matrix says (G-03)."""
    frames = [F(box(100 + 5 * k)) for k in range(4)]
    feats = [FT(e(0))] * 4
    bad = rot(0.5, 300.0, 300.0, it=-1.0)

    def check(rows, ref):
        assert ref.counters["warp"] == 0 and all(_ids(rw) == {0: 1} for rw in rows)
    return frames, feats, [None, bad, bad, bad], DeepOCSortConfig(min_hits=0), check


SCENES = {f.__name__[3:]: f for f in (
    sc_appearance_keeps_ids_at_a_crossing, sc_aw_one_row, sc_aw_one_column, sc_aw_m1_zero, sc_aw_tie_gives_factor_zero,
    sc_similarity_is_zero_without_overlap, sc_alpha_follows_the_score, sc_ocr_match_updates_the_feature,
    sc_cmc_moves_a_frozen_track, sc_negative_w6_is_no_warp)}


# ---- seeded streams ----------------------------------------------------------------------------------------------------------
def deep_stream(seed, n_frames, width=1280, height=720, n_ids=28, camera=True):
    """A synthetic stream with identities: strongsort_yolo_amd.synth's moving boxes, a tenth of the sightings dropped, a share of
    the scores below det_thresh, short-lived false positives, and the identities 0..3 unseen on frames 27..36 (a gap across the boundary
    of 32-frame groups).  Features: a unit vector per identity that shares a common part with all others (similarity about 0.6:
    adaptive weighting has second-best partners to find) plus Gaussian noise, at a random scale; a false positive has a random
    feature.  camera: byte_crowd.camera's warps (rotation up to 0.01 rad, a shift of up to 4 px, every fifth frame none: frames
    31 and 32 both carry one) and the rows moved by the accumulated warp.
    -> (frames, feats, warps [F,8] or None)"""
    st, rng = make_stream(seed, width, height, n_ids), np.random.default_rng(31000 + seed)
    base = rng.standard_normal((n_ids, FEAT)) * 0.8 + rng.standard_normal(FEAT)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    frames, feats = [], []
    for k in range(n_frames):
        fr = st.next_frame()
        d, who = fr.dets.astype(np.float32).copy(), np.asarray(fr.gt_ids).astype(np.int64)
        n = len(d)
        low = rng.random(n) < 0.15
        d[low, 4] = rng.uniform(0.1, 0.25, int(low.sum())).astype(np.float32)
        keep = rng.random(n) >= 0.1
        if 27 <= k <= 36:
            keep &= ~np.isin(who, (0, 1, 2, 3))
        d, who = d[keep], who[keep]
        f = base[who] + 0.05 * rng.standard_normal((len(d), FEAT))
        nfp = int(rng.integers(0, 3))
        if nfp:
            x, y = rng.uniform(0, width - 80, nfp), rng.uniform(0, height - 160, nfp)
            w, h = rng.uniform(20, 80, nfp), rng.uniform(40, 160, nfp)
            fp = np.stack([x, y, x + w, y + h, rng.uniform(0.1, 0.7, nfp), rng.integers(0, 3, nfp)], 1).astype(np.float32)
            d, f = np.concatenate([d, fp]), np.concatenate([f, rng.standard_normal((nfp, FEAT))])
        f = f * rng.uniform(0.5, 3.0, (len(d), 1))
        frames.append(np.ascontiguousarray(d[:128]))
        feats.append(np.ascontiguousarray(f[:128].astype(np.float32)))
    if not camera:
        return frames, feats, None
    warps, frames = byte_crowd.camera(seed, frames)
    return frames, feats, warps
