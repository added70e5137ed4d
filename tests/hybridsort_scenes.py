"""Scenes for the Hybrid-SORT tracker (docs/HYBRIDSORT.md §5): OC-SORT's hand-built sequences under HybridSortConfig, one branch each,
and one scene per cue (HMIoU, the TCM term of either stage, the four corners, the delta_t sum) built so that the cue decides who
keeps which id: `cue_off` names the configuration change that switches the cue off, and the ids then come out differently.

Not a conftest and not a test module: imported by tests/test_hybridsort_cpu.py and tests/test_gpu_hybridsort.py.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from strongsort_yolo_amd.config import HybridSortConfig
from tests.ocsort_scenes import E, F, box


def _ids(rows):
    return [int(i) for i in rows[:, 4]]


def _id_of_row(rows):
    """det_idx -> track id of one frame's rows."""
    return {int(r[7]): int(r[4]) for r in rows}


# ---- OC-SORT's scenes under HybridSortConfig: name -> (frames, cfg, check(list of rows, reference after the last frame)) ------------
def sc_birth_and_min_hits():
    """Track 1 from frame 1: shown on frames 1..3 by the frame_count clause, from frame 4 by its streak.  Track 2 is born on frame
    5: hit_streak reaches min_hits = 3 on frame 8, its first row."""
    frames = [F(box(100 + 2 * k)) if k < 4 else F(box(100 + 2 * k), box(400, 300)) for k in range(8)]

    def check(rows, ref):
        assert [_ids(r) for r in rows] == [[1]] * 7 + [[2, 1]]
        assert np.array_equal(rows[3][0, :4], frames[3][0, :4])
        t = ref.tracks()
        assert list(t["hits"]) == [7, 3] and list(t["hit_streak"]) == [7, 3] and list(t["age"]) == [7, 3]
        assert list(t["conf"]) == [np.float32(0.9)] * 2 and list(t["conf_prev"]) == [np.float32(0.9)] * 2
    return frames, HybridSortConfig(), check


def _gap(n_missed):
    return [F(box(100)), F(box(101))] + [E] * n_missed + [F(box(102))], HybridSortConfig(max_age=4)


def sc_gap_of_max_age_kept():
    """max_age = 4: after 4 empty frames time_since_update is 4, not > 4: the track is still there and takes the row (id 1)."""
    frames, cfg = _gap(4)

    def check(rows, ref):
        t = ref.tracks()
        assert list(t["track_id"]) == [1] and list(t["hits"]) == [2] and list(t["time_since_update"]) == [0]
        assert ref.counters["oru_tracks"] == 1 and ref.counters["oru"] == 5
    return frames, cfg, check


def sc_gap_past_max_age_removed():
    """max_age = 4: the fifth empty frame makes time_since_update 5 > 4: removed; the row gives birth to track 2."""
    frames, cfg = _gap(5)

    def check(rows, ref):
        t = ref.tracks()
        assert list(t["track_id"]) == [2] and list(t["hits"]) == [0] and ref.counters["oru_tracks"] == 0
        assert list(t["conf_prev"]) == [np.float32(-1.0)]
    return frames, cfg, check


def sc_oru_straight_line():
    """A box on a straight line, seen on frames 1..4 with score 0.9, missed on 5..7, seen again on the line on frame 8 with score
    0.5: the frozen filter is re-filtered over 4 virtual observations whose confidence goes 0.8, 0.7, 0.6, 0.5."""
    frames = [F(box(100 + 10 * k, 50 + 5 * k)) for k in range(4)] + [E] * 3 + [F(box(170, 85, score=0.5))]

    def check(rows, ref):
        t = ref.tracks()
        assert list(t["track_id"]) == [1] and ref.counters["oru_tracks"] == 1 and ref.counters["oru"] == 4
        assert list(t["frozen"]) == [0] and list(t["hits"]) == [4]
        assert 0.5 < t["x"][0, 3] < 0.7 and t["x"][0, 8] < 0.0            # the confidence state came down the line, its velocity negative
    return frames, HybridSortConfig(), check


def sc_ocr_recovers_from_last_observation():
    """A box moves 12 px a frame for 5 frames, then stops where it was last seen and is missed for 6 frames: the filter's box drifts
    on, the first association finds nothing; OCR matches the row to the track's last observation."""
    frames = [F(box(100 + 12 * k)) for k in range(5)] + [E] * 6 + [F(box(148))]

    def check(rows, ref):
        t = ref.tracks()
        assert ref.counters["ocr"] == 1 and list(t["track_id"]) == [1] and list(t["hits"]) == [5]
    return frames, HybridSortConfig(), check


def sc_byte_rescues_low_row():
    """The second frame's row scores 0.15 (between low_thresh and det_thresh): no high row, the BYTE stage matches it (IoU .905
    minus |0.15 - 0.25| of the TCM term)."""
    frames = [F(box(100)), F(box(102, score=0.15)), F(box(104))]

    def check(rows, ref):
        assert ref.counters["byte"] == 1 and [_ids(r) for r in rows] == [[1], [1], [1]]
        assert rows[1][0, 6] == np.float32(0.15)
        assert list(ref.tracks()["conf_prev"]) == [np.float32(0.15)]
    return frames, HybridSortConfig(), check


def sc_low_row_without_byte():
    """The same frames with use_byte off: the low row is not looked at, the track misses a frame (hit_streak restarts)."""
    frames = sc_byte_rescues_low_row()[0]

    def check(rows, ref):
        assert [_ids(r) for r in rows] == [[1], [], [1]] and list(ref.tracks()["hit_streak"]) == [1]
    return frames, HybridSortConfig(use_byte=False), check


def sc_scores_at_the_thresholds():
    """Scores compare in float32, strictly: a row exactly at det_thresh is neither high nor second; a row exactly at low_thresh is
    not second; the 0.2 of frame 4 is a second row and is matched."""
    frames = [F(box(100), box(300, score=0.25)), F(box(101, score=0.25)), F(box(102, score=0.1)), F(box(103, score=0.2))]

    def check(rows, ref):
        t = ref.tracks()
        assert list(t["track_id"]) == [1] and ref.counters["byte"] == 1 and list(t["hits"]) == [1]
        assert [len(r) for r in rows] == [1, 0, 0, 0]
    return frames, HybridSortConfig(), check


def sc_shrinking_box_clamps_area_velocity():
    """A box that shrinks fast: the filter's area velocity would take the area below zero, so predict sets vs to 0 first."""
    frames = [F(box(100, 0, 80.0 * 0.45 ** k, 160.0 * 0.45 ** k)) for k in range(5)] + [E, E, E]

    def check(rows, ref):
        assert ref.counters["clamp"] >= 1 and np.isfinite(ref.tracks()["x"]).all()
    return frames, HybridSortConfig(iou_threshold=0.05), check                  # HMIoU of successive boxes: .45^2 * .45 = .09


# ---- one scene per cue: name -> (frames, cfg, cue_off: the fields that switch the cue off, check(rows, ref, on)) --------------------
def cue_hmiou():
    """Two standing 100 x 200 people, B (id 1) 60 px below and A (id 2) 30 px to the right of where the last frame's single row
    appears: its IoU with either is 14000 / 26000 = .538 exactly.  The heights overlap fully with A and 140 / 260 with B: HMIoU
    is .538 against .290, A keeps the row.  Plain IoU leaves a tie, which the LSAP's order gives to the first track, B."""
    two = F(box(0, 60, 100, 200), box(30, 0, 100, 200))
    frames = [two] * 4 + [F(box(0, 0, 100, 200))]

    def check(rows, ref, on):
        assert _id_of_row(rows[3]) == {0: 1, 1: 2}
        assert _ids(rows[4]) == ([2] if on else [1])
        assert (ref.counters["height"] > 0) == on
    return frames, HybridSortConfig(min_hits=0), dict(asso="iou"), check


def cue_tcm_first():
    """Two nearly coincident standing people 3 px apart, the left one (id 1) always scored 0.9 and the right one (id 2) 0.4, so their
    confidence states are 0.9 and 0.4.  On the last frame the 0.9 row stands 2.5 px to the right and the 0.4 row 0.5 px: geometry
    favours the swapped pairing (IoU .975 + .975 against .882 + .882), the TCM term charges it |0.9 - 0.4| twice."""
    frames = [F(box(100, score=0.9), box(103, score=0.4))] * 4 + [F(box(102.5, score=0.9), box(100.5, score=0.4))]

    def check(rows, ref, on):
        assert _id_of_row(rows[3]) == {0: 1, 1: 2}
        assert _id_of_row(rows[4]) == ({0: 1, 1: 2} if on else {0: 2, 1: 1})
        assert (ref.counters["tcm"] > 0) == on and ref.counters["lsap"] >= 1
    return frames, HybridSortConfig(min_hits=0), dict(tcm_first_weight=0.0), check


def cue_tcm_byte():
    """A standing person scored 0.9 (linear confidence clipped to det_thresh = 0.25), then a row scored 0.12 18 px aside: its IoU
    22 / 58 = .379 passes the threshold, .379 - |0.12 - 0.25| = .249 does not: the BYTE stage refuses it."""
    frames = [F(box(100))] * 3 + [F(box(118, score=0.12))]

    def check(rows, ref, on):
        assert _ids(rows[3]) == ([] if on else [1])
        assert ref.counters["byte"] == (0 if on else 1) and ref.counters["byte_tcm_refused"] == (1 if on else 0)
    return frames, HybridSortConfig(min_hits=0), dict(tcm_byte_weight=0.0), check


GROW = (40.0, 44.0, 48.0, 52.0)               # the growing box's widths (height = 2 width), centre fixed
GROW_BIG, GROW_SMALL = 62.0, 50.5             # the last frame's two rows, same centre


def _centred(w, score=0.9):
    return box(200.0 - w / 2.0, 200.0 - w, w, 2.0 * w, score)


def cue_four_corners():
    """A box that grows while standing still (the centre's direction is undefined, every corner moves outwards), delta_t = 1.  The last
    frame has two rows on the same centre: one larger than the last observation (row 0), one smaller (row 1) and slightly ahead on
    IoU with the predicted box.  The corners' term is +4 asin(1) / pi for the larger and -4 asin(1) / pi for the smaller one."""
    frames = [F(_centred(w)) for w in GROW] + [F(_centred(GROW_BIG), _centred(GROW_SMALL))]

    def check(rows, ref, on):
        assert _id_of_row(rows[4]) == ({0: 1, 1: 2} if on else {0: 2, 1: 1})
        assert ref.counters["lsap"] >= 1
    return frames, HybridSortConfig(min_hits=0, delta_t=1, asso="iou"), dict(inertia=0.0), check


def cue_delta_t_sum():
    """A box moving 10 px a frame along x.  With delta_t = 3 its corner velocities are sums of three unit vectors (norm 3 before the
    clip), so every row within 70 degrees of the line gets the full term; with delta_t = 1 the term falls off with the angle.  The
    filter predicts x = 150.  The last frame has a row straight ahead at 164 (row 0: A = 26 / 54 = .481, term .09 either way) and one
    at (146, 110), 59 degrees off the line as seen from the last observation and 21 degrees as seen from the one three frames back
    (row 1: A = .505; term .031 for the single direction, .09 for the clipped sum): the sum takes row 1, the single direction row 0."""
    frames = [F(box(100 + 10 * k, 100)) for k in range(5)] + [F(box(164, 100), box(146, 110))]

    def check(rows, ref, on):
        assert _id_of_row(rows[5]) == ({0: 2, 1: 1} if on else {0: 1, 1: 2})
        assert (ref.counters["vel_over_one"] > 0) == on and (ref.counters["vel_sum"] > 0) == on
    return frames, HybridSortConfig(min_hits=0, delta_t=3), dict(delta_t=1), check


SCENARIOS = {f.__name__[3:]: f for f in (
    sc_birth_and_min_hits, sc_gap_of_max_age_kept, sc_gap_past_max_age_removed, sc_oru_straight_line,
    sc_ocr_recovers_from_last_observation, sc_byte_rescues_low_row, sc_low_row_without_byte, sc_scores_at_the_thresholds,
    sc_shrinking_box_clamps_area_velocity)}
CUES = {f.__name__[4:]: f for f in (cue_hmiou, cue_tcm_first, cue_tcm_byte, cue_four_corners, cue_delta_t_sum)}


def cue_off(cfg, off):
    return dataclasses.replace(cfg, **off)


# ---- a seeded scene of people who overlap, cross and differ in height and confidence (the document's identity-switch figure) --------
def crossing_people(seed=0, n=12, frames=120):
    """-> (per frame detections [N,6], per frame ground truth [N,5] id,x1,y1,x2,y2): people of different heights walk across each other
    on two depth rows; each keeps a confidence level of its own, lowered while somebody stands in front; a tenth of the sightings drop."""
    rng = np.random.default_rng(seed)
    h = rng.uniform(120.0, 220.0, n)
    w = h * rng.uniform(0.36, 0.44, n)
    x0 = rng.uniform(50.0, 900.0, n)
    vx = rng.uniform(2.0, 6.0, n) * rng.choice([-1.0, 1.0], n)
    y0 = 300.0 + rng.uniform(-25.0, 25.0, n)
    level = rng.uniform(0.45, 0.95, n)
    dets, gts = [], []
    for k in range(frames):
        cx = x0 + vx * k
        cy = y0 + 3.0 * np.sin(0.2 * k + np.arange(n))
        b = np.stack([cx - w / 2, cy - h, cx + w / 2, cy], 1)
        sc = level + rng.normal(0.0, 0.03, n)
        for i in range(n):                                         # somebody lower in the picture covers part of i
            for j in range(n):
                if j != i and b[j, 3] > b[i, 3]:
                    ov = max(0.0, min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0])) / w[i]
                    sc[i] -= 0.35 * ov
        keep = (rng.random(n) > 0.1) & (sc > 0.12)
        jit = rng.normal(0.0, 1.5, (n, 4))
        d = np.concatenate([b + jit, np.clip(sc, 0.0, 1.0)[:, None], np.zeros((n, 1))], 1)[keep]
        dets.append(d.astype(np.float32))
        gts.append(np.concatenate([np.arange(1, n + 1)[:, None], b], 1))
    return dets, gts
