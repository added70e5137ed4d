"""Scenes for the OC-SORT tracker (docs/OCSORT.md §5): the hand-built sequences with hand-derived outcomes, one branch each, and the
two-frame pairs that make the first association an LSAP of an exact size with a tie.

Not a conftest and not a test module: imported by tests/test_ocsort_cpu.py and tests/test_gpu_ocsort.py.
"""
from __future__ import annotations

import numpy as np

from strongsort_yolo_amd.config import OCSortConfig
from tests.byte_crowd import _lattice, _rows

# (n_tracks, n_rows): the last LDS-resident size (2048 entries), the first spilled ones, the 64-column edge of the solver's forms in
# both orientations, and the largest frame against as many tracks
EDGE_SIZES = ((32, 64), (33, 64), (64, 33), (64, 64), (65, 64), (64, 65), (128, 128))


def edge_pair(n_tracks, n_rows):
    """Two frames: n_tracks separated boxes (all born on frame 1), then n_rows high-score rows — n_rows - 1 boxes over the first
    cells, slightly moved, the others on cells of their own, and one of the rows over a track repeated exactly.  That track has
    two partners above the IoU threshold, so upstream's shortcut does not apply: the first association is an LSAP of exactly
    n_rows x n_tracks with two tied rows."""
    rng = np.random.default_rng(24000 + 131 * n_tracks + n_rows)
    cells = _lattice(16, 8, 70.0, 50.0)
    f1 = _rows(cells[:n_tracks], 44.0, 30.0, rng.uniform(0.5, 0.95, n_tracks))
    f2 = _rows(cells[:n_rows - 1] + rng.normal(0.0, 1.5, (n_rows - 1, 2)), 44.0, 30.0, rng.uniform(0.5, 0.95, n_rows - 1))
    f2 = np.concatenate([f2, f2[int(rng.integers(0, min(n_tracks, n_rows - 1)))][None]])
    return [f1, np.ascontiguousarray(f2[rng.permutation(n_rows)])]


# ---- hand-built scenarios: name -> (frames, cfg, check(list of rows, reference after the last frame)) ------------------------------
def box(x, y=0.0, w=40.0, h=80.0, score=0.9, cls=0.0):
    return [x, y, x + w, y + h, score, cls]


def F(*rows):
    return np.asarray(rows, np.float32).reshape(-1, 6)


E = F()


def _ids(rows):
    return [int(i) for i in rows[:, 4]]


def sc_birth_and_min_hits():
    """Track 1 from frame 1: shown on frames 1..3 by the frame_count clause (hit_streak 0, 1, 2), from frame 4 by its streak.
    Track 2 is born on frame 5, past the clause: hit_streak reaches min_hits = 3 on frame 8, its first row."""
    frames = [F(box(100 + 2 * k)) if k < 4 else F(box(100 + 2 * k), box(400, 300)) for k in range(8)]

    def check(rows, ref):
        assert [_ids(r) for r in rows] == [[1]] * 7 + [[2, 1]]                       # newest track first
        assert all(r[-1, 7] == 0 for r in rows) and rows[7][0, 7] == 1
        assert np.array_equal(rows[3][0, :4], frames[3][0, :4])                      # the row's own box, not the filter's
        t = ref.tracks()
        assert list(t["hits"]) == [7, 3] and list(t["hit_streak"]) == [7, 3] and list(t["age"]) == [7, 3]
    return frames, OCSortConfig(), check


def _gap(n_missed):
    cfg = OCSortConfig(max_age=4)
    frames = [F(box(100)), F(box(101))] + [E] * n_missed + [F(box(102))]
    return frames, cfg


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
        assert all(len(r) == 0 for r in rows[2:])                                    # frame_count > min_hits, no streak
    return frames, cfg, check


def sc_oru_straight_line():
    """A box on a straight line (10 px a frame), seen on frames 1..4, missed on 5..7, seen again on the line on frame 8: the
    filter frozen at frame 5 is re-filtered over 4 virtual observations (tests/test_ocsort_cpu.py compares the state)."""
    frames = [F(box(100 + 10 * k, 50 + 5 * k)) for k in range(4)] + [E] * 3 + [F(box(170, 85))]

    def check(rows, ref):
        t = ref.tracks()
        assert list(t["track_id"]) == [1] and ref.counters["oru_tracks"] == 1 and ref.counters["oru"] == 4
        assert list(t["frozen"]) == [0] and list(t["hits"]) == [4]
    return frames, OCSortConfig(), check


def sc_ocr_recovers_from_last_observation():
    """A box moves 12 px a frame for 5 frames, then stops for good where it was last seen and is missed for 6 frames: the
    filter's box drifts on (about 12 px a frame: no overlap after 6 frames), so the first association finds nothing; OCR matches
    the row to the track's last observation (IoU 1)."""
    frames = [F(box(100 + 12 * k)) for k in range(5)] + [E] * 6 + [F(box(148))]

    def check(rows, ref):
        t = ref.tracks()
        assert ref.counters["ocr"] == 1 and list(t["track_id"]) == [1] and list(t["hits"]) == [5]
    return frames, OCSortConfig(), check


def sc_byte_rescues_low_row():
    """use_byte: the second frame's row scores 0.15 (between low_thresh and det_thresh): no high row, the BYTE stage matches it."""
    frames = [F(box(100)), F(box(102, score=0.15)), F(box(104))]

    def check(rows, ref):
        assert ref.counters["byte"] == 1 and [_ids(r) for r in rows] == [[1], [1], [1]]
        assert rows[1][0, 6] == np.float32(0.15)
    return frames, OCSortConfig(use_byte=True), check


def sc_low_row_without_byte():
    """The same frames without use_byte: the low row is not looked at, the track misses a frame (hit_streak restarts)."""
    frames = sc_byte_rescues_low_row()[0]

    def check(rows, ref):
        assert [_ids(r) for r in rows] == [[1], [], [1]] and list(ref.tracks()["hit_streak"]) == [1]
    return frames, OCSortConfig(), check


def sc_scores_at_the_thresholds():
    """Scores compare in float32, strictly: a row exactly at det_thresh is neither high nor second; a row exactly at low_thresh is
    not second.  Frame 1 gives birth only to the 0.9 row; with use_byte the track's own row then scores exactly 0.25 (frame 2) and
    exactly 0.1 (frame 3): not matched; the 0.2 of frame 4 is a second row and is."""
    frames = [F(box(100), box(300, score=0.25)), F(box(101, score=0.25)), F(box(102, score=0.1)), F(box(103, score=0.2))]

    def check(rows, ref):
        t = ref.tracks()
        assert list(t["track_id"]) == [1] and ref.counters["byte"] == 1 and list(t["hits"]) == [1]
        assert [len(r) for r in rows] == [1, 0, 0, 0]
    return frames, OCSortConfig(use_byte=True), check


def sc_shrinking_box_clamps_area_velocity():
    """A box that shrinks fast: the filter's area velocity would take the area below zero, so predict sets x[6] to 0 first."""
    frames = [F(box(100, 0, 80.0 * 0.45 ** k, 160.0 * 0.45 ** k)) for k in range(5)] + [E, E, E]

    def check(rows, ref):
        assert ref.counters["clamp"] >= 1 and np.isfinite(ref.tracks()["x"]).all()
    return frames, OCSortConfig(iou_threshold=0.1), check


def sc_momentum_keeps_ids_at_a_crossing():
    """Two tall boxes (40 x 160) cross at right angles, 15 px a frame: A along x at y = 100, B along y at x = 100, eight pixels
    behind A so that the two rows never coincide.  The filters predict (115, 100) and (100, 107) for frame 6.  Its rows (106, 100)
    and (106, 94) lie between the two: the predicted boxes' IoUs are .633 / .685 (row 0 with A / B) and .595 / .641 (row 1), so the
    swapped pairing is ahead by .006 and IoU alone (inertia = 0, tests/test_ocsort_cpu.py) swaps the ids.  Row 0 lies straight
    ahead of A (cos 1, against .986 for row 1) and row 1 is the straighter one for B: the momentum term, .169 for the straight
    pairing against .161, turns the assignment."""
    frames, cfg = crossing()

    def check(rows, ref):
        assert all({int(r[7]): int(r[4]) for r in rw} == {0: 1, 1: 2} for rw in rows)    # row 0 stays A (id 1), row 1 stays B
        assert ref.counters["lsap"] >= 1
    return frames, cfg, check


CROSS_A, CROSS_B = (106.0, 100.0), (106.0, 94.0)               # the decisive frame's rows (top-left corners)


def crossing(inertia=0.2):
    frames = [F(box(40 + 15 * k, 100, 40, 160), box(100, 32 + 15 * k, 40, 160)) for k in range(5)]
    frames.append(F(box(CROSS_A[0], CROSS_A[1], 40, 160), box(CROSS_B[0], CROSS_B[1], 40, 160)))
    return frames, OCSortConfig(inertia=inertia, min_hits=0)


SCENARIOS = {f.__name__[3:]: f for f in (
    sc_birth_and_min_hits, sc_gap_of_max_age_kept, sc_gap_past_max_age_removed, sc_oru_straight_line,
    sc_ocr_recovers_from_last_observation, sc_byte_rescues_low_row, sc_low_row_without_byte, sc_scores_at_the_thresholds,
    sc_shrinking_box_clamps_area_velocity, sc_momentum_keeps_ids_at_a_crossing)}
