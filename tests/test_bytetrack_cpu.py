"""The BYTE tracker family (docs/BYTETRACK.md): the CPU reference (tests/bytetrack_ref.py) on hand-built sequences with
hand-derived outcomes, one branch each; the configuration, YOLO(tracker_type=...) validation and the CLI's --tracker.
The same scenarios run on the device in tests/test_gpu_bytetrack.py."""
import numpy as np
import pytest

from strongsort_yolo_amd.config import ByteTrackConfig, byte_config
from strongsort_yolo_amd.synth import make_stream
from tests.bytetrack_ref import LOST, TRACKED, ByteTrackRef, fuse_score, iou_cost


def box(x, y=0.0, w=40.0, h=80.0, score=0.9, cls=0.0):
    return [x, y, x + w, y + h, score, cls]


def F(*rows):
    return np.asarray(rows, np.float32).reshape(-1, 6)


E = F()                                                       # a frame without detections


def byte_stream(seed, n_frames, width=1280, height=720, n_ids=28):
    """A synthetic stream for the BYTE family: a seeded share of the scores pushed into (0.1, 0.25), dropped sightings,
    short-lived false positives, and some scores exactly at the thresholds."""
    st, rng = make_stream(seed, width, height, n_ids), np.random.default_rng(1000 + seed)
    out = []
    for _ in range(n_frames):
        d = st.next_frame().dets.astype(np.float32).copy()
        n = len(d)
        low = rng.random(n) < 0.25
        d[low, 4] = rng.uniform(0.1, 0.25, int(low.sum())).astype(np.float32)
        edge = rng.random(n) < 0.03
        d[edge, 4] = rng.choice(np.array([0.25, 0.1], np.float32), int(edge.sum()))
        d = d[rng.random(n) >= 0.1]
        k = int(rng.integers(0, 3))
        if k:
            x, y = rng.uniform(0, width - 80, k), rng.uniform(0, height - 160, k)
            w, h = rng.uniform(20, 80, k), rng.uniform(40, 160, k)
            fp = np.stack([x, y, x + w, y + h, rng.uniform(0.1, 0.7, k), rng.integers(0, 3, k)], 1).astype(np.float32)
            d = np.concatenate([d, fp])
        out.append(np.ascontiguousarray(d[:128]))
    return out


def _ids(rows):
    return [int(i) for i in rows[:, 4]]


# ---- scenarios: (frames, kalman, check(list of rows, reference after the last frame)) ------------------------------------------
def sc_low_rescue():
    frames = [F(box(100)), F(box(102, score=0.15))]

    def check(rows, ref):
        assert _ids(rows[0]) == [1]
        assert _ids(rows[1]) == [1] and rows[1][0, 7] == 0 and rows[1][0, 6] == np.float32(0.15)    # rescued by the low row
    return frames, "xyah", check


def sc_reactivate():
    frames = [F(box(100)), E, E, E, F(box(100))]

    def check(rows, ref):
        assert _ids(rows[0]) == [1] and all(len(r) == 0 for r in rows[1:4])
        assert _ids(rows[4]) == [1] and ref.next_id == 2            # re-activated with its id, no birth
    return frames, "xyah", check


def sc_kept_at_max_time_lost():
    frames = [F(box(100))] + [E] * 30 + [F(box(100))]               # lost at frame 2 (end 1); frame 31: 31 - 1 = 30, kept

    def check(rows, ref):
        assert _ids(rows[-1]) == [1] and ref.next_id == 2
    return frames, "xyah", check


def sc_removed_after_max_time_lost():
    frames = [F(box(100))] + [E] * 31 + [F(box(100)), F(box(100))]  # frame 32: 32 - 1 = 31 > 30, removed

    def check(rows, ref):
        assert len(rows[32]) == 0                                   # frame 33: a new track (id 2), not activated yet
        assert _ids(rows[33]) == [2]
    return frames, "xyah", check


def sc_unconfirmed_removed():
    A, B = box(100), box(600)
    frames = [F(A), F(A, B), F(A), F(A, B), F(A, B)]

    def check(rows, ref):
        assert _ids(rows[0]) == [1] and _ids(rows[1]) == [1]       # B (id 2) born unconfirmed: no row
        assert _ids(rows[2]) == [1]                                 # ... and removed after one miss
        assert _ids(rows[3]) == [1] and _ids(rows[4]) == [1, 3]     # B again: id 3, activated by its second sighting
    return frames, "xyah", check


def sc_activation_frame1_only():
    A, B = box(100), box(600)
    frames = [F(A, B), F(A, B, box(1000)), F(A, B, box(1000))]

    def check(rows, ref):
        assert _ids(rows[0]) == [1, 2]                              # frame 1: births are activated at once
        assert _ids(rows[1]) == [1, 2] and _ids(rows[2]) == [1, 2, 3]
    return frames, "xyah", check


def sc_duplicate_lost_goes():
    P, Q = box(100), box(102)
    frames = [F(P), F(P, Q), F(P, Q), F(P)]

    def check(rows, ref):
        # frame 4: id 2 (start 2, end 3) is lost beside id 1 (start 1, end 4): 1 - IoU < 0.15, the shorter-lived lost one goes
        assert _ids(rows[3]) == [1] and [t.id for t in ref.tracked] == [1] and ref.lost == []
    return frames, "xyah", check


def sc_duplicate_tie_tracked_goes():
    P, Q = box(100), box(102)
    frames = [F(P), F(P, Q), F(P, Q), F(Q), F(Q)]

    def check(rows, ref):
        # frame 4: id 2 (start 2) tracked, id 1 (start 1, end 3) lost: both lived 2 frames -> the tracked one goes
        assert len(rows[3]) == 0
        assert _ids(rows[4]) == [1]                                 # and the kept lost track is re-found
    return frames, "xyah", check


def sc_score_and_cost_edges():
    frames = [F(box(0, score=0.25)),                                # exactly track_high_thresh: high, a birth
              F(box(0, w=32, score=0.25), box(400, score=np.float32(0.1)))]     # fused cost exactly 0.8: matched; 0.1: not low

    def check(rows, ref):
        assert _ids(rows[0]) == [1]
        assert _ids(rows[1]) == [1] and rows[1][0, 7] == 0 and ref.next_id == 2
    return frames, "xyah", check


def sc_cost_above_thresh():
    frames = [F(box(0, score=0.25)), F(box(0, w=31, score=0.25))]  # fused cost just above 0.8: no match, a new track

    def check(rows, ref):
        assert len(rows[1]) == 0 and ref.next_id == 3 and [t.state for t in ref.lost] == [LOST]
    return frames, "xyah", check


def _growing(kalman):
    frames = [F(box(100, w=40 + 20 * k)) for k in range(4)] + [E, E]

    def check(rows, ref):
        (t,) = ref.lost
        assert t.mean[7] == 0.0
        if kalman == "xywh":
            assert t.mean[6] == 0.0                                 # BoT-SORT: width velocity zeroed too
        else:
            assert t.mean[6] != 0.0                                 # ByteTrack: aspect velocity kept
    return frames, kalman, check


SCENARIOS = {
    "low_rescue": sc_low_rescue, "reactivate": sc_reactivate, "kept_at_max_time_lost": sc_kept_at_max_time_lost,
    "removed_after_max_time_lost": sc_removed_after_max_time_lost, "unconfirmed_removed": sc_unconfirmed_removed,
    "activation_frame1_only": sc_activation_frame1_only, "duplicate_lost_goes": sc_duplicate_lost_goes,
    "duplicate_tie_tracked_goes": sc_duplicate_tie_tracked_goes, "score_and_cost_edges": sc_score_and_cost_edges,
    "cost_above_thresh": sc_cost_above_thresh, "velocity_zeroing_xyah": lambda: _growing("xyah"),
    "velocity_zeroing_xywh": lambda: _growing("xywh"),
}


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_reference_scenario(name):
    frames, kalman, check = SCENARIOS[name]()
    ref = ByteTrackRef(ByteTrackConfig(kalman=kalman))
    rows = [ref.update(d) for d in frames]
    for r in rows:
        assert r.dtype == np.float32 and r.shape[1] == 8 and (r[:, 7] >= 0).all()
    check(rows, ref)


def test_edge_constructions_are_exact():
    """The thresholds the edge scenarios sit on are hit exactly, not approximately."""
    c = fuse_score(iou_cost([[0, 0, 40, 80]], [[0, 0, 32, 80]]), [0.25])[0, 0]
    assert c == 0.8
    assert fuse_score(iou_cost([[0, 0, 40, 80]], [[0, 0, 31, 80]]), [0.25])[0, 0] > 0.8


def test_ids_count_per_stream_and_restart_on_reset():
    a, b = ByteTrackRef(), ByteTrackRef()
    assert _ids(a.update(F(box(0), box(500)))) == [1, 2]
    assert _ids(b.update(F(box(900)))) == [1]
    a.reset()
    assert _ids(a.update(F(box(300)))) == [1] and a.frame_id == 1


def test_reference_on_a_synthetic_stream_keeps_its_invariants():
    for kalman in ("xyah", "xywh"):
        ref = ByteTrackRef(ByteTrackConfig(kalman=kalman))
        for d in byte_stream(3, 60):
            rows = ref.update(d)
            ids = [t.id for t in ref.tracked + ref.lost]
            assert len(ids) == len(set(ids)) and len(ids) <= 256
            assert all(t.state == TRACKED for t in ref.tracked) and all(t.state == LOST for t in ref.lost)
            assert len(rows) == sum(t.activated for t in ref.tracked) and ((rows[:, 7] >= 0) & (rows[:, 7] < len(d))).all()


def test_config_defaults_and_validation():
    c = ByteTrackConfig()
    assert (c.track_high_thresh, c.track_low_thresh, c.new_track_thresh, c.track_buffer, c.match_thresh) == (0.25, 0.1, 0.25, 30, 0.8)
    assert c.fuse_score and c.frame_rate == 30 and c.kalman == "xyah" and c.max_time_lost == 30
    assert (c.std_weight_position, c.std_weight_velocity, c.max_tracks, c.max_dets) == (1 / 20, 1 / 160, 256, 128)
    assert ByteTrackConfig(frame_rate=60).max_time_lost == 60
    with pytest.raises(ValueError):
        ByteTrackConfig(kalman="xyxy")
    with pytest.raises(ValueError):
        ByteTrackConfig(max_tracks=300)
    assert byte_config("strongsort") is None and byte_config("botsort").kalman == "xywh" and byte_config("bytetrack").kalman == "xyah"


def test_yolo_tracker_type_is_validated():
    import warnings
    from strongsort_yolo_amd.yolo import YOLO
    with pytest.raises(ValueError):
        YOLO("yolov8n.pt", random_init_ok=True, tracker_type="deepsort")
    with pytest.raises(ValueError):
        YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack", camera_motion=True)
    m = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort")
    assert m.tracker_type == "botsort" and m._pipe_kw["tracker"] == "botsort"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m._check_tracker("botsort.yaml")                            # the model's own family: quiet
        m._check_tracker("bytetrack.yaml")                          # the other one: tracker_type rules, said once
        m._check_tracker("strongsort.yaml")
    assert len([x for x in w if issubclass(x.category, RuntimeWarning)]) == 1
    with pytest.raises(ValueError):
        m._check_tracker("deepsort.yaml")
    assert YOLO("yolov8n.pt", random_init_ok=True).tracker_type == "strongsort"


def test_cli_tracker_flag(monkeypatch):
    from strongsort_yolo_amd import cli
    monkeypatch.setattr(cli, "process_video", lambda job: job)
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--tracker", "bytetrack"])
    assert job["tracker"] == "bytetrack" and job["reid_weights"] is None
    (job,) = cli.main(["--source", "synthetic:3"])
    assert job["tracker"] == "strongsort"
    with pytest.raises(SystemExit):
        cli.main(["--tracker", "deepsort"])
