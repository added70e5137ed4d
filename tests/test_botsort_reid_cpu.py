"""BoT-SORT's ReID branch (docs/BYTETRACK.md §1c, R-01..) on the CPU: hand-derived scenarios on the reference
(tests/botsort_reid_ref.py) — crossing tracks, the proximity mask, appearance_thresh, the feature EMA, births, all-zero
features, re-activation — and the config / YOLO / CLI / ABI surface.  The device runs are in tests/test_gpu_botsort_reid.py."""
import os

import numpy as np
import pytest

from oracle import cexact
from strongsort_yolo_amd.config import ByteTrackConfig, byte_config
from tests.botsort_reid_ref import BotSortReidRef, get_dists
from tests.bytetrack_ref import ByteTrackRef
from tests.test_bytetrack_cpu import F, box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 90.0                                      # box width: a shift of W/9 gives IoU 0.8, a shift of W/4 gives IoU 0.6
XA, XB = 0.0, 32.5                            # tracks A and B (IoU 57.5 / 122.5 = 0.47 between them)
X1, X2 = 10.0, 22.5                           # d1: IoU 0.8 with A, 0.6 with B; d2: IoU 0.6 with A, 0.8 with B


def unit(i):
    v = np.zeros(512, np.float32)
    v[i] = 1.0
    return v


def with_dot(c):
    """A unit vector whose dot product with unit(0) is c."""
    v = np.zeros(512, np.float32)
    v[0], v[1] = c, np.sqrt(1.0 - c * c)
    return v


def B(x, score=0.9):
    return box(x, 100.0, W, 180.0, score)


def run(ref, frames):
    """frames: [(rows, feats)] -> the rows of every frame."""
    return [ref.update(F(*d), np.asarray(f, np.float32).reshape(-1, 512)) for d, f in frames]


def plain(frames):
    ref = ByteTrackRef(ByteTrackConfig(kalman="xywh"))
    return [ref.update(F(*d)) for d, _ in frames]


def id_of(rows, det):
    (r,) = [r for r in rows if int(r[7]) == det]
    return int(r[4])


def crossing(fa, fb, n_still=3):
    """A and B stand still for n_still frames, then d1 (near A) carries fb and d2 (near B) carries fa."""
    return [([B(XA), B(XB)], [unit(0), unit(1)])] * n_still + [([B(X1), B(X2)], [fb, fa])]


def test_crossing_ids_follow_appearance():
    frames = crossing(unit(0), unit(1))
    r_iou = plain(frames)[-1]
    assert (id_of(r_iou, 0), id_of(r_iou, 1)) == (1, 2)           # IoU only: A-d1, B-d2
    r = run(BotSortReidRef(), frames)[-1]
    assert (id_of(r, 0), id_of(r, 1)) == (2, 1)                   # ReID: A-d2, B-d1


def test_appearance_just_above_the_threshold_falls_back_to_iou():
    cfg = ByteTrackConfig(kalman="xywh", with_reid=True)
    tl = [[XA, 100.0, W, 180.0]]
    dl = [[X2, 100.0, W, 180.0]]                                  # IoU 0.6: unmasked
    iou_only = 1.0 - 0.6 * np.float32(0.9)
    near = get_dists(cfg, tl, dl, [np.float32(0.9)], [unit(0)], [with_dot(0.51)])[0, 0]      # (1 - 0.51) / 2 = 0.245
    far = get_dists(cfg, tl, dl, [np.float32(0.9)], [unit(0)], [with_dot(0.49)])[0, 0]       # 0.255 > 0.25
    assert 0.24 < near < 0.25
    assert far == pytest.approx(iou_only, abs=1e-6) and far > 0.45
    # in the tracker: a crossing whose swapped appearances are that weak keeps the IoU matches
    va, vb = np.zeros(512, np.float32), np.zeros(512, np.float32)
    va[0], va[2] = 0.49, np.sqrt(1 - 0.49 ** 2)                   # dot 0.49 with A's feature, 0 with B's
    vb[1], vb[3] = 0.49, np.sqrt(1 - 0.49 ** 2)                   # dot 0.49 with B's feature, 0 with A's
    r = run(BotSortReidRef(), crossing(va, vb))[-1]
    assert (id_of(r, 0), id_of(r, 1)) == (1, 2)


def test_proximity_mask_iou_below_half_never_matches_on_appearance():
    cfg = ByteTrackConfig(kalman="xywh", with_reid=True)
    x = W * (1 - 0.45) / (1 + 0.45)                               # IoU 0.45 with A
    c = get_dists(cfg, [[XA, 100.0, W, 180.0]], [[x, 100.0, W, 180.0]], [np.float32(0.9)], [unit(0)], [unit(0)])[0, 0]
    assert c == pytest.approx(1.0 - 0.45 * 0.9, abs=1e-6)        # the same feature, still the fused IoU cost
    # in the tracker: IoU 0.2 (fused cost 0.82 > match_thresh) with A's own appearance starts a new track
    x = W * (1 - 0.2) / (1 + 0.2)
    ref = BotSortReidRef()
    run(ref, [([B(XA)], [unit(0)])] * 2 + [([B(x)], [unit(0)])])
    ids, states, act, _ = ref.tracks()
    assert list(ids) == [2, 1] and list(states) == [1, 2] and list(act) == [0, 1]     # a new unconfirmed track, A lost


def test_birth_copies_the_unit_feature():
    raw = (np.arange(512, dtype=np.float32) - 100.0) * np.float32(0.37)
    ref = BotSortReidRef()
    ref.update(F(B(XA)), raw[None])
    assert ref.features().tobytes() == cexact.normalize(raw).tobytes()
    assert abs(float(np.linalg.norm(ref.features()[0])) - 1.0) < 1e-6


def test_low_row_match_moves_the_ema():
    g = with_dot(0.3) * np.float32(4.0)
    ref = BotSortReidRef()
    ref.update(F(B(XA)), unit(0)[None])
    ref.update(F(B(XA, score=0.15)), g[None])                     # a low row: stage 5, plain IoU
    exp = cexact.ema(unit(0), cexact.normalize(g), 0.9)
    assert ref.features().tobytes() == exp.tobytes()
    assert not np.array_equal(exp, unit(0))


def test_all_zero_feature():
    ref = BotSortReidRef()
    ref.update(F(B(XA)), np.zeros((1, 512), np.float32))
    assert not ref.features().any()                               # D-17: stays zero, no NaN
    ref.update(F(B(XA)), (3 * unit(5))[None])
    assert ref.features().tobytes() == cexact.ema(np.zeros(512, np.float32), unit(5), 0.9).tobytes()
    # a zero feature never matches on appearance: (1 - 0) / 2 = 0.5 > appearance_thresh
    cfg = ByteTrackConfig(kalman="xywh", with_reid=True)
    c = get_dists(cfg, [[XA, 100.0, W, 180.0]], [[X2, 100.0, W, 180.0]], [np.float32(0.9)], [np.zeros(512, np.float32)], [unit(0)])
    assert c[0, 0] == pytest.approx(1.0 - 0.6 * 0.9, abs=1e-6)


def test_lost_track_reactivated_through_appearance():
    frames = [([B(XA), B(XB)], [unit(0), unit(1)])] * 3 + [([], [])] * 2 + [([B(X2)], [unit(0)])]
    assert [int(r[4]) for r in plain(frames)[-1]] == [2]          # IoU 0.8 with B wins without appearance
    ref = BotSortReidRef()
    rows = run(ref, frames)
    assert [int(r[4]) for r in rows[3]] == [] and [int(r[4]) for r in rows[-1]] == [1]
    ids, states, _, _ = ref.tracks()
    assert list(ids) == [1, 2] and list(states) == [1, 2]         # A tracked again, B still lost and keeps its feature
    assert ref.features()[1].tobytes() == unit(1).tobytes()


def test_unrelated_features_leave_the_iou_result_unchanged():
    from tests.test_bytetrack_cpu import byte_stream
    rng = np.random.default_rng(7)
    ref, base = BotSortReidRef(), ByteTrackRef(ByteTrackConfig(kalman="xywh"))
    for d in byte_stream(3, 40):
        # independent random features: halved cosine distances near 0.5 > appearance_thresh, so every entry is the IoU cost
        f = rng.standard_normal((len(d), 512)).astype(np.float32)
        assert ref.update(d, f).tobytes() == base.update(d).tobytes()


def test_config():
    c = ByteTrackConfig()
    assert (c.with_reid, c.proximity_thresh, c.appearance_thresh, c.feat_alpha) == (False, 0.5, 0.25, 0.9)
    with pytest.raises(ValueError):
        ByteTrackConfig(kalman="xyah", with_reid=True)
    assert ByteTrackConfig(kalman="xywh", with_reid=True).with_reid
    assert byte_config("botsort", True).with_reid and not byte_config("botsort").with_reid
    for t in ("bytetrack", "strongsort"):
        with pytest.raises(ValueError):
            byte_config(t, True)
    with pytest.raises(ValueError):
        BotSortReidRef(ByteTrackConfig(kalman="xywh"))


def test_yolo_with_reid_arguments():
    from strongsort_yolo_amd.yolo import YOLO
    m = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", with_reid=True)
    assert m._pipe_kw["with_reid"] is True and m._pipe_kw["tracker"] == "botsort" and m._pipe_kw["reid_half"] is False
    m = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", with_reid=True, reid_fp32=False)
    assert "reid_half" not in m._pipe_kw
    assert "with_reid" not in YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort")._pipe_kw
    for t in ("bytetrack", "strongsort"):
        with pytest.raises(ValueError):
            YOLO("yolov8n.pt", random_init_ok=True, tracker_type=t, with_reid=True)


def test_cli_with_reid_flag(monkeypatch):
    from strongsort_yolo_amd import cli
    monkeypatch.setattr(cli, "process_video", lambda job: job)
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--tracker", "botsort", "--with-reid"])
    assert job["with_reid"] is True and job["tracker"] == "botsort"
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--tracker", "botsort"])
    assert job["with_reid"] is False
    for t in ("bytetrack", "strongsort"):
        with pytest.raises(SystemExit):
            cli.main(["--source", "synthetic:3", "--track", "--tracker", t, "--with-reid"])


def test_cli_passes_with_reid_to_the_model(monkeypatch):
    from strongsort_yolo_amd import cli, yolo
    seen = {}

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(yolo, "YOLO", fake)
    with pytest.raises(Stop):
        cli.process_video({"source": "synthetic:2", "track": True, "count": False, "tracker": "botsort", "with_reid": True})
    assert seen["with_reid"] is True and seen["tracker_type"] == "botsort"


def test_reid_entry_points_are_declared_and_exported():
    from strongsort_yolo_amd import lib
    src = open(os.path.join(ROOT, "include", "strongsort_hip.h")).read()
    for decl in ("int ss_byte_set_reid(ss_ctx* ctx, int on, double proximity_thresh, double appearance_thresh, double alpha);",
                 "int ss_byte_get_features(ss_ctx* ctx, int stream, int cap, float* smooth);",
                 "int ss_byte_update_group_feats(ss_ctx* ctx, int n_frames,"):
        assert decl in src
    L = lib.load()
    for name in ("ss_byte_set_reid", "ss_byte_update_group_feats", "ss_byte_get_features"):
        assert name in lib.EXPORTS and getattr(L, name).argtypes is not None
