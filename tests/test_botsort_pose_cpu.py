"""BoT-SORT's keypoint term (docs/BYTETRACK.md §1e, K-01..) on the CPU: `ss_expneg` against numpy.exp, the reference
(tests/botsort_pose_ref.py) without usable keypoints against plain BoT-SORT byte for byte, identity switches of people who meet and turn back
(and of people who cross) with and without the term, hand-derived entries, and the config / YOLO / CLI / ABI surface.  The device runs are in
tests/test_gpu_botsort_pose.py."""
import os

import numpy as np
import pytest

from strongsort_yolo_amd.config import ByteTrackConfig, COCO_KPT_SIGMAS, byte_config, check_pose
from tests.botsort_pose_ref import BotSortPoseRef, EXPNEG_CUT, oks_entry, original_pixels, ss_expneg, track_pose, visible
from tests.bytetrack_ref import ByteTrackRef
from tests.test_bytetrack_cpu import F, box, byte_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 17
POSE = ByteTrackConfig(kalman="xywh", with_pose=True)
XYWH = ByteTrackConfig(kalman="xywh")


# ---- streams ------------------------------------------------------------------------------------------------------------
def skeleton(rng):
    """One identity's K keypoints in box-normalised coordinates (u, v in about [-0.5, 0.5])."""
    base = np.stack([np.linspace(-0.3, 0.3, K) * np.where(np.arange(K) % 2, 1.0, -1.0), np.linspace(-0.45, 0.45, K)], 1)
    return np.clip(base + rng.normal(0.0, 0.15, (K, 2)), -0.5, 0.5)


def place(sk, b, rng, jitter=1.5, p_occl=0.15):
    """The skeleton on box b (x1, y1, x2, y2) with pixel jitter and random occlusion -> [K,3] f32 (x, y, v)."""
    cx, cy, w, h = (b[0] + b[2]) / 2, (b[1] + b[3]) / 2, b[2] - b[0], b[3] - b[1]
    k = np.zeros((K, 3), np.float32)
    k[:, 0] = cx + sk[:, 0] * w + rng.normal(0.0, jitter, K)
    k[:, 1] = cy + sk[:, 1] * h + rng.normal(0.0, jitter, K)
    k[:, 2] = np.where(rng.random(K) < p_occl, rng.uniform(0.05, 0.4, K), rng.uniform(0.6, 0.99, K))
    return k


def crossing_stream(seed, n_frames, n_pairs=3, width=1280, turn=True):
    """Pairs of people walking towards each other, each pair in a band of its own.  turn=True (meet and turn back): when a pair's
    boxes overlap by IoU > 0.62 both stop for four frames and walk back the way they came — what a constant-velocity filter does
    not predict.  turn=False (a true crossing): they walk on through each other, overlapping by more than half on the way.  Every
    identity has its own skeleton.  -> [(dets [N,6] f32, kpts [N,K,3] f32, identities [N])], rows in a seeded order."""
    rng = np.random.default_rng(5000 + seed)
    people = []
    for p in range(n_pairs):
        y, w, h = 40.0 + 230.0 * p, rng.uniform(70, 90), rng.uniform(170, 200)
        gap, v = rng.uniform(260, 420), rng.uniform(5.0, 8.0)
        x0 = rng.uniform(100, width - 100 - gap - w)
        for side in (0, 1):
            people.append(dict(x=x0 + side * gap, y=y + rng.uniform(-4, 4), w=w * rng.uniform(0.95, 1.05), h=h * rng.uniform(0.95, 1.05),
                               v=v if side == 0 else -v, sk=skeleton(rng), pair=p, hold=0, turned=False))
    out = []
    for _ in range(n_frames):
        for p in range(n_pairs):
            a, b = people[2 * p], people[2 * p + 1]
            ov = max(0.0, min(a["x"] + a["w"], b["x"] + b["w"]) - max(a["x"], b["x"]))
            iou = ov * min(a["h"], b["h"]) / (a["w"] * a["h"] + b["w"] * b["h"] - ov * min(a["h"], b["h"]))
            if turn and not a["turned"] and iou > 0.62:
                for q in (a, b):
                    q["turned"], q["hold"], q["v"] = True, 4, -q["v"]
        rows, kps, ids = [], [], []
        for i, q in enumerate(people):
            if q["hold"] > 0:
                q["hold"] -= 1
            else:
                q["x"] += q["v"]
            bx = np.array([q["x"], q["y"], q["x"] + q["w"], q["y"] + q["h"]]) + rng.normal(0.0, 1.0, 4)
            rows.append([*bx, rng.uniform(0.6, 0.95), 0.0])
            kps.append(place(q["sk"], bx, rng))
            ids.append(i)
        order = rng.permutation(len(rows))
        out.append((np.asarray(rows, np.float32)[order], np.stack(kps)[order], [ids[j] for j in order]))
    return out


def switches(ref, stream, pose):
    """Identity switches against the generator's identities: an identity whose row carries another track id than its previous one."""
    last, n = {}, 0
    for d, k, ids in stream:
        rows = ref.update(d, k) if pose else ref.update(d)
        for r in rows:
            who, tid = ids[int(r[7])], int(r[4])
            if who in last and last[who] != tid:
                n += 1
            last[who] = tid
    return n


def pose_stream(seed, n_frames, width=1280, height=720, n_ids=28):
    """tests/test_bytetrack_cpu.byte_stream's perturbations (low scores, threshold scores, dropped sightings, false positives)
    with keypoints: every identity's skeleton on its box, random keypoints for the false positives, some visibilities exactly at
    the threshold.  -> [(dets [N,6] f32, kpts [N,K,3] f32)]"""
    from strongsort_yolo_amd.synth import make_stream
    st, rng = make_stream(seed, width, height, n_ids), np.random.default_rng(3000 + seed)
    sks, out = {}, []
    for _ in range(n_frames):
        fr = st.next_frame()
        d = fr.dets.astype(np.float32).copy()
        n = len(d)
        who = [int(i) for i in fr.gt_ids]
        kp = np.zeros((n, K, 3), np.float32)
        for i in range(n):
            if who[i] not in sks:
                sks[who[i]] = skeleton(np.random.default_rng(7000 + 97 * seed + int(who[i])))
            kp[i] = place(sks[who[i]], d[i, :4].astype(np.float64), rng)
        low = rng.random(n) < 0.25
        d[low, 4] = rng.uniform(0.1, 0.25, int(low.sum())).astype(np.float32)
        edge = rng.random(n) < 0.03
        d[edge, 4] = rng.choice(np.array([0.25, 0.1], np.float32), int(edge.sum()))
        at = rng.random((n, K)) < 0.02
        kp[..., 2][at] = np.float32(0.5)
        keep = rng.random(n) >= 0.1
        d, kp = d[keep], kp[keep]
        k = int(rng.integers(0, 3))
        if k:
            x, y = rng.uniform(0, width - 80, k), rng.uniform(0, height - 160, k)
            w, h = rng.uniform(20, 80, k), rng.uniform(40, 160, k)
            fp = np.stack([x, y, x + w, y + h, rng.uniform(0.1, 0.7, k), rng.integers(0, 3, k)], 1).astype(np.float32)
            fk = np.stack([rng.uniform(0, width, (k, K)), rng.uniform(0, height, (k, K)), rng.uniform(0, 1, (k, K))], 2).astype(np.float32)
            d, kp = np.concatenate([d, fp]), np.concatenate([kp, fk])
        out.append((np.ascontiguousarray(d[:128]), np.ascontiguousarray(kp[:128])))
    return out


# ---- ss_expneg ------------------------------------------------------------------------------------------------------------
def test_expneg_against_numpy_exp():
    xs = np.concatenate([np.linspace(0.0, EXPNEG_CUT, 700001), np.linspace(0.0, 2.0, 200001),
                         np.random.default_rng(0).uniform(0.0, EXPNEG_CUT, 100000), [0.0, EXPNEG_CUT]])
    got = np.array([ss_expneg(x) for x in xs])
    ref = np.exp(-xs)
    rel = np.abs(got - ref) / ref
    print("ss_expneg: max relative error", rel.max())
    assert rel.max() <= 1e-12
    assert ss_expneg(0.0) == 1.0
    assert ss_expneg(np.nextafter(EXPNEG_CUT, np.inf)) == 0.0 and ss_expneg(np.inf) == 0.0 and ss_expneg(np.nan) == 0.0
    assert EXPNEG_CUT < 708 and ss_expneg(EXPNEG_CUT) > 0.0


# ---- invariance: no usable keypoints = plain BoT-SORT ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 3, 11])
def test_all_invisible_equals_plain_botsort(seed):
    rng = np.random.default_rng(seed)
    ref, base = BotSortPoseRef(POSE), ByteTrackRef(XYWH)
    for d in byte_stream(seed, 60):
        kp = np.stack([rng.uniform(0, 1280, (len(d), K)), rng.uniform(0, 720, (len(d), K)), np.zeros((len(d), K))], 2).astype(np.float32)
        assert ref.update(d, kp).tobytes() == base.update(d).tobytes()
    for a, b in zip(ref.tracks(), base.tracks()):
        assert a.tobytes() == b.tobytes()
    assert not ref.keypoints()[1].any()


# ---- usefulness: people whose boxes overlap by more than half ----------------------------------------------------------------
# The seeds are fixed and every one is asserted.  Meet-and-turn-back is the motion that makes IoU association fail: the filter
# predicts that both walk on.  On a true crossing the prediction mostly keeps the ids by itself (59 of the seeds 0..59 show no
# switch without the term); that leg checks that the term does no harm there, and includes the one seed of those that switches.
CROSSING_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)
THROUGH_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 30)


def _switch_counts(seeds, turn):
    plain, pose = [], []
    for seed in seeds:
        st = crossing_stream(seed, 90, turn=turn)
        plain.append(switches(ByteTrackRef(XYWH), st, False))
        pose.append(switches(BotSortPoseRef(POSE), st, True))
    print("identity switches, turn", turn, "plain:", plain, "pose:", pose)
    return plain, pose


def test_people_who_meet_and_turn_back_switch_less_with_the_pose_term():
    plain, pose = _switch_counts(CROSSING_SEEDS, True)
    assert len(CROSSING_SEEDS) >= 8
    assert all(p >= 1 for p in plain), plain                       # every seed of the list shows the problem
    assert all(b <= a for a, b in zip(plain, pose)), (plain, pose)
    assert sum(pose) < sum(plain)
    assert plain == [4, 4, 2, 6, 6, 6, 6, 2, 4, 6] and pose == [0, 0, 0, 0, 0, 0, 2, 2, 0, 2]      # the counts docs/BYTETRACK.md states


def test_people_who_cross_keep_their_ids_with_the_pose_term():
    plain, pose = _switch_counts(THROUGH_SEEDS, False)
    assert all(b <= a for a, b in zip(plain, pose)), (plain, pose)
    assert plain == [0, 0, 0, 0, 0, 0, 0, 0, 4] and pose == [0] * 9


def _iou(a, b):
    w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    return w * h / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - w * h)


@pytest.mark.parametrize("turn", [True, False])
def test_pairs_overlap_by_more_than_half(turn):
    for seed in CROSSING_SEEDS if turn else THROUGH_SEEDS:
        best = [0.0] * 3
        for d, _, ids in crossing_stream(seed, 90, turn=turn):
            pos = {who: i for i, who in enumerate(ids)}
            best = [max(best[p], _iou(d[pos[2 * p]], d[pos[2 * p + 1]])) for p in range(3)]
        assert min(best) > 0.5, (seed, best)


# ---- hand-derived entries -------------------------------------------------------------------------------------------------
def _kp(b, off, v=0.9):
    """K keypoints on box b = (x, y, w, h) at the normalised offsets `off` [K,2]."""
    k = np.zeros((K, 3), np.float32)
    k[:, 0], k[:, 1], k[:, 2] = b[0] + b[2] / 2 + off[:, 0] * b[2], b[1] + b[3] / 2 + off[:, 1] * b[3], v
    return k


OFF = np.stack([np.linspace(-0.25, 0.25, K), np.linspace(-0.5, 0.5, K)], 1)      # exact binary fractions of a 128 x 256 box


def test_entry_of_a_perfect_match_is_zero_and_thresholds():
    b = (100.0, 50.0, 128.0, 256.0)
    z = [b[0] + b[2] / 2, b[1] + b[3] / 2, b[2], b[3]]
    kp = _kp(b, OFF)
    pose, pvis = track_pose(z, kp, visible(kp, 0.5))
    assert np.array_equal(np.array(pose), OFF)
    assert oks_entry(POSE, z, pose, pvis, kp, visible(kp, 0.5), b) == 0.0
    # fewer than min_common_kpts on both sides, or an empty box: no entry
    two = kp.copy()
    two[2:, 2] = 0.1
    assert oks_entry(POSE, z, pose, pvis, two, visible(two, 0.5), b) == 1.0
    three = kp.copy()
    three[3:, 2] = 0.1
    assert oks_entry(POSE, z, pose, pvis, three, visible(three, 0.5), b) == 0.0
    assert oks_entry(POSE, z, pose, pvis, kp, visible(kp, 0.5), (100.0, 50.0, 0.0, 256.0)) == 1.0
    # v exactly at the threshold counts (>=), float32
    at = kp.copy()
    at[:, 2] = np.float32(0.5)
    assert visible(at, 0.5).all() and not visible(at, np.nextafter(np.float32(0.5), np.float32(1))).any()
    # every keypoint 32 px off: t = exp(-1024 / (2 * 32768 * (2 sigma)^2)); the mean in keypoint order
    far = kp.copy()
    far[:, 0] += 32.0
    t = [np.exp(-1024.0 / (2.0 * 32768.0 * (2 * s) ** 2)) for s in COCO_KPT_SIGMAS]
    e = (1.0 - sum(t) / K) / 2.0
    got = oks_entry(ByteTrackConfig(kalman="xywh", with_pose=True, pose_thresh=1.0), z, pose, pvis, far, visible(far, 0.5), b)
    assert got == pytest.approx(e, rel=1e-12) and 0.25 < e < 0.5
    assert oks_entry(POSE, z, pose, pvis, far, visible(far, 0.5), b) == 1.0          # above pose_thresh: no entry
    # a box without extent stores an all-invisible pose
    assert not any(track_pose([10.0, 10.0, 0.0, 5.0], kp, visible(kp, 0.5))[1])


def test_pose_decides_between_two_overlapping_rows():
    """Two people standing close (IoU 0.78); then row 0 lies nearer to A but carries B's skeleton, row 1 nearer to B with A's."""
    w, h = 128.0, 256.0
    offs = (OFF, OFF[::-1].copy())                               # A's and B's skeletons
    still, then = (0.0, 16.0), (6.0, 10.0)
    plain, pose = ByteTrackRef(XYWH), BotSortPoseRef(POSE)
    for i in range(4):
        xs, who = (still, (0, 1)) if i < 3 else (then, (1, 0))
        d = F(*[box(x, 100.0, w, h) for x in xs])
        kp = np.stack([_kp((xs[j], 100.0, w, h), offs[who[j]]) for j in range(2)])
        rp, rk = plain.update(d), pose.update(d, kp)
    ids = lambda rows: {int(r[7]): int(r[4]) for r in rows}
    assert ids(rp) == {0: 1, 1: 2}                                # IoU: the nearer box
    assert ids(rk) == {0: 2, 1: 1}                                # pose: the own skeleton
    off, vis = pose.keypoints()
    assert off.shape == (2, K, 2) and list(vis) == [(1 << K) - 1] * 2


def test_last_observation_wins_and_lost_tracks_keep_their_pose():
    b = (100.0, 50.0, 128.0, 256.0)
    ref = BotSortPoseRef(POSE)
    k1, k2 = _kp(b, OFF), _kp(b, OFF * 0.5)
    ref.update(F(box(*b)), k1[None])
    assert np.array_equal(ref.keypoints()[0][0], OFF)
    ref.update(F(box(*b)), k2[None])
    assert np.array_equal(ref.keypoints()[0][0], OFF * 0.5)       # replaced, not smoothed (K-03)
    ref.update(F(), np.zeros((0, K, 3), np.float32))
    ids, states, _, _ = ref.tracks()
    assert list(states) == [2] and np.array_equal(ref.keypoints()[0][0], OFF * 0.5)
    ref.reset()
    assert ref.keypoints()[0].shape == (0, K, 2)


def test_geometry_path_gives_the_floats_results_show():
    import torch
    rng = np.random.default_rng(1)
    k = rng.uniform(0, 640, (5, K, 3)).astype(np.float32)
    gain, px, py = 0.5, 0.0, 140.0
    t = torch.from_numpy(k.copy())
    t[..., 0] = (t[..., 0] - px) / gain
    t[..., 1] = (t[..., 1] - py) / gain
    assert original_pixels(k, gain, px, py).tobytes() == t.numpy().tobytes()
    gain = 640.0 / 1280.0 * 0.7312
    t = torch.from_numpy(k.copy())
    t[..., 0] = (t[..., 0] - px) / gain
    assert original_pixels(k, gain, px, py)[..., 0].tobytes() == t[..., 0].numpy().tobytes()


def test_perturbed_pose_streams_run_and_differ_from_plain():
    diff = 0
    for seed in (0, 1):
        ref, base = BotSortPoseRef(POSE), ByteTrackRef(XYWH)
        for d, k in pose_stream(seed, 40):
            diff += ref.update(d, k).tobytes() != base.update(d).tobytes()
        assert ref.keypoints()[0].shape[0] == len(ref.tracked) + len(ref.lost)
    print("frames whose rows differ from plain BoT-SORT:", diff)


# ---- config / YOLO / CLI / ABI --------------------------------------------------------------------------------------------
def test_config():
    c = ByteTrackConfig()
    assert (c.with_pose, c.pose_thresh, c.kpt_vis_thresh, c.min_common_kpts, c.kpt_sigmas) == (False, 0.25, 0.5, 3, COCO_KPT_SIGMAS)
    assert len(COCO_KPT_SIGMAS) == 17
    with pytest.raises(ValueError):
        ByteTrackConfig(kalman="xyah", with_pose=True)
    with pytest.raises(ValueError):
        ByteTrackConfig(kalman="xywh", with_pose=True, with_reid=True)
    assert byte_config("botsort", False, True).with_pose and not byte_config("botsort").with_pose
    for t in ("bytetrack", "strongsort"):
        with pytest.raises(ValueError):
            byte_config(t, False, True)
    with pytest.raises(ValueError):
        byte_config("botsort", True, True)
    with pytest.raises(ValueError):
        check_pose(POSE, 0)                                       # no keypoint columns
    with pytest.raises(ValueError):
        check_pose(POSE, 3 * 16)                                  # nk // 3 != len(kpt_sigmas)
    check_pose(POSE, 51)
    check_pose(XYWH, 0)
    with pytest.raises(ValueError):
        BotSortPoseRef(XYWH)


def test_yolo_with_pose_arguments():
    from strongsort_yolo_amd.yolo import YOLO
    m = YOLO("yolo11n-pose.pt", random_init_ok=True, tracker_type="botsort", with_pose=True)
    assert m._pipe_kw["with_pose"] is True and m._pipe_kw["tracker"] == "botsort"
    assert "with_pose" not in YOLO("yolo11n-pose.pt", random_init_ok=True, tracker_type="botsort")._pipe_kw
    for t in ("bytetrack", "strongsort"):
        with pytest.raises(ValueError):
            YOLO("yolo11n-pose.pt", random_init_ok=True, tracker_type=t, with_pose=True)
    with pytest.raises(ValueError):                               # nk == 0
        YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", with_pose=True)
    with pytest.raises(ValueError):
        YOLO("yolo11n-pose.pt", random_init_ok=True, tracker_type="botsort", with_pose=True, with_reid=True)


def test_cli_with_pose_flag(monkeypatch):
    from strongsort_yolo_amd import cli
    monkeypatch.setattr(cli, "process_video", lambda job: job)
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--tracker", "botsort", "--with-pose"])
    assert job["with_pose"] is True and job["tracker"] == "botsort"
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--tracker", "botsort"])
    assert job["with_pose"] is False
    for t in ("bytetrack", "strongsort"):
        with pytest.raises(SystemExit):
            cli.main(["--source", "synthetic:3", "--track", "--tracker", t, "--with-pose"])
    with pytest.raises(SystemExit):
        cli.main(["--source", "synthetic:3", "--track", "--tracker", "botsort", "--with-pose", "--with-reid"])
    with pytest.raises(SystemExit):                               # a detector without keypoints
        cli.main(["--source", "synthetic:3", "--track", "--tracker", "botsort", "--with-pose", "--weights", "yolov8n.pt"])


def test_cli_passes_with_pose_to_the_model(monkeypatch):
    from strongsort_yolo_amd import cli, yolo
    seen = {}

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(yolo, "YOLO", fake)
    with pytest.raises(Stop):
        cli.process_video({"source": "synthetic:2", "track": True, "count": False, "tracker": "botsort", "with_pose": True})
    assert seen["with_pose"] is True and seen["tracker_type"] == "botsort"


def test_pose_entry_points_are_declared_and_exported():
    from strongsort_yolo_amd import lib
    src = open(os.path.join(ROOT, "include", "strongsort_hip.h")).read()
    for decl in ("int ss_byte_set_pose(ss_ctx* ctx, int on, int n_kpt, const double* sigmas, double proximity_thresh, double pose_thresh,",
                 "int ss_byte_update_group_kpts(ss_ctx* ctx, int n_frames, const float* d_dets, const int* d_ndets, const float* d_kpts,",
                 "int ss_byte_get_keypoints(ss_ctx* ctx, int stream, int cap,",
                 "int ss_byte_get_det_keypoints(ss_ctx* ctx, int frame, int stream, float* xy, unsigned* visible);"):
        assert decl in src
    L = lib.load()
    for name in ("ss_byte_set_pose", "ss_byte_update_group_kpts", "ss_byte_get_keypoints", "ss_byte_get_det_keypoints"):
        assert name in lib.EXPORTS and getattr(L, name).argtypes is not None
    # every argument is checked before the device is touched: no context, no call
    assert L.ss_byte_set_pose(None, 1, 17, None, 0.5, 0.25, 0.5, 3) == lib.SS_ERR_INVALID
    assert L.ss_byte_update_group_kpts(None, 1, None, None, None, 51, 0, None, None, None) == lib.SS_ERR_INVALID
    assert L.ss_byte_get_keypoints(None, 0, 256, None, None) == lib.SS_ERR_INVALID
    assert L.ss_byte_get_det_keypoints(None, 0, 0, None, None) == lib.SS_ERR_INVALID
