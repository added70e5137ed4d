"""BoT-SORT with camera-motion compensation (docs/BYTETRACK.md §1b, G-01..G-06) on the CPU: step 3b of the reference
(tests/botsort_gmc_ref.py) against the dense matrix form, a pan that only GMC survives, the no-warp identity, and the
YOLO / CLI / ABI surface.  The device runs are in tests/test_gpu_botsort_gmc.py."""
import os

import numpy as np
import pytest

from strongsort_yolo_amd.config import ByteTrackConfig
from tests.botsort_gmc_ref import BotSortGmcRef, gmc_apply
from tests.bytetrack_ref import ByteTrackRef
from tests.test_bytetrack_cpu import F, box, byte_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _warp(theta, tx, ty, it=5.0):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([c, -s, tx, s, c, ty, it, 0.0])


def _dense(mean, cov, w):
    R8 = np.kron(np.eye(4), np.array([[w[0], w[1]], [w[3], w[4]]]))
    m = R8 @ np.asarray(mean)
    m[:2] += [w[2], w[5]]
    return m, R8 @ np.asarray(cov).reshape(8, 8) @ R8.T


def _state(rng):
    mean = np.concatenate([rng.uniform(50, 1200, 2), rng.uniform(20, 200, 2), rng.normal(0, 3, 4)])
    A = rng.normal(0, 4, (8, 8))
    return mean, (A @ A.T + np.eye(8)).reshape(64)


def test_step_3b_equals_the_dense_product():
    rng = np.random.default_rng(0)
    for _ in range(200):
        mean, cov = _state(rng)
        w = _warp(rng.uniform(-0.2, 0.2), rng.uniform(-40, 40), rng.uniform(-40, 40))
        m, P = gmc_apply(mean, cov, w)
        dm, dP = _dense(mean, cov, w)
        assert np.allclose(m, dm, rtol=1e-12, atol=0) and np.allclose(np.reshape(P, (8, 8)), dP, rtol=1e-12, atol=1e-12 * np.abs(dP).max())


def test_step_3b_pure_translation_is_exact():
    rng = np.random.default_rng(1)
    for _ in range(50):
        mean, cov = _state(rng)
        t = rng.uniform(-40, 40, 2)
        m, P = gmc_apply(mean, cov, [1.0, 0.0, t[0], 0.0, 1.0, t[1], 3.0, 0.0])
        exp = mean.copy()
        exp[0] += t[0]
        exp[1] += t[1]
        assert np.asarray(m).tobytes() == exp.tobytes() and np.asarray(P).tobytes() == cov.tobytes()


def _pan_frames():
    """Three people standing still; between frames 5 and 6 the camera pans, so the scene jumps 60 px to the left in the
    image.  The boxes are 40 px wide: the old and new boxes do not overlap."""
    xs = [100.0, 400.0, 800.0]
    return [F(*[box(x - (60.0 if k >= 5 else 0.0)) for x in xs]) for k in range(9)]


def _pan_warps(exact):
    w = []
    for k in range(9):
        if k == 0:
            w.append(None)                                      # first frame: no predecessor
        elif k == 5 and exact:
            w.append([1.0, 0.0, -60.0, 0.0, 1.0, 0.0, 4.0, 0.0])
        else:
            w.append([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 2.0 if exact else -1.0, 0.0])
    return w


def test_a_pan_renumbers_without_gmc_and_keeps_ids_with_it():
    plain, gmc = BotSortGmcRef(), BotSortGmcRef()
    frames = _pan_frames()
    rows_p = [plain.update(d, w) for d, w in zip(frames, _pan_warps(False))]
    rows_g = [gmc.update(d, w) for d, w in zip(frames, _pan_warps(True))]
    assert [sorted(int(i) for i in r[:, 4]) for r in rows_g] == [[1, 2, 3]] * 9
    assert np.array_equal(rows_g[8][:, :4], frames[8][:, :4])   # the moved tracks sit on the detections
    assert len(rows_p[5]) == 0                                  # the jump: every track lost, three unconfirmed births
    assert sorted(int(i) for i in rows_p[8][:, 4]) == [4, 5, 6] and [t.id for t in plain.lost] == [1, 2, 3]


def test_unconfirmed_tracks_are_moved_too():
    """id 2 is born on frame 2 (unconfirmed); on frame 3 the camera pans 30 px: 1 - IoU of a 40 px box shifted by 30 is 6/7,
    fused 0.871 > 0.7, so only the moved unconfirmed track meets its detection again."""
    def run(warp):
        ref = BotSortGmcRef()
        ref.update(F(box(100)))
        ref.update(F(box(100), box(600)), [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 2.0, 0.0])
        assert [t.activated for t in ref.tracked] == [True, False]
        return ref, ref.update(F(box(70), box(570)), warp)
    ref, rows = run([1.0, 0.0, -30.0, 0.0, 1.0, 0.0, 3.0, 0.0])
    assert sorted(int(i) for i in rows[:, 4]) == [1, 2] and all(t.activated for t in ref.tracked)
    ref, rows = run(None)
    assert len(rows) == 0 and [t.id for t in ref.lost] == [1] and ref.next_id == 5     # id 2 removed, two unconfirmed births


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_no_warp_rows_equal_the_plain_tracker(seed):
    cfg = ByteTrackConfig(kalman="xywh")
    a, b = BotSortGmcRef(cfg), ByteTrackRef(cfg)
    none = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0, 0.0]
    for k, d in enumerate(byte_stream(seed, 150)):
        ra, rb = a.update(d, none if k % 2 else None), b.update(d)
        assert ra.tobytes() == rb.tobytes(), f"seed {seed} frame {k}"


def test_reference_refuses_xyah():
    with pytest.raises(ValueError):
        BotSortGmcRef(ByteTrackConfig(kalman="xyah"))


def test_yolo_botsort_with_camera_motion():
    from strongsort_yolo_amd.yolo import YOLO
    m = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", camera_motion=True)
    assert m._pipe_kw["cmc"] is True and m._pipe_kw["tracker"] == "botsort"
    with pytest.raises(ValueError):
        YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack", camera_motion=True)
    assert YOLO("yolov8n.pt", random_init_ok=True, camera_motion=True)._pipe_kw["cmc"] is True


def test_cli_camera_motion_flag(monkeypatch):
    from strongsort_yolo_amd import cli
    monkeypatch.setattr(cli, "process_video", lambda job: job)
    for tracker in ("strongsort", "botsort"):
        (job,) = cli.main(["--source", "synthetic:3", "--track", "--tracker", tracker, "--camera-motion"])
        assert job["camera_motion"] is True and job["tracker"] == tracker
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--tracker", "botsort"])
    assert job["camera_motion"] is False
    with pytest.raises(SystemExit):
        cli.main(["--source", "synthetic:3", "--track", "--tracker", "bytetrack", "--camera-motion"])


def test_cli_passes_camera_motion_to_the_model(monkeypatch):
    from strongsort_yolo_amd import cli, yolo
    seen = {}

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(yolo, "YOLO", fake)
    with pytest.raises(Stop):
        cli.process_video({"source": "synthetic:2", "track": True, "count": False, "tracker": "botsort", "camera_motion": True})
    assert seen["camera_motion"] is True and seen["tracker_type"] == "botsort"


def test_set_gmc_is_declared_and_exported():
    from strongsort_yolo_amd import lib
    src = open(os.path.join(ROOT, "include", "strongsort_hip.h")).read()
    assert "int ss_byte_set_gmc(ss_ctx* ctx, const double* d_warps);" in src
    assert "ss_byte_set_gmc" in lib.EXPORTS
    L = lib.load()
    assert L.ss_byte_set_gmc.argtypes is not None
