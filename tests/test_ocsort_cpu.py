"""OC-SORT (docs/OCSORT.md): the CPU reference (tests/ocsort_ref.py) on hand-built sequences with hand-derived outcomes, one branch
each (tests/ocsort_scenes.py); ss_asin; the 7x7 Joseph update against a NumPy filter; the configuration, YOLO(tracker_type="ocsort")
validation and the CLI's --tracker ocsort.  The same scenarios run on the device in tests/test_gpu_ocsort.py."""
import copy
import math

import numpy as np
import pytest

from strongsort_yolo_amd.config import OCSortConfig, ByteTrackConfig, byte_config, ocsort_config
from tests.ocsort_ref import OCSortRef, R_DIAG, box_to_z, iou_matrix, kf_init, kf_oru, kf_predict, kf_update, ss_asin
from tests.ocsort_scenes import EDGE_SIZES, SCENARIOS, F, box, crossing, edge_pair


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_reference_scenario(name):
    frames, cfg, check = SCENARIOS[name]()
    ref = OCSortRef(cfg)
    rows = [ref.update(d) for d in frames]
    for r, d in zip(rows, frames):
        assert r.dtype == np.float32 and r.shape[1] == 8
        assert ((r[:, 7] >= 0) & (r[:, 7] < max(len(d), 1))).all()                     # det_idx >= 0 always
    check(rows, ref)


def test_oru_state_is_the_refiltered_one_and_not_a_plain_update():
    frames, cfg, _ = SCENARIOS["oru_straight_line"]()
    ref = OCSortRef(cfg)
    for d in frames[:-1]:
        ref.update(d)
    t = ref.trackers[0]
    assert t.frozen and t.tsu == 3
    xf, Pf, z1 = list(t.xf), list(t.Pf), box_to_z(t.lobs)
    xl, Pl = kf_predict(t.x, t.P)                                                     # the live filter, predicted to frame 8
    ref.update(frames[-1])
    z2 = box_to_z([float(v) for v in frames[-1][0, :4]])
    x, P = kf_update(*kf_oru(xf, Pf, z1, z2, 4), z2)
    assert t.x == x and t.P == P and not t.frozen
    plain, plainP = kf_update(xl, Pl, z2)
    # on a straight line both means end close to the line (10 px a frame in x, 5 in y), but not on the same bits, and the
    # re-filtered covariance has seen four more observations: every variance is smaller than after the plain update
    assert t.x != plain and abs(t.x[4] - 10.0) < 0.5 and abs(t.x[5] - 5.0) < 0.5
    print("ORU - plain, mean:", max(abs(a - b) for a, b in zip(t.x, plain)), "variances:", [(t.P[i * 8], plainP[i * 8]) for i in range(7)])
    assert all(t.P[i * 8] < plainP[i * 8] for i in range(7))


def test_iou_alone_swaps_the_ids_at_the_crossing():
    frames, cfg = crossing(inertia=0.0)
    ref = OCSortRef(cfg)
    rows = [ref.update(d) for d in frames]
    assert all({int(r[7]): int(r[4]) for r in rw} == {0: 1, 1: 2} for rw in rows[:-1])
    assert {int(r[7]): int(r[4]) for r in rows[-1]} == {0: 2, 1: 1}                   # with inertia = 0.2: {0: 1, 1: 2} (the scenario)


def test_shortcut_and_lsap_give_the_same_pairs_where_both_apply():
    """Separated boxes: every row and track has one partner above the threshold, so the shortcut applies; the LSAP of the same
    matrix (forced by a threshold the shortcut's test cannot pass: a second, far frame keeps it off) finds the same pairs."""
    from tests.ocsort_ref import lsap
    frames = edge_pair(32, 33)
    d2 = frames[1][np.unique(frames[1], axis=0, return_index=True)[1]]                # without the repeated row: the shortcut's case
    ref = OCSortRef(OCSortConfig())
    ref.update(frames[0])
    twin = copy.deepcopy(ref)
    rows = ref.update(d2)
    assert ref.counters["shortcut"] == 1 and ref.counters["lsap"] == 0
    for t in twin.trackers:                                                           # the same frame by hand: predict, IoU, LSAP
        t.x, t.P = kf_predict(t.x, t.P)
    from tests.ocsort_ref import x_to_box
    iou = iou_matrix(d2[:, :4].astype(np.float64), [x_to_box(t.x) for t in twin.trackers])
    pairs = {(r, k) for r, k in lsap(-iou) if not iou[r, k] < 0.3}
    assert pairs == {(r, k) for r, k in zip(*np.nonzero(iou > 0.3))} and len(pairs) == 32
    assert sorted(int(i) for i in rows[:, 4]) == list(range(1, 33))


@pytest.mark.parametrize("n_tracks,n_rows", EDGE_SIZES)
def test_edge_pairs_are_an_lsap_of_that_size(n_tracks, n_rows):
    f1, f2 = edge_pair(n_tracks, n_rows)
    assert len(f1) == n_tracks and len(f2) == n_rows and len(np.unique(f2, axis=0)) == n_rows - 1
    ref = OCSortRef(OCSortConfig())
    ref.update(f1)
    ref.update(f2)
    assert ref.counters["lsap"] == 1 and ref.counters["shortcut"] == 0


def test_ss_asin_is_within_1e_12_of_libm():
    grid = np.concatenate([np.linspace(-1.0, 1.0, 400001), [-1.0, -0.5, 0.0, 0.5, 1.0, np.nextafter(0.5, 1), np.nextafter(-0.5, -1)]])
    got = ss_asin(grid)
    err = max(abs(float(g) - math.asin(float(c))) for g, c in zip(got, grid))
    print(f"ss_asin: max |error| {err:.3e} on {len(grid)} points")
    assert err <= 1e-12
    assert float(ss_asin(1.0)) == math.pi / 2 and float(ss_asin(-1.0)) == -math.pi / 2 and float(ss_asin(0.0)) == 0.0
    assert abs(float(ss_asin(0.5)) - math.pi / 6) <= 1e-15


def test_ss_asin_header_and_reference_agree_on_every_bit(tmp_path):
    """csrc/ss_asin.h built by a host compiler (no contraction, as the library) against tests/ocsort_ref.ss_asin."""
    import os
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "asin_host")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "clang++"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", os.path.join(here, "asin_host_main.cpp"), "-o", exe])
    rng = np.random.default_rng(3)
    grid = np.concatenate([np.linspace(-1.0, 1.0, 20001), rng.uniform(-1.0, 1.0, 20000), [0.5, -0.5, np.nextafter(0.5, 1), -0.0, 1e-300]])
    out = subprocess.run([exe], input=grid.tobytes(), stdout=subprocess.PIPE, check=True).stdout
    assert out == np.ascontiguousarray(ss_asin(grid), np.float64).tobytes()


def test_joseph_update_matches_a_numpy_filter():
    """The restatement, not the bits: the 7x7 Joseph update within 1e-9 relative of inv-based NumPy on random SPD inputs."""
    rng = np.random.default_rng(7)
    H = np.eye(4, 7)
    R = np.diag(R_DIAG)
    for _ in range(50):
        A = rng.standard_normal((7, 7))
        P = A @ A.T + 7.0 * np.eye(7)
        x, z = rng.standard_normal(7) * 50.0, rng.standard_normal(4) * 50.0
        S = H @ P @ H.T + R
        K = P @ H.T @ np.linalg.inv(S)
        xe = x + K @ (z - H @ x)
        IKH = np.eye(7) - K @ H
        Pe = IKH @ P @ IKH.T + K @ R @ K.T
        xg, Pg = kf_update(list(x), list(P.reshape(-1)), list(z))
        assert np.abs(np.array(xg) - xe).max() <= 1e-9 * np.abs(xe).max()
        assert np.abs(np.array(Pg).reshape(7, 7) - Pe).max() <= 1e-9 * np.abs(Pe).max()
    x0, P0 = kf_init([1.0, 2.0, 3.0, 4.0])
    x1, P1 = kf_predict(x0, P0)
    Fm = np.eye(7)
    Fm[0, 4] = Fm[1, 5] = Fm[2, 6] = 1.0
    Pe = Fm @ np.array(P0).reshape(7, 7) @ Fm.T + np.diag([1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 0.0001])
    assert np.array_equal(np.array(P1).reshape(7, 7), Pe) and x1 == x0


def test_ids_count_per_stream_and_restart_on_reset():
    a, b = OCSortRef(), OCSortRef()
    assert [int(i) for i in a.update(F(box(0), box(200)))[:, 4]] == [2, 1]            # newest first
    assert [int(i) for i in b.update(F(box(0)))[:, 4]] == [1]                         # a counter per stream (O-08)
    a.reset()
    assert [int(i) for i in a.update(F(box(0)))[:, 4]] == [1]


def test_config_defaults_and_validation():
    c = OCSortConfig()
    assert (c.det_thresh, c.low_thresh, c.max_age, c.min_hits, c.iou_threshold, c.delta_t, c.inertia) == (0.25, 0.1, 30, 3, 0.3, 3, 0.2)
    assert c.use_byte is False and (c.max_tracks, c.max_dets) == (256, 128)
    assert c.det_thresh == ByteTrackConfig().track_high_thresh
    for bad in (dict(delta_t=0), dict(delta_t=9), dict(max_tracks=300), dict(max_dets=129), dict(max_age=0), dict(iou_threshold=0.0),
                dict(inertia=-0.1), dict(min_hits=-1), dict(low_thresh=0.5)):
        with pytest.raises(ValueError):
            OCSortConfig(**bad)
    assert OCSortConfig(delta_t=1).delta_t == 1 and OCSortConfig(delta_t=8).delta_t == 8
    assert isinstance(ocsort_config("ocsort"), OCSortConfig) and ocsort_config("ocsort", use_byte=True).use_byte
    assert ocsort_config("bytetrack") is None and ocsort_config("strongsort") is None
    assert byte_config("ocsort") is None                                              # never a ByteTrackConfig
    assert byte_config("strongsort") is None and byte_config("botsort").kalman == "xywh" and byte_config("bytetrack").kalman == "xyah"
    for kw in (dict(camera_motion=True), dict(with_reid=True), dict(with_pose=True)):
        with pytest.raises(ValueError):
            ocsort_config("ocsort", **kw)
    with pytest.raises(ValueError):
        ocsort_config("bytetrack", use_byte=True)
    with pytest.raises(ValueError):
        ocsort_config("deepocsort")


def test_binding_has_the_ocsort_entries():
    import ctypes
    from strongsort_yolo_amd import lib
    for n in ("ss_ocsort_create", "ss_ocsort_destroy", "ss_ocsort_update_group", "ss_ocsort_update", "ss_ocsort_reset", "ss_ocsort_get_tracks"):
        assert n in lib.EXPORTS
    assert ctypes.sizeof(lib.ss_ocsort_config) == 56 and ctypes.sizeof(lib.ss_byte_config) == 72
    c = lib.make_ocsort_config(OCSortConfig(use_byte=True, delta_t=5))
    assert (c.det_thresh, c.low_thresh, c.iou_threshold, c.inertia) == (0.25, 0.1, 0.3, 0.2)
    assert (c.max_age, c.min_hits, c.delta_t, c.use_byte, c.max_tracks, c.max_dets) == (30, 3, 5, 1, 256, 128)
    lib.build()
    L = lib.load()
    out = (ctypes.c_float * 8)()
    assert L.ss_ocsort_create(None, ctypes.byref(c)) == lib.SS_ERR_INVALID            # checked before the device is touched
    assert L.ss_ocsort_update_group(None, 1, None, None, None, None) == lib.SS_ERR_INVALID
    assert L.ss_ocsort_reset(None, 0) == lib.SS_ERR_INVALID and L.ss_ocsort_destroy(None) == lib.SS_ERR_INVALID
    assert L.ss_ocsort_get_tracks(None, 0, 0, None, None, None, None, None, None, None, None, None, None, None, out, None) == lib.SS_ERR_INVALID


def test_yolo_ocsort_is_validated():
    import warnings
    from strongsort_yolo_amd.yolo import YOLO
    m = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="ocsort")
    assert m.tracker_type == "ocsort" and m._pipe_kw["tracker"] == "ocsort" and "ocsort_use_byte" not in m._pipe_kw
    assert YOLO("yolov8n.pt", random_init_ok=True, tracker_type="ocsort", ocsort_use_byte=True)._pipe_kw["ocsort_use_byte"] is True
    for kw in (dict(camera_motion=True), dict(with_reid=True), dict(with_pose=True)):
        with pytest.raises(ValueError):
            YOLO("yolo11n-pose.pt", random_init_ok=True, tracker_type="ocsort", **kw)
    with pytest.raises(ValueError):
        YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack", ocsort_use_byte=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m._check_tracker("ocsort.yaml")                                               # the model's own: quiet
        m._check_tracker("botsort.yaml")                                              # another family: tracker_type rules, said once
        m._check_tracker("bytetrack.yaml")
    said = [x for x in w if issubclass(x.category, RuntimeWarning)]
    assert len(said) == 1 and "OCSortConfig" in str(said[0].message)
    with pytest.raises(ValueError):
        m._check_tracker("deepocsort.yaml")


def test_cli_ocsort_flags(monkeypatch):
    from strongsort_yolo_amd import cli
    monkeypatch.setattr(cli, "process_video", lambda job: job)
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--tracker", "ocsort"])
    assert job["tracker"] == "ocsort" and job["reid_weights"] is None and job["ocsort_use_byte"] is False
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--tracker", "ocsort", "--ocsort-use-byte"])
    assert job["ocsort_use_byte"] is True
    for extra in (["--camera-motion"], ["--with-reid"], ["--with-pose"]):
        with pytest.raises(SystemExit):
            cli.main(["--source", "synthetic:3", "--track", "--tracker", "ocsort"] + extra)
    with pytest.raises(SystemExit):
        cli.main(["--source", "synthetic:3", "--track", "--tracker", "bytetrack", "--ocsort-use-byte"])
