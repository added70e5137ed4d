"""Hybrid-SORT on the CPU (docs/HYBRIDSORT.md): the reference's scenes, one scene per cue, the five-component filter against a dense
NumPy 9 x 9 filter, the host-side checks of the C entries, the configuration, YOLO and the CLI.  No GPU."""
import ctypes

import numpy as np
import pytest

from strongsort_yolo_amd.config import (ByteTrackConfig, HybridSortConfig, OCSortConfig, TRACKER_TYPES, byte_config, deep_ocsort_config,
                                        hybridsort_config, ocsort_config)
from tests.hybridsort_ref import (HybridSortRef, assoc_matrix, box_to_z5, flt_to_dense, kf_init, kf_oru, kf_predict, kf_update)
from tests.hybridsort_scenes import CUES, SCENARIOS, crossing_people, cue_off
from tests.ocsort_ref import OCSortRef
from tests.ocsort_scenes import E, F, box


def _run(frames, cfg):
    ref = HybridSortRef(cfg)
    return [ref.update(d) for d in frames], ref


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_reference_scenario(name):
    frames, cfg, check = SCENARIOS[name]()
    rows, ref = _run(frames, cfg)
    check(rows, ref)
    assert not ref.capacity_error


@pytest.mark.parametrize("name", sorted(CUES))
def test_each_cue_decides_its_scene_and_switching_it_off_changes_the_ids(name):
    frames, cfg, off, check = CUES[name]()
    rows_on, ref_on = _run(frames, cfg)
    check(rows_on, ref_on, True)
    rows_off, ref_off = _run(frames, cue_off(cfg, off))
    check(rows_off, ref_off, False)
    assert any(a.tobytes() != b.tobytes() for a, b in zip(rows_on, rows_off))


def test_hmiou_worked_numbers():
    row, side, below = [0.0, 0.0, 100.0, 200.0], [30.0, 0.0, 130.0, 200.0], [0.0, 60.0, 100.0, 260.0]
    a, iou = assoc_matrix([row], [side, below], "hmiou")
    assert iou[0, 0] == iou[0, 1] == 14000.0 / 26000.0
    assert a[0, 0] == iou[0, 0] and abs(a[0, 1] - 0.538461538 * 140.0 / 260.0) < 1e-8
    assert assoc_matrix([row], [[500.0, 0.0, 600.0, 200.0]], "hmiou")[0][0, 0] == 0.0        # no overlap: 0, not a negative ratio
    assert assoc_matrix([row], [side], "iou")[0][0, 0] == iou[0, 0]


# ---- the filter ------------------------------------------------------------------------------------------------------------------
def _dense_model():
    Fm, H = np.eye(9), np.zeros((5, 9))
    for i in range(4):
        Fm[i, 5 + i] = 1.0
    for i in range(5):
        H[i, i] = 1.0
    Q = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 1e-4, 1e-4])
    R = np.diag([1.0, 1.0, 10.0, 10.0, 10.0])
    P0 = np.diag([10.0] * 5 + [1e4] * 4)
    return Fm, H, Q, R, P0


def _dense_update(x, P, z, H, R):
    K = P @ H.T @ np.linalg.inv(H @ P @ H.T + R)
    x = x + K @ (np.asarray(z) - H @ x)
    A = np.eye(9) - K @ H
    return x, A @ P @ A.T + K @ R @ K.T


def _close(f, x, P):
    fx, fP = flt_to_dense(f)
    np.testing.assert_allclose(fx, x, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(np.array(fP).reshape(9, 9), P, rtol=1e-9, atol=1e-9)


def test_five_components_equal_a_dense_joseph_filter_over_a_sequence_with_gaps():
    Fm, H, Q, R, P0 = _dense_model()
    rng = np.random.default_rng(5)
    z = box_to_z5([100.0, 50.0, 160.0, 200.0], 0.8)
    f, x, P = kf_init(z), np.array(z + [0.0] * 4), P0.copy()
    worst = 0.0
    for k in range(200):
        f = kf_predict(f)
        x, P = Fm @ x, Fm @ P @ Fm.T + Q
        if k % 17 not in (5, 6, 7):                                 # gaps of three frames
            b = [100.0 + 3.0 * k + rng.normal(0, 2), 50.0 + k + rng.normal(0, 2), 160.0 + 3.2 * k + rng.normal(0, 2), 200.0 + 1.5 * k + rng.normal(0, 2)]
            z = box_to_z5(b, float(np.clip(0.7 + 0.2 * np.sin(k / 9.0) + rng.normal(0, 0.05), 0, 1)))
            f = kf_update(f, z)
            x, P = _dense_update(x, P, z, H, R)
        _close(f, x, P)
        block = np.zeros((9, 9), bool)
        for i in range(4):
            block[np.ix_([i, 5 + i], [i, 5 + i])] = True
        block[4, 4] = True
        worst = max(worst, float(np.abs(P[~block]).max()))
        assert all(v == 0.0 and not np.signbit(v) for v in np.array(flt_to_dense(f)[1]).reshape(9, 9)[~block])
    assert worst < 1e-12                                            # the dense filter's off-block entries are rounding noise


def test_oru_state_equals_the_dense_filter_refiltered_over_the_virtual_observations():
    frames, cfg, _ = SCENARIOS["oru_straight_line"]()
    _, ref = _run(frames, cfg)
    assert ref.counters["oru_tracks"] == 1
    Fm, H, Q, R, P0 = _dense_model()
    z = [box_to_z5([float(v) for v in fr[0, :4]], fr[0, 4]) for fr in frames if len(fr)]
    x, P = np.array(z[0] + [0.0] * 4), P0.copy()
    for zi in z[1:4]:                                               # frames 2..4; frame 1 is the birth
        x, P = Fm @ x, Fm @ P @ Fm.T + Q
        x, P = _dense_update(x, P, zi, H, R)
    x, P = Fm @ x, Fm @ P @ Fm.T + Q                                # frozen after the predict of the first missed frame
    z1, z2, g = z[3], z[4], 4
    w1, h1, w2, h2 = np.sqrt(z1[2] * z1[4]), np.sqrt(z1[2] / z1[4]), np.sqrt(z2[2] * z2[4]), np.sqrt(z2[2] / z2[4])
    for i in range(1, g + 1):
        w, h = w1 + i * (w2 - w1) / g, h1 + i * (h2 - h1) / g
        v = [z1[0] + i * (z2[0] - z1[0]) / g, z1[1] + i * (z2[1] - z1[1]) / g, w * h, z1[3] + i * (z2[3] - z1[3]) / g, w / h]
        x, P = _dense_update(x, P, v, H, R)
        if i < g:
            x, P = Fm @ x, Fm @ P @ Fm.T + Q
    x, P = _dense_update(x, P, z2, H, R)                            # O-02
    t = ref.tracks()
    np.testing.assert_allclose(t["x"][0], x, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(t["P"][0].reshape(9, 9), P, rtol=1e-9, atol=1e-9)
    plain = kf_update(kf_predict(kf_predict(kf_predict(kf_predict(ref_frozen(frames, cfg))))), z2)
    assert not np.allclose(flt_to_dense(plain)[0], t["x"][0], rtol=1e-3, atol=1e-3)      # and not a plain update of the drifted filter


def ref_frozen(frames, cfg):
    ref = HybridSortRef(cfg)
    for d in frames[:4]:
        ref.update(d)
    return list(ref.trackers[0].f)


def test_kf_oru_counts_and_interpolates_the_confidence():
    z1, z2 = box_to_z5([0.0, 0.0, 40.0, 80.0], 0.9), box_to_z5([30.0, 0.0, 70.0, 80.0], 0.3)
    cnt = dict(oru=0)
    f = kf_oru(kf_init(z1), z1, z2, 3, cnt)
    assert cnt["oru"] == 3 and f[18] < 0.6 and f[19] < 0.0             # the state followed 0.7, 0.5, 0.3 down


def test_ids_count_per_stream_and_restart_on_reset():
    a, b = HybridSortRef(), HybridSortRef()
    assert [int(i) for i in a.update(F(box(0), box(200)))[:, 4]] == [2, 1]
    assert [int(i) for i in b.update(F(box(0)))[:, 4]] == [1]
    a.reset()
    assert [int(i) for i in a.update(F(box(0)))[:, 4]] == [1] and a.update(E).shape == (0, 8)


def test_identity_switches_against_ocsort_on_crossing_people():
    """A figure for docs/HYBRIDSORT.md §5, not a gate: the same rows through both references, scored by tests/moteval_ref.py."""
    from tests.moteval_ref import evaluate
    seed = 0
    dets, gts = crossing_people(seed)
    gt = np.array([[k, g[0], g[1], g[2], g[3], g[4], 1.0, 0.0] for k, gs in enumerate(gts) for g in gs])
    out = {}
    for name, ref in (("hybridsort", HybridSortRef(HybridSortConfig())), ("ocsort", OCSortRef(OCSortConfig(use_byte=True)))):
        rows = [[k, r[4], r[0], r[1], r[2], r[3], r[6], 0.0] for k, d in enumerate(dets) for r in ref.update(d)]
        out[name] = evaluate(gt, np.array(rows))
    print("crossing_people seed", seed, {k: (v["IDSW"], round(v["MOTA"], 3)) for k, v in out.items()})
    assert all(v["TP"] > 0 for v in out.values())


# ---- configuration, binding, YOLO, CLI ---------------------------------------------------------------------------------------------
def test_config_defaults_and_validation():
    c = HybridSortConfig()
    assert (c.det_thresh, c.low_thresh, c.max_age, c.min_hits, c.iou_threshold, c.delta_t, c.inertia) == (0.25, 0.1, 30, 3, 0.3, 3, 0.05)
    assert c.use_byte is True and c.asso == "hmiou" and (c.tcm_first_weight, c.tcm_byte_weight) == (1.0, 1.0)
    assert (c.max_tracks, c.max_dets) == (256, 128) and c.det_thresh == ByteTrackConfig().track_high_thresh
    with pytest.raises(Exception):
        c.asso = "iou"                                              # frozen
    for bad in (dict(delta_t=0), dict(delta_t=9), dict(max_tracks=300), dict(max_dets=129), dict(max_age=0), dict(iou_threshold=0.0),
                dict(iou_threshold=1.5), dict(inertia=-0.1), dict(min_hits=-1), dict(low_thresh=0.5), dict(asso="giou"),
                dict(tcm_first_weight=-1.0), dict(tcm_byte_weight=-0.5), dict(tcm_first_weight=float("nan"))):
        with pytest.raises(ValueError):
            HybridSortConfig(**bad)
    assert HybridSortConfig(tcm_first_weight=0.0, tcm_byte_weight=0.0, asso="iou", delta_t=8).delta_t == 8
    assert "hybridsort" in TRACKER_TYPES
    h = hybridsort_config("hybridsort", "iou", False)
    assert isinstance(h, HybridSortConfig) and h.asso == "iou" and h.use_byte is False
    assert hybridsort_config("hybridsort").use_byte is True
    for other in ("strongsort", "bytetrack", "botsort", "ocsort", "deep_ocsort"):
        assert hybridsort_config(other) is None
    assert ocsort_config("hybridsort") is None and deep_ocsort_config("hybridsort") is None and byte_config("hybridsort") is None
    for kw in (dict(camera_motion=True), dict(with_reid=True), dict(with_pose=True), dict(ocsort_use_byte=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            hybridsort_config("hybridsort", **kw)
    for kw in (dict(asso="iou"), dict(use_byte=False)):
        with pytest.raises(ValueError, match="hybridsort"):
            hybridsort_config("ocsort", **kw)
    with pytest.raises(ValueError):
        hybridsort_config("hybrid_sort")
    with pytest.raises(ValueError):
        hybridsort_config("hybridsort", asso="giou")


def test_binding_and_host_side_checks_without_a_device():
    from strongsort_yolo_amd import lib
    names = ("ss_hybridsort_create", "ss_hybridsort_destroy", "ss_hybridsort_update_group", "ss_hybridsort_update", "ss_hybridsort_reset",
             "ss_hybridsort_get_tracks")
    for n in names:
        assert n in lib.EXPORTS
    assert ctypes.sizeof(lib.ss_hybridsort_config) == 6 * 8 + 7 * 4 + 4                 # 6 doubles + 7 ints, padded to 8
    c = lib.make_hybridsort_config(HybridSortConfig(use_byte=False, asso="iou", delta_t=5, tcm_byte_weight=0.5))
    assert (c.det_thresh, c.low_thresh, c.iou_threshold, c.inertia, c.tcm_first_weight, c.tcm_byte_weight) == (0.25, 0.1, 0.3, 0.05, 1.0, 0.5)
    assert (c.max_age, c.min_hits, c.delta_t, c.use_byte, c.hmiou, c.max_tracks, c.max_dets) == (30, 3, 5, 0, 0, 256, 128)
    assert lib.make_hybridsort_config(HybridSortConfig()).hmiou == 1
    lib.build()
    L = lib.load()
    INV = lib.SS_ERR_INVALID
    last = lambda: L.ss_last_error(None).decode()
    # every bad field is refused by the argument check, before the context is looked at (so before any device call)
    good = dict(det_thresh=0.25, low_thresh=0.1, iou_threshold=0.3, inertia=0.05, tcm_first_weight=1.0, tcm_byte_weight=1.0, max_age=30,
                min_hits=3, delta_t=3, use_byte=1, hmiou=1, max_tracks=256, max_dets=128)
    for bad in (dict(max_tracks=0), dict(max_tracks=257), dict(max_dets=0), dict(max_dets=129), dict(delta_t=0), dict(delta_t=9),
                dict(max_age=0), dict(min_hits=-1), dict(iou_threshold=0.0), dict(iou_threshold=1.01), dict(iou_threshold=float("nan")),
                dict(inertia=-1.0), dict(inertia=float("nan")), dict(tcm_first_weight=-0.1), dict(tcm_byte_weight=-0.1),
                dict(tcm_byte_weight=float("nan")), dict(low_thresh=0.3), dict(use_byte=2), dict(use_byte=-1), dict(hmiou=2)):
        cfg = lib.ss_hybridsort_config(**dict(good, **bad))
        assert L.ss_hybridsort_create(None, ctypes.byref(cfg)) == INV and "1 <= max_tracks <= 256" in last(), bad
    assert L.ss_hybridsort_create(None, None) == INV and "null argument" in last()
    cfg = lib.ss_hybridsort_config(**good)
    assert L.ss_hybridsort_create(None, ctypes.byref(cfg)) == INV and "null context" in last()      # a sound configuration gets that far
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                                       # dummy non-null pointers: never read, the refusal comes first
    upd = lambda n=1, d=p, nd=p, o=p, no=p: L.ss_hybridsort_update_group(None, n, d, nd, o, no)
    for kw in (dict(d=None), dict(nd=None), dict(o=None), dict(no=None)):
        assert upd(**kw) == INV and "null argument" in last(), kw
    for n in (0, -1, 33):
        assert upd(n=n) == INV and "n_frames" in last(), n
    assert upd() == INV and "null context" in last()
    assert L.ss_hybridsort_update(None, None, p, p, p) == INV and "null argument" in last()
    assert L.ss_hybridsort_update(None, p, p, p, p) == INV and "null context" in last()
    assert L.ss_hybridsort_reset(None, 0) == INV and L.ss_hybridsort_destroy(None) == INV
    out = (ctypes.c_float * 8)()
    assert L.ss_hybridsort_get_tracks(None, 0, 0, *([None] * 11), out, None, None, None) == INV
    assert L.ss_hybridsort_get_tracks(None, 0, -1, *([None] * 15)) == INV


def test_yolo_hybridsort_is_validated():
    import warnings
    from strongsort_yolo_amd.yolo import YOLO
    assert "hybridsort.yaml" in YOLO.TRACKERS and "hybrid_sort.yaml" not in YOLO.TRACKERS
    m = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="hybridsort")
    assert m.tracker_type == "hybridsort" and m._pipe_kw["tracker"] == "hybridsort"
    assert "hybrid_asso" not in m._pipe_kw and "hybrid_use_byte" not in m._pipe_kw and "ocsort_use_byte" not in m._pipe_kw
    m2 = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="hybridsort", hybrid_asso="iou", hybrid_use_byte=False)
    assert m2._pipe_kw["hybrid_asso"] == "iou" and m2._pipe_kw["hybrid_use_byte"] is False
    for kw, word in ((dict(camera_motion=True), "camera_motion"), (dict(with_reid=True), "with_reid"), (dict(with_pose=True), "with_pose"),
                     (dict(with_reid=True, reid_model="auto"), "with_reid"), (dict(reid_model="auto"), "reid_model"),
                     (dict(ocsort_use_byte=True), "ocsort_use_byte"), (dict(gmc_method="sparseOptFlow"), "gmc_method"),
                     (dict(camera_motion=True, gmc_method="sparseOptFlow"), "camera_motion"), (dict(track_bank=True), "track_bank"),
                     (dict(hybrid_asso="giou"), "asso")):
        with pytest.raises(ValueError, match=word):
            YOLO("yolo11n-pose.pt", random_init_ok=True, tracker_type="hybridsort", **kw)
    with pytest.raises(ValueError, match="oriented-box"):
        YOLO("yolo11n-obb.pt", random_init_ok=True, tracker_type="hybridsort")
    for kw in (dict(hybrid_asso="iou"), dict(hybrid_use_byte=False)):
        with pytest.raises(ValueError, match="hybridsort"):
            YOLO("yolov8n.pt", random_init_ok=True, tracker_type="ocsort", **kw)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m._check_tracker("hybridsort.yaml")                         # the model's own: quiet
        m._check_tracker("ocsort.yaml")                             # another family: tracker_type rules, said once
        m._check_tracker("botsort.yaml")
    said = [x for x in w if issubclass(x.category, RuntimeWarning)]
    assert len(said) == 1 and "HybridSortConfig" in str(said[0].message)
    with pytest.raises(ValueError):
        m._check_tracker("hybrid_sort.yaml")


def test_track_bank_refusal_names_the_tracker():
    from strongsort_yolo_amd import mtmc
    why = mtmc.bank_refusal("hybridsort")
    assert why and "hybridsort" in why and mtmc.NO_FEATURES in why


def test_cli_hybridsort_flags(monkeypatch):
    from strongsort_yolo_amd import cli
    monkeypatch.setattr(cli, "process_video", lambda job: job)
    base = ["--source", "synthetic:3", "--track", "--tracker", "hybridsort"]
    (job,) = cli.main(base)
    assert job["tracker"] == "hybridsort" and job["reid_weights"] is None
    assert job["hybrid_asso"] == "hmiou" and job["hybrid_no_byte"] is False and job["ocsort_use_byte"] is False
    (job,) = cli.main(base + ["--hybrid-asso", "iou", "--hybrid-no-byte"])
    assert job["hybrid_asso"] == "iou" and job["hybrid_no_byte"] is True
    for extra in (["--camera-motion"], ["--with-reid"], ["--with-pose"], ["--ocsort-use-byte"], ["--with-reid", "--reid-model", "auto"],
                  ["--camera-motion", "--gmc-method", "sparseOptFlow"], ["--hybrid-asso", "giou"], ["--weights", "yolo11n-obb.pt"]):
        with pytest.raises(SystemExit):
            cli.main(base + extra)
    with pytest.raises(SystemExit):
        cli.main(["--source", "synthetic:3", "--source", "synthetic:4", "--track", "--tracker", "hybridsort", "--mtmc"])
    for extra in (["--hybrid-asso", "iou"], ["--hybrid-no-byte"]):
        with pytest.raises(SystemExit):
            cli.main(["--source", "synthetic:3", "--track", "--tracker", "ocsort"] + extra)
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--tracker", "ocsort"])      # the other trackers' jobs carry the defaults
    assert job["hybrid_asso"] == "hmiou" and job["hybrid_no_byte"] is False
