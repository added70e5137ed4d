"""Deep OC-SORT without a GPU (docs/DEEPOCSORT.md §5): the reference against OCSortRef, the hand-built scenes, adaptive weighting
against a NumPy restatement, the configuration, YOLO, the CLI and the ABI's argument checks."""
import numpy as np
import pytest

from strongsort_yolo_amd.config import (DeepOCSortConfig, OCSortConfig, byte_config, check_gmc_method, check_reid_model,
                                        deep_ocsort_config, ocsort_config)
from tests.deepocsort_ref import DeepOCSortRef, aw_weights, warp_filter
from tests.deepocsort_scenes import SCENES, FT, deep_stream, e, rot
from tests.ocsort_ref import OCSortRef
from tests.ocsort_scenes import SCENARIOS, F, box, crossing
from tests.test_bytetrack_cpu import byte_stream


def _as_deep(oc: OCSortConfig, **kw) -> DeepOCSortConfig:
    return DeepOCSortConfig(det_thresh=oc.det_thresh, max_age=oc.max_age, min_hits=oc.min_hits, iou_threshold=oc.iou_threshold,
                            delta_t=oc.delta_t, inertia=oc.inertia, **kw)


@pytest.mark.parametrize("name", sorted(n for n, f in SCENARIOS.items() if not f()[1].use_byte))
def test_without_appearance_it_is_ocsort_on_the_ocsort_scenes(name):
    frames, oc, _ = SCENARIOS[name]()
    a, b = DeepOCSortRef(_as_deep(oc, appearance=False)), OCSortRef(oc)
    for k, d in enumerate(frames):
        assert a.update(d).tobytes() == b.update(d).tobytes(), f"{name} frame {k}"
    ta, tb = a.tracks(), b.tracks()
    assert all(np.asarray(ta[k]).tobytes() == np.asarray(tb[k]).tobytes() for k in tb)


def test_without_appearance_it_is_ocsort_on_a_stream():
    frames = byte_stream(2, 64)
    a, b = DeepOCSortRef(DeepOCSortConfig(appearance=False)), OCSortRef(OCSortConfig())
    for k, d in enumerate(frames):
        assert a.update(d).tobytes() == b.update(d).tobytes(), f"frame {k}"
    assert b.counters["oru_tracks"] > 0 and b.counters["lsap"] > 0
    assert all(np.asarray(a.tracks()[k]).tobytes() == np.asarray(b.tracks()[k]).tobytes() for k in b.tracks())


@pytest.mark.parametrize("name", sorted(SCENES))
def test_hand_built_scenes(name):
    frames, feats, warps, cfg, check = SCENES[name]()
    ref = DeepOCSortRef(cfg)
    check([ref.update(d, f, w) for d, f, w in zip(frames, feats, warps)], ref)


def test_ocsort_swaps_the_crossing_that_appearance_keeps():
    frames, oc = crossing(inertia=0.0)
    ref = OCSortRef(oc)
    rows = [ref.update(d) for d in frames]
    assert {int(r[7]): int(r[4]) for r in rows[-1]} == {0: 2, 1: 1}                  # IoU alone swaps the ids


def test_cmc_moves_the_frozen_filter_the_ring_and_the_last_observation():
    """the scene of the same name, against the run without the warps: on the first warped frame the filter, its frozen copy, the
    last observation and the ring's entries are the unwarped ones moved once."""
    frames, feats, warps, cfg, _ = SCENES["cmc_moves_a_frozen_track"]()
    a, b = DeepOCSortRef(cfg), DeepOCSortRef(cfg)
    for k in range(5):
        a.update(frames[k], feats[k], warps[k]); b.update(frames[k], feats[k])
    w = [float(v) for v in warps[5][:6]]
    ta, tb = a.trackers[0], b.trackers[0]
    assert ta.frozen and ta.has_obs and sorted(ta.obs) == [1, 2, 3] and ta.age == 4
    xf, Pf, lobs, obs = list(ta.xf), list(ta.Pf), list(ta.lobs), {k: list(v) for k, v in ta.obs.items()}
    a.update(frames[5], feats[5], warps[5])
    mx, mP = warp_filter(w, xf, Pf)
    assert ta.xf == mx and ta.Pf == mP and ta.xf != xf
    cx, cy = w[0] * lobs[0] + w[1] * lobs[1] + w[2], w[3] * lobs[0] + w[4] * lobs[1] + w[5]
    assert ta.lobs[:2] == [float(np.float32(cx)), float(np.float32(cy))]
    assert all(ta.obs[k] != obs[k] for k in (1, 2, 3))                               # ages 4 - 3 .. 4
    # only the (x, y) and (vx, vy) blocks of P change (DO-03)
    # (the scene's blocks are multiples of the identity, which a rotation keeps: a filter with an uneven P shows the blocks)
    P0 = np.arange(49.0).reshape(7, 7) + np.arange(49.0).reshape(7, 7).T + 1.0
    x1, P1 = warp_filter(w, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0], list(P0.reshape(-1)))
    P1 = np.array(P1).reshape(7, 7)
    mask = np.zeros((7, 7), bool)
    mask[0:2, 0:2] = mask[4:6, 4:6] = True
    R = np.array([[w[0], w[1]], [w[3], w[4]]])
    assert np.array_equal(P0[~mask], P1[~mask]) and (P0[mask] != P1[mask]).all()
    assert np.allclose(P1[0:2, 0:2], R @ P0[0:2, 0:2] @ R.T, rtol=1e-14) and np.allclose(P1[4:6, 4:6], R @ P0[4:6, 4:6] @ R.T, rtol=1e-14)
    assert x1[2:4] == [3.0, 4.0] and x1[6] == 7.0 and np.allclose(x1[0:2], R @ [1.0, 2.0] + [w[2], w[5]]) and np.allclose(x1[4:6], R @ [5.0, 6.0])


def test_ring_entries_outside_the_window_stay():
    t_cfg = DeepOCSortConfig(min_hits=0, delta_t=2)
    ref = DeepOCSortRef(t_cfg)
    for k in range(3):
        ref.update(F(box(100 + 5 * k)), FT(e(0)))
    for _ in range(4):
        ref.update(F(), np.zeros((0, 512), np.float32))
    t = ref.trackers[0]
    before = {k: list(v) for k, v in t.obs.items()}
    assert t.age == 6 and max(before) == 2                                           # the newest entry is 4 ages old: outside 6 - 2 .. 6
    ref.update(F(), np.zeros((0, 512), np.float32), rot(0.1, 5.0, 5.0))
    assert {k: list(v) for k, v in t.obs.items()} == before and ref.counters["warp"] == 1


def test_reset_forgets_tracks_features_and_counters():
    frames, feats, warps, cfg, _ = SCENES["aw_one_row"]()
    ref = DeepOCSortRef(cfg)
    first = [ref.update(d, f) for d, f in zip(frames, feats)]
    assert ref.features().shape == (2, 512)
    ref.reset()
    assert ref.features().shape == (0, 512) and ref.frame_count == 0 and ref.next_id == 1
    again = [ref.update(d, f) for d, f in zip(frames, feats)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


def test_adaptive_weights_against_an_argsort_restatement():
    rng = np.random.default_rng(5)
    for H, T in ((1, 1), (1, 5), (5, 1), (2, 2), (7, 9), (33, 20)):
        for trial in range(20):
            E = rng.uniform(-0.3, 1.0, (H, T))
            E[rng.random((H, T)) < 0.4] = 0.0
            if trial == 0 and T >= 2:
                E[0] = 0.0                                                            # m1 == 0
            if trial == 1 and T >= 2:
                E[0, :2] = E[0].max() + 0.1                                           # m1 == m2
            w, aw = 0.75, float(rng.uniform(0.0, 0.9))
            W = np.full((H, T), w)
            if T >= 2:
                s = np.sort(E, axis=1)[:, ::-1]
                with np.errstate(all="ignore"):
                    f = np.where(s[:, 0] == 0.0, 0.0, 1.0 - np.maximum(s[:, 1] / s[:, 0] - aw, 0.0) / (1.0 - aw))
                W = W * f[:, None]
            if H >= 2:
                idx = np.argsort(-E, axis=0)
                m1, m2 = np.take_along_axis(E, idx[:1], 0)[0], np.take_along_axis(E, idx[1:2], 0)[0]
                with np.errstate(all="ignore"):
                    f = np.where(m1 == 0.0, 0.0, 1.0 - np.maximum(m2 / m1 - aw, 0.0) / (1.0 - aw))
                W = W * f[None, :]
            assert np.abs(aw_weights(E, w, aw) - W).max() <= 1e-12


def test_all_negative_similarities_follow_the_formula():
    """m1 < 0: m2 / m1 >= 1, so the factor is 1 - (m2 / m1 - aw) / (1 - aw) <= 0 (DO-08)"""
    W = aw_weights(np.array([[-0.2, -0.4]]), 0.75, 0.5)
    assert np.allclose(W, 0.75 * (1.0 - (2.0 - 0.5) / 0.5)) and (W < 0).all()


def test_streams_reach_every_branch_on_the_cpu():
    tot = {}
    for seed, n in ((0, 28), (2, 6)):
        frames, feats, warps = deep_stream(seed, 48, n_ids=n)
        ref = DeepOCSortRef()
        for d, f, w in zip(frames, feats, warps):
            ref.update(d, f, w)
        for k, v in ref.counters.items():
            tot[k] = tot.get(k, 0) + v
    for k in ("lsap_emb", "shortcut", "aw_rows", "aw_cols", "oru_tracks", "warp_frozen"):
        assert tot[k] > 0, k


def test_config_defaults_and_validation():
    c = DeepOCSortConfig()
    assert (c.det_thresh, c.max_age, c.min_hits, c.iou_threshold, c.delta_t, c.inertia) == (0.25, 30, 3, 0.3, 3, 0.2)
    assert (c.w_association_emb, c.alpha_fixed_emb, c.aw_param) == (0.75, 0.95, 0.5)
    assert c.appearance and c.dynamic_appearance and c.adaptive_weighting and (c.max_tracks, c.max_dets) == (256, 128)
    assert not hasattr(c, "use_byte")
    for bad in (dict(delta_t=0), dict(delta_t=9), dict(max_tracks=300), dict(max_dets=129), dict(max_age=0), dict(iou_threshold=0.0),
                dict(inertia=-0.1), dict(min_hits=-1), dict(w_association_emb=-0.1), dict(alpha_fixed_emb=1.1), dict(alpha_fixed_emb=-0.1),
                dict(aw_param=1.0), dict(aw_param=-0.1), dict(det_thresh=1.0)):
        with pytest.raises(ValueError):
            DeepOCSortConfig(**bad)
    assert DeepOCSortConfig(aw_param=0.0, alpha_fixed_emb=1.0, w_association_emb=0.0).aw_param == 0.0
    assert isinstance(deep_ocsort_config("deep_ocsort"), DeepOCSortConfig)
    assert all(deep_ocsort_config(t) is None for t in ("strongsort", "bytetrack", "botsort", "ocsort"))
    assert byte_config("deep_ocsort") is None and ocsort_config("deep_ocsort") is None
    for kw in (dict(with_reid=True), dict(with_pose=True), dict(ocsort_use_byte=True)):
        with pytest.raises(ValueError):
            deep_ocsort_config("deep_ocsort", **kw)
    with pytest.raises(ValueError):
        byte_config("deep_ocsort", with_reid=True)
    with pytest.raises(ValueError):
        ocsort_config("deep_ocsort", use_byte=True)
    with pytest.raises(ValueError):
        deep_ocsort_config("deepocsort")                                              # the other spelling stays refused
    assert check_gmc_method("sparseOptFlow", True, "deep_ocsort") == "sparseOptFlow" and check_gmc_method("ecc", True, "deep_ocsort") == "ecc"
    with pytest.raises(ValueError):
        check_gmc_method("sparseOptFlow", False, "deep_ocsort")
    with pytest.raises(ValueError):
        check_reid_model("auto", False)                                               # deep_ocsort never sets with_reid


def test_binding_has_the_deepoc_entries():
    import ctypes
    from strongsort_yolo_amd import lib
    for n in ("ss_deepoc_create", "ss_deepoc_destroy", "ss_deepoc_update_group", "ss_deepoc_update", "ss_deepoc_set_gmc", "ss_deepoc_reset",
              "ss_deepoc_get_tracks", "ss_deepoc_get_features"):
        assert n in lib.EXPORTS
    assert ctypes.sizeof(lib.ss_deepoc_config) == 80 and ctypes.sizeof(lib.ss_ocsort_config) == 56
    c = lib.make_deepoc_config(DeepOCSortConfig(delta_t=5, adaptive_weighting=False))
    assert (c.det_thresh, c.iou_threshold, c.inertia, c.w_association_emb, c.alpha_fixed_emb, c.aw_param) == (0.25, 0.3, 0.2, 0.75, 0.95, 0.5)
    assert (c.max_age, c.min_hits, c.delta_t, c.appearance, c.dynamic_appearance, c.adaptive_weighting, c.max_tracks, c.max_dets) == \
        (30, 3, 5, 1, 1, 0, 256, 128)
    lib.build()
    L = lib.load()
    out = (ctypes.c_float * 8)()
    assert L.ss_deepoc_create(None, ctypes.byref(c)) == lib.SS_ERR_INVALID            # checked before the device is touched
    assert L.ss_deepoc_update_group(None, 1, None, None, None, None, None) == lib.SS_ERR_INVALID
    assert L.ss_deepoc_update(None, None, None, None, None, None) == lib.SS_ERR_INVALID
    assert L.ss_deepoc_set_gmc(None, None) == lib.SS_ERR_INVALID
    assert L.ss_deepoc_reset(None, 0) == lib.SS_ERR_INVALID and L.ss_deepoc_destroy(None) == lib.SS_ERR_INVALID
    assert L.ss_deepoc_get_tracks(None, 0, 0, None, None, None, None, None, None, None, None, None, None, None, out, None) == lib.SS_ERR_INVALID
    assert L.ss_deepoc_get_features(None, 0, 0, out) == lib.SS_ERR_INVALID


def test_yolo_deep_ocsort_is_validated():
    import warnings
    from strongsort_yolo_amd.yolo import YOLO
    m = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="deep_ocsort")
    assert m.tracker_type == "deep_ocsort" and m._pipe_kw["tracker"] == "deep_ocsort" and "cmc" not in m._pipe_kw
    m2 = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="deep_ocsort", camera_motion=True, gmc_method="sparseOptFlow")
    assert m2._pipe_kw["cmc"] is True and m2._pipe_kw["gmc_method"] == "sparseOptFlow"
    for kw in (dict(with_reid=True), dict(with_pose=True), dict(ocsort_use_byte=True), dict(reid_model="auto")):
        with pytest.raises(ValueError):
            YOLO("yolo11n-pose.pt", random_init_ok=True, tracker_type="deep_ocsort", **kw)
    with pytest.raises(ValueError):
        YOLO("yolov8n.pt", random_init_ok=True, tracker_type="deepocsort")
    assert "deep_ocsort.yaml" in YOLO.TRACKERS and "deepocsort.yaml" not in YOLO.TRACKERS
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m._check_tracker("deep_ocsort.yaml")                                          # the model's own: quiet
        m._check_tracker("ocsort.yaml")                                               # another family: tracker_type rules, said once
        m._check_tracker("botsort.yaml")
    said = [x for x in w if issubclass(x.category, RuntimeWarning)]
    assert len(said) == 1 and "DeepOCSortConfig" in str(said[0].message)
    with pytest.raises(ValueError):
        m._check_tracker("deepocsort.yaml")


def test_cli_deep_ocsort_flags(monkeypatch):
    from strongsort_yolo_amd import cli
    monkeypatch.setattr(cli, "process_video", lambda job: job)
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--tracker", "deep_ocsort", "--random-init"])
    assert job["tracker"] == "deep_ocsort" and job["camera_motion"] is False
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--tracker", "deep_ocsort", "--random-init", "--camera-motion",
                       "--gmc-method", "sparseOptFlow"])
    assert job["camera_motion"] is True and job["gmc_method"] == "sparseOptFlow"
    for extra in (["--with-reid"], ["--with-pose"], ["--ocsort-use-byte"], ["--reid-model", "auto"]):
        with pytest.raises(SystemExit):
            cli.main(["--source", "synthetic:3", "--track", "--tracker", "deep_ocsort", "--random-init"] + extra)
    with pytest.raises(SystemExit):
        cli.main(["--source", "synthetic:3", "--track", "--tracker", "deepocsort"])
