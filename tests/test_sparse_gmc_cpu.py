"""The sparse-optical-flow camera-motion estimator (docs/BYTETRACK.md §1f, decisions S-01..) on the CPU: properties of the
reference tests/sparse_gmc_ref.py, the selection of corners, and every refusal of the configuration, the CLI and the C ABI."""
import os

import numpy as np
import pytest

from tests import sparse_gmc_ref as R
from tests.test_gpu_cmc import _scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(320, 240), (322, 246), (160, 120)]                   # (W, H)
PANS = [(7, -5), (3, 0), (21, 13)]
_CANVAS = {}


def _canvas(wh):
    if wh not in _CANVAS:
        _CANVAS[wh] = _scene(wh[1], wh[0], 3)
    return _CANVAS[wh]


def _view(wh, dx=0, dy=0):
    W, H = wh
    return _canvas(wh)[100 + dy:100 + dy + H, 100 + dx:100 + dx + W]


# ---- 1. reference properties ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wh", SIZES)
def test_identical_frames_give_the_identity_with_every_point_an_inlier(wh):
    a = _view(wh)
    w, rec = R.estimate_pair(a, a)
    assert np.array_equal(w[:6], [1, 0, 0, 0, 1, 0])
    n = len(rec["corners"])
    assert n > 0 and w[6] == n and w[7] == n and rec["status"].all() and rec["inliers"].all()
    assert np.array_equal(rec["points"], rec["corners"].astype(np.float64))


@pytest.mark.parametrize("wh", SIZES)
@pytest.mark.parametrize("pan", PANS)
def test_panned_views_give_the_pan(wh, pan):
    """The camera moves by (dx, dy): the scene moves by (-dx, -dy) in the image.  1.5 px: the bound tests/test_gpu_cmc.py uses for
    recovered drift."""
    dx, dy = pan
    w, rec = R.estimate_pair(_view(wh), _view(wh, dx, dy))
    print(wh, pan, w)
    assert w[6] >= 2 and w[7] >= 5
    assert abs(w[2] + dx) < 1.5 and abs(w[5] + dy) < 1.5, w
    assert abs(w[0] - 1) < 0.01 and abs(w[1]) < 0.01 and w[4] == w[0] and w[3] == -w[1], w


def test_flat_frames_and_too_few_matches_give_no_warp():
    a = _view((320, 240))
    flat = np.full_like(a, 90)
    none = [1, 0, 0, 0, 1, 0, -1]
    for prev, cur in ((a, flat), (flat, a), (flat, flat)):       # S-12: a pair with a cornerless image
        w, rec = R.estimate_pair(prev, cur)
        assert np.array_equal(w[:7], none) and not rec["status"].any() and not rec["inliers"].any()
    # fewer than 5 matches: four tracked corners are not enough, five are
    src = np.array([[10, 10], [50, 12], [30, 40], [70, 60], [20, 70], [90, 90]], np.int32)
    dst = src.astype(np.float64) + [2.0, -1.0]
    st = np.array([1, 1, 1, 1, 0, 0], np.uint8)
    w, mask = R.fit(src, dst, st)
    assert np.array_equal(w, [1, 0, 0, 0, 1, 0, -1, 4]) and not mask.any()
    st[4] = 1
    w, mask = R.fit(src, dst, st)
    assert np.allclose(w, [1, 0, 4, 0, 1, -2, 5, 5], atol=1e-12) and np.array_equal(mask, [1, 1, 1, 1, 1, 0])


def test_first_frame_reset_and_partial_groups_give_no_warp():
    fr = np.stack([_view((160, 120), 2 * k, k) for k in range(4)])[:, None]
    ref = R.SparseGmcRef(1)
    w = ref.estimate(fr)
    assert w[0, 0, 6] == -1 and (w[1:, 0, 6] >= 2).all()
    w = ref.estimate(fr[::-1], n_valid=2)                        # frames 3, 2 are real; the buffer's last two are stale
    assert (w[:2, 0, 6] >= 2).all() and (w[2:, 0, 6] == -1).all() and (2, 0) not in ref.last
    w = ref.estimate(fr[1:2])                                    # continues from frame 2, the last real one
    assert w[0, 0, 6] >= 2 and abs(w[0, 0, 2] - 2) < 1.5
    ref.reset()
    assert ref.estimate(fr[:1])[0, 0, 6] == -1


def test_outliers_do_not_move_the_fit():
    rng = np.random.default_rng(0)
    src = rng.integers(0, 300, (200, 2)).astype(np.int32)
    th, sc = 0.01, 1.002
    a, b = sc * np.cos(th), sc * np.sin(th)
    dst = np.stack([a * src[:, 0] - b * src[:, 1] + 5.5, b * src[:, 0] + a * src[:, 1] - 3.25], axis=1)
    dst[:60] += rng.uniform(-40, 40, (60, 2))                    # 30 % wild matches
    w, mask = R.fit(src, dst, np.ones(200, np.uint8))
    assert mask[60:].all() and mask[:60].sum() <= 6 and w[6] == mask.sum() and w[7] == 200
    assert abs(w[0] - a) < 1e-3 and abs(w[3] - b) < 1e-3 and abs(w[2] - 11.0) < 0.3 and abs(w[5] + 6.5) < 0.3


def test_integer_stages():
    rng = np.random.default_rng(1)
    bgr = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    g = R.grey(bgr)
    assert g.dtype == np.uint8 and np.abs(g.astype(float) - bgr.astype(float) @ [0.114, 0.587, 0.299]).max() <= 1
    h = R.half(g)
    assert h.shape == (4, 5)                                     # the odd last row and column are dropped (S-02)
    assert h[1, 2] == (int(g[2, 4]) + int(g[2, 5]) + int(g[3, 4]) + int(g[3, 5]) + 2) >> 2
    assert R.pyr_down(np.full((7, 9), 200, np.uint8)).tolist() == [[200] * 5] * 4        # size (n + 1) // 2, a constant stays
    a = rng.integers(0, 256, (7, 9), dtype=np.uint8)
    k = np.array([1, 4, 6, 4, 1])
    p = np.pad(a.astype(int), 2, mode="reflect")
    assert R.pyr_down(a)[3, 4] == (int((np.outer(k, k) * p[6:11, 8:13]).sum()) + 128) >> 8     # the last pixel, border reflected


# ---- 2. selection -----------------------------------------------------------------------------------------------------------
def test_selection_is_a_cut_of_a_total_order():
    l0 = R.pyramid(_view((320, 240)))[0]
    pts, n_cand = R.corners(l0)
    assert n_cand > 1000 and len(pts) == 1000                    # truncation is exercised
    lam = R.min_eig_map(l0)
    v, idx = lam[pts[:, 1], pts[:, 0]], pts[:, 1] * l0.shape[1] + pts[:, 0]
    assert len(set(idx.tolist())) == 1000                        # distinct pixels: minDistance 1 rejects nothing (S-05)
    assert all(v[i] > v[i + 1] or (v[i] == v[i + 1] and idx[i] < idx[i + 1]) for i in range(999))
    assert v[-1] >= np.float32(0.01) * lam.max() and v[0] == lam.max()
    pts2, n2 = R.corners(R.pyramid(_view((160, 120)))[0])
    assert 0 < n2 < 1000 and len(pts2) == n2                     # below the cut: every candidate is kept
    assert R.corners(np.full((60, 80), 7, np.uint8)) [1] == 0


# ---- 3. configuration and CLI ---------------------------------------------------------------------------------------------
def test_unknown_gmc_method_is_refused():
    from strongsort_yolo_amd.config import check_gmc_method
    from strongsort_yolo_amd.yolo import YOLO
    assert check_gmc_method("ecc", False, "strongsort") == "ecc" and check_gmc_method("sparseOptFlow", True, "botsort") == "sparseOptFlow"
    with pytest.raises(ValueError, match="gmc_method must be one of"):
        check_gmc_method("orb", True, "botsort")
    with pytest.raises(ValueError, match="gmc_method must be one of"):
        YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", camera_motion=True, gmc_method="sift")


def test_sparse_flow_without_camera_motion_is_refused():
    from strongsort_yolo_amd.config import ByteTrackConfig
    from strongsort_yolo_amd.pipeline import FramePipeline
    from strongsort_yolo_amd.tracker import BYTETracker
    from strongsort_yolo_amd.yolo import YOLO
    with pytest.raises(ValueError, match="needs camera_motion=True"):
        YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", gmc_method="sparseOptFlow")
    with pytest.raises(ValueError, match="needs camera_motion=True"):
        BYTETracker(ByteTrackConfig(kalman="xywh"), gmc_method="sparseOptFlow")
    with pytest.raises(ValueError, match="needs camera_motion=True"):
        FramePipeline("yolov8n", 1, (240, 320), tracker="botsort", gmc_method="sparseOptFlow")


@pytest.mark.parametrize("tracker", ["strongsort", "bytetrack"])
def test_sparse_flow_with_another_tracker_is_refused(tracker):
    from strongsort_yolo_amd.pipeline import FramePipeline
    from strongsort_yolo_amd.yolo import YOLO
    with pytest.raises(ValueError):
        YOLO("yolov8n.pt", random_init_ok=True, tracker_type=tracker, camera_motion=True, gmc_method="sparseOptFlow")
    if tracker == "strongsort":                                  # (bytetrack with camera_motion is refused before the method is looked at)
        with pytest.raises(ValueError, match="tracker_type 'botsort'"):
            YOLO("yolov8n.pt", random_init_ok=True, tracker_type=tracker, camera_motion=True, gmc_method="sparseOptFlow")
        with pytest.raises(ValueError, match="tracker_type 'botsort'"):
            FramePipeline("yolov8n", 1, (240, 320), tracker=tracker, cmc=True, gmc_method="sparseOptFlow")


def test_bytetracker_xyah_with_sparse_flow_is_refused():
    from strongsort_yolo_amd.config import ByteTrackConfig
    from strongsort_yolo_amd.tracker import BYTETracker
    with pytest.raises(ValueError, match="tracker_type 'botsort'"):
        BYTETracker(ByteTrackConfig(kalman="xyah"), camera_motion=True, gmc_method="sparseOptFlow")


def test_yolo_passes_the_method_to_its_pipelines():
    from strongsort_yolo_amd.yolo import YOLO
    m = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", camera_motion=True, gmc_method="sparseOptFlow")
    assert m._pipe_kw["cmc"] is True and m._pipe_kw["gmc_method"] == "sparseOptFlow" and m.gmc_method == "sparseOptFlow"
    m = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", camera_motion=True)
    assert "gmc_method" not in m._pipe_kw and m.gmc_method == "ecc"           # the default: what camera_motion=True has always meant


def test_cli_gmc_method_flag(monkeypatch):
    from strongsort_yolo_amd import cli
    monkeypatch.setattr(cli, "process_video", lambda job: job)
    base = ["--source", "synthetic:3", "--track"]
    (job,) = cli.main(base + ["--tracker", "botsort", "--camera-motion", "--gmc-method", "sparseOptFlow"])
    assert job["gmc_method"] == "sparseOptFlow" and job["camera_motion"] is True
    (job,) = cli.main(base + ["--tracker", "botsort", "--camera-motion"])
    assert job["gmc_method"] == "ecc"
    with pytest.raises(SystemExit):                              # unknown value
        cli.main(base + ["--tracker", "botsort", "--camera-motion", "--gmc-method", "orb"])
    with pytest.raises(SystemExit):                              # without --camera-motion
        cli.main(base + ["--tracker", "botsort", "--gmc-method", "sparseOptFlow"])
    for tracker in ("strongsort", "bytetrack"):                  # another tracker
        with pytest.raises(SystemExit):
            cli.main(base + ["--tracker", tracker, "--camera-motion", "--gmc-method", "sparseOptFlow"])


def test_cli_passes_the_method_to_the_model(monkeypatch):
    from strongsort_yolo_amd import cli, yolo
    seen = {}

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(yolo, "YOLO", fake)
    with pytest.raises(Stop):
        cli.process_video({"source": "synthetic:2", "track": True, "count": False, "tracker": "botsort", "camera_motion": True,
                           "gmc_method": "sparseOptFlow"})
    assert seen["gmc_method"] == "sparseOptFlow" and seen["camera_motion"] is True


# ---- 4. the C ABI without a device ------------------------------------------------------------------------------------------
def test_abi_is_declared_exported_and_checks_its_arguments_without_a_gpu():
    import ctypes as C
    from strongsort_yolo_amd import lib
    src = open(os.path.join(ROOT, "include", "strongsort_hip.h")).read()
    assert "int ss_gmc_sparse_estimate(ss_ctx* ctx, void* hip_stream, const uint8_t* d_frames, int n_frames" in src
    assert "int ss_gmc_sparse_get(ss_ctx* ctx, int frame, int stream" in src
    assert "ss_gmc_sparse_estimate" in lib.EXPORTS and "ss_gmc_sparse_get" in lib.EXPORTS
    lib.build()
    L = lib.load()
    fr, wp = C.c_void_p(4096), C.c_void_p(8192)                  # never dereferenced: every call below is refused first
    est = L.ss_gmc_sparse_estimate
    bad = lib.SS_ERR_INVALID
    assert est(None, None, None, 1, 0, 240, 320, 960, None, wp) == bad          # no frames
    assert est(None, None, fr, 1, 0, 240, 320, 960, None, None) == bad          # no warps
    assert est(None, None, fr, 0, 0, 240, 320, 960, None, wp) == bad            # n_frames outside 1..32
    assert est(None, None, fr, 33, 0, 240, 320, 960, None, wp) == bad
    assert est(None, None, fr, 1, 0, 63, 320, 960, None, wp) == bad             # too small for a level-3 image
    assert est(None, None, fr, 1, 0, 240, 62, 960, None, wp) == bad
    assert est(None, None, fr, 1, 0, 240, 320, 959, None, wp) == bad            # rows overlap
    assert est(None, None, fr, 1, 0, 240, 320, 960, None, wp) == bad            # good arguments, no context
    assert b"null context" in L.ss_last_error(None)
    assert L.ss_gmc_sparse_get(None, 0, 0, None, None, None, None, None, None, None, None, None, None) == bad
    assert R.MIN_SIDE == 64
