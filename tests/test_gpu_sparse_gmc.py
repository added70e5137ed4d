"""The sparse-optical-flow camera-motion estimator on the MI355X (csrc/ss_gmc.hip, docs/BYTETRACK.md §1f) against
tests/sparse_gmc_ref.py, bit for bit: every stage through ss_gmc_sparse_get, the warps, the BoT-SORT tracker fed by them, and
YOLO(tracker_type="botsort", camera_motion=True, gmc_method="sparseOptFlow") end to end."""
import numpy as np
import pytest
import torch

from strongsort_yolo_amd.config import ByteTrackConfig
from strongsort_yolo_amd.synth import make_stream
from tests.botsort_gmc_ref import BotSortGmcRef
from tests.sparse_gmc_ref import SparseGmcRef
from tests.test_bytetrack_cpu import byte_stream
from tests.test_gpu_cmc import _scene

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
XYWH = ByteTrackConfig(kalman="xywh")


def _check_stages(eng, ref, F, S, what):
    for f in range(F):
        for s in range(S):
            rec = ref.last.get((f, s))
            if rec is None:                                    # no predecessor, or a frame past n_valid: nothing to compare
                continue
            got = eng.gmc_sparse_stages(f, s)
            w = f"{what} frame {f} stream {s}"
            for L in range(4):
                assert np.array_equal(got["pyramid"][L], rec["pyramid"][L]), f"{w}: pyramid level {L}"
            assert got["n_candidates"] == rec["n_candidates"], f"{w}: candidates {got['n_candidates']} != {rec['n_candidates']}"
            assert np.array_equal(got["corners"], rec["corners"]), f"{w}: corner list"
            assert np.array_equal(got["status"], rec["status"]), f"{w}: LK status"
            assert np.array_equal(got["points"], rec["points"]), f"{w}: LK points, max |diff| {np.abs(got['points'] - rec['points']).max()}"
            assert np.array_equal(got["inliers"], rec["inliers"]), f"{w}: inlier mask"


# 320x240: baseline, more than 1000 corner candidates; 322x246: odd half size 161x123 and odd pyramid levels; 160x120: level 3 is
# 20x15, smaller than the LK window
@pytest.mark.parametrize("wh,S,F", [((320, 240), 1, 3), ((322, 246), 2, 2), ((160, 120), 1, 4)])
def test_stages_and_warps_equal_reference(wh, S, F):
    from strongsort_yolo_amd.engine import TrackerEngine
    W, H = wh
    eng, ref = TrackerEngine(n_streams=S, debug=False), SparseGmcRef(S)
    canv = [_scene(H, W, 10 * s + 1) for s in range(S)]
    rng = np.random.default_rng(W + S)
    k = 0                                                      # frames so far: the camera drifts by (7, -5) px a frame, with one jump

    def frames_of(call):
        nonlocal k
        fr = np.zeros((F, S, H, W, 3), np.uint8)
        for f in range(F):
            jump = int(rng.integers(-12, 13)) if (call == 0 and f == F - 1) else 0
            for s in range(S):
                ox, oy = 100 + (7 * k) % 60 + jump, 100 - (5 * k) % 60
                fr[f, s] = canv[s][oy:oy + H, ox:ox + W]
            k += 1
        return fr

    def run(fr, n_valid=None):
        nf = fr.shape[0]
        d = torch.from_numpy(fr.reshape(nf * S, H, W, 3)).to(DEV)
        nv = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int32, device=DEV)
        got = eng.gmc_sparse_estimate(d, nf, n_valid=nv).cpu().numpy()
        exp = ref.estimate(fr, n_valid)
        return got, exp

    # call 0: no predecessor for the first frame
    fr = frames_of(0)
    got, exp = run(fr)
    _check_stages(eng, ref, F, S, "call 0")
    assert np.array_equal(got[..., :8], exp[..., :8]), f"call 0: max |diff| {np.abs(got - exp).max()}"
    assert (exp[0, :, 6] == -1).all() and (exp[1:, :, 6] >= 2).all()
    if W == 320:
        assert ref.last[(1, 0)]["n_candidates"] > 1000           # the cut to 1000 corners is exercised
    # call 1: the remembered frame is used; a flat frame in the middle: it and its successor get no warp
    fr = frames_of(1)
    fr[1, 0] = 90
    got, exp = run(fr)
    _check_stages(eng, ref, F, S, "call 1")
    assert np.array_equal(got[..., :8], exp[..., :8]), f"call 1: max |diff| {np.abs(got - exp).max()}"
    assert exp[0, 0, 6] >= 2 and exp[1, 0, 6] == -1 and (F < 3 or exp[2, 0, 6] == -1)
    # call 2: a partial group: the frames past n_valid get -1 and the last real one is remembered
    fr = frames_of(2)
    got, exp = run(fr, n_valid=F - 1)
    _check_stages(eng, ref, F, S, "call 2")
    assert np.array_equal(got[..., :8], exp[..., :8]), f"call 2: max |diff| {np.abs(got - exp).max()}"
    assert (exp[F - 1, :, 6] == -1).all() and (F != 2 or exp[0, 0, 6] == -1)      # F = 2: the flat frame's successor is here
    # call 3 continues from frame F - 2 of call 2 (the last real one)
    got, exp = run(fr[F - 1:])
    _check_stages(eng, ref, 1, S, "call 3")
    assert np.array_equal(got[..., :8], exp[..., :8]) and (exp[0, :, 6] >= 2).all()
    # G-04: a reset forgets the remembered frame of that stream only
    eng.reset(0)
    ref.reset(0)
    got, exp = run(frames_of(4)[:1])
    assert np.array_equal(got[..., :8], exp[..., :8]) and exp[0, 0, 6] == -1 and (exp[0, 1:, 6] >= 2).all()
    eng.close()


# ---- device sparse warps into the tracker ----------------------------------------------------------------------------------
H_, W_, NF_ = 120, 160, 24
_CASE = {}


def _pan_case():
    """byte_stream detections of a 1280x720 scene over frames cut from one 160x120 canvas; the camera pans 3 px a frame from frame 8
    and the detections move with it.  The reference's warps are computed once."""
    if not _CASE:
        canvas = _scene(H_, W_, 3)
        dets, frames = [], []
        for k, d in enumerate(byte_stream(9, NF_)):
            pan = 3 * (k - 7) if k >= 8 else 0
            d = d.copy()
            d[:, [0, 2]] = np.clip(d[:, [0, 2]] - pan, 0, 1279)
            dets.append(np.ascontiguousarray(d[d[:, 2] - d[:, 0] > 4]))
            frames.append(np.ascontiguousarray(canvas[100:100 + H_, 100 + pan:100 + pan + W_]))
        ref = SparseGmcRef(1)
        warps = np.concatenate([ref.estimate(f[None, None]) for f in frames])[:, 0]
        _CASE.update(dets=dets, frames=frames, warps=warps)
    return _CASE["dets"], _CASE["frames"], _CASE["warps"]


def _run_tracker(group):
    from strongsort_yolo_amd.engine import ByteTrackEngine
    dets, frames, _ = _pan_case()
    eng = ByteTrackEngine(XYWH, 1, 0)
    out = torch.zeros(group, 1, 256, 8, device=DEV)
    nout = torch.zeros(group, 1, dtype=torch.int32, device=DEV)
    rows, warps = [], []
    for k0 in range(0, NF_, group):
        w = eng.gmc_sparse_estimate(torch.from_numpy(np.stack(frames[k0:k0 + group])).to(DEV), group)
        eng.set_cmc(w)
        hd, hn = np.zeros((group, 1, 128, 6), np.float32), np.zeros((group, 1), np.int32)
        for f in range(group):
            d = dets[k0 + f]
            hd[f, 0, :len(d)], hn[f, 0] = d, len(d)
        eng.update_group(group, torch.from_numpy(hd).to(DEV), torch.from_numpy(hn).to(DEV), None, None, out, nout)
        eng.check_errors()
        ho, hno = out.cpu().numpy(), nout.cpu().numpy()
        rows += [ho[f, 0, :hno[f, 0]].copy() for f in range(group)]
        warps.append(w.cpu().numpy()[:, 0])
    table = eng.tracks(0)
    eng.close()
    return rows, np.concatenate(warps), table


@pytest.mark.parametrize("group", [1, 4])
def test_tracker_with_device_sparse_warps_equals_reference(group):
    dets, _, rw = _pan_case()
    assert (rw[1:, 6] >= 2).sum() >= 20 and rw[0, 6] == -1
    assert np.abs(rw[9:, 2] + 3).max() < 1.5 and np.abs(rw[9:, 5]).max() < 1.5       # the pan is recovered
    rows, warps, t = _run_tracker(group)
    assert np.array_equal(warps, rw)
    ref = BotSortGmcRef(XYWH)
    for k in range(NF_):
        exp = ref.update(dets[k], rw[k])
        assert rows[k].shape == exp.shape and rows[k].tobytes() == exp.tobytes(), f"group {group} frame {k}"
    ids, st, act, mean = ref.tracks()
    assert t["n_tracked"] == len(ref.tracked) and t["n_lost"] == len(ref.lost) and t["next_id"] == ref.next_id
    assert np.array_equal(t["track_id"], ids) and np.array_equal(t["state"], st) and np.array_equal(t["activated"], act)
    assert t["mean"].tobytes() == mean.tobytes()
    if group == 4:                                             # group 4 against group 1
        rows1, warps1, t1 = _run_tracker(1)
        assert np.array_equal(warps1, warps) and t1["mean"].tobytes() == t["mean"].tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(rows1, rows))


def test_estimate_errors_are_loud():
    from strongsort_yolo_amd import lib
    from strongsort_yolo_amd.engine import TrackerEngine
    eng = TrackerEngine(n_streams=1)
    with pytest.raises(lib.SSError) as ei:                       # nothing estimated yet
        eng._gmc_hw = (64, 64)
        eng.gmc_sparse_stages(0, 0)
    assert ei.value.code == lib.SS_ERR_INVALID
    with pytest.raises(lib.SSError) as ei:                       # level 3 would be smaller than 4 x 4
        eng.gmc_sparse_estimate(torch.zeros(1, 62, 64, 3, dtype=torch.uint8, device=DEV), 1)
    assert ei.value.code == lib.SS_ERR_INVALID
    w = eng.gmc_sparse_estimate(torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device=DEV), 1).cpu().numpy()
    assert w[0, 0, 6] == -1
    eng.close()


# ---- YOLO(tracker_type="botsort", camera_motion=True, gmc_method="sparseOptFlow") end to end --------------------------------
HE_, WE_, NE_ = 240, 320, 16


def _gmc_model():
    """tests/test_gpu_botsort_gmc._gmc_model with the sparse estimator at 320x240: synthetic detector heads over a panning camera."""
    from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry
    from strongsort_yolo_amd.synth import synth_prediction
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", camera_motion=True, gmc_method="sparseOptFlow")
    model.overrides.update(conf=0.3, iou=0.4, agnostic_nms=False, max_det=1000)
    model._pipe_kw.update(det_source="synthetic")
    g = letterbox_geometry(HE_, WE_)
    gs = scale_geometry(g, HE_, WE_)
    A = sum((g.out_h // s) * (g.out_w // s) for s in (8, 16, 32))
    canvas = _scene(HE_, WE_, 5)
    st, rng = make_stream(44, WE_, HE_, 6), np.random.default_rng(44)
    frames, preds = [], []
    for k in range(NE_):
        o = 4 * k if k < 10 else 36 + 15 * (k - 9) if k < 12 else 66
        d = st.next_frame().dets.copy()
        d[:, [0, 2]] = np.clip(d[:, [0, 2]] - o, 0, WE_ - 1)             # the scene moves left by the pan
        d = d[d[:, 2] - d[:, 0] > 4]
        d[:, 4] = np.where(rng.random(len(d)) < 0.3, rng.uniform(0.12, 0.24, len(d)), d[:, 4]).astype(np.float32)
        pred, _ = synth_prediction(d, A, 80, gs[0], (gs[1], gs[2]), rng)
        frames.append(np.ascontiguousarray(canvas[100:100 + HE_, o:o + WE_])); preds.append(pred)
    dp = torch.from_numpy(np.stack(preds)).to(DEV)
    model._fill = lambda b, v, k: b.pred_in[v].copy_(dp[k])
    return model, frames


def _same(a, b, what):
    assert len(a.boxes) == len(b.boxes), what
    if len(b.boxes):
        assert torch.equal(a.boxes.id, b.boxes.id) and torch.equal(a.boxes.xyxy, b.boxes.xyxy) and torch.equal(a.boxes.conf, b.boxes.conf), what


def test_yolo_botsort_sparse_gmc_track_and_stream_equal_reference():
    model, frames = _gmc_model()
    sref = SparseGmcRef(1)
    rw = np.concatenate([sref.estimate(f[None, None]) for f in frames])[:, 0]
    assert (rw[1:, 6] >= 2).sum() >= NE_ - 2 and rw[0, 6] == -1
    ref, per_frame = BotSortGmcRef(XYWH), []
    for k in range(NE_):
        res = model.track(frames[k], verbose=False, device=0, persist=True, tracker="botsort.yaml")
        pipe = model._pipe
        assert pipe.reid is None and pipe.cmc and pipe.gmc_method == "sparseOptFlow" and pipe.byte is not None
        assert np.array_equal(pipe.warps.cpu().numpy()[0, 0], rw[k]), f"frame {k}: warp"
        rows = pipe.detections()[0]
        exp = ref.update(rows[:, :6], rw[k])
        r = res[0]
        assert len(r.boxes) == len(exp), f"frame {k}"
        if len(exp):
            assert np.array_equal(r.boxes.id.numpy(), exp[:, 4]) and np.array_equal(r.boxes.xyxy.numpy(), exp[:, :4]), f"frame {k}"
        per_frame.append(r)
    # persist=False: the tracker and the remembered frame are forgotten: ids restart, the first frame has no warp (G-04)
    model._frame_index = 0
    for k in range(NE_):
        res = model.track(frames[k], verbose=False, device=0, persist=k > 0, tracker="botsort.yaml")
        if k == 0:
            assert model._pipe.warps.cpu().numpy()[0, 0, 6] == -1
        _same(res[0], per_frame[k], f"persist=False restart, frame {k}")
    # the overlapped stream pipeline: one full group, then a new pipeline whose last group is partial (16 = 2 x 7 + 2)
    for batch in (32, 7):
        model._frame_index = 0
        got = list(model.track_stream(frames, batch=batch))
        assert len(got) == NE_ and model._stream_pipe.cmc and model._stream_pipe.gmc_method == "sparseOptFlow"
        for k, (a, b) in enumerate(zip(got, per_frame)):
            _same(a[0], b, f"track_stream batch {batch} frame {k}")
    model.close()
