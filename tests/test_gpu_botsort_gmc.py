"""BoT-SORT with camera-motion compensation on the MI355X (csrc/ss_byte.hip, k_byte_group's GMC variant, docs/BYTETRACK.md
§1b) against tests/botsort_gmc_ref.py, bit for bit: host-made warps, device ECC warps, and YOLO(tracker_type="botsort",
camera_motion=True) end to end."""
import numpy as np
import pytest
import torch

from strongsort_yolo_amd.config import ByteTrackConfig
from strongsort_yolo_amd.synth import make_stream
from tests.botsort_gmc_ref import BotSortGmcRef
from tests.bytetrack_ref import ByteTrackRef
from tests.test_bytetrack_cpu import byte_stream
from tests.test_gpu_cmc import _oracle_warp, _scene

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
XYWH = ByteTrackConfig(kalman="xywh")


def _warps(seed, F, S):
    """Seeded warps [F,S,8]: rotations up to 0.02 rad, translations up to 40 px, every 5th frame none (w6 = -1)."""
    rng = np.random.default_rng(100 + seed)
    th = rng.uniform(-0.02, 0.02, (F, S))
    w = np.zeros((F, S, 8))
    w[..., 0], w[..., 1], w[..., 3], w[..., 4] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    w[..., 2], w[..., 5] = rng.uniform(-40, 40, (F, S)), rng.uniform(-40, 40, (F, S))
    w[..., 6] = rng.integers(1, 60, (F, S))
    w[::5, :, 6] = -1.0
    return w


def _run_engine(eng, streams, group, warps=None):
    """streams: per stream a list of [N,6] frames -> per stream a list of rows; warps [F,S,8] (host) installed per call."""
    S, F = len(streams), len(streams[0])
    out_all = [[] for _ in range(S)]
    out = torch.zeros(32, S, 256, 8, device=DEV)
    nout = torch.zeros(32, S, dtype=torch.int32, device=DEV)
    for f0 in range(0, F, group):
        n = min(group, F - f0)
        hd, hn = np.zeros((n, S, 128, 6), np.float32), np.zeros((n, S), np.int32)
        for f in range(n):
            for s in range(S):
                d = streams[s][f0 + f]
                hd[f, s, :len(d)], hn[f, s] = d, len(d)
        if warps is not None:
            eng.set_cmc(torch.from_numpy(np.ascontiguousarray(warps[f0:f0 + n])).to(DEV))
        eng.update_group(n, torch.from_numpy(hd).to(DEV), torch.from_numpy(hn).to(DEV), None, None, out[:n], nout[:n])
        eng.check_errors()
        ho, hno = out[:n].cpu().numpy(), nout[:n].cpu().numpy()
        for f in range(n):
            for s in range(S):
                out_all[s].append(ho[f, s, :hno[f, s]].copy())
    return out_all


def _assert_rows(got, ref, what):
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), f"{what}:\n{got}\n!=\n{ref}"


def test_host_warps_rows_and_tables_equal_reference():
    from strongsort_yolo_amd.engine import ByteTrackEngine
    for seed in (0, 1, 2):
        streams = [byte_stream(10 * seed + s, 150) for s in range(3)]
        w = _warps(seed, 150, 3)
        eng = ByteTrackEngine(XYWH, 3, 0)
        got = _run_engine(eng, streams, 32, w)
        for s in range(3):
            ref = BotSortGmcRef(XYWH)
            for k, d in enumerate(streams[s]):
                _assert_rows(got[s][k], ref.update(d, w[k, s]), f"seed {seed} stream {s} frame {k}")
            t = eng.tracks(s)
            ids, st, act, mean = ref.tracks()
            assert t["n_tracked"] == len(ref.tracked) and t["n_lost"] == len(ref.lost) and t["next_id"] == ref.next_id
            assert np.array_equal(t["track_id"], ids) and np.array_equal(t["state"], st) and np.array_equal(t["activated"], act)
            assert t["mean"].tobytes() == mean.tobytes(), f"seed {seed} stream {s}: track means"
        eng.close()


def test_group_sizes_give_identical_rows():
    from strongsort_yolo_amd.engine import ByteTrackEngine
    streams = [byte_stream(7 + s, 64) for s in range(2)]
    w = _warps(7, 64, 2)
    res = []
    for g in (1, 7, 32):
        eng = ByteTrackEngine(XYWH, 2, 0)
        res.append(_run_engine(eng, streams, g, w))
        eng.close()
    for s in range(2):
        for k in range(64):
            assert res[0][s][k].tobytes() == res[1][s][k].tobytes() == res[2][s][k].tobytes(), f"stream {s} frame {k}"


def test_no_warp_equals_the_plain_tracker():
    from strongsort_yolo_amd.engine import ByteTrackEngine
    streams = [byte_stream(20 + s, 80) for s in range(2)]
    none = np.zeros((80, 2, 8))
    none[..., 0] = none[..., 4] = 1.0
    none[..., 6] = -1.0
    eng = ByteTrackEngine(XYWH, 2, 0)
    plain = _run_engine(eng, streams, 32)
    eng.close()
    eng = ByteTrackEngine(XYWH, 2, 0)
    off = _run_engine(eng, streams, 32, none)
    eng.close()
    eng = ByteTrackEngine(XYWH, 2, 0)
    eng.set_cmc(torch.from_numpy(_warps(3, 32, 2)).to(DEV))
    eng.set_cmc(None)                                             # switched off again: the plain kernel
    unset = _run_engine(eng, streams, 32)
    eng.close()
    for s in range(2):
        ref = ByteTrackRef(XYWH)
        for k in range(80):
            r = ref.update(streams[s][k])
            _assert_rows(plain[s][k], r, f"plain stream {s} frame {k}")
            assert off[s][k].tobytes() == r.tobytes() and unset[s][k].tobytes() == r.tobytes(), f"stream {s} frame {k}"


def test_set_gmc_errors_are_loud():
    from strongsort_yolo_amd import lib
    from strongsort_yolo_amd.engine import ByteTrackEngine, TrackerEngine
    from strongsort_yolo_amd.tracker import BYTETracker
    w = torch.zeros(1, 1, 8, dtype=torch.float64, device=DEV)
    base = TrackerEngine(n_streams=1)
    with pytest.raises(lib.SSError) as ei:                       # no BYTE state on this context
        base._ck(base.L.ss_byte_set_gmc(base.ctx, w.data_ptr()))
    assert ei.value.code == lib.SS_ERR_INVALID
    base.close()
    eng = ByteTrackEngine(ByteTrackConfig(kalman="xyah"), 1, 0)
    with pytest.raises(lib.SSError) as ei:                       # G-05: ByteTrack has no GMC
        eng.set_cmc(w)
    assert ei.value.code == lib.SS_ERR_INVALID
    eng.set_cmc(None)
    eng.close()
    with pytest.raises(ValueError):
        BYTETracker(ByteTrackConfig(kalman="xyah"), camera_motion=True)
    trk = BYTETracker(XYWH, camera_motion=True)
    with pytest.raises(ValueError):
        trk.update(np.zeros((0, 6), np.float32))
    trk.close()


# ---- device ECC warps into the tracker ------------------------------------------------------------------------------------
H_, W_, NF_ = 480, 640, 24


def _pan_offset(k):
    return 0 if k < 8 else (30 if k < 16 else 60)                # two camera jumps of 30 px (3 px in the 0.1x images)


def _pan_case():
    """Frames cut from one canvas with the camera jumping 30 px right at frames 8 and 16; six 24 px wide people standing
    still in the scene, so their boxes jump 30 px left: no overlap with the old boxes."""
    canvas = _scene(H_, W_, 3)
    xs = [60.0, 150.0, 240.0, 330.0, 420.0, 510.0]
    frames, dets = [], []
    for k in range(NF_):
        o = _pan_offset(k)
        frames.append(np.ascontiguousarray(canvas[100:100 + H_, 100 + o:100 + o + W_]))
        dets.append(np.asarray([[x - o, 200.0, x - o + 24.0, 260.0, 0.9, 0.0] for x in xs], np.float32))
    return frames, dets


def _oracle_warps(frames):
    out, prev = [], None
    for cur in frames:
        out.append(None if prev is None else _oracle_warp(prev, cur))
        prev = cur
    return out


def test_device_ecc_into_tracker_equals_reference_and_keeps_ids():
    from strongsort_yolo_amd.engine import ByteTrackEngine
    frames, dets = _pan_case()
    ow = _oracle_warps(frames)
    assert all(w[6] >= 1 for w in ow[1:]) and abs(ow[8][2] + 30) < 1 and abs(ow[16][2] + 30) < 1
    ref, plain = BotSortGmcRef(XYWH), BotSortGmcRef(XYWH)
    eng = ByteTrackEngine(XYWH, 1, 0)
    out = torch.zeros(4, 1, 256, 8, device=DEV)
    nout = torch.zeros(4, 1, dtype=torch.int32, device=DEV)
    ids_gmc, ids_plain = set(), set()
    for k0 in range(0, NF_, 4):
        fr = torch.from_numpy(np.stack(frames[k0:k0 + 4])).to(DEV)
        warps = eng.cmc_estimate(fr, 4)
        eng.set_cmc(warps)
        hd = np.zeros((4, 1, 128, 6), np.float32)
        for f in range(4):
            hd[f, 0, :6] = dets[k0 + f]
        eng.update_group(4, torch.from_numpy(hd).to(DEV), torch.full((4, 1), 6, dtype=torch.int32, device=DEV), None, None, out, nout)
        eng.check_errors()
        ho, hno = out.cpu().numpy(), nout.cpu().numpy()
        for f in range(4):
            k = k0 + f
            r = ref.update(dets[k], ow[k])
            _assert_rows(ho[f, 0, :hno[f, 0]], r, f"frame {k}")
            ids_gmc |= {int(i) for i in r[:, 4]}
            ids_plain |= {int(i) for i in plain.update(dets[k])[:, 4]}
    assert ids_gmc == set(range(1, 7)), "GMC keeps every id through both jumps"
    assert len(ids_plain) >= 18, "without GMC every jump renumbers the six people"
    # G-04: a reset forgets the stream's previous frame, so the next estimate is "no warp"
    eng.reset()
    w = eng.cmc_estimate(torch.from_numpy(np.stack(frames[:2])).to(DEV), 2).cpu().numpy()
    assert w[0, 0, 6] == -1 and w[1, 0, 6] >= 1
    eng.close()


def test_bytetracker_with_camera_motion_equals_reference():
    from strongsort_yolo_amd.tracker import BYTETracker
    frames, dets = _pan_case()
    ow = _oracle_warps(frames)
    trk, ref = BYTETracker(XYWH, camera_motion=True), BotSortGmcRef(XYWH)
    for k in range(NF_):
        fr = frames[k] if k % 2 else torch.from_numpy(frames[k]).to(DEV)      # numpy or a device tensor
        _assert_rows(trk.update(dets[k], fr), ref.update(dets[k], ow[k]), f"frame {k}")
    trk.reset()
    ref = BotSortGmcRef(XYWH)
    for k in range(8, 12):                                         # restarted: the first frame has no predecessor (G-04)
        _assert_rows(trk.update(dets[k], frames[k]), ref.update(dets[k], None if k == 8 else ow[k]), f"after reset, frame {k}")
    trk.close()


# ---- YOLO(tracker_type="botsort", camera_motion=True) end to end ------------------------------------------------------------
def _gmc_model():
    """Synthetic detector heads (as tests/test_gpu_bytetrack._byte_model) over a panning camera: a drifting stream's boxes,
    moved with the pan, drawn into frames cut from one canvas."""
    from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry
    from strongsort_yolo_amd.synth import synth_prediction
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", camera_motion=True)
    model.overrides.update(conf=0.3, iou=0.4, agnostic_nms=False, max_det=1000)
    model._pipe_kw.update(det_source="synthetic")
    g = letterbox_geometry(H_, W_)
    gs = scale_geometry(g, H_, W_)
    A = sum((g.out_h // s) * (g.out_w // s) for s in (8, 16, 32))
    canvas = _scene(H_, W_, 5)
    st, rng = make_stream(44, W_, H_, 9), np.random.default_rng(44)
    frames, preds = [], []
    for k in range(NF_):
        o = 4 * k if k < 12 else 48 + 25 * (k - 11) if k < 14 else 98
        d = st.next_frame().dets.copy()
        d[:, [0, 2]] = np.clip(d[:, [0, 2]] - o, 0, W_ - 1)               # the scene moves left by the pan
        d = d[d[:, 2] - d[:, 0] > 4]
        d[:, 4] = np.where(rng.random(len(d)) < 0.3, rng.uniform(0.12, 0.24, len(d)), d[:, 4]).astype(np.float32)
        pred, _ = synth_prediction(d, A, 80, gs[0], (gs[1], gs[2]), rng)
        frames.append(np.ascontiguousarray(canvas[100:100 + H_, o:o + W_])); preds.append(pred)
    dp = torch.from_numpy(np.stack(preds)).to(DEV)
    model._fill = lambda b, v, k: b.pred_in[v].copy_(dp[k])
    return model, frames


def _same(a, b, what):
    assert len(a.boxes) == len(b.boxes), what
    if len(b.boxes):
        assert torch.equal(a.boxes.id, b.boxes.id) and torch.equal(a.boxes.xyxy, b.boxes.xyxy) and torch.equal(a.boxes.conf, b.boxes.conf), what


def test_yolo_botsort_camera_motion_track_and_stream_equal_reference():
    model, frames = _gmc_model()
    ow = _oracle_warps(frames)
    assert sum(w[6] >= 1 for w in ow[1:]) >= 20
    ref, per_frame = BotSortGmcRef(XYWH), []
    for k in range(NF_):
        res = model.track(frames[k], verbose=False, device=0, persist=True, tracker="botsort.yaml")
        pipe = model._pipe
        assert pipe.reid is None and pipe.cmc and pipe.byte is not None
        rows = pipe.detections()[0]
        exp = ref.update(rows[:, :6], ow[k])
        r = res[0]
        assert len(r.boxes) == len(exp), f"frame {k}"
        if len(exp):
            assert np.array_equal(r.boxes.id.numpy(), exp[:, 4]) and np.array_equal(r.boxes.xyxy.numpy(), exp[:, :4]), f"frame {k}"
        per_frame.append(r)
    # persist=False: the tracker and the previous grey frame are forgotten, so the pass repeats exactly (G-04)
    model._frame_index = 0
    for k in range(NF_):
        res = model.track(frames[k], verbose=False, device=0, persist=k > 0, tracker="botsort.yaml")
        _same(res[0], per_frame[k], f"persist=False restart, frame {k}")
    # the overlapped stream pipeline, a full group and then a new pipeline whose last group is partial (24 = 3 x 7 + 3):
    # each starts with a fresh tracker and no warp on its first frame
    for batch in (32, 7):
        model._frame_index = 0
        got = list(model.track_stream(frames, batch=batch))
        assert len(got) == NF_ and model._stream_pipe.cmc and model._stream_pipe.reid is None
        for k, (a, b) in enumerate(zip(got, per_frame)):
            _same(a[0], b, f"track_stream batch {batch} frame {k}")
    model.close()
