"""The BYTE tracker family on the MI355X (csrc/ss_byte.hip) against its CPU reference (tests/bytetrack_ref.py), bit for bit."""
import numpy as np
import pytest
import torch

from strongsort_yolo_amd.config import ByteTrackConfig
from strongsort_yolo_amd.synth import make_stream
from tests.bytetrack_ref import ByteTrackRef
from tests.test_bytetrack_cpu import SCENARIOS, byte_stream

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _run_engine(eng, streams, group):
    """streams: per stream a list of [N,6] frames (equal lengths) -> per stream a list of rows, through update_group calls of
    `group` frames."""
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
        eng.update_group(n, torch.from_numpy(hd).to(DEV), torch.from_numpy(hn).to(DEV), None, None, out[:n], nout[:n])
        eng.check_errors()
        ho, hno = out[:n].cpu().numpy(), nout[:n].cpu().numpy()
        for f in range(n):
            for s in range(S):
                out_all[s].append(ho[f, s, :hno[f, s]].copy())
    return out_all


def _assert_rows(got, ref, what):
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), f"{what}:\n{got}\n!=\n{ref}"


@pytest.mark.parametrize("kalman", ["xyah", "xywh"])
def test_group_rows_and_tables_equal_reference(kalman):
    from strongsort_yolo_amd.engine import ByteTrackEngine
    cfg = ByteTrackConfig(kalman=kalman)
    for seed in (0, 1, 2):
        streams = [byte_stream(10 * seed + s, 150) for s in range(3)]
        eng = ByteTrackEngine(cfg, 3, 0)
        got = _run_engine(eng, streams, 32)
        for s in range(3):
            ref = ByteTrackRef(cfg)
            for k, d in enumerate(streams[s]):
                _assert_rows(got[s][k], ref.update(d), f"{kalman} seed {seed} stream {s} frame {k}")
            t = eng.tracks(s)
            ids, st, act, mean = ref.tracks()
            assert t["n_tracked"] == len(ref.tracked) and t["n_lost"] == len(ref.lost) and t["next_id"] == ref.next_id
            assert np.array_equal(t["track_id"], ids) and np.array_equal(t["state"], st) and np.array_equal(t["activated"], act)
            assert t["mean"].tobytes() == mean.tobytes(), f"{kalman} seed {seed} stream {s}: track means"
        eng.close()


def test_group_sizes_give_identical_rows():
    from strongsort_yolo_amd.engine import ByteTrackEngine
    streams = [byte_stream(7 + s, 64) for s in range(2)]
    res = []
    for g in (1, 7, 32):
        eng = ByteTrackEngine(ByteTrackConfig(), 2, 0)
        res.append(_run_engine(eng, streams, g))
        eng.close()
    for s in range(2):
        for k in range(64):
            assert res[0][s][k].tobytes() == res[1][s][k].tobytes() == res[2][s][k].tobytes(), f"stream {s} frame {k}"


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_hand_built_scenarios_on_device(name):
    from strongsort_yolo_amd.tracker import BYTETracker
    frames, kalman, _ = SCENARIOS[name]()
    cfg = ByteTrackConfig(kalman=kalman)
    trk, ref = BYTETracker(cfg), ByteTrackRef(cfg)
    for k, d in enumerate(frames):
        _assert_rows(trk.update(d), ref.update(d), f"{name} frame {k}")
    trk.close()


def test_over_full_table_is_reported_and_reset_recovers():
    from strongsort_yolo_amd.engine import ByteTrackEngine
    from strongsort_yolo_amd import lib
    cfg = ByteTrackConfig(max_tracks=16)
    rng = np.random.default_rng(5)
    frames = []
    for k in range(6):                                    # 12 fresh, far-apart boxes a frame: births overflow 16 slots
        x = rng.uniform(0, 1200, 12).astype(np.float32) + k * 3000
        frames.append(np.stack([x, x * 0 + 10, x + 20, x * 0 + 60, np.full(12, 0.9, np.float32), np.zeros(12, np.float32)], 1))
    eng = ByteTrackEngine(cfg, 1, 0)
    out = torch.zeros(1, 1, 256, 8, device=DEV)
    nout = torch.zeros(1, 1, dtype=torch.int32, device=DEV)
    ref = ByteTrackRef(cfg)
    for d in frames:
        hd = np.zeros((1, 1, 128, 6), np.float32)
        hd[0, 0, :len(d)] = d
        eng.update_group(1, torch.from_numpy(hd).to(DEV), torch.tensor([[len(d)]], dtype=torch.int32, device=DEV), None, None, out, nout)
        r = ref.update(d)
        got = out[0, 0, :int(nout[0, 0])].cpu().numpy()
        assert int(nout[0, 0]) <= 16
        _assert_rows(got, r, "over-full table")
    assert ref.capacity_error
    with pytest.raises(lib.SSError) as ei:
        eng.check_errors()
    assert ei.value.code == lib.SS_ERR_CAPACITY
    t = eng.tracks(0)
    assert t["n_tracked"] + t["n_lost"] <= 16
    # more rows than a frame holds: tracked on the first 128, flagged
    eng.reset()
    eng.check_errors()
    hd = torch.zeros(1, 1, 128, 6, device=DEV)
    eng.update_group(1, hd, torch.tensor([[500]], dtype=torch.int32, device=DEV), None, None, out, nout)
    with pytest.raises(lib.SSError):
        eng.check_errors()
    eng.reset()
    ref = ByteTrackRef(cfg)
    d = frames[0]
    hd = np.zeros((1, 1, 128, 6), np.float32)
    hd[0, 0, :len(d)] = d
    eng.update_group(1, torch.from_numpy(hd).to(DEV), torch.tensor([[len(d)]], dtype=torch.int32, device=DEV), None, None, out, nout)
    eng.check_errors()
    _assert_rows(out[0, 0, :int(nout[0, 0])].cpu().numpy(), ref.update(d), "after reset")
    eng.close()


# ---- YOLO(tracker_type=...) end to end ----------------------------------------------------------------------------------
H_, W_, NF_ = 480, 640, 24


def _byte_model(weights, nk, tracker_type="bytetrack", **kw):
    from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry
    from strongsort_yolo_amd.synth import synth_prediction
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO(weights, tracker_type=tracker_type, **kw)
    model.overrides.update(conf=0.3, iou=0.4, agnostic_nms=False, max_det=1000)
    model._pipe_kw.update(det_source="synthetic")
    g = letterbox_geometry(H_, W_)
    gs = scale_geometry(g, H_, W_)
    A = sum((g.out_h // s) * (g.out_w // s) for s in (8, 16, 32))
    nc = 1 if nk else 80
    st, rng = make_stream(43, W_, H_, 9), np.random.default_rng(43)
    frames, preds = [], []
    for k in range(NF_):
        d = st.next_frame().dets.copy()
        d[:, 4] = np.where(rng.random(len(d)) < 0.3, rng.uniform(0.12, 0.24, len(d)), d[:, 4]).astype(np.float32)   # low-score rows
        if nk:
            d[:, 5] = 0
        pred, _ = synth_prediction(d, A, nc, gs[0], (gs[1], gs[2]), rng)
        if nk:
            pred = np.concatenate([pred, rng.uniform(0, 400, (nk, A)).astype(np.float32)])
        frames.append(st.frame_pixels(k).copy()); preds.append(pred)
    dp = torch.from_numpy(np.stack(preds)).to(DEV)
    model._fill = lambda b, v, k: b.pred_in[v].copy_(dp[k])
    return model, frames


def _check(res, pipe_rows, ref_rows, nk, pipe):
    r = res[0]
    assert len(r.boxes) == len(ref_rows)
    if len(ref_rows) == 0:
        return
    assert np.array_equal(r.boxes.id.numpy(), ref_rows[:, 4]) and np.array_equal(r.boxes.xyxy.numpy(), ref_rows[:, :4])
    assert np.array_equal(r.boxes.cls.numpy(), ref_rows[:, 5]) and np.array_equal(r.boxes.conf.numpy(), ref_rows[:, 6])
    if nk:                                                   # keypoints follow det_idx
        k = torch.from_numpy(pipe_rows[:, 6:6 + nk]).reshape(len(pipe_rows), nk // 3, 3).clone()
        k[..., 0] = (k[..., 0] - pipe.pad_x) / pipe.gain
        k[..., 1] = (k[..., 1] - pipe.pad_y) / pipe.gain
        assert torch.equal(r.keypoints.data, k[torch.from_numpy(ref_rows[:, 7]).long()])


@pytest.mark.parametrize("weights,nk", [("yolov8n.pt", 0), ("yolo11n-pose.pt", 51)])
def test_yolo_bytetrack_track_and_stream_equal_reference(weights, nk):
    model, frames = _byte_model(weights, nk, random_init_ok=True)
    ref, per_frame, low = ByteTrackRef(ByteTrackConfig()), [], 0
    for k in range(NF_):
        res = model.track(frames[k], verbose=False, device=0, persist=True, tracker="bytetrack.yaml")
        pipe = model._pipe
        assert pipe.reid is None and pipe.dcfg.conf == 0.1
        rows = pipe.detections()[0]
        assert (rows[:, 4] > np.float32(0.1)).all()
        low += int((rows[:, 4] < 0.25).sum())
        exp = ref.update(rows[:, :6])
        _check(res, rows, exp, nk, pipe)
        per_frame.append(res[0])
    assert low > 0, "low-score rows reach the tracker"
    model._frame_index = 0
    got = list(model.track_stream(frames, batch=32))
    assert model._stream_pipe.reid is None
    assert len(got) == NF_
    for k, (a, b) in enumerate(zip(got, per_frame)):
        a = a[0]
        assert len(a.boxes) == len(b.boxes), f"frame {k}"
        if len(b.boxes):
            assert torch.equal(a.boxes.id, b.boxes.id) and torch.equal(a.boxes.xyxy, b.boxes.xyxy) and torch.equal(a.boxes.conf, b.boxes.conf)
            if nk:
                assert torch.equal(a.keypoints.data, b.keypoints.data)
    model.close()


def test_detector_only_checkpoint_is_enough_to_track(tmp_path, monkeypatch):
    from strongsort_yolo_amd import nets
    from strongsort_yolo_amd.yolo import YOLO
    monkeypatch.delenv("SS_RANDOM_INIT", raising=False)
    path = str(tmp_path / "yolov8n.pt")
    torch.save(nets.build_detector("yolov8n", 3).state_dict(), path)
    frame = make_stream(3, W_, H_, 5).frame_pixels(0).copy()
    m = YOLO(path, tracker_type="bytetrack", random_init_ok=False)
    res = m.track(frame, verbose=False, device=0, persist=True, tracker="bytetrack.yaml")
    assert isinstance(res, list) and len(res) == 1 and m._pipe.reid is None
    m.close()
    s = YOLO(path, random_init_ok=False)
    with pytest.raises(FileNotFoundError):
        s.track(frame, verbose=False, device=0, persist=True, tracker="bytetrack.yaml")
    s.close()
