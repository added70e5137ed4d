"""OC-SORT on the MI355X (csrc/ss_ocsort.hip) against its CPU reference (tests/ocsort_ref.py), bit for bit."""
import functools

import numpy as np
import pytest
import torch

from strongsort_yolo_amd.config import OCSortConfig
from strongsort_yolo_amd.synth import make_stream
from tests import byte_crowd
from tests.ocsort_ref import OCSortRef
from tests.ocsort_scenes import EDGE_SIZES, SCENARIOS, edge_pair
from tests.test_bytetrack_cpu import byte_stream

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TABLE = ("track_id", "age", "time_since_update", "hits", "hit_streak", "frozen", "x", "P", "last_obs", "velocity")


def _run_engine(eng, streams, group, check=True):
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
        if check:
            eng.check_errors()
        ho, hno = out[:n].cpu().numpy(), nout[:n].cpu().numpy()
        for f in range(n):
            for s in range(S):
                out_all[s].append(ho[f, s, :hno[f, s]].copy())
    return out_all


def _assert_rows(got, ref, what):
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), f"{what}:\n{got}\n!=\n{ref}"


def _assert_table(eng, s, ref, what):
    t, r = eng.tracks(s), ref.tracks()
    assert (t["n_tracks"], t["next_id"], t["frame_count"]) == (r["n_tracks"], r["next_id"], r["frame_count"]), what
    for k in TABLE:
        assert t[k].shape == r[k].shape and t[k].tobytes() == r[k].tobytes(), f"{what}: {k}\n{t[k]}\n!=\n{r[k]}"


@functools.lru_cache(maxsize=None)
def _reference(cfg, maker, *args):
    """One reference run per (configuration, scene), shared by the tests and never changed: (rows per frame, the reference)."""
    ref = OCSortRef(cfg)
    return [ref.update(d) for d in maker(*args)], ref


@pytest.mark.parametrize("use_byte", [False, True])
@pytest.mark.parametrize("seed", [0, 1])
def test_group_rows_and_tables_equal_reference(seed, use_byte):
    from strongsort_yolo_amd.engine import OCSortEngine
    cfg = OCSortConfig(use_byte=use_byte)
    streams = [byte_stream(10 * seed + s, 96) for s in range(3)]
    eng = OCSortEngine(cfg, 3, 0)
    got = _run_engine(eng, streams, 32)
    for s in range(3):
        rows, ref = _reference(cfg, byte_stream, 10 * seed + s, 96)
        for k in range(96):
            _assert_rows(got[s][k], rows[k], f"use_byte {use_byte} seed {seed} stream {s} frame {k}")
        _assert_table(eng, s, ref, f"use_byte {use_byte} seed {seed} stream {s}")
    eng.close()


@pytest.mark.parametrize("use_byte", [False, True])
def test_streams_reach_every_branch(use_byte):
    """From the reference's own counters over the six streams of the test above."""
    cfg, tot = OCSortConfig(use_byte=use_byte), {}
    for seed in (0, 1):
        for s in range(3):
            for k, v in _reference(cfg, byte_stream, 10 * seed + s, 96)[1].counters.items():
                tot[k] = tot.get(k, 0) + v
    print(tot)
    assert tot["oru_tracks"] >= 500 and tot["lsap"] >= 100 and tot["shortcut"] >= 1 and tot["clamp"] >= 1
    if use_byte:
        assert tot["byte"] >= 1000
    else:
        assert tot["ocr"] >= 1


def test_group_sizes_give_identical_rows():
    from strongsort_yolo_amd.engine import OCSortEngine
    streams = [byte_stream(7 + s, 64) for s in range(2)]
    res = []
    for g in (1, 7, 32):
        eng = OCSortEngine(OCSortConfig(), 2, 0)
        res.append(_run_engine(eng, streams, g))
        eng.close()
    for s in range(2):
        rows, ref = _reference(OCSortConfig(), byte_stream, 7 + s, 64)
        assert ref.counters["oru_tracks"] > 0
        for k in range(64):
            assert res[0][s][k].tobytes() == res[1][s][k].tobytes() == res[2][s][k].tobytes() == rows[k].tobytes(), f"stream {s} frame {k}"


@pytest.mark.parametrize("scene", ["two_crowds", "twin_crowds", "dense_crowd"])
def test_crowds_equal_reference(scene):
    from strongsort_yolo_amd.engine import OCSortEngine
    cfg = OCSortConfig()
    frames = getattr(byte_crowd, scene)(0)
    rows, ref = _reference(cfg, getattr(byte_crowd, scene), 0)
    eng = OCSortEngine(cfg, 1, 0)
    got = _run_engine(eng, [frames], 32)
    for k in range(len(frames)):
        _assert_rows(got[0][k], rows[k], f"{scene} frame {k}")
    _assert_table(eng, 0, ref, scene)
    assert ref.counters["lsap"] >= 1
    eng.close()


def test_three_crowds_overflow_is_reported_and_reset_recovers():
    from strongsort_yolo_amd import lib
    from strongsort_yolo_amd.engine import OCSortEngine
    cfg = OCSortConfig()
    frames = byte_crowd.three_crowds(0)
    rows, ref = _reference(cfg, byte_crowd.three_crowds, 0)
    assert ref.capacity_error
    eng = OCSortEngine(cfg, 1, 0)
    got = _run_engine(eng, [frames], 32, check=False)
    for k in range(len(frames)):
        _assert_rows(got[0][k], rows[k], f"three_crowds frame {k}")
    with pytest.raises(lib.SSError) as ei:
        eng.check_errors()
    assert ei.value.code == lib.SS_ERR_CAPACITY
    assert eng.tracks(0)["n_tracks"] <= 256
    _assert_table(eng, 0, ref, "three_crowds")
    eng.reset()
    eng.check_errors()
    got = _run_engine(eng, [frames[:2]], 2)
    for k in range(2):
        _assert_rows(got[0][k], rows[k], f"after reset, frame {k}")
    eng.close()


@pytest.mark.parametrize("n_tracks,n_rows", EDGE_SIZES)
def test_edge_sizes_equal_reference(n_tracks, n_rows):
    from strongsort_yolo_amd.engine import OCSortEngine
    cfg = OCSortConfig()
    frames = edge_pair(n_tracks, n_rows)
    rows, ref = _reference(cfg, edge_pair, n_tracks, n_rows)
    assert ref.counters["lsap"] == 1 and ref.counters["shortcut"] == 0 and len(frames[1]) == n_rows
    eng = OCSortEngine(cfg, 1, 0)
    got = _run_engine(eng, [frames], 2)
    for k in range(2):
        _assert_rows(got[0][k], rows[k], f"edge pair {n_tracks} x {n_rows} frame {k}")
    _assert_table(eng, 0, ref, f"edge pair {n_tracks} x {n_rows}")
    eng.close()


def test_more_rows_than_a_frame_holds_is_flagged():
    from strongsort_yolo_amd import lib
    from strongsort_yolo_amd.engine import OCSortEngine
    cfg = OCSortConfig()
    eng, ref = OCSortEngine(cfg, 1, 0), OCSortRef(cfg)
    d = byte_crowd._rows(byte_crowd._lattice(16, 9, 70.0, 50.0), 44.0, 30.0, np.full(144, 0.8))
    hd = torch.zeros(1, 1, 128, 6, device=DEV)
    hd[0, 0] = torch.from_numpy(d[:128])
    out, nout = torch.zeros(1, 1, 256, 8, device=DEV), torch.zeros(1, 1, dtype=torch.int32, device=DEV)
    eng.update_group(1, hd, torch.tensor([[144]], dtype=torch.int32, device=DEV), None, None, out, nout)
    _assert_rows(out[0, 0, :int(nout[0, 0])].cpu().numpy(), ref.update(d), "first 128 rows")
    assert ref.capacity_error
    with pytest.raises(lib.SSError) as ei:
        eng.check_errors()
    assert ei.value.code == lib.SS_ERR_CAPACITY
    eng.close()


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_hand_built_scenarios_on_device(name):
    from strongsort_yolo_amd.tracker import OCSORTTracker
    frames, cfg, _ = SCENARIOS[name]()
    trk, ref = OCSORTTracker(cfg), OCSortRef(cfg)
    for k, d in enumerate(frames):
        _assert_rows(trk.update(d), ref.update(d), f"{name} frame {k}")
    _assert_table(trk.eng, 0, ref, name)
    trk.close()


@pytest.mark.parametrize("delta_t", [1, 8])
def test_delta_t_edges_equal_reference(delta_t):
    from strongsort_yolo_amd.engine import OCSortEngine
    cfg = OCSortConfig(delta_t=delta_t)
    frames = byte_stream(3, 48)
    rows, ref = _reference(cfg, byte_stream, 3, 48)
    eng = OCSortEngine(cfg, 1, 0)
    got = _run_engine(eng, [frames], 32)
    for k in range(48):
        _assert_rows(got[0][k], rows[k], f"delta_t {delta_t} frame {k}")
    _assert_table(eng, 0, ref, f"delta_t {delta_t}")
    eng.close()


# ---- YOLO(tracker_type="ocsort") end to end (the synthetic-prediction set-up of tests/test_gpu_bytetrack.py) ---------------------
H_, W_, NF_ = 480, 640, 24
# synth_prediction's clutter anchors score in (0.1, 0.29): below the set-up's conf 0.3, but rows at the tracking conf 0.1, a fifth
# of them above det_thresh.  OC-SORT keeps an unmatched birth for max_age = 30 frames (the BYTE family drops an unconfirmed
# track after one), so the default 200 anchors a frame (about 45 births) fill the 256 slots by frame 8; 24 anchors a frame (about
# 5 births) leave the 24 frames well inside the table, and low-score rows still reach the tracker.
CLUTTER_ = 24


def _ocsort_model(weights, **kw):
    from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry
    from strongsort_yolo_amd.synth import synth_prediction
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO(weights, tracker_type="ocsort", **kw)
    model.overrides.update(conf=0.3, iou=0.4, agnostic_nms=False, max_det=1000)
    model._pipe_kw.update(det_source="synthetic")
    g = letterbox_geometry(H_, W_)
    gs = scale_geometry(g, H_, W_)
    A = sum((g.out_h // s) * (g.out_w // s) for s in (8, 16, 32))
    st, rng = make_stream(43, W_, H_, 9), np.random.default_rng(43)
    frames, preds = [], []
    for k in range(NF_):
        d = st.next_frame().dets.copy()
        d[:, 4] = np.where(rng.random(len(d)) < 0.3, rng.uniform(0.12, 0.24, len(d)), d[:, 4]).astype(np.float32)   # low-score rows
        pred, _ = synth_prediction(d, A, 80, gs[0], (gs[1], gs[2]), rng, clutter=CLUTTER_)
        frames.append(st.frame_pixels(k).copy()); preds.append(pred)
    dp = torch.from_numpy(np.stack(preds)).to(DEV)
    model._fill = lambda b, v, k: b.pred_in[v].copy_(dp[k])
    return model, frames


@pytest.mark.parametrize("use_byte", [False, True])
def test_yolo_ocsort_track_and_stream_equal_reference(use_byte):
    model, frames = _ocsort_model("yolov8n.pt", random_init_ok=True, ocsort_use_byte=use_byte)
    ref, per_frame, low, shown = OCSortRef(OCSortConfig(use_byte=use_byte)), [], 0, 0
    for k in range(NF_):
        res = model.track(frames[k], verbose=False, device=0, persist=True, tracker="ocsort.yaml")
        pipe = model._pipe
        assert pipe.reid is None and pipe.dcfg.conf == 0.1
        rows = pipe.detections()[0]
        assert (rows[:, 4] > np.float32(0.1)).all()
        low += int((rows[:, 4] < 0.25).sum())
        exp = ref.update(rows[:, :6])
        r = res[0]
        assert len(r.boxes) == len(exp), f"frame {k}"
        shown += len(exp)
        if len(exp):
            assert np.array_equal(r.boxes.id.numpy(), exp[:, 4]) and np.array_equal(r.boxes.xyxy.numpy(), exp[:, :4])
            assert np.array_equal(r.boxes.cls.numpy(), exp[:, 5]) and np.array_equal(r.boxes.conf.numpy(), exp[:, 6])
        per_frame.append(r)
    assert low > 0 and shown > NF_, "low-score rows reach the tracker, and tracks are shown"
    assert not ref.capacity_error and ref.counters["match"] > 4 * NF_
    assert ref.counters["byte"] > 0 if use_byte else ref.counters["byte"] == 0
    model._frame_index = 0
    got = list(model.track_stream(frames, batch=32))
    assert model._stream_pipe.reid is None and len(got) == NF_
    for k, (a, b) in enumerate(zip(got, per_frame)):
        a = a[0]
        assert len(a.boxes) == len(b.boxes), f"frame {k}"
        if len(b.boxes):
            assert torch.equal(a.boxes.id, b.boxes.id) and torch.equal(a.boxes.xyxy, b.boxes.xyxy) and torch.equal(a.boxes.conf, b.boxes.conf)
    model.close()
