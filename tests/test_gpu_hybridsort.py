"""Hybrid-SORT on the MI355X (csrc/ss_hybrid.hip) against its CPU reference (tests/hybridsort_ref.py), bit for bit."""
import functools

import numpy as np
import pytest
import torch

from strongsort_yolo_amd.config import HybridSortConfig
from strongsort_yolo_amd.synth import make_stream
from tests import byte_crowd
from tests.hybridsort_ref import HybridSortRef
from tests.hybridsort_scenes import CUES, SCENARIOS, cue_off
from tests.ocsort_scenes import EDGE_SIZES, edge_pair
from tests.test_bytetrack_cpu import byte_stream

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TABLE = ("track_id", "age", "time_since_update", "hits", "hit_streak", "frozen", "x", "P", "last_obs", "velocity", "conf", "conf_prev")


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
    ref = HybridSortRef(cfg)
    return [ref.update(d) for d in maker(*args)], ref


STREAM_RUNS = [(True, "hmiou", 0), (True, "hmiou", 1), (False, "hmiou", 0), (False, "hmiou", 1), (True, "iou", 0)]


@pytest.mark.parametrize("use_byte,asso,seed", STREAM_RUNS)
def test_group_rows_and_tables_equal_reference(use_byte, asso, seed):
    from strongsort_yolo_amd.engine import HybridSortEngine
    cfg = HybridSortConfig(use_byte=use_byte, asso=asso)
    streams = [byte_stream(10 * seed + s, 96) for s in range(3)]
    eng = HybridSortEngine(cfg, 3, 0)
    got = _run_engine(eng, streams, 32)
    for s in range(3):
        rows, ref = _reference(cfg, byte_stream, 10 * seed + s, 96)
        for k in range(96):
            _assert_rows(got[s][k], rows[k], f"use_byte {use_byte} {asso} seed {seed} stream {s} frame {k}")
        _assert_table(eng, s, ref, f"use_byte {use_byte} {asso} seed {seed} stream {s}")
    eng.close()


@pytest.mark.parametrize("use_byte", [False, True])
def test_streams_reach_every_branch(use_byte):
    """From the reference's own counters over the six hmiou streams of the test above.  The bounds are about half of what the
    reference counts on these seeds (with BYTE: 1 703 re-updated tracks, 415 LSAPs, 155 shortcuts, 2 clamps, 3 337 BYTE matches,
    491 525 non-zero TCM entries, 43 961 entries changed by the height factor; without: 3 354 re-updated tracks, 6 OCR matches)."""
    cfg, tot = HybridSortConfig(use_byte=use_byte), {}
    for seed in (0, 1):
        for s in range(3):
            for k, v in _reference(cfg, byte_stream, 10 * seed + s, 96)[1].counters.items():
                tot[k] = tot.get(k, 0) + int(v)
    print(tot)
    assert tot["lsap"] >= 200 and tot["shortcut"] >= 75 and tot["clamp"] >= 1
    assert tot["tcm"] >= 200000 and tot["height"] >= 15000 and tot["vel_over_one"] >= 3000
    if use_byte:
        assert tot["byte"] >= 1500 and tot["oru_tracks"] >= 800 and tot["byte_tcm_refused"] >= 1
    else:
        assert tot["ocr"] >= 1 and tot["oru_tracks"] >= 1500 and tot["byte"] == 0


def test_group_sizes_give_identical_rows():
    """Group sizes 1, 7 and 32: with size 1 every gap, ring entry and conf_prev crosses a call boundary."""
    from strongsort_yolo_amd.engine import HybridSortEngine
    cfg = HybridSortConfig()
    streams = [byte_stream(7 + s, 64) for s in range(2)]
    res = []
    for g in (1, 7, 32):
        eng = HybridSortEngine(cfg, 2, 0)
        res.append(_run_engine(eng, streams, g))
        for s in range(2):
            _assert_table(eng, s, _reference(cfg, byte_stream, 7 + s, 64)[1], f"group {g} stream {s}")
        eng.close()
    for s in range(2):
        rows, ref = _reference(cfg, byte_stream, 7 + s, 64)
        assert ref.counters["oru_tracks"] > 0 and ref.counters["byte"] > 0 and (ref.tracks()["conf_prev"] >= 0).any()
        for k in range(64):
            assert res[0][s][k].tobytes() == res[1][s][k].tobytes() == res[2][s][k].tobytes() == rows[k].tobytes(), f"stream {s} frame {k}"


@pytest.mark.parametrize("scene", ["two_crowds", "twin_crowds", "dense_crowd"])
def test_crowds_equal_reference(scene):
    from strongsort_yolo_amd.engine import HybridSortEngine
    cfg = HybridSortConfig()
    frames = getattr(byte_crowd, scene)(0)
    rows, ref = _reference(cfg, getattr(byte_crowd, scene), 0)
    eng = HybridSortEngine(cfg, 1, 0)
    got = _run_engine(eng, [frames], 32)
    for k in range(len(frames)):
        _assert_rows(got[0][k], rows[k], f"{scene} frame {k}")
    _assert_table(eng, 0, ref, scene)
    assert ref.counters["lsap"] >= 1
    eng.close()


def test_three_crowds_overflow_is_reported_and_reset_recovers():
    from strongsort_yolo_amd import lib
    from strongsort_yolo_amd.engine import HybridSortEngine
    cfg = HybridSortConfig()
    frames = byte_crowd.three_crowds(0)
    rows, ref = _reference(cfg, byte_crowd.three_crowds, 0)
    assert ref.capacity_error
    eng = HybridSortEngine(cfg, 1, 0)
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
    from strongsort_yolo_amd.engine import HybridSortEngine
    cfg = HybridSortConfig()
    frames = edge_pair(n_tracks, n_rows)
    rows, ref = _reference(cfg, edge_pair, n_tracks, n_rows)
    assert ref.counters["lsap"] == 1 and ref.counters["shortcut"] == 0 and len(frames[1]) == n_rows
    eng = HybridSortEngine(cfg, 1, 0)
    got = _run_engine(eng, [frames], 2)
    for k in range(2):
        _assert_rows(got[0][k], rows[k], f"edge pair {n_tracks} x {n_rows} frame {k}")
    _assert_table(eng, 0, ref, f"edge pair {n_tracks} x {n_rows}")
    eng.close()


def test_more_rows_than_a_frame_holds_is_flagged():
    from strongsort_yolo_amd import lib
    from strongsort_yolo_amd.engine import HybridSortEngine
    cfg = HybridSortConfig()
    eng, ref = HybridSortEngine(cfg, 1, 0), HybridSortRef(cfg)
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


def _scene_cases():
    for name in sorted(SCENARIOS):
        frames, cfg, _ = SCENARIOS[name]()
        yield pytest.param(frames, cfg, id=name)
    for name in sorted(CUES):
        frames, cfg, off, _ = CUES[name]()
        yield pytest.param(frames, cfg, id=f"{name}-on")
        yield pytest.param(frames, cue_off(cfg, off), id=f"{name}-off")


@pytest.mark.parametrize("frames,cfg", list(_scene_cases()))
def test_hand_built_scenes_on_device(frames, cfg):
    from strongsort_yolo_amd.tracker import HybridSORTTracker
    trk, ref = HybridSORTTracker(cfg), HybridSortRef(cfg)
    for k, d in enumerate(frames):
        _assert_rows(trk.update(d), ref.update(d), f"frame {k}")
    _assert_table(trk.eng, 0, ref, "table")
    trk.close()


@pytest.mark.parametrize("delta_t", [1, 8])
def test_delta_t_edges_equal_reference(delta_t):
    from strongsort_yolo_amd.engine import HybridSortEngine
    cfg = HybridSortConfig(delta_t=delta_t)
    frames = byte_stream(3, 48)
    rows, ref = _reference(cfg, byte_stream, 3, 48)
    eng = HybridSortEngine(cfg, 1, 0)
    got = _run_engine(eng, [frames], 32)
    for k in range(48):
        _assert_rows(got[0][k], rows[k], f"delta_t {delta_t} frame {k}")
    _assert_table(eng, 0, ref, f"delta_t {delta_t}")
    eng.close()


def test_recreating_the_state_and_resetting_one_stream_leave_the_other_alone():
    """A second engine on a live context replaces the state (ss_hybridsort_create) and starts clean; resetting stream 0 in the
    middle leaves stream 1's rows and table exactly the uninterrupted reference's."""
    from strongsort_yolo_amd.engine import HybridSortEngine, TrackerEngine
    from strongsort_yolo_amd.config import StrongSortConfig
    cfg = HybridSortConfig()
    streams = [byte_stream(20, 40), byte_stream(21, 40)]
    base = TrackerEngine(StrongSortConfig(), 2, 0)
    first = HybridSortEngine(cfg, engine=base)
    _run_engine(first, [s[:9] for s in streams], 9)                 # a used state ...
    eng = HybridSortEngine(cfg, engine=base)                        # ... replaced on the live context: ids restart at 1
    got = _run_engine(eng, [s[:16] for s in streams], 16)
    eng.reset(0)
    got2 = _run_engine(eng, [s[16:] for s in streams], 32)
    rows1, ref1 = _reference(cfg, byte_stream, 21, 40)
    for k in range(40):
        _assert_rows((got[1] + got2[1])[k], rows1[k], f"stream 1 frame {k}")
    _assert_table(eng, 1, ref1, "stream 1")
    ref0 = HybridSortRef(cfg)
    for k in range(16):
        _assert_rows(got[0][k], ref0.update(streams[0][k]), f"stream 0 frame {k}")
    ref0.reset()
    for k in range(16, 40):
        _assert_rows(got2[0][k - 16], ref0.update(streams[0][k]), f"stream 0 after its reset, frame {k}")
    _assert_table(eng, 0, ref0, "stream 0")
    eng.close()
    base.close()


# ---- YOLO(tracker_type="hybridsort") end to end (the synthetic-prediction set-up of tests/test_gpu_ocsort.py) ----------------------
H_, W_, NF_ = 480, 640, 24
CLUTTER_ = 24                     # as tests/test_gpu_ocsort.py: unmatched births live max_age frames, 24 anchors a frame keep the table open


def _hybrid_model(weights, **kw):
    from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry
    from strongsort_yolo_amd.synth import synth_prediction
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO(weights, tracker_type="hybridsort", **kw)
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


def test_yolo_hybridsort_track_and_stream_equal_reference():
    model, frames = _hybrid_model("yolov8n.pt", random_init_ok=True)
    ref, per_frame, low, shown = HybridSortRef(HybridSortConfig()), [], 0, 0
    for k in range(NF_):
        res = model.track(frames[k], verbose=False, device=0, persist=True, tracker="hybridsort.yaml")
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
    assert not ref.capacity_error and ref.counters["match"] > 4 * NF_ and ref.counters["byte"] > 0
    model._frame_index = 0
    got = list(model.track_stream(frames, batch=32))
    assert model._stream_pipe.reid is None and len(got) == NF_
    for k, (a, b) in enumerate(zip(got, per_frame)):
        a = a[0]
        assert len(a.boxes) == len(b.boxes), f"frame {k}"
        if len(b.boxes):
            assert torch.equal(a.boxes.id, b.boxes.id) and torch.equal(a.boxes.xyxy, b.boxes.xyxy) and torch.equal(a.boxes.conf, b.boxes.conf)
    model.close()
