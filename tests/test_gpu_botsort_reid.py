"""BoT-SORT's ReID branch on the MI355X (csrc/ss_byte.hip: k_byte_feats and k_byte_group's REID variants, docs/BYTETRACK.md
§1c) against tests/botsort_reid_ref.py, bit for bit: rows, track tables and smoothed features over seeded streams with
per-identity features and swapped-appearance crossings, group sizes, camera motion, reset and capacity, and
YOLO(tracker_type="botsort", with_reid=True) end to end."""
import numpy as np
import pytest
import torch

from strongsort_yolo_amd.config import ByteTrackConfig
from strongsort_yolo_amd.synth import make_stream
from tests.botsort_reid_ref import BotSortReidRef
from tests.bytetrack_ref import ByteTrackRef
from tests.test_gpu_botsort_gmc import _warps

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
REID = ByteTrackConfig(kalman="xywh", with_reid=True)
XYWH = ByteTrackConfig(kalman="xywh")


def _iou(a, b):
    w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    i = w * h
    return i / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - i)


def reid_stream(seed, n_frames, width=1280, height=720, n_ids=28):
    """tests/test_bytetrack_cpu.byte_stream's perturbations (low scores, threshold scores, dropped sightings, false positives)
    with raw features: every identity's synth feature (noise 0.02) at a random scale, random ones for the false positives,
    an all-zero row now and then, and crossings: the features of two overlapping rows swapped.
    -> [(dets [N,6] f32, feats [N,512] f32)]"""
    st, rng = make_stream(seed, width, height, n_ids), np.random.default_rng(2000 + seed)
    out = []
    for _ in range(n_frames):
        fr = st.next_frame()
        d = fr.dets.astype(np.float32).copy()
        f = (fr.feats * rng.uniform(0.5, 3.0, (len(d), 1))).astype(np.float32)
        n = len(d)
        low = rng.random(n) < 0.25
        d[low, 4] = rng.uniform(0.1, 0.25, int(low.sum())).astype(np.float32)
        edge = rng.random(n) < 0.03
        d[edge, 4] = rng.choice(np.array([0.25, 0.1], np.float32), int(edge.sum()))
        keep = rng.random(n) >= 0.1
        d, f = d[keep], f[keep]
        pairs = [(i, j) for i in range(len(d)) for j in range(i + 1, len(d)) if _iou(d[i], d[j]) > 0.2]
        for i, j in pairs:
            if rng.random() < 0.5:
                f[[i, j]] = f[[j, i]]
        if len(d) and rng.random() < 0.05:
            f[int(rng.integers(0, len(d)))] = 0.0
        k = int(rng.integers(0, 3))
        if k:
            x, y = rng.uniform(0, width - 80, k), rng.uniform(0, height - 160, k)
            w, h = rng.uniform(20, 80, k), rng.uniform(40, 160, k)
            fp = np.stack([x, y, x + w, y + h, rng.uniform(0.1, 0.7, k), rng.integers(0, 3, k)], 1).astype(np.float32)
            d = np.concatenate([d, fp])
            f = np.concatenate([f, rng.standard_normal((k, 512)).astype(np.float32)])
        out.append((np.ascontiguousarray(d[:128]), np.ascontiguousarray(f[:128])))
    return out


def _run_engine(eng, streams, group, warps=None, feats=True):
    """streams: per stream a list of (dets, feats) -> per stream a list of rows; warps [F,S,8] (host) installed per call."""
    S, F = len(streams), len(streams[0])
    out_all = [[] for _ in range(S)]
    out = torch.zeros(32, S, 256, 8, device=DEV)
    nout = torch.zeros(32, S, dtype=torch.int32, device=DEV)
    for f0 in range(0, F, group):
        n = min(group, F - f0)
        hd, hn = np.zeros((n, S, 128, 6), np.float32), np.zeros((n, S), np.int32)
        hf = np.zeros((n, S, 128, 512), np.float32)
        for f in range(n):
            for s in range(S):
                d, ft = streams[s][f0 + f]
                hd[f, s, :len(d)], hf[f, s, :len(d)], hn[f, s] = d, ft, len(d)
        if warps is not None:
            eng.set_cmc(torch.from_numpy(np.ascontiguousarray(warps[f0:f0 + n])).to(DEV))
        eng.update_group(n, torch.from_numpy(hd).to(DEV), torch.from_numpy(hn).to(DEV), torch.from_numpy(hf).to(DEV) if feats else None,
                         None, out[:n], nout[:n])
        eng.check_errors()
        ho, hno = out[:n].cpu().numpy(), nout[:n].cpu().numpy()
        for f in range(n):
            for s in range(S):
                out_all[s].append(ho[f, s, :hno[f, s]].copy())
    return out_all


def _assert_rows(got, ref, what):
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), f"{what}:\n{got}\n!=\n{ref}"


def _assert_table(eng, s, ref, what):
    t = eng.tracks(s)
    ids, st, act, mean = ref.tracks()
    assert t["n_tracked"] == len(ref.tracked) and t["n_lost"] == len(ref.lost) and t["next_id"] == ref.next_id, what
    assert np.array_equal(t["track_id"], ids) and np.array_equal(t["state"], st) and np.array_equal(t["activated"], act), what
    assert t["mean"].tobytes() == mean.tobytes(), f"{what}: track means"
    assert eng.features(s).tobytes() == ref.features().tobytes(), f"{what}: smoothed features"


def _check(streams, got, warps=None, what=""):
    refs = []
    for s in range(len(streams)):
        ref = BotSortReidRef(REID)
        for k, (d, f) in enumerate(streams[s]):
            _assert_rows(got[s][k], ref.update(d, f, None if warps is None else warps[k, s]), f"{what} stream {s} frame {k}")
        refs.append(ref)
    return refs


def test_rows_tables_and_features_equal_reference():
    from strongsort_yolo_amd.engine import ByteTrackEngine
    swaps = 0
    for seed in (0, 1, 2):
        streams = [reid_stream(10 * seed + s, 150) for s in range(3)]
        eng = ByteTrackEngine(REID, 3, 0)
        got = _run_engine(eng, streams, 32)
        refs = _check(streams, got, what=f"seed {seed}")
        for s, ref in enumerate(refs):
            _assert_table(eng, s, ref, f"seed {seed} stream {s}")
        # the appearance term changed some association: the same rows without ReID differ somewhere
        for s in range(3):
            plain = ByteTrackRef(XYWH)
            swaps += sum(plain.update(d).tobytes() != got[s][k].tobytes() for k, (d, _) in enumerate(streams[s]))
        eng.close()
    assert swaps > 0


def test_group_sizes_give_identical_rows_and_features():
    from strongsort_yolo_amd.engine import ByteTrackEngine
    streams = [reid_stream(7 + s, 64) for s in range(2)]
    res, feats = [], []
    for g in (1, 7, 32):
        eng = ByteTrackEngine(REID, 2, 0)
        res.append(_run_engine(eng, streams, g))
        feats.append([eng.features(s).tobytes() for s in range(2)])
        eng.close()
    for s in range(2):
        for k in range(64):
            assert res[0][s][k].tobytes() == res[1][s][k].tobytes() == res[2][s][k].tobytes(), f"stream {s} frame {k}"
        assert feats[0][s] == feats[1][s] == feats[2][s]
    _check(streams, res[0], what="group 1")


def test_reid_with_camera_motion_equals_reference():
    from strongsort_yolo_amd.engine import ByteTrackEngine
    streams = [reid_stream(30 + s, 96) for s in range(3)]
    w = _warps(5, 96, 3)
    eng = ByteTrackEngine(REID, 3, 0)
    got = _run_engine(eng, streams, 32, w)
    refs = _check(streams, got, w, "gmc")
    for s, ref in enumerate(refs):
        _assert_table(eng, s, ref, f"gmc stream {s}")
    eng.close()


def test_plain_botsort_is_unchanged():
    from strongsort_yolo_amd.engine import ByteTrackEngine
    streams = [reid_stream(40 + s, 80) for s in range(2)]
    eng = ByteTrackEngine(XYWH, 2, 0)
    got = _run_engine(eng, streams, 32, feats=False)
    for s in range(2):
        ref = ByteTrackRef(XYWH)
        for k, (d, _) in enumerate(streams[s]):
            _assert_rows(got[s][k], ref.update(d), f"plain stream {s} frame {k}")
    eng.close()


def test_reset_one_stream_and_errors():
    from strongsort_yolo_amd import lib
    from strongsort_yolo_amd.engine import ByteTrackEngine, TrackerEngine
    streams = [reid_stream(50 + s, 60) for s in range(2)]
    eng = ByteTrackEngine(REID, 2, 0)
    a = _run_engine(eng, [st[:30] for st in streams], 16)
    eng.reset(1)
    assert eng.features(1).shape == (0, 512) and eng.features(0).shape[0] > 0
    b = _run_engine(eng, [st[30:] for st in streams], 16)
    ref0 = _check([streams[0]], [a[0] + b[0]], what="kept")[0]
    ref1 = _check([streams[1][30:]], [b[1]], what="after reset")[0]
    _assert_table(eng, 0, ref0, "kept stream")
    _assert_table(eng, 1, ref1, "reset stream")
    dets = torch.zeros(1, 2, 128, 6, device=DEV)
    n = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):                               # ReID needs features
        eng.update_group(1, dets, n, None, None, eng.out[None], eng.nout[None])
    with pytest.raises(lib.SSError) as ei:                        # ... and the featureless entry point refuses
        eng._ck(eng.L.ss_byte_update_group(eng.ctx, 1, dets.data_ptr(), n.data_ptr(), eng.out.data_ptr(), eng.nout.data_ptr()))
    assert ei.value.code == lib.SS_ERR_INVALID
    eng.close()
    # capacity: births beyond max_tracks are dropped (as the reference drops them) and reported
    small = ByteTrackConfig(kalman="xywh", with_reid=True, max_tracks=6)
    st = reid_stream(60, 12)
    eng = ByteTrackEngine(small, 1, 0)
    with pytest.raises(lib.SSError) as ei:
        _run_engine(eng, [st], 12)
    assert ei.value.code == lib.SS_ERR_CAPACITY
    ref = BotSortReidRef(small)
    for d, f in st:
        ref.update(d, f)
    assert ref.capacity_error
    _assert_table(eng, 0, ref, "capacity")
    eng.close()
    # no ReID on ByteTrack, no features before ReID was ever on
    x = ByteTrackEngine(ByteTrackConfig(kalman="xyah"), 1, 0)
    with pytest.raises(lib.SSError) as ei:
        x._ck(x.L.ss_byte_set_reid(x.ctx, 1, 0.5, 0.25, 0.9))
    assert ei.value.code == lib.SS_ERR_INVALID
    with pytest.raises(RuntimeError):
        x.features(0)
    sm = np.zeros((256, 512), np.float32)
    with pytest.raises(lib.SSError):
        x._ck(x.L.ss_byte_get_features(x.ctx, 0, 256, sm.ctypes.data_as(lib.C.POINTER(lib.C.c_float))))
    x.close()
    base = TrackerEngine(n_streams=1)
    with pytest.raises(lib.SSError):
        base._ck(base.L.ss_byte_set_reid(base.ctx, 1, 0.5, 0.25, 0.9))
    base.close()


def test_bytetracker_with_reid():
    from strongsort_yolo_amd.tracker import BYTETracker
    st = reid_stream(70, 40)
    trk, ref = BYTETracker(REID, random_init_ok=True), BotSortReidRef(REID)
    for k, (d, f) in enumerate(st):
        _assert_rows(trk.update(d, features=f), ref.update(d, f), f"frame {k}")
    with pytest.raises(ValueError):                               # neither a frame nor features
        trk.update(st[0][0])
    # the tracker's own crops and OSNet: the rows equal the reference fed with the features it computed
    trk.reset()
    ref = BotSortReidRef(REID)
    s2 = make_stream(71, 640, 480, 8)
    for k in range(12):
        fr = s2.next_frame()
        d = fr.dets.astype(np.float32)
        rows = trk.update(d, s2.frame_pixels(k))
        _assert_rows(rows, ref.update(d, trk._feats[0, :len(d)].cpu().numpy()), f"own features, frame {k}")
    trk.close()


# ---- YOLO(tracker_type="botsort", with_reid=True) end to end ---------------------------------------------------------------
H_, W_, NF_ = 480, 640, 24


def _reid_model(feat_source, reid_fp32=True):
    """Synthetic detector heads; the tracker reads OSNet's features of the crops (feat_source "reid") or the identities'
    synthetic features (feat_source "by_anchor": OSNet still runs)."""
    from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry
    from strongsort_yolo_amd.synth import synth_prediction
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", with_reid=True, reid_fp32=reid_fp32)
    model.overrides.update(conf=0.3, iou=0.4, agnostic_nms=False, max_det=1000)
    model._pipe_kw.update(det_source="synthetic", feat_source=feat_source, reid_batch=32)
    g = letterbox_geometry(H_, W_)
    gs = scale_geometry(g, H_, W_)
    A = sum((g.out_h // s) * (g.out_w // s) for s in (8, 16, 32))
    st, rng = make_stream(45, W_, H_, 9), np.random.default_rng(45)
    frames, preds, agts, feats = [], [], [], []
    for k in range(NF_):
        fr = st.next_frame()
        d = fr.dets.copy()
        d[:, 4] = np.where(rng.random(len(d)) < 0.3, rng.uniform(0.12, 0.24, len(d)), d[:, 4]).astype(np.float32)
        pred, agt = synth_prediction(d, A, 80, gs[0], (gs[1], gs[2]), rng)
        f = np.zeros((128, 512), np.float32)
        f[:len(fr.feats)] = fr.feats
        frames.append(st.frame_pixels(k).copy()); preds.append(pred); agts.append(agt); feats.append(f)
    dp, da, df = (torch.from_numpy(np.stack(x)).to(DEV) for x in (preds, agts, feats))

    def fill(b, v, k):
        b.pred_in[v].copy_(dp[k]); b.anchor_gt[v].copy_(da[k]); b.gt_feats[v].copy_(df[k])

    model._fill = fill
    return model, frames


def _same(a, b, what):
    assert len(a.boxes) == len(b.boxes), what
    if len(b.boxes):
        assert torch.equal(a.boxes.id, b.boxes.id) and torch.equal(a.boxes.xyxy, b.boxes.xyxy) and torch.equal(a.boxes.conf, b.boxes.conf), what


def _track_against_engine(model, frames):
    """track() frame by frame; every frame's rows equal a ByteTrackEngine (and the reference) fed with the pipeline's own
    rows and features."""
    from strongsort_yolo_amd.engine import ByteTrackEngine
    eng, ref, per_frame = ByteTrackEngine(REID, 1, 0), BotSortReidRef(REID), []
    for k in range(NF_):
        res = model.track(frames[k], verbose=False, device=0, persist=True, tracker="botsort.yaml")
        pipe = model._pipe
        assert pipe.reid is not None and pipe.byte is not None and pipe.byte.reid and pipe.max_det == (32 if pipe.feat_source == "reid" else 128)
        rows = pipe.detections()[0][:, :6]
        feats = pipe.feats_in[0, :len(rows)].cpu().numpy()
        d = torch.zeros(1, 128, 6, device=DEV)
        f = torch.zeros(1, 128, 512, device=DEV)
        d[0, :len(rows)], f[0, :len(rows)] = torch.from_numpy(rows).to(DEV), torch.from_numpy(feats).to(DEV)
        o, n = eng.update_device(d, torch.full((1,), len(rows), dtype=torch.int32, device=DEV), f)
        e = o[0, :int(n[0])].cpu().numpy()
        _assert_rows(e, ref.update(rows, feats), f"engine, frame {k}")
        r = res[0]
        assert len(r.boxes) == len(e), f"frame {k}"
        if len(e):
            assert np.array_equal(r.boxes.id.numpy(), e[:, 4]) and np.array_equal(r.boxes.xyxy.numpy(), e[:, :4]), f"frame {k}"
        per_frame.append(r)
    eng.close()
    return per_frame


@pytest.mark.parametrize("reid_fp32", [True, False])
def test_yolo_track_with_osnet_features_equals_engine(reid_fp32):
    model, frames = _reid_model("reid", reid_fp32)
    _track_against_engine(model, frames)
    assert model._pipe.reid_half == (not reid_fp32)
    model.close()


def test_yolo_track_and_track_stream_equal():
    model, frames = _reid_model("by_anchor")
    per_frame = _track_against_engine(model, frames)
    for batch in (32, 7):                                          # a full group; a partial last group (24 = 3 x 7 + 3)
        model._frame_index = 0
        got = list(model.track_stream(frames, batch=batch))
        assert len(got) == NF_ and model._stream_pipe.reid is not None and model._stream_pipe.byte.reid
        for k, (a, b) in enumerate(zip(got, per_frame)):
            _same(a[0], b, f"track_stream batch {batch} frame {k}")
    model.close()
