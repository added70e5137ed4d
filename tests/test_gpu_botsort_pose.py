"""BoT-SORT's keypoint term on the MI355X (csrc/ss_byte.hip: k_byte_kpts and k_byte_group's POSE variants, docs/BYTETRACK.md
§1e) against tests/botsort_pose_ref.py, bit for bit: the prepared keypoints, rows, track tables and stored poses over crossing
and perturbed streams, group sizes, stream counts, camera motion, full frames and the spilled cost matrix, capacity, reset,
graph capture, the refusals, and YOLO("yolo11n-pose.pt", tracker_type="botsort", with_pose=True) end to end."""
import numpy as np
import pytest
import torch

from strongsort_yolo_amd.config import ByteTrackConfig
from strongsort_yolo_amd.synth import make_stream
from tests.botsort_pose_ref import BotSortPoseRef, original_pixels, visible
from tests.bytetrack_ref import ByteTrackRef
from tests.test_botsort_pose_cpu import K, crossing_stream, place, pose_stream, skeleton
from tests.test_gpu_botsort_gmc import _warps

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
POSE = ByteTrackConfig(kalman="xywh", with_pose=True)
XYWH = ByteTrackConfig(kalman="xywh")


def _crossing(seed, n):
    return [(d, k) for d, k, _ in crossing_stream(seed, n)]


def _pack(streams, f0, n):
    S = len(streams)
    hd, hn, hk = np.zeros((n, S, 128, 6), np.float32), np.zeros((n, S), np.int32), np.zeros((n, S, 128, K, 3), np.float32)
    for f in range(n):
        for s in range(S):
            d, kp = streams[s][f0 + f]
            hd[f, s, :len(d)], hk[f, s, :len(d)], hn[f, s] = d, kp, len(d)
    return hd, hn, hk


def _run_engine(eng, streams, group, warps=None, kpts=True):
    """streams: per stream a list of (dets, kpts) -> per stream a list of rows; warps [F,S,8] (host) installed per call."""
    S, F = len(streams), len(streams[0])
    out_all = [[] for _ in range(S)]
    out = torch.zeros(32, S, 256, 8, device=DEV)
    nout = torch.zeros(32, S, dtype=torch.int32, device=DEV)
    for f0 in range(0, F, group):
        n = min(group, F - f0)
        hd, hn, hk = _pack(streams, f0, n)
        if warps is not None:
            eng.set_cmc(torch.from_numpy(np.ascontiguousarray(warps[f0:f0 + n])).to(DEV))
        eng.update_group(n, torch.from_numpy(hd).to(DEV), torch.from_numpy(hn).to(DEV), None, None, out[:n], nout[:n],
                         kpts=torch.from_numpy(hk).to(DEV) if kpts else None)
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
    off, vis = eng.keypoints(s)
    roff, rvis = ref.keypoints()
    assert np.array_equal(vis, rvis), f"{what}: pose visibility"
    assert off.tobytes() == roff.tobytes(), f"{what}: stored poses"


def _check(streams, got, warps=None, what="", cfg=POSE):
    refs = []
    for s in range(len(streams)):
        ref = BotSortPoseRef(cfg)
        for k, (d, kp) in enumerate(streams[s]):
            _assert_rows(got[s][k], ref.update(d, kp, None if warps is None else warps[k, s]), f"{what} stream {s} frame {k}")
        refs.append(ref)
    return refs


def _engine(cfg, S):
    from strongsort_yolo_amd.engine import ByteTrackEngine
    return ByteTrackEngine(cfg, S, 0)


# ---- k_byte_kpts ----------------------------------------------------------------------------------------------------------
def test_prepared_keypoints_geometry_path_and_flag_path():
    rng = np.random.default_rng(4)
    F, S, C_ = 3, 2, 6 + 3 * K + 5                                 # NMS-shaped rows: box, keypoints from column 6, 5 more columns
    eng = _engine(POSE, S)
    rows = rng.uniform(0, 640, (F * S, 128, C_)).astype(np.float32)
    rows[..., 6 + 2:6 + 3 * K:3] = rng.uniform(0, 1, (F * S, 128, K))
    rows[:, ::7, 6 + 2] = np.float32(0.5)                          # exactly at the threshold: visible
    nd = rng.integers(0, 129, (F, S)).astype(np.int32)
    nd[0, 0], nd[0, 1] = 128, 0
    geom = np.array([[0.5, 0.0, 12.0, 1280, 720], [0.4321, 7.5, 0.0, 1280, 720]] * 3, np.float32)
    xy, wh = rng.uniform(0, 1100, (F, S, 128, 2)), rng.uniform(30, 150, (F, S, 128, 2))
    dets = torch.from_numpy(np.concatenate([xy, xy + wh, rng.uniform(0.3, 0.9, (F, S, 128, 1)), np.zeros((F, S, 128, 1))], -1).astype(np.float32)).to(DEV)
    out, nout = torch.zeros(F, S, 256, 8, device=DEV), torch.zeros(F, S, dtype=torch.int32, device=DEV)
    kp = rows[..., 6:6 + 3 * K].reshape(F * S, 128, K, 3)
    for use_geom in (True, False):
        if use_geom:
            eng.update_group(F, dets, torch.from_numpy(nd).to(DEV), None, None, out, nout, kpts=torch.from_numpy(rows).to(DEV), kpt_col=6,
                             geom=torch.from_numpy(geom).to(DEV))
        else:
            eng.update_group(F, dets, torch.from_numpy(nd).to(DEV), None, None, out, nout,
                             kpts=torch.from_numpy(np.ascontiguousarray(kp)).to(DEV).view(F, S, 128, K, 3))
        for f in range(F):
            for s in range(S):
                i, n = f * S + s, int(nd[f, s])
                exp = original_pixels(kp[i], *geom[i, :3]) if use_geom else kp[i]
                xy, vis = eng.det_keypoints(f, s)
                assert xy[:n].tobytes() == np.ascontiguousarray(exp[:n, :, :2]).tobytes(), f"geom {use_geom} image {f},{s}"
                words = [sum(1 << k for k in range(K) if v[k]) for v in visible(kp[i][:n], 0.5)]
                assert list(vis[:n]) == words, f"geom {use_geom} image {f},{s}: visibility"
        eng.reset(-1)
    eng.close()


# ---- rows, tables, poses --------------------------------------------------------------------------------------------------
def test_crossing_streams_equal_reference():
    differs = 0
    for seed in (0, 3):
        streams = [_crossing(seed + s, 90) for s in range(3)]
        eng = _engine(POSE, 3)
        got = _run_engine(eng, streams, 32)
        for s, ref in enumerate(_check(streams, got, what=f"crossing seed {seed}")):
            _assert_table(eng, s, ref, f"crossing seed {seed} stream {s}")
        for s in range(3):                                         # the term changed some association
            plain = ByteTrackRef(XYWH)
            differs += sum(plain.update(d).tobytes() != got[s][k].tobytes() for k, (d, _) in enumerate(streams[s]))
        eng.close()
    assert differs > 0


def test_perturbed_streams_equal_reference():
    streams = [pose_stream(10 + s, 120) for s in range(3)]
    eng = _engine(POSE, 3)
    got = _run_engine(eng, streams, 32)
    for s, ref in enumerate(_check(streams, got, what="perturbed")):
        _assert_table(eng, s, ref, f"perturbed stream {s}")
    eng.close()


def test_group_sizes_give_identical_rows_and_poses():
    streams = [pose_stream(7, 64)]
    res, poses = [], []
    for g in (1, 7, 32):
        eng = _engine(POSE, 1)
        res.append(_run_engine(eng, streams, g))
        poses.append(eng.keypoints(0)[0].tobytes())
        eng.close()
    for k in range(64):
        assert res[0][0][k].tobytes() == res[1][0][k].tobytes() == res[2][0][k].tobytes(), f"frame {k}"
    assert poses[0] == poses[1] == poses[2]
    _check(streams, res[0], what="group 1")


def test_eight_streams_equal_reference():
    streams = [pose_stream(20 + s, 48) if s % 2 else _crossing(20 + s, 48) for s in range(8)]
    eng = _engine(POSE, 8)
    got = _run_engine(eng, streams, 7)
    for s, ref in enumerate(_check(streams, got, what="S = 8")):
        _assert_table(eng, s, ref, f"S = 8 stream {s}")
    eng.close()


def test_pose_with_camera_motion_equals_reference():
    streams = [pose_stream(30 + s, 96) for s in range(3)]
    w = _warps(5, 96, 3)
    eng = _engine(POSE, 3)
    got = _run_engine(eng, streams, 32, w)
    for s, ref in enumerate(_check(streams, got, w, "gmc")):
        _assert_table(eng, s, ref, f"gmc stream {s}")
    eng.close()


def _full_frames(n_frames, seed=0):
    """128 rows a frame on a 16 x 8 grid, every score high: 128 tracks x 128 rows = 16 384 cost entries (the spill path)."""
    rng = np.random.default_rng(900 + seed)
    sks = [skeleton(rng) for _ in range(128)]
    gx, gy = np.meshgrid(np.arange(16) * 78.0 + 5, np.arange(8) * 88.0 + 5)
    x0, y0 = gx.reshape(-1), gy.reshape(-1)
    out = []
    for f in range(n_frames):
        d, kp = np.zeros((128, 6), np.float32), np.zeros((128, K, 3), np.float32)
        for i in range(128):
            x, y = x0[i] + 3.0 * f + rng.normal(0, 1.5), y0[i] + rng.normal(0, 1.5)
            d[i] = [x, y, x + 90, y + 110, rng.uniform(0.5, 0.95), 0]
            kp[i] = place(sks[i], d[i, :4].astype(np.float64), rng)
        p = rng.permutation(128)
        out.append((d[p], kp[p]))
    return out


def test_full_frames_and_the_spilled_cost_matrix():
    streams = [_full_frames(6)]
    eng = _engine(POSE, 1)
    got = _run_engine(eng, streams, 6)
    assert len(got[0][1]) == 128 and 128 * 128 > 2048
    (ref,) = _check(streams, got, what="128 rows")
    _assert_table(eng, 0, ref, "128 rows")
    eng.close()


def test_capacity_reset_and_refusals():
    from strongsort_yolo_amd import lib
    from strongsort_yolo_amd.engine import ByteTrackEngine, TrackerEngine
    # births beyond max_tracks are dropped (as the reference drops them) and reported
    small = ByteTrackConfig(kalman="xywh", with_pose=True, max_tracks=6)
    st = pose_stream(60, 12)
    eng = _engine(small, 1)
    with pytest.raises(lib.SSError) as ei:
        _run_engine(eng, [st], 12)
    assert ei.value.code == lib.SS_ERR_CAPACITY
    ref = BotSortPoseRef(small)
    for d, kp in st:
        ref.update(d, kp)
    assert ref.capacity_error
    _assert_table(eng, 0, ref, "capacity")
    eng.close()
    # reset of one stream in mid-stream
    streams = [pose_stream(50 + s, 60) for s in range(2)]
    eng = _engine(POSE, 2)
    a = _run_engine(eng, [s[:30] for s in streams], 16)
    eng.reset(1)
    assert eng.keypoints(1)[0].shape == (0, K, 2) and eng.keypoints(0)[0].shape[0] > 0
    b = _run_engine(eng, [s[30:] for s in streams], 16)
    ref0 = _check([streams[0]], [a[0] + b[0]], what="kept")[0]
    ref1 = _check([streams[1][30:]], [b[1]], what="after reset")[0]
    _assert_table(eng, 0, ref0, "kept stream")
    _assert_table(eng, 1, ref1, "reset stream")
    # refusals: SS_ERR_INVALID, nothing launched
    dets = torch.zeros(1, 2, 128, 6, device=DEV)
    n = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    feats = torch.zeros(1, 2, 128, 512, device=DEV)
    kp = torch.zeros(1, 2, 128, K, 3, device=DEV)
    sg = (lib.C.c_double * K)(*POSE.kpt_sigmas)

    def invalid(rc):
        with pytest.raises(lib.SSError) as ei:
            eng._ck(rc)
        assert ei.value.code == lib.SS_ERR_INVALID

    with pytest.raises(ValueError):                               # the keypoint term needs keypoints
        eng.update_group(1, dets, n, None, None, eng.out[None], eng.nout[None])
    invalid(eng.L.ss_byte_update_group(eng.ctx, 1, dets.data_ptr(), n.data_ptr(), eng.out.data_ptr(), eng.nout.data_ptr()))
    invalid(eng.L.ss_byte_update(eng.ctx, dets.data_ptr(), n.data_ptr(), eng.out.data_ptr(), eng.nout.data_ptr()))
    invalid(eng.L.ss_byte_update_group_feats(eng.ctx, 1, dets.data_ptr(), n.data_ptr(), feats.data_ptr(), eng.out.data_ptr(), eng.nout.data_ptr()))
    invalid(eng.L.ss_byte_set_reid(eng.ctx, 1, 0.5, 0.25, 0.9))
    invalid(eng.L.ss_byte_set_pose(eng.ctx, 1, 0, sg, 0.5, 0.25, 0.5, 3))
    invalid(eng.L.ss_byte_set_pose(eng.ctx, 1, 33, sg, 0.5, 0.25, 0.5, 3))
    invalid(eng.L.ss_byte_update_group_kpts(eng.ctx, 1, dets.data_ptr(), n.data_ptr(), kp.data_ptr(), 3 * K - 1, 0, None, eng.out.data_ptr(), eng.nout.data_ptr()))
    invalid(eng.L.ss_byte_update_group_kpts(eng.ctx, 33, dets.data_ptr(), n.data_ptr(), kp.data_ptr(), 3 * K, 0, None, eng.out.data_ptr(), eng.nout.data_ptr()))
    invalid(eng.L.ss_byte_update_group_kpts(eng.ctx, 1, dets.data_ptr(), n.data_ptr(), None, 3 * K, 0, None, eng.out.data_ptr(), eng.nout.data_ptr()))
    _assert_table(eng, 0, ref0, "kept stream, after the refused calls")          # none of them touched the state
    eng.close()
    x = ByteTrackEngine(ByteTrackConfig(kalman="xyah"), 1, 0)     # no keypoint term on ByteTrack
    with pytest.raises(lib.SSError) as ei:
        x._ck(x.L.ss_byte_set_pose(x.ctx, 1, K, sg, 0.5, 0.25, 0.5, 3))
    assert ei.value.code == lib.SS_ERR_INVALID
    with pytest.raises(RuntimeError):
        x.keypoints(0)
    with pytest.raises(lib.SSError):                              # never switched on
        x._ck(x.L.ss_byte_get_keypoints(x.ctx, 0, 256, None, None))
    x.close()
    r = ByteTrackEngine(ByteTrackConfig(kalman="xywh", with_reid=True), 1, 0)    # ... nor beside ReID
    with pytest.raises(lib.SSError) as ei:
        r._ck(r.L.ss_byte_set_pose(r.ctx, 1, K, sg, 0.5, 0.25, 0.5, 3))
    assert ei.value.code == lib.SS_ERR_INVALID
    r.close()
    base = TrackerEngine(n_streams=1)                             # no BYTE state
    with pytest.raises(lib.SSError) as ei:
        base._ck(base.L.ss_byte_set_pose(base.ctx, 1, K, sg, 0.5, 0.25, 0.5, 3))
    assert ei.value.code == lib.SS_ERR_INVALID
    base.close()


def test_graph_capture_equals_plain_launches():
    streams = [pose_stream(80 + s, 32) for s in range(2)]
    G, S = 8, 2
    eng = _engine(POSE, S)
    plain = _run_engine(eng, streams, G)
    eng.reset(-1)
    d, n, kp = torch.zeros(G, S, 128, 6, device=DEV), torch.zeros(G, S, dtype=torch.int32, device=DEV), torch.zeros(G, S, 128, K, 3, device=DEV)
    out, nout = torch.zeros(G, S, 256, 8, device=DEV), torch.zeros(G, S, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        eng.use_current_stream()
        eng.update_group(G, d, n, None, None, out, nout, kpts=kp)                 # warm-up on empty frames
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            eng.use_current_stream()
            eng.update_group(G, d, n, None, None, out, nout, kpts=kp)
    torch.cuda.synchronize(DEV)
    eng.use_current_stream()
    eng.reset(-1)
    for f0 in range(0, 32, G):
        hd, hn, hk = _pack(streams, f0, G)
        d.copy_(torch.from_numpy(hd)); n.copy_(torch.from_numpy(hn)); kp.copy_(torch.from_numpy(hk))
        torch.cuda.synchronize(DEV)
        graph.replay()
        torch.cuda.synchronize(DEV)
        eng.check_errors()
        ho, hno = out.cpu().numpy(), nout.cpu().numpy()
        for f in range(G):
            for s in range(S):
                _assert_rows(ho[f, s, :hno[f, s]], plain[s][f0 + f], f"replayed group at {f0}, frame {f} stream {s}")
    del graph
    eng.close()


def test_all_invisible_equals_the_plain_engine():
    streams = [pose_stream(90 + s, 64) for s in range(2)]
    hidden = [[(d, np.concatenate([kp[..., :2], np.zeros_like(kp[..., 2:])], -1)) for d, kp in st] for st in streams]
    eng = _engine(POSE, 2)
    got = _run_engine(eng, hidden, 32)
    eng.close()
    base = _engine(XYWH, 2)
    exp = _run_engine(base, streams, 32, kpts=False)
    base.close()
    for s in range(2):
        for k in range(64):
            _assert_rows(got[s][k], exp[s][k], f"stream {s} frame {k}")


def test_bytetracker_with_keypoints():
    from strongsort_yolo_amd.tracker import BYTETracker
    st = _crossing(70, 50)
    trk, ref = BYTETracker(POSE), BotSortPoseRef(POSE)
    for k, (d, kp) in enumerate(st):
        _assert_rows(trk.update(d, keypoints=kp), ref.update(d, kp), f"frame {k}")
    with pytest.raises(ValueError):
        trk.update(st[0][0])
    trk.close()
    plain = BYTETracker(XYWH)
    with pytest.raises(ValueError):
        plain.update(st[0][0], keypoints=st[0][1])
    plain.close()


# ---- YOLO("yolo11n-pose.pt", tracker_type="botsort", with_pose=True) end to end ------------------------------------------------
H_, W_, NF_ = 480, 640, 24


def _pose_model():
    """Synthetic detector heads of a pose model: the rows of a seeded stream, every anchor of an identity carrying that identity's
    skeleton on its own box (network-input pixels)."""
    from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry
    from strongsort_yolo_amd.synth import synth_prediction
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO("yolo11n-pose.pt", random_init_ok=True, tracker_type="botsort", with_pose=True)
    model.overrides.update(conf=0.3, iou=0.4, agnostic_nms=False, max_det=1000)
    model._pipe_kw.update(det_source="synthetic", reid_batch=32)
    g = letterbox_geometry(H_, W_)
    gs = scale_geometry(g, H_, W_)
    A = sum((g.out_h // s) * (g.out_w // s) for s in (8, 16, 32))
    st, rng = make_stream(46, W_, H_, 9), np.random.default_rng(46)
    sks = [skeleton(np.random.default_rng(460 + i)) for i in range(9)]
    frames, preds = [], []
    for k in range(NF_):
        fr = st.next_frame()
        d = fr.dets.copy()
        d[:, 4] = np.where(rng.random(len(d)) < 0.3, rng.uniform(0.12, 0.24, len(d)), d[:, 4]).astype(np.float32)
        pred, agt = synth_prediction(d, A, 1, gs[0], (gs[1], gs[2]), rng)
        kp = np.stack([rng.uniform(0, 640, (A, K)), rng.uniform(0, 480, (A, K)), rng.uniform(0, 1, (A, K))], 2).astype(np.float32)
        for a in np.nonzero(agt >= 0)[0]:
            cx, cy, w, h = pred[:4, a]
            kp[a] = place(sks[int(fr.gt_ids[agt[a]])], np.array([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], np.float64), rng, jitter=0.7)
        frames.append(st.frame_pixels(k).copy())
        preds.append(np.concatenate([pred, kp.reshape(A, 3 * K).T]))
    dp = torch.from_numpy(np.stack(preds)).to(DEV)

    def fill(b, v, k):
        b.pred_in[v].copy_(dp[k])

    model._fill = fill
    return model, frames


def test_yolo_track_and_track_stream_equal_reference():
    model, frames = _pose_model()
    ref, plain, per_frame, differs = BotSortPoseRef(POSE), ByteTrackRef(XYWH), [], 0
    for k in range(NF_):
        res = model.track(frames[k], verbose=False, device=0, persist=True, tracker="botsort.yaml")
        pipe = model._pipe
        assert pipe.byte is not None and pipe.byte.pose and pipe.reid is None and pipe.nk == 3 * K
        full = pipe.detections()[0]
        rows = full[:, :6]
        kp = original_pixels(full[:, 6:6 + 3 * K].reshape(-1, K, 3), pipe.gain, pipe.pad_x, pipe.pad_y)
        e = ref.update(rows, kp)
        differs += plain.update(rows).tobytes() != e.tobytes()
        r = res[0]
        assert len(r.boxes) == len(e), f"frame {k}"
        if len(e):
            assert np.array_equal(r.boxes.id.numpy(), e[:, 4]) and np.array_equal(r.boxes.xyxy.numpy(), e[:, :4]), f"frame {k}"
            # Results.keypoints still follow det_idx, and they are the floats the tracker saw
            assert r.keypoints.data.numpy().tobytes() == np.ascontiguousarray(kp[e[:, 7].astype(int)]).tobytes(), f"frame {k}: keypoints"
        per_frame.append(r)
    print("frames whose rows differ from plain BoT-SORT:", differs)
    for batch in (32, 7):                                          # a full group; a partial last group (24 = 3 x 7 + 3)
        model._frame_index = 0
        got = list(model.track_stream(frames, batch=batch))
        assert len(got) == NF_ and model._stream_pipe.byte.pose
        for k, (a, b) in enumerate(zip(got, per_frame)):
            a = a[0]
            assert len(a.boxes) == len(b.boxes), f"track_stream batch {batch} frame {k}"
            if len(b.boxes):
                assert torch.equal(a.boxes.id, b.boxes.id) and torch.equal(a.boxes.xyxy, b.boxes.xyxy) and torch.equal(a.boxes.conf, b.boxes.conf)
                assert torch.equal(a.keypoints.data, b.keypoints.data), f"track_stream batch {batch} frame {k}: keypoints"
    model.close()


def test_pipeline_refuses_a_detector_without_keypoints():
    from strongsort_yolo_amd.pipeline import FramePipeline
    with pytest.raises(ValueError):
        FramePipeline("yolov8n", 1, (H_, W_), tracker="botsort", with_pose=True, graph="none")
