"""Deep OC-SORT on the MI355X (csrc/ss_deepoc.hip) against its CPU reference (tests/deepocsort_ref.py), bit for bit: rows every
frame, the track table and the tracks' features at the end."""
import functools

import numpy as np
import pytest
import torch

from strongsort_yolo_amd.config import DeepOCSortConfig, OCSortConfig
from strongsort_yolo_amd.synth import make_stream
from tests import byte_crowd
from tests.deepocsort_ref import DeepOCSortRef
from tests.deepocsort_scenes import SCENES, deep_stream
from tests.ocsort_scenes import EDGE_SIZES, edge_pair
from tests.test_gpu_cmc import _scene

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TABLE = ("track_id", "age", "time_since_update", "hits", "hit_streak", "frozen", "x", "P", "last_obs", "velocity")
NO_WARP = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0, 0.0])
# the three streams of the main test: (seed, identities): two crowded ones (every first association an LSAP) and a sparse one
# (most of its first associations take the shortcut)
STREAMS = ((0, 28), (1, 28), (2, 6))


def _warp_rows(warps, n_frames):
    """per frame a warp [8] or None -> [F,8] with `no warp` rows"""
    if warps is None:
        return None
    return np.stack([NO_WARP if w is None else np.asarray(w, np.float64) for w in warps[:n_frames]])


def _run_engine(eng, streams, group, check=True):
    """streams: per stream (frames, feats, warps or None), equal lengths -> per stream a list of rows, through update_group calls
    of `group` frames; the group's warps are installed before each call when any stream has some."""
    S, F = len(streams), len(streams[0][0])
    wr = [_warp_rows(w, F) for _, _, w in streams]
    use_w = any(w is not None for w in wr)
    out_all = [[] for _ in range(S)]
    out = torch.zeros(32, S, 256, 8, device=DEV)
    nout = torch.zeros(32, S, dtype=torch.int32, device=DEV)
    for f0 in range(0, F, group):
        n = min(group, F - f0)
        hd, hn = np.zeros((n, S, 128, 6), np.float32), np.zeros((n, S), np.int32)
        hf, hw = np.zeros((n, S, 128, 512), np.float32), np.tile(NO_WARP, (n, S, 1))
        for f in range(n):
            for s in range(S):
                d, ft = streams[s][0][f0 + f], streams[s][1][f0 + f]
                m = min(len(d), 128)
                hd[f, s, :m], hn[f, s], hf[f, s, :m] = d[:m], len(d), ft[:m]
                if wr[s] is not None:
                    hw[f, s] = wr[s][f0 + f]
        if use_w:
            eng.set_cmc(torch.from_numpy(hw).to(DEV))
        eng.update_group(n, torch.from_numpy(hd).to(DEV), torch.from_numpy(hn).to(DEV), torch.from_numpy(hf).to(DEV), None, out[:n], nout[:n])
        if check:
            eng.check_errors()
        ho, hno = out[:n].cpu().numpy(), nout[:n].cpu().numpy()
        for f in range(n):
            for s in range(S):
                out_all[s].append(ho[f, s, :hno[f, s]].copy())
    return out_all


def _assert_rows(got, ref, what):
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), f"{what}:\n{got}\n!=\n{ref}"


def _assert_table(eng, s, ref, what, features=True):
    t, r = eng.tracks(s), ref.tracks()
    assert (t["n_tracks"], t["next_id"], t["frame_count"]) == (r["n_tracks"], r["next_id"], r["frame_count"]), what
    for k in TABLE:
        assert t[k].shape == r[k].shape and t[k].tobytes() == r[k].tobytes(), f"{what}: {k}\n{t[k]}\n!=\n{r[k]}"
    if features:
        a, b = eng.features(s), ref.features()
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: features"


def _replay(cfg, stream):
    ref = DeepOCSortRef(cfg)
    frames, feats, warps = stream
    return [ref.update(d, f, None if warps is None else warps[k]) for k, (d, f) in enumerate(zip(frames, feats))], ref


@functools.lru_cache(maxsize=None)
def _stream_reference(cfg, seed, n_frames, n_ids=28, camera=True):
    """One reference run per (configuration, stream), shared by the tests and never changed: (stream, rows per frame, reference)."""
    st = deep_stream(seed, n_frames, n_ids=n_ids, camera=camera)
    return (st,) + tuple(_replay(cfg, st))


def _check(eng, streams, refs, group, what, check=True):
    got = _run_engine(eng, streams, group, check)
    for s, (rows, ref) in enumerate(refs):
        for k in range(len(rows)):
            _assert_rows(got[s][k], rows[k], f"{what} stream {s} frame {k}")
        _assert_table(eng, s, ref, f"{what} stream {s}")
    return got


def test_group_rows_tables_and_features_equal_reference():
    from strongsort_yolo_amd.engine import DeepOCSortEngine
    cfg = DeepOCSortConfig()
    runs = [_stream_reference(cfg, seed, 96, n) for seed, n in STREAMS]
    eng = DeepOCSortEngine(cfg, 3, 0)
    _check(eng, [r[0] for r in runs], [r[1:] for r in runs], 32, "streams")
    eng.close()


def test_streams_reach_every_branch():
    """From the reference's own counters over the three streams of the test above."""
    cfg, tot = DeepOCSortConfig(), {}
    for seed, n in STREAMS:
        st, _, ref = _stream_reference(cfg, seed, 96, n)
        assert st[2][31, 6] >= 0 and st[2][32, 6] >= 0                 # a warp on both sides of the group boundary
        for k, v in ref.counters.items():
            tot[k] = tot.get(k, 0) + v
    print(tot)
    for k in ("lsap_emb", "shortcut", "aw_rows", "aw_cols", "oru_tracks", "ocr", "warp_frozen"):
        assert tot[k] > 0, k


def test_group_sizes_give_identical_rows():
    """the identities 0..3 are unseen on frames 27..36 and frames 31 and 32 carry warps: a gap and a warp across every group size's
    boundaries"""
    from strongsort_yolo_amd.engine import DeepOCSortEngine
    cfg = DeepOCSortConfig()
    runs = [_stream_reference(cfg, 5 + s, 64) for s in range(2)]
    assert all(r[2].counters["oru_tracks"] > 0 and r[2].counters["warp_frozen"] > 0 for r in runs)
    for g in (1, 7, 32):
        eng = DeepOCSortEngine(cfg, 2, 0)
        _check(eng, [r[0] for r in runs], [r[1:] for r in runs], g, f"group {g}")
        eng.close()


def _with_features(frames, seed):
    """seeded features for rows without identities: a common part plus noise (similarities about 0.6 between any two rows)"""
    rng = np.random.default_rng(33000 + seed)
    common = rng.standard_normal(512)
    return [(common + 0.8 * rng.standard_normal((len(d), 512))).astype(np.float32) for d in frames]


# 2049 = 3 x 683 has no factorisation within 128 rows x 256 tracks: 2050 = 41 x 50 is the smallest spilled matrix the table can hold
SPILL_EDGE = ((41, 50), (50, 41))


@pytest.mark.parametrize("n_tracks,n_rows", EDGE_SIZES + SPILL_EDGE)
def test_edge_sizes_equal_reference(n_tracks, n_rows):
    """the first association is exactly n_rows x n_tracks: 2048 entries (the last LDS-resident size), 2050 (the first spilled size
    that exists) and 2112, 64 and 65 columns in both orientations, 128 x 128"""
    from strongsort_yolo_amd.engine import DeepOCSortEngine
    cfg = DeepOCSortConfig()
    frames = edge_pair(n_tracks, n_rows)
    st = (frames, _with_features(frames, n_tracks * 131 + n_rows), None)
    rows, ref = _replay(cfg, st)
    assert ref.counters["lsap_emb"] == 1 and ref.counters["shortcut"] == 0 and ref.last_E.shape == (n_rows, n_tracks)
    assert ref.counters["aw_cols"] > 0                            # the twice-claimed track's column, at least
    eng = DeepOCSortEngine(cfg, 1, 0)
    _check(eng, [st], [(rows, ref)], 2, f"edge pair {n_tracks} x {n_rows}")
    eng.close()


def test_more_rows_than_a_frame_holds_is_flagged():
    from strongsort_yolo_amd import lib
    from strongsort_yolo_amd.engine import DeepOCSortEngine
    cfg = DeepOCSortConfig()
    d = byte_crowd._rows(byte_crowd._lattice(16, 9, 70.0, 50.0), 44.0, 30.0, np.full(144, 0.8))
    frames = [d, d]
    st = (frames, _with_features(frames, 7), None)
    rows, ref = _replay(cfg, st)
    assert ref.capacity_error
    eng = DeepOCSortEngine(cfg, 1, 0)
    got = _run_engine(eng, [st], 2, check=False)
    for k in range(2):
        _assert_rows(got[0][k], rows[k], f"first 128 rows, frame {k}")
    with pytest.raises(lib.SSError) as ei:
        eng.check_errors()
    assert ei.value.code == lib.SS_ERR_CAPACITY
    _assert_table(eng, 0, ref, "144 rows")
    eng.close()


def test_three_crowds_overflow_is_reported_and_reset_recovers():
    """the over-full 256-track crowd of tests/byte_crowd.py, with its features: 128 x 256 similarities, the spilled matrix"""
    from strongsort_yolo_amd import lib
    from strongsort_yolo_amd.engine import DeepOCSortEngine
    cfg = DeepOCSortConfig()
    frames, ids = byte_crowd.three_crowds(0, ids=True)
    st = (frames, byte_crowd.features(0, frames, ids), None)
    rows, ref = _replay(cfg, st)
    assert ref.capacity_error and ref.counters["lsap_emb"] >= 1
    eng = DeepOCSortEngine(cfg, 1, 0)
    got = _run_engine(eng, [st], 32, check=False)
    for k in range(len(frames)):
        _assert_rows(got[0][k], rows[k], f"three_crowds frame {k}")
    with pytest.raises(lib.SSError) as ei:
        eng.check_errors()
    assert ei.value.code == lib.SS_ERR_CAPACITY
    assert eng.tracks(0)["n_tracks"] <= 256
    _assert_table(eng, 0, ref, "three_crowds")
    eng.reset()
    eng.check_errors()
    assert eng.tracks(0)["n_tracks"] == 0
    got = _run_engine(eng, [(frames[:2], st[1][:2], None)], 2)
    for k in range(2):
        _assert_rows(got[0][k], rows[k], f"after reset, frame {k}")
    eng.close()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_hand_built_scenes_on_device(name):
    from strongsort_yolo_amd.engine import DeepOCSortEngine
    frames, feats, warps, cfg, check = SCENES[name]()
    st = (frames, feats, warps)
    rows, ref = _replay(cfg, st)
    check(rows, ref)
    eng = DeepOCSortEngine(cfg, 1, 0)
    _check(eng, [st], [(rows, ref)], 1, name)
    eng.close()


def test_tracker_class_takes_features_and_resets():
    from strongsort_yolo_amd.tracker import DeepOCSORTTracker
    frames, feats, _, cfg, _ = SCENES["appearance_keeps_ids_at_a_crossing"]()
    trk = DeepOCSORTTracker(cfg)
    for rnd in range(2):
        ref = DeepOCSortRef(cfg)
        for k, (d, f) in enumerate(zip(frames, feats)):
            _assert_rows(trk.update(d, features=f), ref.update(d, f), f"round {rnd} frame {k}")
        _assert_table(trk.eng, 0, ref, f"round {rnd}")
        trk.reset()
    with pytest.raises(ValueError):                               # neither a network nor features
        trk.update(frames[0])
    trk.close()


def test_without_appearance_and_warps_it_is_ocsort():
    """appearance=False without warps: k_deepoc_group's rows and table equal k_ocsort_group's on the same input"""
    from strongsort_yolo_amd.engine import DeepOCSortEngine, OCSortEngine
    frames, feats, _ = deep_stream(4, 64, camera=False)
    a, b = DeepOCSortEngine(DeepOCSortConfig(appearance=False), 1, 0), OCSortEngine(OCSortConfig(), 1, 0)
    got = _run_engine(a, [(frames, feats, None)], 32)
    out, nout = torch.zeros(32, 1, 256, 8, device=DEV), torch.zeros(32, 1, dtype=torch.int32, device=DEV)
    for f0 in (0, 32):
        hd, hn = np.zeros((32, 1, 128, 6), np.float32), np.zeros((32, 1), np.int32)
        for f in range(32):
            d = frames[f0 + f]
            hd[f, 0, :len(d)], hn[f, 0] = d, len(d)
        b.update_group(32, torch.from_numpy(hd).to(DEV), torch.from_numpy(hn).to(DEV), None, None, out, nout)
        ho, hno = out.cpu().numpy(), nout.cpu().numpy()
        for f in range(32):
            _assert_rows(got[0][f0 + f], ho[f, 0, :hno[f, 0]], f"frame {f0 + f}")
    ta, tb = a.tracks(0), b.tracks(0)
    assert ta["n_tracks"] == tb["n_tracks"] > 0
    for k in TABLE:
        assert ta[k].tobytes() == tb[k].tobytes(), k
    assert not a.features(0).any()
    a.close(); b.close()


@pytest.mark.parametrize("delta_t", [1, 8])
def test_delta_t_edges_equal_reference(delta_t):
    from strongsort_yolo_amd.engine import DeepOCSortEngine
    cfg = DeepOCSortConfig(delta_t=delta_t)
    st, rows, ref = _stream_reference(cfg, 3, 48)
    assert ref.counters["warp_frozen"] > 0
    eng = DeepOCSortEngine(cfg, 1, 0)
    _check(eng, [st], [(rows, ref)], 32, f"delta_t {delta_t}")
    eng.close()


# ---- YOLO(tracker_type="deep_ocsort") end to end (the synthetic-prediction set-up of tests/test_gpu_ocsort.py) --------------------
H_, W_, NF_ = 480, 640, 24
CLUTTER_ = 24                                                     # tests/test_gpu_ocsort.py: unmatched births live max_age frames


def _model(camera_motion):
    from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry
    from strongsort_yolo_amd.synth import synth_prediction
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="deep_ocsort", camera_motion=camera_motion)
    model.overrides.update(conf=0.3, iou=0.4, agnostic_nms=False, max_det=1000)
    model._pipe_kw.update(det_source="synthetic", reid_batch=32)
    g = letterbox_geometry(H_, W_)
    gs = scale_geometry(g, H_, W_)
    A = sum((g.out_h // s) * (g.out_w // s) for s in (8, 16, 32))
    canvas = _scene(H_, W_, 6)                                     # a panning camera over one textured canvas: ECC has something to align
    st, rng = make_stream(47, W_, H_, 9), np.random.default_rng(47)
    frames, preds = [], []
    for k in range(NF_):
        o = 4 * k if k < 12 else 48 + 25 * (k - 11) if k < 14 else 98
        d = st.next_frame().dets.copy()
        d[:, [0, 2]] = np.clip(d[:, [0, 2]] - o, 0, W_ - 1)           # the scene moves left by the pan
        d = d[d[:, 2] - d[:, 0] > 4]
        pred, _ = synth_prediction(d, A, 80, gs[0], (gs[1], gs[2]), rng, clutter=CLUTTER_)
        frames.append(np.ascontiguousarray(canvas[100:100 + H_, o:o + W_])); preds.append(pred)
    dp = torch.from_numpy(np.stack(preds)).to(DEV)
    model._fill = lambda b, v, k: b.pred_in[v].copy_(dp[k])
    return model, frames


@pytest.mark.parametrize("camera_motion", [False, True])
def test_yolo_deep_ocsort_track_and_stream_equal_reference(camera_motion):
    """track() frame by frame equals the reference replayed on the pipeline's own rows, OSNet features and warps; track_stream
    equals track()."""
    model, frames = _model(camera_motion)
    ref, per_frame, shown, warped = DeepOCSortRef(DeepOCSortConfig()), [], 0, 0
    for k in range(NF_):
        res = model.track(frames[k], verbose=False, device=0, persist=True, tracker="deep_ocsort.yaml")
        pipe = model._pipe
        assert pipe.reid is not None and pipe.byte is pipe.trk and pipe.byte.reid and pipe.dcfg.conf == 0.1 and pipe.max_det == 32
        rows = pipe.detections()[0][:, :6]
        feats = pipe.feats_in[0, :len(rows)].cpu().numpy()
        warp = pipe.warps.reshape(-1, 8)[0].cpu().numpy() if camera_motion else None
        warped += int(warp is not None and warp[6] >= 0)
        exp = ref.update(rows, feats, warp)
        r = res[0]
        assert len(r.boxes) == len(exp), f"frame {k}"
        shown += len(exp)
        if len(exp):
            assert np.array_equal(r.boxes.id.numpy(), exp[:, 4]) and np.array_equal(r.boxes.xyxy.numpy(), exp[:, :4]), f"frame {k}"
            assert np.array_equal(r.boxes.cls.numpy(), exp[:, 5]) and np.array_equal(r.boxes.conf.numpy(), exp[:, 6])
        per_frame.append(r)
    assert shown > NF_ and not ref.capacity_error and ref.counters["ema"] > 4 * NF_
    assert warped >= 20 if camera_motion else warped == 0
    a, b = pipe.trk.features(0), ref.features()
    assert a.shape == b.shape and a.tobytes() == b.tobytes()
    model._frame_index = 0
    got = list(model.track_stream(frames, batch=32))
    assert model._stream_pipe.reid is not None and len(got) == NF_
    for k, (a, b) in enumerate(zip(got, per_frame)):
        a = a[0]
        assert len(a.boxes) == len(b.boxes), f"frame {k}"
        if len(b.boxes):
            assert torch.equal(a.boxes.id, b.boxes.id) and torch.equal(a.boxes.xyxy, b.boxes.xyxy) and torch.equal(a.boxes.conf, b.boxes.conf)
    model.close()
