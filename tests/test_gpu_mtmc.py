"""Multi-camera linking on the device (csrc/ss_mtmc.hip, docs/MTMC.md) against tests/mtmc_ref.py through the C ABI: the track bank bit for
bit, behind two trackers and behind both YOLO paths; the distances on exact and on random operands; the clustering's partition and
merge record bit for bit; and the whole chain from trackers to the rewritten labels files."""
import os

import numpy as np
import pytest
import torch

from strongsort_yolo_amd import cli, lib, mtmc
from strongsort_yolo_amd.engine import DeepOCSortEngine, TrackerEngine
from strongsort_yolo_amd.synth import make_stream
from tests import mtmc_ref as R
from tests.test_mtmc_cpu import SCENE_IDS, partition, scene_streams

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MAXT, MAXD = lib.MAX_TRACKS, lib.MAX_DETS


def _same_table(got, want, what):
    assert set(got) == set(want) == set(mtmc.KEYS)
    for k in mtmc.KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, f"{what}: {k} {got[k].shape} vs {want[k].shape}"
        assert got[k].tobytes() == want[k].tobytes(), f"{what}: {k} differs in {int((got[k] != want[k]).sum())} places"


def _device_group(rows, feats, S):
    """rows[f][s]: an [n, 8] array or None (sat out); feats[f][s]: [128, 512] -> the device tensors of one group."""
    F = len(rows)
    r, n, ft = np.zeros((F, S, MAXT, 8), np.float32), np.zeros((F, S), np.int32), np.zeros((F, S, MAXD, 512), np.float32)
    for f in range(F):
        for s in range(S):
            ft[f, s] = feats[f][s]
            if rows[f][s] is None:
                n[f, s] = -1
            else:
                n[f, s] = len(rows[f][s])
                r[f, s, :len(rows[f][s])] = rows[f][s]
    return tuple(torch.from_numpy(v).to(DEV) for v in (r, n, ft))


def _run_bank(bank, rows, feats, S, groups):
    at = 0
    for g in groups:
        d = _device_group(rows[at:at + g], feats[at:at + g], S)
        bank.update_group_device(*d, g)
        at += g
    assert at == len(rows)
    torch.cuda.synchronize()


def _ref_tables(rows, feats, S, max_ids):
    refs = [R.Bank(max_ids) for _ in range(S)]
    for f in range(len(rows)):
        for s in range(S):
            refs[s].update(rows[f][s], feats[f][s])
    return refs


def _random_frames(seed, F, S, n_ids=40, max_rows=24, sit_out=()):
    rng = np.random.default_rng(seed)
    rows, feats = [], []
    for f in range(F):
        rr, ff = [], []
        for s in range(S):
            ft = (rng.standard_normal((MAXD, 512)) * rng.uniform(0.1, 30)).astype(np.float32)
            ft[rng.integers(0, MAXD)] = 0.0                                        # an all-zero feature row
            n = int(rng.integers(0, max_rows + 1))
            r = np.zeros((n, 8), np.float32)
            r[:, 4] = rng.permutation(n_ids)[:n] + 1                               # an id at most once a frame and stream
            r[:, 5], r[:, 6] = rng.integers(0, 5, n), rng.uniform(0.3, 0.9, n)
            r[:, 7] = np.where(rng.random(n) < 0.2, -1, rng.permutation(MAXD)[:n])   # rows without a detection
            rr.append(None if (f, s) in sit_out else r)
            ff.append(ft)
        rows.append(rr)
        feats.append(ff)
    return rows, feats


# ---- 6. the bank, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, F, S, groups, sit_out", [
    ("one frame", 1, 1, [1], ()),
    ("33 frames as 32 + 1", 33, 1, [32, 1], ()),
    ("two streams, one sitting a frame out", 9, 2, [4, 5], ((2, 1), (3, 1), (6, 0))),
])
def test_bank_equals_the_restatement(name, F, S, groups, sit_out):
    eng = TrackerEngine(None, S, 0)
    bank = mtmc.TrackBank(eng, 64)
    rows, feats = _random_frames(len(name), F, S, sit_out=sit_out)
    if F == 1:
        rows[0][0] = rows[0][0][:1].copy() if len(rows[0][0]) else np.array([[0, 0, 1, 1, 1, 0, 0.5, 0]], np.float32)
        rows[0][0][0, 4], rows[0][0][0, 7] = 3, 5
        feats[0][0][5, 0] = 1.0
    _run_bank(bank, rows, feats, S, groups)
    eng.check_errors()
    refs = _ref_tables(rows, feats, S, 64)
    for s in range(S):
        assert len(refs[s].n) > 0
        _same_table(bank.table(s), refs[s].table(), f"{name}, stream {s}")
    # reset: one stream, then nothing is left and the frame counter starts again
    bank.reset(0)
    assert len(bank.table(0)["ids"]) == 0 and (S == 1 or len(bank.table(1)["ids"]) > 0)
    _run_bank(bank, rows[:1], feats[:1], S, [1])
    ref0 = _ref_tables(rows[:1], feats[:1], S, 64)[0]
    _same_table(bank.table(0), ref0.table(), f"{name}, after the reset")
    eng.close()


def test_bank_full_frame_and_single_frame_calls():
    rng = np.random.default_rng(7)
    eng = TrackerEngine(None, 1, 0)
    bank = mtmc.TrackBank(eng, 300)
    ft = rng.standard_normal((MAXD, 512)).astype(np.float32)
    r = np.zeros((MAXT, 8), np.float32)
    r[:, 4], r[:, 5], r[:, 7] = rng.permutation(MAXT) + 1, rng.integers(0, 3, MAXT), rng.integers(0, MAXD, MAXT)
    rows, feats = [[r], [r[::-1].copy()]], [[ft], [ft[::-1].copy()]]
    _run_bank(bank, rows, feats, 1, [2])
    t = bank.table(0)
    assert len(t["ids"]) == MAXT and (t["n"] == 2).all()
    _same_table(t, _ref_tables(rows, feats, 1, 300)[0].table(), "a frame with SS_MAX_TRACKS rows")
    # one group of 32 equals 32 single-frame calls, byte for byte
    rows, feats = _random_frames(11, 32, 1)
    bank.reset()
    _run_bank(bank, rows, feats, 1, [32])
    whole = bank.table(0)
    bank.reset()
    _run_bank(bank, rows, feats, 1, [1] * 32)
    _same_table(bank.table(0), whole, "32 single-frame calls")
    _same_table(whole, _ref_tables(rows, feats, 1, 300)[0].table(), "one group of 32")
    eng.close()


def test_bank_capacity_and_arguments():
    rng = np.random.default_rng(3)
    eng = TrackerEngine(None, 1, 0)
    bank = mtmc.TrackBank(eng, 16)
    ft = rng.standard_normal((MAXD, 512)).astype(np.float32)
    r = np.array([[0, 0, 1, 1, 16, 2, 0.5, 0], [0, 0, 1, 1, 17, 2, 0.5, 1], [0, 0, 1, 1, 2, 1, 0.5, 2]], np.float32)
    _run_bank(bank, [[r]], [[ft]], 1, [1])
    with pytest.raises(lib.SSError) as e:
        eng.check_errors()
    assert e.value.code == lib.SS_ERR_CAPACITY and "16" in str(e.value)
    with pytest.raises(lib.SSError):                                 # it stays set
        eng.check_errors()
    ref = _ref_tables([[r]], [[ft]], 1, 16)[0]
    assert ref.err
    _same_table(bank.table(0), ref.table(), "ids max_ids and max_ids + 1")
    assert bank.table(0)["ids"].tolist() == [2, 16]
    bank.reset()
    eng.check_errors()
    d = _device_group([[r]], [[ft]], 1)
    for bad in (lambda: eng.bank_update_group(0, *d), lambda: eng.bank_update_group(33, *d), lambda: eng.bank_update_group(1, d[0], d[1], None),
                lambda: eng.bank_get(1), lambda: eng.bank_create(0), lambda: eng.bank_create(eng.L.ss_bank_max_ids() + 1)):
        with pytest.raises(lib.SSError) as e:
            bad()
        assert e.value.code == lib.SS_ERR_INVALID
    bank.close()
    with pytest.raises(lib.SSError):
        eng.bank_get(0)
    eng.close()


# ---- 7. the bank behind a tracker ------------------------------------------------------------------------------------------------
def _tracker_groups(eng, trk, stream, n_frames, groups, bank):
    """The stream through trk in groups, the bank behind every call -> the downloaded rows and the features per frame."""
    S, at, rows, feats = 1, 0, [], []
    hw = torch.tensor([[stream.cfg.height, stream.cfg.width]], dtype=torch.int32, device=DEV)
    for g in groups:
        d, n, ft = np.zeros((g, S, MAXD, 6), np.float32), np.zeros((g, S), np.int32), np.zeros((g, S, MAXD, 512), np.float32)
        for f in range(g):
            fr = stream.next_frame()
            d[f, 0, :len(fr.dets)], n[f, 0], ft[f, 0, :len(fr.dets)] = fr.dets, len(fr.dets), fr.feats
        dd, dn, df = (torch.from_numpy(v).to(DEV) for v in (d, n, ft))
        out, nout = torch.zeros(g, S, MAXT, 8, device=DEV), torch.zeros(g, S, dtype=torch.int32, device=DEV)
        trk.update_group(g, dd, dn, df, hw, out, nout)
        bank.update_group_device(out, nout, df, g)
        torch.cuda.synchronize()
        o, c = out.cpu().numpy(), nout.cpu().numpy()
        for f in range(g):
            rows.append([o[f, 0, :c[f, 0]].copy()])
            feats.append([ft[f, 0]])
        at += g
    assert at == n_frames
    return rows, feats


@pytest.mark.parametrize("kind", ["strongsort", "deep_ocsort"])
def test_bank_behind_a_tracker(kind):
    eng = TrackerEngine(None, 1, 0)
    trk = eng if kind == "strongsort" else DeepOCSortEngine(None, 1, 0, engine=eng)
    bank = mtmc.TrackBank(trk, 256)
    rows, feats = _tracker_groups(eng, trk, make_stream(21, 640, 480, 10, p_vanish=0.05), 40, [32, 8], bank)
    eng.check_errors()
    allr = np.concatenate([r[0] for r in rows])
    assert len(allr) > 200 and (allr[:, 7] >= 0).any()
    if kind == "strongsort":
        assert (allr[:, 7] < 0).any()                               # StrongSORT's rows without a detection are in the scene
    ref = _ref_tables(rows, feats, 1, 256)[0]
    _same_table(bank.table(0), ref.table(), kind)
    if trk is not eng:
        trk.close()
    eng.close()


# ---- 8. the order of the bank launch and the release of a buffer set ------------------------------------------------------------
H_, W_, NF_ = 480, 640, 70


def _bank_model():
    from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry
    from strongsort_yolo_amd.synth import synth_prediction
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO("yolov8n.pt", random_init_ok=True, track_bank=True)
    model.overrides.update(conf=0.3, iou=0.4, agnostic_nms=False, max_det=1000)
    model._pipe_kw.update(det_source="synthetic", feat_source="by_anchor", reid_batch=32)
    g = letterbox_geometry(H_, W_)
    gs = scale_geometry(g, H_, W_)
    A = sum((g.out_h // s) * (g.out_w // s) for s in (8, 16, 32))
    st, rng = make_stream(52, W_, H_, 9), np.random.default_rng(52)
    frames, preds, agts, feats = [], [], [], []
    for k in range(NF_):
        fr = st.next_frame()
        pred, agt = synth_prediction(fr.dets, A, 80, gs[0], (gs[1], gs[2]), rng)
        f = np.zeros((128, 512), np.float32)
        f[:len(fr.feats)] = fr.feats * np.float32(1.0 + 0.01 * k)                 # every frame's features differ in length too
        frames.append(st.frame_pixels(k).copy()); preds.append(pred); agts.append(agt); feats.append(f)
    dp, da, df = (torch.from_numpy(np.stack(x)).to(DEV) for x in (preds, agts, feats))

    def fill(b, v, k):
        b.pred_in[v].copy_(dp[k]); b.anchor_gt[v].copy_(da[k]); b.gt_feats[v].copy_(df[k])

    model._fill = fill
    return model, frames


def test_track_stream_and_track_leave_the_same_bank():
    model, frames = _bank_model()
    for k in range(NF_):
        model.track(frames[k], verbose=False, device=0, persist=True)
    per_frame = model.track_bank()
    assert len(per_frame["ids"]) >= 9 and per_frame["n"].sum() > 400 and per_frame["last"].max() == NF_ - 1
    model._frame_index = 0
    got = list(model.track_stream(frames, batch=16))
    assert len(got) == NF_ and model._stream_pipe.bank is not None
    _same_table(model.track_bank(), per_frame, "track_stream(batch=16) against track()")
    model.close()


# ---- 9. the distances ------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 15, 16, 17, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def engine():
    eng = TrackerEngine(None, 1, 0)
    yield eng
    eng.close()


def _link(eng, desc, cam=None, first=None, last=None, n=None, thr=0.2, min_rows=1):
    T = len(desc)
    cam = np.arange(T) if cam is None else cam
    first = np.zeros(T) if first is None else first
    last = np.zeros(T) if last is None else last
    n = np.ones(T) if n is None else n
    gid, merges, D = eng.mtmc_link(desc, cam, first, last, n, thr, min_rows, want_dist=True)
    return gid, merges, D, (cam, first, last, n)


def _against_ref(eng, desc, what, **kw):
    """The device's partition and merge record equal the restatement's on the device's own distances, bit for bit."""
    gid, merges, D, meta = _link(eng, desc, **kw)
    want_gid, want_merges = R.cluster(D, *meta, kw.get("thr", 0.2), kw.get("min_rows", 1))
    assert gid.tolist() == want_gid.tolist(), what
    want = np.array(want_merges, np.float64).reshape(-1, 3)
    assert merges.shape == want.shape and merges.tobytes() == want.tobytes(), f"{what}: the merge record differs"
    assert np.array_equal(D, np.triu(D, 1))
    return gid, merges, D


@pytest.mark.parametrize("T", SIZES)
def test_distances_exact_and_random(engine, T):
    rng = np.random.default_rng(T)
    exact = rng.choice(np.array([0, 0, 0.125, -0.125, 0.25, -0.25, 0.5, -0.5], np.float32), (T, 512))
    _, _, D, _ = _link(engine, exact, thr=-1.0)
    want = R.dist_exact(exact)
    assert D.shape == (T, T) and np.array_equal(D.astype(np.float64), want), "exact operands"
    x = rng.standard_normal((T, 512))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    if T > 2:
        x[1] = x[0]                                                 # a distance near 0, where 1 - dot cancels
        x[2] = (x[0] + 0.05 * x[2]) / np.linalg.norm(x[0] + 0.05 * x[2])
    _, _, D, _ = _link(engine, x, thr=-1.0)
    err = float(np.abs(D.astype(np.float64) - R.dist64(x)).max())
    print(f"T = {T}: largest |D - f64| = {err:.3e}")
    assert err <= 1e-4


# ---- 10. the clustering ----------------------------------------------------------------------------------------------------------
def _clustered(seed, T, groups, sigma=0.02):
    """T unit descriptors: the first `groups` clusters of a few noisy sightings each, the rest unrelated."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, 512))
    at = 0
    for g in range(groups):
        k = min(int(rng.integers(2, 5)), T - at)
        if k < 2:
            break
        x[at + 1:at + k] = x[at] / np.linalg.norm(x[at]) + sigma * rng.standard_normal((k - 1, 512))
        at += k
    x = x[rng.permutation(T)]
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("T, groups", [(1, 0), (2, 1), (3, 1), (64, 12), (65, 12), (1025, 16)])
def test_clustering_equals_the_restatement(engine, T, groups):
    gid, merges, _ = _against_ref(engine, _clustered(T, T, groups), f"T = {T}", thr=0.5)
    assert len(merges) == T - len(set(gid.tolist()))
    if T == 1025:
        assert 16 <= len(merges) <= 48                               # a few dozen merges, one past the workgroup's width
    elif T > 1:
        assert len(merges) >= 1


def test_clustering_with_cameras_and_intervals(engine):
    rng = np.random.default_rng(77)
    T = 150
    x = _clustered(78, T, 30, sigma=0.03)
    cam = np.sort(rng.integers(0, 3, T))
    first = rng.integers(0, 200, T)
    last = first + rng.integers(0, 60, T)
    n = rng.integers(1, 9, T)
    for min_rows in (1, 4):                                          # min_rows above some tracklets' counts
        gid, merges, _ = _against_ref(engine, x, f"min_rows {min_rows}", cam=cam, first=first, last=last, n=n, thr=0.6, min_rows=min_rows)
        assert len(merges) > 10
        conf = R.conflicts(cam, first, last, n, min_rows)
        for members in partition(gid):
            assert not conf[np.ix_(members, members)].any()


def test_clustering_ties_conflicts_and_the_threshold(engine):
    e = np.eye(8, 512, dtype=np.float32)
    # duplicates: every distance is 0 or 1, the (d, a, b) rule alone orders the merges
    desc = e[[0, 1, 0, 2, 1, 0, 2, 1, 0]]
    gid, merges, D = _against_ref(engine, desc, "duplicates", thr=0.5)
    assert gid.tolist() == [1, 2, 1, 3, 2, 1, 3, 2, 1] and merges[:, :2].tolist()[:3] == [[0, 2], [0, 5], [0, 8]] and (merges[:, 2] == 0).all()
    # one camera, every interval overlapping: nothing may merge
    gid, merges, _ = _against_ref(engine, desc, "one camera", cam=np.zeros(9), first=np.arange(9), last=np.full(9, 20), thr=0.5)
    assert gid.tolist() == list(range(1, 10)) and len(merges) == 0
    # a chain: 0 and 2 share a camera and a time, 1 is near both; once 1 has joined 0, the pair (1, 2) that was allowed is not
    v = np.zeros((3, 512), np.float32)
    v[0, :2], v[1, :2], v[2, :2] = (1, 0), (0.9375, 0.25), (0.875, 0.25)
    gid, merges, D = _against_ref(engine, v, "chain", cam=np.array([0, 1, 0]), first=np.array([0, 0, 5]), last=np.array([10, 10, 15]), thr=0.5)
    assert gid.tolist() == [1, 1, 2] and merges.tolist() == [[0, 1, 0.0625]] and D[1, 2] == 0.1171875
    # a pair exactly at the threshold is left out; one step above it merges
    p = np.zeros((2, 512), np.float32)
    p[0, 0], p[1, 0], p[1, 1] = 1, 0.75, 0.5
    gid, merges, D = _against_ref(engine, p, "at thr", thr=0.25)
    assert D[0, 1] == 0.25 and gid.tolist() == [1, 2] and len(merges) == 0
    gid, merges, _ = _against_ref(engine, p, "above thr", thr=float(np.nextafter(0.25, 1)))
    assert gid.tolist() == [1, 1] and merges.tolist() == [[0, 1, 0.25]]


def test_clustering_capacity_determinism_and_scratch_reuse(engine):
    cap = int(engine.L.ss_mtmc_max_tracklets())
    assert cap >= 2048 and int(engine.L.ss_bank_max_ids()) >= 4096
    with pytest.raises(lib.SSError) as e:
        engine.mtmc_link(np.zeros((cap + 1, 512), np.float32), *(np.zeros(cap + 1),) * 4, 0.2)
    assert e.value.code == lib.SS_ERR_CAPACITY and str(cap + 1) in str(e.value)
    with pytest.raises(lib.SSError) as e:
        engine.mtmc_link(np.zeros((2, 512), np.float32), *(np.zeros(2),) * 4, float("nan"))
    assert e.value.code == lib.SS_ERR_INVALID
    small, large = _clustered(5, 40, 8), _clustered(6, 700, 40)
    fresh = TrackerEngine(None, 1, 0)
    alone = _link(fresh, small, thr=0.5)[:3]
    fresh.close()
    a = _link(engine, large, thr=0.5)[:3]
    b = _link(engine, large, thr=0.5)[:3]
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b)) and len(a[1]) > 30           # two identical calls: the same bytes
    after = _link(engine, small, thr=0.5)[:3]
    assert all(u.tobytes() == v.tobytes() and u.shape == v.shape for u, v in zip(alone, after))   # a small call after a large one


# ---- 11. end to end --------------------------------------------------------------------------------------------------------------
def test_three_trackers_to_global_ids(tmp_path):
    streams = scene_streams()
    eng = TrackerEngine(None, 3, 0)
    bank = mtmc.TrackBank(eng, 256)
    F, S = 60, 3
    hw = torch.tensor([[480, 640]] * S, dtype=torch.int32, device=DEV)
    label_lines = [[] for _ in range(S)]
    for g0, g in ((0, 32), (32, 28)):
        d, n, ft = np.zeros((g, S, MAXD, 6), np.float32), np.zeros((g, S), np.int32), np.zeros((g, S, MAXD, 512), np.float32)
        for f in range(g):
            for s in range(S):
                fr = streams[s][0][g0 + f]
                d[f, s, :len(fr.dets)], n[f, s], ft[f, s, :len(fr.dets)] = fr.dets, len(fr.dets), fr.feats
        dd, dn, df = (torch.from_numpy(v).to(DEV) for v in (d, n, ft))
        out, nout = torch.zeros(g, S, MAXT, 8, device=DEV), torch.zeros(g, S, dtype=torch.int32, device=DEV)
        eng.update_group(g, dd, dn, df, hw, out, nout)
        bank.update_group_device(out, nout, df, g)
        torch.cuda.synchronize()
        o, c = out.cpu().numpy(), nout.cpu().numpy()
        for f in range(g):
            for s in range(S):
                for r in o[f, s, :c[f, s]]:
                    if r[7] >= 0:
                        label_lines[s].append(f"{g0 + f} {int(r[5])} {int(r[4])} {round(float(r[6]), 3)} {int(r[0])} {int(r[1])} {int(r[2])} {int(r[3])} -1 -1 -1 -1\n")
    eng.check_errors()
    tables = [bank.table(s) for s in range(S)]
    assert all(len(t["ids"]) >= len(ids) for t, ids in zip(tables, SCENE_IDS))
    # the scene qualifies: no f64 distance within 1e-4 of thr, and the restatement's partition survives 16 perturbations of D by +-1e-4
    desc, cam, ids, first, last, n = R.tracklets(tables)
    D64 = R.dist64(desc)
    iu = np.triu_indices(len(cam), 1)
    assert np.abs(D64[iu] - 0.2).min() > 1e-4
    want_maps, _ = R.link(tables, thr=0.2)
    want_gid = R.cluster(D64.astype(np.float32), cam, first, last, n, 0.2)[0]
    for k in range(16):
        noise = np.triu(np.random.default_rng(k).choice([-1e-4, 1e-4], D64.shape), 1)
        assert R.cluster((D64 + noise).astype(np.float32), cam, first, last, n, 0.2)[0].tolist() == want_gid.tolist()
    info = {}
    maps = mtmc.link(tables, eng, info=info)
    assert maps == want_maps and info["tracklets"] == len(cam) and info["clusters"] == len(set(want_gid.tolist()))
    # every identity that is seen has one global id across the cameras that saw it (the trackers did not split or swap ids here)
    assert info["clusters"] == 12
    # the CLI's post step: the tables from their files, the labels files rewritten with global ids
    out = str(tmp_path)
    names = [f"cam{s}" for s in range(S)]
    for s, name in enumerate(names):
        mtmc.save_table(os.path.join(out, f"{name}_bank.npz"), tables[s])
        with open(os.path.join(out, f"{name}_labels.txt"), "w") as f:
            f.writelines(label_lines[s])
    summary = cli.mtmc_post([f"{n_}.npy" for n_ in names], out, eng, 0.2, 1)
    assert summary["clusters"] == 12 and summary["tracklets"] == [len(t["ids"]) for t in tables]
    for s, name in enumerate(names):
        mtmc.rewrite_labels(os.path.join(out, f"{name}_labels.txt"), os.path.join(out, f"{name}_want.txt"), want_maps[s])
        got, want = (open(os.path.join(out, f"{name}_{k}.txt"), "rb").read() for k in ("labels_mtmc", "want"))
        assert got == want and len(got) > 0
        assert open(os.path.join(out, f"{name}_labels.txt")).read() == "".join(label_lines[s])
    eng.close()
