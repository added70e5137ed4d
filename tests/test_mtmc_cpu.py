"""Multi-camera linking without a device (docs/MTMC.md): the restatement tests/mtmc_ref.py against SciPy, its constraint property, the
shared-identity scene, the bank's rules, and the host layer (refusals, relabel, concat, the labels rewrite)."""
import json

import numpy as np
import pytest

from strongsort_yolo_amd import mtmc
from strongsort_yolo_amd.synth import SynthStream
from tests import mtmc_ref as R


def partition(labels):
    groups = {}
    for i, g in enumerate(labels):
        groups.setdefault(int(g), []).append(i)
    return sorted(groups.values())


# ---- 1. the restatement against SciPy -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_restatement_without_conflicts_is_scipy_average_linkage(seed):
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    rng = np.random.default_rng(seed)
    T = int(rng.integers(2, 40))
    centre = rng.standard_normal((6, 512))
    x = rng.standard_normal((T, 512)) + 3.0 * centre[rng.integers(0, 6, T)]
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    D = R.dist64(x).astype(np.float32)
    gid, merges = R.cluster(D, np.arange(T), np.zeros(T), np.zeros(T), np.ones(T), 0.5)        # every tracklet its own camera
    full = D.astype(np.float64)
    fc = fcluster(linkage(squareform(full + full.T, checks=False), "average"), 0.5, "distance")
    assert partition(gid) == partition(fc)
    assert len(merges) == T - len(set(gid.tolist()))
    assert [g for g in gid[np.unique(gid, return_index=True)[1]]] == sorted(set(gid.tolist()))   # ids rise with the smallest member


# ---- 2. the constraint property -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_no_cluster_holds_a_conflict_and_short_tracklets_stay_alone(seed):
    rng = np.random.default_rng(1000 + seed)
    T = int(rng.integers(6, 60))
    centre = rng.standard_normal((5, 512))
    x = rng.standard_normal((T, 512)) * 0.3 + 3.0 * centre[rng.integers(0, 5, T)]
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    cam = np.sort(rng.integers(0, 3, T))
    first = rng.integers(0, 80, T)
    last = first + rng.integers(0, 30, T)
    n = rng.integers(1, 12, T)
    gid, merges = R.cluster(R.dist64(x).astype(np.float32), cam, first, last, n, 0.5, min_rows=4)
    assert merges, "the problem must merge something"
    conf = R.conflicts(cam, first, last, n, 4)
    for members in partition(gid):
        for i in members:
            for j in members:
                assert not conf[i, j], (members, i, j)
        if any(n[i] < 4 for i in members):
            assert len(members) == 1
    heights = [h for _, _, h in merges]
    assert all(h < 0.5 for h in heights) and all(a < b for a, b, _ in merges)


# ---- 3. the shared-identity scene ------------------------------------------------------------------------------------------------
SCENE_IDS = (list(range(0, 8)), list(range(4, 12)), [0, 1, 5, 6, 10, 11])


def scene_streams(frames=60):
    """Three streams whose identities are drawn from one set of 12 prototypes -> per camera the frames and the identity of every
    local ground-truth id."""
    shared = SynthStream(seed=100, n_ids=12).proto
    out = []
    for seed, ids in enumerate(SCENE_IDS):
        st = SynthStream(seed=seed, n_ids=len(ids), width=640, height=480)
        st.proto = shared[ids].copy()
        out.append(([st.next_frame() for _ in range(frames)], ids))
    return out


def gt_rows(fr):
    """A frame's detections as tracker rows with the ground-truth id + 1 as the track id."""
    r = np.zeros((len(fr.dets), 8), np.float32)
    r[:, :4], r[:, 4], r[:, 5], r[:, 6], r[:, 7] = fr.dets[:, :4], fr.gt_ids + 1, fr.dets[:, 5], fr.dets[:, 4], np.arange(len(fr.dets))
    return r


def gt_tables(streams):
    tables = []
    for frames, _ in streams:
        bank = R.Bank(64)
        for fr in frames:
            f = np.zeros((R.MAX_DETS, 512), np.float32)
            f[:len(fr.feats)] = fr.feats
            bank.update(gt_rows(fr), f)
        tables.append(bank.table())
    return tables


def test_shared_identity_scene_is_recovered_exactly():
    streams = scene_streams()
    tables = gt_tables(streams)
    maps, merges = R.link(tables, thr=0.2)
    ident = {}
    for (_, ids), m in zip(streams, maps):
        assert sorted(m) == list(range(1, len(ids) + 1))
        for local, g in m.items():
            ident.setdefault(g, set()).add(ids[local - 1])
    assert len(ident) == 12 and all(len(v) == 1 for v in ident.values())
    assert sorted(next(iter(v)) for v in ident.values()) == list(range(12))
    assert len(merges) == sum(len(i) for i in SCENE_IDS) - 12
    # the margin the threshold has in this scene
    desc, cam, ids, *_ = R.tracklets(tables)
    who = np.array([SCENE_IDS[c][i - 1] for c, i in zip(cam, ids)])
    D = R.dist64(desc)
    iu = np.triu_indices(len(who), 1)
    same = who[iu[0]] == who[iu[1]]
    assert D[iu][same].max() < 0.02 and D[iu][~same].min() > 0.8


# ---- 4. the bank's rules ---------------------------------------------------------------------------------------------------------
def test_bank_rules():
    rng = np.random.default_rng(5)
    feats = rng.standard_normal((R.MAX_DETS, 512)).astype(np.float32)
    feats[3] = 0.0
    bank = R.Bank(10)
    row = lambda tid, det, cls=2: [0, 0, 1, 1, tid, cls, 0.5, det]
    bank.update(np.array([row(1, 0), row(2, -1), row(3, 3), row(10, 4), row(11, 5)], np.float32), feats)      # frame 0
    assert bank.err and sorted(bank.n) == [1, 10]                                  # det_idx -1, a zero feature and id 11 are skipped
    bank.update(None, feats)                                                     # sat out: the counter stays
    assert bank.frame == 1
    bank.update(np.zeros((0, 8), np.float32), feats)                             # an empty frame counts
    bank.update(np.array([row(1, 7, 4), row(2, 1)], np.float32), feats)          # frame 2
    t = bank.table()
    assert t["ids"].tolist() == [1, 2, 10] and t["n"].tolist() == [2, 1, 1]
    assert t["first"].tolist() == [0, 2, 0] and t["last"].tolist() == [2, 2, 0] and t["cls"].tolist() == [4, 2, 2]
    u0, u7 = R.unit_row(feats[0]), R.unit_row(feats[7])
    s = u0 + u7
    want = (s / np.sqrt(R.butterfly(s * s))).astype(np.float32)
    assert t["desc"][0].tobytes() == want.tobytes()
    assert abs(np.linalg.norm(t["desc"].astype(np.float64), axis=1) - 1).max() < 1e-6
    assert R.unit_row(np.full(512, np.inf, np.float32)) is None and R.unit_row(np.zeros(512, np.float32)) is None
    # the butterfly is a fixed order, not NumPy's pairwise sum
    p = rng.standard_normal(512) ** 2
    m = p.reshape(8, 64).copy()
    v = ((((((m[0] + m[1]) + m[2]) + m[3]) + m[4]) + m[5]) + m[6]) + m[7]
    for h in (32, 16, 8, 4, 2, 1):
        v = v[:h] + v[h:]
    assert R.butterfly(p) == v[0]


# ---- 5. the host layer -----------------------------------------------------------------------------------------------------------
BASE = ["--track", "--mtmc", "--random-init"]


@pytest.mark.parametrize("argv, message", [
    (["--mtmc", "--source", "synthetic:4", "synthetic:5"], "it needs --track"),
    (BASE + ["--source", "synthetic:4"], "at least two --source"),
    (BASE + ["--source", "a/synthetic:4", "b/synthetic:4"], "share the output name"),
    (BASE + ["--source", "synthetic:4", "synthetic:5", "--tracker", "bytetrack"], "tracker_type 'bytetrack' has no appearance features"),
    (BASE + ["--source", "synthetic:4", "synthetic:5", "--tracker", "ocsort"], "tracker_type 'ocsort' has no appearance features"),
    (BASE + ["--source", "synthetic:4", "synthetic:5", "--tracker", "botsort"], "'botsort' without with_reid has no appearance features"),
    (BASE + ["--source", "synthetic:4", "synthetic:5", "--tracker", "botsort", "--with-reid", "--reid-model", "auto"], "reid_model='auto' reads the detector's own features"),
    (BASE + ["--source", "synthetic:4", "synthetic:5", "--tracker", "bytetrack", "--weights", "yolov8n-obb.pt"], "an oriented-box model has no appearance features"),
    (["--track", "--source", "synthetic:4", "synthetic:5", "--mtmc-thr", "0.3"], "options of --mtmc"),
])
def test_cli_refusals(argv, message, capsys):
    from strongsort_yolo_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2 and message in capsys.readouterr().err


@pytest.mark.parametrize("kw, message", [
    (dict(tracker_type="bytetrack"), "tracker_type 'bytetrack'"),
    (dict(tracker_type="ocsort"), "tracker_type 'ocsort'"),
    (dict(tracker_type="botsort"), "without with_reid"),
    (dict(tracker_type="botsort", with_reid=True, reid_model="auto"), "reid_model='auto'"),
])
def test_yolo_refuses_a_bank_without_features(kw, message):
    from strongsort_yolo_amd.yolo import YOLO
    with pytest.raises(ValueError, match=message):
        YOLO("yolov8n.pt", random_init_ok=True, track_bank=True, **kw)
    with pytest.raises(ValueError, match="oriented-box"):
        YOLO("yolov8n-obb.pt", random_init_ok=True, tracker_type="bytetrack", track_bank=True)
    for ok in (dict(), dict(tracker_type="deep_ocsort"), dict(tracker_type="botsort", with_reid=True)):
        assert YOLO("yolov8n.pt", random_init_ok=True, track_bank=True, **ok)._pipe_kw["track_bank"] is True
    m = YOLO("yolov8n.pt", random_init_ok=True)
    assert "track_bank" not in m._pipe_kw
    with pytest.raises(RuntimeError):
        m.track_bank()


def test_relabel_concat_and_tables(tmp_path):
    rows = np.array([[0, 1, 10, 10, 20, 20, 0.9, 0], [0, 2, 30, 30, 40, 40, 0.8, 0], [1, 1, 11, 10, 21, 20, 0.9, 0]], np.float64)
    out = mtmc.relabel(rows, {1: 7, 2: 3})
    assert out[:, 1].tolist() == [7, 3, 7] and np.array_equal(np.delete(out, 1, 1), np.delete(rows, 1, 1)) and rows[0, 1] == 1
    with pytest.raises(KeyError):
        mtmc.relabel(rows, {1: 7})
    b = rows.copy()
    b[:, 0] += 5
    cat = mtmc.concat([rows, b, np.zeros((0, 8))])
    assert cat[:, 0].tolist() == [0, 0, 1, 2, 2, 3] and np.array_equal(cat[:, 1:], np.concatenate([rows, b])[:, 1:])
    assert mtmc.concat([]).shape == (0, 8)
    t = {"ids": np.array([1, 4], np.int32), "n": np.array([3, 1], np.int32), "first": np.array([0, 2], np.int32), "last": np.array([5, 2], np.int32),
         "cls": np.array([0, 1], np.int32), "desc": np.eye(2, 512, dtype=np.float32)}
    path = str(tmp_path / "sub" / "cam_bank.npz")
    mtmc.save_table(path, t)
    back = mtmc.load_table(path)
    assert all(back[k].dtype == t[k].dtype and np.array_equal(back[k], t[k]) for k in mtmc.KEYS)
    with pytest.raises(ValueError):
        mtmc.tracklets([dict(t, ids=np.array([4, 1], np.int32))])
    with pytest.raises(ValueError):
        mtmc.link([t], None)
    s = mtmc.write_summary(str(tmp_path / "mtmc.json"), ["a.npy", "b.npy"], [t, t], [{1: 1, 4: 2}, {1: 1, 4: 3}], {"merges": [(0, 2, 0.01)], "thr": 0.2, "min_rows": 1})
    assert s["clusters"] == 3 and s["global_ids"]["1"] == [["a.npy", 1], ["b.npy", 1]] and json.load(open(tmp_path / "mtmc.json")) == s


def test_labels_rewrite_changes_only_the_id_column(tmp_path):
    lines = ["0 0 1 0.913 10 20 30 40 -1 -1 -1 -1\n", "0 2 12 0.5 1 2 3 4 -1 -1 -1 -1\n", "3 0 1 0.9 11 21 31 41 -1 -1 -1 -1\n", "4 0 5 0.7 0 0 9 9 -1 -1 -1 -1\n"]
    src, dst = tmp_path / "cam_labels.txt", tmp_path / "cam_labels_mtmc.txt"
    src.write_text("".join(lines))
    assert mtmc.rewrite_labels(str(src), str(dst), {1: 4, 12: 1}) == 4
    got = dst.read_text().splitlines(keepends=True)
    assert len(got) == len(lines)
    for a, b, want in zip(lines, got, ("4", "1", "4", "0")):                       # an id without a descriptor gets 0
        pa, pb = a.split(" "), b.split(" ")
        assert pb[2] == want and pa[:2] + pa[3:] == pb[:2] + pb[3:]
    assert src.read_text() == "".join(lines)
