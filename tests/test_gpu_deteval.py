"""COCO AP / AR on the MI355X (csrc/ss_ap.hip, docs/DETEVAL.md) against tests/deteval_ref.py, by equality: the ranks and the match
record as integers, `precision` and `recall` as bytes, the figures by json.dumps."""
import json
import os

import numpy as np
import pytest

from strongsort_yolo_amd import cli, deteval, gsi, lib
from tests import deteval_ref as ref
from tests.golden.make_deteval_golden import NAMES
from tests.gpu_util import engine

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ref.FIGURES + ("AP_class", "classes")


@pytest.fixture(scope="module")
def eng():
    e = engine(debug=False)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "deteval_cases.npz"))


def _check(eng, gt, dt, what="", **kw):
    """one device call through deteval.evaluate_full, twice (the same bytes), against the restatement -> the restatement's dict"""
    got, rec = deteval.evaluate_full(gt, dt, eng, **kw)
    again, rec2 = deteval.evaluate_full(gt, dt, eng, **kw)
    for k in ("precision", "recall", "rank", "kept_rows", "match", "ignored"):
        assert rec[k].tobytes() == rec2[k].tobytes(), f"{what}: the same call twice differs in {k}"
    want = ref.evaluate_full(gt, dt, **kw)
    assert rec["rank"].shape == want["rank"].shape and (rec["rank"] == want["rank"]).all(), f"{what}: {np.count_nonzero(rec['rank'] != want['rank'])} ranks differ"
    assert rec["kept_rows"].tolist() == want["kept_rows"].tolist(), f"{what}: the kept detections"
    assert rec["match"].shape == want["match"].shape and (rec["match"] == want["match"]).all(), f"{what}: {np.count_nonzero(rec['match'] != want['match'])} matches differ"
    assert (rec["ignored"] == want["ignored"]).all(), f"{what}: {np.count_nonzero(rec['ignored'] != want['ignored'])} ignored bits differ"
    for k in ("precision", "recall"):
        assert rec[k].dtype == np.float64 and rec[k].shape == want[k].shape
        assert rec[k].tobytes() == want[k].tobytes(), f"{what}: {np.count_nonzero(rec[k] != want[k])} of {rec[k].size} {k} entries differ"
    assert tuple(got) == KEYS
    assert json.dumps(got) == json.dumps({k: want[k] for k in KEYS}), what
    assert json.dumps(again) == json.dumps(got)
    assert json.dumps(deteval.evaluate(gt, dt, eng, **kw)) == json.dumps(got), f"{what}: without the ranks and the record the figures differ"
    return want


def _cell(rng, n_gt, n_dt, ignored, decimals=2):
    """one image of one class: n_gt boxes whose areas straddle 32^2 and 96^2 (with `ignored` a sixth of them crowd regions), n_dt
    detections: jittered copies and strays"""
    xy, wh = rng.uniform(0, 900, (n_gt, 2)), rng.uniform(8, 160, (n_gt, 2))
    gt = np.zeros((n_gt, 8))
    gt[:, 1] = np.arange(n_gt)
    if ignored and n_gt:
        gt[rng.random(n_gt) < 1 / 6, 1] = -1
    gt[:, 2:4], gt[:, 4:6], gt[:, 6] = xy, xy + wh, 1.0
    dt = np.zeros((n_dt, 8))
    dt[:, 1] = -1
    p, s = rng.uniform(0, 900, (n_dt, 2)), rng.uniform(8, 160, (n_dt, 2))
    dt[:, 2:4], dt[:, 4:6] = p, p + s
    if n_gt:
        hit = rng.random(n_dt) < 0.7
        src = gt[rng.integers(0, n_gt, n_dt), 2:6] + rng.normal(0, 4, (n_dt, 4))
        src[:, 2:] = np.maximum(src[:, 2:], src[:, :2] + 1)
        dt[hit, 2:6] = src[hit]
    dt[:, 6] = np.round(rng.random(n_dt), decimals)
    gt[:, 2:6], dt[:, 2:6] = np.round(gt[:, 2:6] * 8) / 8, np.round(dt[:, 2:6] * 8) / 8
    return gt, dt


# ---- sizes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ignored", [False, True])
@pytest.mark.parametrize("n_gt", [0, 1, 63, 64, 65, 1024])
def test_ground_truth_rows_a_cell(eng, n_gt, ignored):
    """the lanes' edge (63, 64, 65 rows) and the cap; without ignored rows the single range [0, 1e10] keeps every row in the first walk"""
    gt, dt = _cell(np.random.default_rng(n_gt + 7 * ignored), n_gt, 24, ignored)
    kw = {} if ignored else {"areas": [[0, 1e10]]}
    want = _check(eng, gt, dt, f"{n_gt} rows", **kw)
    if n_gt >= 63:
        assert (want["match"] >= 0).any() and want["AR100"] > 0
    if ignored and n_gt >= 63:
        assert want["ignored"].any() and (gt[:, 1] < 0).any()


def test_one_row_too_many_is_refused_and_the_context_scores_on(eng):
    gt, dt = _cell(np.random.default_rng(1), 1025, 3, False)
    with pytest.raises(lib.SSError, match="class 0: image 0: 1025 ground-truth rows: at most 1024 a cell"):
        deteval.evaluate(gt, dt, eng)
    _check(eng, gt[:1024], dt, "after the refusal")


@pytest.mark.parametrize("n_dt", [0, 1, 99, 100, 101])
def test_detections_a_cell_around_the_cut(eng, n_dt):
    gt, dt = _cell(np.random.default_rng(n_dt), 12, n_dt, True)
    want = _check(eng, gt, dt, f"{n_dt} detections")
    assert len(want["kept_rows"]) == min(n_dt, 100)


def test_4096_detections_a_cell_cut_at_1024(eng):
    gt, dt = _cell(np.random.default_rng(4096), 6, 4096, True, decimals=3)
    want = _check(eng, gt, dt, "4096 detections", max_dets=(1, 10, 1024), iou_thrs=[0.5, 0.75], areas=[[0, 1e10], [0, 96.0 ** 2]])
    assert len(want["kept_rows"]) == 1024 and want["rank"].max() == 4095


def _class_of(rng, n_dt, per_image=37):
    """one class with exactly n_dt detections over images of up to per_image detections, scores rounded to one decimal"""
    gts, dts = [], []
    for im, at in enumerate(range(0, n_dt, per_image)):
        g, d = _cell(rng, per_image // 2, min(per_image, n_dt - at), im % 2 == 0, decimals=1)
        g[:, 0], d[:, 0] = im, im
        gts.append(g)
        dts.append(d)
    return np.concatenate(gts), np.concatenate(dts)


@pytest.mark.parametrize("n_dt", [1, 255, 256, 257, 1023, 1025])
def test_detections_a_class_across_the_chunk_borders(eng, n_dt):
    """256 is the sort's and the scan's chunk: one chunk, its edge, the first merge pass, several passes.  Scores have one decimal, so
    ties run across images and within cells."""
    gt, dt = _class_of(np.random.default_rng(n_dt), n_dt)
    want = _check(eng, gt, dt, f"{n_dt} detections a class")
    assert sorted(want["rank"].tolist()) == list(range(n_dt))


def test_70000_detections_a_class_from_one_box_cells(eng):
    """274 chunks and 9 merge passes; one-box cells, two thresholds and one area range (which leaves ignored rows on both sides) keep
    the restatement's loops to about three seconds"""
    gt, dt = ref.one_box_cells(np.random.default_rng(70000), 70001)
    want = _check(eng, gt, dt, "70001 cells", iou_thrs=[0.5, 0.95], areas=[[0, 64.0 ** 2]], max_dets=(1,))
    assert 0.3 < want["AP"] < 0.9 and abs(want["AR100"] - 0.7) < 0.02 and want["ignored"].any() and not want["ignored"].all()


# ---- scores and ties ----------------------------------------------------------------------------------------------------------------
def test_negative_zero_ties_zero(eng):
    rng = np.random.default_rng(5)
    gt, dt = _class_of(rng, 300)
    dt[:, 6] = np.where(rng.random(len(dt)) < 0.5, -0.0, 0.0)
    dt[::7, 6] = 0.5
    dt[3::11, 6] = -0.5
    want = _check(eng, gt, dt[rng.permutation(len(dt))], "signed zeros")
    assert np.signbit(dt[:, 6]).any() and (dt[:, 6] == 0).sum() > 100 and want["AR100"] > 0


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_golden_cases(eng, golden, name):
    """mixed (crowd regions), ties, sizes (three classes of very different size in one call), sparse (recall never reaches 1)"""
    gt, dt = golden[f"{name}_gt"], golden[f"{name}_dt"]
    got, rec = deteval.evaluate_full(gt, dt, eng)
    assert json.dumps(got) == str(golden[f"{name}_figures"])
    assert rec["precision"].tobytes() == golden[f"{name}_precision"].tobytes() and rec["recall"].tobytes() == golden[f"{name}_recall"].tobytes()
    assert (rec["rank"] == golden[f"{name}_rank"]).all() and (rec["kept_rows"] == golden[f"{name}_kept_rows"]).all()
    assert (rec["match"] == golden[f"{name}_match"]).all() and (rec["ignored"] == golden[f"{name}_ignored"]).all()
    _check(eng, gt, dt, name)


def _g(frame, x, y, w, h, cls=0, crowd=False, i=0):
    return [frame, -1 if crowd else i, x, y, x + w, y + h, 1.0, cls]


def _d(frame, x, y, w, h, score, cls=0):
    return [frame, -1, x, y, x + w, y + h, score, cls]


def test_closed_forms(eng, golden):
    P1 = 1.0 / (1.0 + 2.0 ** -52)
    # a set against itself
    gt = golden["sizes_gt"]
    gt = np.concatenate([gt[gt[:, 1] >= 0], np.array([_g(2, 5, 5, 40, 40, cls=9)], np.float64)])
    gt = gt[np.sort(np.unique(gt[:, [0, 7, 2, 3, 4, 5]], axis=0, return_index=True)[1])]
    dt = gt.copy()
    dt[:, 1], dt[:, 6] = -1, 1.0
    want = _check(eng, gt, dt, "self")
    assert want["AR100"] == 1.0 and set(want["precision"][:, :, :, 0, -1].ravel().tolist()) == {1.0, 0.9999999999999998}
    # TP, FP, TP
    gt = np.array([_g(0, 0, 0, 10, 10, i=0), _g(0, 100, 100, 20, 20, i=1)], np.float64)
    dt = np.array([_d(0, 0, 0, 10, 10, 0.9), _d(0, 300, 300, 10, 10, 0.8), _d(0, 100, 100, 20, 20, 0.7)], np.float64)
    got = deteval.evaluate(gt, dt, eng)
    assert abs(got["AP"] - 0.834983) < 1e-6 and got["AR1"] == 0.5 and got["APm"] == -1.0 and got["APl"] == -1.0
    _check(eng, gt, dt, "tp fp tp")
    # a class without detections, a class without ground truth
    gt = np.array([_g(0, 0, 0, 40, 40, cls=1), _g(1, 0, 0, 40, 40, cls=2)], np.float64)
    dt = np.array([_d(1, 0, 0, 40, 40, 0.5, cls=2), _d(0, 5, 5, 40, 40, 0.9, cls=7)], np.float64)
    want = _check(eng, gt, dt, "empty sides")
    assert (want["precision"][:, :, 0, 0] == 0).all() and (want["precision"][:, :, 2] == -1).all() and want["AP_class"][2] == -1.0
    _check(eng, gt, np.zeros((0, 8)), "no detections at all")
    _check(eng, np.zeros((0, 8)), dt, "no ground truth at all")
    # similarity exactly 1/2
    want = _check(eng, np.array([_g(0, 0, 0, 20, 10)], np.float64), np.array([_d(0, 0, 0, 10, 10, 0.9)], np.float64), "one half")
    assert want["match"][0, :, 0].tolist() == [0] + [-1] * 9
    # an area of exactly 32^2
    want = _check(eng, np.array([_g(0, 0, 0, 32, 32)], np.float64), np.array([_d(0, 0, 0, 32, 32, 0.9)], np.float64), "32 squared")
    assert (want["precision"][:, :, 0, 1:3, -1] == P1).all()
    # a crowd region absorbs
    gt = np.array([_g(0, 0, 0, 100, 100, crowd=True), _g(0, 200, 200, 50, 50, i=1)], np.float64)
    dt = np.array([_d(0, 10, 10, 20, 20, 0.9), _d(0, 40, 40, 20, 20, 0.8), _d(0, 70, 70, 20, 20, 0.7), _d(0, 200, 200, 50, 50, 0.6)], np.float64)
    want = _check(eng, gt, dt, "crowd")
    assert want["match"][0, 0].tolist() == [0, 0, 0, 1] and want["ignored"][0, 0].tolist() == [True, True, True, False]
    # an unmatched detection outside the area range
    gt = np.array([_g(0, 0, 0, 20, 20)], np.float64)
    dt = np.array([_d(0, 300, 300, 200, 200, 0.9), _d(0, 0, 0, 20, 20, 0.8)], np.float64)
    want = _check(eng, gt, dt, "outside")
    assert (want["precision"][:, :, 0, 1, -1] == P1).all() and (want["precision"][:, :, 0, 0, -1] == 0.5).all()
    # two identical ground-truth boxes
    gt = np.array([_g(0, 0, 0, 30, 30, i=0), _g(0, 0, 0, 30, 30, i=1)], np.float64)
    dt = np.array([_d(0, 0, 0, 30, 30, 0.9), _d(0, 0, 0, 30, 30, 0.8)], np.float64)
    assert _check(eng, gt, dt, "twins")["match"][0, 0].tolist() == [1, 0]


def test_custom_thresholds_and_max_dets(eng, golden):
    gt, dt = golden["mixed_gt"], golden["mixed_dt"]
    exact = dt[::5].copy()                                         # detections that are a ground-truth box: similarity 1 passes the threshold 1.0
    exact[:, 2:6] = gt[np.arange(len(exact)) % len(gt), 2:6]
    exact[:, [0, 7]] = gt[np.arange(len(exact)) % len(gt)][:, [0, 7]]
    dt = np.concatenate([dt, exact])
    want = _check(eng, gt, dt, "custom", iou_thrs=[0.3, 0.75, 1.0], rec_thrs=np.linspace(0, 1, 11), areas=[[0, 1e10], [0, 50.0 ** 2]], max_dets=(2, 5))
    assert (want["match"][0, 2] >= 0).any() and want["precision"].shape == (3, 11, 4, 2, 2) and want["APm"] == -1.0
    _check(eng, gt, dt, "sixteen thresholds", iou_thrs=np.linspace(0.25, 1.0, 16), max_dets=(1, 3, 7, 1000), rec_thrs=np.linspace(0, 1, 1024),
           areas=[[0, 1e10]] + [[k * 1000.0, (k + 2) * 1000.0] for k in range(7)])


def test_evaluate_with_classes(eng, golden):
    gt, dt = golden["mixed_gt"], golden["mixed_dt"]
    got = deteval.evaluate(gt, dt, eng, classes=[1, 3])
    assert got["classes"] == [1.0, 3.0]
    assert json.dumps(got) == json.dumps(ref.evaluate(gt, dt, classes=[1, 3]))
    keep_g, keep_d = np.isin(gt[:, 7], (1, 3)), np.isin(dt[:, 7], (1, 3))
    assert json.dumps(got) == json.dumps(deteval.evaluate(gt[keep_g], dt[keep_d], eng))


def test_probiou_on_rotated_scenes(eng):
    from tests import obb_ref
    rng = np.random.default_rng(11)
    gts, dts = [], []
    for im in range(6):
        b = obb_ref.probiou_boxes(20, 100 + im)[6:].astype(np.float64)          # (rows 0 .. 5 are the degenerate ones)
        g = np.zeros((len(b), 9))
        g[:, 0], g[:, 1], g[:, 2:7], g[:, 7], g[:, 8] = im, np.arange(len(b)), b, 1.0, rng.integers(0, 2, len(b))
        d = g[rng.random(len(g)) < 0.8].copy()
        d[:, 2:4] += rng.normal(0, 1.5, (len(d), 2))
        d[:, 6] += rng.normal(0, 0.05, len(d))
        d[:, 1], d[:, 7] = -1, np.round(rng.random(len(d)), 2)
        stray = d[:3].copy()
        stray[:, 2:4] += 500.0
        gts.append(g)
        dts += [d, stray]
    gt, dt = np.concatenate(gts), np.concatenate(dts)
    gt[:, 2:7], dt[:, 2:7] = gt[:, 2:7].astype(np.float32), dt[:, 2:7].astype(np.float32)
    want = _check(eng, gt, dt, "probiou", similarity="probiou")
    assert 0.05 < want["AP"] < 1 and (want["match"] >= 0).any()
    crowd = gt.copy()
    crowd[0, 1] = -1
    with pytest.raises(ValueError, match="crowd region cannot be scored with probiou"):
        deteval.evaluate(crowd, dt, eng, similarity="probiou")
    _check(eng, gt, dt, "probiou after the refusal", similarity="probiou", max_dets=(5,))


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_cli_eval_det_gt_with_and_without_track(eng, tmp_path):
    """--eval-det-gt scores <name>_dets.txt against the given file; without the flag every file is byte for byte what it was"""
    from strongsort_yolo_amd.yolo import YOLO
    z = np.load(os.path.join(GOLD, "jpeg_sequence.npz"))
    src = tmp_path / "seq.npy"
    np.save(src, np.stack([np.ascontiguousarray(z[f"rgb_{i}"][:, :, ::-1]) for i in range(8)]))
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack")
    base = {"source": str(src), "track": True, "count": False, "tracker": "bytetrack", "batch": 4, "random_init": True}
    plain = cli.process_video({**base, "outdir": str(tmp_path / "a")}, model=model)
    assert sorted(os.listdir(tmp_path / "a")) == ["seq_labels.txt"] and not {"AP", "AP50", "AR100"} & set(plain)
    rows = deteval.read_labels(str(tmp_path / "a" / "seq_labels.txt"))
    assert len(rows)
    rng = np.random.default_rng(0)
    truth = rows[rng.random(len(rows)) >= 0.2]
    truth[:, 2:6] += 2.0
    gsi.write_labels(str(tmp_path / "gt.txt"), truth)
    truth = deteval.read_labels(str(tmp_path / "gt.txt"))
    for run, extra in (("b", {}), ("c", {"track": False, "eval_det_max_dets": [1, 5], "eval_det_classes": sorted(set(truth[:, 7].astype(int).tolist()))[:2]})):
        model._stream_pipe.reset_tracker(-1)
        model._frame_index = 0
        out = cli.process_video({**base, "outdir": str(tmp_path / run), "eval_det_gt": str(tmp_path / "gt.txt"), **extra}, model=model)
        dets = deteval.read_labels(str(tmp_path / run / "seq_dets.txt"))
        assert len(dets) and (dets[:, 1] == -1).all()
        ok = lambda r: (r[:, 4] > r[:, 2]) & (r[:, 5] > r[:, 3])
        kw = {"max_dets": (1, 5), "classes": extra["eval_det_classes"]} if run == "c" else {}
        want = ref.evaluate(truth[ok(truth)], dets[ok(dets)], **kw)
        got = json.loads((tmp_path / run / "seq_det_metrics.json").read_text())
        assert json.dumps({k: got[k] for k in KEYS}) == json.dumps(want)
        assert [out[k] for k in ("AP", "AP50", "AR100")] == [want[k] for k in ("AP", "AP50", "AR100")]
        assert got["gt_rows"] == int(ok(truth).sum()) and got["det_rows"] == int(ok(dets).sum()) and got["similarity"] == "iou"
    assert (tmp_path / "b" / "seq_labels.txt").read_bytes() == (tmp_path / "a" / "seq_labels.txt").read_bytes()
    assert sorted(os.listdir(tmp_path / "b")) == ["seq_det_metrics.json", "seq_dets.txt", "seq_labels.txt"]
    model.close()


def test_cli_eval_det_gt_scores_an_obb_model_by_probiou(tmp_path):
    """an -obb model: <name>_dets_obb.txt against the ground truth's `_obb` file, by ProbIoU"""
    from tests.test_gpu_obb import _obb_model
    model, frames, _, _ = _obb_model("bytetrack")
    np.save(tmp_path / "clip.npy", np.stack(frames))
    base = {"source": str(tmp_path / "clip.npy"), "track": True, "count": False, "tracker": "bytetrack", "batch": 8}
    cli.process_video({**base, "outdir": str(tmp_path / "a")}, model=model)
    model.close()
    lines = (tmp_path / "a" / "clip_labels_obb.txt").read_text().splitlines()
    assert len(lines) > 20 and sorted(os.listdir(tmp_path / "a")) == ["clip_labels.txt", "clip_labels_obb.txt"]
    (tmp_path / "gt.txt").write_text("")                                      # the axis-aligned half of the pair is not read for an -obb model
    (tmp_path / "gt_obb.txt").write_text("\n".join(ln for k, ln in enumerate(lines) if k % 5) + "\n")
    model = _obb_model("bytetrack")[0]
    out = cli.process_video({**base, "outdir": str(tmp_path / "b"), "eval_det_gt": str(tmp_path / "gt.txt")}, model=model)
    model.close()
    assert (tmp_path / "b" / "clip_labels_obb.txt").read_text().splitlines() == lines
    gt, dt = deteval.read_labels_obb(str(tmp_path / "gt_obb.txt")), deteval.read_labels_obb(str(tmp_path / "b" / "clip_dets_obb.txt"))
    assert len(dt) >= len(lines) and (dt[:, 1] == -1).all() and len(deteval.read_labels(str(tmp_path / "b" / "clip_dets.txt"))) == len(dt)
    want = ref.evaluate(gt, dt, similarity="probiou")
    got = json.loads((tmp_path / "b" / "clip_det_metrics.json").read_text())
    assert json.dumps({k: got[k] for k in KEYS}) == json.dumps(want) and got["similarity"] == "probiou" and got["dropped_rows"] == 0
    assert out["AP"] == want["AP"] > 0.5 and out["AR100"] == want["AR100"]
