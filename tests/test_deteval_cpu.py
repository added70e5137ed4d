"""COCO AP / AR without a GPU (docs/DETEVAL.md): the restatement tests/deteval_ref.py against closed forms and against a second,
vectorised statement written the way pycocotools accumulates (whole-matrix IoU, np.maximum.accumulate on the reversed precision,
np.searchsorted); the host half of strongsort_yolo_amd.deteval on top of that second statement; the golden file; the labels readers;
the parser; and every refusal ss_ap_eval makes before it looks at the context, through the library with ctx NULL."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from strongsort_yolo_amd import cli, deteval, lib
from tests import deteval_ref as ref
from tests.golden.make_deteval_golden import NAMES, check_deterministic, make_case

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P1 = 1.0 / (1.0 + 2.0 ** -52)
# the largest |difference| between the restatement's floats and the vectorised statement's seen on the golden cases is 0.0 (every
# float is the same elementwise expression on the same integers); the bound is ten times that (docs/DETEVAL.md §5)
VEC_BOUND = 10 * 0.0


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "deteval_cases.npz"))


def _gt(frame, x, y, w, h, cls=0, crowd=False, i=0):
    return [frame, -1 if crowd else i, x, y, x + w, y + h, 1.0, cls]


def _dt(frame, x, y, w, h, score, cls=0):
    return [frame, -1, x, y, x + w, y + h, score, cls]


# ---- closed forms ------------------------------------------------------------------------------------------------------------------
def test_a_set_scored_against_itself(golden):
    gt = golden["sizes_gt"]
    gt = np.concatenate([gt[gt[:, 1] >= 0], np.array([_gt(2, 5, 5, 40, 40, cls=9)], np.float64)])       # and a class of one box
    # identical boxes of a cell would share their matches: keep the first of each
    _, first = np.unique(gt[:, [0, 7, 2, 3, 4, 5]], axis=0, return_index=True)
    gt = gt[np.sort(first)]
    dt = gt.copy()
    dt[:, 1], dt[:, 6] = -1, 1.0
    out = ref.evaluate_full(gt, dt)
    n = np.array([np.count_nonzero(gt[:, 7] == c) for c in out["classes"]])
    assert 1 in n and n.max() > 1
    want = n / (n + 2.0 ** -52)
    assert sorted(set(want.tolist())) == [0.9999999999999998, 1.0]
    for k in range(len(n)):
        assert (out["precision"][:, :, k, 0, -1] == want[k]).all()
    p = out["precision"][..., -1]                                                    # (with fewer kept detections than boxes recall stays below 1)
    assert np.isin(p[p > -1], (1.0, 0.9999999999999998)).all()
    assert out["AR100"] == 1.0 and (out["recall"][:, :, 0, -1] == 1.0).all()


def test_tp_fp_tp_on_one_image():
    gt = np.array([_gt(0, 0, 0, 10, 10, i=0), _gt(0, 100, 100, 20, 20, i=1)], np.float64)
    dt = np.array([_dt(0, 0, 0, 10, 10, 0.9), _dt(0, 300, 300, 10, 10, 0.8), _dt(0, 100, 100, 20, 20, 0.7)], np.float64)
    out = ref.evaluate_full(gt, dt)
    row = np.array([P1] * 51 + [2.0 / 3.0] * 50)
    assert (out["precision"][:, :, 0, 0, -1] == row[None, :]).all()
    assert abs(out["AP"] - (51 * P1 + 50 * (2 / 3)) / 101) < 1e-13 and abs(out["AP"] - 0.834983) < 1e-6
    assert out["AR1"] == 0.5 and out["AR10"] == 1.0 and out["AR100"] == 1.0
    assert out["APm"] == -1.0 and out["APl"] == -1.0 and out["ARm"] == -1.0
    assert out["match"][0, 0].tolist() == [0, -1, 1] and not out["ignored"][0].any()


def test_a_class_without_detections_and_a_class_without_ground_truth():
    gt = np.array([_gt(0, 0, 0, 40, 40, cls=1), _gt(1, 0, 0, 40, 40, cls=2)], np.float64)
    dt = np.array([_dt(1, 0, 0, 40, 40, 0.5, cls=2), _dt(0, 5, 5, 40, 40, 0.9, cls=7)], np.float64)
    out = ref.evaluate_full(gt, dt)
    assert out["classes"] == [1.0, 2.0, 7.0]
    assert (out["precision"][:, :, 0, 0, :] == 0.0).all() and (out["recall"][:, 0, 0, :] == 0.0).all()          # ground truth, no detections
    assert (out["precision"][:, :, 2] == -1.0).all() and (out["recall"][:, 2] == -1.0).all()                      # detections, no ground truth
    assert (out["precision"][:, :, 1, 0, -1] == P1).all()
    assert out["AP_class"][0] == 0.0 and abs(out["AP_class"][1] - P1) < 1e-13 and out["AP_class"][2] == -1.0
    assert abs(out["AP"] - P1 / 2) < 1e-13                                                                         # class 7 does not enter


def test_similarity_exactly_one_half_matches_at_one_half():
    gt = np.array([_gt(0, 0, 0, 20, 10)], np.float64)
    dt = np.array([_dt(0, 0, 0, 10, 10, 0.9)], np.float64)                          # inside a box of twice its area
    assert ref.sim_iou(dt[0, 2:6], gt[:, 2:6], np.array([False]))[0] == 0.5
    out = ref.evaluate_full(gt, dt)
    assert out["match"][0, :, 0].tolist() == [0] + [-1] * 9
    assert out["recall"][:, 0, 0, -1].tolist() == [1.0] + [0.0] * 9


def test_an_area_of_exactly_32_squared_is_small_and_medium():
    gt = np.array([_gt(0, 0, 0, 32, 32)], np.float64)
    dt = np.array([_dt(0, 0, 0, 32, 32, 0.9)], np.float64)
    out = ref.evaluate_full(gt, dt)
    assert (out["precision"][:, :, 0, 1:3, -1] == P1).all() and (out["precision"][:, :, 0, 3, -1] == -1.0).all()
    assert abs(out["APs"] - P1) < 1e-13 and abs(out["APm"] - P1) < 1e-13 and out["APl"] == -1.0
    assert out["ARs"] == 1.0 and out["ARm"] == 1.0


def test_a_crowd_region_absorbs_detections():
    gt = np.array([_gt(0, 0, 0, 100, 100, crowd=True), _gt(0, 200, 200, 50, 50, i=1)], np.float64)
    dt = np.array([_dt(0, 10, 10, 20, 20, 0.9), _dt(0, 40, 40, 20, 20, 0.8), _dt(0, 70, 70, 20, 20, 0.7), _dt(0, 200, 200, 50, 50, 0.6)], np.float64)
    out = ref.evaluate_full(gt, dt)
    assert out["match"][0, 0].tolist() == [0, 0, 0, 1]                                # inside the region: similarity 1 against it
    assert out["ignored"][0, 0].tolist() == [True, True, True, False]
    assert (out["precision"][:, :, 0, 0, -1] == P1).all() and out["AR100"] == 1.0      # none of the three is a false positive


def test_an_unmatched_detection_outside_the_area_range_is_no_false_positive():
    gt = np.array([_gt(0, 0, 0, 20, 20)], np.float64)                                 # small
    dt = np.array([_dt(0, 300, 300, 200, 200, 0.9), _dt(0, 0, 0, 20, 20, 0.8)], np.float64)      # a large stray ahead of the hit
    out = ref.evaluate_full(gt, dt)
    assert out["ignored"][1, 0].tolist() == [True, False] and out["ignored"][0, 0].tolist() == [False, False]
    assert (out["precision"][:, :, 0, 1, -1] == P1).all()                             # small: the stray does not count
    assert (out["precision"][:, :, 0, 0, -1] == 0.5).all()                            # all: it does: 1 / (2 + 2^-52)


def test_of_two_identical_ground_truth_boxes_the_later_is_taken_first():
    gt = np.array([_gt(0, 0, 0, 30, 30, i=0), _gt(0, 0, 0, 30, 30, i=1)], np.float64)
    dt = np.array([_dt(0, 0, 0, 30, 30, 0.9), _dt(0, 0, 0, 30, 30, 0.8)], np.float64)
    out = ref.evaluate_full(gt, dt)
    assert out["match"][0, 0].tolist() == [1, 0]


def test_negative_zero_and_zero_scores_tie():
    gt = np.array([_gt(f, 0, 0, 30, 30) for f in range(3)], np.float64)
    dt = np.array([_dt(2, 0, 0, 30, 30, 0.0), _dt(0, 0, 0, 30, 30, -0.0), _dt(1, 0, 0, 30, 30, 0.0), _dt(0, 50, 50, 30, 30, 0.0)], np.float64)
    assert ref.evaluate_full(gt, dt)["rank"].tolist() == [3, 0, 2, 1]                 # (image, input index) alone


def test_refused_rows():
    gt = np.array([_gt(0, 0, 0, 10, 10)], np.float64)
    for bad, msg in ((np.nan, "NaN or infinity"), (np.inf, "NaN or infinity")):
        d = np.array([_dt(0, 0, 0, 10, 10, bad)], np.float64)
        for f in (ref.evaluate_full, lambda g, x: deteval.evaluate_full(g, x, None)):
            with pytest.raises(ValueError, match=msg):
                f(gt, d)
    for box in ([0, -1, 5, 5, 5, 9, 0.5, 0], [0, -1, 5, 5, 9, 4, 0.5, 0]):
        for f in (ref.evaluate_full, lambda g, x: deteval.evaluate_full(g, x, None)):
            with pytest.raises(ValueError, match="x2 <= x1 or y2 <= y1"):
                f(gt, np.array([box], np.float64))
    g9 = np.array([[0, -1, 50, 50, 20, 10, 0.1, 1.0, 0]], np.float64)
    d9 = np.array([[0, -1, 50, 50, 20, 10, 0.1, 0.9, 0]], np.float64)
    for f in (lambda g, x: ref.evaluate_full(g, x, similarity="probiou"), lambda g, x: deteval.evaluate_full(g, x, None, similarity="probiou")):
        with pytest.raises(ValueError, match="crowd region cannot be scored with probiou"):
            f(g9, d9)
        bad = d9.copy()
        bad[0, 4] = 0.0
        with pytest.raises(ValueError, match="w <= 0 or h <= 0"):
            f(g9 * [1, -1, 1, 1, 1, 1, 1, 1, 1], bad)
    with pytest.raises(ValueError, match=r"iou_thrs must be in \(0, 1\]"):
        deteval.evaluate_full(gt, np.array([_dt(0, 0, 0, 10, 10, 0.5)], np.float64), None, iou_thrs=[0.5, 1.5])
    with pytest.raises(ValueError, match="nothing to score"):
        deteval.evaluate_full(np.zeros((0, 8)), np.zeros((0, 8)), None)


# ---- the second statement: ss_ap_eval's packed arguments in, its arrays out ----------------------------------------------------------
def vec_ap_eval(similarity, class_cell_off, cell_image, cell_gt_off, cell_det_off, gt_boxes, gt_crowd, det_boxes, det_scores, iou_thrs, rec_thrs,
                areas, max_dets, want_rank=False, want_record=False):
    assert similarity == 0
    gt_boxes, det_boxes, gt_crowd = np.asarray(gt_boxes, np.float64).reshape(-1, 4), np.asarray(det_boxes, np.float64).reshape(-1, 4), np.asarray(gt_crowd) != 0
    areas = np.asarray(areas, np.float64).reshape(-1, 2)
    K, T, R, A, M = len(class_cell_off) - 1, len(iou_thrs), len(rec_thrs), len(areas), len(max_dets)
    keep = int(max_dets[-1])
    g_area = np.prod(gt_boxes[:, 2:] - gt_boxes[:, :2], 1)
    d_area = np.prod(det_boxes[:, 2:] - det_boxes[:, :2], 1)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    rank = np.zeros(len(det_scores), np.int32)
    n_kept = int(np.minimum(np.diff(cell_det_off), keep).sum())
    match, ignored = -np.ones((A, T, n_kept), np.int32), np.zeros((A, T, n_kept), np.int32)
    slot = -np.ones(len(det_scores), np.int64)
    pos = np.zeros(len(det_scores), np.int64)
    at = 0
    for k in range(K):
        c0, c1 = int(class_cell_off[k]), int(class_cell_off[k + 1])
        d0, d1 = int(cell_det_off[c0]), int(cell_det_off[c1])
        order = d0 + np.argsort(-np.asarray(det_scores[d0:d1]), kind="stable")
        rank[order] = np.arange(d1 - d0)
        for c in range(c0, c1):
            g = slice(int(cell_gt_off[c]), int(cell_gt_off[c + 1]))
            d = np.arange(int(cell_det_off[c]), int(cell_det_off[c + 1]))
            d = d[np.argsort(rank[d], kind="stable")]
            pos[d] = np.arange(len(d))
            d = d[:keep]
            slot[d] = at + np.arange(len(d))
            G, D = gt_boxes[g], det_boxes[d]
            wh = np.clip(np.minimum(D[:, None, 2:], G[None, :, 2:]) - np.maximum(D[:, None, :2], G[None, :, :2]), 0, None)
            inter = wh[..., 0] * wh[..., 1]
            S = np.where(gt_crowd[g][None, :], inter / d_area[d][:, None], inter / ((d_area[d][:, None] + g_area[g][None, :]) - inter))
            for a, (lo, hi) in enumerate(areas):
                g_ig = gt_crowd[g] | (g_area[g] < lo) | (g_area[g] > hi)
                for t, thr in enumerate(iou_thrs):
                    taken = np.zeros(len(G), bool)
                    for p in range(len(d)):
                        ok = (S[p] >= min(thr, 1 - 1e-10)) & (~taken | gt_crowd[g])
                        m = -1
                        for group in (ok & ~g_ig, ok & g_ig):
                            if group.any():
                                best = S[p][group].max()
                                m = int(np.nonzero(group & (S[p] == best))[0][-1])
                                break
                        match[a, t, at + p] = m
                        ignored[a, t, at + p] = g_ig[m] if m >= 0 else (d_area[d[p]] < lo or d_area[d[p]] > hi)
                        if m >= 0:
                            taken[m] = True
            at += len(d)
        gk = slice(int(cell_gt_off[c0]), int(cell_gt_off[c1]))
        for a, (lo, hi) in enumerate(areas):
            npig = int(np.count_nonzero(~gt_crowd[gk] & (g_area[gk] >= lo) & (g_area[gk] <= hi)))
            if npig == 0:
                continue
            for mi, md in enumerate(max_dets):
                lst = order[pos[order] < md]
                for t in range(T):
                    mt, ig = match[a, t, slot[lst]] >= 0, ignored[a, t, slot[lst]] != 0
                    tp, fp = np.cumsum(mt & ~ig), np.cumsum(~mt & ~ig)
                    rc, pr = tp / npig, tp / ((fp + tp) + np.spacing(1))
                    recall[t, k, a, mi] = rc[-1] if len(lst) else 0.0
                    env = np.maximum.accumulate(pr[::-1])[::-1]
                    inds = np.searchsorted(rc, rec_thrs, side="left")
                    q = np.zeros(R)
                    q[inds < len(lst)] = env[inds[inds < len(lst)]]
                    precision[t, :, k, a, mi] = q
    out = (precision, recall)
    if want_rank:
        out += (rank,)
    if want_record:
        out += (match, ignored)
    return out


class VecEngine:
    calls = 0

    def ap_eval(self, *a, **kw):
        self.calls += 1
        return vec_ap_eval(*a, **kw)


def _same(got, rec, want, bound=0.0):
    """deteval's (figures, record) against the restatement's dict: integers and records equal, floats within `bound`"""
    assert (rec["rank"] == want["rank"]).all() and rec["rank"].shape == want["rank"].shape
    assert rec["kept_rows"].tolist() == want["kept_rows"].tolist()
    assert rec["match"].shape == want["match"].shape and (rec["match"] == want["match"]).all() and (rec["ignored"] == want["ignored"]).all()
    worst = 0.0
    for k in ("precision", "recall"):
        assert rec[k].shape == want[k].shape
        worst = max(worst, float(np.abs(rec[k] - want[k]).max()) if rec[k].size else 0.0)
    for k in ref.FIGURES:
        worst = max(worst, abs(got[k] - want[k]))
    assert got["classes"] == want["classes"] and len(got["AP_class"]) == len(want["AP_class"])
    assert worst <= bound, worst
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_the_vectorised_statement(golden, name):
    gt, dt = golden[f"{name}_gt"], golden[f"{name}_dt"]
    eng = VecEngine()
    got, rec = deteval.evaluate_full(gt, dt, eng)
    assert eng.calls == 1
    worst = _same(got, rec, ref.evaluate_full(gt, dt), VEC_BOUND)
    print(f"{name}: largest difference {worst}")


def test_module_host_half_on_custom_parameters_and_any_row_order(golden):
    gt, dt = golden["mixed_gt"], golden["mixed_dt"]
    eng = VecEngine()
    kw = dict(iou_thrs=[0.3, 0.75, 1.0], rec_thrs=np.linspace(0, 1, 11), areas=[[0, 1e10], [0, 50.0 ** 2]], max_dets=(2, 5))
    got, rec = deteval.evaluate_full(gt, dt, eng, **kw)
    want = ref.evaluate_full(gt, dt, **kw)
    _same(got, rec, want)
    assert want["APm"] == -1.0 and want["AR100"] == got["AR100"] and rec["precision"].shape == (3, 11, 4, 2, 2)
    assert json.dumps(deteval.evaluate(gt, dt, eng, classes=[0, 2])) == json.dumps(ref.evaluate(gt, dt, classes=[0, 2]))
    assert deteval.evaluate(gt, dt, eng, classes=[0, 2])["classes"] == [0.0, 2.0]
    # the figures do not depend on the order of the ground-truth rows' images or of the classes' rows among each other
    perm = np.random.default_rng(3).permutation(len(dt))
    a, b = deteval.evaluate_full(gt, dt[perm], eng), ref.evaluate_full(gt, dt[perm])
    _same(a[0], a[1], b)


def test_golden_file_is_what_the_restatement_computes(golden):
    assert os.path.getsize(os.path.join(GOLD, "deteval_cases.npz")) < 1 << 20
    for name in NAMES:
        gt, dt = make_case(name)
        assert gt.tobytes() == golden[f"{name}_gt"].tobytes() and dt.tobytes() == golden[f"{name}_dt"].tobytes(), name
        check_deterministic(name, gt, dt)
        full = ref.evaluate_full(gt, dt)
        assert json.dumps({k: full[k] for k in ref.FIGURES + ("AP_class", "classes")}) == str(golden[f"{name}_figures"]), name
        assert full["precision"].tobytes() == golden[f"{name}_precision"].tobytes() and full["recall"].tobytes() == golden[f"{name}_recall"].tobytes()
        assert (full["rank"] == golden[f"{name}_rank"]).all() and (full["kept_rows"] == golden[f"{name}_kept_rows"]).all()
        assert (full["match"] == golden[f"{name}_match"]).all() and (full["ignored"] == golden[f"{name}_ignored"]).all()
    sp = golden["sparse_precision"]
    assert (sp[:, -1, :, 0, -1] == 0).all() and (golden["sparse_recall"][:, :, 0, -1] < 1).all()             # recall never reaches 1: trailing zeros
    assert (golden["sparse_recall"][:, :, 0, -1] > 0).any()
    assert (golden["ties_dt"][:, 6] * 10 == np.round(golden["ties_dt"][:, 6] * 10)).all()


# ---- labels, parser ----------------------------------------------------------------------------------------------------------------
def test_read_labels_obb(tmp_path):
    (tmp_path / "o.txt").write_text("3 2 -1 0.875 100.25 50.50 40.00 10.00 0.78540\n\n4 0 7 0.5 1.00 2.00 3.00 4.00 -0.10000\n")
    got = deteval.read_labels_obb(str(tmp_path / "o.txt"))
    assert got.dtype == np.float64 and got.tolist() == [[3, -1, 100.25, 50.5, 40, 10, 0.7854, 0.875, 2], [4, 7, 1, 2, 3, 4, -0.1, 0.5, 0]]
    (tmp_path / "e.txt").write_text("")
    assert deteval.read_labels_obb(str(tmp_path / "e.txt")).shape == (0, 9)
    (tmp_path / "bad.txt").write_text("1 2 3 4 5 6 7 8\n")
    with pytest.raises(ValueError, match="bad.txt:1"):
        deteval.read_labels_obb(str(tmp_path / "bad.txt"))
    assert deteval.read_labels is __import__("strongsort_yolo_amd.moteval", fromlist=["x"]).read_labels


def test_eval_det_gt_parser_errors(capsys, tmp_path):
    with pytest.raises(SystemExit):
        cli.main(["--source", "synthetic:2", "synthetic:3", "--eval-det-gt", "gt.txt"])
    assert "one ground-truth file per --source" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["--source", "synthetic:2", "--eval-det-gt", str(tmp_path / "missing.txt")])
    assert "no such file" in capsys.readouterr().err
    (tmp_path / "gt.txt").write_text("")
    with pytest.raises(SystemExit):
        cli.main(["--source", "synthetic:2", "--eval-det-gt", str(tmp_path / "gt.txt"), "--eval-det-max-dets", "10", "5"])
    assert "--eval-det-max-dets must be positive and rising" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["--source", "synthetic:2", "--eval-det-max-dets", "1", "10"])
    assert "needs --eval-det-gt" in capsys.readouterr().err


# ---- refusals before the device ----------------------------------------------------------------------------------------------------------
# two classes; class 0: images 0 and 2, class 1: image 1
GOOD = dict(similarity=0, class_cell_off=[0, 2, 3], cell_image=[0, 2, 1], cell_gt_off=[0, 2, 2, 3], cell_det_off=[0, 1, 3, 3],
            gt_boxes=[[0, 0, 10, 10], [20, 0, 30, 10], [0, 0, 5, 5]], gt_crowd=[0, 1, 0], det_boxes=[[0, 0, 10, 10], [0, 0, 5, 5], [9, 9, 12, 12]],
            det_scores=[0.9, 0.8, 0.7], iou_thrs=[0.5, 0.75], rec_thrs=[0.0, 0.5, 1.0], areas=[[0, 1e10], [0, 1024]], max_dets=[1, 10])
INTS = ("class_cell_off", "cell_image", "cell_gt_off", "cell_det_off", "gt_crowd", "max_dets")


def _call(L, null=(), record=False, **change):
    a = {**GOOD, **change}
    v = {k: np.ascontiguousarray(a[k], np.int32 if k in INTS else np.float64) for k in a if k != "similarity"}
    T, R, A, M, K = len(v["iou_thrs"]), len(v["rec_thrs"]), v["areas"].size // 2, len(v["max_dets"]), len(v["class_cell_off"]) - 1
    n = max(int(v["cell_det_off"][-1]), 1)
    outs = dict(precision=np.zeros(max(T * R * K * A * M, 1)), recall=np.zeros(max(T * K * A * M, 1)), det_rank=np.zeros(n, np.int32),
                rec_match=np.zeros(A * T * n, np.int32) if record else None, rec_ignored=np.zeros(A * T * n, np.int32) if record else None)
    v.update(outs)
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    p = lambda k: None if k in null or v[k] is None else v[k].ctypes.data_as(pd if v[k].dtype == np.float64 else pi)
    rc = L.ss_ap_eval(None, int(a["similarity"]), K, len(v["cell_image"]), p("class_cell_off"), p("cell_image"), p("cell_gt_off"), p("cell_det_off"),
                      p("gt_boxes"), p("gt_crowd"), p("det_boxes"), p("det_scores"), T, p("iou_thrs"), R, p("rec_thrs"), A, p("areas"), M, p("max_dets"),
                      p("precision"), p("recall"), p("det_rank"), p("rec_match"), p("rec_ignored"))
    return rc, (L.ss_last_error(None) or b"").decode()


def test_every_argument_refusal_comes_before_the_context():
    lib.build()
    L = lib.load()
    assert deteval.caps() == {"gts": 1024, "cell_dets": 4096, "keep": 1024, "dets": 1 << 22}
    rc, msg = _call(L)
    assert rc == lib.SS_ERR_INVALID and msg == "ss_ap_eval: null context"              # the arguments themselves pass
    assert _call(L, record=True)[1] == "ss_ap_eval: null context" and _call(L, null=("det_rank",))[1] == "ss_ap_eval: null context"
    for k in ("class_cell_off", "cell_image", "cell_gt_off", "cell_det_off", "gt_boxes", "gt_crowd", "det_boxes", "det_scores", "iou_thrs", "rec_thrs",
              "areas", "max_dets", "precision", "recall"):
        rc, msg = _call(L, null=(k,))
        assert rc == lib.SS_ERR_INVALID and "null argument" in msg, k
    rc, msg = _call(L, record=True, null=("rec_ignored",))
    assert rc == lib.SS_ERR_INVALID and "rec_match and rec_ignored come together" in msg
    box = lambda v: [GOOD["gt_boxes"][0], v, GOOD["gt_boxes"][2]]
    cases = [
        (dict(similarity=2), "similarity must be 0 (iou) or 1 (probiou)"),
        (dict(class_cell_off=[1, 2, 3]), "offsets must start at 0"),
        (dict(cell_gt_off=[1, 2, 2, 3]), "offsets must start at 0"),
        (dict(cell_det_off=[1, 1, 3, 3]), "offsets must start at 0"),
        (dict(class_cell_off=[0, 4, 3]), "class 0: cell offsets decrease or pass n_cells"),
        (dict(class_cell_off=[0, 2, 2]), "class_cell_off must end at n_cells"),
        (dict(cell_image=[0, 0, 1]), "class 0: image 0: the images of a class must be non-negative and rising"),
        (dict(cell_image=[0, 2, -1]), "class 1: image -1: the images of a class must be non-negative and rising"),
        (dict(cell_gt_off=[0, 2, 1, 3]), "class 0: image 2: ground-truth row offsets decrease"),
        (dict(cell_det_off=[0, 1, 3, 2]), "class 1: image 1: detection offsets decrease"),
        (dict(gt_boxes=box([20, 0, 20, 10])), "class 0: image 0: a ground-truth box has x2 <= x1 or y2 <= y1"),
        (dict(gt_boxes=box([20, 0, np.nan, 10])), "class 0: image 0: a ground-truth box is NaN or infinite"),
        (dict(det_boxes=[[0, 0, 10, 10], [0, 0, 5, 5], [9, 9, np.inf, 12]]), "class 0: image 2: a detection box is NaN or infinite"),
        (dict(det_boxes=[[0, 0, 10, 10], [0, 0, 5, -5], [9, 9, 12, 12]]), "class 0: image 2: a detection box has x2 <= x1 or y2 <= y1"),
        (dict(det_scores=[0.9, np.nan, 0.7]), "class 0: image 2: a score is NaN or infinite"),
        (dict(gt_crowd=[0, 2, 0]), "class 0: image 0: a crowd flag is neither 0 nor 1"),
        (dict(iou_thrs=[0.5, 0.0]), "iou_thrs must be in (0, 1]"),
        (dict(iou_thrs=[0.5, 1.0000001]), "iou_thrs must be in (0, 1]"),
        (dict(iou_thrs=[np.nan]), "iou_thrs must be in (0, 1]"),
        (dict(rec_thrs=[0.0, np.inf]), "rec_thrs must be finite and must not decrease"),
        (dict(rec_thrs=[0.5, 0.25]), "rec_thrs must be finite and must not decrease"),
        (dict(areas=[[0, 1e10], [5, 1]]), "an area range is not finite or has hi < lo"),
        (dict(max_dets=[1, 1]), "max_dets must be at least 1 and rising"),
        (dict(max_dets=[0, 10]), "max_dets must be at least 1 and rising"),
        (dict(iou_thrs=[]), "a parameter array is empty"),
    ]
    for change, want in cases:
        rc, msg = _call(L, **change)
        assert rc == lib.SS_ERR_INVALID and want in msg, (want, msg)
    five = lambda rows: [[5, 5, r[2] - r[0], r[3] - r[1], 0.1] for r in rows]
    obb = dict(similarity=1, gt_boxes=five(GOOD["gt_boxes"]), det_boxes=five(GOOD["det_boxes"]))
    rc, msg = _call(L, **obb)
    assert rc == lib.SS_ERR_INVALID and "class 0: image 0: a crowd region cannot be scored with probiou" in msg
    assert _call(L, **obb, gt_crowd=[0, 0, 0])[1] == "ss_ap_eval: null context"
    rc, msg = _call(L, **{**obb, "det_boxes": [[5, 5, 0, 3, 0.1]] * 3}, gt_crowd=[0, 0, 0])
    assert rc == lib.SS_ERR_INVALID and "a detection box has w <= 0 or h <= 0" in msg
    assert _call(L, iou_thrs=[1.0])[1] == "ss_ap_eval: null context"


def test_capacities_are_refused_before_the_context_too():
    L = lib.load()
    one = dict(class_cell_off=[0, 1], cell_image=[7])
    rc, msg = _call(L, **one, cell_gt_off=[0, 1025], cell_det_off=[0, 1], gt_boxes=np.tile([0.0, 0, 1, 1], (1025, 1)), gt_crowd=[0] * 1025,
                    det_boxes=[[0, 0, 1, 1]], det_scores=[0.5])
    assert rc == lib.SS_ERR_CAPACITY and "class 0: image 7: 1025 ground-truth rows: at most 1024 a cell" in msg
    rc, msg = _call(L, **one, cell_gt_off=[0, 1], cell_det_off=[0, 4097], gt_boxes=[[0, 0, 1, 1]], gt_crowd=[0],
                    det_boxes=np.tile([0.0, 0, 1, 1], (4097, 1)), det_scores=np.zeros(4097))
    assert rc == lib.SS_ERR_CAPACITY and "class 0: image 7: 4097 detections: at most 4096 a cell" in msg
    assert _call(L, **one, cell_gt_off=[0, 1024], cell_det_off=[0, 4096], gt_boxes=np.tile([0.0, 0, 1, 1], (1024, 1)), gt_crowd=[0] * 1024,
                 det_boxes=np.tile([0.0, 0, 1, 1], (4096, 1)), det_scores=np.zeros(4096), max_dets=[1024])[1] == "ss_ap_eval: null context"
    rc, msg = _call(L, max_dets=[1, 1025])
    assert rc == lib.SS_ERR_CAPACITY and "max_dets 1025: at most 1024" in msg
    for change, want in ((dict(iou_thrs=np.linspace(0.1, 0.9, 17)), "17 thresholds: at most 16"),
                         (dict(areas=[[0, 1]] * 9), "9 area ranges: at most 8"),
                         (dict(max_dets=[1, 2, 3, 4, 5]), "5 max_dets entries: at most 4"),
                         (dict(rec_thrs=np.linspace(0, 1, 1025)), "1025 recall thresholds: at most 1024")):
        rc, msg = _call(L, **change)
        assert rc == lib.SS_ERR_CAPACITY and want in msg, (want, msg)
    # 2^22 + 1 detections in cells of 4096
    n_cells = 1025
    off = np.minimum(np.arange(n_cells + 1) * 4096, (1 << 22) + 1)
    rc, msg = _call(L, class_cell_off=[0, n_cells], cell_image=np.arange(n_cells), cell_gt_off=np.zeros(n_cells + 1), cell_det_off=off,
                    det_boxes=np.tile([0.0, 0, 1, 1], (off[-1], 1)), det_scores=np.zeros(off[-1]))
    assert rc == lib.SS_ERR_CAPACITY and "class 0: image 1024: more than 4194304 detections a call" in msg
