"""HOTA and CLEAR MOT on the CPU (docs/MOTEVAL.md): the restatement tests/moteval_ref.py against closed forms and against a second,
vectorised statement written here; the host half of strongsort_yolo_amd.moteval (dense ids, packing, the figures from the per-row
record) against the restatement, fed by a stand-in engine that answers with the restatement's record; the labels reader; and every
refusal ss_mot_eval makes before it looks at a context or the device."""
import ctypes as C
import json
import os

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from strongsort_yolo_amd import cli, gsi, lib, moteval
from tests import moteval_ref as ref
from tests.golden.make_moteval_golden import NAMES, case_rows, make_case, to_file

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# Largest difference of any float between the restatement (sequential sums) and the vectorised statement (np.sum, whole-matrix IoU)
# over the golden cases, measured: 3.8e-15 (docs/MOTEVAL.md §6).  The bound is ten times that: other NumPy builds block np.sum differently.
MEASURED_SUM_ORDER = 3.8e-15
SUM_ORDER_BOUND = 10 * MEASURED_SUM_ORDER


def _row(f, i, x, y=10.0, w=50.0, h=100.0):
    return [f, i, x, y, x + w, y + h, 1.0, 0]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "moteval_cases.npz"))


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
def test_a_sequence_against_itself_is_perfect(golden):
    gt = case_rows(golden["id30_gt"])
    m = ref.evaluate(gt, gt)
    assert m["HOTA"] == m["DetA"] == m["AssA"] == m["LocA"] == 1.0 and m["MOTA"] == 1.0 and m["IDSW"] == 0
    assert m["HOTA(0)"] == m["LocA(0)"] == 1.0 and m["MOTP"] == 1.0 and (m["FN"], m["FP"]) == (0, 0) and m["MT"] == m["gt_ids"]


def test_a_consistent_renaming_of_the_tracker_ids_changes_nothing(golden):
    gt, tr = case_rows(golden["id30_gt"]), case_rows(golden["id30_tr"])
    ids = np.unique(tr[:, 1])
    new = dict(zip(ids, np.random.default_rng(0).permutation(len(ids)) * 7 + 5000))
    tr2 = tr.copy()
    tr2[:, 1] = [new[i] for i in tr[:, 1]]
    (a, ra), (b, rb) = ref.evaluate_full(gt, tr), ref.evaluate_full(gt, tr2)

    def named(rec, which):
        """the matching as (frame, ground-truth id, tracker id by its ORIGINAL name).  HOTA assigns every row of the smaller side, so
        a box that overlaps nothing is given one of several columns of score exactly 0: which one follows the column order, and no
        threshold counts it (S = 0).  Those are left out; every match with S > 0 is compared."""
        p, idx = rec["pair"], rec[which]
        frame_of = np.repeat(np.arange(len(p.frames)), np.diff(p.gt_off))
        sel = (idx >= 0) & (rec[which.replace("idx", "s")] > 0)
        names = p.tr[p.tr_off[frame_of[sel]] + idx[sel], 1]
        return sorted(zip(p.gt[sel, 0].tolist(), p.gt[sel, 1].tolist(), names.tolist()))

    back = {v: k for k, v in new.items()}
    for which in ("hota_idx", "clear_idx"):
        assert named(ra, which) == [(f, g, back[t]) for f, g, t in named(rb, which)], which      # the same matching, frame by frame
    # (the dense ids follow the names' order, so the sums over id pairs run in another order: integers equal, floats to rounding)
    for k in a:
        if isinstance(a[k], int):
            assert a[k] == b[k], k
        else:
            assert np.allclose(a[k], b[k], rtol=0, atol=1e-14), k
    keep = dict(zip(ids, ids * 3 + 11))                          # an order-preserving renaming: identical bits
    tr3 = tr.copy()
    tr3[:, 1] = [keep[i] for i in tr[:, 1]]
    assert json.dumps(ref.evaluate(gt, tr3)) == json.dumps(a)


def test_two_tracks_whose_tracker_ids_swap_at_the_midpoint():
    n = 20
    gt = [_row(f, i + 1, 10 + 300 * i) for f in range(n) for i in range(2)]
    tr = [_row(f, (i if f < n // 2 else 1 - i) + 1, 10 + 300 * i) for f in range(n) for i in range(2)]
    m = ref.evaluate(gt, tr)
    assert m["DetA"] == 1.0 and abs(m["AssA"] - 1 / 3) < 1e-15 and abs(m["HOTA"] - np.sqrt(1 / 3)) < 1e-15
    assert m["IDSW"] == 2 and m["MOTA"] == 1 - 2 / (2 * n) and m["Frag"] == 0


def test_dropping_one_tracker_id_lowers_recall_only(golden):
    gt = case_rows(golden["id6_gt"])
    tr = gt[gt[:, 1] != gt[0, 1]]
    full, m = ref.evaluate(gt, gt), ref.evaluate(gt, tr)
    assert m["DetRe"] < full["DetRe"] == 1.0 and m["DetPr"] == 1.0 and m["FP"] == 0 and m["FN"] == len(gt) - len(tr) and m["ML"] == 1


def test_refused_rows():
    good = np.array([_row(0, 1, 10), _row(1, 1, 10)], np.float64)
    for bad, what in ((np.array([_row(0, 1, 10), _row(0, 1, 30)]), "duplicate"), (np.array([_row(0, 1, 10, w=0.0)]), "x2 <= x1"),
                      (np.array([_row(0, 1, 10, h=-1.0)]), "y2 <= y1"), (np.array([_row(0, 1, np.nan)]), "NaN"), (np.array([_row(0, 1, np.inf)]), "NaN")):
        for f in (lambda: ref.evaluate(good, bad), lambda: ref.evaluate(bad, good), lambda: moteval.evaluate(good, bad, None), lambda: moteval.evaluate(bad, good, None)):
            with pytest.raises(ValueError, match=what):
                f()


# ---- the restatement against a second, vectorised statement ------------------------------------------------------------------------
def _vectorised(gt, tr, thr=0.5):
    """HOTA and CLEAR as one would write them with whole-matrix operations and np.sum -> (integers, floats)"""
    gt, tr = gt[np.lexsort((gt[:, 1], gt[:, 0]))], tr[np.lexsort((tr[:, 1], tr[:, 0]))]
    gid, tid = np.unique(gt[:, 1], return_inverse=True)[1].reshape(-1), np.unique(tr[:, 1], return_inverse=True)[1].reshape(-1)
    nG, nT = gid.max() + 1, tid.max() + 1
    frames = np.union1d(gt[:, 0], tr[:, 0])
    per, pot = [], np.zeros((nG, nT))
    for f in frames:
        a, b = np.nonzero(gt[:, 0] == f)[0], np.nonzero(tr[:, 0] == f)[0]
        A, B = gt[a, 2:6], tr[b, 2:6]
        wh = np.clip(np.minimum(A[:, None, 2:], B[None, :, 2:]) - np.maximum(A[:, None, :2], B[None, :, :2]), 0, None)
        inter = wh[..., 0] * wh[..., 1]
        S = inter / (np.prod(A[:, 2:] - A[:, :2], 1)[:, None] + np.prod(B[:, 2:] - B[:, :2], 1)[None, :] - inter)
        per.append((a, b, S))
        if S.size:
            den = S.sum(0)[None, :] + S.sum(1)[:, None] - S
            pot[gid[a][:, None], tid[b][None, :]] += np.where(den > ref.EPS, S / np.maximum(den, ref.EPS), 0)
    cg, ct = np.bincount(gid, minlength=nG), np.bincount(tid, minlength=nT)
    GA = pot / (cg[:, None] + ct[None, :] - pot)
    hg, ht, hs = [], [], []
    cl_g, cl_t, cl_s, idsw = [], [], [], 0
    prev, prev_t = np.full(nG, -1), np.full(nG, -1)
    for a, b, S in per:
        if not S.size:
            continue
        r, c = linear_sum_assignment(-(GA[gid[a][:, None], tid[b][None, :]] * S))
        hg += list(gid[a][r]); ht += list(tid[b][c]); hs += list(S[r, c])
        sc = 1000.0 * (tid[b][None, :] == prev_t[gid[a]][:, None]) + S
        sc[S < thr - ref.EPS] = 0
        r, c = linear_sum_assignment(-sc)
        ok = sc[r, c] > ref.EPS
        g, t = gid[a][r[ok]], tid[b][c[ok]]
        idsw += np.sum((prev[g] >= 0) & (prev[g] != t))
        prev[g] = t
        prev_t[:] = -1
        prev_t[g] = t
        cl_g += list(g); cl_t += list(t); cl_s += list(S[r[ok], c[ok]])
    hg, ht, hs = np.array(hg, np.int64), np.array(ht, np.int64), np.array(hs)
    ints, floats = {}, {k: [] for k in ref.HOTA_FIELDS}
    for alpha in ref.ALPHAS:
        m = hs >= alpha - ref.EPS
        tp = int(m.sum())
        fn, fp = len(gt) - tp, len(tr) - tp
        c = np.zeros((nG, nT))
        np.add.at(c, (hg[m], ht[m]), 1)
        ass = [np.sum(c * c / np.maximum(1, d)) / max(1, tp) for d in (cg[:, None] + ct[None, :] - c, cg[:, None] + 0 * c, ct[None, :] + 0 * c)]
        det_a = tp / max(1, tp + fn + fp)
        for k, v in zip(ref.HOTA_FIELDS, (np.sqrt(det_a * ass[0]), det_a, ass[0], tp / max(1, tp + fn), tp / max(1, tp + fp), ass[1], ass[2],
                                          max(1e-10, np.sum(hs[m])) / max(1e-10, tp))):
            floats[k].append(float(v))
        ints.setdefault("TP_alpha", []).append(tp)
    out_f = {k + "_alpha": v for k, v in floats.items()}
    out_f.update({k: float(np.mean(v)) for k, v in floats.items()})
    tp = len(cl_g)
    ints.update(TP=tp, FN=len(gt) - tp, FP=len(tr) - tp, IDSW=int(idsw), hota_pairs=sorted(zip(hg.tolist(), ht.tolist())), clear_pairs=sorted(zip(cl_g, cl_t)))
    out_f.update(MOTA=(tp - (len(tr) - tp) - idsw) / max(1, len(gt)), MOTP=float(np.sum(cl_s)) / max(1, tp))
    return ints, out_f


def test_restatement_against_the_vectorised_statement(golden):
    """Every integer and every matching equal; the floats differ by summation order only.  Measured over the golden cases: the
    largest difference is MEASURED_SUM_ORDER; the bound is ten times that."""
    worst = 0.0
    for name in NAMES:
        gt, tr = case_rows(golden[f"{name}_gt"]), case_rows(golden[f"{name}_tr"])
        m, rec = ref.evaluate_full(gt, tr)
        ints, floats = _vectorised(gt, tr)
        p = rec["pair"]
        frame_of = np.repeat(np.arange(len(p.frames)), np.diff(p.gt_off))
        for which, key in (("hota_idx", "hota_pairs"), ("clear_idx", "clear_pairs")):
            sel = rec[which] >= 0
            pairs = sorted(zip(p.gt_id[sel].tolist(), p.tr_id[p.tr_off[frame_of[sel]] + rec[which][sel]].tolist()))
            assert pairs == ints[key], f"{name}: the {which} matching differs"
        assert (m["TP"], m["FN"], m["FP"], m["IDSW"]) == (ints["TP"], ints["FN"], ints["FP"], ints["IDSW"]), name
        assert [round(d * (m["gt_rows"] + m["tracker_rows"]) / (1 + d)) for d in m["DetA_alpha"]] == ints["TP_alpha"], name
        for k, v in floats.items():
            d = float(np.abs(np.asarray(m[k]) - np.asarray(v)).max())
            worst = max(worst, d)
            assert d <= SUM_ORDER_BOUND, (name, k, d)
    print(f"moteval_ref vs the vectorised statement: largest difference {worst:.3e}")


def test_golden_file_is_what_the_restatement_computes(golden):
    assert os.path.getsize(os.path.join(GOLD, "moteval_cases.npz")) < 200_000
    for name in NAMES:
        gt, tr = make_case(name)
        assert golden[f"{name}_gt"].tolist() == to_file(gt).tolist() and golden[f"{name}_tr"].tolist() == to_file(tr).tolist(), name
        m, rec = ref.evaluate_full(case_rows(golden[f"{name}_gt"]), case_rows(golden[f"{name}_tr"]))
        assert json.dumps(m) == str(golden[f"{name}_metrics"]), name
        if name in ("more_tr", "b256"):
            assert rec["hota_idx"].tolist() == golden[f"{name}_hota_idx"].tolist() and rec["clear_idx"].tolist() == golden[f"{name}_clear_idx"].tolist()
    m = {n: json.loads(str(golden[f"{n}_metrics"])) for n in NAMES}
    assert m["id6"]["HOTA"] == 1.0 and m["id6"]["IDSW"] == 0
    assert 0.6 < m["id30"]["HOTA"] < 0.72 and m["id30"]["IDSW"] == 16 and 0.42 < m["id100"]["HOTA"] < 0.52 and 40 <= m["id100"]["IDSW"] <= 80
    p = ref.Pair(case_rows(golden["more_tr_gt"]), case_rows(golden["more_tr_tr"]))
    assert (np.diff(p.tr_off) > np.diff(p.gt_off)).all(), "more tracker than ground-truth boxes in every frame"
    p = ref.Pair(case_rows(golden["b256_gt"]), case_rows(golden["b256_tr"]))
    assert np.diff(p.gt_off).tolist() == [256] * 3 == np.diff(p.tr_off).tolist()


# ---- the module's host half, fed with the restatement's record -------------------------------------------------------------------------
class RecordEngine:
    """Stands in for TrackerEngine.mot_eval: unpacks the call into rows again and answers with the restatement's record."""

    def __init__(self):
        self.calls = 0

    def mot_eval(self, frame_off, gt_off, tr_off, gt_ids, tr_ids, gt_boxes, tr_boxes, n_gt_ids, n_tr_ids, thr=0.5, want_ga=False):
        self.calls += 1
        assert gt_off[0] == 0 and tr_off[0] == 0 and (np.diff(gt_off) >= 0).all() and (np.diff(tr_off) >= 0).all() and len(gt_off) == frame_off[-1] + 1
        hi, hs, ci, cs, ga = [], [], [], [], []
        for p in range(len(frame_off) - 1):
            f0, f1 = frame_off[p], frame_off[p + 1]
            sides = []
            for off, ids, boxes, n in ((gt_off, gt_ids, gt_boxes, n_gt_ids[p]), (tr_off, tr_ids, tr_boxes, n_tr_ids[p])):
                a, b = off[f0], off[f1]
                r = np.zeros((b - a, 8))
                r[:, 0] = np.repeat(np.arange(f1 - f0), np.diff(off[f0:f1 + 1]))
                r[:, 1], r[:, 2:6] = ids[a:b], boxes[a:b]
                assert b == a or (ids[a:b].min() >= 0 and ids[a:b].max() == n - 1)
                sides.append(r)
            rec = ref.evaluate_full(sides[0], sides[1], thr)[1]
            hi.append(rec["hota_idx"]); hs.append(rec["hota_s"]); ci.append(rec["clear_idx"]); cs.append(rec["clear_s"]); ga.append(rec["GA"].ravel())
        cat = lambda v, dt: np.concatenate(v).astype(dt)
        return (cat(hi, np.int32), cat(hs, np.float64), cat(ci, np.int32), cat(cs, np.float64)) + ((cat(ga, np.float64),) if want_ga else ())


def test_module_host_half_equals_the_restatement(golden):
    eng = RecordEngine()
    gt = case_rows(golden["id30_gt"])
    trs = [case_rows(golden["id30_tr"]), gt.copy(), gt[gt[:, 0] % 3 != 1], np.zeros((0, 8))]
    got, rec = moteval.evaluate_full(gt[np.random.default_rng(0).permutation(len(gt))], trs, eng, want_ga=True)      # any row order
    assert eng.calls == 1 and len(got) == 4
    for k, tr in enumerate(trs):
        want, wrec = ref.evaluate_full(gt, tr)
        assert json.dumps(got[k]) == json.dumps(want), k
        assert rec[k]["GA"].tobytes() == wrec["GA"].tobytes() and rec[k]["GA"].shape == wrec["GA"].shape
    for name in ("id100", "more_tr", "b256", "id6"):
        gt, tr = case_rows(golden[f"{name}_gt"]), case_rows(golden[f"{name}_tr"])
        assert json.dumps(moteval.evaluate(gt, tr, eng)[0]) == str(golden[f"{name}_metrics"]), name
    # holes, one-sided frames, Frag and IDSW replayed from the record
    gt = np.array([_row(3, 1, 100), _row(4, 1, 100), _row(9, 1, 100), _row(20, 1, 100), _row(21, 1, 100), _row(22, 1, 100), _row(23, 1, 100)])
    tr = np.array([_row(3, 7, 100), _row(4, 7, 100), _row(12, 7, 100), _row(20, 7, 300), _row(21, 8, 100), _row(22, 7, 300), _row(23, 7, 100)])
    want = ref.evaluate(gt, tr)
    assert (want["IDSW"], want["Frag"], want["TP"]) == (2, 2, 4)
    assert json.dumps(moteval.evaluate(gt, tr, eng)[0]) == json.dumps(want)
    assert moteval.evaluate(gt, [], eng) == []
    with pytest.raises(ValueError, match="IDF1"):
        moteval.evaluate(gt, tr, eng, metrics=["IDF1"])
    got = moteval.evaluate(np.concatenate([gt, np.array([_row(3, 2, 500)[:7] + [5]])]), tr, eng, classes=[0])[0]
    assert json.dumps(got) == json.dumps(want)


# ---- labels, metrics file, parser ----------------------------------------------------------------------------------------------------
def test_read_labels_round_trips_both_writers(tmp_path):
    import torch
    from strongsort_yolo_amd.yolo import Boxes, Results
    rows = np.array([[3, 12, 10.9, 20.2, 110.7, 220.999, 0.87654, 2], [4, 12, -0.5, 20.0, 99.5, 100.0, 0.0, 0]])
    gsi.write_labels(str(tmp_path / "g.txt"), rows)
    got = moteval.read_labels(str(tmp_path / "g.txt"))
    assert got.dtype == np.float64 and got.tolist() == [[3, 12, 10, 20, 110, 220, 0.877, 2], [4, 12, 0, 20, 99, 100, 0.0, 0]]
    w = cli.LabelsWriter(str(tmp_path / "w.txt"))
    b = Boxes(torch.tensor([[1.5, 2.25, 30.75, 40.5], [5.0, 6.0, 7.0, 8.0]]), torch.tensor([0.5, 0.25]), torch.tensor([0.0, 3.0]), torch.tensor([7.0, 9.0]))
    assert w.write(11, [Results(None, {}, b)]) == 2
    w.close()
    assert moteval.read_labels(str(tmp_path / "w.txt")).tolist() == [[11, 7, 1, 2, 30, 40, 0.5, 0], [11, 9, 5, 6, 7, 8, 0.25, 3]]
    (tmp_path / "e.txt").write_text("")
    assert moteval.read_labels(str(tmp_path / "e.txt")).shape == (0, 8)
    (tmp_path / "bad.txt").write_text("1 2 3\n")
    with pytest.raises(ValueError, match="bad.txt:1"):
        moteval.read_labels(str(tmp_path / "bad.txt"))
    moteval.write_metrics(str(tmp_path / "m.json"), {"HOTA": 0.5, "HOTA_alpha": [0.1, 0.2], "IDSW": 3})
    assert json.loads((tmp_path / "m.json").read_text()) == {"HOTA": 0.5, "HOTA_alpha": [0.1, 0.2], "IDSW": 3}


def test_eval_gt_without_track_is_a_parser_error(capsys, tmp_path):
    with pytest.raises(SystemExit):
        cli.main(["--source", "synthetic:2", "--eval-gt", "gt.txt"])
    err = capsys.readouterr().err
    assert "--eval-gt" in err and "--track" in err
    with pytest.raises(SystemExit):
        cli.main(["--source", "synthetic:2", "synthetic:3", "--track", "--eval-gt", "gt.txt"])
    assert "one ground-truth file per --source" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["--source", "synthetic:2", "--track", "--eval-gt", str(tmp_path / "missing.txt")])
    assert "no such file" in capsys.readouterr().err and "missing.txt" not in os.listdir(tmp_path)
    (tmp_path / "gt.txt").write_text("")
    with pytest.raises(SystemExit):
        cli.main(["--source", "synthetic:2", "--track", "--eval-gt", str(tmp_path / "gt.txt"), "--eval-thr", "0"])
    assert "--eval-thr must be in (0, 1]" in capsys.readouterr().err


# ---- refusals before the device ----------------------------------------------------------------------------------------------------------
GOOD = dict(frame_off=[0, 2, 3], gt_off=[0, 2, 3, 4], tr_off=[0, 1, 1, 3], gt_ids=[0, 1, 1, 0], tr_ids=[0, 1, 0],
            gt_boxes=[[0, 0, 10, 10], [20, 0, 30, 10], [20, 0, 30, 10], [0, 0, 5, 5]], tr_boxes=[[0, 0, 10, 10], [0, 0, 5, 5], [9, 9, 12, 12]],
            n_gt_ids=[2, 1], n_tr_ids=[1, 2], thr=0.5)
ORDER = ("frame_off", "gt_off", "tr_off", "gt_ids", "tr_ids", "gt_boxes", "tr_boxes", "n_gt_ids", "n_tr_ids")


def _call(L, null=None, **change):
    a = {**GOOD, **change}
    arrs = [np.ascontiguousarray(a[k], np.float64 if k.endswith("boxes") else np.int32) for k in ORDER]
    n = max(len(arrs[3]), 1)
    outs = [np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.int32), np.zeros(n)]
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    args = [v.ctypes.data_as(pd if v.dtype == np.float64 else pi) for v in arrs] + [float(a["thr"])] + [v.ctypes.data_as(pd if v.dtype == np.float64 else pi) for v in outs] + [None]
    if null is not None:
        args[null] = None
    rc = L.ss_mot_eval(None, len(arrs[0]) - 1, *args)
    return rc, (L.ss_last_error(None) or b"").decode()


def test_every_argument_refusal_comes_before_the_context():
    lib.build()
    L = lib.load()
    assert L.ss_mot_max_boxes() == 256 == moteval.MAX_BOXES == ref.MAX_BOXES == moteval.max_boxes()
    rc, msg = _call(L)
    assert rc == lib.SS_ERR_INVALID and msg == "ss_mot_eval: null context"            # the arguments themselves pass
    for null in list(range(9)) + [10, 11, 12, 13]:
        rc, msg = _call(L, null=null)
        assert rc == lib.SS_ERR_INVALID and "null argument" in msg, null
    box = lambda v: [GOOD["gt_boxes"][0], v] + GOOD["gt_boxes"][2:]
    cases = [
        (dict(frame_off=[1, 2, 3]), "offsets must start at 0"),
        (dict(gt_off=[1, 2, 3, 4]), "offsets must start at 0"),
        (dict(tr_off=[1, 1, 1, 3]), "offsets must start at 0"),
        (dict(frame_off=[0, 4, 3]), "pair 1: frame offsets decrease"),
        (dict(gt_off=[0, 2, 1, 4]), "pair 0: frame 1: ground-truth row offsets decrease"),
        (dict(tr_off=[0, 1, 3, 2]), "pair 1: frame 0: tracker row offsets decrease"),
        (dict(gt_ids=[0, 2, 1, 0]), "pair 0: frame 0: a ground-truth id is out of range"),
        (dict(gt_ids=[0, -1, 1, 0]), "pair 0: frame 0: a ground-truth id is out of range"),
        (dict(tr_ids=[0, 1, 2]), "pair 1: frame 0: a tracker id is out of range"),
        (dict(gt_ids=[1, 1, 1, 0]), "pair 0: frame 0: a ground-truth id appears twice"),
        (dict(tr_ids=[0, 1, 1]), "pair 1: frame 0: a tracker id appears twice"),
        (dict(gt_boxes=box([20, 0, 20, 10])), "pair 0: frame 0: a ground-truth box has x2 <= x1 or y2 <= y1"),
        (dict(gt_boxes=box([20, 0, 30, -1])), "pair 0: frame 0: a ground-truth box has x2 <= x1 or y2 <= y1"),
        (dict(gt_boxes=box([20, 0, np.nan, 10])), "pair 0: frame 0: a ground-truth box is NaN or infinite"),
        (dict(gt_boxes=box([-np.inf, 0, 30, 10])), "pair 0: frame 0: a ground-truth box is NaN or infinite"),
        (dict(tr_boxes=[[0, 0, 10, 10], [0, 0, 5, 5], [9, 9, np.inf, 12]]), "pair 1: frame 0: a tracker box is NaN or infinite"),
        (dict(n_gt_ids=[2, -1]), "pair 1: an id count is negative"),
        (dict(n_gt_ids=[4, 1]), "pair 0: more ids than rows"),
        (dict(n_tr_ids=[1, 3]), "pair 1: more ids than rows"),
        (dict(n_gt_ids=[2 ** 31 - 1, 1], n_tr_ids=[0, 2]), "pair 0: more ids than rows"),      # (not an allocation of gigabytes)
    ]
    for change, want in cases:
        rc, msg = _call(L, **change)
        assert rc == lib.SS_ERR_INVALID and want in msg, (want, msg)
    for thr in (0.0, -0.5, 1.0000001, np.nan, np.inf):
        rc, msg = _call(L, thr=thr)
        assert rc == lib.SS_ERR_INVALID and "thr must be in (0, 1]" in msg, thr
    assert _call(L, thr=1.0)[1] == "ss_mot_eval: null context"
    z = np.zeros(8, np.int32)
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    zi, zd = z.ctypes.data_as(pi), z.ctypes.data_as(pd)
    assert L.ss_mot_eval(None, 0, zi, zi, zi, zi, zi, zd, zd, zi, zi, 0.5, zi, zd, zi, zd, None) == lib.SS_ERR_INVALID
    assert b"n_pairs must be at least 1" in L.ss_last_error(None)


def test_capacities_are_refused_before_the_context_too():
    L = lib.load()
    rc, msg = _call(L, frame_off=[0, 1], gt_off=[0, 257], tr_off=[0, 1], gt_ids=list(range(257)), tr_ids=[0], gt_boxes=[[0, 0, 1, 1]] * 257,
                    tr_boxes=[[0, 0, 1, 1]], n_gt_ids=[257], n_tr_ids=[1])
    assert rc == lib.SS_ERR_CAPACITY and "pair 0: frame 0: 257 ground-truth boxes: at most 256 a frame" in msg
    rc, msg = _call(L, frame_off=list(range(66)), gt_off=[0] * 66, tr_off=[0] * 66, gt_ids=[], tr_ids=[], gt_boxes=np.zeros((1, 4)), tr_boxes=np.zeros((1, 4)),
                    n_gt_ids=[0] * 65, n_tr_ids=[0] * 65)
    assert rc == lib.SS_ERR_CAPACITY and "65 pairs: at most 64 a call" in msg
    rc, msg = _call(L, frame_off=[0, 65537], gt_off=[0] * 65538, tr_off=[0] * 65538, gt_ids=[], tr_ids=[], gt_boxes=np.zeros((1, 4)), tr_boxes=np.zeros((1, 4)),
                    n_gt_ids=[0], n_tr_ids=[0])
    assert rc == lib.SS_ERR_CAPACITY and "pair 0: 65537 frames: at most 65536 a pair" in msg
    # 64 frames of 256 ground-truth and 65 tracker boxes, every id once: 16 384 x 4 160 id cells are more than 2^26
    ng, nt = 64 * 256, 64 * 65
    rc, msg = _call(L, frame_off=[0, 64], gt_off=np.arange(65) * 256, tr_off=np.arange(65) * 65, gt_ids=np.arange(ng), tr_ids=np.arange(nt),
                    gt_boxes=np.tile([0.0, 0, 1, 1], (ng, 1)), tr_boxes=np.tile([0.0, 0, 1, 1], (nt, 1)), n_gt_ids=[ng], n_tr_ids=[nt])
    assert rc == lib.SS_ERR_CAPACITY and f"{ng * nt} ground-truth id x tracker id cells: at most 67108864 a call" in msg
    # 2 049 frames of 256 x 256 boxes are 2^27 + 65 536 box x box cells
    F, n = 2049, 2049 * 256
    rc, msg = _call(L, frame_off=[0, F], gt_off=np.arange(F + 1) * 256, tr_off=np.arange(F + 1) * 256, gt_ids=np.tile(np.arange(256), F),
                    tr_ids=np.tile(np.arange(256), F), gt_boxes=np.tile([0.0, 0, 1, 1], (n, 1)), tr_boxes=np.tile([0.0, 0, 1, 1], (n, 1)),
                    n_gt_ids=[256], n_tr_ids=[256])
    assert rc == lib.SS_ERR_CAPACITY and f"{F * 65536} box x box cells: at most 134217728 a call" in msg
    rc, msg = _call(L, frame_off=[0, F - 1], gt_off=np.arange(F) * 256, tr_off=np.arange(F) * 256, gt_ids=np.tile(np.arange(256), F - 1),
                    tr_ids=np.tile(np.arange(256), F - 1), gt_boxes=np.tile([0.0, 0, 1, 1], (n - 256, 1)), tr_boxes=np.tile([0.0, 0, 1, 1], (n - 256, 1)),
                    n_gt_ids=[256], n_tr_ids=[256])
    assert rc == lib.SS_ERR_INVALID and msg == "ss_mot_eval: null context"             # exactly 2^27 cells pass the checks
    # the constants moteval.py names are the kernel file's own
    import re
    src = open(os.path.join(lib.CSRC, "ss_mot.hip")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (MOT_[A-Z_]+) (\d+)\b", src, flags=re.M)}
    assert (defs["MOT_MAX_BOXES"], defs["MOT_LDS_CELLS"]) == (moteval.MAX_BOXES, moteval.LDS_CELLS)
