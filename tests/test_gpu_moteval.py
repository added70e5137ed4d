"""HOTA and CLEAR MOT on the MI355X (csrc/ss_mot.hip, docs/MOTEVAL.md) against the CPU restatement (tests/moteval_ref.py), by equality:
match indices as integers, S, GA and every reported float by bytes."""
import json
import os

import numpy as np
import pytest

from strongsort_yolo_amd import cli, gsi, lib, moteval
from tests import moteval_ref as ref
from tests.golden.make_moteval_golden import NAMES, case_rows
from tests.gpu_util import engine

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def eng():
    e = engine(debug=False)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "moteval_cases.npz"))


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape, what
    if a.tobytes() != b.tobytes():
        bad = np.nonzero(a.view(np.int64).ravel() != b.view(np.int64).ravel())[0]
        raise AssertionError(f"{what}: {len(bad)} of {a.size} values differ, first at {bad[0]}: {a.ravel()[bad[0]]!r} != {b.ravel()[bad[0]]!r}")


def _same_metrics(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert type(got[k]) is type(want[k]) and json.dumps(got[k]) == json.dumps(want[k]), f"{what}: {k}: {got[k]!r} != {want[k]!r}"


def _check(eng, gt, trs, thr=0.5, what=""):
    """one device call for all tracker row sets against gt; every pair against the restatement -> the restatement's metrics"""
    got_m, got_r = moteval.evaluate_full(gt, list(trs), eng, thr=thr, want_ga=True)
    out = []
    for k, tr in enumerate(trs):
        m, r = ref.evaluate_full(gt, tr, thr)
        w = f"{what} pair {k}"
        for f in ("hota_idx", "clear_idx"):
            assert got_r[k][f].dtype == np.int32 and got_r[k][f].tolist() == r[f].tolist(), f"{w}: {f}"
        _bits(got_r[k]["hota_s"], r["hota_s"], w + ": hota_s")
        _bits(got_r[k]["clear_s"], r["clear_s"], w + ": clear_s")
        _bits(got_r[k]["GA"], r["GA"], w + ": GA")
        _same_metrics(got_m[k], m, w)
        out.append(m)
    return out


# ---- every path of the matching: the solver's three forms, LDS and scratch, both orientations ---------------------------------------
@pytest.mark.parametrize("nc", [1, 63, 64, 65, 128, 129, 256])
def test_box_counts_at_every_solver_boundary(eng, nc):
    """nc boxes on the column side (the larger one) and nc - nc // 4 on the row side: lsap_wave's forms switch at 64 and 128 columns,
    the matrix leaves the LDS above moteval.LDS_CELLS cells.  One frame and three frames, more ground truth and more tracker boxes,
    and the square case."""
    nr = max(1, nc - nc // 4)
    assert (nc * nr > moteval.LDS_CELLS) == (nc == 256)
    rng = np.random.default_rng(nc)
    for frames in (1, 3):
        for ng, nt in ((nc, nr), (nr, nc), (nc, nc)):
            gt, tr = ref.random_frames(rng, [(ng, nt)] * frames, first_frame=2, step=3)
            m = _check(eng, gt, [tr], what=f"{ng} x {nt}, {frames} frames")[0]
            assert m["frames"] == frames and m["gt_rows"] == ng * frames and m["tracker_rows"] == nt * frames


@pytest.mark.parametrize("name", NAMES)
def test_golden_cases(eng, golden, name):
    gt, tr = case_rows(golden[f"{name}_gt"]), case_rows(golden[f"{name}_tr"])
    m = _check(eng, gt, [tr], what=name)[0]
    _same_metrics(m, json.loads(str(golden[f"{name}_metrics"])), name + " against the file")
    if name == "b256":
        got = moteval.evaluate_full(gt, tr, eng)[1][0]
        assert got["hota_idx"].tolist() == golden["b256_hota_idx"].tolist() and got["clear_idx"].tolist() == golden["b256_clear_idx"].tolist()


# ---- frames with one side only, holes in the frame numbers, CLEAR's tables across them -------------------------------------------
def _row(f, i, x, y=10.0, w=50.0, h=100.0):
    return [f, i, x, y, x + w, y + h, 1.0, 0]


def test_one_sided_frames_holes_and_the_tables_across_them(eng):
    """Ground-truth id 1 is matched to tracker 7 in frames 3 and 4.  Frame 9 has only ground truth, frame 12 only tracker boxes:
    neither is processed, so in frame 20 prev_t[1] is still 7 and the bonus keeps 7 (IoU 0.6...) ahead of the perfectly placed
    tracker 8.  Ground-truth id 2 reappears in frame 20 under tracker 9 after tracker 5: one identity switch."""
    gt = [_row(3, 1, 100), _row(3, 2, 400), _row(4, 1, 100), _row(4, 2, 400), _row(9, 1, 100), _row(9, 2, 400), _row(20, 1, 100), _row(20, 2, 400),
          _row(31, 1, 100)]
    tr = [_row(3, 7, 100), _row(3, 5, 400), _row(4, 7, 104), _row(4, 5, 400), _row(12, 7, 100), _row(12, 5, 400),
          _row(20, 7, 112), _row(20, 8, 100), _row(20, 9, 400), _row(31, 8, 100)]
    m = _check(eng, np.array(gt, np.float64), [np.array(tr, np.float64)], what="one-sided frames")[0]
    assert m["frames"] == 6 and (m["TP"], m["FN"], m["FP"]) == (7, 2, 3)
    assert m["IDSW"] == 2 and m["Frag"] == 0          # 2: 5 -> 9 in frame 20, and 1: 7 -> 8 in frame 31
    # the same with the one-sided frames processed would reset prev_t: drop them and nothing changes, since they touch no table
    keep_g = [r for r in gt if r[0] != 9]
    keep_t = [r for r in tr if r[0] != 12]
    m2 = _check(eng, np.array(keep_g, np.float64), [np.array(keep_t, np.float64)], what="without them")[0]
    assert (m2["IDSW"], m2["TP"], m2["FN"], m2["FP"]) == (2, 7, 0, 1)


def test_a_pair_with_an_empty_side(eng):
    gt = np.array([_row(0, 1, 10), _row(1, 1, 12)], np.float64)
    m = _check(eng, gt, [np.zeros((0, 8)), gt], what="no tracker rows")
    assert (m[0]["TP"], m[0]["FN"], m[0]["HOTA"], m[0]["MOTA"]) == (0, 2, 0.0, 0.0) and m[1]["HOTA"] == 1.0
    m = _check(eng, np.zeros((0, 8)), [gt], what="no ground truth")[0]
    assert (m["TP"], m["FP"], m["HOTA"]) == (0, 2, 0.0)


# ---- exact ties ----------------------------------------------------------------------------------------------------------------
def test_duplicate_tracker_boxes_tie_as_scipy_breaks_them(eng):
    gt, tr = [], []
    for f in range(4):
        for i in range(3):
            gt.append(_row(f, i + 1, 100 + 200 * i))
            for d in range(2 + (f + i) % 2):                      # two or three identical tracker boxes over every ground-truth box
                tr.append(_row(f, 10 * (i + 1) + (d + f) % 3, 100 + 200 * i + 2 * (f % 2)))
    m = _check(eng, np.array(gt, np.float64), [np.array(tr, np.float64)], what="duplicates")[0]
    assert m["TP"] == 12
    # one ground-truth box, 70 and 130 copies: ties across the lanes of the solver's wider forms
    for n in (70, 130):
        one = np.array([_row(0, 1, 100)], np.float64)
        many = np.array([_row(0, k + 1, 100) for k in range(n)], np.float64)
        _check(eng, one, [many], what=f"1 x {n}")
        _check(eng, many, [one], what=f"{n} x 1")


def test_a_clear_frame_whose_score_matrix_is_all_zero(eng):
    gt = np.array([_row(0, 1, 100), _row(0, 2, 300), _row(0, 3, 500), _row(1, 1, 100)], np.float64)
    tr = np.array([_row(0, 1, 130), _row(0, 2, 330), _row(0, 3, 530), _row(0, 4, 900), _row(1, 1, 100)], np.float64)     # IoU 0.25 < 0.5
    m, r = ref.evaluate_full(gt, tr)
    assert r["clear_idx"].tolist() == [-1, -1, -1, 0] and (r["hota_idx"] >= 0).all() and (r["hota_s"][:3] == 0.25).all()
    got = _check(eng, gt, [tr], what="zero scores")[0]
    assert (got["TP"], got["FN"], got["FP"]) == (1, 3, 4)
    assert _check(eng, gt, [tr], thr=0.25, what="thr 0.25")[0]["TP"] == 4


# ---- several pairs a call, scratch -----------------------------------------------------------------------------------------------
def test_four_pairs_in_one_call_equal_four_calls_and_scratch_is_reused(eng, golden):
    gt = case_rows(golden["id30_gt"])
    base = case_rows(golden["id30_tr"])
    rng = np.random.default_rng(4)
    trs = [base, gt.copy(), ref.perturb(gt, rng, 7, 0.2, 3.0, 1.0), base[base[:, 0] % 2 == 0]]
    whole = moteval.evaluate_full(gt, trs, eng, want_ga=True)
    again = moteval.evaluate_full(gt, trs, eng, want_ga=True)
    for k, tr in enumerate(trs):
        alone = moteval.evaluate_full(gt, [tr], eng, want_ga=True)
        for other, what in ((alone, "alone"), (again, "the same call again")):
            o = 0 if other is alone else k
            _same_metrics(whole[0][k], other[0][o], f"pair {k} {what}")
            for f in ("hota_idx", "clear_idx", "hota_s", "clear_s", "GA"):
                assert whole[1][k][f].tobytes() == other[1][o][f].tobytes(), (k, f, what)
    _check(eng, gt, trs, what="four pairs")
    assert whole[0][1]["HOTA"] == 1.0 and whole[0][1]["IDSW"] == 0


def test_257_boxes_are_a_capacity_error_and_the_context_lives_on(eng):
    rng = np.random.default_rng(257)
    gt, tr = ref.random_frames(rng, [(5, 5), (257, 4)])
    with pytest.raises(lib.SSError, match=r"pair 0: frame 1: 257 ground-truth boxes") as e:
        moteval.evaluate(gt, tr, eng)
    assert e.value.code == lib.SS_ERR_CAPACITY
    gt, tr = ref.random_frames(rng, [(5, 5), (4, 257)])
    with pytest.raises(lib.SSError, match=r"pair 1: frame 1: 257 tracker boxes") as e:
        moteval.evaluate(gt, [gt, tr], eng)
    assert e.value.code == lib.SS_ERR_CAPACITY
    gt, tr = ref.random_frames(rng, [(5, 7), (7, 5)])
    _check(eng, gt, [tr], what="after the refusals")
    eng.check_errors()
    assert moteval.max_boxes() == 256


def test_evaluate_with_a_class_filter(eng):
    rng = np.random.default_rng(8)
    gt, tr = ref.random_frames(rng, [(12, 9)] * 5)
    gt[::3, 7], tr[::2, 7] = 2.0, 2.0
    got = moteval.evaluate(gt, tr, eng, classes=[2])
    assert isinstance(got, list) and len(got) == 1
    _same_metrics(got[0], ref.evaluate(gt[gt[:, 7] == 2], tr[tr[:, 7] == 2]), "classes=[2]")
    with pytest.raises(ValueError, match="IDF1"):
        moteval.evaluate(gt, tr, eng, metrics=("HOTA", "IDF1"))


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def test_cli_scores_the_labels_and_the_gsi_labels_in_one_metrics_file(tmp_path):
    from strongsort_yolo_amd.yolo import YOLO
    z = np.load(os.path.join(GOLD, "jpeg_sequence.npz"))
    src = tmp_path / "seq.npy"
    np.save(src, np.stack([np.ascontiguousarray(z[f"rgb_{i}"][:, :, ::-1]) for i in range(12)]))
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack")
    base = {"source": str(src), "track": True, "count": False, "tracker": "bytetrack", "batch": 4, "random_init": True}
    cli.process_video({**base, "outdir": str(tmp_path / "a")}, model=model)
    rows = moteval.read_labels(str(tmp_path / "a" / "seq_labels.txt"))
    assert len(rows) and not (tmp_path / "a" / "seq_metrics.json").exists()
    rng = np.random.default_rng(0)
    truth = rows[rng.random(len(rows)) >= 0.2]                    # the ground truth: the tracker's own rows, a fifth of them missing, moved by 2 px
    truth[:, 2:6] += 2.0
    gsi.write_labels(str(tmp_path / "gt.txt"), truth)
    outs = {}
    for run, extra in (("b", {}), ("c", {"gsi": True})):
        model._stream_pipe.reset_tracker(-1)
        model._frame_index = 0
        outs[run] = cli.process_video({**base, "outdir": str(tmp_path / run), "eval_gt": str(tmp_path / "gt.txt"), **extra}, model=model)
    model.close()
    assert (tmp_path / "b" / "seq_labels.txt").read_bytes() == (tmp_path / "a" / "seq_labels.txt").read_bytes()
    want = ref.evaluate(truth, rows)
    one = json.loads((tmp_path / "b" / "seq_metrics.json").read_text())
    _same_metrics(one, want, "labels")
    both = json.loads((tmp_path / "c" / "seq_metrics.json").read_text())
    assert sorted(both) == ["labels", "labels_gsi"]
    _same_metrics(both["labels"], want, "labels beside gsi")
    want_gsi = ref.evaluate(truth, moteval.read_labels(str(tmp_path / "c" / "seq_labels_gsi.txt")))
    _same_metrics(both["labels_gsi"], want_gsi, "labels_gsi")
    assert (outs["b"]["HOTA"], outs["b"]["MOTA"], outs["b"]["IDSW"]) == (want["HOTA"], want["MOTA"], want["IDSW"]) and "HOTA_gsi" not in outs["b"]
    assert (outs["c"]["HOTA_gsi"], outs["c"]["MOTA_gsi"], outs["c"]["IDSW_gsi"]) == (want_gsi["HOTA"], want_gsi["MOTA"], want_gsi["IDSW"])
    assert 0.0 < want["HOTA"] < 1.0 and want["FP"] > 0
