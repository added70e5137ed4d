"""The identity metrics on the MI355X (k_id_count and k_id_solve of csrc/ss_mot.hip, docs/MOTEVAL.md §1 "Identity") against
tests/identity_ref.py, by equality: the counts as integers against pot_of, IDTP / IDFN / IDFP against SciPy on the reduction, the
floats by json.dumps.  The optimum weight is unique; the matching that reaches it is not, and is checked by its properties."""
import json
import os

import numpy as np
import pytest

from strongsort_yolo_amd import cli, gsi, lib, moteval
from tests import identity_ref as iref
from tests import moteval_ref as ref
from tests.golden.make_moteval_golden import NAMES, case_rows
from tests.gpu_util import engine

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIX = ("IDTP", "IDFN", "IDFP", "IDF1", "IDP", "IDR")


@pytest.fixture(scope="module")
def eng():
    e = engine(debug=False)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "moteval_cases.npz"))


def _pair(gt, tr):
    return moteval._Pair(moteval._rows(gt, "ground truth"), moteval._rows(tr, "tracker rows"))


def _call(eng, pairs, thr=0.5):
    """TrackerEngine.mot_identity for a list of packed pairs, twice: the same bytes -> (idtp, per pair gt_to_tr, per pair pot)"""
    a = eng.mot_identity(*moteval.pack(pairs), thr=thr, want_pot=True)
    b = eng.mot_identity(*moteval.pack(pairs), thr=thr, want_pot=True)
    assert [x.dtype for x in a] == [np.int32] * 3
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "the same call twice differs"
    c = eng.mot_identity(*moteval.pack(pairs), thr=thr)
    assert len(c) == 2 and c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes(), "without the counts the result differs"
    g_at, c_at, match, pots = 0, 0, [], []
    for p in pairs:
        match.append(a[1][g_at:g_at + p.n_gid])
        pots.append(a[2][c_at:c_at + p.n_gid * p.n_tid].reshape(p.n_gid, p.n_tid))
        g_at, c_at = g_at + p.n_gid, c_at + p.n_gid * p.n_tid
    assert g_at == len(a[1])
    return a[0], match, pots


def _check_pair(p, idtp, match, pot, thr, what):
    """one pair's device result against identity_ref -> the six figures"""
    want_pot, _ = iref.pot_of(p.gt, p.tr, thr)
    assert pot.shape == want_pot.shape and (pot == want_pot).all(), f"{what}: {np.count_nonzero(pot != want_pot)} counts differ"
    w = iref.reduced(want_pot)
    assert int(idtp) == w, f"{what}: IDTP {int(idtp)} != {w}"
    assert match.shape == (p.n_gid,) and ((match >= -1) & (match < max(p.n_tid, 1))).all(), f"{what}: a match out of range"
    g = np.nonzero(match >= 0)[0]
    assert len(np.unique(match[g])) == len(g), f"{what}: a tracker id is matched twice"
    assert (pot[g, match[g]] > 0).all(), f"{what}: a matched pair with count 0"
    assert int(pot[g, match[g]].sum()) == w, f"{what}: the matching's weight"
    return iref.figures(w, len(p.gt), len(p.tr))


def _check(eng, gt, trs, thr=0.5, what=""):
    """one device call for all tracker row sets against gt, through the engine and through moteval.identity -> identity_ref's figures"""
    pairs = [_pair(gt, t) for t in trs]
    idtp, match, pots = _call(eng, pairs, thr)
    want = [_check_pair(p, idtp[k], match[k], pots[k], thr, f"{what} pair {k}") for k, p in enumerate(pairs)]
    got = moteval.identity(gt, list(trs), eng, thr=thr)
    for k, tr in enumerate(trs):
        assert tuple(got[k]) == SIX
        for f in SIX:
            assert type(got[k][f]) is type(want[k][f]) and json.dumps(got[k][f]) == json.dumps(want[k][f]), f"{what} pair {k}: {f}"
    return want


# ---- the solver's boundaries: one lane, the wave edge, the workgroup edge, a thread's second and third column ---------------------------
@pytest.mark.parametrize("nc", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_id_counts_at_every_solver_boundary(eng, nc):
    """nc ids on the column side (the larger one) and nc - nc // 4 on the row side, more ground-truth ids and more tracker ids;
    square at 65 and 1025.  24 frames of up to 256 boxes a side, 2 frames for the tiny ones."""
    nr = max(1, nc - nc // 4)
    rng = np.random.default_rng(nc)
    shapes = [(nc, nr), (nr, nc)] + ([(nc, nc)] if nc in (65, 1025) else [])
    for n_g, n_t in shapes if nc > 1 else shapes[:1]:
        gt, tr = iref.crowd(rng, n_g, n_t, 24 if nc >= 63 else 2)
        m = _check(eng, gt, [tr], what=f"{n_g} x {n_t} ids")[0]
        assert m["IDTP"] + m["IDFN"] == len(gt) and (nc == 1 or m["IDTP"] > 0)


def test_ids_that_never_meet_the_other_side(eng):
    gt, tr = iref.crowd(np.random.default_rng(7), 400, 300, 12, meet=0.75)
    pot, _ = iref.pot_of(gt, tr)
    assert (pot.sum(1) == 0).sum() >= 100 and (pot.sum(0) == 0).sum() >= 75           # zero rows and zero columns
    for g, t in ((gt, tr), (tr, gt)):                                                 # both orientations
        pairs = [_pair(g, t)]
        idtp, match, pots = _call(eng, pairs)
        _check_pair(pairs[0], idtp[0], match[0], pots[0], 0.5, "zero rows")
        assert (match[0][pots[0].sum(1) == 0] == -1).all()


# ---- the cap ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_g,n_t,frames", [(4096, 3072, 40), (3072, 4096, 40), (4096, 4096, 20)])
def test_pairs_at_the_ids_cap(eng, n_g, n_t, frames):
    gt, tr = iref.crowd(np.random.default_rng(n_g + frames), n_g, n_t, frames)
    m = _check(eng, gt, [tr], what=f"{n_g} x {n_t} ids")[0]
    assert m["IDTP"] > min(n_g, n_t) // 2


def test_4097_ids_are_a_capacity_error_and_the_context_lives_on(eng):
    rng = np.random.default_rng(4097)
    gt, tr = iref.crowd(rng, 4097, 10, 1)
    with pytest.raises(lib.SSError, match=r"pair 0: 4097 ground-truth ids: at most 4096 a side") as e:
        moteval.identity(gt, tr, eng)
    assert e.value.code == lib.SS_ERR_CAPACITY
    with pytest.raises(lib.SSError, match=r"pair 1: 4097 tracker ids") as e:
        moteval.identity_full(tr, [tr, gt], eng)
    assert e.value.code == lib.SS_ERR_CAPACITY
    gt, tr = ref.random_frames(rng, [(5, 7), (7, 5)])
    _check(eng, gt, [tr], what="after the refusals")
    eng.check_errors()
    assert moteval.max_ids() == 4096


# ---- the golden pairs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_golden_cases(eng, golden, name):
    """(b256: three frames of 256 x 256 boxes; this call stores no similarity and has no box x box cap)"""
    z = np.load(os.path.join(GOLD, "identity_cases.npz"))
    gt, tr = case_rows(golden[f"{name}_gt"]), case_rows(golden[f"{name}_tr"])
    m = _check(eng, gt, [tr], what=name)[0]
    assert json.dumps(m) == str(z[f"{name}_identity"]), name
    assert json.dumps(moteval.identity(gt, tr, eng)[0]) == str(z[f"{name}_identity"]), name


# ---- the threshold --------------------------------------------------------------------------------------------------------------
def _row(f, i, x, y=10.0, w=50.0, h=100.0):
    return [f, i, x, y, x + w, y + h, 1.0, 0]


def test_a_similarity_of_exactly_the_threshold_counts(eng):
    gt = np.array([[0, 1, 0, 0, 10, 10, 1, 0], [1, 1, 0, 0, 10, 10, 1, 0]], np.float64)
    tr = np.array([[0, 5, 0, 0, 20, 10, 1, 0], [1, 5, 0, 0, 10, 20, 1, 0]], np.float64)      # inside a box of twice the area: S = 0.5
    assert _check(eng, gt, [tr], thr=0.5, what="S = thr")[0]["IDTP"] == 2
    assert _check(eng, gt, [tr], thr=0.5 + 2.0 ** -40, what="S < thr")[0]["IDTP"] == 0
    # the all-0.25 frame of tests/test_gpu_moteval.py
    gt = np.array([_row(0, 1, 100), _row(0, 2, 300), _row(0, 3, 500), _row(1, 1, 100)], np.float64)
    tr = np.array([_row(0, 1, 130), _row(0, 2, 330), _row(0, 3, 530), _row(0, 4, 900), _row(1, 1, 100)], np.float64)
    assert _check(eng, gt, [tr], thr=0.5, what="thr 0.5")[0]["IDTP"] == 1
    assert _check(eng, gt, [tr], thr=0.25, what="thr 0.25")[0]["IDTP"] == 4
    # thr = 1: only identical boxes count
    moved = tr.copy()
    moved[1:3, 2:6] += 0.25
    m = _check(eng, tr, [tr.copy(), moved], thr=1.0, what="thr 1")
    assert (m[0]["IDTP"], m[0]["IDF1"]) == (5, 1.0) and (m[1]["IDTP"], m[1]["IDFN"], m[1]["IDFP"]) == (3, 2, 2)


def test_a_pair_with_an_empty_side(eng):
    gt = np.array([_row(0, 1, 10), _row(1, 1, 12), _row(1, 2, 300)], np.float64)
    m = _check(eng, gt, [np.zeros((0, 8)), gt], what="no tracker rows")
    assert (m[0]["IDTP"], m[0]["IDFN"], m[0]["IDFP"], m[0]["IDF1"]) == (0, 3, 0, 0.0) and m[1]["IDF1"] == 1.0
    m = _check(eng, np.zeros((0, 8)), [gt], what="no ground truth")[0]
    assert (m["IDTP"], m["IDFN"], m["IDFP"], m["IDF1"]) == (0, 0, 3, 0.0)


# ---- several pairs a call, scratch -----------------------------------------------------------------------------------------------
def test_four_pairs_in_one_call_equal_four_calls_and_scratch_is_reused(eng, golden):
    """A pot that is not zeroed by every call, or scratch sized by an earlier call, shows here: the large pairs come first, the
    small ones are then scored alone in what the large ones left behind."""
    rng = np.random.default_rng(44)
    g30, t30 = case_rows(golden["id30_gt"]), case_rows(golden["id30_tr"])
    pairs = [_pair(*iref.crowd(rng, 300, 280, 24)), _pair(g30, t30), _pair(*iref.crowd(rng, 40, 70, 6)), _pair(g30, g30)]
    whole = _call(eng, pairs)
    for k, p in enumerate(pairs):
        _check_pair(p, whole[0][k], whole[1][k], whole[2][k], 0.5, f"pair {k} of four")
        alone = _call(eng, [p])
        assert alone[0][0] == whole[0][k] and alone[1][0].tobytes() == whole[1][k].tobytes() and alone[2][0].tobytes() == whole[2][k].tobytes(), k
    again = _call(eng, pairs)
    for a, b in zip(whole[1] + whole[2], again[1] + again[2]):
        assert a.tobytes() == b.tobytes()
    assert whole[0].tobytes() == again[0].tobytes() and whole[0][3] == len(g30)


def test_mot_eval_and_mot_identity_alternate_on_one_engine_across_a_growth(eng, golden):
    """The two calls share the context's pinned and device images, lay them out differently and size them by different totals:
    small eval, large identity (grows both), large eval (grows both again), small identity (under-fills them).  Every result
    equals, bit for bit, the same call on a fresh engine."""
    rng = np.random.default_rng(44)
    g6, t6 = case_rows(golden["id6_gt"]), case_rows(golden["id6_tr"])                    # the smallest golden pair
    g30, t30 = case_rows(golden["id30_gt"]), case_rows(golden["id30_tr"])
    small = [_pair(g6, t6)]
    four = [_pair(*iref.crowd(rng, 300, 280, 24)), _pair(g30, t30), _pair(*iref.crowd(rng, 40, 70, 6)), _pair(g30, g30)]
    calls = [("mot_eval", small, {"want_ga": True}), ("mot_identity", four, {"want_pot": True}), ("mot_eval", four, {"want_ga": True}),
             ("mot_identity", small, {"want_pot": True})]
    own = engine(debug=False)                            # not the module's engine: its images have grown already
    got = [getattr(own, name)(*moteval.pack(pairs), **kw) for name, pairs, kw in calls]
    own.close()
    for k, (name, pairs, kw) in enumerate(calls):
        if k == 0:
            continue                                     # (the first call ran on a fresh engine)
        fresh = engine(debug=False)
        want = getattr(fresh, name)(*moteval.pack(pairs), **kw)
        fresh.close()
        assert len(got[k]) == len(want) and len(want) == (5 if name == "mot_eval" else 3)
        for a, b in zip(got[k], want):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"call {k} ({name}) differs from a fresh engine's"


# ---- evaluate ------------------------------------------------------------------------------------------------------------------------
def test_evaluate_with_identity_is_evaluate_plus_six_keys(eng, golden):
    gt, trs = case_rows(golden["id30_gt"]), [case_rows(golden["id30_tr"]), case_rows(golden["id30_gt"])[::2]]
    plain = moteval.evaluate(gt, trs, eng)
    both = moteval.evaluate(gt, trs, eng, identity=True)
    for k, tr in enumerate(trs):
        assert list(both[k]) == list(plain[k]) + list(SIX)
        for f in plain[k]:
            assert type(both[k][f]) is type(plain[k][f]) and json.dumps(both[k][f]) == json.dumps(plain[k][f]), (k, f)      # every old key bit for bit
        assert json.dumps({f: both[k][f] for f in SIX}) == json.dumps(iref.identity(gt, tr)), k
    assert json.dumps(moteval.evaluate(gt, trs, eng)) == json.dumps(plain)                # and the default call after it
    with pytest.raises(ValueError, match="IDF1"):
        moteval.evaluate(gt, trs, eng, metrics=("IDF1",))
    with pytest.raises(ValueError, match="IDF1"):
        moteval.evaluate(gt, trs, eng, metrics=("HOTA", "IDF1"), identity=True)


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def test_cli_adds_the_identity_metrics_to_the_metrics_file(tmp_path):
    from strongsort_yolo_amd.yolo import YOLO
    z = np.load(os.path.join(GOLD, "jpeg_sequence.npz"))
    src = tmp_path / "seq.npy"
    np.save(src, np.stack([np.ascontiguousarray(z[f"rgb_{i}"][:, :, ::-1]) for i in range(12)]))
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack")
    base = {"source": str(src), "track": True, "count": False, "tracker": "bytetrack", "batch": 4, "random_init": True}
    cli.process_video({**base, "outdir": str(tmp_path / "a")}, model=model)
    rows = moteval.read_labels(str(tmp_path / "a" / "seq_labels.txt"))
    assert len(rows)
    truth = rows[np.random.default_rng(0).random(len(rows)) >= 0.2]             # the ground truth: the tracker's own rows, a fifth of them missing
    gsi.write_labels(str(tmp_path / "gt.txt"), truth)
    outs = {}
    for run, extra in (("b", {"eval_identity": True}), ("c", {"eval_identity": True, "gsi": True}), ("d", {})):
        model._stream_pipe.reset_tracker(-1)
        model._frame_index = 0
        outs[run] = cli.process_video({**base, "outdir": str(tmp_path / run), "eval_gt": str(tmp_path / "gt.txt"), **extra}, model=model)
    model.close()
    today, want = ref.evaluate(truth, rows), iref.identity(truth, rows)
    assert 0.0 < want["IDF1"] < 1.0 and want["IDFN"] == 0 and want["IDFP"] == len(rows) - len(truth)
    one = json.loads((tmp_path / "b" / "seq_metrics.json").read_text())
    assert sorted(one) == sorted(list(today) + list(SIX)) and json.dumps({f: one[f] for f in SIX}) == json.dumps(want)
    assert json.dumps({f: one[f] for f in today}) == json.dumps(today)
    both = json.loads((tmp_path / "c" / "seq_metrics.json").read_text())
    assert sorted(both) == ["labels", "labels_gsi"]
    assert json.dumps(both["labels"]) == json.dumps(one)
    want_gsi = iref.identity(truth, moteval.read_labels(str(tmp_path / "c" / "seq_labels_gsi.txt")))
    assert json.dumps({f: both["labels_gsi"][f] for f in SIX}) == json.dumps(want_gsi) and len(both["labels_gsi"]) == len(one)
    assert outs["b"]["IDF1"] == want["IDF1"] and "IDF1_gsi" not in outs["b"]
    assert (outs["c"]["IDF1"], outs["c"]["IDF1_gsi"]) == (want["IDF1"], want_gsi["IDF1"])
    # without the flag: today's file and summary
    plain = json.loads((tmp_path / "d" / "seq_metrics.json").read_text())
    assert sorted(plain) == sorted(today) and json.dumps({f: plain[f] for f in today}) == json.dumps(today)
    assert "IDF1" not in outs["d"] and sorted(set(outs["b"]) - set(outs["d"])) == ["IDF1"]
