"""The identity metrics IDF1, IDP, IDR on the CPU (docs/MOTEVAL.md §1 "Identity"): TrackEval's (G+T)² formulation as this project
restates it against the reduction to a G x T maximum-weight matching (tests/identity_ref.py), closed forms, the host half of
strongsort_yolo_amd.moteval fed by a stand-in engine that answers from identity_ref, every refusal ss_mot_identity makes before it
looks at a context or the device, the parser and the golden file."""
import ctypes as C
import json
import os

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from strongsort_yolo_amd import cli, lib, moteval
from tests import identity_ref as iref
from tests import moteval_ref as ref
from tests.golden.make_identity_golden import figures_by_full
from tests.golden.make_moteval_golden import NAMES, case_rows
from tests.test_moteval_cpu import GOOD, ORDER, RecordEngine

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIX = ("IDTP", "IDFN", "IDFP", "IDF1", "IDP", "IDR")


def _row(f, i, x, y=10.0, w=50.0, h=100.0):
    return [f, i, x, y, x + w, y + h, 1.0, 0]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "moteval_cases.npz"))


def _full_equals_reduced(gt, tr, what):
    pot, p = iref.pot_of(gt, tr)
    w = iref.reduced(pot)
    want = (w, len(p.gt) - w, len(p.tr) - w)
    assert iref.full(pot, p.cnt_g, p.cnt_t) == want, what
    return pot, want


# ---- the reduction: optimum of the (G+T)² matrix == rows of both sides - 2 W ----------------------------------------------------------
def test_full_formulation_equals_the_reduction_on_the_golden_pairs(golden):
    for name in NAMES:
        _full_equals_reduced(case_rows(golden[f"{name}_gt"]), case_rows(golden[f"{name}_tr"]), name)


@pytest.mark.parametrize("n_gid,n_tid,frames,meet", [(1, 1, 2, 1.0), (7, 12, 4, 1.0), (63, 48, 6, 1.0), (100, 130, 12, 0.75), (300, 280, 24, 1.0), (290, 300, 24, 0.75)])
def test_full_formulation_equals_the_reduction_on_crowds(n_gid, n_tid, frames, meet):
    gt, tr = iref.crowd(np.random.default_rng(n_gid * 1000 + n_tid), n_gid, n_tid, frames, meet=meet)
    pot, _ = _full_equals_reduced(gt, tr, (n_gid, n_tid))
    assert pot.shape == (n_gid, n_tid)
    if meet < 1.0:                                       # a quarter of the ids of each side never meets the other side
        assert (pot.sum(1) == 0).sum() >= n_gid // 4 and (pot.sum(0) == 0).sum() >= n_tid // 4


def test_full_formulation_equals_the_reduction_near_1100_ids():
    gt, tr = iref.crowd(np.random.default_rng(1100), 1100, 1030, 24)
    pot, _ = _full_equals_reduced(gt, tr, "1100 x 1030")
    assert pot.shape == (1100, 1030) and 4 <= pot.max() <= 12 and (pot > 0).mean() > 0.25      # small counts, massive ties


def test_the_crowd_generator_passes_a_third_to_a_half_of_a_frames_cells():
    gt, tr = iref.crowd(np.random.default_rng(0), 256, 256, 24)
    pot, p = iref.pot_of(gt, tr)
    assert len(p.frames) == 24 and 1 / 3 < pot.sum() / (24 * 256 * 256) < 1 / 2


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
def test_a_sequence_against_itself_is_perfect(golden):
    gt = case_rows(golden["id30_gt"])
    m = iref.identity(gt, gt)
    assert m["IDF1"] == m["IDP"] == m["IDR"] == 1.0 and (m["IDTP"], m["IDFN"], m["IDFP"]) == (len(gt), 0, 0)


def test_two_tracks_whose_tracker_ids_swap_at_the_midpoint():
    """HOTA 0.577 and MOTA 0.95 for the same input in tests/test_moteval_cpu.py: IDF1 is the figure that halves."""
    n = 20
    gt = [_row(f, i + 1, 10 + 300 * i) for f in range(n) for i in range(2)]
    tr = [_row(f, (i if f < n // 2 else 1 - i) + 1, 10 + 300 * i) for f in range(n) for i in range(2)]
    m = iref.identity(gt, tr)
    assert (m["IDTP"], m["IDFN"], m["IDFP"]) == (20, 20, 20) and m["IDF1"] == 0.5 == m["IDP"] == m["IDR"]
    assert figures_by_full(np.array(gt, np.float64), np.array(tr, np.float64)) == m


def test_dropping_one_tracker_id_lowers_recall_only(golden):
    gt = case_rows(golden["id6_gt"])
    tr = gt[gt[:, 1] != gt[0, 1]]
    m = iref.identity(gt, tr)
    assert m["IDR"] < 1.0 and m["IDP"] == 1.0 and m["IDFP"] == 0 and m["IDFN"] == len(gt) - len(tr)


def test_a_similarity_of_exactly_one_half_counts_at_one_half():
    gt = np.array([[0, 1, 0, 0, 10, 10, 1, 0]], np.float64)
    tr = np.array([[0, 5, 0, 0, 20, 10, 1, 0]], np.float64)          # the ground-truth box lies inside one of twice its area
    assert ref.similarity(gt[:, 2:6], tr[:, 2:6])[0, 0] == 0.5
    assert iref.identity(gt, tr, 0.5)["IDTP"] == 1 and iref.identity(gt, tr, 0.5 + 2.0 ** -40)["IDTP"] == 0
    assert iref.identity(gt, tr, 0.25)["IDF1"] == 1.0


# ---- the golden file --------------------------------------------------------------------------------------------------------------
def test_golden_file_is_what_the_full_formulation_computes(golden):
    z = np.load(os.path.join(GOLD, "identity_cases.npz"))
    assert os.path.getsize(os.path.join(GOLD, "identity_cases.npz")) < 4096
    for name in NAMES:
        gt, tr = case_rows(golden[f"{name}_gt"]), case_rows(golden[f"{name}_tr"])
        want = json.loads(str(z[f"{name}_identity"]))
        assert tuple(want) == SIX
        assert json.dumps(figures_by_full(gt, tr)) == str(z[f"{name}_identity"]) == json.dumps(iref.identity(gt, tr)), name
    assert json.loads(str(z["id6_identity"]))["IDF1"] == 1.0 and 0.8 < json.loads(str(z["id30_identity"]))["IDF1"] < 0.84


# ---- the module's host half, fed from identity_ref -----------------------------------------------------------------------------------
class IdentityEngine(RecordEngine):
    """RecordEngine plus a stand-in for TrackerEngine.mot_identity: unpacks the call into rows again and answers with identity_ref's
    counts, SciPy's weight and SciPy's matching (cells of count 0 are no match)."""

    def __init__(self):
        super().__init__()
        self.identity_calls = 0

    def mot_identity(self, frame_off, gt_off, tr_off, gt_ids, tr_ids, gt_boxes, tr_boxes, n_gt_ids, n_tr_ids, thr=0.5, want_pot=False):
        self.identity_calls += 1
        idtp, match, pots = [], [], []
        for p in range(len(frame_off) - 1):
            f0, f1 = frame_off[p], frame_off[p + 1]
            sides = []
            for off, ids, boxes in ((gt_off, gt_ids, gt_boxes), (tr_off, tr_ids, tr_boxes)):
                a, b = off[f0], off[f1]
                r = np.zeros((b - a, 8))
                r[:, 0] = np.repeat(np.arange(f1 - f0), np.diff(off[f0:f1 + 1]))
                r[:, 1], r[:, 2:6] = ids[a:b], boxes[a:b]
                sides.append(r)
            pot, pr = iref.pot_of(sides[0], sides[1], thr)
            assert pot.shape == (n_gt_ids[p], n_tr_ids[p])
            m = np.full(n_gt_ids[p], -1, np.int32)
            if pot.size:
                r, c = linear_sum_assignment(-pot)
                m[r[pot[r, c] > 0]] = c[pot[r, c] > 0]
            idtp.append(iref.reduced(pot)); match.append(m); pots.append(pot.ravel().astype(np.int32))
        return (np.asarray(idtp, np.int32), np.concatenate(match)) + ((np.concatenate(pots),) if want_pot else ())


def test_module_host_half_equals_identity_ref(golden):
    eng = IdentityEngine()
    gt = case_rows(golden["id30_gt"])
    trs = [case_rows(golden["id30_tr"]), gt.copy(), gt[gt[:, 0] % 3 != 1], np.zeros((0, 8))]
    shuffled = gt[np.random.default_rng(0).permutation(len(gt))]                      # any row order
    got = moteval.identity(shuffled, trs, eng)
    assert (eng.identity_calls, eng.calls) == (1, 0) and len(got) == 4
    for k, tr in enumerate(trs):
        want = iref.identity(gt, tr)
        assert tuple(got[k]) == SIX and json.dumps(got[k]) == json.dumps(want), k
        assert all(type(got[k][f]) is int for f in SIX[:3]) and all(type(got[k][f]) is float for f in SIX[3:])
    assert (got[3]["IDTP"], got[3]["IDFN"], got[3]["IDFP"], got[3]["IDF1"]) == (0, len(gt), 0, 0.0)           # an empty tracker row set
    assert moteval.identity(gt, [], eng) == [] and moteval.identity_full(gt, [], eng) == ([], [])
    none = moteval.identity(np.zeros((0, 8)), gt, eng)[0]                              # an empty ground truth
    assert (none["IDTP"], none["IDFN"], none["IDFP"], none["IDF1"], none["IDP"]) == (0, 0, len(gt), 0.0, 0.0)
    # identity_full: the matching by original ids and the counts
    res, rec = moteval.identity_full(shuffled, trs[:2], eng)
    assert json.dumps(res) == json.dumps(got[:2])
    pot, p = iref.pot_of(gt, trs[0])
    assert rec[0]["pot"].shape == pot.shape and (rec[0]["pot"] == pot).all()
    m = rec[0]["gt_to_tr"]
    assert len(set(m.values())) == len(m) and set(m) <= set(gt[:, 1]) and set(m.values()) <= set(trs[0][:, 1])
    assert sum(int(pot[np.searchsorted(p.gt_uid, g), np.searchsorted(p.tr_uid, t)]) for g, t in m.items()) == res[0]["IDTP"]
    assert rec[1]["gt_to_tr"] == {i: i for i in np.unique(gt[:, 1])}
    # a class filter drops rows on the host first
    extra = np.concatenate([gt, np.array([_row(3, 999, 500)[:7] + [5]])])
    assert json.dumps(moteval.identity(extra, trs[0], eng, classes=[0])[0]) == json.dumps(got[0])
    with pytest.raises(ValueError, match="thr"):
        moteval.identity(gt, trs[0], eng, thr=0.0)


def test_evaluate_with_identity_adds_six_keys_through_a_second_call(golden):
    eng = IdentityEngine()
    gt, trs = case_rows(golden["more_tr_gt"]), [case_rows(golden["more_tr_tr"]), np.zeros((0, 8))]
    plain = moteval.evaluate(gt, trs, eng)
    assert (eng.calls, eng.identity_calls) == (1, 0)
    both = moteval.evaluate(gt, trs, eng, identity=True)
    assert (eng.calls, eng.identity_calls) == (2, 1)
    full, _ = moteval.evaluate_full(gt, trs, eng, identity=True)
    for k, tr in enumerate(trs):
        assert list(both[k]) == list(plain[k]) + list(SIX) == list(full[k])
        assert json.dumps({f: both[k][f] for f in plain[k]}) == json.dumps(plain[k])
        assert json.dumps({f: both[k][f] for f in SIX}) == json.dumps(iref.identity(gt, tr)) == json.dumps({f: full[k][f] for f in SIX})
    # without the flag an engine that has no mot_identity serves: exactly one call
    old = RecordEngine()
    assert not hasattr(old, "mot_identity")
    assert json.dumps(moteval.evaluate(gt, trs, old)) == json.dumps(plain) and old.calls == 1
    for f in ("IDF1", "IDP", "IDR"):
        with pytest.raises(ValueError, match=f + r".*identity=True.*moteval\.identity"):
            moteval.evaluate(gt, trs, eng, metrics=(f,), identity=True)


# ---- refusals before the device -------------------------------------------------------------------------------------------------
def _call(L, null=None, want_pot=False, **change):
    a = {**GOOD, **change}
    arrs = [np.ascontiguousarray(a[k], np.float64 if k.endswith("boxes") else np.int32) for k in ORDER]
    outs = [np.zeros(max(len(arrs[7]), 1), np.int32), np.zeros(max(len(arrs[3]), 1), np.int32)]
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    args = [v.ctypes.data_as(pd if v.dtype == np.float64 else pi) for v in arrs] + [float(a["thr"])] + [v.ctypes.data_as(pi) for v in outs]
    args.append(np.zeros(64, np.int32).ctypes.data_as(pi) if want_pot else None)
    if null is not None:
        args[null] = None
    rc = L.ss_mot_identity(None, len(arrs[0]) - 1, *args)
    return rc, (L.ss_last_error(None) or b"").decode()


def test_every_argument_refusal_comes_before_the_context():
    lib.build()
    L = lib.load()
    assert L.ss_mot_max_ids() == 4096 == moteval.max_ids()
    for want_pot in (False, True):
        rc, msg = _call(L, want_pot=want_pot)
        assert rc == lib.SS_ERR_INVALID and msg == "ss_mot_identity: null context"        # the arguments themselves pass; pot may be NULL
    for null in list(range(9)) + [10, 11]:
        rc, msg = _call(L, null=null)
        assert rc == lib.SS_ERR_INVALID and msg == "ss_mot_identity: null argument", null
    cases = [
        (dict(frame_off=[1, 2, 3]), "offsets must start at 0"),
        (dict(tr_off=[1, 1, 1, 3]), "offsets must start at 0"),
        (dict(frame_off=[0, 4, 3]), "pair 1: frame offsets decrease"),
        (dict(gt_off=[0, 2, 1, 4]), "pair 0: frame 1: ground-truth row offsets decrease"),
        (dict(tr_off=[0, 1, 3, 2]), "pair 1: frame 0: tracker row offsets decrease"),
        (dict(gt_ids=[0, 2, 1, 0]), "pair 0: frame 0: a ground-truth id is out of range"),
        (dict(gt_ids=[0, -1, 1, 0]), "pair 0: frame 0: a ground-truth id is out of range"),
        (dict(tr_ids=[0, 1, 2]), "pair 1: frame 0: a tracker id is out of range"),
        (dict(tr_ids=[0, 1, 1]), "pair 1: frame 0: a tracker id appears twice"),
        (dict(tr_boxes=[[0, 0, 10, 10], [0, 0, 5, 5], [9, 9, np.inf, 12]]), "pair 1: frame 0: a tracker box is NaN or infinite"),
        (dict(gt_boxes=[[0, 0, 10, 10], [20, 0, 20, 10]] + GOOD["gt_boxes"][2:]), "pair 0: frame 0: a ground-truth box has x2 <= x1 or y2 <= y1"),
        (dict(n_gt_ids=[2, -1]), "pair 1: an id count is negative"),
        (dict(n_tr_ids=[1, 3]), "pair 1: more ids than rows"),
    ]
    for change, want in cases:
        rc, msg = _call(L, **change)
        assert rc == lib.SS_ERR_INVALID and msg.startswith("ss_mot_identity: ") and want in msg, (want, msg)
    for thr in (0.0, -0.5, 1.0000001, np.nan):
        rc, msg = _call(L, thr=thr)
        assert rc == lib.SS_ERR_INVALID and "thr must be in (0, 1]" in msg, thr
    assert _call(L, thr=1.0)[1] == "ss_mot_identity: null context"


def _many_ids(n_g, n_t):
    """one pair in which every id has one row: frames of up to 256 boxes a side"""
    frames = -(-max(n_g, n_t) // 256)
    off = lambda n: np.minimum(np.arange(frames + 1) * 256, n)
    return dict(frame_off=[0, frames], gt_off=off(n_g), tr_off=off(n_t), gt_ids=np.arange(n_g), tr_ids=np.arange(n_t),
                gt_boxes=np.tile([0.0, 0, 1, 1], (n_g, 1)), tr_boxes=np.tile([0.0, 0, 1, 1], (n_t, 1)), n_gt_ids=[n_g], n_tr_ids=[n_t])


def test_the_ids_cap_is_refused_before_the_context_and_the_box_cap_is_gone():
    L = lib.load()
    rc, msg = _call(L, **_many_ids(4097, 3))
    assert rc == lib.SS_ERR_CAPACITY and msg == "ss_mot_identity: pair 0: 4097 ground-truth ids: at most 4096 a side"
    rc, msg = _call(L, **_many_ids(3, 4097))
    assert rc == lib.SS_ERR_CAPACITY and msg == "ss_mot_identity: pair 0: 4097 tracker ids: at most 4096 a side"
    two = _many_ids(5, 4097)
    two.update(frame_off=[0, 0, two["frame_off"][1]], n_gt_ids=[0, 5], n_tr_ids=[0, 4097])
    assert "pair 1: 4097 tracker ids" in _call(L, **two)[1]
    assert _call(L, **_many_ids(4096, 4096)) == (lib.SS_ERR_INVALID, "ss_mot_identity: null context")
    # 2 049 frames of 256 x 256 boxes are more than the 2^27 box x box cells ss_mot_eval may store: no cap here, nothing is stored
    F, n = 2049, 2049 * 256
    rc, msg = _call(L, frame_off=[0, F], gt_off=np.arange(F + 1) * 256, tr_off=np.arange(F + 1) * 256, gt_ids=np.tile(np.arange(256), F),
                    tr_ids=np.tile(np.arange(256), F), gt_boxes=np.tile([0.0, 0, 1, 1], (n, 1)), tr_boxes=np.tile([0.0, 0, 1, 1], (n, 1)),
                    n_gt_ids=[256], n_tr_ids=[256])
    assert (rc, msg) == (lib.SS_ERR_INVALID, "ss_mot_identity: null context")
    # the caps that stay: boxes a frame, pairs a call
    rc, msg = _call(L, frame_off=[0, 1], gt_off=[0, 257], tr_off=[0, 1], gt_ids=list(range(257)), tr_ids=[0], gt_boxes=[[0, 0, 1, 1]] * 257,
                    tr_boxes=[[0, 0, 1, 1]], n_gt_ids=[257], n_tr_ids=[1])
    assert rc == lib.SS_ERR_CAPACITY and "pair 0: frame 0: 257 ground-truth boxes: at most 256 a frame" in msg


# ---- the parser -----------------------------------------------------------------------------------------------------------------
def test_eval_identity_without_eval_gt_is_a_parser_error(capsys):
    with pytest.raises(SystemExit):
        cli.main(["--source", "synthetic:2", "--track", "--eval-identity"])
    err = capsys.readouterr().err
    assert "--eval-identity" in err and "--eval-gt" in err
