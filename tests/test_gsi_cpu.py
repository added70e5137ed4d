"""GSI on the CPU (docs/GSI.md): the restatement tests/gsi_ref.py against scikit-learn and against a known trajectory, the host half
of strongsort_yolo_amd.gsi (interpolation, length scale, labels) against the restatement, and every refusal ss_gsi_smooth makes
before it looks at a context or the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from strongsort_yolo_amd import cli, gsi, lib
from tests import gsi_ref
from tests.golden.make_gsi_golden import case_rows

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SK_LENGTHS = list(range(1, 70)) + [100, 127, 128, 129, 191, 192, 193, 256, 300]
SK_BOUND = 2e-3     # px: alpha = 1e-10 makes the system's condition number ~1e10, so two f64 solvers differ by ~cond * eps * |y| ~ 1e-3 px


# ---- the restatement -------------------------------------------------------------------------------------------------------
def test_restatement_against_scikit_learn():
    """Every length of SK_LENGTHS, with and without gaps of 20 .. 60 frames, tau 5 / 10 / 20, coordinates up to ~1.6e3 px.
    Measured: no pivot failure, largest difference 2.5e-4 px (docs/GSI.md "Measured")."""
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF
    rng = np.random.default_rng(2024)
    worst, cases = 0.0, 0
    for tau in (5.0, 10.0, 20.0):
        for gaps in (False, True):
            for n in SK_LENGTHS:
                r = gsi_ref.make_track(rng, n, gaps)
                frames, vals, l = r[:, 0].astype(np.int64), gsi_ref.tlwh(r), gsi_ref.length_scale(n, tau)
                assert np.abs(r[:, 2:6]).max() < 2e3
                m, st = gsi_ref.solve_track(frames, vals, l)
                assert st == 0, (tau, gaps, n)
                X = frames.astype(np.float64).reshape(-1, 1)
                gp = GaussianProcessRegressor(RBF(l, "fixed"), alpha=1e-10, optimizer=None).fit(X, vals)
                worst = max(worst, float(np.abs(gp.predict(X) - m).max()))
                cases += 1
    print(f"gsi_ref vs scikit-learn: {cases} cases, largest difference {worst:.3e} px")
    assert cases == 6 * len(SK_LENGTHS) and worst <= SK_BOUND


def test_column_schedule_equals_the_element_by_element_statement():
    rng = np.random.default_rng(1)
    for n, gaps in ((1, False), (2, False), (3, True), (17, False), (33, True), (40, False)):
        r = gsi_ref.make_track(rng, n, gaps)
        a = gsi_ref.solve_track(r[:, 0].astype(np.int64), gsi_ref.tlwh(r), gsi_ref.length_scale(n))
        b = gsi_ref.solve_track_scalar(r[:, 0].astype(np.int64), gsi_ref.tlwh(r), gsi_ref.length_scale(n))
        assert a[1] == b[1] == 0 and a[0].tobytes() == b[0].tobytes(), n


def test_expneg_on_arrays_equals_the_scalar_sequence():
    x = np.concatenate([[0.0, 700.0, np.nextafter(700.0, np.inf), np.inf, 1e-300], np.random.default_rng(0).uniform(0, 710, 2000)])
    assert gsi_ref.expneg_array(x).tobytes() == np.array([gsi_ref.ss_expneg(v) for v in x]).tobytes()
    K = gsi_ref.kernel_matrix([0, 1, 5], 2.0)
    assert (np.diag(K) == 1.0).all() and K[0, 2] == gsi_ref.ss_expneg(25.0 / 8.0)


def test_smoothing_brings_noisy_tracks_closer_to_their_trajectory():
    rng = np.random.default_rng(77)
    for n in (20, 30, 60, 120, 200):
        for k in range(5):
            r = gsi_ref.make_track(rng, n)
            truth = gsi_ref.trajectory(r[:, 0])
            out, st = gsi_ref.smooth(r)
            assert st == {1: 0}
            before = np.sqrt(np.mean((r[:, 2:6] - truth) ** 2))
            after = np.sqrt(np.mean((out[:, 2:6] - truth) ** 2))
            print(f"n={n} track {k}: rms {before:.3f} -> {after:.3f} px")
            assert after < 0.75 * before


def test_zero_pivot_is_status_1_and_rows_pass_through():
    r = gsi_ref.make_track(np.random.default_rng(3), 2)
    m, st = gsi_ref.solve_track([0, 1], gsi_ref.tlwh(r), 1e9, 0.0)
    assert st == 1 and m.tobytes() == gsi_ref.tlwh(r).tobytes()


# ---- interpolation -----------------------------------------------------------------------------------------------------------
def _track(frames, tid=1, cls=2.0):
    rng = np.random.default_rng(int(frames[-1]))
    r = np.zeros((len(frames), 8))
    r[:, 0], r[:, 1], r[:, 6], r[:, 7] = frames, tid, 0.8, cls
    r[:, 2:6] = rng.uniform(0, 1000, (len(frames), 4))
    return r


def test_gaps_below_the_interval_are_filled_and_longer_ones_stay():
    r = _track([0, 2, 21, 41, 62, 63])                  # gaps of 2, 19, 20, 21, 1
    out = gsi_ref.interpolate(r)
    assert list(out[:, 0]) == [0, 1, 2] + list(range(3, 21)) + [21, 41, 62, 63]
    new = out[~np.isin(out[:, 0], r[:, 0])]
    assert len(new) == 1 + 18 and (new[:, 6] == 0.0).all() and (new[:, 7] == 2.0).all() and (new[:, 1] == 1).all()
    assert gsi_ref.interpolate(r, interval=22)[:, 0].tolist() == list(range(0, 64))          # now 20 and 21 are short enough
    assert len(gsi_ref.interpolate(r, interval=2)) == len(r)


def test_interpolated_values_follow_the_operation_order_and_cls_is_the_earlier_rows():
    r = _track([10, 17])
    r[1, 7] = 5.0
    out = gsi_ref.interpolate(r)
    assert len(out) == 8
    for j in range(1, 7):
        row = out[j]
        assert row[0] == 10 + j and row[6] == 0.0 and row[7] == 2.0
        for c in range(2, 6):
            step = (r[1, c] - r[0, c]) / 7.0
            assert row[c] == r[0, c] + step * float(j)


def test_duplicates_raise_and_the_output_is_sorted_by_frame_then_id():
    a, b = _track([0, 3, 4], tid=7), _track([1, 2, 6], tid=3)
    rows = np.concatenate([a, b], 0)[[4, 0, 5, 2, 1, 3]]
    for f in (gsi_ref.interpolate, gsi.interpolate):
        out = f(rows)
        key = out[:, 0] * 1000 + out[:, 1]
        assert (np.diff(key) > 0).all() and len(out) == 6 + 2 + 3
        with pytest.raises(ValueError, match="duplicate"):
            f(np.concatenate([rows, rows[:1]], 0))
    assert len(gsi.interpolate(np.zeros((0, 8)))) == 0


def test_package_interpolation_equals_the_restatement_byte_for_byte():
    rng = np.random.default_rng(8)
    rows = []
    for tid in range(1, 30):
        t = gsi_ref.make_track(rng, int(rng.integers(1, 80)), False, tid=tid, start=int(rng.integers(0, 100)))
        keep = rng.uniform(size=len(t)) > 0.3
        keep[0] = True
        rows.append(t[keep])
    rows = np.concatenate(rows, 0)[rng.permutation(sum(len(t) for t in rows))]
    for interval in (20, 5, 1):
        a, b = gsi.interpolate(rows, interval), gsi_ref.interpolate(rows, interval)
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert len(gsi.interpolate(rows)) > len(rows)


# ---- length scale, cap --------------------------------------------------------------------------------------------------------
def test_length_scale_at_the_clip_edges():
    assert gsi.length_scale(1, 10) == 10.0 * np.log(1000.0) < 100.0                       # the upper clip is not reached at tau = 10
    assert gsi.length_scale(1, 2) == 4.0 == gsi_ref.length_scale(1, 2)                     # 2 ln 8 = 4.16 -> tau^2
    assert gsi.length_scale(990, 10) == 10.0 * np.log(1000.0 / 990.0) > 0.1
    assert gsi.length_scale(991, 10) == 0.1 == gsi.length_scale(5000, 10)
    for n in (1, 2, 50, 300, 990, 991, 1024):
        for tau in (5, 10.0, 20):
            assert gsi.length_scale(n, tau) == gsi_ref.length_scale(n, tau)


def test_the_cap_is_1024_and_longer_tracks_are_settled_on_the_host():
    lib.build()
    L = lib.load()
    assert L.ss_gsi_max_len() == 1024 == gsi.MAX_LEN == gsi_ref.MAX_LEN == gsi.max_len()
    assert gsi.BOUNDARIES[-1] == gsi.MAX_LEN and gsi.LDS_MAX < gsi.MAX_LEN
    # the path boundaries gsi.py names (tests/test_gpu_gsi.py builds its lengths from them) are the kernel's own constants
    src = open(os.path.join(lib.CSRC, "ss_gsi.hip")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (GSI_[A-Z_]+) (\d+)\b", src, flags=re.M)}
    assert (defs["GSI_MAX_LEN"], defs["GSI_LDS_MAX"], defs["GSI_PANEL"], defs["GSI_TILE"]) == (gsi.MAX_LEN, gsi.LDS_MAX, gsi.PANEL, gsi.TILE)
    assert gsi.BOUNDARIES == (gsi.TILE, gsi.PANEL, gsi.LDS_MAX, gsi.MAX_LEN)
    # status 2 is decided on the host: a call that holds only a 1025-row track and an empty one needs neither a device nor a context
    z = np.load(os.path.join(GOLD, "gsi_cases.npz"))
    rows = case_rows(z["p1025_frames"], z["p1025_xyxy"])
    ref, st = gsi_ref.smooth(rows)
    assert st == {1: 2} and ref.tobytes() == rows.tobytes()
    vals = gsi_ref.tlwh(rows)
    off, frames = np.array([0, 1025, 1025], np.int32), rows[:, 0].astype(np.int32)
    ls, out, status = np.array([0.1, 1.0]), np.zeros((1025, 4)), np.full(2, -1, np.int32)
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    assert L.ss_gsi_smooth(None, 2, off.ctypes.data_as(pi), frames.ctypes.data_as(pi), vals.ctypes.data_as(pd), ls.ctypes.data_as(pd), 1e-10,
                           out.ctypes.data_as(pd), status.ctypes.data_as(pi)) == lib.SS_OK
    assert status.tolist() == [2, 0] and out.tobytes() == vals.tobytes()


def test_golden_case_is_what_the_restatement_computes():
    z = np.load(os.path.join(GOLD, "gsi_cases.npz"))
    assert os.path.getsize(os.path.join(GOLD, "gsi_cases.npz")) < 200_000
    rows = case_rows(z["g1024_frames"], z["g1024_xyxy"])
    assert len(rows) == 1024 and np.diff(rows[:, 0]).max() >= 20
    out, st = gsi_ref.smooth(rows)
    assert st == {1: 0} and out[:, 2:6].tobytes() == z["g1024_out"].tobytes()
    assert len(z["c1024_frames"]) == 1024 and (np.diff(z["c1024_frames"]) == 1).all() and len(z["p1025_frames"]) == 1025


# ---- labels, parser ---------------------------------------------------------------------------------------------------------
def test_write_labels_line_format(tmp_path):
    rows = np.array([[3, 12, 10.9, 20.2, 110.7, 220.999, 0.87654, 2], [4, 12, -0.5, 20.0, 99.5, 100.0, 0.0, 0]])
    assert gsi.write_labels(str(tmp_path / "x.txt"), rows) == 2
    text = (tmp_path / "x.txt").read_text()
    assert text == "3 2 12 0.877 10 20 110 220 -1 -1 -1 -1\n4 0 12 0.0 0 20 99 100 -1 -1 -1 -1\n" == gsi_ref.label_lines(rows)


def test_rows_of_keeps_the_float_corners():
    import torch
    from strongsort_yolo_amd.yolo import Boxes, Results
    b = Boxes(torch.tensor([[1.5, 2.25, 30.75, 40.5], [5.0, 6.0, 7.0, 8.0]]), torch.tensor([0.5, 0.25]), torch.tensor([0.0, 3.0]), torch.tensor([7.0, 9.0]))
    rows = gsi.rows_of([Results(None, {}, b), Results(None, {}, None)], 11)
    assert rows.dtype == np.float64 and rows.tolist() == [[11, 7, 1.5, 2.25, 30.75, 40.5, 0.5, 0], [11, 9, 5, 6, 7, 8, 0.25, 3]]
    assert gsi.rows_of([Results(None, {}, Boxes(b.xyxy, b.conf, b.cls, None))], 0).shape == (0, 8)


def test_gsi_without_track_is_a_parser_error(capsys):
    with pytest.raises(SystemExit):
        cli.main(["--source", "synthetic:2", "--gsi"])
    err = capsys.readouterr().err
    assert "--gsi" in err and "--track" in err


# ---- refusals before the device ------------------------------------------------------------------------------------------------
def _call(L, offsets, frames, vals, ls, alpha=1e-10, null=None):
    offsets, frames = np.ascontiguousarray(offsets, np.int32), np.ascontiguousarray(frames, np.int32)
    vals, ls = np.ascontiguousarray(vals, np.float64), np.ascontiguousarray(ls, np.float64)
    out, status = np.zeros((max(len(frames), 1), 4)), np.zeros(max(len(ls), 1), np.int32)
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    args = [offsets.ctypes.data_as(pi), frames.ctypes.data_as(pi), vals.ctypes.data_as(pd), ls.ctypes.data_as(pd), float(alpha),
            out.ctypes.data_as(pd), status.ctypes.data_as(pi)]
    if null is not None:
        args[null] = None
    rc = L.ss_gsi_smooth(None, len(offsets) - 1, *args)
    return rc, (L.ss_last_error(None) or b"").decode()


def test_every_argument_refusal_comes_before_the_context():
    lib.build()
    L = lib.load()
    good = ([0, 3, 3, 5], [4, 5, 9, 0, 1], np.ones((5, 4)), [1.0, 2.0, 3.0])
    rc, msg = _call(L, *good)
    assert rc == lib.SS_ERR_INVALID and msg == "ss_gsi_smooth: null context"          # the arguments themselves pass
    for null in (0, 1, 2, 3, 5, 6):
        rc, msg = _call(L, *good, null=null)
        assert rc == lib.SS_ERR_INVALID and "null argument" in msg, null
    cases = [
        (([1, 3, 3, 5],) + good[1:], "offsets[0] must be 0"),
        (([0, 3, 2, 5],) + good[1:], "track 1: offsets decrease"),
        ((good[0], [4, 5, 5, 0, 1]) + good[2:], "track 0: frames must increase strictly"),
        ((good[0], [4, 5, 9, 1, 0]) + good[2:], "track 2: frames must increase strictly"),
        (good[:3] + ([1.0, 2.0, 0.0],), "track 2: len_scale"),
        (good[:3] + ([-1.0, 2.0, 1.0],), "track 0: len_scale"),
        (good[:3] + ([1.0, np.nan, 1.0],), "track 1: len_scale"),
        (good[:3] + ([1.0, np.inf, 1.0],), "track 1: len_scale"),
    ]
    for args, want in cases:
        rc, msg = _call(L, *args)
        assert rc == lib.SS_ERR_INVALID and want in msg, (want, msg)
    for bad in (np.nan, np.inf, -np.inf):
        v = np.ones((5, 4))
        v[4, 2] = bad
        rc, msg = _call(L, good[0], good[1], v, good[3])
        assert rc == lib.SS_ERR_INVALID and "track 2: a value is NaN or infinite" in msg
    for alpha in (-1e-10, np.nan, np.inf):
        rc, msg = _call(L, *good, alpha=alpha)
        assert rc == lib.SS_ERR_INVALID and "alpha" in msg
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    z = np.zeros(4)
    for n in (0, -1, 65537):
        assert L.ss_gsi_smooth(None, n, z.ctypes.data_as(pi), z.ctypes.data_as(pi), z.ctypes.data_as(pd), z.ctypes.data_as(pd), 1e-10,
                               z.ctypes.data_as(pd), z.ctypes.data_as(pi)) == lib.SS_ERR_INVALID
        assert b"n_tracks must be 1 .. 65536" in L.ss_last_error(None)
