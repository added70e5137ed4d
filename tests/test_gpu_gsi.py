"""GSI's smoothing kernel on the MI355X (csrc/ss_gsi.hip, docs/GSI.md) against its CPU restatement (tests/gsi_ref.py), bit for bit."""
import os

import numpy as np
import pytest

from strongsort_yolo_amd import cli, gsi, lib
from tests import gsi_ref
from tests.golden.make_gsi_golden import case_rows
from tests.gpu_util import engine

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def eng():
    e = engine(debug=False)
    yield e
    e.close()


def _lengths():
    """1, 2, 3, the wave and block edges, and B-1, B, B+1 for every path boundary the kernel has (gsi.BOUNDARIES follows the kernel:
    tile, panel, the LDS / device-memory switch, the cap — beyond the cap is status 2, the golden 1025-row case)."""
    ns = {1, 2, 3, 63, 64, 65, 127, 128, 129}
    for b in gsi.BOUNDARIES:
        ns |= {b - 1, b, b + 1}
    ns |= {gsi.LDS_MAX + gsi.PANEL, gsi.LDS_MAX + gsi.PANEL + 1}          # the first whole panel and ragged tile behind the switch
    return sorted(n for n in ns if 1 <= n < gsi.MAX_LEN)                    # (the cap and beyond: the golden cases)


def _many(rng, lengths, gaps):
    return np.concatenate([gsi_ref.make_track(rng, n, gaps, tid=k + 1, start=int(rng.integers(0, 50))) for k, n in enumerate(lengths)], 0)


def _same(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape, what
    if got.tobytes() != ref.tobytes():
        bad = np.nonzero((got != ref).any(1))[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} rows differ, first frame/id {got[bad[0], :2]}, largest difference "
                             f"{np.abs(got - ref).max():.3e}")


@pytest.mark.parametrize("gaps", [False, True])
def test_every_path_boundary_equals_the_restatement(eng, gaps):
    rng = np.random.default_rng(7 + gaps)
    rows = _many(rng, _lengths(), gaps)
    got, st = gsi.smooth(rows, eng)
    ref, rst = gsi_ref.smooth(rows)
    assert st == rst and set(st.values()) == {0}
    _same(got, ref, f"gaps={gaps}")
    assert not np.array_equal(got[:, 2:6], gsi_ref._sorted(rows)[:, 2:6])     # something was smoothed


def test_halves_400_frames_apart_give_a_block_diagonal_kernel(eng):
    """n = 400 at tau = 10: l = 9.16, so every cross term has d d / (2 l l) >= 952 > 700 and is an exact zero."""
    r = gsi_ref.make_track(np.random.default_rng(11), 400)
    r[200:, 0] += 399
    l = gsi_ref.length_scale(400)
    assert r[200, 0] - r[199, 0] == 400 and 400.0 ** 2 / ((2.0 * l) * l) > 700 and (gsi_ref.kernel_matrix(r[:, 0], l)[:200, 200:] == 0.0).all()
    got, st = gsi.smooth(r, eng)
    ref, rst = gsi_ref.smooth(r)
    assert st == rst == {1: 0}
    _same(got, ref, "halves 400 apart")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "gsi_cases.npz"))


@pytest.mark.parametrize("name", ["c1024", "g1024"])
def test_golden_long_tracks(eng, golden, name):
    rows = case_rows(golden[f"{name}_frames"], golden[f"{name}_xyxy"])
    got, st = gsi.smooth(rows, eng)
    assert st == {1: 0}
    _same(got[:, 2:6], golden[f"{name}_out"], name)


def test_golden_1025_rows_pass_through_with_status_2(eng, golden):
    rows = case_rows(golden["p1025_frames"], golden["p1025_xyxy"])
    short = gsi_ref.make_track(np.random.default_rng(3), 40, tid=2)
    both = np.concatenate([rows, short], 0)
    got, st = gsi.smooth(both, eng)
    assert st == {1: 2, 2: 0}
    _same(got[got[:, 1] == 1], rows, "1025 rows")
    _same(got[got[:, 1] == 2], gsi_ref.smooth(short)[0], "the short track beside it")


def test_many_short_tracks_one_long_an_empty_one_and_any_order(eng):
    rng = np.random.default_rng(5)
    tracks = [gsi_ref.make_track(rng, 5, tid=k + 1, start=int(rng.integers(0, 200))) for k in range(300)]
    tracks.insert(150, gsi_ref.make_track(rng, 300, tid=1000))

    def call(order):
        """engine.gsi_smooth with the tracks in `order`, an empty track in the middle -> per track id its [n, 4] result"""
        lens = [len(tracks[k]) for k in order]
        lens.insert(len(lens) // 2, 0)
        ids = [int(tracks[k][0, 1]) for k in order]
        ids.insert(len(ids) // 2, -1)
        t = np.concatenate([tracks[k] for k in order], 0)
        off = np.concatenate([[0], np.cumsum(lens)])
        ls = [gsi_ref.length_scale(max(n, 1)) for n in lens]
        out, st = eng.gsi_smooth(off, t[:, 0], gsi_ref.tlwh(t), ls)
        assert (st == 0).all()
        return {i: out[off[k]:off[k + 1]] for k, i in enumerate(ids)}

    a = call(list(range(301)))
    b = call(list(rng.permutation(301)))
    assert len(a[-1]) == 0
    for tr in tracks:
        i = int(tr[0, 1])
        ref, st = gsi_ref.solve_track(tr[:, 0].astype(np.int64), gsi_ref.tlwh(tr), gsi_ref.length_scale(len(tr)))
        assert st == 0
        _same(a[i], ref, f"track {i}")
        _same(b[i], ref, f"track {i}, permuted call")


def test_more_long_tracks_than_scratch_slots(eng):
    """260 tracks of 193 .. 200 rows: the device-memory path has 256 slots, so four workgroups take a second track into their slot.
    The call equals the same tracks sent in two calls that need no second round, and the restatement on the tracks that share slots."""
    rng = np.random.default_rng(21)
    tracks = [gsi_ref.make_track(rng, 193 + k % 8, k % 3 == 0, tid=k + 1) for k in range(260)]
    assert all(len(t) > gsi.LDS_MAX for t in tracks)

    def call(sel):
        t = np.concatenate([tracks[k] for k in sel], 0)
        lens = [len(tracks[k]) for k in sel]
        off = np.concatenate([[0], np.cumsum(lens)])
        out, st = eng.gsi_smooth(off, t[:, 0], gsi_ref.tlwh(t), [gsi_ref.length_scale(n) for n in lens])
        assert (st == 0).all()
        return [out[off[k]:off[k + 1]] for k in range(len(sel))]

    whole = call(range(260))
    halves = call(range(130)) + call(range(130, 260))
    for k in range(260):
        _same(whole[k], halves[k], f"track {k}")
    # the call orders its tracks by falling length (stable): positions 0 .. 3 and 256 .. 259 of that order share slots 0 .. 3
    order = sorted(range(260), key=lambda k: -len(tracks[k]))
    for k in order[:4] + order[256:]:
        ref, st = gsi_ref.solve_track(tracks[k][:, 0].astype(np.int64), gsi_ref.tlwh(tracks[k]), gsi_ref.length_scale(len(tracks[k])))
        assert st == 0
        _same(whole[k], ref, f"track {k} against the restatement")


def test_zero_pivot_is_status_1_and_the_rows_pass_through(eng):
    rng = np.random.default_rng(9)
    bad, good = gsi_ref.make_track(rng, 2, tid=1), gsi_ref.make_track(rng, 30, tid=2)
    vals = np.concatenate([gsi_ref.tlwh(bad), gsi_ref.tlwh(good)], 0)
    frames = np.concatenate([bad[:, 0], good[:, 0]])
    ls = [1e9, 0.8]                                                           # (alpha = 0: the other track needs a well-conditioned K)
    out, st = eng.gsi_smooth([0, 2, 32], frames, vals, ls, alpha=0.0)
    assert gsi_ref.ss_expneg(1.0 / (2.0 * 1e9 * 1e9)) == 1.0                  # K is all ones: the second pivot is exactly 0
    r0, s0 = gsi_ref.solve_track(bad[:, 0].astype(np.int64), vals[:2], 1e9, 0.0)
    r1, s1 = gsi_ref.solve_track(good[:, 0].astype(np.int64), vals[2:], ls[1], 0.0)
    assert (s0, s1) == (1, 0) and list(st) == [1, 0]
    _same(out[:2], vals[:2], "status 1 passes through")
    _same(out[:2], r0, "as the restatement does")
    _same(out[2:], r1, "the other track is still smoothed")


def test_scratch_reuse_and_a_refused_call_between(eng):
    rng = np.random.default_rng(13)
    long_, short = gsi_ref.make_track(rng, 260, True), gsi_ref.make_track(rng, 200)
    for r in (long_, short, long_):                       # a short long-path call after a longer one: the slot is reused
        got, st = gsi.smooth(r, eng)
        assert st == {1: 0}
        _same(got, gsi_ref.smooth(r)[0], f"n={len(r)}")
    with pytest.raises(lib.SSError, match="track 1: frames must increase"):
        eng.gsi_smooth([0, 3, 6], [0, 1, 2, 5, 5, 6], np.ones((6, 4)), [1.0, 1.0])
    got, st = gsi.smooth(short, eng)
    assert st == {1: 0}
    _same(got, gsi_ref.smooth(short)[0], "after the refusal")
    eng.check_errors()


def _sequence_stack():
    z = np.load(os.path.join(GOLD, "jpeg_sequence.npz"))
    return np.stack([np.ascontiguousarray(z[f"rgb_{i}"][:, :, ::-1]) for i in range(12)])


def test_gsi_end_to_end_on_tracked_rows_with_gaps(eng):
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack")
    rows = np.concatenate([gsi.rows_of(res, k) for k, res in enumerate(model.track_stream(iter(_sequence_stack()), batch=4))], 0)
    model.close()
    assert len(rows) and rows.dtype == np.float64
    ids, counts = np.unique(rows[:, 1], return_counts=True)
    assert counts.max() >= 5, "the fixture should give at least one track of five frames"
    keep = np.ones(len(rows), bool)
    for tid in ids[counts >= 5]:                          # drop the third and fourth row of every longer track: a gap of 3 frames
        at = np.nonzero(rows[:, 1] == tid)[0]
        keep[at[np.argsort(rows[at, 0])][2:4]] = False
    cut = rows[~keep]
    rows = rows[keep]
    got, st = gsi.gsi(rows, eng)
    ref, rst = gsi_ref.gsi(rows)
    assert st == rst
    _same(got, ref, "gsi")
    assert len(got) >= len(rows) + len(cut) and (got[:, 6] == 0.0).sum() >= len(cut)        # the gaps were filled


def test_cli_writes_the_smoothed_labels_beside_the_untouched_labels(tmp_path):
    from strongsort_yolo_amd.yolo import YOLO
    src = tmp_path / "seq.npy"
    np.save(src, _sequence_stack())
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack")
    labels, outs = [], []
    for run, extra in (("a", {}), ("b", {"gsi": True})):
        out = cli.process_video({"source": str(src), "track": True, "count": False, "tracker": "bytetrack", "batch": 4, "random_init": True,
                                 "outdir": str(tmp_path / run), **extra}, model=model)
        assert out["frames"] == 12
        outs.append(out)
        labels.append((tmp_path / run / "seq_labels.txt").read_bytes())
        model._stream_pipe.reset_tracker(-1)
        model._frame_index = 0
    assert labels[0] == labels[1] and labels[0]
    assert not (tmp_path / "a" / "seq_labels_gsi.txt").exists() and "gsi_rows" not in outs[0]
    rows = np.concatenate([gsi.rows_of(res, k) for k, res in enumerate(model.track_stream(iter(_sequence_stack()), batch=4))], 0)
    model.close()
    ref, rst = gsi_ref.gsi(rows)
    assert (tmp_path / "b" / "seq_labels_gsi.txt").read_text() == gsi_ref.label_lines(ref)
    assert outs[1]["gsi_rows"] == len(ref) and outs[1]["gsi_status"] == {k: sum(1 for v in rst.values() if v == k) for k in (0, 1, 2)}
