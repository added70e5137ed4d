"""The scenes of tests/strongsort_crowd.py reach what their docstrings claim — from the oracle alone, no GPU.  These are conditions on
the inputs: tests/test_gpu_strongsort_crowd.py relies on them and does not re-derive them from the device."""
import numpy as np
import pytest

from oracle.strongsort_np import OracleStrongSort
from tests import strongsort_crowd as sc
from tests.strongsort_crowd import COST_CAP, EDGE_SIZES, MAX_DETS, MAX_TRACKS, edge_args, reference, solver_form

ALL = ([("two_crowds", 0), ("two_crowds", 1), ("dense_crowd", 0), ("dense_crowd", 1), ("churn", 0, 5), ("churn", 0, 6), ("overflow", 0), ("sparse", 5)]
       + [("edge_scene", *edge_args(*s)) for s in EDGE_SIZES])


@pytest.mark.parametrize("case", ALL, ids=lambda c: "-".join(str(x) for x in c))
def test_frames_fit_the_device_tables(case):
    """At most 128 rows a frame, unit features, boxes inside 1920 x 1080, a capacity error only where the scene is about one."""
    run = reference(*case)
    for d, f in run.frames:
        assert d.dtype == np.float32 and f.dtype == np.float32 and d.shape == (len(d), 6) and f.shape == (len(d), 512)
        assert len(d) <= MAX_DETS
        assert np.allclose(np.linalg.norm(f.astype(np.float64), axis=1), 1.0, atol=1e-6)
        assert (d[:, :2] >= 0).all() and (d[:, 2] < sc.W).all() and (d[:, 3] < sc.H).all() and (d[:, 2:4] > d[:, :2]).all()
    assert max(run.n_tracks) <= MAX_TRACKS
    assert run.orc.capacity_error == (case[0] == "overflow")
    assert len(run.frames) <= 12


@pytest.mark.parametrize("seed", [0, 1])
def test_two_crowds_record(seed):
    run = reference("two_crowds", seed)
    assert all(len(d) == 128 for d, _ in run.frames)
    assert run.n_tracks == [128, 128, 128, 256, 256, 256, 256, 256, 256]
    a, b = [s[0] for s in run.stages], [s[1] for s in run.stages]
    assert a[:3] == [(0, 128, 0)] * 3 and a[3:6] == [(128, 128, 1)] * 3 and a[6:] == [(256, 128, 2)] * 3
    assert [b[k] for k in (1, 2, 4, 5)] == [(128, 128, 2)] * 4
    assert all(b[k][2] != 2 for k in (0, 3, 6, 7, 8))
    # 256 x 128: transposed, spilled, the four-column form; 128 x 128: spilled, the two-column form
    assert 256 * 128 > COST_CAP and 128 * 128 > COST_CAP and solver_form(256, 128) == 4 and solver_form(128, 128) == 2
    # the exact twins of each crowd's first frame: tied rows in the next frame's stage B, and SciPy's order is not the naive one
    for k in (1, 4):
        seen, flips = sc.tie_flips(type(run)(lasts=[run.lasts[k]]))
        assert seen == 8 and 0 < flips, (k, seen, flips)
    assert sc.lsap_shapes(run) == ((256, 128), (128, 128))


def test_edge_sizes_cover_the_code_paths():
    """EDGE_SIZES against lsap_wave's dispatch and k_frame's spill condition, restated in solver_form / COST_CAP."""
    got = {(solver_form(t, d), d < t) for t, d in EDGE_SIZES}
    assert got == {(1, False), (1, True), (2, False), (2, True), (4, True)}          # (4, False) would need more than 128 detections
    assert (96, 128) in EDGE_SIZES and 96 * 128 == COST_CAP and (97, 128) in EDGE_SIZES
    # both sides of each form edge, in both orientations (a frame has no 129 detections)
    assert {(64, 64), (65, 64), (64, 65), (128, 65), (128, 128), (129, 128)} <= set(EDGE_SIZES)
    assert (MAX_TRACKS, MAX_DETS) in EDGE_SIZES


@pytest.mark.parametrize("size", EDGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edge_scene_record(size):
    T, d = size
    n_a, n_b, _ = edge_args(T, d)
    run = reference("edge_scene", n_a, n_b, d)
    assert [len(x) for x, _ in run.frames] == [n_a] * 3 + [n_b] * 3 + [d]
    assert run.n_tracks[:6] == [n_a] * 3 + [T] * 3
    assert run.stages[6][0] == (T, d, 2)
    assert all(s[0][2] != 2 for s in run.stages[:6])                               # the only stage A LSAP is the last frame's
    assert run.stages[1][1] == (n_a, n_a, 2) and run.stages[2][1] == (n_a, n_a, 2)  # the exact copy: tied rows and columns in stage B
    seen, flips = sc.tie_flips(type(run)(lasts=[run.lasts[6]]))
    assert seen >= 1                                                               # two tracks equal in every bit, both matched
    if T <= d:
        assert flips >= 1
    ok = ~(run.lasts[6]["cost_a"] > run.cfg.max_dist)
    assert ok.sum(1).max() == 2 and ok.sum(0).max() == 2                           # the ambiguity is the twins', nothing else's


@pytest.mark.parametrize("seed", [0, 1])
def test_dense_crowd_record(seed):
    run = reference("dense_crowd", seed)
    assert len(run.frames[0][0]) == 128 and all(len(d) == 120 for d, _ in run.frames[1:])
    assert run.stages[1] == ((0, 120, 0), (128, 120, 2)) and run.stages[2][0][2] == 0 and run.stages[2][1][2] == 2
    both = [k for k, (a, b) in enumerate(run.stages) if a[2] == 2 and b[2] == 2]
    assert len(both) >= 3 and min(both) >= 3                                        # after confirmation: an LSAP in both stages of a frame
    # exact duplicates among the rows of every later frame
    for d, _ in run.frames[1:]:
        assert len(d) - len(np.unique(d, axis=0)) == 4
    a = [s[0] for s in run.stages]
    assert any(r > c and r * c > COST_CAP and p == 2 for r, c, p in a)                # a tall spilled stage A on the two-column form
    assert any(r <= c and r * c > COST_CAP and p == 2 for r, c, p in a)               # and a wide one
    assert 128 < max(run.n_tracks) < MAX_TRACKS


@pytest.mark.parametrize("max_age", [5, 6])
def test_churn_record(max_age):
    run = reference("churn", 0, max_age)
    if max_age == 5:
        assert run.n_tracks == [85] * 3 + [170] * 3 + [255, 255, 170, 255, 255, 170]
    else:
        assert run.n_tracks == [85] * 3 + [170] * 3 + [255] * 6
        assert run.stages[9][0][:2] == (255, 85)                                    # 255 confirmed tracks enter frame 9 ...
        ids = run.orc.snapshot()["track_id"]
        assert run.orc.next_id == 341 and ids.min() == 86                           # ... 85 die and 85 are born in it
    assert max(run.n_tracks) == 255 and not run.orc.capacity_error
    assert all(p != 2 for st in run.stages for _, _, p in st)                        # unambiguous throughout: the shortcut, not the LSAP


def test_overflow_record():
    run = reference("overflow", 0)
    assert run.n_tracks == [100] * 3 + [200] * 3 + [256] * 3 and run.orc.capacity_error
    assert len(run.rows[8]) == 56 and run.orc.next_id == 257
    # the 56 births of frame 6 are its 56 lowest unmatched detection indices: all rows are unmatched, so rows 0 .. 55
    born = [t for t in run.orc.tracks if t.track_id > 200]
    assert [t.track_id for t in born] == list(range(201, 257))
    unlimited = OracleStrongSort(run.cfg, "c")
    for d, f in run.frames[:7]:
        unlimited.update(d, f, (sc.H, sc.W))
    assert len(unlimited.tracks) == 300 and not unlimited.capacity_error          # max_tracks=None keeps the behaviour without a limit
    first56 = {t.track_id: t for t in unlimited.tracks if 200 < t.track_id <= 256}
    lim = OracleStrongSort(run.cfg, "c", max_tracks=MAX_TRACKS)
    for d, f in run.frames[:7]:
        lim.update(d, f, (sc.H, sc.W))
    assert lim.capacity_error and len(lim.tracks) == 256
    for t in lim.tracks[200:]:
        assert t.det_idx == first56[t.track_id].det_idx == t.track_id - 201 and np.array_equal(t.mean, first56[t.track_id].mean)


def test_capacity_model_counts_the_slots_freed_in_the_frame():
    """Survivors plus births against the capacity: tracks that die in a frame make room for that frame's births."""
    run = reference("churn", 0, 6)
    lim = OracleStrongSort(run.cfg, "c", max_tracks=255)
    for d, f in run.frames:
        lim.update(d, f, (sc.H, sc.W))
    assert not lim.capacity_error and len(lim.tracks) == 255
    lim = OracleStrongSort(run.cfg, "c", max_tracks=200)
    for d, f in run.frames[:7]:
        lim.update(d, f, (sc.H, sc.W))
    assert lim.capacity_error and len(lim.tracks) == 200 and lim.next_id == 201


class _OtherTies:
    """The oracle's numerics with another tie order in the LSAP: the same solver on the matrix with its rows, its columns or both
    reversed.  Its assignment costs the same, so it is as optimal as SciPy's; only ties come out differently."""

    def __init__(self, nx, rows=True, cols=True):
        self.nx, self.sr, self.sc = nx, -1 if rows else 1, -1 if cols else 1

    def __getattr__(self, name):
        return getattr(self.nx, name)

    def lsap(self, cost):
        r, c = self.nx.lsap(np.ascontiguousarray(cost[::self.sr, ::self.sc]))
        r = cost.shape[0] - 1 - np.asarray(r) if self.sr < 0 else np.asarray(r)
        c = cost.shape[1] - 1 - np.asarray(c) if self.sc < 0 else np.asarray(c)
        o = np.argsort(r)
        return r[o], c[o]


@pytest.mark.parametrize("case", [("two_crowds", 0), ("dense_crowd", 0), ("edge_scene", *edge_args(256, 128)), ("edge_scene", *edge_args(128, 128)),
                                  ("edge_scene", *edge_args(64, 64)), ("edge_scene", *edge_args(200, 3))], ids=lambda c: "-".join(str(x) for x in c))
def test_rows_depend_on_the_tie_order(case):
    """The tie order shows in the rows: an oracle whose LSAP breaks ties differently (and is otherwise as optimal) reports other
    (track id, detection) pairs on these scenes — so a device solver with a wrong tie rule cannot equal the reference's rows.
    (Which reversal shows depends on the orientation: a pair of equal rows is symmetric under some of them.)"""
    run = reference(*case)
    differ = {}
    for flip in ((True, True), (True, False), (False, True)):
        other = OracleStrongSort(run.cfg, "c", max_tracks=MAX_TRACKS)
        other.nx = _OtherTies(other.nx, *flip)
        differ[flip] = 0
        for k, (d, f) in enumerate(run.frames):
            rows = other.update(d, f, (sc.H, sc.W))
            differ[flip] += rows.shape != run.rows[k].shape or rows.tobytes() != run.rows[k].tobytes()
    print(case, differ)
    assert max(differ.values()) >= 1


def test_other_tie_order_is_as_optimal():
    run = reference("two_crowds", 0)
    nx = _OtherTies(run.orc.nx)
    for k in (4, 6):
        for cost in (run.lasts[k]["cost_a"], run.lasts[k]["cost_b"]):
            if cost.size:
                r0, c0 = run.orc.nx.lsap(cost)
                r1, c1 = nx.lsap(cost)
                assert len(r0) == len(r1) and len(set(c1.tolist())) == len(c1)
                assert abs(cost[r0, c0].sum() - cost[r1, c1].sum()) < 1e-9
