"""The crowded scenes of tests/byte_crowd.py on the CPU references alone: every scene must put the references' SciPy calls into
the regimes that tests/test_gpu_byte_crowd.py is there for (docs/BYTETRACK.md §5) — more than 64 and more than 128 rows, more
tracks than rows, more than SS_BYTE_COST_CAP = 2048 entries in the first, second and third association, a saturated table — so
that a later edit of a generator cannot quietly shrink them back under 64 x 64.  The floors are conditions on the inputs: they
are counted on the reference and never on the device."""
import numpy as np
import pytest

from tests import byte_crowd as bc
from tests.bytetrack_ref import iou_cost


def _calls(run, stage=None):
    """(n_rows, n_cols, entries below 1.0) of the run's linear_sum_assignment calls, of one association (0, 1, 2) or of all."""
    return [(r, c, b) for _, s, r, c, b, _, _ in run.calls if stage is None or s == stage]


@pytest.mark.parametrize("variant", bc.VARIANTS)
def test_two_crowds_reach_the_tall_spilled_forms_in_all_three_associations(variant):
    """Counted on every variant's own reference (seed 0): 32 calls, 19 of them 240 x 51 ... 120 (the pool of both crowds against
    one crowd's high rows), one third association of 120 x 120, eight second associations of 50 x 50 ... 69 x 69; the GMC, ReID and
    pose references give the same counts as the plain ones, so all five variants keep the same floors."""
    run = bc.reference("two_crowds", variant)
    assert not run.ref.capacity_error
    assert sum(r > c and r > 128 for r, c, _ in _calls(run)) >= 15
    assert sum(r > c and r > 128 and c > 64 for r, c, _ in _calls(run, 0)) >= 10      # ... of them past 64 columns after the transposition
    assert sum(r * c > bc.COST_CAP for r, c, _ in _calls(run, 2)) >= 1
    assert sum(r * c > bc.COST_CAP for r, c, _ in _calls(run, 1)) >= 3
    assert (len(run.ref.tracked), len(run.ref.lost), run.ref.next_id) == (120, 120, 241)
    assert max(len(d) for d in run.scene.frames) <= 128


@pytest.mark.parametrize("variant", bc.VARIANTS)
def test_twin_crowds_tie_exactly_below_the_threshold_in_the_tall_form(variant):
    """Counted on every variant's reference (seed 0): frame 4's first association is 248 x 120 with 8 tracks that repeat another
    track's cost row exactly, each with an entry below 1.0 (its own box is back); the floors are 80 % of the counts, rounded down.
    The twin that SciPy picks carries on under its id; the other one stays lost."""
    run = bc.reference("twin_crowds", variant)
    assert not run.ref.capacity_error
    tall = [c for c in run.calls if c[1] == 0 and c[2] > c[3] and c[2] > 128 and c[2] * c[3] > bc.COST_CAP]
    assert len(tall) >= 2                                          # counted: 3
    assert max(c[5] for c in tall) >= 6                            # counted: 8 tied rows
    assert any(c[4] >= 102 for c in tall if c[5] >= 6)             # counted: 128 entries below 1.0 in that matrix
    assert max(len(d) for d in run.scene.frames) <= 128


@pytest.mark.parametrize("variant", bc.VARIANTS)
def test_dense_crowd_is_a_real_optimisation_past_the_lds_matrix(variant):
    """Counted (seed 0): 19 of 48 calls above 2048 entries on every variant; the largest matrix is 100 x 84 with 244 entries below
    1.0 (pose: 101 x 84 with 247).  All of them clear the floors of the plain variants, which therefore hold for every variant."""
    run = bc.reference("dense_crowd", variant)
    assert not run.ref.capacity_error
    calls = _calls(run)
    assert sum(r * c > bc.COST_CAP for r, c, _ in calls) >= 15
    assert max(calls, key=lambda x: x[0] * x[1])[2] >= 200
    assert any(r > c > 64 for r, c, _ in calls)                    # tall, and past 64 columns after the transposition
    assert max(len(d) for d in run.scene.frames) <= 128


def test_dense_crowd_duplicates_tie_exactly():
    frames = bc.dense_crowd(0)
    for k, d in enumerate(frames):
        n_dup = len(d) - len({r.tobytes() for r in d})
        assert n_dup == (8 if k % 4 == 3 else 0), k
    d = frames[3]
    tl = np.column_stack([d[:, :2], d[:, 2:4] - d[:, :2]]).astype(np.float64)
    below = (iou_cost(tl, tl) < 1.0).sum(1)
    assert below.min() >= 2 and np.median(below) >= 3              # every box overlaps a neighbour (and itself)


def test_three_crowds_saturate_the_table():
    """Counted (seed 0): the third crowd finds 200 live tracks and gets 56 births; the first crowd's return is a 256 x 100 first
    association; 100 tracked and 156 lost at the end."""
    run = bc.reference("three_crowds", "xyah")
    assert run.ref.capacity_error
    assert len(run.ref.tracked) + len(run.ref.lost) == run.scene.cfg.max_tracks == 256
    assert any(r == 256 and c >= 80 for r, c, _ in _calls(run, 0))


@pytest.mark.parametrize("size", bc.BOUNDARY_SIZES)
def test_boundary_pair_has_exactly_the_stated_first_association(size):
    for variant in ("xyah", "xywh") + (("reid",) if size in bc.SPILL_EDGE_SIZES else ()):
        run = bc.reference("boundary_pair", variant, 0, size)
        assert [c[:4] for c in run.calls] == [(1, 0, size[0], size[1])], variant
        assert run.calls[0][4] == min(size)                        # one entry below the plateau per box that is still there
        assert not run.ref.capacity_error and len(run.rows[1]) == min(size)
    assert (size[0] * size[1] > bc.COST_CAP) == (size != (32, 64))


def test_scenes_are_seeded_and_the_crowds_never_overlap():
    for gen in (bc.two_crowds, bc.twin_crowds, bc.dense_crowd, bc.three_crowds):
        a, b, c = gen(3), gen(3), gen(4)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and any(x.tobytes() != y.tobytes() for x, y in zip(a, c))
        assert all(x.dtype == np.float32 and x.shape[1] == 6 for x in a)
    frames = bc.two_crowds(0)
    tl = [np.column_stack([d[:, :2], d[:, 2:4] - d[:, :2]]).astype(np.float64) for d in frames]
    assert (iou_cost(tl[2], tl[3]) == 1.0).all() and (iou_cost(tl[2], tl[2]) == 1.0).sum() == 120 * 119     # A x B: the plateau
    low = [int(((d[:, 4] > 0.1) & (d[:, 4] < 0.25)).sum()) for d in frames]
    assert all((n > 40) == (k % 3 == 2) and (n == 0) == (k % 3 != 2) for k, n in enumerate(low))


def test_camera_moves_the_boxes_with_the_accumulated_warp():
    frames = bc.two_crowds(0)
    w, moved = bc.camera(0, frames)
    assert (w[::5, 6] == -1).all() and (np.delete(w[:, 6], np.s_[::5]) >= 1).all()
    assert moved[0].tobytes() == frames[0].tobytes()               # no warp yet
    assert all(np.allclose(m[:, 2:4] - m[:, :2], (44.0, 30.0), atol=1e-3) for m in moved)
    assert max(np.abs(m[:, :2] - d[:, :2]).max() for m, d in zip(moved, frames)) > 8.0
