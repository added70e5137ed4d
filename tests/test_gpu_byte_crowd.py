"""The BYTE tracker family on crowded frames (csrc/ss_byte.hip, docs/BYTETRACK.md §5) against its CPU references, bit for bit:
the scenes of tests/byte_crowd.py put the three associations past 64 and 128 rows, into the transposed orientation, past the
LDS-resident cost matrix into the stream's spill area and onto the solver's 128- and 256-column forms, in the xyah, xywh, GMC,
ReID and pose kernels; tests/test_byte_crowd_cpu.py asserts that the scenes reach those regimes.  Every frame's rows and, at
the end, the track table (with the smoothed features / stored poses) are compared; the engine is driven as in the family's
own device tests."""
import numpy as np
import pytest
import torch

from tests import byte_crowd as bc
from tests import test_gpu_botsort_gmc as gmc_t
from tests import test_gpu_botsort_pose as pose_t
from tests import test_gpu_botsort_reid as reid_t
from tests import test_gpu_bytetrack as byte_t
from tests.test_gpu_bytetrack import _assert_rows

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _assert_table(eng, s, ref, what):
    if eng.reid:
        return reid_t._assert_table(eng, s, ref, what)            # ... and the smoothed features
    if eng.pose:
        return pose_t._assert_table(eng, s, ref, what)            # ... and the stored poses
    t = eng.tracks(s)
    ids, st, act, mean = ref.tracks()
    assert t["n_tracked"] == len(ref.tracked) and t["n_lost"] == len(ref.lost) and t["next_id"] == ref.next_id, what
    assert np.array_equal(t["track_id"], ids) and np.array_equal(t["state"], st) and np.array_equal(t["activated"], act), what
    assert t["mean"].tobytes() == mean.tobytes(), f"{what}: track means"


def _drive(scenes, group):
    """One engine, one stream per scene (all of one variant and length), update_group calls of `group` frames.
    -> (engine, per stream the list of rows)"""
    from strongsort_yolo_amd.engine import ByteTrackEngine
    v = scenes[0].variant
    eng = ByteTrackEngine(scenes[0].cfg, len(scenes), 0)
    if v == "reid":
        got = reid_t._run_engine(eng, [list(zip(sc.frames, sc.side)) for sc in scenes], group)
    elif v == "pose":
        got = pose_t._run_engine(eng, [list(zip(sc.frames, sc.side)) for sc in scenes], group)
    elif v == "gmc":
        got = gmc_t._run_engine(eng, [sc.frames for sc in scenes], group, np.stack([sc.warps for sc in scenes], 1))
    else:
        got = byte_t._run_engine(eng, [sc.frames for sc in scenes], group)
    return eng, got


def _check(runs, group, what):
    eng, got = _drive([r.scene for r in runs], group)
    try:
        for s, run in enumerate(runs):
            assert len(got[s]) == len(run.rows)
            for k, exp in enumerate(run.rows):
                _assert_rows(got[s][k], exp, f"{what}, group {group}, stream {s} frame {k}")
            _assert_table(eng, s, run.ref, f"{what}, group {group}, stream {s}")
    finally:
        eng.close()


@pytest.mark.parametrize("variant", bc.VARIANTS)
def test_two_crowds_equal_reference_in_every_group_size(variant):
    """240 pool tracks x 51 ... 120 high rows (transposed, spilled, the 256-column form), a third association of 120 x 120 and second
    associations of 50 x 50 ... 69 x 69, both spilled; groups of 1, 5 and 24 frames move where the table crosses LDS and global
    memory, and all equal the one reference, so their rows are identical."""
    run = bc.reference("two_crowds", variant)
    for group in (24, 5, 1):
        _check([run], group, f"two_crowds {variant}")


@pytest.mark.parametrize("variant", bc.VARIANTS)
def test_twin_crowds_equal_reference(variant):
    """248 pool tracks x 120 rows with eight pairs of exactly tied tracks whose shared entry lies below match_thresh: the tie order of
    the 256-column form, through the transposition, decides which twin's id the rows carry."""
    _check([bc.reference("twin_crowds", variant)], 6, f"twin_crowds {variant}")


@pytest.mark.parametrize("variant", bc.VARIANTS)
def test_dense_crowd_equals_reference(variant):
    """About 100 pool tracks x 60 ... 84 high rows with three or so entries below 1 per column and exactly tied duplicate columns."""
    _check([bc.reference("dense_crowd", variant)], 20, f"dense_crowd {variant}")


@pytest.mark.parametrize("size", bc.BOUNDARY_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_boundary_pairs_equal_reference(size):
    """The last LDS-resident first association (32 x 64 = 2048 entries), the first spilled ones, and both orientations across the
    64- and 128-column edges of the solver's forms; the four sizes around 2048 on the ReID cost path as well."""
    for variant in ("xyah", "xywh") + (("reid",) if size in bc.SPILL_EDGE_SIZES else ()):
        _check([bc.reference("boundary_pair", variant, 0, size)], 2, f"boundary_pair {size} {variant}")


def test_three_crowds_fill_the_table_and_report_capacity():
    from strongsort_yolo_amd import lib
    from strongsort_yolo_amd.engine import ByteTrackEngine
    run = bc.reference("three_crowds", "xyah")
    assert run.ref.capacity_error
    frames = run.scene.frames
    F = len(frames)
    eng = ByteTrackEngine(run.scene.cfg, 1, 0)
    hd, hn = np.zeros((F, 1, 128, 6), np.float32), np.zeros((F, 1), np.int32)
    for f, d in enumerate(frames):
        hd[f, 0, :len(d)], hn[f, 0] = d, len(d)
    out, nout = torch.zeros(F, 1, 256, 8, device=DEV), torch.zeros(F, 1, dtype=torch.int32, device=DEV)
    eng.update_group(F, torch.from_numpy(hd).to(DEV), torch.from_numpy(hn).to(DEV), None, None, out, nout)
    with pytest.raises(lib.SSError) as ei:
        eng.check_errors()
    assert ei.value.code == lib.SS_ERR_CAPACITY
    ho, hno = out.cpu().numpy(), nout.cpu().numpy()
    for k, exp in enumerate(run.rows):                             # births beyond 256 tracks are dropped as the reference drops them
        _assert_rows(ho[k, 0, :hno[k, 0]], exp, f"three_crowds frame {k}")
    _assert_table(eng, 0, run.ref, "three_crowds")
    t = eng.tracks(0)
    assert t["n_tracked"] + t["n_lost"] == 256
    eng.close()


def test_three_crowded_streams_side_by_side():
    """Three workgroups with their spill areas in use together: two seeds of two_crowds around a dense crowd."""
    runs = [bc.reference("two_crowds", "xywh"), bc.reference("dense_crowd", "xywh", 1, None, 24), bc.reference("two_crowds", "xywh", 1)]
    _check(runs, 24, "three streams")
