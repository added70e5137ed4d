"""The C oracle's NMS against a plain float64 NMS and against answers known from the definition (docs: tests/front_fields.py).

tests/test_gpu_front_edges.py compares the device with the oracle bit for bit on the same fields; this file is what says that the
oracle (float32, class offset cls * max_wh added to the boxes) computes a correct NMS on them, and that the fields reach the paths the
GPU tests name: no IoU of a decided pair lies closer to the threshold than the offset's rounding can move it, the large fields run the
greedy pass to their last block, the dense ones hit every cap up to 1024."""
import functools

import numpy as np
import pytest

from oracle import cexact
from tests import front_fields as ff

CONF, IOU, MAX_WH, MAX_NMS = 0.3, 0.4, 7680.0, 8192


@functools.lru_cache(maxsize=None)
def _field(n, per):
    pred = ff.field(n, per)
    pred.setflags(write=False)
    return pred


@pytest.mark.parametrize("max_det", [1000, 300])
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("n,per", ff.FIELD_PAIRS)
def test_oracle_nms_is_the_plain_nms(n, per, agnostic, max_det):
    """Margins: adding cls * 7680 in float32 moves a 40-pixel side by up to 4.9e-4 px and an IoU near 0.4 by about 2e-5, so a decided
    pair at least 1e-4 from the threshold (1e-5 without the offset: only the float32 rounding of the IoU itself, ~1e-7) is decided the
    same way by both.  The suppressed-past-rank-4096 condition is asserted where the pass is not cut short by max_det (the per = 24
    fields at max_det = 1000); on the dense fields and at max_det = 300 the pass ends at the cap before rank 4096 by construction."""
    pred = _field(n, per)
    assert int(np.count_nonzero(pred[4:].max(axis=0) > np.float32(CONF))) == n
    keep, _ = cexact.nms(pred, 2, CONF, IOU, agnostic, MAX_WH, MAX_NMS, max_det)
    pkeep, margin = ff.plain_nms(pred, 2, CONF, IOU, agnostic, max_det)
    print(f"n={n} per={per} agnostic={agnostic} max_det={max_det}: kept {len(keep)}, margin {margin:.3e}")
    assert np.array_equal(keep, pkeep)
    assert margin >= (1e-5 if agnostic else 1e-4)
    if per == 24:
        assert len(keep) < 1000                                      # at max_det = 1000 the scan runs to the last block
        if n >= 4097 and max_det == 1000:
            assert ff.suppressed_past(pred, 2, CONF, keep, max_det) >= 1
    if (n, per) in ((8192, 5), (5000, 4)):
        assert len(keep) == max_det
        full, _ = cexact.nms(pred, 2, CONF, IOU, agnostic, MAX_WH, MAX_NMS, n)
        assert len(full) >= 1024                                     # every cap up to the engine's 1024 is hit


def _run(case, agnostic=False):
    keep, rows = cexact.nms(case["pred"], case["nc"], case["conf"], case["iou"], agnostic, MAX_WH, MAX_NMS, 1000)
    return keep.tolist(), rows[:, 5].astype(int).tolist()


@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("case", ff.known_answers(), ids=lambda c: c["name"])
def test_oracle_known_answers(case, pad):
    case = ff.padded(case) if pad else case
    keep, cls = _run(case)
    assert keep == case["keep"] and cls == case["cls"]
    pkeep, _ = ff.plain_nms(case["pred"], case["nc"], case["conf"], case["iou"], False, 1000)
    assert pkeep.tolist() == case["keep"]


def test_known_answer_fields_are_what_they_claim():
    """the IoU of the two boxes is exactly 0.5 in float32 arithmetic, with and without the class-1 offset"""
    for off in (np.float32(0), np.float32(7680)):
        a = np.array([1.5 - 1.5, 0.5 - 0.5, 1.5 + 1.5, 0.5 + 0.5], np.float32) + off
        b = np.array([2.5 - 1.5, 0.5 - 0.5, 2.5 + 1.5, 0.5 + 0.5], np.float32) + off
        iw = np.float32(min(a[2], b[2]) - max(a[0], b[0])); ih = np.float32(min(a[3], b[3]) - max(a[1], b[1]))
        inter = np.float32(iw * ih)
        aa = np.float32((a[2] - a[0]) * (a[3] - a[1])); ab = np.float32((b[2] - b[0]) * (b[3] - b[1]))
        assert np.float32(inter / np.float32(aa + ab - inter)) == np.float32(0.5)
    names = [c["name"] for c in ff.known_answers()]
    assert len(set(names)) == len(names) == 8
