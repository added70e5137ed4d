"""The front end (csrc/ss_front.hip) at its edges, through the C ABI: both NMS launch forms (ss_set_option "nms_fused" 1 / 0) at the
candidate counts where the sort, the bit matrix and the greedy scan change shape, at the capacity, at every max_det cap, on a stale
workspace, at class counts around the filter's loop bounds; the packed crop form and ss_unpack_feats against the oracle's crops.

References: oracle/cexact (bit for bit), tests/front_fields.plain_nms (float64, independent of the oracle) and the known answers of
tests/front_fields.py; tests/test_front_edges_cpu.py holds the proofs about the fields themselves (margins, kept counts)."""
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

from oracle import cexact
from strongsort_yolo_amd.config import DetectConfig
from strongsort_yolo_amd.lib import SSError, SS_ERR_CAPACITY
from tests import front_fields as ff
from tests.gpu_util import engine, bits_equal

pytestmark = pytest.mark.gpu

FORMS = [0, 1]
FORM_IDS = ["four_launches", "fused"]


@pytest.fixture(scope="module")
def eng():
    e = engine(debug=False)
    yield e
    e.set_option("nms_fused", 1)
    e.close()


@pytest.fixture(params=FORMS, ids=FORM_IDS)
def fused(request, eng):
    """the option is process-wide: whatever the test does, the default form is back afterwards"""
    eng.set_option("nms_fused", request.param)
    yield request.param
    eng.set_option("nms_fused", 1)


# ---- references, computed once and shared by both forms ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _field(n, per=None):
    pred = ff.field(n, per)
    pred.setflags(write=False)
    return pred


@functools.lru_cache(maxsize=None)
def _oracle(n, per, agnostic, max_det):
    d = DetectConfig()
    return cexact.nms(_field(n, per), 2, d.conf, d.iou, agnostic, d.max_wh, d.max_nms, max_det)


@functools.lru_cache(maxsize=None)
def _plain(n, per, agnostic, max_det):
    d = DetectConfig()
    return ff.plain_nms(_field(n, per), 2, d.conf, d.iou, agnostic, max_det)[0]


def _oracle_of(pred, nc, dcfg, geom, max_det=None, classes=None):
    rkeep, rrows = cexact.nms(pred, nc, dcfg.conf, dcfg.iou, dcfg.agnostic_nms, dcfg.max_wh, dcfg.max_nms,
                              min(dcfg.max_det, 1024) if max_det is None else max_det, classes=classes)
    return rkeep, cexact.scale_boxes(rrows, *geom)


GEOM1 = (1.0, 0.0, 0.0, 4096, 4096)


def _run(eng, pred, nc, dcfg, geom=GEOM1, **kw):
    rows, keep, count = eng.nms(torch.tensor(pred).to(eng.device), nc, dcfg, *geom, **kw)
    k = int(count.item())
    return rows.cpu().numpy(), keep.cpu().numpy(), k


def _check(got, ref):
    rows, keep, k = got
    rkeep, rrows = ref
    assert k == len(rkeep)
    assert np.array_equal(keep[:k], rkeep)
    assert bits_equal(rows[:k, :6], rrows)


# ---- candidate counts ----------------------------------------------------------------------------------------------------------------
COUNTS = [0, 1, 63, 64, 65, 128, 129, 1024, 1025, 4095, 4096, 4097, 8191, 8192]


@pytest.mark.parametrize("n_cand", COUNTS)
@pytest.mark.parametrize("agnostic", [False, True])
def test_nms_candidate_counts_both_forms(eng, fused, agnostic, n_cand):
    """One wave (<= 64), one 64-block more, the sort's power-of-two padding (1024 / 1025), the second removed-word register of the
    scan (> 4096: blocks 64..127) and the last candidate the workspace holds (8192).  Above 4096 the fields keep 342..686 rows, so
    the scan walks every block, and rows of rank >= 4096 are suppressed by rows of the first blocks (test_front_edges_cpu.py)."""
    dcfg = replace(DetectConfig(), agnostic_nms=agnostic)
    per = ff.PER_OF(n_cand)
    got = _run(eng, _field(n_cand, per), 2, dcfg)
    rkeep, rrows = _oracle(n_cand, per, agnostic, 1000)
    _check(got, (rkeep, cexact.scale_boxes(rrows, *GEOM1)))
    assert np.array_equal(got[1][:got[2]], _plain(n_cand, per, agnostic, 1000))
    assert (got[2] > 0) == (n_cand > 0)
    eng.check_errors()


@pytest.mark.parametrize("agnostic", [False, True])
def test_nms_large_path_scaled_and_clamped(eng, fused, agnostic):
    """4097 candidates mapped back with gain 0.5 and pads (3, 12) into 1280 x 720: the field spans 3000 px, most rows clamp"""
    dcfg = replace(DetectConfig(), agnostic_nms=agnostic)
    geom = (0.5, 3.0, 12.0, 1280, 720)
    got = _run(eng, _field(4097, 24), 2, dcfg, geom)
    rkeep, rrows = _oracle(4097, 24, agnostic, 1000)
    rrows = cexact.scale_boxes(rrows, *geom)
    _check(got, (rkeep, rrows))
    assert np.any(rrows[:, 2] == 1280) and np.any(rrows[:, 3] == 720) and np.any(rrows[:, 2] < 1280)
    eng.check_errors()


# ---- capacity ------------------------------------------------------------------------------------------------------------------------
def test_nms_capacity_edge(eng, fused):
    dcfg = DetectConfig()
    _check(_run(eng, _field(8192, 24), 2, dcfg), _oracle_of(_field(8192, 24), 2, dcfg, GEOM1))
    eng.check_errors()
    pred = _field(8193, 24)
    assert int(np.count_nonzero(pred[4:].max(axis=0) > np.float32(dcfg.conf))) == 8193
    try:
        rows, keep, k = _run(eng, pred, 2, dcfg)
        assert k == 0
        with pytest.raises(SSError) as ei:
            eng.check_errors()
        assert ei.value.code == SS_ERR_CAPACITY
    finally:
        eng.reset(-1)
    eng.check_errors()
    _check(_run(eng, _field(65), 2, dcfg), _oracle_of(_field(65), 2, dcfg, GEOM1))      # the workspace is usable again
    eng.check_errors()


def test_nms_capacity_in_a_batch(eng, fused):
    """the overflowing image yields nothing and raises; its neighbours in the same launch are untouched"""
    dcfg = DetectConfig()
    preds = [_field(5000, 4), _field(8193, 24), _field(65)]
    G = torch.tensor([GEOM1] * 3, dtype=torch.float32, device=eng.device)
    P = torch.from_numpy(np.stack(preds)).to(eng.device)

    def check(rows, keep, count, imgs):
        rows, keep, count = rows.cpu().numpy(), keep.cpu().numpy(), count.cpu().numpy()
        for b, i in enumerate(imgs):
            _check((rows[b], keep[b], int(count[b])), _oracle_of(preds[i], 2, dcfg, GEOM1))
        return count
    try:
        rows, keep, count = eng.nms_batch(P, 2, dcfg, G)
        assert int(count[1].item()) == 0
        check(rows[[0, 2]], keep[[0, 2]], count[[0, 2]], [0, 2])
        with pytest.raises(SSError) as ei:
            eng.check_errors()
        assert ei.value.code == SS_ERR_CAPACITY
    finally:
        eng.reset(-1)
    eng.check_errors()
    c = check(*eng.nms_batch(P[[0, 2]].contiguous(), 2, dcfg, G[:2]), [0, 2])
    assert c[0] == 1000 and c[1] > 0
    eng.check_errors()


# ---- max_det -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_det", [1, 63, 64, 65, 300, 1000, 1024, 5000])
def test_nms_max_det_caps(eng, fused, max_det):
    """the cap falls inside a 64-block, on its edge and one past it; the engine clamps to 1024.  The field keeps >= 1024 uncapped."""
    dcfg = replace(DetectConfig(), max_det=max_det)
    cap = min(max_det, 1024)
    pred = _field(5000, 4)
    rows = torch.full((1024 + 8, 6), -7.0, dtype=torch.float32, device=eng.device)
    keep = torch.full((1024 + 8,), -7, dtype=torch.int32, device=eng.device)
    count = torch.full((1,), -7, dtype=torch.int32, device=eng.device)
    got = _run(eng, pred, 2, dcfg, rows=rows, keep=keep, count=count)
    assert got[2] == cap
    _check(got, _oracle_of(pred, 2, dcfg, GEOM1, max_det=cap))
    assert np.all(got[0][cap:] == -7.0) and np.all(got[1][cap:] == -7)
    eng.check_errors()


# ---- stale workspace -----------------------------------------------------------------------------------------------------------------
def test_nms_small_image_after_a_large_one(eng, fused):
    """keys, boxes and bit-matrix rows of the previous image stay in the workspace; nothing of them may be read"""
    dcfg = DetectConfig()
    for n in (8192, 65, 64, 0, 4097):
        _check(_run(eng, _field(n), 2, dcfg), _oracle_of(_field(n), 2, dcfg, GEOM1))
    eng.check_errors()


# ---- classes -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _class_field(nc):
    N = 1344
    base = ff.nms_field(200, 5, N=N, nc=2, seed=nc)
    rng = np.random.default_rng(500 + nc)
    score = base[4:6].max(axis=0)
    cand = np.nonzero(score > 0)[0]
    pred = np.zeros((4 + nc, N), np.float32)
    pred[:4] = base[:4]
    cls = rng.integers(0, nc, len(cand))
    forced = [0, nc - 1] + ([80] if nc > 80 else [])
    cls[:len(forced)] = forced
    pred[4 + cls, cand] = score[cand]
    if nc >= 2:                                                      # two anchors whose two best classes tie bit for bit
        for a, (c0, c1) in zip(cand[-2:], [(0, nc - 1), (min(nc // 2, nc - 2), nc - 1)]):
            pred[4:, a] = 0.0
            pred[4 + c0, a] = pred[4 + c1, a] = score[a]
    pred[4:] += (pred[4:] == 0) * rng.uniform(0.0, 0.25, (nc, N)).astype(np.float32)   # every class row carries scores below conf
    pred.setflags(write=False)
    return pred


@pytest.mark.parametrize("nc", [1, 2, 7, 8, 9, 79, 80, 81, 88, 100, 128])
def test_nms_class_counts(eng, fused, nc):
    """the filter deals classes g, g + 8, ... to eight waves, ten per trip: waves without a class (nc < 8), a second trip (nc > 80)"""
    dcfg = DetectConfig()
    pred = _class_field(nc)
    ref = _oracle_of(pred, nc, dcfg, GEOM1)
    got = _run(eng, pred, nc, dcfg)
    _check(got, ref)
    seen = set(ref[1][:, 5].astype(int).tolist())
    assert got[2] >= 30 and {0, nc - 1} <= seen and (nc <= 80 or 80 in seen)
    eng.check_errors()


@pytest.mark.parametrize("classes", [[63], [64], [127], [0, 64, 127]])
def test_nms_class_mask_second_word(eng, fused, classes):
    dcfg = DetectConfig()
    pred = _class_field(128).copy()
    rng = np.random.default_rng(7)
    cand = np.nonzero(pred[4:].max(axis=0) > np.float32(dcfg.conf))[0]
    for a in cand[10:-2:3]:                                          # enough rows on the classes asked for
        s = pred[4:, a].max()
        pred[4:, a] = np.minimum(pred[4:, a], 0.2)
        pred[4 + int(rng.choice([0, 63, 64, 127])), a] = s
    try:
        eng.nms_set_classes(classes)
        got = _run(eng, pred, 128, dcfg)
    finally:
        eng.nms_set_classes(None)
    ref = _oracle_of(pred, 128, dcfg, GEOM1, classes=classes)
    _check(got, ref)
    assert set(ref[1][:, 5].astype(int).tolist()) == set(classes)
    _check(_run(eng, pred, 128, dcfg), _oracle_of(pred, 128, dcfg, GEOM1))       # and the mask is off again
    eng.check_errors()


# ---- known answers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [False, True], ids=["one_wave", "workgroup"])
@pytest.mark.parametrize("case", ff.known_answers(), ids=lambda c: c["name"])
def test_nms_known_answers(eng, fused, case, pad):
    case = ff.padded(case) if pad else case
    dcfg = replace(DetectConfig(), conf=case["conf"], iou=case["iou"])
    rows, keep, k = _run(eng, case["pred"], case["nc"], dcfg)
    assert keep[:k].tolist() == case["keep"]
    assert rows[:k, 5].astype(int).tolist() == case["cls"]
    _check((rows, keep, k), _oracle_of(case["pred"], case["nc"], dcfg, GEOM1))
    eng.check_errors()


# ---- batch ---------------------------------------------------------------------------------------------------------------------------
def test_nms_batch_mixed_counts_extra_channels_strided_pred(eng, fused):
    dcfg = DetectConfig()
    nc, ne, N = 2, 51, 8400
    counts = [0, 1, 64, 65, 700, 5000]
    B = len(counts)
    rng = np.random.default_rng(17)
    big = np.zeros((2 * B, 4 + nc + ne, N), np.float32)
    big[:, 4 + nc:] = rng.standard_normal((2 * B, ne, N))
    big[:, :4] = 50.0
    big[1::2, 4] = 0.95                                              # the images between: all candidates, never to be read
    geoms = []
    for b, n in enumerate(counts):
        big[2 * b, :4 + nc] = _field(n, 4 if n == 5000 else ff.PER_OF(n))
        geoms.append([1.0 / (1 + b % 3), float(b), 2.0 * b, 1280.0 + 16 * b, 720.0 + 8 * b])
    Pbig = torch.from_numpy(big).to(eng.device)
    P = Pbig[::2]
    assert not P.is_contiguous() and P.stride(0) == 2 * (4 + nc + ne) * N
    G = torch.tensor(geoms, dtype=torch.float32, device=eng.device)
    refs = [_oracle_of(big[2 * b, :4 + nc], nc, dcfg, geoms[b]) for b in range(B)]
    for rep in range(2):
        rows, keep, count = eng.nms_batch(P, nc, dcfg, G, n_extra=ne)
        rows, keep, count = rows.cpu().numpy(), keep.cpu().numpy(), count.cpu().numpy()
        for b in range(B):
            k = int(count[b])
            _check((rows[b], keep[b], k), refs[b])
            assert bits_equal(rows[b, :k, 6:], big[2 * b][4 + nc:][:, keep[b, :k]].T)
        assert count.tolist()[:2] == [0, 1] and count[5] == 1000
    eng.check_errors()


# =====================================================================================================================================
# packed crops, unaligned frames, more than 1024 images, feature unpacking
# =====================================================================================================================================
SENT = {torch.float32: 7.0, torch.float16: 7.0, torch.uint8: 7}
DTYPES = [torch.float32, torch.float16, torch.uint8]
DT_IDS = ["f32", "f16", "u8"]


def _out(eng, slots, dt):
    return torch.full((slots, 3, 256, 128), SENT[dt], dtype=dt, device=eng.device).contiguous(memory_format=torch.channels_last)


def _values(t):
    """device crops -> numpy NCHW, byte crops through the expression their consumer applies"""
    from strongsort_yolo_amd import fused32
    return (fused32.crops_from_u8(t) if t.dtype == torch.uint8 else t).cpu().numpy()


def _ref_crops(img, dets, dt):
    r = cexact.crop_norm(img, dets)
    return r.astype(np.float16) if dt == torch.float16 else r


@pytest.fixture(scope="module")
def packed_inputs():
    W, H, B = 1280, 720, 4
    rng = np.random.default_rng(41)
    frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    dets, counts = ff.packed_case(W, H, B)
    return frames, dets, counts


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_crop_packed_against_the_oracle(eng, packed_inputs, dt):
    """the form the pipeline runs (k_crop_offsets, then k_crop_hwc8 with the offsets): slot, prefix sum and the min(count, n) clamp"""
    frames, dets, counts = packed_inputs
    B, n = len(counts), 32
    F, D = torch.from_numpy(frames).to(eng.device), torch.from_numpy(dets).to(eng.device)
    C = torch.tensor(counts, dtype=torch.int32, device=eng.device)
    off = torch.full((B + 1,), -1, dtype=torch.int32, device=eng.device)
    out = _out(eng, B * n, dt)
    eng.crop_norm_packed(F, D, n, C, off, out, half=dt == torch.float16)
    o = off.cpu().tolist()
    assert o == [0, 32, 32, 49, 81]
    got = _values(out[:81])
    for i in range(B):
        k = min(counts[i], n)
        assert bits_equal(got[o[i]:o[i] + k], _ref_crops(frames[i], dets[i, :k], dt)), i
    assert bool((out[81:] == SENT[dt]).all())
    # nothing to crop: offsets all 0, nothing written
    out2 = _out(eng, 4, dt)
    eng.crop_norm_packed(F, D, n, torch.zeros(B, dtype=torch.int32, device=eng.device), off, out2, half=dt == torch.float16)
    assert off.cpu().tolist() == [0] * (B + 1) and bool((out2 == SENT[dt]).all())
    eng.check_errors()


@pytest.mark.parametrize("W,shift", [(33, 0), (36, 0), (36, 1), (36, 2), (36, 3)])
def test_crop_unaligned_frames(eng, W, shift):
    """a row pitch of 99 bytes, and an aligned pitch (108) behind a base 1, 2, 3 bytes off: the kernel must take the byte loads"""
    H, B, n = 31, 2, 8
    rng = np.random.default_rng(100 + W + shift)
    size = B * H * W * 3
    buf = torch.from_numpy(rng.integers(0, 256, size + 8, dtype=np.uint8)).to(eng.device)
    F = buf[shift:shift + size].view(B, H, W, 3)
    assert F.data_ptr() % 4 == shift and (W * 3) % 4 == (3 if W == 33 else 0)
    frames = F.cpu().numpy()
    d = ff.small_frame_boxes(W, H)
    dets = np.stack([d, d[::-1]]).copy()
    D = torch.from_numpy(dets).to(eng.device)
    C = torch.tensor([8, 5], dtype=torch.int32, device=eng.device)
    for dt in DTYPES:
        half = dt == torch.float16
        ob = _out(eng, B * n, dt)
        eng.crop_norm_batch(F, D, n, counts=C, half=half, out=ob, channels_last=True)
        op, off = _out(eng, B * n, dt), torch.zeros(B + 1, dtype=torch.int32, device=eng.device)
        eng.crop_norm_packed(F, D, n, C, off, op, half=half)
        assert off.cpu().tolist() == [0, 8, 13]
        gb, gp = _values(ob), _values(op[:13])
        r0, r1 = _ref_crops(frames[0], dets[0], dt), _ref_crops(frames[1], dets[1, :5], dt)
        assert bits_equal(gb[:8], r0) and bits_equal(gb[8:13], r1)
        assert bits_equal(gp[:8], r0) and bits_equal(gp[8:13], r1)
        assert bool((ob[13:] == SENT[dt]).all()) and bool((op[13:] == SENT[dt]).all())
    eng.check_errors()


def test_crop_offsets_more_than_1024_images(eng):
    """k_crop_offsets gives every thread ceil(B / 1024) images once B > 1024"""
    B, n, W, H = 1030, 2, 32, 24
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    x1 = rng.uniform(-2, W - 6, (B, 3)); y1 = rng.uniform(-2, H - 6, (B, 3))
    dets = np.stack([x1, y1, x1 + rng.uniform(0.5, 20, (B, 3)), y1 + rng.uniform(0.5, 20, (B, 3)), np.ones((B, 3)), np.zeros((B, 3))],
                    2).astype(np.float32)
    counts = np.array([0, 1, 2, 3] * 258, np.int32)[:B]
    want = np.concatenate([[0], np.cumsum(np.minimum(counts, n))]).astype(np.int32)
    total = int(want[B])
    dt = torch.uint8
    out = _out(eng, B * n, dt)                                       # the documented size: a wrong prefix still lands inside it
    off = torch.full((B + 1,), -1, dtype=torch.int32, device=eng.device)
    eng.crop_norm_packed(torch.from_numpy(frames).to(eng.device), torch.from_numpy(dets).to(eng.device), n,
                         torch.from_numpy(counts).to(eng.device), off, out)
    assert np.array_equal(off.cpu().numpy(), want)
    # the first thread's two images, the second thread's first, the images around 1024 (thread 512's first) and the last ones
    for i in (0, 1, 2, 3, 1022, 1023, 1024, 1025, 1026, 1027, 1029):
        k = min(int(counts[i]), n)
        assert bits_equal(_values(out[int(want[i]):int(want[i]) + k]), _ref_crops(frames[i], dets[i, :k], dt)), i
    assert bool((out[total:] == SENT[dt]).all())
    filled = (out[:total] != SENT[dt]).any(dim=3).any(dim=2).any(dim=1)              # every slot below the total was written
    assert bool(filled.all())
    eng.check_errors()


@pytest.mark.parametrize("dt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_unpack_feats(eng, dt):
    counts, n, B = [32, 0, 17, 40], 32, 4
    off = [0, 32, 32, 49, 81]
    emb = torch.randn(81, 512, generator=torch.Generator().manual_seed(9)).to(dt).to(eng.device)
    feats = torch.full((B, 128, 512), -3.0, dtype=torch.float32, device=eng.device)
    eng.unpack_feats(emb, torch.tensor(off, dtype=torch.int32, device=eng.device),
                     torch.tensor(counts, dtype=torch.int32, device=eng.device), n, feats)
    got, e = feats.cpu().numpy(), emb.float().cpu().numpy()
    for i in range(B):
        k = min(counts[i], n)
        assert bits_equal(got[i, :k], e[off[i]:off[i] + k])
        assert np.all(got[i, k:] == -3.0)
    eng.check_errors()
