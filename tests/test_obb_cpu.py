"""Oriented boxes without a GPU (docs/OBB.md): csrc/ss_probiou.h built by a host compiler against tests/obb_ref.py bit for bit, the three
fixed sequences against libm within the derived ulp bounds, ProbIoU's known answers, nms_rotated on hand-made cases (R-02 .. R-05), the
fields of the GPU tests, the models, the checkpoint key mapping and the library's refusals."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import obb_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]          # tests/test_ocsort_cpu.py's, for asin_host_main.cpp

# docs/OBB.md §1c: bounds derived from the truncated series and the rounding of every step, in ulps of the result
LOG_ULP, SINCOS_ULP, EXPNEG_ULP = 5.0, 6.0, 6.0
IDENTICAL = float(1.0 - math.sqrt(1.0 - R.ss_expneg(R.EPS)[0] + R.EPS))       # docs/OBB.md §1d: what two identical boxes give


def _cxx():
    return os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "clang++"


def _inputs():
    rng = np.random.default_rng(11)
    sq = R.SQRT2
    lg = np.concatenate([10.0 ** rng.uniform(-7, 25, 20000), np.linspace(0.5, 2.0, 4001),
                         [1.0, sq, np.nextafter(sq, 2), np.nextafter(sq, 1), 1e-7, 1e25, 0.0, -1.0, np.inf, np.nan, 5e-324]])
    an = np.concatenate([rng.uniform(-R.SINCOS_MAX, R.SINCOS_MAX, 10000), rng.uniform(-np.pi, 2 * np.pi, 20000), np.arange(-64, 65) * (np.pi / 4),
                         [np.nextafter(np.pi / 4, 0), np.nextafter(np.pi / 4, 1), R.SINCOS_MAX, -R.SINCOS_MAX, np.nan, np.inf, 2.0e6]])
    ex = np.concatenate([rng.uniform(0, 100, 10000), [R.EPS, 0.0, 100.0, 700.0, 701.0, np.nan]])
    bx = np.concatenate([R.probiou_boxes(40, 1), R.probiou_boxes(30, 2)])
    return lg, an, ex, bx


def _host_output(exe, lg, an, ex, bx):
    inp = np.array([len(lg), len(an), len(ex), len(bx)], np.int64).tobytes() + lg.tobytes() + an.tobytes() + ex.tobytes() + bx.tobytes()
    out = np.frombuffer(subprocess.run([exe], input=inp, stdout=subprocess.PIPE, check=True).stdout, np.float64)
    cuts = np.cumsum([len(lg), 2 * len(an), len(ex), 6 * len(bx), len(bx) ** 2])
    assert len(out) == cuts[-1]
    return np.split(out, cuts[:-1])


def _same_bits(got, ref):
    return np.ascontiguousarray(got, np.float64).tobytes() == np.ascontiguousarray(ref, np.float64).tobytes()


def test_probiou_header_and_reference_agree_on_every_bit(tmp_path):
    exe = str(tmp_path / "probiou_host")
    subprocess.check_call([_cxx()] + FLAGS + [os.path.join(HERE, "probiou_host_main.cpp"), "-o", exe])
    lg, an, ex, bx = _inputs()
    o_log, o_sc, o_exp, o_terms, o_m = _host_output(exe, lg, an, ex, bx)
    s, c = R.ss_sincos(an)
    assert _same_bits(o_log, R.ss_log(lg))
    assert _same_bits(o_sc.reshape(-1, 2)[:, 0], s) and _same_bits(o_sc.reshape(-1, 2)[:, 1], c)
    assert _same_bits(o_exp, R.ss_expneg(ex))
    assert _same_bits(o_terms, R.box_terms(bx).ravel())
    assert _same_bits(o_m, R.probiou(bx, bx).ravel())


def test_probiou_header_under_address_and_undefined_sanitizers(tmp_path):
    """the same stand-alone program (its own main, nothing preloaded) built with the sanitizers, run once"""
    exe = str(tmp_path / "probiou_host_san")
    subprocess.check_call([_cxx()] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                              os.path.join(HERE, "probiou_host_main.cpp"), "-o", exe])
    lg, an, ex, bx = _inputs()
    o_m = _host_output(exe, lg[-200:], an[-200:], ex[-200:], bx)[4]
    assert _same_bits(o_m, R.probiou(bx, bx).ravel())


def _ulps(got, ref):
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(got, np.float64) - ref) / np.spacing(np.abs(ref))).max())


def test_fixed_sequences_against_libm_within_the_derived_bounds():
    """log on 1e-7 .. 1e25, sine and cosine on the whole domain |t| <= 2^20 with the multiples of pi/4 and the reduction's boundaries,
    exp(-x) on 0 .. 100 (ProbIoU's clamp).  The bounds are docs/OBB.md §1c's, derived, not read off this run."""
    lg, an, ex, _ = _inputs()
    lg, an, ex = lg[:-5], an[:-3], ex[:-2]
    u_log = _ulps(R.ss_log(lg), [math.log(x) for x in lg])
    s, c = R.ss_sincos(an)
    u_sin, u_cos = _ulps(s, [math.sin(t) for t in an]), _ulps(c, [math.cos(t) for t in an])
    u_exp = _ulps(R.ss_expneg(ex), [math.exp(-x) for x in ex])
    print(f"largest error in ulps: ss_log {u_log}, ss_sincos sine {u_sin} cosine {u_cos}, ss_expneg {u_exp}")
    assert u_log <= LOG_ULP and u_sin <= SINCOS_ULP and u_cos <= SINCOS_ULP and u_exp <= EXPNEG_ULP
    assert R.LOG_C == [1.0 / (2 * k + 1) for k in range(12)]
    assert R.SIN_C == [(-1) ** k / math.factorial(2 * k + 1) for k in range(9)] and R.COS_C == [(-1) ** k / math.factorial(2 * k) for k in range(10)]
    assert float.hex(R.PIO2_1) == "0x1.921fb54400000p+0" and float.hex(R.PIO2_2) == "0x1.0b4611a600000p-34"      # 33 bits each: k P exact
    assert float.hex(R.PIO2_3) == "0x1.3198a2e000000p-69" and R.PIO2_1 + R.PIO2_2 == math.pi / 2
    assert np.isnan(R.ss_log([0.0, -1.0, np.inf, np.nan, 5e-324])).all()                                     # outside the domain: NaN
    assert np.isnan(np.stack(R.ss_sincos([np.nan, np.inf, np.nextafter(R.SINCOS_MAX, np.inf)]))).all()


def _libm_probiou(a, b):
    eps = 1e-7

    def terms(x):
        cx, cy, w, h, t = (float(v) for v in x)
        a_, b_, c, s = w * w / 12, h * h / 12, math.cos(t), math.sin(t)
        return cx, cy, a_ * c * c + b_ * s * s, a_ * s * s + b_ * c * c, (a_ - b_) * c * s
    x1, y1, A1, B1, C1 = terms(a)
    x2, y2, A2, B2, C2 = terms(b)
    sa, sb, sc, dx, dy = A1 + A2, B1 + B2, C1 + C2, x1 - x2, y1 - y2
    den = sa * sb - sc * sc
    t1 = (sa * dy * dy + sb * dx * dx) / (den + eps) * 0.25
    t2 = (sc * (-dx) * dy) / (den + eps) * 0.5
    t3 = 0.5 * math.log(den / (4 * math.sqrt(max(A1 * B1 - C1 * C1, 0) * max(A2 * B2 - C2 * C2, 0)) + eps) + eps)
    bd = min(max(t1 + t2 + t3, eps), 100.0)
    return 1.0 - math.sqrt(1.0 - math.exp(-bd) + eps)


def test_probiou_known_answers():
    box = np.array([[100, 80, 60, 20, 0.3]], np.float32)
    # identical boxes: bd falls below eps and is clamped, so the value is one constant whatever the box (docs/OBB.md §1d)
    for b in ([100, 80, 60, 20, 0.3], [5, 5, 2, 1, -0.7], [1e4, -3e3, 900, 30, 3.0], [0, 0, 7, 7, 1.0]):
        assert R.probiou([b], [b])[0, 0] == IDENTICAL
    assert abs(IDENTICAL - (1.0 - math.sqrt(2e-7))) < 1e-11
    # a box and itself turned by pi
    assert R.probiou(box, box + np.array([0, 0, 0, 0, np.pi], np.float32))[0, 0] == IDENTICAL
    # a square is invariant under theta
    other = np.array([[110, 90, 30, 50, 0.9]], np.float32)
    sq = np.array([[100, 80, 40, 40, t] for t in np.linspace(-0.7, 3.1, 9)], np.float32)
    v = R.probiou(sq, other)[:, 0]
    assert 0.05 < v[0] < 0.95 and np.abs(v - v[0]).max() < 1e-12
    # symmetry, bit for bit
    a, b = R.probiou_boxes(40, 1), R.probiou_boxes(40, 2)
    assert _same_bits(R.probiou(a, b), R.probiou(b, a).T)
    # far apart: the bd = 100 clamp
    far = R.probiou(box, [[5000, 80, 60, 20, 0.3]])[0, 0]
    assert far == float(1.0 - math.sqrt(1.0 - R.ss_expneg(100.0)[0] + R.EPS)) and abs(far) < 1e-7
    # R-01: degenerate boxes have ProbIoU 0 with everything, themselves and each other included
    m = R.probiou(a, a)
    assert np.all(m[:6] == 0.0) and np.all(m[:, :6] == 0.0) and not np.isnan(m).any()
    assert R.probiou([[0, 0, 0, 0, 0]], [[500, 500, 0, 0, 0]])[0, 0] == 0.0          # upstream's formula gives about 1 here
    assert np.all(m[6:, 6:] > -1e-7) and np.all(m[6:, 6:] <= IDENTICAL)
    # the formula through libm: docs/OBB.md §1e bounds the difference by 1e-7 for aspect ratios up to 8
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(400):
        p = np.array([rng.uniform(0, 100), rng.uniform(0, 100), rng.uniform(10, 80), rng.uniform(10, 80), rng.uniform(-0.78, 3.14)], np.float32)
        q = (p + np.array([rng.normal(0, 8), rng.normal(0, 8), rng.normal(0, 3), rng.normal(0, 3), rng.normal(0, 0.5)])).astype(np.float32)
        q[2:4] = np.clip(q[2:4], 10, 80)
        worst = max(worst, abs(R.probiou([p], [q])[0, 0] - _libm_probiou(p, q)))
    print(f"largest difference from the libm formula: {worst:.3e}")
    assert worst <= 1e-7


def _pred(boxes, scores, classes, nc=3, A=None):
    """hand-made prediction tensor: candidate q at anchor q"""
    n = len(boxes)
    pred = np.zeros((4 + nc + 1, A or n), np.float32)
    for q, (b, s, k) in enumerate(zip(boxes, scores, classes)):
        pred[:4, q], pred[4 + k, q], pred[4 + nc, q] = b[:4], s, b[4]
    return pred


G0 = (1.0, 0.0, 0.0, 1000.0, 1000.0)


def test_nms_rotated_any_higher_scored_overlap_removes_not_a_greedy_scan():
    """R-02: A > B > C along a line; A overlaps B, B overlaps C, A does not overlap C.  C goes although B, its only suppressor, is itself
    removed; a greedy scan keeps C."""
    A_, B_, C_ = [100, 100, 80, 20, 0.0], [118, 100, 80, 20, 0.0], [136, 100, 80, 20, 0.0]
    v = R.probiou([A_, B_, C_], [A_, B_, C_])
    thr = 0.5 * (v[0, 1] + v[0, 2])
    assert v[0, 1] > thr and v[1, 2] > thr and v[0, 2] < thr
    pred = _pred([A_, B_, C_], [0.9, 0.8, 0.7], [0, 0, 0])
    keep, rows = R.nms_rotated(pred, 3, 0.25, thr, False, 300, G0)
    assert keep.tolist() == [0]
    terms = R.box_terms(np.array([A_, B_, C_], np.float32))
    assert R.greedy_nms(terms, np.zeros(3, int), thr, False).tolist() == [False, True, False]
    assert R.removed_mask(terms, np.zeros(3, int), thr, False).tolist() == [False, True, True]


def test_nms_rotated_threshold_is_attained_with_greater_or_equal():
    a, b = [100, 100, 80, 20, 0.2], [110, 104, 70, 24, 0.5]
    v = R.probiou([a], [b])[0, 0]
    t32 = np.float32(v)
    pred = _pred([a, b], [0.9, 0.8], [1, 1])
    for thr in (np.nextafter(t32, np.float32(0)), t32, np.nextafter(t32, np.float32(1))):
        keep, _ = R.nms_rotated(pred, 3, 0.25, thr, False, 300, G0)
        assert (len(keep) == 1) == (v >= float(thr)), thr
    # a threshold the value attains exactly: the float64 value of a float32 threshold compared with >=
    d = [100, 100, 80, 20, 0.2]
    keep, _ = R.nms_rotated(_pred([d, d], [0.9, 0.8], [1, 1]), 3, 0.25, np.float32(R.probiou([d], [d])[0, 0]), False, 300, G0)
    exact = R.probiou([d], [d])[0, 0] >= float(np.float32(R.probiou([d], [d])[0, 0]))
    assert (len(keep) == 1) == exact


def test_nms_rotated_classes_ties_and_max_det():
    a, b, c = [100, 100, 80, 20, 0.2], [101, 100, 80, 20, 0.2], [500, 500, 40, 10, 1.0]
    # R-03: equal class is required unless agnostic
    pred = _pred([a, b, c], [0.9, 0.8, 0.7], [0, 1, 1])
    assert R.nms_rotated(pred, 3, 0.25, 0.4, False, 300, G0)[0].tolist() == [0, 1, 2]
    assert R.nms_rotated(pred, 3, 0.25, 0.4, True, 300, G0)[0].tolist() == [0, 2]
    assert R.nms_rotated(pred, 3, 0.25, 0.4, False, 300, G0, classes=(1,))[0].tolist() == [1, 2]
    # score ties go by anchor: the lower anchor is the higher-ranked candidate and removes the other
    tie = _pred([c, a, b], [0.5, 0.8, 0.8], [1, 0, 0])
    assert R.nms_rotated(tie, 3, 0.25, 0.4, False, 300, G0)[0].tolist() == [1, 0]
    # max_det cuts the kept list in score order
    far = [[60 * i + 30, 40, 50, 10, 0.1 * i] for i in range(8)]
    many = _pred(far, [0.9 - 0.05 * i for i in range(8)], [0] * 8)
    assert R.nms_rotated(many, 3, 0.25, 0.4, False, 300, G0)[0].tolist() == list(range(8))
    assert R.nms_rotated(many, 3, 0.25, 0.4, False, 3, G0)[0].tolist() == [0, 1, 2]
    # conf is a strict bound
    low = _pred([a], [0.25], [0])
    assert len(R.nms_rotated(low, 3, 0.25, 0.4, False, 300, G0)[0]) == 0


def test_regularise_and_envelope():
    pi, h = R.F32_PI, R.F32_PI_2
    b = np.array([[50, 50, 40, 10, 0.5],          # w > h: kept
                  [50, 50, 10, 40, 0.5],          # swapped, theta + pi/2
                  [50, 50, 20, 20, 0.5],          # w == h: swapped (w > h is false), theta + pi/2
                  [50, 50, 40, 10, -0.3],         # theta < 0: + pi
                  [50, 50, 10, 40, h],            # pi/2 + pi/2 lands on pi exactly: - pi = 0
                  [50, 50, 40, 10, pi]], np.float32)
    r = R.regularise(b)
    assert r[0].tolist() == b[0].tolist()
    assert r[1, 2:].tolist() == [40.0, 10.0, float(np.float32(0.5) + h)]
    assert r[2, 2:].tolist() == [20.0, 20.0, float(np.float32(0.5) + h)]
    assert r[3, 4] == np.float32(-0.3) + pi
    assert h + h == pi and r[4, 2:].tolist() == [40.0, 10.0, 0.0]
    assert r[5, 4] == 0.0
    assert np.all(r[:, 2] >= r[:, 3]) and np.all((r[:, 4] >= 0) & (r[:, 4] < pi))
    # scale: (c - pad) / gain, sizes / gain, no clipping (R-04)
    s = R.scale_rbox([[10, 20, 30, 8, 0.1]], 0.5, 4.0, 6.0)
    assert s[0].tolist() == [12.0, 28.0, 60.0, 16.0, float(np.float32(0.1))]
    assert R.scale_rbox([[1, 1, 30, 8, 0.1]], 0.5, 4.0, 6.0)[0, 0] == -6.0
    # envelope: an axis-parallel box is its own envelope; a right angle swaps the sides; clipped at the border
    assert R.envelope([[50, 40, 30, 10, 0.0]], 100, 100)[0].tolist() == [35.0, 35.0, 65.0, 45.0]
    e = R.envelope([[50, 40, 30, 10, h]], 100, 100)[0]
    assert np.abs(e - np.array([45, 25, 55, 55], np.float32)).max() < 1e-5
    assert R.envelope([[5, 95, 30, 10, 0.0]], 100, 100)[0].tolist() == [0.0, 90.0, 20.0, 100.0]
    d = R.envelope([[50, 50, 40, 40, 0.78539816]], 100, 100)[0]
    assert np.abs(d - np.array([50 - 20 * math.sqrt(2), 50 - 20 * math.sqrt(2), 50 + 20 * math.sqrt(2), 50 + 20 * math.sqrt(2)])).max() < 1e-4
    # upstream's corner order: ctr + v1 + v2, ctr + v1 - v2, ctr - v1 - v2, ctr - v1 + v2
    assert R.corners([[50, 40, 30, 10, 0.0]])[0].tolist() == [[65.0, 45.0], [65.0, 35.0], [35.0, 35.0], [35.0, 45.0]]


def _aabb_iou(a, b):
    iw, ih = max(0.0, min(a[2], b[2]) - max(a[0], b[0])), max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = iw * ih
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


@pytest.mark.parametrize("n_cand", [63, 64, 65, 1025, 8192])
def test_gpu_nms_fields_are_not_vacuous(n_cand):
    """the fields of tests/test_gpu_obb.py: exactly n_cand candidates, each field keeps and removes some, class-aware and agnostic differ,
    and (below the large count) some pair is decided differently by the axis-aligned rule on the envelopes"""
    pred = R.obb_field(n_cand, *R.field_shape(n_cand), nc=15, seed=n_cand + 15)
    idx, score, cls = R.candidates(pred, 15, 0.25)
    assert len(idx) == n_cand and np.all(np.diff(score.astype(np.float64)) <= 0)
    boxes = np.stack([pred[0, idx], pred[1, idx], pred[2, idx], pred[3, idx], pred[19, idx]], axis=1)
    terms = R.box_terms(boxes)
    rm, rm_ag = R.removed_mask(terms, cls, 0.4, False), R.removed_mask(terms, cls, 0.4, True)
    assert 0 < rm.sum() < n_cand and rm_ag.sum() > rm.sum()
    if n_cand == 8192:
        assert n_cand - len(np.unique(score)) > 0                  # exact score ties: the anchor decides
        return
    env = R.envelope(boxes, 4096, 4096)
    v = R.probiou_terms(terms, terms)
    differ = sum(1 for i in range(min(n_cand, 130)) for j in range(i + 1, min(n_cand, 130))
                 if (v[i, j] >= float(np.float32(0.4))) != (_aabb_iou(env[i], env[j]) > 0.4))
    assert differ > 0


def test_obb_models_and_registry():
    from strongsort_yolo_amd import nets
    assert sorted(nets.OBB_DETECTORS) == ["yolo11n-obb", "yolov8n-obb", "yolov8s-obb"] and not set(nets.OBB_DETECTORS) & set(nets.DETECTORS)
    for name in nets.OBB_DETECTORS:
        m = nets.build_detector(name + ".pt", 2).float()
        assert (m.nc, m.ne, m.nk, m.nm) == (15, 1, 0, 0) and m.detect.cv4[0][2].out_channels == 1
        assert m.detect.cv4[0][0].conv.out_channels == max(m.detect.cv2[0][0].conv.in_channels // 4, 1)
        with torch.no_grad():
            y = m(torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(1)))
        assert y.shape == (1, 20, 84) and torch.isfinite(y).all()
        th = y[:, 19]
        assert (th >= -math.pi / 4).all() and (th < 3 * math.pi / 4).all() and (y[:, 2:4] > 0).all()
    with pytest.raises(ValueError, match="yolov8n-obb"):
        nets.build_detector("yolov9-obb")
    with pytest.raises(ValueError):
        nets.Detect(15, (64, 128, 256), nk=51, ne=1)
    with pytest.raises(ValueError):
        nets.Detect(15, (64, 128, 256), nm=32, ne=1)


def test_decode_statement_is_dist2rbox():
    """the CPU module's rows against the formula of docs/OBB.md §2, evaluated here from the branch outputs"""
    from strongsort_yolo_amd import nets
    g = torch.Generator().manual_seed(4)
    det = nets.Detect(15, (64, 128, 256), ne=1).float().eval()
    feats = [torch.randn(2, c, s, s, generator=g) for c, s in ((64, 8), (128, 4), (256, 2))]
    with torch.no_grad():
        y = det._forward_torch(feats)
        B = 2
        box = torch.cat([det.cv2[i](f).reshape(B, 64, -1) for i, f in enumerate(feats)], 2)
        ang = torch.cat([det.cv4[i](f).reshape(B, 1, -1) for i, f in enumerate(feats)], 2)
    d = (box.view(B, 4, 16, -1).softmax(2) * torch.arange(16.0).view(1, 1, 16, 1)).sum(2)
    l, t, r, b = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
    anchors, strides = det._make_anchors(feats)
    th = (ang[:, 0].sigmoid() - 0.25) * math.pi
    xf, yf = (r - l) / 2, (b - t) / 2
    cx = (anchors[0, 0] + xf * th.cos() - yf * th.sin()) * strides[0, 0]
    cy = (anchors[0, 1] + xf * th.sin() + yf * th.cos()) * strides[0, 0]
    ref = torch.stack([cx, cy, (l + r) * strides[0, 0], (t + b) * strides[0, 0]], 1)
    assert y.shape == (2, 20, 84) and (y[:, :4] - ref).abs().max() < 1e-3 and (y[:, 19] - th).abs().max() < 1e-6


def test_ultralytics_obb_state_dict_keys_map_onto_the_module():
    """no OBB checkpoint is available: a synthetic state dict with upstream's key names (model.<i>.…, Conv + BatchNorm pairs, cv4 included)"""
    from strongsort_yolo_amd import nets
    m = nets.build_detector("yolov8n-obb", 0).float()
    ours = m.state_dict()
    layer = {f"b{i}": i for i in range(10)} | {"h12": 12, "h15": 15, "h16": 16, "h18": 18, "h19": 19, "h21": 21, "detect": 22}
    g = torch.Generator().manual_seed(9)
    sd = {}
    for k, v in ours.items():
        top, rest = k.split(".", 1)
        pre = f"model.{layer[top]}.{rest}"
        if rest.endswith("conv.weight"):
            sd[pre] = torch.randn(v.shape, generator=g)
            bn = pre[:-len("conv.weight")] + "bn."
            c = v.shape[0]
            sd[bn + "weight"], sd[bn + "bias"] = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
            sd[bn + "running_mean"], sd[bn + "running_var"] = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
            sd[bn + "num_batches_tracked"] = torch.tensor(1)
        elif not rest.endswith("conv.bias"):
            sd[pre] = torch.randn(v.shape, generator=g)           # the plain last 1x1 of a head branch: weight and bias
    sd["model.22.dfl.conv.weight"] = torch.arange(16.0).view(1, 16, 1, 1)
    assert any(k.startswith("model.22.cv4.2.2.") for k in sd) and "model.22.cv4.0.0.bn.running_var" in sd
    out = nets.convert_ultralytics_state_dict(m, sd)
    assert sorted(out) == sorted(ours) and all(out[k].shape == ours[k].shape for k in ours)
    m.load_state_dict(out, strict=True)
    k = "detect.cv4.1.0.conv"
    scale = sd["model.22.cv4.1.0.bn.weight"] / torch.sqrt(sd["model.22.cv4.1.0.bn.running_var"] + 1e-3)
    assert torch.allclose(out[k + ".weight"], sd["model.22.cv4.1.0.conv.weight"] * scale.view(-1, 1, 1, 1))
    assert torch.allclose(out[k + ".bias"], sd["model.22.cv4.1.0.bn.bias"] - sd["model.22.cv4.1.0.bn.running_mean"] * scale)
    assert torch.equal(out["detect.cv4.2.2.weight"], sd["model.22.cv4.2.2.weight"])


def test_obb_result_properties():
    """yolo.OBB over the rows of nms_rotated: the columns, the corners in upstream's order, the envelope, length / indexing / iteration"""
    from strongsort_yolo_amd.yolo import OBB, Results, DOTA_NAMES
    pred = R.obb_field(65, 84, 15, seed=80)
    keep, rows = R.nms_rotated(pred, 15, 0.25, 0.4, False, 300, (0.5, 3.0, 12.0, 1280.0, 720.0))
    o = OBB.from_rows(rows)
    assert len(o) == len(keep) > 3 and not o.is_track and o.id is None
    assert np.array_equal(o.xywhr.numpy(), rows[:, 6:11]) and np.array_equal(o.xyxy.numpy(), rows[:, :4])
    assert np.array_equal(o.conf.numpy(), rows[:, 4]) and np.array_equal(o.cls.numpy(), rows[:, 5])
    c = o.xyxyxyxy.numpy()
    assert c.shape == (len(o), 4, 2) and np.abs(c - R.corners(rows[:, 6:11])).max() < 1e-3
    inside = (rows[:, 0] > 0) & (rows[:, 1] > 0) & (rows[:, 2] < 1280) & (rows[:, 3] < 720)
    assert inside.any() and np.abs(c[inside].min(axis=1) - rows[inside, :2]).max() < 1e-3 and np.abs(c[inside].max(axis=1) - rows[inside, 2:4]).max() < 1e-3
    one = o[1]
    assert len(one) == 1 and one.xywhr.shape == (1, 5) and one.xyxyxyxy.shape == (1, 4, 2) and float(one.conf[0]) == float(rows[1, 4])
    assert len(o[-1]) == 1 and [float(b.conf[0]) for b in o] == rows[:, 4].tolist() and len(o[1:3]) == 2
    with pytest.raises(IndexError):
        o[len(o)]
    with pytest.raises(ValueError):
        OBB.from_rows(rows[:, :6])
    t = OBB.from_rows(rows, ids=torch.arange(len(rows)))
    assert t.is_track and int(t[2].id[0]) == 2
    res = Results(None, dict(enumerate(DOTA_NAMES)), None, obb=o)
    assert res.boxes is None and res.obb is o and len(res) == len(o) and len(DOTA_NAMES) == 15
    assert len(Results(None, {}, None)) == 0


def test_overlay_commands_draw_an_obb_result_as_closed_polylines():
    from strongsort_yolo_amd import overlay as ov
    from strongsort_yolo_amd.yolo import OBB, Results, DOTA_NAMES
    rows = np.array([[0, 0, 0, 0, 0.9, 1, 100, 80, 60, 20, 0.0], [0, 0, 0, 0, 0.5, 9, 300, 200, 40, 40, math.pi / 4]], np.float32)
    names = dict(enumerate(DOTA_NAMES))
    cl = ov.Overlay(names).commands([Results(None, names, None, obb=OBB.from_rows(rows))])
    r, _ = cl.arrays()
    lines = r[r[:, 0] == ov.LINE]
    assert len(lines) == 8 and len(r) == 8 + 2 * 2 and not (r[:, 0] == ov.RECT).any()           # two closed quads, a plate and a text each
    quad = lines[:4, 1:5].tolist()
    assert quad == [[130, 90, 130, 70], [130, 70, 70, 70], [70, 70, 70, 90], [70, 90, 130, 90]]  # corner order, closed back to the first
    texts = r[r[:, 0] == ov.TEXT]
    assert texts[0, 1:3].tolist() == [70, 70 - 3]                                                 # the top-most corner (the left one of a tie)
    top = 200 - 20 * math.sqrt(2)
    assert abs(texts[1, 1] - 300) <= 1 and abs(texts[1, 2] + 3 - top) <= 1
    assert bytes(cl.chars).decode().startswith(" ship 90.0%")
    # tracked: ids in the label, trails through the rotated boxes' centres
    o = ov.Overlay(names)
    for k in range(3):
        moved = rows.copy()
        moved[:, 6] += 10 * k
        cl = o.commands([Results(None, names, None, obb=OBB.from_rows(moved, ids=torch.tensor([7, 8])))])
    r, _ = cl.arrays()
    assert sorted(o.trails) == [7, 8] and list(o.trails[7]) == [(100.0, 80.0), (110.0, 80.0), (120.0, 80.0)]
    assert (r[:, 0] == ov.LINE).sum() == 8 + 2 * 2 and bytes(cl.chars).decode().startswith(" ID: 7 ship")
    o.commands([Results(None, names, None, obb=OBB.from_rows(rows[:1], ids=torch.tensor([7])))])
    assert sorted(o.trails) == [7]                                                                # a track that left takes its trail along
    # a plain result is drawn as before
    from strongsort_yolo_amd.yolo import Boxes
    b = Boxes(torch.tensor([[10.0, 20.0, 50.0, 60.0]]), torch.tensor([0.5]), torch.tensor([0.0]))
    r, _ = ov.Overlay({0: "person"}).commands([Results(None, {0: "person"}, b)]).arrays()
    assert r[:, 0].tolist() == [ov.RECT, ov.FILL, ov.TEXT]


def test_what_is_not_built_for_rotated_boxes_is_refused_by_name():
    """docs/OBB.md §5: with an -obb model the trackers on axis-aligned boxes and the options below are ValueErrors that name themselves,
    raised before anything is allocated (no GPU is touched here)"""
    from strongsort_yolo_amd.pipeline import FramePipeline, OverlappedPipeline
    from strongsort_yolo_amd.yolo import YOLO, DOTA_NAMES
    for cls in (FramePipeline, OverlappedPipeline):
        for trk in ("strongsort", "ocsort", "deep_ocsort"):
            with pytest.raises(ValueError, match=f"tracker '{trk}'.*'bytetrack' or 'botsort'"):
                cls("yolov8n-obb.pt", 1, (64, 64), tracker=trk)
        for kw, what in ((dict(with_reid=True), "with_reid"), (dict(with_reid=True, reid_model="auto"), "with_reid"), (dict(with_pose=True), "with_pose"),
                         (dict(cmc=True), "camera_motion"), (dict(slice_cfg=object()), "slice_hw")):
            with pytest.raises(ValueError, match=what):
                cls("YOLO11n-OBB", 1, (64, 64), tracker="botsort", **kw)
    for trk in ("ocsort", "deep_ocsort"):
        with pytest.raises(ValueError, match="'bytetrack' or 'botsort'"):
            YOLO("yolov8n-obb.pt", tracker_type=trk)
    for kw, what in ((dict(with_reid=True), "with_reid"), (dict(with_reid=True, reid_model="auto"), "with_reid"), (dict(with_pose=True), "with_pose"),
                     (dict(camera_motion=True), "camera_motion"), (dict(slice_hw=(32, 32)), "slice_hw"), (dict(device_masks=True), "device_masks")):
        with pytest.raises(ValueError, match=what):
            YOLO("yolov8s-obb.pt", tracker_type="botsort", **kw)
    m = YOLO("yolov8n-obb.pt", random_init_ok=True)                      # predict-only by default: tracking with StrongSORT is refused by name
    assert m.names == dict(enumerate(DOTA_NAMES)) and len(m.names) == 15
    with pytest.raises(ValueError, match="'strongsort'.*'bytetrack' or 'botsort'"):
        m.track(np.zeros((64, 64, 3), np.uint8))
    with pytest.raises(ValueError, match="'strongsort'.*'bytetrack' or 'botsort'"):
        next(m.track_stream([np.zeros((64, 64, 3), np.uint8)]))


def test_cli_refuses_what_is_not_built_for_rotated_boxes_by_name(tmp_path):
    """an -obb weight name through cli.process_video: the trackers on axis-aligned boxes (the default StrongSORT included, per frame and
    through track_stream) and --slice, --with-reid, --camera-motion, --device-masks are the named ValueErrors of YOLO; no GPU is touched"""
    from strongsort_yolo_amd import cli
    base = {"source": "synthetic:2", "track": True, "count": False, "weights": "yolov8n-obb.pt", "random_init": True, "outdir": str(tmp_path)}
    for trk in ("ocsort", "deep_ocsort"):
        with pytest.raises(ValueError, match=f"{trk}.*'bytetrack' or 'botsort'"):
            cli.process_video({**base, "tracker": trk})
    for batch in (1, 8):
        with pytest.raises(ValueError, match="'strongsort'.*'bytetrack' or 'botsort'"):
            cli.process_video({**base, "batch": batch})
    for kw, what in (({"slice": (32, 32)}, "slice_hw"), ({"with_reid": True}, "with_reid"), ({"camera_motion": True}, "camera_motion"),
                     ({"device_masks": True}, "device_masks"), ({"with_pose": True}, "with_pose")):
        with pytest.raises(ValueError, match=what):
            cli.process_video({**base, "tracker": "botsort", **kw})


def test_library_entries_refuse_a_null_context_and_bad_arguments():
    from strongsort_yolo_amd import lib
    lib.build()
    L = lib.load()
    assert L.ss_nms_obb_batch(None, None, 1, 0, 84, 15, 0.25, 0.4, 0, 300, None, None, 11, 0, None, 0, None) == lib.SS_ERR_INVALID
    fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
    a, o = (ctypes.c_float * 5)(), (ctypes.c_double * 1)()
    assert L.ss_probiou(None, a, 1, a, 1, o) == lib.SS_ERR_INVALID
    assert L.ss_probiou.argtypes[1] == fp and L.ss_probiou.argtypes[5] == dp
    with pytest.raises(ctypes.ArgumentError):
        L.ss_probiou(None, (ctypes.c_double * 5)(), 1, a, 1, o)
    # the decode entries know mode 2 only with one angle
    H = (ctypes.c_int * 3)(8, 4, 2)
    three = (ctypes.c_void_p * 3)()
    assert L.ss_op32_v8_decode(None, three, three, three, 2, 8, 2, H, H, H, 1, 15, 16, None) == lib.SS_ERR_INVALID
    assert L.ss_op_v8_decode_ext_f16(None, three, three, three, three, three, 2, 8, 2, H, H, H, 1, 15, 16, None) == lib.SS_ERR_INVALID
    assert L.ss_op_v8_decode_ext_f16(None, three, three, three, three, three, 1, 8, 3, H, H, H, 1, 15, 16, None) == lib.SS_ERR_INVALID


# ---- BYTE tracking on rotated boxes (docs/OBB.md §4): the reference alone ----------------------------------------------------------------
SCENES = ((1, 18.0), (2, 18.0), (3, 18.0), (1, 6.0))             # (seed, lane spacing): the fourth is the one on which the xywh filter differs too


@pytest.mark.parametrize("kalman", ["xyah", "xywh"])
def test_tracker_scenes_are_not_vacuous(kalman):
    """every scene loses and re-finds a track and removes a duplicate; on at least one scene the axis-aligned tracker fed the envelopes
    of the same rows gives another id sequence than the tracker on ProbIoU (xyah: on all four; xywh: on the fourth, whose lanes are 6
    pixels apart)"""
    from strongsort_yolo_amd.config import ByteTrackConfig
    from tests.bytetrack_ref import ByteTrackRef
    differs = []
    for seed, lane in SCENES:
        a, p = R.ByteTrackObbRef(ByteTrackConfig(kalman=kalman)), ByteTrackRef(ByteTrackConfig(kalman=kalman))
        ida, idp = [], []
        for d in R.rotating_scene(seed, lane=lane):
            rows, rbox = a.update(d)
            assert rows.shape[1] == 8 and rbox.shape == (rows.shape[0], 5) and rows.dtype == rbox.dtype == np.float32
            assert np.all(rows[:, 0] <= rbox[:, 0]) and np.all(rbox[:, 0] <= rows[:, 2])                # the envelope holds the centre
            ida.append(sorted(zip(rows[:, 7].astype(int).tolist(), rows[:, 4].astype(int).tolist())))
            r2 = p.update(d[:, :6])
            idp.append(sorted(zip(r2[:, 7].astype(int).tolist(), r2[:, 4].astype(int).tolist())))
        assert a.n_refound >= 1 and a.n_duplicates >= 1, (seed, a.n_refound, a.n_duplicates)
        assert len(a.angles()) == len(a.tracked) + len(a.lost)
        differs.append(ida != idp)
    assert differs == ([True] * 4 if kalman == "xyah" else [False, False, False, True])


def test_tracker_reference_carries_the_last_rows_angle():
    """R-06: update, re-activation and birth set the angle to the row's; a lost track keeps it"""
    from strongsort_yolo_amd.config import ByteTrackConfig
    ref = R.ByteTrackObbRef(ByteTrackConfig())
    box = lambda th: R.obb_rows(np.array([[100.0, 100.0, 80.0, 20.0, th]], np.float32), np.float32(0.9), np.float32(0))
    ref.update(box(0.5))
    assert ref.angles().tolist() == [np.float32(0.5)]
    ref.update(box(0.625))
    assert ref.angles().tolist() == [np.float32(0.625)]
    ref.update(np.zeros((0, 11), np.float32))
    assert len(ref.lost) == 1 and ref.angles().tolist() == [np.float32(0.625)]
    rows, rbox = ref.update(box(0.75))
    assert len(ref.tracked) == 1 and rbox[0, 4] == np.float32(0.75) and rows[0, 4] == 1.0


def test_tracker_entries_refuse_a_null_context():
    from strongsort_yolo_amd import lib
    lib.build()
    L = lib.load()
    f, i = (ctypes.c_float * 11)(), (ctypes.c_int * 1)()
    assert L.ss_byte_set_obb(None, 1) == lib.SS_ERR_INVALID
    assert L.ss_byte_update_group_obb(None, 1, f, i, f, f, i) == lib.SS_ERR_INVALID
    assert L.ss_byte_get_angles(None, 0, 1, f) == lib.SS_ERR_INVALID


def test_byte_engine_refuses_oriented_boxes_with_reid_or_pose():
    from strongsort_yolo_amd.config import ByteTrackConfig
    from strongsort_yolo_amd.engine import ByteTrackEngine
    for kw in (dict(with_reid=True), dict(with_pose=True)):
        with pytest.raises(ValueError, match="oriented boxes"):
            ByteTrackEngine(ByteTrackConfig(kalman="xywh", **kw), 1, 0, obb=True)
