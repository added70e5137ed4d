"""Oriented boxes on the device, through the C ABI (docs/OBB.md): ss_probiou and ss_nms_obb_batch against tests/obb_ref.py, bit for bit.
tests/test_obb_cpu.py holds the proofs about the reference and about the fields used here (each keeps and removes candidates; the
rotated and the axis-aligned rule decide at least one pair differently)."""
import ctypes
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

from strongsort_yolo_amd.config import DetectConfig
from strongsort_yolo_amd.lib import SSError, SS_ERR_CAPACITY
from tests import obb_ref as R
from tests.gpu_util import engine, bits_equal

pytestmark = pytest.mark.gpu

NMS_MAX_CAND = 8192
GEOM1 = (1.0, 0.0, 0.0, 1024.0, 1024.0)
GEOMS = [(1.0, 0.0, 0.0, 1024.0, 1024.0), (0.5, 3.0, 12.0, 1280.0, 720.0), (0.75, 0.0, 40.0, 640.0, 480.0), (2.0, 16.0, 0.0, 320.0, 320.0),
         (0.33333334, 7.0, 9.0, 1920.0, 1080.0)]


@pytest.fixture(scope="module")
def eng():
    e = engine(debug=False)
    yield e
    e.close()


# ---- ss_probiou ---------------------------------------------------------------------------------------------------------------------
def test_probiou_matrix_equals_the_reference_bit_for_bit(eng):
    """70 x 70: past one wave's 64 in both directions; the degenerate rows of R-01 included"""
    a, b = R.probiou_boxes(70, 1), R.probiou_boxes(70, 2)
    got = eng.probiou(a, b)
    ref = R.probiou(a, b)
    assert got.shape == (70, 70) and bits_equal(got, ref)
    assert np.count_nonzero(ref == 0.0) >= 70 * 6 and np.count_nonzero(ref > 0.5) >= 3          # degenerate rows; near-copies
    assert bits_equal(eng.probiou(a[:1], b[:0]), np.zeros((1, 0)))


# ---- decode mode 2 ------------------------------------------------------------------------------------------------------------------
# docs/OBB.md §2b: the largest absolute error of (xywh, theta) of the fp32 path against the CPU fp32 module, measured once on an MI355X;
# the test asserts at twice these.  The f16 path is held to the bound of the f16 whole-network tests (tests/test_gpu_nets.py).
MEASURED32 = {("yolov8n-obb", (64, 64)): (3.052e-05, 1.788e-07), ("yolov8n-obb", (96, 160)): (6.104e-05, 2.384e-07),
              ("yolov8s-obb", (64, 64)): (6.104e-05, 2.384e-07), ("yolov8s-obb", (96, 160)): (6.104e-05, 2.384e-07),
              ("yolo11n-obb", (64, 64)): (6.104e-05, 1.788e-07), ("yolo11n-obb", (96, 160)): (9.155e-05, 2.384e-07)}


@pytest.mark.parametrize("name,hw", sorted(MEASURED32))
def test_decode_mode_2_on_both_paths_against_the_cpu_module(name, hw, monkeypatch):
    from strongsort_yolo_amd import fused, fused32, nets
    dev = torch.device("cuda", 0)
    # no quiet fall-back: each device forward must end in its decode launch with ext_mode 2 (the last positional argument)
    modes = {"f16": [], "fp32": []}
    for key, mod in (("f16", fused), ("fp32", fused32)):
        def counted(*a, _fn=mod.v8_decode, _key=key, **kw):
            modes[_key].append(a[-1])
            return _fn(*a, **kw)
        monkeypatch.setattr(mod, "v8_decode", counted)
    x = torch.rand(2, 3, *hw, generator=torch.Generator().manual_seed(hw[0] + hw[1]))
    A = sum((hw[0] // s) * (hw[1] // s) for s in (8, 16, 32))
    with torch.no_grad():
        ref = nets.build_detector(name, 2).float()(x)
        m32 = nets.build_detector(name, 2).float().to(dev)
        got32 = m32(x.to(dev).contiguous(memory_format=torch.channels_last)).cpu()
        assert modes == {"f16": [], "fp32": [2]}, modes
        m16 = nets.build_detector(name, 2).to(dev, torch.float16).to(memory_format=torch.channels_last)
        got16 = m16(x.to(dev, torch.float16).contiguous(memory_format=torch.channels_last)).float().cpu()
    assert modes == {"f16": [2], "fp32": [2]}, modes
    assert all(h._ext_ok() for h in m16.modules() if hasattr(h, "_ext_ok")) and any(hasattr(h, "_ext_ok") for h in m16.modules())
    assert fused.ENABLED and fused32.DET and getattr(m32, "_own32", None) in (True, None)
    assert ref.shape == got32.shape == got16.shape == (2, 20, A)
    e32 = (float((got32[:, :4] - ref[:, :4]).abs().max()), float((got32[:, 19] - ref[:, 19]).abs().max()))
    e16 = (float((got16[:, :4] - ref[:, :4]).abs().max()), float((got16[:, 19] - ref[:, 19]).abs().max()))
    print(f"{name} {hw}: fp32 xywh {e32[0]:.3e} theta {e32[1]:.3e}; f16 xywh {e16[0]:.3e} theta {e16[1]:.3e}")
    assert e32[0] <= 2 * MEASURED32[name, hw][0] and e32[1] <= 2 * MEASURED32[name, hw][1]
    bound16 = 2e-2 * (ref.abs().max().item() + 1e-6)
    assert torch.isfinite(got16).all() and e16[0] <= bound16 and e16[1] <= bound16
    assert float((got32[:, 4:19] - ref[:, 4:19]).abs().max()) <= 1e-6 and float((got16[:, 4:19] - ref[:, 4:19]).abs().max()) <= bound16


# ---- ss_nms_obb_batch ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _field(n_cand, nc=15):
    pred = R.obb_field(n_cand, *R.field_shape(n_cand), nc=nc, seed=n_cand + nc)
    pred.setflags(write=False)
    return pred


@functools.lru_cache(maxsize=None)
def _ref(n_cand, nc, agnostic, max_det, geom, classes=None):
    d = DetectConfig()
    return R.nms_rotated(_field(n_cand, nc), nc, d.conf, d.iou, agnostic, max_det, geom, classes=classes)


def _run(eng, preds, nc, dcfg, geoms, max_det=300):
    P = torch.from_numpy(np.stack(preds)).to(eng.device)
    G = torch.tensor(geoms, dtype=torch.float32, device=eng.device)
    rows, keep, count = eng.nms_obb_batch(P, nc, dcfg, G, max_det=max_det)
    return rows.cpu().numpy(), keep.cpu().numpy(), count.cpu().numpy()


def _check(rows, keep, k, ref):
    rkeep, rrows = ref
    assert int(k) == len(rkeep)
    assert np.array_equal(keep[:k], rkeep)
    assert np.array_equal(rows[:k], rrows) and bits_equal(rows[:k], rrows)


@pytest.mark.parametrize("n_cand", [0, 1, 63, 64, 65, 1025, NMS_MAX_CAND])
@pytest.mark.parametrize("agnostic", [False, True])
def test_nms_obb_candidate_counts(eng, agnostic, n_cand):
    """none, one, a wave less one, a wave, a wave and one (two block rows), past the sort's power of two, the capacity"""
    dcfg = replace(DetectConfig(), agnostic_nms=agnostic)
    rows, keep, count = _run(eng, [_field(n_cand)], 15, dcfg, [GEOM1])
    ref = _ref(n_cand, 15, agnostic, 300, GEOM1)
    _check(rows[0], keep[0], count[0], ref)
    assert (count[0] > 0) == (n_cand > 0)
    eng.check_errors()


@pytest.mark.parametrize("nc", [1, 15, 80])
def test_nms_obb_class_counts(eng, nc):
    dcfg = DetectConfig()
    rows, keep, count = _run(eng, [_field(65, nc)], nc, dcfg, [GEOM1])
    _check(rows[0], keep[0], count[0], _ref(65, nc, False, 300, GEOM1))
    eng.check_errors()


def test_nms_obb_classes_mask(eng):
    dcfg = DetectConfig()
    allowed = (0, 3, 7, 14)
    eng.nms_set_classes(allowed)
    try:
        rows, keep, count = _run(eng, [_field(1025)], 15, dcfg, [GEOM1])
    finally:
        eng.nms_set_classes(None)
    ref = _ref(1025, 15, False, 300, GEOM1, classes=allowed)
    _check(rows[0], keep[0], count[0], ref)
    assert 0 < len(ref[0]) < len(_ref(1025, 15, False, 300, GEOM1)[0]) and set(ref[1][:, 5].astype(int)) <= set(allowed)
    eng.check_errors()


@pytest.mark.parametrize("max_det", [1, 300])
def test_nms_obb_max_det(eng, max_det):
    """the cut falls inside the first 64-block and past several; rows beyond it stay untouched"""
    dcfg = DetectConfig()
    P = torch.from_numpy(_field(1025)[None].copy()).to(eng.device)
    G = torch.tensor([GEOM1], dtype=torch.float32, device=eng.device)
    rows = torch.full((1, max_det + 8, 11), -7.0, dtype=torch.float32, device=eng.device)
    keep = torch.full((1, max_det + 8), -7, dtype=torch.int32, device=eng.device)
    count = torch.full((1,), -7, dtype=torch.int32, device=eng.device)
    eng.nms_obb_batch(P, 15, dcfg, G, rows=rows, keep=keep, count=count, max_det=max_det)
    rows, keep, k = rows.cpu().numpy()[0], keep.cpu().numpy()[0], int(count.item())
    assert k == max_det
    _check(rows, keep, k, _ref(1025, 15, False, max_det, GEOM1))
    assert np.all(rows[k:] == -7.0) and np.all(keep[k:] == -7)
    eng.check_errors()


def test_nms_obb_batch_of_five_geometries(eng):
    """five images of one launch, each with its own gain, pads and frame size: envelopes clip at different borders"""
    dcfg = DetectConfig()
    counts = [65, 0, 64, 1, 63]
    rows, keep, count = _run(eng, [_field(n) for n in counts], 15, dcfg, GEOMS)
    clipped = 0
    for b, n in enumerate(counts):
        ref = _ref(n, 15, False, 300, GEOMS[b])
        _check(rows[b], keep[b], count[b], ref)
        clipped += int(np.count_nonzero((ref[1][:, 2] == GEOMS[b][3]) | (ref[1][:, 3] == GEOMS[b][4])))
    assert clipped > 0
    eng.check_errors()


def test_nms_obb_on_a_stale_workspace(eng):
    """terms, classes and keys of a larger image, and the axis-aligned rule's boxes and bit matrix (the same bytes), stay in the workspace
    unit; nothing of them may be read"""
    dcfg = DetectConfig()
    for n in (NMS_MAX_CAND, 65, 64, 0, 1025):
        rows, keep, count = _run(eng, [_field(n)], 15, dcfg, [GEOM1])
        _check(rows[0], keep[0], count[0], _ref(n, 15, False, 300, GEOM1))
        P = torch.from_numpy(_field(1025)[None].copy()).to(eng.device)
        G = torch.tensor([GEOM1], dtype=torch.float32, device=eng.device)
        eng.nms_batch(P, 15, dcfg, G, n_extra=1)
    eng.check_errors()


def test_nms_obb_capacity(eng):
    """one candidate over the capacity: count 0 and SS_ERR_CAPACITY at check_errors; the neighbour in the launch is untouched"""
    dcfg = DetectConfig()
    big = R.obb_field(NMS_MAX_CAND + 1, 9000, 15, seed=3, per=64)
    assert int(np.count_nonzero(big[4:19].max(axis=0) > np.float32(dcfg.conf))) == NMS_MAX_CAND + 1
    pad = np.zeros((20, 9000), np.float32)
    pad[:, :84] = _field(65)
    try:
        rows, keep, count = _run(eng, [big, pad], 15, dcfg, [GEOM1, GEOM1])
        assert count[0] == 0
        _check(rows[1], keep[1], count[1], _ref(65, 15, False, 300, GEOM1))
        with pytest.raises(SSError) as ei:
            eng.check_errors()
        assert ei.value.code == SS_ERR_CAPACITY
    finally:
        eng.reset(-1)
    eng.check_errors()
    rows, keep, count = _run(eng, [_field(65)], 15, dcfg, [GEOM1])            # the workspace is usable again
    _check(rows[0], keep[0], count[0], _ref(65, 15, False, 300, GEOM1))
    eng.check_errors()


def test_nms_obb_captured_and_replayed(eng):
    """a HIP graph of the call, replayed on two different tensors: nothing of the first replay is left in the workspace"""
    dcfg = DetectConfig()
    dev = eng.device
    P = torch.zeros(2, 20, 1100, dtype=torch.float32, device=dev)
    G = torch.tensor([GEOM1, GEOMS[1]], dtype=torch.float32, device=dev)
    rows = torch.zeros(2, 300, 11, dtype=torch.float32, device=dev)
    keep = torch.zeros(2, 300, dtype=torch.int32, device=dev)
    count = torch.zeros(2, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        eng.use_current_stream()
        eng.nms_obb_batch(P, 15, dcfg, G, rows=rows, keep=keep, count=count, max_det=300)      # the workspace grows outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            eng.use_current_stream()
            eng.nms_obb_batch(P, 15, dcfg, G, rows=rows, keep=keep, count=count, max_det=300)
    torch.cuda.synchronize(dev)
    eng.use_current_stream()
    small = np.zeros((20, 1100), np.float32)
    small[:, :84] = _field(65)
    for first, second in ((_field(1025), small), (small, _field(1025))):
        P.copy_(torch.from_numpy(np.stack([first, second])).to(dev))
        torch.cuda.synchronize(dev)
        graph.replay()
        torch.cuda.synchronize(dev)
        r, k, c = rows.cpu().numpy(), keep.cpu().numpy(), count.cpu().numpy()
        for b, (n, g) in enumerate(((1025, GEOM1), (65, GEOMS[1])) if first is not small else ((65, GEOM1), (1025, GEOMS[1]))):
            _check(r[b], k[b], c[b], _ref(n, 15, False, 300, g))
    eng.check_errors()


# ---- ss_byte_update_group_obb (docs/OBB.md §4) against ByteTrackObbRef, bit for bit ----------------------------------------------------
from strongsort_yolo_amd.config import ByteTrackConfig                                                           # noqa: E402

DEV = torch.device("cuda", 0)


def _run_obb(eng, streams, groups):
    """streams: per stream a list of [N, 11] frames (equal lengths); groups: the calls' frame counts -> per stream lists of rows, rboxes"""
    S = len(streams)
    rows_all, rb_all = [[] for _ in range(S)], [[] for _ in range(S)]
    out = torch.zeros(32, S, 256, 8, device=DEV)
    rb = torch.zeros(32, S, 256, 5, device=DEV)
    nout = torch.zeros(32, S, dtype=torch.int32, device=DEV)
    f0 = 0
    for n in groups:
        hd, hn = np.zeros((n, S, 128, 11), np.float32), np.zeros((n, S), np.int32)
        for f in range(n):
            for s in range(S):
                d = streams[s][f0 + f]
                hd[f, s, :min(len(d), 128)], hn[f, s] = d[:128], len(d)
        eng.update_group(n, torch.from_numpy(hd).to(DEV), torch.from_numpy(hn).to(DEV), None, None, out[:n], nout[:n], rbox=rb[:n])
        ho, hr, hno = out[:n].cpu().numpy(), rb[:n].cpu().numpy(), nout[:n].cpu().numpy()
        for f in range(n):
            for s in range(S):
                rows_all[s].append(ho[f, s, :hno[f, s]].copy())
                rb_all[s].append(hr[f, s, :hno[f, s]].copy())
        f0 += n
    return rows_all, rb_all


def _same(got, ref, what):
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), f"{what}:\n{got}\n!=\n{ref}"


def _against_ref(eng, cfg, streams, groups, what):
    rows, rbs = _run_obb(eng, streams, groups)
    eng.check_errors()
    for s, frames in enumerate(streams):
        ref = R.ByteTrackObbRef(cfg)
        for k, d in enumerate(frames):
            r, b = ref.update(d)
            _same(rows[s][k], r, f"{what} stream {s} frame {k} rows")
            _same(rbs[s][k], b, f"{what} stream {s} frame {k} rboxes")
        t = eng.tracks(s)
        ids, st, act, mean = ref.tracks()
        assert t["n_tracked"] == len(ref.tracked) and t["n_lost"] == len(ref.lost) and t["next_id"] == ref.next_id
        assert np.array_equal(t["track_id"], ids) and np.array_equal(t["state"], st) and np.array_equal(t["activated"], act)
        assert t["mean"].tobytes() == mean.tobytes(), f"{what} stream {s}: track means"
        assert eng.angles(s).tobytes() == ref.angles().tobytes(), f"{what} stream {s}: angles"
    return rows, rbs


@pytest.fixture(scope="module")
def scenes():
    return {1: R.rotating_scene(1), 2: R.rotating_scene(2), 3: R.rotating_scene(3), 4: R.rotating_scene(1, lane=6.0)}


@pytest.mark.parametrize("kalman", ["xyah", "xywh"])
def test_byte_obb_group_equals_the_reference(kalman, scenes):
    """three streams with different scenes (on the third the axis-aligned tracker gives other ids with either filter:
    tests/test_obb_cpu.py), 40 frames as groups of 32 + 1 + 7: rows, rboxes, the track table and the angles"""
    from strongsort_yolo_amd.engine import ByteTrackEngine
    cfg = ByteTrackConfig(kalman=kalman)
    eng = ByteTrackEngine(cfg, 3, 0, obb=True)
    _against_ref(eng, cfg, [scenes[1], scenes[2], scenes[4]], (32, 1, 7), kalman)
    eng.close()


def test_byte_obb_group_sizes_and_reset(scenes):
    """1 + 4 frames against 5 in one call; after reset the stream starts over with id 1"""
    from strongsort_yolo_amd.engine import ByteTrackEngine
    cfg = ByteTrackConfig()
    eng = ByteTrackEngine(cfg, 1, 0, obb=True)
    five = [scenes[3][:5]]
    a, ra = _run_obb(eng, five, (1, 4))
    eng.reset()
    b, rb = _against_ref(eng, cfg, five, (5,), "after reset")
    for k in range(5):
        _same(a[0][k], b[0][k], f"frame {k}")
        _same(ra[0][k], rb[0][k], f"frame {k} rbox")
    eng.close()


def _crowd(seed, n):
    """n elongated boxes on a grid with random angles, jittered frame to frame by the caller; scores straddle the thresholds"""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    b = np.stack([60.0 + 110.0 * (i % 12), 40.0 + 45.0 * (i // 12), np.full(n, 90.0), np.full(n, 16.0), rng.uniform(0, np.pi, n)], 1)
    return b.astype(np.float32), rng.uniform(0.15, 0.95, n).astype(np.float32)


@pytest.mark.parametrize("kalman", ["xyah", "xywh"])
def test_byte_obb_crowded_frames_past_a_wave_and_an_empty_one(kalman):
    """65 rows (past a wave), 128 rows (SS_MAX_DETS), 0 rows, then 128 again: cost matrices past the LDS cap go through the spill area"""
    from strongsort_yolo_amd.engine import ByteTrackEngine
    cfg = ByteTrackConfig(kalman=kalman)
    frames = []
    for k, n in enumerate((65, 128, 128, 0, 128, 65)):
        b, sc = _crowd(9, 128)
        b[:, 0] += np.float32(2.0 * k)
        b[:, 4] = (b[:, 4] + np.float32(0.03 * k)) % R.F32_PI
        frames.append(R.obb_rows(R.regularise(b[:n]), sc[:n], np.zeros(n, np.float32)))
    eng = ByteTrackEngine(cfg, 1, 0, obb=True)
    _against_ref(eng, cfg, [frames], (1, 5), kalman)
    eng.close()


def test_byte_obb_over_full_table_sets_the_capacity_flag():
    from strongsort_yolo_amd.engine import ByteTrackEngine
    cfg = ByteTrackConfig(max_tracks=16)
    frames = []
    for k in range(3):
        b, _ = _crowd(4, 12)
        b[:, 1] += np.float32(2000.0 * k)
        frames.append(R.obb_rows(R.regularise(b), np.full(12, 0.9, np.float32), np.zeros(12, np.float32)))
    eng = ByteTrackEngine(cfg, 1, 0, obb=True)
    rows, rbs = _run_obb(eng, [frames], (3,))
    ref = R.ByteTrackObbRef(cfg)
    for k, d in enumerate(frames):
        r, b = ref.update(d)
        _same(rows[0][k], r, f"frame {k}")
        _same(rbs[0][k], b, f"frame {k} rbox")
    assert ref.capacity_error
    with pytest.raises(SSError) as ei:
        eng.check_errors()
    assert ei.value.code == SS_ERR_CAPACITY
    eng.reset()
    eng.check_errors()
    eng.close()


def test_byte_obb_captured_launch(scenes):
    """a HIP graph of one frame's call, replayed over the scene's frames"""
    from strongsort_yolo_amd.engine import ByteTrackEngine
    cfg = ByteTrackConfig()
    eng = ByteTrackEngine(cfg, 1, 0, obb=True)
    dets = torch.zeros(1, 1, 128, 11, device=DEV)
    nd = torch.zeros(1, 1, dtype=torch.int32, device=DEV)
    out = torch.zeros(1, 1, 256, 8, device=DEV)
    rb = torch.zeros(1, 1, 256, 5, device=DEV)
    nout = torch.zeros(1, 1, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        eng.use_current_stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            eng.use_current_stream()
            eng.update_group(1, dets, nd, None, None, out, nout, rbox=rb)
    torch.cuda.synchronize(DEV)
    eng.use_current_stream()
    ref = R.ByteTrackObbRef(cfg)
    for k, d in enumerate(scenes[1][:12]):
        hd = np.zeros((1, 1, 128, 11), np.float32)
        hd[0, 0, :len(d)] = d
        dets.copy_(torch.from_numpy(hd).to(DEV))
        nd.fill_(len(d))
        torch.cuda.synchronize(DEV)
        graph.replay()
        torch.cuda.synchronize(DEV)
        r, b = ref.update(d)
        n = int(nout[0, 0])
        _same(out[0, 0, :n].cpu().numpy(), r, f"replay {k}")
        _same(rb[0, 0, :n].cpu().numpy(), b, f"replay {k} rbox")
    eng.check_errors()
    eng.close()


def test_plain_byte_entry_is_what_it_was_around_oriented_boxes(scenes):
    """the plain entry on the same context before ss_byte_set_obb(1) and after ss_byte_set_obb(0) equals ByteTrackRef; while oriented boxes
    are on it is refused by name, and so are GMC warps"""
    from strongsort_yolo_amd.engine import ByteTrackEngine
    from tests.bytetrack_ref import ByteTrackRef
    from tests.test_gpu_bytetrack import _run_engine
    cfg = ByteTrackConfig(kalman="xywh")
    plain = [[d[:, :6].copy() for d in scenes[2][:16]]]
    want = []
    ref = ByteTrackRef(cfg)
    for d in plain[0]:
        want.append(ref.update(d))
    eng = ByteTrackEngine(cfg, 1, 0)
    before = _run_engine(eng, plain, 16)
    eng.set_obb(True)
    from strongsort_yolo_amd.engine import _ptr
    d6, n1 = torch.zeros(1, 1, 128, 6, device=DEV), torch.zeros(1, 1, dtype=torch.int32, device=DEV)
    o8 = torch.zeros(1, 1, 256, 8, device=DEV)
    with pytest.raises(SSError, match="ss_byte_update_group_obb"):                       # refused before anything is launched
        eng._ck(eng.L.ss_byte_update_group(eng.ctx, 1, _ptr(d6), _ptr(n1), _ptr(o8), _ptr(n1)))
    with pytest.raises(SSError, match="ss_byte_set_obb"):
        eng.set_cmc(torch.zeros(1, 1, 8, dtype=torch.float64, device=DEV))
    eng.set_obb(False)
    # ss_byte_set_obb's own refusals through the C ABI: while GMC warps, ReID or the keypoint term are on
    from strongsort_yolo_amd.lib import SS_ERR_INVALID, SS_OK
    warps = torch.zeros(1, 1, 8, dtype=torch.float64, device=DEV)
    eng.set_cmc(warps)
    assert eng.L.ss_byte_set_obb(eng.ctx, 1) == SS_ERR_INVALID
    eng.set_cmc(None)
    assert eng.L.ss_byte_set_reid(eng.ctx, 1, 0.5, 0.25, 0.9) == SS_OK and eng.L.ss_byte_set_obb(eng.ctx, 1) == SS_ERR_INVALID
    assert eng.L.ss_byte_set_reid(eng.ctx, 0, 0.5, 0.25, 0.9) == SS_OK
    sg = (ctypes.c_double * 17)(*([0.05] * 17))
    assert eng.L.ss_byte_set_pose(eng.ctx, 1, 17, sg, 0.5, 0.25, 0.5, 3) == SS_OK and eng.L.ss_byte_set_obb(eng.ctx, 1) == SS_ERR_INVALID
    assert eng.L.ss_byte_set_pose(eng.ctx, 0, 17, sg, 0.5, 0.25, 0.5, 3) == SS_OK
    assert eng.L.ss_byte_set_obb(eng.ctx, 1) == SS_OK
    eng.obb = True
    _against_ref(eng, cfg, [scenes[2][:8]], (8,), "between")
    eng.set_obb(False)
    after = _run_engine(eng, plain, 16)
    for k in range(16):
        _same(before[0][k], want[k], f"before, frame {k}")
        _same(after[0][k], want[k], f"after, frame {k}")
    eng.close()


# ---- YOLO("yolov8n-obb.pt") end to end on synthetic heads (docs/OBB.md §5) -----------------------------------------------------------------
E2E_HW, E2E_NF = (64, 64), 20


def _obb_model(tracker_type="bytetrack"):
    """the model with its head replaced by filled tensors [4 + 15 + 1][A]: a rotating scene's boxes scaled into the 64 x 64 frame, one
    per anchor column, their scores in the class rows, their angles in the last row -> (model, frames, the filled tensors)"""
    from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO("yolov8n-obb.pt", tracker_type=tracker_type, random_init_ok=True)
    model.overrides.update(conf=0.25, iou=0.4, agnostic_nms=False, max_det=300)
    model._pipe_kw.update(det_source="synthetic")
    g = letterbox_geometry(*E2E_HW)
    gain, pad_x, pad_y = scale_geometry(g, *E2E_HW)
    A = sum((g.out_h // s) * (g.out_w // s) for s in (8, 16, 32))
    preds = np.zeros((E2E_NF, 20, A), np.float32)
    for k, rows in enumerate(R.rotating_scene(2, frames=E2E_NF)):
        n = len(rows)
        b = rows[:, 6:11].copy()
        b[:, :4] *= np.float32(0.1)                                        # the scene's 640-pixel field into the 64-pixel frame ...
        b[:, 0], b[:, 1] = b[:, 0] * np.float32(gain) + np.float32(pad_x), b[:, 1] * np.float32(gain) + np.float32(pad_y)   # ... as network-input pixels
        b[:, 2:4] *= np.float32(gain)
        preds[k, :4, :n], preds[k, 19, :n] = b[:, :4].T, b[:, 4]
        preds[k, 4 + (np.arange(n) % 3), np.arange(n)] = rows[:, 4]
    dp = torch.from_numpy(preds).to(DEV)
    model._fill = lambda b, v, k: b.pred_in[v].copy_(dp[k])
    frames = [np.full(E2E_HW + (3,), 7 * k % 256, np.uint8) for k in range(E2E_NF)]
    return model, frames, preds, (gain, pad_x, pad_y, float(E2E_HW[1]), float(E2E_HW[0]))


def test_yolo_obb_predict_equals_nms_rotated():
    model, frames, preds, geom = _obb_model()
    for k in (0, 5, E2E_NF - 1):
        model._frame_index = k
        r = model.predict(frames[k])[0]
        keep, rows = R.nms_rotated(preds[k], 15, 0.25, 0.4, False, 300, geom)
        assert model._pred_pipe.pred_in.shape[1] == 20 and model._pred_pipe.nx == 5 and r.boxes is None and len(r.obb) == len(rows) > 0
        assert bits_equal(r.obb.xywhr.numpy(), rows[:, 6:]) and bits_equal(r.obb.xyxy.numpy(), rows[:, :4])
        assert bits_equal(r.obb.conf.numpy(), rows[:, 4]) and bits_equal(r.obb.cls.numpy(), rows[:, 5]) and r.obb.id is None
        assert r.obb.xyxyxyxy.shape == (len(rows), 4, 2)
    model.close()


@pytest.mark.parametrize("tracker_type", ["bytetrack", "botsort"])
def test_yolo_obb_track_and_stream_equal_the_reference(tracker_type):
    from strongsort_yolo_amd.config import byte_config
    model, frames, preds, geom = _obb_model(tracker_type)
    ref, per_frame = R.ByteTrackObbRef(byte_config(tracker_type)), []
    for k in range(E2E_NF):
        r = model.track(frames[k], tracker=f"{tracker_type}.yaml")[0]
        pipe = model._pipe
        dets = pipe.detections()[0]
        keep, rows = R.nms_rotated(preds[k], 15, 0.1, 0.4, False, 128, geom)
        assert pipe.reid is None and pipe.dcfg.conf == 0.1 and bits_equal(dets, rows)
        exp, erb = ref.update(dets)
        exp, erb = exp[exp[:, 7] >= 0], erb[exp[:, 7] >= 0]
        assert r.boxes is None and len(r.obb) == len(exp), f"frame {k}"
        assert bits_equal(r.obb.id.numpy(), exp[:, 4]) and bits_equal(r.obb.xyxy.numpy(), exp[:, :4]) and bits_equal(r.obb.xywhr.numpy(), erb)
        assert bits_equal(r.obb.conf.numpy(), exp[:, 6]) and bits_equal(r.obb.cls.numpy(), exp[:, 5])
        per_frame.append(r)
    assert ref.next_id > 3 and any(len(r.obb) for r in per_frame)
    model._frame_index = 0
    got = list(model.track_stream(frames, batch=32))
    assert len(got) == E2E_NF
    for k, (a, b) in enumerate(zip(got, per_frame)):
        a = a[0]
        assert a.boxes is None and len(a.obb) == len(b.obb), f"frame {k}"
        if len(b.obb):
            assert torch.equal(a.obb.id, b.obb.id) and torch.equal(a.obb.xywhr, b.obb.xywhr) and torch.equal(a.obb.xyxy, b.obb.xyxy)
            assert torch.equal(a.obb.conf, b.obb.conf) and torch.equal(a.obb.cls, b.obb.cls)
    model.close()


def test_yolo_obb_real_network_gives_finite_rows():
    """the seeded random-init network itself (no trained checkpoint exists here): shapes and finiteness only"""
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO("yolov8n-obb.pt", tracker_type="bytetrack", random_init_ok=True)
    img = np.random.default_rng(0).integers(0, 256, E2E_HW + (3,), dtype=np.uint8)
    model.overrides.update(conf=0.999)
    model.predict(img)
    pred = model._pred_pipe.pred_in[0].cpu()
    assert pred.shape[0] == 20 and torch.isfinite(pred).all()
    # untrained scores have no meaning: the threshold that lets about 200 of the anchors through (the candidate cap is 8192)
    conf = float(pred[4:19].max(0).values.sort(descending=True).values[200])
    model.overrides.update(conf=conf)
    r = model.predict(img)[0]
    assert 0 < len(r.obb) <= 200
    assert r.boxes is None and r.obb.xywhr.shape == (len(r.obb), 5) and torch.isfinite(r.obb.xywhr).all() and torch.isfinite(r.obb.xyxy).all()
    t = model.track(img, tracker="bytetrack.yaml", conf=conf)[0]
    assert t.boxes is None and t.obb.xywhr.shape == (len(t.obb), 5) and torch.isfinite(t.obb.xywhr).all()
    model.close()


def test_cli_tracks_an_obb_model_and_writes_both_labels_files(tmp_path):
    """--track --tracker bytetrack with --count, --gsi, --zone and --save: <name>_labels.txt keeps its format with the envelopes,
    <name>_labels_obb.txt beside it holds `frame cls id conf cx cy w h theta` of the same rows"""
    from strongsort_yolo_amd import cli, zones
    model, frames, preds, geom = _obb_model("bytetrack")
    np.save(tmp_path / "clip.npy", np.stack(frames))
    out = cli.process_video({"source": str(tmp_path / "clip.npy"), "track": True, "count": True, "tracker": "bytetrack", "batch": 8,
                             "outdir": str(tmp_path), "gsi": True, "zones": [zones.parse_zone("2,2,62,2,62,62,2,62")],
                             "save": str(tmp_path / "out.npy")}, model=model)
    assert out["frames"] == E2E_NF and sum(out["counts"].values()) >= 3 and "zones" in out and out["gsi_rows"] > 0
    plain = [ln.split() for ln in open(tmp_path / "clip_labels.txt")]
    obb = [ln.split() for ln in open(tmp_path / "clip_labels_obb.txt")]
    assert len(plain) == len(obb) > E2E_NF and all(len(p) == 12 and len(q) == 9 for p, q in zip(plain, obb))
    assert all(p[:4] == q[:4] for p, q in zip(plain, obb))                                   # frame, cls, id, conf of the same rows
    assert all(int(p[4]) <= float(q[4]) <= int(p[6]) + 1 and 0.0 <= float(q[8]) < 3.1416 for p, q in zip(plain, obb))   # the envelope holds the centre
    assert (tmp_path / "clip_labels_gsi.txt").exists() and (tmp_path / "clip_zones.json").exists()
    assert np.load(tmp_path / "out.npy").shape == (E2E_NF,) + E2E_HW + (3,)
    model.close()


def test_stand_alone_byte_tracker_on_oriented_boxes(scenes):
    from strongsort_yolo_amd.tracker import BYTETracker
    cfg = ByteTrackConfig(kalman="xywh")
    with pytest.raises(ValueError, match="obb=True"):
        BYTETracker(cfg, camera_motion=True, obb=True)
    trk, ref = BYTETracker(cfg, obb=True), R.ByteTrackObbRef(cfg)
    for k, d in enumerate(scenes[3][:10]):
        got = trk.update(np.concatenate([d[:, 6:11], d[:, 4:6]], 1))
        rows, rbox = ref.update(d)
        _same(got, np.concatenate([rows, rbox], 1), f"frame {k}")
    with pytest.raises(ValueError, match="7"):
        trk.update(np.zeros((2, 6), np.float32))
    trk.close()
