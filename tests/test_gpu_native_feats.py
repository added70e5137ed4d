"""BoT-SORT's `model: auto` ReID features on the MI355X (csrc/ss_native.hip k_native_feats, docs/BYTETRACK.md §1d): the kernel
through the C ABI against tests/native_feats_ref.py bit for bit, the features both pipelines hand the tracker against the
restatement of that step's own head inputs and keep list, the tracked rows against ByteTrackEngine and BotSortReidRef, and
the fp32 features against Ultralytics' expression on the CPU fp32 detector."""
import numpy as np
import pytest
import torch

from strongsort_yolo_amd.config import ByteTrackConfig, DetectConfig
from strongsort_yolo_amd.synth import make_stream
from tests.botsort_reid_ref import BotSortReidRef
from tests.native_feats_ref import native_feats, ultralytics_obj_feats

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
REID = ByteTrackConfig(kalman="xywh", with_reid=True)
SHAPES = ((12, 20), (6, 10), (3, 5))
A_ = sum(h * w for h, w in SHAPES)


def _maps(chans, dtype, B, seed, slice_level=1):
    """Device maps [B, C_l, H_l, W_l] channels-last; level `slice_level` is a channel slice of a wider map."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for lv, (c, (h, w)) in enumerate(zip(chans, SHAPES)):
        extra = 24 if lv == slice_level else 0
        x = (torch.randn(B, c + extra, h, w, generator=g) * 2).to(dtype).to(DEV).contiguous(memory_format=torch.channels_last)
        out.append(x[:, 16:16 + c] if extra else x)
    return out


def _keep(B, counts, seed):
    rng = np.random.default_rng(seed)
    k = np.full((B, 128), -5, np.int32)
    edges = [0, 239, 240, 299, 300, 314]
    for b, n in enumerate(counts):
        row = rng.integers(0, A_, n).astype(np.int32)
        row[:min(n, len(edges))] = edges[:min(n, len(edges))]
        k[b, :n] = row
    return k


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("chans", [(64, 128, 256), (128, 256, 512), (192, 384, 576), (256, 512, 512)])
def test_kernel_equals_restatement(dtype, chans):
    from strongsort_yolo_amd.engine import TrackerEngine
    eng = TrackerEngine(n_streams=1)
    counts = [0, 1, 128, 57, 6]
    B = len(counts)
    maps = _maps(chans, dtype, B, seed=chans[0] + (dtype == torch.float16))
    if chans[0] == 128:
        maps[2] = maps[2].contiguous()                          # channel stride != 1: the engine copies it channels-last first
    keep = _keep(B, counts, chans[1])
    out = torch.full((B, 128, 512), float("nan"), device=DEV)
    eng.native_feats(maps, torch.from_numpy(keep).to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV), out)
    torch.cuda.synchronize()
    eng.check_errors()
    got = out.cpu().numpy()
    ref = native_feats([m.cpu() for m in maps], keep, counts)
    s = min(chans)
    for b, n in enumerate(counts):
        assert got[b, :n].tobytes() == ref[b, :n].tobytes(), (b, n)
        assert not got[b, :n, s:].any()                          # columns s..511: zeros
        assert np.isnan(got[b, n:]).all()                        # rows past the count: not written
    eng.close()


def test_kernel_argument_checks():
    from strongsort_yolo_amd import lib
    from strongsort_yolo_amd.engine import TrackerEngine, _ptr
    eng = TrackerEngine(n_streams=1)
    L, B = eng.L, 2
    maps = _maps((64, 128, 256), torch.float16, B, 5, slice_level=-1)
    keep = torch.zeros(B, 128, dtype=torch.int32, device=DEV)
    cnt = torch.full((B,), 3, dtype=torch.int32, device=DEV)
    out = torch.full((B, 128, 512), float("nan"), device=DEV)

    def desc():
        d = (lib.ss_native_map * 3)()
        for x, m in zip(d, maps):
            x.data, x.img_stride, x.row_stride, x.pix_stride = m.data_ptr(), m.stride(0), m.stride(2), m.stride(3)
            x.channels, x.height, x.width = m.shape[1], m.shape[2], m.shape[3]
        return d

    def call(n_img=B, half=1, d=None, s=64, keep_p=_ptr(keep), ks=128, cnt_p=_ptr(cnt), out_p=_ptr(out)):
        return L.ss_native_feats(eng.ctx, n_img, half, desc() if d is None else d, s, keep_p, ks, cnt_p, out_p)

    def bad(**kw):
        d = desc()
        for k, v in kw.pop("map", {}).items():
            setattr(d[1], k, v)
        return call(d=d, **kw)

    assert call() == lib.SS_OK                                   # the valid call the cases below break one argument of
    torch.cuda.synchronize()
    out.fill_(float("nan"))
    torch.cuda.synchronize()
    cases = [dict(n_img=0), dict(n_img=65536), dict(half=2), dict(s=0), dict(s=513), dict(s=48), dict(s=128), dict(ks=127),
             dict(keep_p=None), dict(cnt_p=None), dict(out_p=None), dict(map={"data": 0}), dict(map={"data": maps[1].data_ptr() + 1}),
             dict(map={"height": 0}), dict(map={"width": 0}), dict(map={"pix_stride": 127}), dict(map={"row_stride": 128 * 10 - 1}),
             dict(map={"img_stride": 10}), dict(map={"channels": 96})]
    for kw in cases:
        assert bad(**kw) == lib.SS_ERR_INVALID, kw
    assert L.ss_native_feats(eng.ctx, B, 1, None, 64, _ptr(keep), 128, _ptr(cnt), _ptr(out)) == lib.SS_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                # nothing was launched
    with pytest.raises(ValueError):                              # the engine: mixed dtypes, a wrong output shape
        eng.native_feats([maps[0], maps[1].float(), maps[2]], keep, cnt, out)
    with pytest.raises(ValueError):
        eng.native_feats(maps, keep, cnt, out[:, :64])
    with pytest.raises(lib.SSError):                             # s = 512 > the smallest map's channels
        eng.native_feats(maps, keep, cnt, out, s=512)
    eng.close()


# ---- the pipelines -------------------------------------------------------------------------------------------------------------
H_, W_, NF_ = 480, 640, 24


@pytest.fixture
def spy(monkeypatch):
    """Every FramePipeline also keeps the head inputs its last forward pre-hook saw (the captured graph's own tensors)."""
    from strongsort_yolo_amd.pipeline import FramePipeline
    orig = FramePipeline._take_head_inputs

    def take(self, module, args):
        orig(self, module, args)
        self._test_maps = list(args[0])

    monkeypatch.setattr(FramePipeline, "_take_head_inputs", take)


def _auto_model(weights="yolov8n.pt", half=True, cmc=False):
    from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry
    from strongsort_yolo_amd.synth import synth_prediction
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO(weights, random_init_ok=True, tracker_type="botsort", with_reid=True, reid_model="auto", half=half, camera_motion=cmc)
    model.overrides.update(conf=0.3, iou=0.4, agnostic_nms=False, max_det=1000)
    model._pipe_kw.update(det_source="synthetic")
    g = letterbox_geometry(H_, W_)
    gs = scale_geometry(g, H_, W_)
    A = sum((g.out_h // s) * (g.out_w // s) for s in (8, 16, 32))
    nk = 51 if "pose" in weights else 0
    nm = 32 if "seg" in weights else 0
    nc = 1 if nk else 80
    st, rng = make_stream(47, W_, H_, 9), np.random.default_rng(47)
    frames, preds = [], []
    for k in range(NF_):
        d = st.next_frame().dets.copy()
        d[:, 4] = np.where(rng.random(len(d)) < 0.3, rng.uniform(0.12, 0.24, len(d)), d[:, 4]).astype(np.float32)   # low-score rows
        if nk:
            d[:, 5] = 0
        pred, _ = synth_prediction(d, A, nc, gs[0], (gs[1], gs[2]), rng)
        if nk or nm:                                             # keypoint / mask-coefficient rows: any values
            pred = np.concatenate([pred, rng.uniform(0, 400, (nk + nm, A)).astype(np.float32)])
        frames.append(st.frame_pixels(k).copy()); preds.append(pred)
    dp = torch.from_numpy(np.stack(preds)).to(DEV)
    model._fill = lambda b, v, k: b.pred_in[v].copy_(dp[k])
    return model, frames


def _assert_rows(got, ref, what):
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), f"{what}:\n{got}\n!=\n{ref}"


def _track_checked(model, frames, cmc=False):
    """track() frame by frame: the features the tracker read equal the restatement of that step's head inputs and keep list,
    and the rows equal a ByteTrackEngine and BotSortReidRef fed with the pipeline's rows and those features."""
    from strongsort_yolo_amd.engine import ByteTrackEngine
    eng, ref, per_frame, rows_seen = ByteTrackEngine(REID, 1, 0), BotSortReidRef(REID), [], 0
    for k in range(NF_):
        res = model.track(frames[k], verbose=False, device=0, persist=True, tracker="botsort.yaml")
        pipe = model._pipe
        assert pipe.native and pipe.reid is None and pipe.crops.numel() == 0 and pipe.max_det == 128
        assert pipe.byte is not None and pipe.byte.reid
        n = int(pipe.ndets[0])
        feats = pipe.feats_in[0, :n].cpu().numpy()
        want = native_feats(pipe._test_maps, pipe.keep, pipe.ndets)[0, :n]
        assert feats.tobytes() == want.tobytes(), f"features, frame {k}"
        rows_seen += n
        rows = pipe.detections()[0][:, :6]
        d = torch.zeros(1, 128, 6, device=DEV)
        f = torch.zeros(1, 128, 512, device=DEV)
        d[0, :n], f[0, :n] = torch.from_numpy(rows).to(DEV), torch.from_numpy(feats).to(DEV)
        w = None
        if cmc:
            w = pipe.warps.clone()
            eng.set_cmc(w)
        o, no = eng.update_device(d, torch.full((1,), n, dtype=torch.int32, device=DEV), f)
        e = o[0, :int(no[0])].cpu().numpy()
        _assert_rows(e, ref.update(rows, feats, None if w is None else w[0, 0].cpu().numpy()), f"engine, frame {k}")
        r = res[0]
        assert len(r.boxes) == len(e), f"frame {k}"
        if len(e):
            assert np.array_equal(r.boxes.id.numpy(), e[:, 4]) and np.array_equal(r.boxes.xyxy.numpy(), e[:, :4]), f"frame {k}"
        per_frame.append(r)
    assert rows_seen > 50
    eng.close()
    return per_frame


def _same(a, b, what):
    assert len(a.boxes) == len(b.boxes), what
    if len(b.boxes):
        assert torch.equal(a.boxes.id, b.boxes.id) and torch.equal(a.boxes.xyxy, b.boxes.xyxy) and torch.equal(a.boxes.conf, b.boxes.conf), what


@pytest.mark.parametrize("weights,half", [("yolov8n.pt", True), ("yolov8n.pt", False), ("yolo11n-pose.pt", True), ("yolov8n-seg.pt", True)])
def test_track_features_and_rows(spy, weights, half):
    model, frames = _auto_model(weights, half)
    _track_checked(model, frames)
    assert model._pipe.dtype == (torch.float16 if half else torch.float32)
    model.close()


@pytest.mark.parametrize("cmc", [False, True])
def test_track_stream_equals_track(spy, cmc):
    model, frames = _auto_model(cmc=cmc)
    per_frame = _track_checked(model, frames, cmc)
    for batch in (32, 7):                                          # a full group; a partial last group (24 = 3 x 7 + 3)
        model._frame_index = 0
        got = list(model.track_stream(frames, batch=batch))
        p = model._stream_pipe
        assert len(got) == NF_ and p.native and p.reid is None and p.crops.numel() == 0 and p.byte.reid and p.max_det == 128
        for k, (a, b) in enumerate(zip(got, per_frame)):
            _same(a[0], b, f"track_stream batch {batch} frame {k}")
    model.close()


@pytest.mark.parametrize("half", [True, False])
def test_overlapped_pipeline_features_every_group(half):
    """OverlappedPipeline group by group: feats_v of every real frame equals the restatement of the buffer set's own head inputs
    (stage 0's graph tensors, read by the NMS stage's graph) and keep list."""
    from strongsort_yolo_amd.pipeline import OverlappedPipeline
    model, frames = _auto_model(half=half)
    F = 7
    pipe = OverlappedPipeline("yolov8n", 1, (H_, W_), half=half, tracker="botsort", with_reid=True, reid_model="auto", frame_batch=F,
                              graph="front", defer_track=True, det_source="synthetic", dcfg=DetectConfig(conf=0.1, iou=0.4, max_det=1000))
    assert pipe.reid is None and pipe.n == 2
    checked = 0
    for g0 in range(0, NF_, F):
        chunk = frames[g0:g0 + F]
        b = pipe.begin_frame()
        with torch.cuda.stream(pipe.s_in):
            pipe.eng.upload_batch(b.frames, chunk, pipe.s_in)
            for f in range(len(chunk)):
                model._fill(b, f, g0 + f)
        pipe.submit(len(chunk))
        pipe.flush()
        torch.cuda.synchronize()
        pipe.eng.check_errors()
        want = native_feats(b.maps, b.keep, b.ndets)
        got = b.feats_v.cpu().numpy()
        for v, n in enumerate(b.ndets.cpu().numpy()[:len(chunk)]):
            assert got[v, :n].tobytes() == want[v, :n].tobytes(), f"group {g0 // F} frame {v}"
            checked += int(n)
    assert checked > 50
    pipe.close()
    model.close()


def test_fp32_features_match_ultralytics_on_the_cpu_network(spy):
    """half=False: the features equal Ultralytics' get_obj_feats on the CPU fp32 detector's own head inputs (pre-hook on the CPU
    module, same seed, the pipeline's letterboxed frame) to within 2e-5 of the feature table's scale — the fp32 detector's
    agreement with the CPU network (tests/test_gpu_detector32.py)."""
    from strongsort_yolo_amd import nets
    model, frames = _auto_model(half=False)
    cpu = nets.build_detector("yolov8n", model.seed).float().eval()
    seen = {}
    cpu.detect.register_forward_pre_hook(lambda m, a: seen.__setitem__("maps", list(a[0])))
    worst = 0.0
    for k in range(6):
        model.track(frames[k], verbose=False, device=0, persist=True, tracker="botsort.yaml")
        pipe = model._pipe
        n = int(pipe.ndets[0])
        with torch.no_grad():
            cpu(pipe.lb.cpu().contiguous())
        ult = ultralytics_obj_feats(seen["maps"], [pipe.keep[0, :n].long().cpu()])[0]
        got = pipe.feats_in[0, :n].cpu()
        s = ult.shape[1]
        assert not got[:, s:].any()
        scale = ult.abs().max().item() + 1e-30
        err = (got[:, :s].double() - ult.double()).abs().max().item() if n else 0.0
        worst = max(worst, err / scale)
        assert err <= 2e-5 * scale, (k, err, scale)
    print(f"fp32 features vs Ultralytics' expression on the CPU network: max |diff| / scale = {worst:.3g}")
    model.close()


def test_bytetracker_pads_short_features():
    """BYTETracker(reid_model="auto") with a detector's own k-long vectors: the rows equal the reference fed the zero-padded ones."""
    from strongsort_yolo_amd.tracker import BYTETracker
    from tests.test_gpu_botsort_reid import reid_stream
    st = reid_stream(80, 30)
    trk, ref = BYTETracker(REID, reid_model="auto"), BotSortReidRef(REID)
    assert trk.reid is None
    for k, (d, f) in enumerate(st):
        short = f[:, :64]
        pad = np.zeros_like(f)
        pad[:, :64] = short
        _assert_rows(trk.update(d, features=short), ref.update(d, pad), f"frame {k}")
    with pytest.raises(ValueError):                               # no features: auto has no network to run on the frame
        trk.update(st[0][0], np.zeros((64, 64, 3), np.uint8))
    with pytest.raises(ValueError):
        trk.update(st[0][0], features=np.zeros((len(st[0][0]), 513), np.float32))
    trk.close()
