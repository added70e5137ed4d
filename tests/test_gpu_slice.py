"""Sliced inference on the device (csrc/ss_slice.hip, docs/SLICE.md): the tiled letterbox against the existing letterbox on crops and the
C oracle, the cross-tile merge against tests/slice_ref.py bit for bit, and the pipelines end to end."""
import functools

import numpy as np
import pytest
import torch

from oracle import cexact
from strongsort_yolo_amd import lib, slicing
from strongsort_yolo_amd.engine import LetterboxGeom
from tests import slice_fields as sf, slice_ref as ref
from tests.gpu_util import engine, bits_equal

pytestmark = pytest.mark.gpu
SEED = 7                      # tests/test_slice_cpu.py checks on the reference alone that this seed's fields are not vacuous


@pytest.fixture(scope="module")
def eng():
    e = engine(debug=False)
    yield e
    e.close()


# ---- letterbox --------------------------------------------------------------------------------------------------------------
def _frames(H, W, pitch, seed):
    """batch 2, rows of `pitch` bytes (> 3 * W): the frames are a view into a wider buffer."""
    rng = np.random.default_rng(seed)
    wide = rng.integers(0, 256, (2, H, pitch), dtype=np.uint8)
    return wide, wide[:, :, :3 * W].reshape(2, H, W, 3)


@pytest.mark.parametrize("hw,imgsz", [((64, 64), 96), ((50, 70), 96), ((64, 64), 64)], ids=["scaled", "odd", "identity"])
def test_letterbox_equals_the_existing_one_on_crops(eng, hw, imgsz):
    H, W, pitch = 96, 160, 3 * 160 + 13
    cfg = slicing.SliceConfig(hw, 0.25, True)
    g, table = slicing.canvas(H, W, cfg, imgsz=imgsz)
    T = len(table)
    assert T == 7 or hw != (64, 64)
    if imgsz == 64:
        assert (table[0][4], table[0][5]) == (64, 64)            # the identity path: new size == tile size
    wide, frames = _frames(H, W, pitch, 3)
    d_wide = torch.from_numpy(wide).to(eng.device)
    d_frames = torch.as_strided(d_wide, (2, H, W, 3), (H * pitch, pitch, 3, 1))
    eng.slice_config(table, (H, W), (g.out_h, g.out_w), 8)
    for half in (False, True):
        for cl in (False, True):
            got = eng.slice_letterbox_batch(d_frames, half=half, channels_last=cl)
            assert got.shape == (2 * T, 3, g.out_h, g.out_w)
            got = got.cpu().numpy()
            for b in range(2):
                for t, (x0, y0, tw, th, nw, nh, pl, pt) in enumerate(table.tolist()):
                    crop = np.ascontiguousarray(frames[b, y0:y0 + th, x0:x0 + tw])
                    tg = LetterboxGeom(g.out_h, g.out_w, nh, nw, pt, pl, 0.0)
                    want = eng.letterbox_batch(torch.from_numpy(crop[None]).to(eng.device), tg, half=half, channels_last=cl).cpu().numpy()[0]
                    assert bits_equal(got[b * T + t], want), (b, t, half, cl)
                    if not half and not cl:
                        assert bits_equal(got[b * T + t], cexact.letterbox(crop, g.out_h, g.out_w, nh, nw, pt, pl)), (b, t)


def test_letterbox_unaligned_output(eng):
    """An output that starts off a 16-byte boundary: every line has head and tail values, none may leak outside it."""
    H, W = 96, 160
    cfg = slicing.SliceConfig((50, 70), 0.25, True)
    g, table = slicing.canvas(H, W, cfg, imgsz=96)
    T = len(table)
    _, frames = _frames(H, W, 3 * W, 5)
    d_frames = torch.from_numpy(np.ascontiguousarray(frames)).to(eng.device)
    eng.slice_config(table, (H, W), (g.out_h, g.out_w), 8)
    want = eng.slice_letterbox_batch(d_frames, half=True, channels_last=True)
    n = want.numel()
    buf = torch.full((n + 16,), 7.0, dtype=torch.float16, device=eng.device)
    out = torch.as_strided(buf, want.shape, want.stride(), storage_offset=3)          # 6 bytes off
    eng.slice_letterbox_batch(d_frames, half=True, channels_last=True, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert bool((buf[:3] == 7.0).all()) and bool((buf[n + 3:] == 7.0).all())


# ---- merge ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _field(name, seed, n_extra=0):
    su = sf.setup(name)
    return (su,) + sf.field(su, seed, n_extra=n_extra)


def _run(eng, su, rows, counts, mode, metric, agnostic, out_cap, n_extra=0, n_kpt=0, thr=0.5):
    """One device call on B frames (rows [B,T,R,ld], counts [B,T]) -> per-frame (rows, count, src)."""
    eng.slice_config(su["table"], (su["H"], su["W"]), (su["g"].out_h, su["g"].out_w), su["R"], n_extra=n_extra, n_kpt=n_kpt, kpt_geom=su["frame_geom"])
    o, c, s = eng.slice_merge(torch.from_numpy(rows).to(eng.device), torch.from_numpy(counts).to(eng.device), mode, metric, thr, agnostic, out_cap)
    torch.cuda.synchronize()
    o, c, s = o.cpu().numpy(), c.cpu().numpy(), s.cpu().numpy()
    return [(o[b, :c[b]], int(c[b]), s[b, :c[b]]) for b in range(len(c))]


def _want(su, rows, counts, mode, metric, agnostic, out_cap, n_kpt=0, thr=0.5, stats=False):
    return ref.merge(rows, counts, su["table"][:, :2], su["R"], mode, metric, thr, agnostic, out_cap, n_kpt=n_kpt, tile_geom=su["tile_geom"],
                     frame_geom=su["frame_geom"], want_stats=stats)


def _same(got, want):
    return got[1] == want[1] and np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])


ALL = [(mo, me, ag) for mo in ("nmm", "nms") for me in ("ios", "iou") for ag in (False, True)]


@pytest.mark.parametrize("mode,metric,agnostic", ALL)
@pytest.mark.parametrize("name", list(sf.CASES))
def test_merge_bit_exact(eng, name, mode, metric, agnostic):
    su, rows, counts, seen = _field(name, SEED)
    assert int(counts.sum()) == su["total"]
    got = _run(eng, su, rows[None], counts[None], mode, metric, agnostic, 1024)[0]
    want = _want(su, rows, counts, mode, metric, agnostic, 1024, stats=True)
    assert _same(got, want)
    if su["total"] >= 63:                                          # the field is not vacuous
        assert (seen >= 2).mean() >= 1 / 3
        merged_all = _want(su, rows, counts, mode, metric, agnostic, su["T"] * su["R"])[1]
        assert merged_all < su["total"]
        if mode == "nmm":
            assert want[3]["rechecks"] >= 1


@pytest.mark.parametrize("out_cap", [1, 128, 1024])
def test_merge_out_cap(eng, out_cap):
    su, rows, counts, _ = _field("n1025", SEED)
    got = _run(eng, su, rows[None], counts[None], "nmm", "ios", False, out_cap)[0]
    want = _want(su, rows, counts, "nmm", "ios", False, out_cap)
    assert _same(got, want) and got[1] == min(out_cap, _want(su, rows, counts, "nmm", "ios", False, 8192)[1])


@pytest.mark.parametrize("name", ["n64", "n1025"])
def test_merge_counts_outside_the_rows(eng, name):
    """A count above rows_per_tile is read as rows_per_tile, a negative one as 0."""
    su, rows, counts, _ = _field(name, SEED)
    rows, counts = rows.copy(), counts.copy()
    R = su["R"]
    rng = np.random.default_rng(2)
    rows[1, :, :2] = rng.uniform(0, 40, (R, 2))                   # tile 1: every one of its R rows is a real row now
    rows[1, :, 2:4] = rows[1, :, :2] + rng.uniform(5, 24, (R, 2)).astype(np.float32)
    rows[1, :, 4] = np.linspace(0.9, 0.31, R, dtype=np.float32)
    rows[1, :, 5] = 1.0
    counts[1] = R + 5
    counts[2] = -3
    got = _run(eng, su, rows[None], counts[None], "nmm", "ios", False, 1024)[0]
    want = _want(su, rows, counts, "nmm", "ios", False, 1024)
    assert _same(got, want)
    assert not np.any(got[2] // R == 2) and np.any(got[2] // R == 1)


@pytest.mark.parametrize("name", ["n64", "n1025"])
def test_merge_keypoints(eng, name):
    """n_extra = 51 with 17 keypoint triples: x, y re-expressed in the whole frame's letterbox, confidences and the rest copied."""
    su, rows, counts, _ = _field(name, SEED, 51)
    got = _run(eng, su, rows[None], counts[None], "nmm", "ios", False, 1024, n_extra=51, n_kpt=17)[0]
    want = _want(su, rows, counts, "nmm", "ios", False, 1024, n_kpt=17)
    assert _same(got, want)
    t, r = got[2][0] // su["R"], got[2][0] % su["R"]
    assert np.array_equal(got[0][0, 8::3], rows[t, r, 8::3]) and not np.array_equal(got[0][0, 6:8], rows[t, r, 6:8])
    # with fewer triples than columns the rest is copied as it is
    got = _run(eng, su, rows[None], counts[None], "nmm", "ios", False, 1024, n_extra=51, n_kpt=2)[0]
    assert _same(got, _want(su, rows, counts, "nmm", "ios", False, 1024, n_kpt=2))


def test_merge_grouping_and_capture(eng):
    """5 frames in one call equal 1 + 4 equal the reference; a captured launch replayed on new inputs."""
    su = sf.setup("n1025")
    fields = [sf.field(su, SEED + i)[:2] for i in range(4)] + [sf.field(sf.setup("n65") | dict(R=su["R"]), SEED)[:2]]
    rows, counts = np.stack([f[0] for f in fields]), np.stack([f[1] for f in fields])
    want = [_want(su, rows[b], counts[b], "nmm", "iou", False, 128) for b in range(5)]
    five = _run(eng, su, rows, counts, "nmm", "iou", False, 128)
    split = _run(eng, su, rows[:1], counts[:1], "nmm", "iou", False, 128) + _run(eng, su, rows[1:], counts[1:], "nmm", "iou", False, 128)
    for b in range(5):
        assert _same(five[b], want[b]) and _same(split[b], want[b]), b
    # capture
    dev = eng.device
    d_rows, d_counts = torch.zeros(2, *rows.shape[1:], device=dev), torch.zeros(2, su["T"], dtype=torch.int32, device=dev)
    out = torch.zeros(2, 128, 6, device=dev)
    cnt, src = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, 128, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        eng.use_current_stream()
        eng.slice_merge(d_rows, d_counts, "nmm", "iou", 0.5, False, 128, out, cnt, src)      # the workspace exists before the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            eng.use_current_stream()
            eng.slice_merge(d_rows, d_counts, "nmm", "iou", 0.5, False, 128, out, cnt, src)
    torch.cuda.synchronize(dev)
    eng.use_current_stream()
    for b0 in (0, 2, 3):
        d_rows.copy_(torch.from_numpy(rows[b0:b0 + 2])); d_counts.copy_(torch.from_numpy(counts[b0:b0 + 2]))
        torch.cuda.synchronize(dev)
        graph.replay()
        torch.cuda.synchronize(dev)
        o, c, s = out.cpu().numpy(), cnt.cpu().numpy(), src.cpu().numpy()
        for i in range(2):
            assert _same((o[i, :c[i]], int(c[i]), s[i, :c[i]]), want[b0 + i]), (b0, i)


def test_nms_geometry_rows(eng):
    su = sf.setup("n64")
    eng.slice_config(su["table"], (su["H"], su["W"]), (su["g"].out_h, su["g"].out_w), su["R"])
    g = eng.slice_nms_geom(3).cpu().numpy()
    assert bits_equal(g, np.tile(su["tile_geom"], (3, 1)))


def test_refusals_on_the_device(eng):
    su = sf.setup("n64")
    eng.slice_config(su["table"], (su["H"], su["W"]), (su["g"].out_h, su["g"].out_w), su["R"])
    rows, counts = torch.zeros(1, su["T"], su["R"], 6, device=eng.device), torch.zeros(1, su["T"], dtype=torch.int32, device=eng.device)
    with pytest.raises(lib.SSError, match="out_cap"):
        eng.slice_merge(rows, counts, out_cap=9000, out=torch.zeros(1, 1, 6, device=eng.device))
    with pytest.raises(lib.SSError, match="tiles overlap"):
        eng.slice_merge(torch.zeros(1, su["T"], su["R"] - 1, 6, device=eng.device), counts)      # a tile's rows_per_tile rows run into the next tile's


# ---- end to end -------------------------------------------------------------------------------------------------------------
H_, W_, NF_, IMGSZ_ = 96, 160, 12, 128
DEV = torch.device("cuda", 0)


def _scene(nf, seed, n_obj=7):
    """Boxes drifting over the 96 x 160 frame: per frame rows [n, 6] (x1, y1, x2, y2, score, class) in frame pixels."""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(15, W_ - 15, n_obj), rng.uniform(12, H_ - 12, n_obj)], 1)
    v, wh = rng.uniform(-1.5, 1.5, (n_obj, 2)), rng.uniform(12, 28, (n_obj, 2))
    score, cls = rng.uniform(0.4, 0.9, n_obj), rng.integers(0, 3, n_obj)
    out = []
    for k in range(nf):
        p = c + k * v
        b = np.concatenate([p - wh / 2, p + wh / 2], 1)
        b[:, [0, 2]] = np.clip(b[:, [0, 2]], 0, W_)
        b[:, [1, 3]] = np.clip(b[:, [1, 3]], 0, H_)
        out.append(np.concatenate([b, score[:, None], cls[:, None]], 1).astype(np.float32))
    return out


def _slice_model(weights, nk, **kw):
    """A sliced YOLO on synthetic per-tile heads: every tile's head holds the scene's boxes clipped to that tile -> (model, frames,
    per frame the [T, 4 + nc + nk, A] head tensors, the pipeline-side facts the expectation needs)."""
    from strongsort_yolo_amd.config import DetectConfig
    from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry
    from strongsort_yolo_amd.synth import synth_prediction
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO(weights, random_init_ok=True, tracker_type="bytetrack", slice_hw=(64, 64), slice_overlap=0.25, **kw)
    model.overrides.update(conf=0.3, iou=0.4, agnostic_nms=False, max_det=1000)
    dcfg = DetectConfig(conf=0.1, iou=0.4, agnostic_nms=False, max_det=1000, imgsz=IMGSZ_)     # a 128 x 128 canvas: 336 anchors a tile
    model._pipe_kw.update(det_source="synthetic", dcfg=dcfg)
    g, table = slicing.canvas(H_, W_, model.slice, imgsz=IMGSZ_)
    tg = slicing.nms_geometry(g, table)
    A = sum((g.out_h // s) * (g.out_w // s) for s in (8, 16, 32))
    nc = 1 if nk else 80
    rng = np.random.default_rng(11)
    frames, preds = [], []
    for k, d in enumerate(_scene(NF_, 5)):
        per = []
        for t, (x0, y0, tw, th) in enumerate(table[:, :4].tolist()):
            b = d.copy()
            b[:, [0, 2]] = np.clip(b[:, [0, 2]] - x0, 0, tw)
            b[:, [1, 3]] = np.clip(b[:, [1, 3]] - y0, 0, th)
            b = b[((b[:, 2] - b[:, 0]) >= 6) & ((b[:, 3] - b[:, 1]) >= 6)]
            b[:, 4] += rng.uniform(-0.02, 0.02, len(b)).astype(np.float32)
            if nk:
                b[:, 5] = 0
            b = b[np.argsort(-b[:, 4], kind="stable")]
            pred, _ = synth_prediction(b, A, nc, float(tg[t, 0]), (float(tg[t, 1]), float(tg[t, 2])), rng, dup=2, clutter=0)
            if nk:
                pred = np.concatenate([pred, rng.uniform(0, IMGSZ_, (nk, A)).astype(np.float32)])
            per.append(pred)
        preds.append(np.stack(per))
        frames.append(rng.integers(0, 256, (H_, W_, 3), dtype=np.uint8))
    dp = torch.from_numpy(np.stack(preds)).to(DEV)
    T = len(table)
    model._fill = lambda b, v, k: b.pred_in[v * T:(v + 1) * T].copy_(dp[k])
    gf = letterbox_geometry(H_, W_, IMGSZ_)
    return model, frames, preds, dict(table=table, tg=tg, nc=nc, dcfg=dcfg, frame_geom=scale_geometry(gf, H_, W_), T=T)


def _expected_rows(preds_k, facts, pipe, nk):
    """slice_ref applied to cexact.nms of each tile."""
    dc, R = facts["dcfg"], pipe.tile_rows
    rows, counts = np.zeros((facts["T"], R, 6 + nk), np.float32), np.zeros(facts["T"], np.int32)
    for t in range(facts["T"]):
        keep, r6 = cexact.nms(preds_k[t], facts["nc"], dc.conf, dc.iou, dc.agnostic_nms, dc.max_wh, dc.max_nms, min(pipe.max_det, R))
        gn, px, py, tw, th = (float(v) for v in facts["tg"][t])
        r6 = cexact.scale_boxes(r6, gn, px, py, tw, th)
        rows[t, :len(keep), :6] = r6
        rows[t, :len(keep), 6:] = preds_k[t][4 + facts["nc"]:, keep].T
        counts[t] = len(keep)
    sc = pipe.slice
    return ref.merge(rows, counts, facts["table"][:, :2], R, sc.merge, sc.metric, sc.thr, dc.agnostic_nms, pipe.max_det, n_kpt=nk // 3,
                     tile_geom=facts["tg"], frame_geom=facts["frame_geom"], want_stats=True), int(counts.sum())


@pytest.mark.parametrize("weights,nk", [("yolov8n.pt", 0), ("yolo11n-pose.pt", 51)])
def test_yolo_sliced_track_and_stream_equal_reference(weights, nk):
    from strongsort_yolo_amd.config import ByteTrackConfig
    from tests.bytetrack_ref import ByteTrackRef
    model, frames, preds, facts = _slice_model(weights, nk)
    tracker, per_frame, merged, total = ByteTrackRef(ByteTrackConfig()), [], 0, 0
    for k in range(NF_):
        res = model.track(frames[k], verbose=False, device=0, persist=True, tracker="bytetrack.yaml")
        pipe = model._pipe
        assert pipe.T == 7 and pipe.pred_in.shape[0] == 7 and pipe.lb.shape == (7, 3, IMGSZ_, IMGSZ_) and pipe.tile_rows == 128
        rows = pipe.detections()[0]
        (want, m, src, _), n_tile = _expected_rows(preds[k], facts, pipe, nk)
        assert len(rows) == m and np.array_equal(rows, want)
        assert np.array_equal(pipe.keep[0, :m].cpu().numpy(), src)
        merged, total = merged + m, total + n_tile
        exp = tracker.update(rows[:, :6])
        r = res[0]
        assert len(r.boxes) == len(exp)
        if len(exp):
            assert np.array_equal(r.boxes.id.numpy(), exp[:, 4]) and np.array_equal(r.boxes.xyxy.numpy(), exp[:, :4])
            if nk:
                kk = torch.from_numpy(rows[:, 6:6 + nk]).reshape(len(rows), nk // 3, 3).clone()
                kk[..., 0] = (kk[..., 0] - pipe.pad_x) / pipe.gain
                kk[..., 1] = (kk[..., 1] - pipe.pad_y) / pipe.gain
                assert torch.equal(r.keypoints.data, kk[torch.from_numpy(exp[:, 7]).long()])
        per_frame.append(r)
    assert 0 < merged < total                                  # duplicates along the seams were merged
    model._frame_index = 0
    got = list(model.track_stream(frames, batch=32))
    assert len(got) == NF_ and model._stream_pipe.bufs[0].pred_in.shape[0] == 32 * 7
    for k, (a, b) in enumerate(zip(got, per_frame)):
        a = a[0]
        assert len(a.boxes) == len(b.boxes), f"frame {k}"
        if len(b.boxes):
            assert torch.equal(a.boxes.id, b.boxes.id) and torch.equal(a.boxes.xyxy, b.boxes.xyxy) and torch.equal(a.boxes.conf, b.boxes.conf)
            if nk:
                assert torch.equal(a.keypoints.data, b.keypoints.data)
    model.close()


def test_yolo_sliced_real_network_letterboxes_the_tiles():
    """The real random-init network end to end: predict() runs, and the per-tile detector input equals the existing letterbox on crops."""
    from strongsort_yolo_amd.config import DetectConfig
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack", slice_hw=(64, 64), slice_overlap=0.25)
    model._pipe_kw.update(dcfg=DetectConfig(imgsz=IMGSZ_))
    rng = np.random.default_rng(2)
    frame = rng.integers(0, 256, (H_, W_, 3), dtype=np.uint8)
    res = model.track(frame, verbose=False, device=0, persist=True, tracker="bytetrack.yaml")
    assert isinstance(res, list) and len(res) == 1
    pipe = model._pipe
    assert pipe.det_source == "detector" and pipe.T == 7
    lb = pipe.lb.cpu()
    for t, (x0, y0, tw, th, nw, nh, pl, pt) in enumerate(pipe.tile_table.tolist()):
        crop = torch.from_numpy(np.ascontiguousarray(frame[y0:y0 + th, x0:x0 + tw])[None]).to(pipe.dev)
        tg = LetterboxGeom(pipe.in_geom.out_h, pipe.in_geom.out_w, nh, nw, pt, pl, 0.0)
        want = pipe.eng.letterbox_batch(crop, tg, half=pipe.half, channels_last=True).cpu()
        assert torch.equal(lb[t], want[0]), t
    model.close()


def test_unsliced_pipeline_allocates_nothing_of_it():
    from strongsort_yolo_amd.pipeline import FramePipeline
    p = FramePipeline("yolov8n", 1, (H_, W_), run_nets=False, tracker="bytetrack", graph="none")
    assert p.slice is None and p.T == 1 and not hasattr(p.b, "tile_dets") and p.in_geom is p.geom and p.lb.shape[0] == 1
    p.close()
