"""Device masks on the MI355X (csrc/ss_mask.hip): k_mask_assemble bit for bit against the float32 restatement
(tests/test_masks_device_cpu.py), k_mask_outline point for point against yolo.mask_polygon, and YOLO(device_masks=True) end to end."""
import numpy as np
import pytest
import torch

from tests.test_masks_device_cpu import pack_masks, random_rows, restate_masks

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def eng():
    from tests.gpu_util import engine
    e = engine(debug=False)
    yield e
    e.close()


@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("geom", [(96, 160, 480, 640), (160, 160, 640, 640), (24, 40, 96, 160)])     # yolov8n-seg / yolo11n-seg inputs, a small one
def test_assemble_equals_restatement(eng, f16, geom):
    """Four frames of one group with 0, 1, 28 and 128 rows, each with its own letterbox; boxes crossing every edge, zero-width and
    inverted ones; rows past the counts are left untouched."""
    mh, mw, h0, w0 = geom
    ih, iw, nm, R, F = 4 * mh, 4 * mw, 32, 128, 4
    wpr = (iw + 31) // 32
    rng = np.random.default_rng(mh + f16)
    counts = [0, 1, 28, 128]
    proto = rng.standard_normal((F, nm, mh, mw)).astype(np.float16 if f16 else F32)
    dets = np.zeros((F, R, 6 + nm), F32)
    geo = np.zeros((F, 5), F32)
    for f in range(F):
        gain = F32(min(ih / h0, iw / w0) * (1.0 - 0.1 * f))
        geo[f, :3] = gain, F32((iw - w0 * gain) / 2), F32((ih - h0 * gain) / 2)
        boxes, coef = random_rows(rng, R, nm, w0, h0)
        dets[f, :, :4], dets[f, :, 6:] = boxes, coef
    dev = eng.device
    sentinel = -123456
    bits = torch.full((F, R, ih, wpr), sentinel, dtype=torch.int32, device=dev)
    eng.mask_assemble(torch.from_numpy(proto).to(dev), torch.from_numpy(dets).to(dev), torch.tensor(counts, dtype=torch.int32, device=dev),
                      torch.from_numpy(geo).to(dev), 6, bits)
    torch.cuda.synchronize()
    got = bits.cpu().numpy()
    for f, n in enumerate(counts):
        ref = restate_masks(proto[f].astype(F32), dets[f, :n, 6:], dets[f, :n, :4], geo[f, 0], geo[f, 1:3], (ih, iw))
        assert np.array_equal(got[f, :n], pack_masks(ref)), f"frame {f}: {int((got[f, :n] != pack_masks(ref)).sum())} words differ"
        assert (got[f, n:] == sentinel).all()
    assert got[2, :28].any() and got[3].any()


def _hand_masks(h, w):
    """Masks the outline kernel must trace exactly as yolo.mask_polygon."""
    ms = []
    m = np.zeros((h, w), bool); ms.append(m)                                       # empty
    ms.append(np.ones((h, w), bool))                                               # full image
    m = np.zeros((h, w), bool); m[5, 7] = True; ms.append(m)                       # one isolated pixel
    m = np.zeros((h, w), bool); m[3, 3:5] = True; m[10, 10] = m[11, 11] = True; ms.append(m)          # 2-pixel components
    m = np.zeros((h, w), bool); m[4:9, 4:9] = True; m[14:19, 14:19] = True; m[2:7, 30:35] = True; ms.append(m)   # three tied in size
    m = np.zeros((h, w), bool)
    for i in range(40):                                                            # more than 16 components, sizes 1..4, ties
        y, x = 2 + 6 * (i // 8), 2 + 6 * (i % 8)
        m[y, x:x + 1 + i % 4] = True
    ms.append(m)
    m = np.zeros((h, w), bool); m[5:25, 5:25] = True; m[10:20, 10:20] = False; m[14, 14] = True; ms.append(m)   # ring + island in its hole
    m = np.zeros((h, w), bool)
    y0, x0, y1, x1 = 1, 1, h - 2, w - 2                                            # spiral
    while y0 <= y1 and x0 <= x1:
        m[y0, x0:x1 + 1] = m[y0:y1 + 1, x1] = m[y1, x0:x1 + 1] = True
        m[y0 + 2:y1 + 1, x0] = True
        y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
    ms.append(m)
    m = np.zeros((h, w), bool); m[0:8, 0:6] = True; m[h - 5:h, w - 9:w] = True; m[0, w - 1] = True; m[h - 1, 0] = True; ms.append(m)  # borders
    m = np.zeros((h, w), bool); m[::2, ::2] = True; m[1::2, 1::2] = True; ms.append(m)   # checkerboard: one 8-connected component
    rng = np.random.default_rng(11)
    for p in (0.3, 0.5, 0.7):
        ms.append(rng.random((h, w)) < p)                                          # noise: many components, holes
    m = np.zeros((h, w), bool); m[8:30, 3:w - 3] = True; m[12:26, 9:w - 9] = False; ms.append(m)     # thin ring
    m = np.zeros((h, w), bool); m[::2, ::2] = True; m[1, 1:5] = True; ms.append(m)       # isolated dots: 700 / 1 536 components (more
    #                                                                                       than the kernel's LDS root list at 64 x 96)
    return np.stack(ms)


@pytest.mark.parametrize("hw", [(40, 70), (64, 96)])
def test_outline_equals_mask_polygon_on_hand_made_masks(eng, hw):
    from strongsort_yolo_amd.yolo import mask_polygon
    h, w = hw
    masks = _hand_masks(h, w)
    n = len(masks)
    dev = eng.device
    F, R, cap = 2, n, 4096
    bits = torch.zeros(F, R, h, (w + 31) // 32, dtype=torch.int32)
    bits[0] = torch.from_numpy(pack_masks(masks))
    bits[1, :n - 3] = torch.from_numpy(pack_masks(masks[::-1][:n - 3].copy()))
    counts = torch.tensor([n, n - 3], dtype=torch.int32, device=dev)
    pts = torch.full((F, R, cap, 2), -7, dtype=torch.int32, device=dev)
    npts = torch.full((F, R), -99999, dtype=torch.int32, device=dev)
    scratch = torch.empty(3 * h * w, dtype=torch.int32, device=dev)                # 3 workgroups for 2 x n masks: persistent loop
    copy = torch.zeros_like(bits).pin_memory()
    eng.mask_outline(bits.to(dev), counts, w, pts, npts, scratch, bits_copy=copy)
    torch.cuda.synchronize()
    P, N = pts.cpu().numpy(), npts.cpu().numpy()
    assert torch.equal(copy[0], bits[0]) and torch.equal(copy[1, :n - 3], bits[1, :n - 3])
    for f, ms in ((0, masks), (1, masks[::-1][:n - 3])):
        for r, m in enumerate(ms):
            ref = mask_polygon(m)
            assert N[f, r] == len(ref), (f, r, N[f, r], len(ref))
            assert np.array_equal(P[f, r, :N[f, r]].astype(F32), ref), (f, r)
    assert (N[1, n - 3:] == -99999).all()


def test_outline_longer_than_cap_reports_length_and_falls_back(eng):
    """A polygon longer than cap writes no points and reports -length; yolo.Masks then traces that mask on the host: same polygon."""
    from strongsort_yolo_amd.yolo import Masks, mask_polygon
    h, w = 64, 96
    masks = _hand_masks(h, w)
    dev = eng.device
    n, cap = len(masks), 16
    pts = torch.zeros(1, n, cap, 2, dtype=torch.int32, device=dev)
    npts = torch.zeros(1, n, dtype=torch.int32, device=dev)
    eng.mask_outline(torch.from_numpy(pack_masks(masks))[None].to(dev), torch.tensor([n], dtype=torch.int32, device=dev), w, pts, npts,
                     torch.empty(64 * h * w, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    P, N = pts.cpu().numpy()[0], npts.cpu().numpy()[0]
    refs = [mask_polygon(m) for m in masks]
    assert any(len(r) > cap for r in refs) and any(0 < len(r) <= cap for r in refs)
    for r, ref in enumerate(refs):
        assert N[r] == (len(ref) if len(ref) <= cap else -len(ref))
    polys = [P[r, :k].astype(F32) if k >= 0 else None for r, k in enumerate(N.tolist())]
    z = torch.zeros(n, 4)
    dm = Masks(None, z, z, (h, w), (h, w), 1.0, (0.0, 0.0), _bits=pack_masks(masks), _polys=polys)
    hm = Masks(None, z, z, (h, w), (h, w), 1.0, (0.0, 0.0), _data=torch.from_numpy(masks))
    assert all(np.array_equal(a, b) for a, b in zip(dm.xy, hm.xy))


def _device_restatement(pipe, f, idx):
    """The restatement on the prototypes and rows the device holds for frame f of the pipeline (FramePipeline: f = 0)."""
    d = pipe.dets[f].cpu().numpy()[idx]
    return restate_masks(pipe.proto[f].float().cpu().numpy(), d[:, 6 + pipe.nk:6 + pipe.nk + pipe.nm], d[:, :4],
                         pipe.geom_dev[f, 0].item(), pipe.geom_dev[f, 1:3].cpu().numpy(), (pipe.geom.out_h, pipe.geom.out_w))


def test_yolo_device_masks_end_to_end():
    """YOLO("yolov8n-seg.pt", device_masks=True): predict (the tracking pipeline, max_det 40, and the wide detection-only one, max_det
    300), track (4 calls on one frame: tracks confirm) and track_stream(batch=2) give the default model's boxes and ids;
    masks.data = the restatement on the prototypes of the frame and differs from the host masks only where the host value is within
    1e-5 of 0; masks.xy[i] = the host polygon of the device mask; two fresh runs agree bit for bit."""
    from strongsort_yolo_amd.yolo import YOLO, Masks
    from tests.test_masks_device_cpu import _host_values
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(6)]

    def model(dm):
        m = YOLO("yolov8n-seg.pt", device_masks=dm)
        m.overrides.update(conf=0.5, iou=0.4, agnostic_nms=False, max_det=40)   # random-init head: many anchors pass
        return m

    def check_masks(r, pipe, idx, host):
        n = len(r.boxes)
        assert r.masks is not None and len(r.masks) == n
        assert np.array_equal(r.masks.data.numpy(), _device_restatement(pipe, 0, idx))
        hd = host.masks.data.numpy() if host is not None else None
        if hd is not None:
            d = pipe.dets[0].cpu()[idx]
            b = d[:, :4].clone()
            b[:, [0, 2]] = b[:, [0, 2]] * pipe.gain + pipe.pad_x
            b[:, [1, 3]] = b[:, [1, 3]] * pipe.gain + pipe.pad_y
            hv = _host_values(pipe.proto[0].cpu(), d[:, 6:6 + pipe.nm], b, (pipe.geom.out_h, pipe.geom.out_w)).numpy()
            diff = r.masks.data.numpy() != hd
            assert not (diff & (np.abs(hv) > 1e-5)).any()
        ref = Masks(None, torch.zeros(n, 4), torch.zeros(n, 4), r.masks._in_hw, r.masks.orig_shape, r.masks._gain, r.masks._pad,
                    _data=r.masks.data)
        assert all(np.array_equal(a, b) for a, b in zip(r.masks.xy, ref.xy))

    def check_stream_masks(r, host):
        """track_stream: the buffer set a group used is refilled by later groups, so the frame's prototypes are the ones the
        default model downloaded for the same frame (Masks._proto; equal boxes, same network) and its boxes in input pixels."""
        hm = host.masks
        exp = restate_masks(hm._proto.float().numpy(), hm._coef.numpy(), hm._boxes.numpy(), 1.0, (0.0, 0.0), hm._in_hw)
        assert np.array_equal(r.masks.data.numpy(), exp)               # x * 1 + 0 = x: the boxes enter the kernel's grid arithmetic as-is
        hv = _host_values(hm._proto, hm._coef, hm._boxes, hm._in_hw).numpy()
        assert not ((r.masks.data.numpy() != hm.data.numpy()) & (np.abs(hv) > 1e-5)).any()

    runs = []
    for _ in range(2):
        md, mh = model(True), model(False)
        out = []
        a, b = md.predict(frames[0])[0], mh.predict(frames[0])[0]
        assert torch.equal(a.boxes.xyxy, b.boxes.xyxy) and len(a.boxes) > 0
        check_masks(a, md._pipe, np.arange(len(a.boxes)), b)
        out.append((a.boxes.xyxy.numpy().copy(), a.masks.data.numpy().copy(), [p.copy() for p in a.masks.xy]))
        md.overrides["max_det"] = mh.overrides["max_det"] = 300                   # > 128: the detection-only pipeline of 1 024 rows
        a, b = md.predict(frames[1])[0], mh.predict(frames[1])[0]
        assert torch.equal(a.boxes.xyxy, b.boxes.xyxy) and len(a.boxes) > 40
        check_masks(a, md._pred_pipe, np.arange(len(a.boxes)), b)
        out.append((a.boxes.xyxy.numpy().copy(), a.masks.data.numpy().copy(), [p.copy() for p in a.masks.xy]))
        md.overrides["max_det"] = mh.overrides["max_det"] = 40
        checked = 0
        for k in range(4):
            a, b = md.track(frames[0], persist=True)[0], mh.track(frames[0], persist=True)[0]
            assert torch.equal(a.boxes.xyxy, b.boxes.xyxy) and (a.boxes.id is None) == (b.boxes.id is None)
            if a.boxes.id is not None:
                assert torch.equal(a.boxes.id, b.boxes.id)
                rows = md._pipe.out[0].cpu()[:int(md._pipe.nout[0])]
                di = rows[rows[:, 7] >= 0][:, 7].long().numpy()
                check_masks(a, md._pipe, di, b)
                checked += 1
                out.append((a.boxes.id.numpy().copy(), a.masks.data.numpy().copy(), [p.copy() for p in a.masks.xy]))
        assert checked >= 2                                                       # confirmed from the third call on
        md.close(); mh.close()
        md, mh = model(True), model(False)
        seq = [frames[0]] * 4 + [frames[1]] * 4                                   # tracks confirm within each half
        rs_d = [r[0] for r in md.track_stream(iter(seq), batch=2, device=0)]
        rs_h = [r[0] for r in mh.track_stream(iter(seq), batch=2, device=0)]
        assert len(rs_d) == len(rs_h) == len(seq)
        checked = 0
        for a, b in zip(rs_d, rs_h):
            assert torch.equal(a.boxes.xyxy, b.boxes.xyxy)
            assert (a.boxes.id is None) == (b.boxes.id is None) and (a.boxes.id is None or torch.equal(a.boxes.id, b.boxes.id))
            if a.masks is not None:
                assert len(a.masks) == len(a.boxes)
                n = len(a.boxes)
                ref = Masks(None, torch.zeros(n, 4), torch.zeros(n, 4), a.masks._in_hw, a.masks.orig_shape, a.masks._gain, a.masks._pad,
                            _data=a.masks.data)
                assert all(np.array_equal(u, v) for u, v in zip(a.masks.xy, ref.xy))
                check_stream_masks(a, b)
                checked += 1
                out.append((a.masks.data.numpy().copy(), [p.copy() for p in a.masks.xy]))
        assert checked >= 4
        md.close(); mh.close()
        runs.append(out)

    def same(x, y):
        if isinstance(x, (list, tuple)):
            return len(x) == len(y) and all(same(u, v) for u, v in zip(x, y))
        return np.array_equal(x, y)
    assert same(runs[0], runs[1])
