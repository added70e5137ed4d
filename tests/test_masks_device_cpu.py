"""Device masks (YOLO(device_masks=True), csrc/ss_mask.hip), the parts that need no GPU: the float32 restatement of k_mask_assemble
against the host recipe (yolo.assemble_masks), the C ABI's argument checks, and the device-backed form of yolo.Masks.

`restate_masks` is the specification of k_mask_assemble: tests/test_gpu_masks.py holds the kernel's bits to it bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

F32 = np.float32


def _axis(n_in, n_out):
    """Bilinear source index / weights of one axis, align_corners=False, in float32: scale = in / out,
    src = max(0, (dst + 0.5) * scale - 0.5), i0 = trunc(src), l1 = src - i0, l0 = 1 - l1, i1 = min(i0 + 1, in - 1)."""
    scale = F32(n_in) / F32(n_out)
    src = np.maximum(F32(0), (np.arange(n_out, dtype=F32) + F32(0.5)) * scale - F32(0.5))
    i0 = src.astype(np.int32)
    l1 = src - i0.astype(F32)
    return i0, np.minimum(i0 + 1, n_in - 1), F32(1) - l1, l1


def restate_values(proto, coef, boxes, gain, pad, in_hw):
    """k_mask_assemble's pre-threshold values, float32 op for op.  proto [nm, mh, mw] (read as float32), coef [n, nm], boxes [n, 4]
    in ORIGINAL pixels, gain / pad_xy the frame's letterbox (float32), in_hw the network input -> float32 [n, ih, iw]."""
    proto = np.asarray(proto, np.float32)
    coef, boxes = np.asarray(coef, F32), np.asarray(boxes, F32)
    nm, mh, mw = proto.shape
    ih, iw = in_hw
    g, px, py = F32(gain), F32(pad[0]), F32(pad[1])
    fx, fy = F32(mw / iw), F32(mh / ih)
    yi0, yi1, ly0, ly1 = _axis(mh, ih)
    xi0, xi1, lx0, lx1 = _axis(mw, iw)
    col, row = np.arange(mw, dtype=F32)[None, :], np.arange(mh, dtype=F32)[:, None]
    out = np.zeros((len(coef), ih, iw), F32)
    for i in range(len(coef)):
        x1, y1 = (boxes[i, 0] * g + px) * fx, (boxes[i, 1] * g + py) * fy
        x2, y2 = (boxes[i, 2] * g + px) * fx, (boxes[i, 3] * g + py) * fy
        acc = np.zeros((mh, mw), F32)
        for k in range(nm):                                   # multiply, then add, k ascending
            acc = acc + coef[i, k] * proto[k]
        m = np.where((col >= x1) & (col < x2) & (row >= y1) & (row < y2), acc, F32(0))
        top, bot = m[yi0], m[yi1]                             # [ih, mw]
        ly0c, ly1c = ly0[:, None], ly1[:, None]
        out[i] = (top[:, xi0] * lx0 + top[:, xi1] * lx1) * ly0c + (bot[:, xi0] * lx0 + bot[:, xi1] * lx1) * ly1c
    return out


def restate_masks(proto, coef, boxes, gain, pad, in_hw):
    return restate_values(proto, coef, boxes, gain, pad, in_hw) > 0


def pack_masks(masks):
    """bool [n, ih, iw] -> int32 [n, ih, ceil(iw/32)], bit x % 32 of word x / 32 = pixel (y, x) (the kernels' layout)."""
    masks = np.asarray(masks, bool)
    n, ih, iw = masks.shape
    wpr = (iw + 31) // 32
    padded = np.zeros((n, ih, wpr * 32), bool)
    padded[..., :iw] = masks
    return np.packbits(padded, axis=-1, bitorder="little").view("<u4").astype(np.uint32).view(np.int32).reshape(n, ih, wpr)


def _host_values(proto, coef, boxes_in, in_hw):
    """yolo.assemble_masks without its final `> 0`."""
    import torch.nn.functional as F
    c, mh, mw = proto.shape
    ih, iw = in_hw
    n = coef.shape[0]
    m = (coef.float() @ proto.float().reshape(c, -1)).view(n, mh, mw)
    b = boxes_in.float().clone()
    b[:, [0, 2]] *= mw / iw
    b[:, [1, 3]] *= mh / ih
    x1, y1, x2, y2 = (b[:, i].view(n, 1, 1) for i in range(4))
    col = torch.arange(mw, dtype=torch.float32).view(1, 1, mw)
    row = torch.arange(mh, dtype=torch.float32).view(1, mh, 1)
    m = m * ((col >= x1) & (col < x2) & (row >= y1) & (row < y2))
    return F.interpolate(m[None], (ih, iw), mode="bilinear", align_corners=False)[0]


def random_rows(rng, n, nm, w0, h0):
    """n detection boxes in original pixels (some crossing every edge, some zero-width or inverted) and their coefficients."""
    cx, cy = rng.uniform(-0.1 * w0, 1.1 * w0, n), rng.uniform(-0.1 * h0, 1.1 * h0, n)
    bw, bh = rng.uniform(0, 0.6 * w0, n), rng.uniform(0, 0.6 * h0, n)
    boxes = np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1).astype(F32)
    if n > 3:
        boxes[1, 2] = boxes[1, 0]                              # zero width
        boxes[2, [0, 2]] = boxes[2, [2, 0]]                    # inverted
        boxes[3] = (-20, -20, w0 + 20, h0 + 20)                # the whole frame and beyond
    return boxes, rng.standard_normal((n, nm)).astype(F32)


@pytest.mark.parametrize("seed,f16", [(0, True), (1, False), (2, True)])
def test_restatement_equals_host_assemble_masks(seed, f16):
    """configs[1] geometry (480x640 frame, 384x640 input, 32x96x160 prototypes), 28 masks: the restatement's masks equal
    assemble_masks except where the host's own pre-threshold value is within 1e-5 of 0 (BLAS summation order)."""
    from strongsort_yolo_amd.yolo import assemble_masks
    rng = np.random.default_rng(seed)
    nm, mh, mw, ih, iw, h0, w0 = 32, 96, 160, 384, 640, 480, 640
    gain, pad = F32(1.0), (F32(0.0), F32(32.0))
    proto = rng.standard_normal((nm, mh, mw)).astype(F32)
    if f16:
        proto = proto.astype(np.float16).astype(F32)
    boxes, coef = random_rows(rng, 28, nm, w0, h0)
    got = restate_masks(proto, coef, boxes, gain, pad, (ih, iw))
    b = torch.from_numpy(boxes).clone()                        # YOLO._results: x * gain + pad in float32
    b[:, [0, 2]] = b[:, [0, 2]] * float(gain) + float(pad[0])
    b[:, [1, 3]] = b[:, [1, 3]] * float(gain) + float(pad[1])
    host = assemble_masks(torch.from_numpy(proto), torch.from_numpy(coef), b, (ih, iw)).numpy()
    hv = _host_values(torch.from_numpy(proto), torch.from_numpy(coef), b, (ih, iw)).numpy()
    diff = got != host
    assert not (diff & (np.abs(hv) > 1e-5)).any()
    assert host.sum() > 1000 and diff.sum() <= 1e-4 * diff.size


def test_pack_masks_layout():
    m = np.zeros((1, 2, 40), bool)
    m[0, 0, 0] = m[0, 1, 33] = m[0, 1, 31] = True
    p = pack_masks(m).view(np.uint32)
    assert p.shape == (1, 2, 2) and p[0, 0, 0] == 1 and p[0, 1, 0] == 1 << 31 and p[0, 1, 1] == 2


def _lib():
    from strongsort_yolo_amd import lib
    lib.build()
    return lib, lib.load()


def _assemble_args(**kw):
    a = dict(ctx=None, stream=None, proto=C.c_void_p(64), f16=1, proto_fs=32 * 96 * 160, nm=32, mh=96, mw=160, dets=C.c_void_p(64),
             dets_fs=128 * 38, ld=38, coef_off=6, counts=C.c_void_p(64), F=2, R=128, geom=C.c_void_p(64), geom_fs=5, ih=384, iw=640,
             bits=C.c_void_p(64), bits_fs=128 * 384 * 20)
    a.update(kw)
    return list(a.values())


def _outline_args(**kw):
    a = dict(ctx=None, stream=None, bits=C.c_void_p(64), bits_fs=128 * 384 * 20, counts=C.c_void_p(64), F=2, R=128, ih=384, iw=640,
             cap=2048, pts=C.c_void_p(64), pts_fs=128 * 2048 * 2, npts=C.c_void_p(64), npts_fs=128, copy=None, copy_fs=0,
             scratch=C.c_void_p(64), scratch_bytes=64 * 384 * 640 * 4)
    a.update(kw)
    return list(a.values())


def test_mask_entry_points_reject_bad_arguments_without_a_gpu():
    """ss_mask_assemble / ss_mask_outline check every argument before the context and the device: SS_ERR_INVALID and a message
    that names the problem (with a NULL context, so nothing can reach the GPU)."""
    lib, L = _lib()
    assert "ss_mask_assemble" in lib.EXPORTS and "ss_mask_outline" in lib.EXPORTS

    def rejects(fn, args, words):
        assert fn(*args) == lib.SS_ERR_INVALID
        msg = L.ss_last_error(None).decode()
        assert words in msg, msg

    A, O = L.ss_mask_assemble, L.ss_mask_outline
    rejects(A, _assemble_args(proto=None), "null pointer")
    rejects(A, _assemble_args(bits=None), "null pointer")
    rejects(A, _assemble_args(nm=0), "nm")
    rejects(A, _assemble_args(nm=65, ld=80), "nm")
    rejects(A, _assemble_args(ih=380), "4 x the prototype")
    rejects(A, _assemble_args(mw=300, iw=1200), "4 x the prototype")
    rejects(A, _assemble_args(F=0), "n_frames")
    rejects(A, _assemble_args(R=70000), "max_rows")
    rejects(A, _assemble_args(ld=37), "coefficient")
    rejects(A, _assemble_args(coef_off=2), "coefficient")
    rejects(A, _assemble_args(bits_fs=100), "strides")
    rejects(A, _assemble_args(), "null context")                     # every argument right: the context is what is missing
    rejects(O, _outline_args(scratch=None), "null pointer")
    rejects(O, _outline_args(pts=None), "null pointer")
    rejects(O, _outline_args(ih=1024, iw=1024), "LDS")
    rejects(O, _outline_args(ih=0), "LDS")
    rejects(O, _outline_args(cap=0), "cap")
    rejects(O, _outline_args(scratch_bytes=384 * 640 * 4 - 1), "scratch")
    rejects(O, _outline_args(F=0), "n_frames")
    rejects(O, _outline_args(pts_fs=10), "strides")
    rejects(O, _outline_args(copy=C.c_void_p(64), copy_fs=5), "strides")
    rejects(O, _outline_args(), "null context")


def test_yolo_accepts_device_masks():
    from strongsort_yolo_amd.yolo import YOLO
    assert YOLO("yolov8n-seg.pt", random_init_ok=True, device_masks=True).device_masks is True
    assert YOLO("yolov8n-seg.pt", random_init_ok=True).device_masks is False


def test_cli_passes_device_masks_through(monkeypatch):
    from strongsort_yolo_amd import cli, yolo
    seen = {}

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(yolo, "YOLO", fake)
    with pytest.raises(Stop):
        cli.main(["--source", "synthetic:1", "--device-masks"])
    assert seen.get("device_masks") is True


def test_device_backed_masks_unpack_scale_and_index():
    """Masks(_bits=, _polys=): .data unpacks the bits, .xy applies only scale_coords to the device polygons (None: traced on the
    host from the unpacked mask), indexing by det_idx keeps bits and polygons in step."""
    from strongsort_yolo_amd.yolo import Masks, mask_polygon
    rng = np.random.default_rng(4)
    n, ih, iw = 3, 40, 70
    data = np.zeros((n, ih, iw), bool)
    data[0, 5:20, 10:30] = True
    data[1, 0:ih, 60:70] = True
    data[2, 30:33, 3:5] = True
    data[2] |= rng.random((ih, iw)) > 0.97
    bits = pack_masks(data)
    polys = [mask_polygon(data[0]), None, mask_polygon(data[2])]
    coef, boxes = torch.zeros(n, 4), torch.zeros(n, 4)
    dev = Masks(None, coef, boxes, (ih, iw), (50, 80), 0.875, (0.0, 2.5), _bits=bits, _polys=polys)
    host = Masks(None, coef, boxes, (ih, iw), (50, 80), 0.875, (0.0, 2.5), _data=torch.from_numpy(data))
    assert torch.equal(dev.data, torch.from_numpy(data))
    assert all(np.array_equal(a, b) and a.dtype == np.float32 for a, b in zip(dev.xy, host.xy))
    di = torch.tensor([2, 0])
    sub = dev[di]
    assert torch.equal(sub.data, torch.from_numpy(data[[2, 0]])) and all(np.array_equal(a, host.xy[k]) for a, k in zip(sub.xy, (2, 0)))
    one = dev[1]
    assert len(one) == 1 and np.array_equal(one.xy[0], host.xy[1])
