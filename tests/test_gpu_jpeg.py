"""Baseline JPEG decoded on the device (csrc/ss_jpeg.hip): byte equality with Pillow's arrays stored in tests/golden/ (the
fixtures' generator is tests/golden/make_jpeg_golden.py; nothing here needs Pillow)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from strongsort_yolo_amd import jpeg, lib
from tests.gpu_util import engine

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def cases():
    z = np.load(os.path.join(GOLD, "jpeg_cases.npz"))
    return [(str(n), z[f"bytes_{i}"].tobytes(), z[f"rgb_{i}"]) for i, n in enumerate(z["names"])]


@pytest.fixture(scope="module")
def sequence():
    z = np.load(os.path.join(GOLD, "jpeg_sequence.npz"))
    return [(z[f"bytes_{i}"].tobytes(), z[f"rgb_{i}"]) for i in range(12)]


@pytest.fixture(scope="module")
def refused():
    z = np.load(os.path.join(GOLD, "jpeg_refused.npz"))
    return z["good"].tobytes(), z["good_rgb"], {k: (z[k].tobytes(), v) for k, v in (str(c).split("=") for c in z["causes"])}


@pytest.fixture(scope="module")
def eng():
    e = engine(debug=False)
    yield e
    e.close()


def _same_size(cases, w, h, n):
    pick = [c for c in cases if c[2].shape[:2] == (h, w)]
    assert len(pick) >= n
    return pick[:n]


def test_every_case_alone_bgr_and_rgb(eng, cases):
    bad = []
    for name, data, rgb in cases:
        f = jpeg.EncodedFrame(data)
        assert f.shape == rgb.shape
        got_bgr = jpeg.decode(eng, [f]).cpu().numpy()[0]
        got_rgb = jpeg.decode(eng, [f], rgb=True).cpu().numpy()[0]
        if not (np.array_equal(got_rgb, rgb) and np.array_equal(got_bgr, rgb[:, :, ::-1])):
            bad.append((name, int((got_rgb != rgb).sum()), int((got_bgr != rgb[:, :, ::-1]).sum())))
    assert not bad, f"{len(bad)} of {len(cases)} cases differ: {bad[:8]}"


@pytest.mark.parametrize("n,w,h", [(5, 17, 9), (32, 33, 31), (32, 3, 5)])
def test_batches_of_same_size_cases(eng, cases, n, w, h):
    pick = _same_size(cases, w, h, n)
    assert len({c[0].split("_")[2] for c in pick}) > 1                   # several samplings in one call
    got = jpeg.decode(eng, [jpeg.EncodedFrame(c[1]) for c in pick], rgb=True).cpu().numpy()
    for k, c in enumerate(pick):
        assert np.array_equal(got[k], c[2]), c[0]


@pytest.mark.parametrize("extra", [64, 5])                                # 5: frames that are not dword-aligned take the byte stores
def test_out_frame_stride_leaves_the_gap_untouched(eng, cases, extra):
    pick = _same_size(cases, 61, 45, 4)
    each = 45 * 61 * 3
    buf = torch.full((4, each + extra), 0xA5, dtype=torch.uint8, device=DEV)
    dst = buf[:, :each].view(4, 45, 61, 3)
    assert dst.stride(0) == each + extra
    eng.jpeg_decode_batch(dst, [jpeg.EncodedFrame(c[1]) for c in pick])
    out = buf.cpu().numpy()
    assert (out[:, each:] == 0xA5).all()
    for k, c in enumerate(pick):
        assert np.array_equal(out[k, :each].reshape(45, 61, 3), c[2][:, :, ::-1]), c[0]


def test_threads_1_and_4_agree_and_two_calls_back_to_back(eng, cases):
    a, b = _same_size(cases, 130, 70, 8), _same_size(cases, 61, 45, 8)
    fa, fb = [jpeg.EncodedFrame(c[1]) for c in a], [jpeg.EncodedFrame(c[1]) for c in b]
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):                                           # no synchronisation between the calls: both staging areas in use
        o1 = jpeg.decode(eng, fa, stream=s, threads=1)
        o2 = jpeg.decode(eng, fb, stream=s, threads=4)
        o3 = jpeg.decode(eng, fa, stream=s, threads=4)
    s.synchronize()
    assert torch.equal(o1, o3)
    for k, c in enumerate(a):
        assert np.array_equal(o1[k].cpu().numpy(), c[2][:, :, ::-1]), c[0]
    for k, c in enumerate(b):
        assert np.array_equal(o2[k].cpu().numpy(), c[2][:, :, ::-1]), c[0]


def test_refused_streams_launch_nothing_and_the_context_stays_usable(eng, refused):
    good, good_rgb, bad = refused
    h, w = good_rgb.shape[:2]
    for name, (data, cause) in bad.items():
        if name not in ("cut_scan", "bad_restart"):                       # (those two have sound headers: only the scan shows it)
            with pytest.raises(ValueError, match=cause):
                jpeg.EncodedFrame(data)
        out = torch.full((2, h, w, 3), 0x5A, dtype=torch.uint8, device=DEV)
        ptrs = (C.c_char_p * 2)(good, data)
        sizes = (C.c_size_t * 2)(len(good), len(data))
        rc = eng.L.ss_jpeg_decode_batch(eng.ctx, eng._st(None), ptrs, sizes, 2, h, w, out.data_ptr(), h * w * 3, 0, 2)
        msg = eng.L.ss_last_error(eng.ctx).decode()
        assert rc == lib.SS_ERR_INVALID and "image 1" in msg and cause in msg, (name, rc, msg)
        torch.cuda.synchronize()
        assert bool((out == 0x5A).all()), name
    # a frame of another size than the batch's
    out = torch.full((1, h + 8, w, 3), 0x5A, dtype=torch.uint8, device=DEV)
    rc = eng.L.ss_jpeg_decode_batch(eng.ctx, eng._st(None), (C.c_char_p * 1)(good), (C.c_size_t * 1)(len(good)), 1, h + 8, w, out.data_ptr(), (h + 8) * w * 3, 0, 1)
    assert rc == lib.SS_ERR_INVALID and "differs from the batch's" in eng.L.ss_last_error(eng.ctx).decode()
    assert bool((out == 0x5A).all())
    got = jpeg.decode(eng, [jpeg.EncodedFrame(good)], rgb=True).cpu().numpy()[0]
    assert np.array_equal(got, good_rgb)


def _rows(res):
    b = res[0].boxes
    return (b.xyxy.clone(), None if b.id is None else b.id.clone(), b.conf.clone(), b.cls.clone())


@pytest.mark.parametrize("batch", [4, 5])
def test_track_stream_over_encoded_frames_equals_decoded_arrays(sequence, batch):
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack")
    arrays = [np.ascontiguousarray(rgb[:, :, ::-1]) for _, rgb in sequence]
    frames = [jpeg.EncodedFrame(d) for d, _ in sequence]
    want = [_rows(r) for r in model.track_stream(arrays, batch=batch)]
    model._stream_pipe.reset_tracker(-1)
    model._frame_index = 0
    got = list(model.track_stream(frames, batch=batch, keep_device_frames=True))
    assert len(got) == len(want) == 12
    for k, (r, w) in enumerate(zip(got, want)):
        assert r[0].orig_img is frames[k]
        assert np.array_equal(r[0].orig_img_device.cpu().numpy(), arrays[k]), f"frame {k}"
        g = _rows(r)
        for a, b in zip(g, w):
            assert (a is None and b is None) or torch.equal(a, b), f"frame {k}"
    with pytest.raises(TypeError, match="track_stream"):
        model.track(frames[0])
    with pytest.raises(TypeError):
        list(model.track_stream([frames[0], arrays[1]], batch=batch))
    model.close()
