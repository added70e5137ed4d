"""The JPEG entropy stage on the device (csrc/ss_jpeg.hip k_jpeg_huff / k_jpeg_dc, docs/JPEG.md §12): the pixels equal Pillow's stored
arrays byte for byte, the coefficients equal the host decoder's, the rounds equal the NumPy restatement's (tests/jpeg_huff_ref.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from strongsort_yolo_amd import fused, jpeg, lib
from tests import jpeg_huff_ref as ref
from tests.gpu_util import engine

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"


def _cases(name):
    z = np.load(os.path.join(GOLD, name))
    return [(str(n), z[f"bytes_{i}"].tobytes(), z[f"rgb_{i}"]) for i, n in enumerate(z["names"])]


@pytest.fixture(scope="module")
def cases():
    return _cases("jpeg_cases.npz")


@pytest.fixture(scope="module")
def entropy_cases():
    return _cases("jpeg_entropy_cases.npz")


@pytest.fixture(scope="module")
def sequence():
    z = np.load(os.path.join(GOLD, "jpeg_sequence.npz"))
    return [(z[f"bytes_{i}"].tobytes(), z[f"rgb_{i}"]) for i in range(12)]


@pytest.fixture(scope="module")
def refused():
    z = np.load(os.path.join(GOLD, "jpeg_refused.npz"))
    return z["good"].tobytes(), z["good_rgb"], z["cut_scan"].tobytes()


@pytest.fixture(scope="module")
def eng():
    e = engine(debug=False)
    yield e
    e.close()


@pytest.fixture
def words():
    """Sets the dwords of scan per lane; 32, the default, afterwards."""
    yield lambda w: fused.set_option("jpeg_subseq_words", w)
    fused.set_option("jpeg_subseq_words", 32)


def _same_size(cases, w, h, n):
    pick = [c for c in cases if c[2].shape[:2] == (h, w)]
    assert len(pick) >= n
    return pick[:n]


def _host_coefficients(data, size):
    coef, quant = np.zeros(size, np.int16), np.zeros((4, 64), np.uint16)
    rc = lib.load().ss_jpeg_coefficients(data, len(data), coef.ctypes.data_as(C.POINTER(C.c_short)), size, quant.ctypes.data_as(C.POINTER(C.c_ushort)))
    assert rc == lib.SS_OK
    return coef


@pytest.mark.parametrize("W", [4, 32])
def test_every_case_alone_bgr_and_rgb(eng, cases, entropy_cases, words, W):
    words(W)
    bad = []
    for name, data, rgb in cases + entropy_cases:
        f = jpeg.EncodedFrame(data)
        got_bgr = jpeg.decode(eng, [f], entropy="device").cpu().numpy()[0]
        got_rgb = jpeg.decode(eng, [f], rgb=True, entropy="device").cpu().numpy()[0]
        if not (np.array_equal(got_rgb, rgb) and np.array_equal(got_bgr, rgb[:, :, ::-1])):
            bad.append((name, int((got_rgb != rgb).sum()), int((got_bgr != rgb[:, :, ::-1]).sum())))
    eng.check_errors()
    assert not bad, f"{len(bad)} of {len(cases) + len(entropy_cases)} cases differ at W = {W}: {bad[:8]}"
    # 130 x 70 noise at quality 100 and W = 4 is more than one tile: the carry from tile to tile is in the matrix
    big = max(len(ref.cut(c[1])[0]) for c in cases if c[0].startswith("130x70_noise"))
    assert big > 16 * ref.LANES


@pytest.mark.parametrize("W", [4, 32])
def test_coefficients_and_rounds_equal_the_host_decoder_and_the_restatement(eng, cases, entropy_cases, words, W):
    words(W)
    one_per_sampling = [next(c for c in cases if c[0].startswith("61x45_photo_" + s)) for s in ("444", "422", "420", "grey")]
    for name, data, _ in entropy_cases + one_per_sampling:
        coef, rounds = jpeg.device_coefficients(eng, data)
        assert np.array_equal(coef, _host_coefficients(data, coef.size)), (name, W)
        if name in {c[0] for c in entropy_cases}:
            want = ref.stream(data, W)[3]
            assert rounds == want, (name, W, rounds, want)
            lanes = sum(max(1, -(-s[1] // (4 * W))) for s in ref.cut(data)[1])
            print(f"{name} W={W}: rounds per tile {rounds} of {lanes} lanes")
            assert all(1 <= r <= min(ref.LANES, lanes - t * ref.LANES) for t, r in enumerate(rounds))    # the counted loop's bound


@pytest.mark.parametrize("n,w,h", [(5, 17, 9), (32, 33, 31), (64, 3, 5)])
def test_batches_of_same_size_cases(eng, cases, n, w, h):
    pick = [c for c in cases if c[2].shape[:2] == (h, w)]
    pick = (pick * -(-n // len(pick)))[:n]                               # (48 cases a size: the call's 64 images repeat some)
    assert len(pick) == n and len({c[0].split("_")[2] for c in pick}) > 1 and len({len(c[1]) for c in pick}) > 1     # several samplings and scan lengths in one call
    got = jpeg.decode(eng, [jpeg.EncodedFrame(c[1]) for c in pick], rgb=True, entropy="device").cpu().numpy()
    eng.check_errors()
    for k, c in enumerate(pick):
        assert np.array_equal(got[k], c[2]), c[0]


def test_back_to_back_calls_and_a_host_stage_call_between(eng, cases):
    a, b = _same_size(cases, 130, 70, 8), _same_size(cases, 61, 45, 8)
    fa, fb = [jpeg.EncodedFrame(c[1]) for c in a], [jpeg.EncodedFrame(c[1]) for c in b]
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):                                           # no synchronisation between the calls: both staging slots in use
        o1 = jpeg.decode(eng, fa, stream=s, threads=1, entropy="device")
        o2 = jpeg.decode(eng, fb, stream=s, threads=4, entropy="device")
        o3 = jpeg.decode(eng, fa, stream=s, threads=4, entropy="host")
        o4 = jpeg.decode(eng, fb, stream=s, threads=2, entropy="device")
    s.synchronize()
    eng.check_errors()
    assert torch.equal(o1, o3) and torch.equal(o2, o4)
    for k, c in enumerate(a):
        assert np.array_equal(o1[k].cpu().numpy(), c[2][:, :, ::-1]), c[0]
    for k, c in enumerate(b):
        assert np.array_equal(o2[k].cpu().numpy(), c[2][:, :, ::-1]), c[0]


@pytest.mark.parametrize("extra", [64, 5])
def test_out_frame_stride_leaves_the_gap_untouched(eng, cases, extra):
    pick = _same_size(cases, 61, 45, 4)
    each = 45 * 61 * 3
    buf = torch.full((4, each + extra), 0xA5, dtype=torch.uint8, device=DEV)
    dst = buf[:, :each].view(4, 45, 61, 3)
    eng.jpeg_decode_batch(dst, [jpeg.EncodedFrame(c[1]) for c in pick], entropy="device")
    out = buf.cpu().numpy()
    eng.check_errors()
    assert (out[:, each:] == 0xA5).all()
    for k, c in enumerate(pick):
        assert np.array_equal(out[k, :each].reshape(45, 61, 3), c[2][:, :, ::-1]), c[0]


def test_a_scan_that_ends_early_is_reported_and_the_context_stays_usable(eng, refused):
    good, good_rgb, cut_scan = refused
    frames = [jpeg.EncodedFrame(good), jpeg.EncodedFrame(cut_scan), jpeg.EncodedFrame(good)]
    out = jpeg.decode(eng, frames, rgb=True, entropy="device")           # the headers are sound: nothing is refused here
    with pytest.raises(lib.SSError, match="image 1: data ends before the last MCU") as e:
        eng.check_errors()
    assert e.value.code == lib.SS_ERR_INVALID
    got = out.cpu().numpy()
    assert np.array_equal(got[0], good_rgb) and np.array_equal(got[2], good_rgb)
    assert (got[1] == got[1][0, 0]).all()                                # every block empty: one flat colour
    eng.check_errors()                                                   # reported once
    again = jpeg.decode(eng, frames[::2], rgb=True, entropy="device").cpu().numpy()
    eng.check_errors()
    assert np.array_equal(again[0], good_rgb) and np.array_equal(again[1], good_rgb)
    # without check_errors the next call that reuses the staging slot reports it (two slots: the second call after)
    jpeg.decode(eng, frames, entropy="device")
    jpeg.decode(eng, frames[:1], entropy="device")
    with pytest.raises(lib.SSError, match="image 1: data ends before the last MCU"):
        jpeg.decode(eng, frames[:1], entropy="device")
    eng.check_errors()
    assert np.array_equal(jpeg.decode(eng, frames[:1], rgb=True, entropy="device").cpu().numpy()[0], good_rgb)
    eng.check_errors()


def _rows(res):
    b = res[0].boxes
    return (b.xyxy.clone(), None if b.id is None else b.id.clone(), b.conf.clone(), b.cls.clone())


@pytest.mark.parametrize("batch", [4, 5])
def test_track_stream_with_device_entropy_equals_decoded_arrays(sequence, batch):
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack")
    arrays = [np.ascontiguousarray(rgb[:, :, ::-1]) for _, rgb in sequence]
    frames = [jpeg.EncodedFrame(d) for d, _ in sequence]
    want = [_rows(r) for r in model.track_stream(arrays, batch=batch)]
    model._stream_pipe.reset_tracker(-1)
    model._frame_index = 0
    got = list(model.track_stream(frames, batch=batch, keep_device_frames=True, jpeg_entropy="device"))
    assert len(got) == len(want) == 12
    for k, (r, w) in enumerate(zip(got, want)):
        assert np.array_equal(r[0].orig_img_device.cpu().numpy(), arrays[k]), f"frame {k}"
        for a, b in zip(_rows(r), w):
            assert (a is None and b is None) or torch.equal(a, b), f"frame {k}"
    model._stream_pipe.eng.check_errors()
    model.close()
