"""Frames on the device written as baseline JPEG (csrc/ss_jpeg_enc.hip): byte equality with Pillow's files stored in tests/golden/
(the fixtures' generator is tests/golden/make_jpeg_encode_golden.py; nothing here needs Pillow)."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from strongsort_yolo_amd import cli, jpeg, lib
from tests import jpeg_enc_ref as ref
from tests.gpu_util import engine

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def cases():
    return ref.load_cases()


@pytest.fixture(scope="module")
def eng():
    e = engine(debug=False)
    yield e
    e.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_every_case_alone_bgr_and_rgb(eng, cases):
    bad = []
    for name, bgr, q, s, data, _ in cases:
        (got_bgr,) = jpeg.encode(eng, _dev(bgr), q, s)
        (got_rgb,) = jpeg.encode(eng, _dev(bgr[:, :, ::-1]), q, s, rgb=True)
        if got_bgr != data or got_rgb != data:
            bad.append((name, len(data), len(got_bgr), len(got_rgb)))
    assert not bad, f"{len(bad)} of {len(cases)} cases differ: {bad[:8]}"


def _batch(cases, w, h, s, q, n):
    """n cases of one size, sampling and quality, their contents mixed (the distinct ones in turn)."""
    pick = [c for c in cases if c[1].shape[:2] == (h, w) and c[3] == s and c[2] == q]
    assert len({c[0] for c in pick}) >= 5 and len({c[0].split("_")[1] for c in pick}) >= 4
    return [pick[(3 * k) % len(pick)] for k in range(n)]


@pytest.mark.parametrize("n,w,h,s", [(1, 33, 31, "4:2:0"), (5, 61, 45, "4:2:2"), (32, 130, 70, "4:2:0"), (32, 33, 31, "4:4:4"), (5, 130, 70, "4:4:4")])
def test_batches_of_same_size_cases(eng, cases, n, w, h, s):
    pick = _batch(cases, w, h, s, 85, n)
    got = jpeg.encode(eng, np.stack([c[1] for c in pick]), 85, s)
    assert len(got) == n
    for k, c in enumerate(pick):
        assert got[k] == c[4], (k, c[0])


def test_more_frames_than_one_call_takes(eng, cases):
    pick = _batch(cases, 33, 31, "4:2:0", 85, jpeg.MAX_BATCH + 3)
    got = jpeg.encode(eng, [_dev(c[1]) for c in pick], 85, "4:2:0")
    assert [g == c[4] for g, c in zip(got, pick)] == [True] * (jpeg.MAX_BATCH + 3)


def test_threads_1_and_4_agree_and_two_calls_back_to_back(eng, cases):
    a, b = _batch(cases, 130, 70, "4:2:0", 85, 8), _batch(cases, 61, 45, "4:4:4", 85, 8)
    xa, xb = _dev(np.stack([c[1] for c in a])), _dev(np.stack([c[1] for c in b]))
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                           # no synchronisation between the calls: both slots in use
        o1 = jpeg.encode(eng, xa, 85, "4:2:0", stream=s, threads=1)
        o2 = jpeg.encode(eng, xb, 85, "4:4:4", stream=s, threads=4)
        o3 = jpeg.encode(eng, xa, 85, "4:2:0", stream=s, threads=4)
    assert o1 == o3 == [c[4] for c in a]
    assert o2 == [c[4] for c in b]


@pytest.mark.parametrize("extra", [64, 5])                                # 5: frames at unaligned bases
def test_in_frame_stride_with_a_gap(eng, cases, extra):
    pick = _batch(cases, 61, 45, "4:2:0", 85, 4)
    each = 45 * 61 * 3
    buf = torch.full((4, each + extra), 0xA5, dtype=torch.uint8, device=DEV)
    src = buf[:, :each].view(4, 45, 61, 3)
    src.copy_(_dev(np.stack([c[1] for c in pick])))
    assert src.stride(0) == each + extra
    assert eng.jpeg_encode_batch(src, 85, "4:2:0") == [c[4] for c in pick]
    assert bool((buf[:, each:] == 0xA5).all())


def test_refusals_launch_nothing_and_the_context_stays_usable(eng, cases):
    name, bgr, q, s, data, _ = next(c for c in cases if c[0].startswith("61x45_synth_420"))
    x = _dev(np.stack([bgr, bgr]))
    h, w = bgr.shape[:2]
    bound = eng.L.ss_jpeg_encode_bound(w, h, 2, 2)
    files = np.full((2, bound), 0x5A, np.uint8)
    good = dict(ctx=eng.ctx, stream=eng._st(None), d_in=C.c_void_p(x.data_ptr()), stride=x.stride(0), n=2, height=h, width=w, rgb=0, quality=q, hs=2, vs=2,
                threads=2, out=(C.c_void_p * 2)(files[0].ctypes.data, files[1].ctypes.data), cap=(C.c_size_t * 2)(bound, bound), size=(C.c_size_t * 2)(7, 7))

    def refused(cause, **kw):
        args = dict(good, **kw)
        torch.cuda.synchronize()
        rc = eng.L.ss_jpeg_encode_batch(*args.values())
        msg = eng.L.ss_last_error(eng.ctx).decode()
        assert rc == lib.SS_ERR_INVALID and cause in msg, (kw, rc, msg)
        assert (files == 0x5A).all() and list(good["size"]) == [7, 7], kw       # nothing was written
    for n in (0, 65, -1):
        refused("n <= 64", n=n)
    for side in (0, 8193):
        refused("sides", height=side)
        refused("sides", width=side)
    for quality in (0, 101):
        refused("quality", quality=quality)
    for hs, vs in ((1, 2), (4, 1), (2, 4), (0, 1)):
        refused("sampling", hs=hs, vs=vs)
    for t in (0, 17):
        refused("threads", threads=t)
    refused("null", d_in=None)
    refused("null", out=None)
    refused("null", cap=None)
    refused("null", size=None)
    refused("image 1: null buffer", out=(C.c_void_p * 2)(files[0].ctypes.data, None))
    refused("image 1: out_cap", cap=(C.c_size_t * 2)(bound, bound - 1))
    refused("in_frame_stride", stride=h * w * 3 - 1)
    assert eng.L.ss_jpeg_encode_batch(*good.values()) == lib.SS_OK
    for i in range(2):
        assert files[i, :good["size"][i]].tobytes() == data


def test_round_trip_equals_pillows_decode_of_pillows_bytes(eng, cases):
    done = 0
    for name, bgr, q, s, data, rgb in cases:
        if rgb is None:
            continue
        back = jpeg.decode(eng, jpeg.encode(eng, _dev(bgr), q, s), rgb=True).cpu().numpy()[0]
        assert np.array_equal(back, rgb), name
        done += 1
    assert done >= 4


@pytest.mark.parametrize("batch", [4, 5])                                 # 12 frames: 5 leaves a partial last group
def test_cli_saves_the_same_frames_as_mjpeg(eng, tmp_path, monkeypatch, batch):
    """process_video with --save x.npy, then with --save x.mjpeg --device-encode: the MJPEG's frames are jpeg.encode of the stack's
    frames, the labels files are identical."""
    from strongsort_yolo_amd.yolo import YOLO
    z = np.load(os.path.join(GOLD, "jpeg_sequence.npz"))
    src = tmp_path / "seq.npy"
    np.save(src, np.stack([np.ascontiguousarray(z[f"rgb_{i}"][:, :, ::-1]) for i in range(12)]))
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack")
    labels = []
    for run, extra in (("a", {"save": str(tmp_path / "x.npy")}), ("b", {"save": str(tmp_path / "x.mjpeg"), "device_encode": True})):
        clock = iter(range(10 ** 6))
        monkeypatch.setattr(cli, "time", types.SimpleNamespace(time=lambda: 0.25 * next(clock)))      # the FPS text of both runs is the same
        out = cli.process_video({"source": str(src), "track": True, "count": True, "tracker": "bytetrack", "batch": batch, "outdir": str(tmp_path / run),
                                 **extra}, model=model)
        assert out["frames"] == 12
        labels.append((tmp_path / run / "seq_labels.txt").read_bytes())
        model._stream_pipe.reset_tracker(-1)
        model._frame_index = 0
    assert labels[0] == labels[1] and labels[0]
    stack = np.load(tmp_path / "x.npy")
    frames = list(jpeg.split_mjpeg(str(tmp_path / "x.mjpeg")))
    assert len(frames) == len(stack) == 12 and all(f.shape == stack[0].shape for f in frames)
    want = jpeg.encode(eng, stack)
    assert [f.data == w for f, w in zip(frames, want)] == [True] * 12
    assert not np.array_equal(stack, np.stack([np.ascontiguousarray(z[f"rgb_{i}"][:, :, ::-1]) for i in range(12)]))      # something was drawn
    model.close()
