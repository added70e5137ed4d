"""The encoder's entropy stage on the device (docs/JPEG.md §13, jpeg.encode(..., entropy="device")): byte equality with Pillow's stored files
and, for generated inputs, with the host path (itself held to Pillow by tests/test_jpeg_encode_cpu.py)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from strongsort_yolo_amd import cli, jpeg, lib
from tests import jpeg_enc_huff_ref as href
from tests import jpeg_enc_ref as ref
from tests.gpu_util import engine

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
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


def _first_difference(a, b):
    n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return f"lengths {len(a)} / {len(b)}, first difference at byte {n}: {a[n:n + 8].hex()} / {b[n:n + 8].hex()}"


def test_every_case_alone_bgr_and_rgb(eng, cases):
    bad = []
    for name, bgr, q, s, data, _ in cases:
        (got_bgr,) = jpeg.encode(eng, _dev(bgr), q, s, entropy="device")
        (got_rgb,) = jpeg.encode(eng, _dev(bgr[:, :, ::-1]), q, s, rgb=True, entropy="device")
        if got_bgr != data or got_rgb != data:
            bad.append((name, _first_difference(got_bgr, data), _first_difference(got_rgb, data)))
    assert len(cases) == 180
    assert not bad, f"{len(bad)} of {len(cases)} cases differ: {bad[:6]}"


def _batch(cases, w, h, s, q, n):
    pick = [c for c in cases if c[1].shape[:2] == (h, w) and c[3] == s and c[2] == q]
    assert len({c[0] for c in pick}) >= 5 and len({c[0].split("_")[1] for c in pick}) >= 4
    return [pick[(3 * k) % len(pick)] for k in range(n)]


@pytest.mark.parametrize("n,w,h,s", [(1, 33, 31, "4:2:0"), (5, 61, 45, "4:2:2"), (32, 130, 70, "4:2:0"), (32, 33, 31, "4:4:4")])
def test_batches_of_same_size_cases(eng, cases, n, w, h, s):
    """Images of different lengths side by side in one launch of every kernel."""
    pick = _batch(cases, w, h, s, 85, n)
    got = jpeg.encode(eng, np.stack([c[1] for c in pick]), 85, s, entropy="device")
    assert len(got) == n
    for k, c in enumerate(pick):
        assert got[k] == c[4], (k, c[0], _first_difference(got[k], c[4]))


def test_more_frames_than_one_call_takes(eng, cases):
    pick = _batch(cases, 33, 31, "4:2:0", 85, jpeg.MAX_BATCH + 3)
    got = jpeg.encode(eng, [_dev(c[1]) for c in pick], 85, "4:2:0", entropy="device")
    assert [g == c[4] for g, c in zip(got, pick)] == [True] * (jpeg.MAX_BATCH + 3)


def _host_writer(eng, flat):
    cap = eng.L.ss_jpeg_encode_bound(href.CRAFT_W, href.CRAFT_H, 1, 1)
    out, size = (C.c_ubyte * cap)(), C.c_size_t()
    rc = eng.L.ss_jpeg_entropy_encode(flat.ctypes.data_as(C.POINTER(C.c_short)), href.CRAFT_Q, href.CRAFT_W, href.CRAFT_H, 1, 1, out, cap, C.byref(size))
    assert rc == lib.SS_OK, eng.L.ss_last_error(None)
    return bytes(out[:size.value])


@pytest.mark.parametrize("name", href.CRAFTED)
def test_crafted_coefficients_through_the_entropy_stage_alone(eng, name):
    """(b) maximum-length blocks and category-11 DC differences, (c) three ZRL and no EOB, (d) every AC -1023, (e) all zero, (f) sparse random
    blocks with categories 0 .. 10: ss_jpeg_entropy_encode_device == ss_jpeg_entropy_encode on the same array."""
    flat = href.library_layout(href.crafted(name), href.CRAFT_W, href.CRAFT_H, 1, 1)
    want = _host_writer(eng, flat)
    got = jpeg.entropy_encode_device(eng, flat, href.CRAFT_Q, href.CRAFT_W, href.CRAFT_H, href.CRAFT_S)
    assert got == want, _first_difference(got, want)
    if name == "b_max":
        assert len(want) - 625 == 6866 and b"\xff\x00\xff\x00" in want


def test_a_category_beyond_baseline_is_refused_on_the_host(eng):
    flat = href.library_layout(href.crafted("f_seed1"), href.CRAFT_W, href.CRAFT_H, 1, 1)
    want = _host_writer(eng, flat)
    bad = flat.copy()
    bad[5 * 64 + 17] = 1024                                              # category 11 in an AC slot
    cap = eng.L.ss_jpeg_encode_bound(href.CRAFT_W, href.CRAFT_H, 1, 1)
    out, size = np.full(cap, 0x5A, np.uint8), C.c_size_t(7)
    torch.cuda.synchronize()
    rc = eng.L.ss_jpeg_entropy_encode_device(eng.ctx, bad.ctypes.data_as(C.POINTER(C.c_short)), href.CRAFT_Q, href.CRAFT_W, href.CRAFT_H, 1, 1, out.ctypes.data, cap,
                                             C.byref(size))
    msg = eng.L.ss_last_error(eng.ctx).decode()
    assert rc == lib.SS_ERR_INVALID and "a coefficient beyond the baseline categories (DC difference 11 bits, AC 10 bits)" in msg, (rc, msg)
    assert (out == 0x5A).all() and size.value == 7                      # nothing was written
    hrc = eng.L.ss_jpeg_entropy_encode(bad.ctypes.data_as(C.POINTER(C.c_short)), href.CRAFT_Q, href.CRAFT_W, href.CRAFT_H, 1, 1, out.ctypes.data, cap, C.byref(size))
    assert hrc == lib.SS_ERR_INVALID and eng.L.ss_last_error(None).decode().split(": ", 1)[1] == msg.split(": ", 1)[1]      # the host writer's message
    with pytest.raises(lib.SSError, match="categories"):
        jpeg.entropy_encode_device(eng, bad, href.CRAFT_Q, href.CRAFT_W, href.CRAFT_H, href.CRAFT_S)
    assert jpeg.entropy_encode_device(eng, flat, href.CRAFT_Q, href.CRAFT_W, href.CRAFT_H, href.CRAFT_S) == want      # the context stays usable


@pytest.mark.parametrize("seed,s", [(11, "4:4:4"), (12, "4:2:0")])
def test_consecutive_stuffed_bytes_from_pixels(eng, seed, s):
    rgb = np.random.default_rng(seed).integers(0, 256, (31, 33, 3), dtype=np.uint8)
    (want,) = jpeg.encode(eng, _dev(rgb), 100, s, rgb=True, entropy="host")
    assert b"\xff\x00\xff\x00" in want[623:-2]
    (got,) = jpeg.encode(eng, _dev(rgb), 100, s, rgb=True, entropy="device")
    assert got == want, _first_difference(got, want)


def _constant(name):
    with open(os.path.join(HERE, "..", "strongsort_yolo_amd", "csrc", "ss_jpeg_enc.hip")) as f:
        return int(re.search(rf"^#define {name} (\d+)", f.read(), re.M).group(1))


@pytest.mark.parametrize("quality", [100, 85])
def test_more_than_one_workgroup_at_every_scan_level(eng, quality):
    """640 x 360 at 4:4:4 is 80 x 45 x 3 = 10 800 scan positions.  k_jpegenc_hwrite scans them in ceil(10 800 / JENC_HW_TILE) = 6 chunks of
    1 800, two steps of JENC_HW_THREADS each.  k_jpegenc_ffcount / k_jpegenc_stuff take ceil(bytes / JENC_STUFF_TILE) chunks (64 at the
    most): a flat frame is 14 bits per MCU, 3 600 x 14 / 8 = 6 300 bytes = 4 chunks; the noise frame is far longer (more than JENC_STUFF_TILE x
    JENC_STUFF_CHUNKS bytes: 64 chunks of several steps each).  Both frames in ONE call: the short image's workgroups beyond its end have nothing to do."""
    hw_tile, hw_chunks, st_tile, st_chunks = (_constant(n) for n in ("JENC_HW_TILE", "JENC_HW_CHUNKS", "JENC_STUFF_TILE", "JENC_STUFF_CHUNKS"))
    h, w, nscan = 360, 640, 80 * 45 * 3
    assert 3 <= -(-nscan // hw_tile) <= hw_chunks
    frames = np.stack([np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8), np.full((h, w, 3), 77, np.uint8)])
    x = _dev(frames)
    want = jpeg.encode(eng, x, quality, "4:4:4", entropy="host")
    assert 3 <= -(-(len(want[1]) - 625) // st_tile) <= st_chunks and len(want[0]) - 625 > st_tile * st_chunks
    got = jpeg.encode(eng, x, quality, "4:4:4", entropy="device")
    for k in range(2):
        assert got[k] == want[k], (k, _first_difference(got[k], want[k]))
    for k in range(2):                                                   # and each alone: other chunk sizes
        (one,) = jpeg.encode(eng, x[k], quality, "4:4:4", entropy="device")
        assert one == want[k], (k, _first_difference(one, want[k]))


def test_slot_reuse_and_threads(eng):
    """A long group, a second group, then a short one that lands in the first group's slot: a stream that was not zeroed again would keep
    the long images' bits."""
    rng = np.random.default_rng(21)
    long_ = _dev(rng.integers(0, 256, (8, 70, 130, 3), dtype=np.uint8))
    other = _dev(np.clip(np.add.outer(np.arange(45) * 3, np.arange(61) * 2)[None, :, :, None] + rng.integers(-4, 5, (8, 45, 61, 3)), 0, 255).astype(np.uint8))
    short = _dev(np.stack([np.full((70, 130, 3), 16 * k, np.uint8) for k in range(8)]))
    want = [jpeg.encode(eng, long_, 100, "4:2:0"), jpeg.encode(eng, other, 85, "4:4:4"), jpeg.encode(eng, short, 100, "4:2:0")]
    assert min(len(f) for f in want[0]) > 4 * max(len(f) for f in want[2])
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    for threads in (1, 4):
        with torch.cuda.stream(s):                                       # no synchronisation between the calls
            o1 = jpeg.encode(eng, long_, 100, "4:2:0", stream=s, threads=threads, entropy="device")
            o2 = jpeg.encode(eng, other, 85, "4:4:4", stream=s, threads=threads, entropy="device")
            o3 = jpeg.encode(eng, short, 100, "4:2:0", stream=s, threads=threads, entropy="device")
        assert [o1, o2, o3] == want, threads


@pytest.mark.parametrize("extra", [64, 5])                                # 5: frames at unaligned bases
def test_in_frame_stride_with_a_gap(eng, cases, extra):
    pick = _batch(cases, 61, 45, "4:2:0", 85, 4)
    each = 45 * 61 * 3
    buf = torch.full((4, each + extra), 0xA5, dtype=torch.uint8, device=DEV)
    src = buf[:, :each].view(4, 45, 61, 3)
    src.copy_(_dev(np.stack([c[1] for c in pick])))
    assert src.stride(0) == each + extra
    assert eng.jpeg_encode_batch(src, 85, "4:2:0", entropy="device") == [c[4] for c in pick]
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
        rc = eng.L.ss_jpeg_encode_batch_device(*args.values())
        msg = eng.L.ss_last_error(eng.ctx).decode()
        assert rc == lib.SS_ERR_INVALID and cause in msg and msg.startswith("ss_jpeg_encode_batch_device: "), (kw, rc, msg)
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
    assert eng.L.ss_jpeg_encode_batch_device(*good.values()) == lib.SS_OK
    for i in range(2):
        assert files[i, :good["size"][i]].tobytes() == data


def test_round_trip_through_both_device_entropy_stages(eng, cases):
    done = 0
    for name, bgr, q, s, data, rgb in cases:
        if rgb is None:
            continue
        back = jpeg.decode(eng, jpeg.encode(eng, _dev(bgr), q, s, entropy="device"), rgb=True, entropy="device").cpu().numpy()[0]
        eng.check_errors()
        assert np.array_equal(back, rgb), name
        done += 1
    assert done >= 4


@pytest.mark.parametrize("batch", [4, 5])                                 # 12 frames: 5 leaves a partial last group
def test_cli_writes_the_same_mjpeg_with_the_new_flag(eng, tmp_path, monkeypatch, batch):
    from strongsort_yolo_amd.yolo import YOLO
    z = np.load(os.path.join(GOLD, "jpeg_sequence.npz"))
    src = tmp_path / "seq.npy"
    np.save(src, np.stack([np.ascontiguousarray(z[f"rgb_{i}"][:, :, ::-1]) for i in range(12)]))
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack")
    labels, files = [], []
    for run, extra in (("a", {}), ("b", {"device_encode_entropy": True})):
        clock = iter(range(10 ** 6))
        monkeypatch.setattr(cli, "time", types.SimpleNamespace(time=lambda: 0.25 * next(clock)))      # the FPS text of both runs is the same
        out = cli.process_video({"source": str(src), "track": True, "count": True, "tracker": "bytetrack", "batch": batch, "outdir": str(tmp_path / run),
                                 "save": str(tmp_path / f"{run}.mjpeg"), "device_encode": True, **extra}, model=model)
        assert out["frames"] == 12
        labels.append((tmp_path / run / "seq_labels.txt").read_bytes())
        files.append((tmp_path / f"{run}.mjpeg").read_bytes())
        model._stream_pipe.reset_tracker(-1)
        model._frame_index = 0
    assert labels[0] == labels[1] and labels[0]
    assert files[0] == files[1] and len(list(jpeg.split_bytes(files[1]))) == 12
    model.close()
