"""Encoded frames: baseline JPEG decoded on the device (csrc/ss_jpeg.hip) and written from frames on the device (csrc/ss_jpeg_enc.hip); docs/JPEG.md.

    H, W, components, (h, v) = probe(data)          host only
    f = EncodedFrame(data)                          .shape == (H, W, 3); ValueError with the library's message when refused
    for f in split_mjpeg("clip.mjpeg"): ...         a raw concatenated MJPEG file, no container parsing
    for b in split_bytes(buf): ...                  the same cut on bytes, yielding each frame's bytes unprobed
    t = decode(engine, frames)                      uint8 device tensor [n, H, W, 3], BGR (rgb=True: RGB); entropy="device": Huffman
                                                    decoding on the device too (docs/JPEG.md §12)
    raw, segs, hdr = scan_segments(data)            host only: the host's share of that stage (unstuffed scan cut at its restart markers)
    files = encode(engine, frames, quality=85)      frames on the device (or host arrays) -> baseline JPEG files as bytes (csrc/ss_jpeg_enc.hip);
                                                    entropy="device": Huffman coding on the device too (docs/JPEG.md §13)

`YOLO.track_stream` takes EncodedFrames in place of arrays: the group is decoded straight into the buffer the detector reads.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Iterator, Union

from . import lib

MAX_BATCH = 64
SUBSAMPLING = {"4:2:0": (2, 2), "4:2:2": (2, 1), "4:4:4": (1, 1)}       # luma sampling factors (h, v); chroma is 1 x 1


def probe(data):
    """(H, W, components, (h, v)) of a JPEG the decoder accepts; ValueError with the library's message otherwise."""
    data = bytes(data)
    L = lib.load()
    w, h, nc, hs, vs = (C.c_int() for _ in range(5))
    rc = L.ss_jpeg_probe(data, len(data), C.byref(w), C.byref(h), C.byref(nc), C.byref(hs), C.byref(vs))
    if rc != lib.SS_OK:
        msg = L.ss_last_error(None)
        raise ValueError(msg.decode() if msg else "ss_jpeg_probe failed")
    return h.value, w.value, nc.value, (hs.value, vs.value)


class EncodedFrame:
    """One baseline JPEG, still encoded.  `shape` is what the decoded frame will have."""
    __slots__ = ("data", "shape", "components", "sampling")

    def __init__(self, data):
        self.data = bytes(data)
        h, w, self.components, self.sampling = probe(self.data)
        self.shape = (h, w, 3)

    def __len__(self):
        return len(self.data)

    def __repr__(self):
        return f"EncodedFrame({self.shape[1]}x{self.shape[0]}, {len(self.data)} bytes)"


def split_bytes(buf: bytes) -> Iterator[bytes]:
    """The SOI .. EOI runs of a concatenated stream, as bytes (nothing is probed).  Marker segments are skipped by their length (an FFD9 inside APPn / COM data
    ends nothing); inside entropy-coded data FF is followed by 00 or RSTn, so the first other marker there ends the scan."""
    n, p = len(buf), 0
    while True:
        p = buf.find(b"\xff\xd8", p)
        if p < 0:
            return
        start, p = p, p + 2
        while p + 1 < n:
            if buf[p] != 0xFF:
                p += 1                                             # between segments (not expected in a clean stream)
                continue
            m = buf[p + 1]
            if m == 0xFF:
                p += 1
            elif m == 0xD9:
                p += 2
                yield buf[start:p]
                break
            elif m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
                p += 2
            else:
                if p + 3 >= n:
                    return
                p += 2 + ((buf[p + 2] << 8) | buf[p + 3])
                if m == 0xDA:                                      # the scan: to the next marker that is neither stuffing nor a restart
                    while True:
                        p = buf.find(b"\xff", p)
                        if p < 0 or p + 1 >= n:
                            return
                        if buf[p + 1] == 0 or 0xD0 <= buf[p + 1] <= 0xD7 or buf[p + 1] == 0xFF:
                            p += 1 if buf[p + 1] == 0xFF else 2
                            continue
                        break
        else:
            return


def split_mjpeg(src: Union[str, bytes, bytearray, memoryview, "os.PathLike"]) -> Iterator[EncodedFrame]:
    """EncodedFrames of a raw concatenated MJPEG file (a path) or of its bytes."""
    if isinstance(src, (bytes, bytearray, memoryview)):
        buf = bytes(src)
    else:
        with open(src, "rb") as f:
            buf = f.read()
    for seg in split_bytes(buf):
        yield EncodedFrame(seg)


def decode(engine, frames, out=None, rgb: bool = False, stream=None, threads: int = 4, entropy: str = "host"):
    """EncodedFrames (or bytes) of one size -> uint8 device tensor [n, H, W, 3]; asynchronous on `stream` after the host stage.
    entropy: "host" (Huffman decoding on the host threads) or "device" (on the device too, docs/JPEG.md §12)."""
    import torch
    if entropy not in ("host", "device"):
        raise ValueError(f"jpeg.decode: entropy {entropy!r} (\"host\" or \"device\")")
    frames = [f if isinstance(f, EncodedFrame) else EncodedFrame(f) for f in frames]
    if not frames:
        raise ValueError("jpeg.decode: no frames")
    if out is None:
        out = torch.empty((len(frames),) + frames[0].shape, dtype=torch.uint8, device=engine.device)
    for k in range(0, len(frames), MAX_BATCH):
        engine.jpeg_decode_batch(out[k:k + MAX_BATCH], frames[k:k + MAX_BATCH], stream, threads, rgb, entropy)
    return out


def scan_segments(data):
    """The host's share of the device entropy stage for one file (host only): (unstuffed scan bytes, segments [n, 4] uint32 of
    byte offset / byte length / first block / blocks, the 160 header words); ValueError with the library's message when refused."""
    import numpy as np
    data = bytes(data)
    L = lib.load()
    used, nseg = C.c_size_t(), C.c_int()

    def ck(rc):
        if rc != lib.SS_OK:
            msg = L.ss_last_error(None)
            raise ValueError(msg.decode() if msg else "ss_jpeg_scan_segments failed")
    ck(L.ss_jpeg_scan_segments(data, len(data), None, 0, C.byref(used), None, 0, C.byref(nseg), None))
    raw, segs, hdr = np.zeros(used.value, np.uint8), np.zeros((nseg.value, 4), np.uint32), np.zeros(160, np.uint32)
    ck(L.ss_jpeg_scan_segments(data, len(data), raw.ctypes.data, raw.size, C.byref(used), segs.ctypes.data, nseg.value, C.byref(nseg), hdr.ctypes.data))
    return raw[:used.value].tobytes(), segs, hdr


def device_coefficients(engine, data):
    """The device entropy stage alone on one file: (dense int16 blocks in ss_jpeg_coefficients' layout, the rounds each tile took)."""
    import numpy as np
    data = bytes(data)
    h, w, nc, (hs, vs) = probe(data)
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    coef = np.zeros(mx * my * 64 * (1 if nc == 1 else hs * vs + 2), np.int16)
    engine._ck(engine.L.ss_jpeg_device_coefficients(engine.ctx, data, len(data), coef.ctypes.data_as(C.POINTER(C.c_short)), coef.size))
    rounds = (C.c_int * 4096)()
    n = engine.L.ss_jpeg_device_rounds(engine.ctx, rounds, 4096)
    return coef, list(rounds[:min(n, 4096)])


def encode(engine, frames, quality: int = 85, subsampling: str = "4:2:0", stream=None, threads: int = 4, rgb: bool = False, entropy: str = "host"):
    """Any number of frames of one size -> list of baseline JPEG files (bytes), byte for byte what Pillow writes with
    `quality=quality, subsampling=subsampling`.  `frames`: a uint8 tensor [n, H, W, 3] (or a sequence of [H, W, 3] tensors / arrays),
    BGR unless rgb=True; what is not on the engine's device yet is uploaded first.  Encoded in chunks of MAX_BATCH.
    entropy: "host" (Huffman coding on the host threads) or "device" (on the device too, docs/JPEG.md §13); the same bytes."""
    if entropy not in ("host", "device"):
        raise ValueError(f"jpeg.encode: entropy {entropy!r} (\"host\" or \"device\")")
    import numpy as np
    import torch
    if not isinstance(frames, (torch.Tensor, np.ndarray)):
        frames = list(frames)
        if not frames:
            raise ValueError("jpeg.encode: no frames")
        frames = torch.stack(list(frames)) if isinstance(frames[0], torch.Tensor) else np.stack(frames)
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    if frames.shape[0] == 0:
        raise ValueError("jpeg.encode: no frames")
    frames = frames.to(engine.device).contiguous()
    out = []
    for k in range(0, frames.shape[0], MAX_BATCH):
        out += engine.jpeg_encode_batch(frames[k:k + MAX_BATCH], quality, subsampling, stream, threads, rgb, entropy)
    return out


def entropy_encode_device(engine, coef, quality: int, width: int, height: int, subsampling: str = "4:2:0") -> bytes:
    """The device entropy stage alone, for tests: dense natural-order int16 blocks in ss_jpeg_coefficients' layout (component after
    component, each over its whole-MCU grid) -> the whole file.  The device twin of the library's host-only ss_jpeg_entropy_encode;
    coefficients beyond the baseline categories are refused (engine's error) before anything is launched."""
    import numpy as np
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"jpeg.entropy_encode_device: subsampling {subsampling!r} (one of {', '.join(SUBSAMPLING)})")
    hs, vs = SUBSAMPLING[subsampling]
    coef = np.ascontiguousarray(coef, dtype=np.int16).reshape(-1)
    blocks = -(-int(width) // (8 * hs)) * -(-int(height) // (8 * vs)) * (hs * vs + 2)
    if coef.size != blocks * 64:
        raise ValueError(f"jpeg.entropy_encode_device: {coef.size} values, the shape has {blocks} blocks of 64")
    bound = int(engine.L.ss_jpeg_encode_bound(int(width), int(height), hs, vs))
    if bound < 0:
        lib.check(None, bound)
    out, size = np.empty(bound, np.uint8), C.c_size_t()
    engine._ck(engine.L.ss_jpeg_entropy_encode_device(engine.ctx, coef.ctypes.data_as(C.POINTER(C.c_short)), int(quality), int(width), int(height), hs, vs,
                                                      out.ctypes.data, bound, C.byref(size)))
    return out[:size.value].tobytes()
