"""Timing of the JPEG sink (docs/JPEG.md "Encoding", "Measured").  One JSON line per run on stdout.

The frames: the 32 rendered synthetic 1280x720 frames of tools/jpeg_time.py (its decoded arrays), on the device; 4:2:0, quality 85.

  --mode host     wall time of engine.jpeg_encode_batch on groups of 32: the host entropy stage at threads 1, 4 and 16 (the call returns
                  when the files are written: two launches, the copy of the sparse coefficients, Huffman coding) and the device entropy
                  stage (entropy="device", docs/JPEG.md §13) at threads 1 and 4, the five legs interleaved group by group in one
                  process; the same two calls on 32 flat frames (next to no entropy coding: launches, waits, copies and the wrapper);
                  the bytes that cross PCIe per frame for both stages, and — when Pillow is importable — whether the files equal Pillow's
  --mode kernel   both calls in a loop and nothing else; for the kernels' own times (k_jpegenc_fdct, k_jpegenc_pack and the entropy
                  stage's k_jpegenc_hlen, k_jpegenc_hwrite, k_jpegenc_ffcount, k_jpegenc_stuff) run it under
                  `rocprofv3 --kernel-trace --stats -- python tools/jpeg_encode_time.py --mode kernel` (no counters in that run)
  --mode rates    cli.process_video frames/s (bytetrack, yolov8n with seeded random-init weights, batch 32) with four sinks in ONE
                  process, the legs interleaved over --rounds: (a) --save x.bgr (the raw download), (b) --save x.mjpeg --device-encode,
                  (c) the raw download followed by Pillow's encoder on the host at the same quality (needs Pillow), (d) --save x.mjpeg
                  --device-encode --device-encode-entropy
"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from jpeg_time import G, _spread, make_frames  # noqa: E402

Q, SUB = 85, "4:2:0"


def _pillow(bgr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, "JPEG", quality=Q, subsampling=SUB)
    return buf.getvalue()


def _stream_bytes(L, data, blocks):
    """What the call downloaded for this file: 4 bytes per block table word, 4 per non-zero coefficient, 4 for the total."""
    coef, quant = np.zeros(blocks * 64, np.int16), (C.c_ushort * 256)()
    assert L.ss_jpeg_coefficients(data, len(data), coef.ctypes.data_as(C.POINTER(C.c_short)), coef.size, quant) == 0
    real = coef.reshape(-1, 64)
    return 4 * (blocks + 1) + 4 * int(np.count_nonzero(real)) + 4, int(np.count_nonzero(real))


def host(groups, warmup):
    from strongsort_yolo_amd.engine import TrackerEngine
    _, dec = make_frames()
    eng = TrackerEngine(n_streams=1)
    x = torch.from_numpy(np.stack(dec)).to(eng.device)
    flat = torch.full_like(x, 90)
    res = {"mode": "host", "frame": f"1280x720 {SUB} q{Q}", "group_frames": G, "raw_frame_bytes": 3 * 720 * 1280}
    files = None

    def timed(src, legs):
        """legs: (entropy, threads); interleaved group by group -> {leg: [ms]}, {leg: the last files}."""
        ms, out = {leg: [] for leg in legs}, {}
        for g in range(groups + warmup):
            for leg in (legs if g % 2 == 0 else legs[::-1]):
                torch.cuda.synchronize()
                t = time.perf_counter()
                out[leg] = eng.jpeg_encode_batch(src, Q, SUB, threads=leg[1], entropy=leg[0])
                dt = time.perf_counter() - t
                if g >= warmup:
                    ms[leg].append(dt * 1e3)
        return ms, out
    legs = [("host", 1), ("host", 4), ("host", 16), ("device", 1), ("device", 4)]
    ms, out = timed(x, legs)
    files = out[("host", 16)]
    for leg in legs:
        name = f"threads_{leg[1]}" if leg[0] == "host" else f"device_entropy_threads_{leg[1]}"      # (the host legs keep their earlier names)
        res[f"{name}_ms_per_group"] = _spread(ms[leg])
        res[f"{name}_frames_per_s_median"] = G / (float(np.median(ms[leg])) * 1e-3)
    res["device_entropy_equal_to_host"] = bool(all(out[leg] == files for leg in legs))
    ms, _ = timed(flat, [("host", 16), ("device", 4)])
    res["flat_frames_ms_per_group"] = _spread(ms[("host", 16)])   # launches, waits, copies and the Python wrapper; next to no entropy coding
    res["device_entropy_flat_frames_ms_per_group"] = _spread(ms[("device", 4)])
    blocks = 80 * 45 * 6
    sb = [_stream_bytes(eng.L, f, blocks) for f in files]
    res["file_bytes_per_frame_mean"] = float(np.mean([len(f) for f in files]))
    res["downloaded_bytes_per_frame_mean"] = float(np.mean([b for b, _ in sb]))
    # the device entropy stage copies the stuffed scan (the file without its 625 bytes of header and EOI, rounded up to 16) and 12 bytes of totals
    res["device_entropy_downloaded_bytes_per_frame_mean"] = float(np.mean([(len(f) - 625 + 15) // 16 * 16 + 12 for f in files]))
    res["nonzero_coefficients_per_frame_mean"] = float(np.mean([n for _, n in sb]))
    try:
        res["equal_to_pillow"] = bool(all(_pillow(dec[k]) == files[k] for k in range(G)))
    except ImportError:
        res["equal_to_pillow"] = None
    eng.close()
    return res


def kernel(groups):
    from strongsort_yolo_amd.engine import TrackerEngine
    _, dec = make_frames()
    eng = TrackerEngine(n_streams=1)
    x = torch.from_numpy(np.stack(dec)).to(eng.device)
    for _ in range(groups):
        eng.jpeg_encode_batch(x, Q, SUB, threads=16)
        eng.jpeg_encode_batch(x, Q, SUB, threads=4, entropy="device")
    torch.cuda.synchronize()
    eng.close()
    return {"mode": "kernel", "groups": groups, "group_frames": G, "frame": f"1280x720 {SUB} q{Q}", "calls_per_group": ["entropy=host", "entropy=device"]}


def rates(n_frames, batch, rounds):
    from strongsort_yolo_amd import cli
    from strongsort_yolo_amd.yolo import YOLO
    _, dec = make_frames()
    tmp = tempfile.mkdtemp(prefix="jpeg_encode_time_")
    src = os.path.join(tmp, "clip.npy")
    np.save(src, np.stack([dec[k % G] for k in range(n_frames)]))

    class PillowSink(cli.FrameSink):                         # the raw download, then the host's encoder
        def __init__(self, path, **kw):
            super().__init__(path[:-len(".pil")] + ".bgr")
            self.kind = "pillow"

        def write(self, frame):
            self._f.write(_pillow(frame))
            self.n += 1

        def close(self):
            self._f.close()
    plain = cli.FrameSink
    legs = {"raw_bgr_download": ({"save": os.path.join(tmp, "a.bgr")}, plain),
            "device_encode_mjpeg": ({"save": os.path.join(tmp, "b.mjpeg"), "device_encode": True, "save_quality": Q, "save_subsampling": SUB}, plain),
            "download_then_pillow": ({"save": os.path.join(tmp, "c.pil")}, PillowSink),
            "device_encode_entropy_mjpeg": ({"save": os.path.join(tmp, "d.mjpeg"), "device_encode": True, "device_encode_entropy": True, "save_quality": Q,
                                             "save_subsampling": SUB}, plain)}
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack")

    def run(name, limit=None):
        extra, sink = legs[name]
        cli.FrameSink = sink
        try:
            model._frame_index = 0
            if getattr(model, "_stream_pipe", None) is not None:
                model._stream_pipe.reset_tracker(-1)
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = cli.process_video({"source": src, "track": True, "count": True, "tracker": "bytetrack", "batch": batch, "limit": limit,
                                     "outdir": os.path.join(tmp, "labels"), **extra}, model=model)
            return out["frames"] / (time.perf_counter() - t)
        finally:
            cli.FrameSink = plain
    for k in legs:                                           # builds the pipeline, captures the graphs, sizes every buffer
        run(k, 2 * batch)
    fps = {k: [] for k in legs}
    names = list(legs)
    for r in range(rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            fps[k].append(run(k))
    model.close()
    res = {"mode": "rates", "weights": "yolov8n (seeded random init)", "tracker": "bytetrack", "frame": f"1280x720 {SUB} q{Q}", "batch": batch,
           "frames": n_frames, "rounds": rounds, "host_cpus": len(os.sched_getaffinity(0)),
           "output_bytes": {k: os.path.getsize(v[0]["save"] if not v[0]["save"].endswith(".pil") else v[0]["save"][:-4] + ".bgr") for k, v in legs.items()}}
    for k, v in fps.items():
        res[f"{k}_frames_per_s"] = _spread(v)
        res[f"{k}_all"] = [round(x, 1) for x in v]
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("host", "kernel", "rates"), default="host")
    p.add_argument("--groups", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--frames", type=int, default=128)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--rounds", type=int, default=5)
    a = p.parse_args()
    print(json.dumps(host(a.groups, a.warmup) if a.mode == "host" else kernel(a.groups) if a.mode == "kernel" else rates(a.frames, a.batch, a.rounds)))
