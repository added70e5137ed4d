"""Timing of the JPEG front door (docs/JPEG.md "Measured").  One JSON line per run on stdout.

The frames: 32 rendered synthetic 1280x720 frames (synth.render on a graded background with sensor-like noise), encoded with
Pillow as baseline JPEG, 4:2:0, quality 85 (Pillow is needed here, to make the input and for the comparison leg).

  --mode host     the host stage: wall time of engine.jpeg_decode_batch on groups of 32 (the call returns once the copy and the
                  launches are enqueued), frames/s with the host entropy stage at threads 1, 4 and 16 and with the device entropy
                  stage (docs/JPEG.md section 12) at threads 1 and 4, the five legs interleaved group by group in one process; the
                  device is synchronised between calls; bytes that cross PCIe per frame, both ways, for both stages
  --mode kernel   the same call in a loop and nothing else (--entropy device: with the device entropy stage, which adds k_jpeg_huff
                  and k_jpeg_dc); for the kernels' own times run it under
                  `rocprofv3 --kernel-trace --stats -- python tools/jpeg_time.py --mode kernel` (no counters in that run)
  --mode rates    YOLO.track_stream frames/s (bytetrack, yolov8n with seeded random-init weights, batch 32) from four sources in ONE
                  process, the legs interleaved over --rounds: EncodedFrames (device decode, host entropy stage), EncodedFrames with the
                  device entropy stage, the same frames as decoded arrays (the ceiling: no decoding at all) and Pillow decoding inside
                  the iterator (the directory source of cli.py)
"""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

G = 32


def _spread(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(len(v))}


def make_frames(n=G, H=720, W=1280, seed=0):
    """n encoded frames (bytes) and their Pillow decodes as BGR arrays."""
    from PIL import Image
    from strongsort_yolo_amd.synth import make_stream
    st, rng = make_stream(seed, W, H, 30), np.random.default_rng(seed)
    grade = np.add.outer(np.linspace(0, 60, H), np.linspace(0, 40, W))[:, :, None]
    enc, dec = [], []
    for _ in range(n):
        img = st.render(st.next_frame()).astype(np.float32) + grade - 40 + rng.normal(0, 4, (H, W, 3))
        buf = io.BytesIO()
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)[:, :, ::-1]).save(buf, "JPEG", quality=85, subsampling="4:2:0")
        enc.append(buf.getvalue())
        dec.append(np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(enc[-1])).convert("RGB"))[:, :, ::-1]))
    return enc, dec


def host(groups, warmup):
    from strongsort_yolo_amd import jpeg
    from strongsort_yolo_amd.engine import TrackerEngine
    enc, dec = make_frames()
    frames = [jpeg.EncodedFrame(d) for d in enc]
    eng = TrackerEngine(n_streams=1)
    out = torch.empty((G, 720, 1280, 3), dtype=torch.uint8, device=eng.device)
    res = {"mode": "host", "frame": "1280x720 4:2:0 q85", "group_frames": G, "bytes_per_frame_mean": float(np.mean([len(d) for d in enc]))}
    legs = [("host", 1), ("host", 4), ("host", 16), ("device", 1), ("device", 4)]
    ms = {leg: [] for leg in legs}
    for g in range(groups + warmup):                          # interleaved: every leg sees the same machine
        for leg in (legs if g % 2 == 0 else legs[::-1]):
            torch.cuda.synchronize()
            t = time.perf_counter()
            eng.jpeg_decode_batch(out, frames, threads=leg[1], entropy=leg[0])
            dt = time.perf_counter() - t
            if g >= warmup:
                ms[leg].append(dt * 1e3)
    for (ent, th), v in ms.items():
        key = f"threads_{th}" if ent == "host" else f"device_entropy_threads_{th}"
        res[f"{key}_ms_per_group"] = _spread(v)
        res[f"{key}_frames_per_s_median"] = G / (float(np.median(v)) * 1e-3)
    for ent in ("host", "device"):
        eng.jpeg_decode_batch(out, frames, threads=4, entropy=ent)
        torch.cuda.synchronize()
        eng.check_errors()
        res["equal_to_pillow" + ("" if ent == "host" else "_device_entropy")] = bool(all(np.array_equal(out[k].cpu().numpy(), dec[k]) for k in range(G)))
    # what crosses PCIe per frame: the sparse stream of the host stage (header, block table, entries) against the device stage's
    # header, Huffman tables, segment table and unstuffed scan; back: nothing, and one status word
    import ctypes as C
    up_host, up_dev = [], []
    for f in frames:
        raw, segs, hdr = jpeg.scan_segments(f.data)
        coef, quant = np.zeros(int(hdr[4]) * 64, np.int16), np.zeros((4, 64), np.uint16)
        eng.L.ss_jpeg_coefficients(f.data, len(f.data), coef.ctypes.data_as(C.POINTER(C.c_short)), coef.size, quant.ctypes.data_as(C.POINTER(C.c_ushort)))
        up_host.append(640 + 4 * (int(hdr[4]) + 1) + 4 * int(np.count_nonzero(coef)))
        up_dev.append(640 + int(hdr[0]) * 2 * 1376 + 20 * len(segs) + len(raw))
    res["pcie_up_bytes_per_frame_host_entropy"] = float(np.mean(up_host))
    res["pcie_up_bytes_per_frame_device_entropy"] = float(np.mean(up_dev))
    res["pcie_down_bytes_per_frame_host_entropy"], res["pcie_down_bytes_per_frame_device_entropy"] = 0, 4
    eng.close()
    return res


def kernel(groups, entropy="host"):
    from strongsort_yolo_amd import jpeg
    from strongsort_yolo_amd.engine import TrackerEngine
    enc, _ = make_frames()
    frames = [jpeg.EncodedFrame(d) for d in enc]
    eng = TrackerEngine(n_streams=1)
    out = torch.empty((G, 720, 1280, 3), dtype=torch.uint8, device=eng.device)
    for _ in range(groups):
        eng.jpeg_decode_batch(out, frames, threads=4, entropy=entropy)
    torch.cuda.synchronize()
    eng.check_errors()
    eng.close()
    return {"mode": "kernel", "entropy": entropy, "groups": groups, "group_frames": G, "frame": "1280x720 4:2:0 q85"}


def rates(n_frames, batch, rounds):
    from PIL import Image
    from strongsort_yolo_amd import jpeg
    from strongsort_yolo_amd.yolo import YOLO
    enc, dec = make_frames()
    frames = [jpeg.EncodedFrame(d) for d in enc]

    def pillow():                                            # cli.frame_source's directory branch, the files already in memory
        for k in range(n_frames):
            yield np.asarray(Image.open(io.BytesIO(enc[k % G])).convert("RGB"))[:, :, ::-1].copy()

    kw = {"device_decode_device_entropy": {"jpeg_entropy": "device"}}
    legs = {"device_decode": lambda: (frames[k % G] for k in range(n_frames)),
            "device_decode_device_entropy": lambda: (frames[k % G] for k in range(n_frames)),
            "decoded_arrays": lambda: (dec[k % G] for k in range(n_frames)),
            "pillow_in_iterator": pillow}
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack")
    for name, src in legs.items():                           # builds the pipeline, captures the graphs, sizes the staging areas
        for _ in model.track_stream((f for _, f in zip(range(2 * batch), src())), batch=batch, **kw.get(name, {})):
            pass
    fps = {k: [] for k in legs}
    names = list(legs)
    for r in range(rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in model.track_stream(legs[k](), batch=batch, **kw.get(k, {})):
                pass
            fps[k].append(n_frames / (time.perf_counter() - t))
    model.close()
    res = {"mode": "rates", "weights": "yolov8n (seeded random init)", "tracker": "bytetrack", "frame": "1280x720 4:2:0 q85", "batch": batch,
           "frames": n_frames, "rounds": rounds, "host_cpus": len(os.sched_getaffinity(0))}
    for k, v in fps.items():
        res[f"{k}_track_stream_frames_per_s"] = _spread(v)
        res[f"{k}_all"] = [round(x, 1) for x in v]
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("host", "kernel", "rates"), default="host")
    p.add_argument("--groups", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--frames", type=int, default=512)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--entropy", choices=("host", "device"), default="host", help="--mode kernel: which entropy stage the loop runs")
    a = p.parse_args()
    print(json.dumps(host(a.groups, a.warmup) if a.mode == "host" else kernel(a.groups, a.entropy) if a.mode == "kernel" else rates(a.frames, a.batch, a.rounds)))
