"""Timing of the JPEG front door (docs/JPEG.md "Measured").  One JSON line per run on stdout.

The frames: 32 rendered synthetic 1280x720 frames (synth.render on a graded background with sensor-like noise), encoded with
Pillow as baseline JPEG, 4:2:0, quality 85 (Pillow is needed here, to make the input and for the comparison leg).

  --mode host     the host stage: wall time of engine.jpeg_decode_batch on groups of 32 (the call returns once the coefficient copy
                  and the two launches are enqueued), frames/s at threads 1, 4 and 16; the device is synchronised between calls
  --mode kernel   the same call in a loop and nothing else; for the kernels' own times run it under
                  `rocprofv3 --kernel-trace --stats -- python tools/jpeg_time.py --mode kernel` (no counters in that run)
  --mode rates    YOLO.track_stream frames/s (bytetrack, yolov8n with seeded random-init weights, batch 32) from three sources in ONE
                  process, the legs interleaved over --rounds: EncodedFrames (device decode), the same frames as decoded arrays
                  (the ceiling: no decoding at all) and Pillow decoding inside the iterator (the directory source of cli.py)
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
    for th in (1, 4, 16):
        ms = []
        for g in range(groups + warmup):
            torch.cuda.synchronize()
            t = time.perf_counter()
            eng.jpeg_decode_batch(out, frames, threads=th)
            dt = time.perf_counter() - t
            if g >= warmup:
                ms.append(dt * 1e3)
        res[f"threads_{th}_ms_per_group"] = _spread(ms)
        res[f"threads_{th}_frames_per_s_median"] = G / (float(np.median(ms)) * 1e-3)
    torch.cuda.synchronize()
    res["equal_to_pillow"] = bool(all(np.array_equal(out[k].cpu().numpy(), dec[k]) for k in range(G)))
    eng.close()
    return res


def kernel(groups):
    from strongsort_yolo_amd import jpeg
    from strongsort_yolo_amd.engine import TrackerEngine
    enc, _ = make_frames()
    frames = [jpeg.EncodedFrame(d) for d in enc]
    eng = TrackerEngine(n_streams=1)
    out = torch.empty((G, 720, 1280, 3), dtype=torch.uint8, device=eng.device)
    for _ in range(groups):
        eng.jpeg_decode_batch(out, frames, threads=4)
    torch.cuda.synchronize()
    eng.close()
    return {"mode": "kernel", "groups": groups, "group_frames": G, "frame": "1280x720 4:2:0 q85"}


def rates(n_frames, batch, rounds):
    from PIL import Image
    from strongsort_yolo_amd import jpeg
    from strongsort_yolo_amd.yolo import YOLO
    enc, dec = make_frames()
    frames = [jpeg.EncodedFrame(d) for d in enc]

    def pillow():                                            # cli.frame_source's directory branch, the files already in memory
        for k in range(n_frames):
            yield np.asarray(Image.open(io.BytesIO(enc[k % G])).convert("RGB"))[:, :, ::-1].copy()

    legs = {"device_decode": lambda: (frames[k % G] for k in range(n_frames)),
            "decoded_arrays": lambda: (dec[k % G] for k in range(n_frames)),
            "pillow_in_iterator": pillow}
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack")
    for src in legs.values():                                # builds the pipeline, captures the graphs, sizes the staging areas
        for _ in model.track_stream((f for _, f in zip(range(2 * batch), src())), batch=batch):
            pass
    fps = {k: [] for k in legs}
    names = list(legs)
    for r in range(rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in model.track_stream(legs[k](), batch=batch):
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
    a = p.parse_args()
    print(json.dumps(host(a.groups, a.warmup) if a.mode == "host" else kernel(a.groups) if a.mode == "kernel" else rates(a.frames, a.batch, a.rounds)))
