"""Timing of the BYTE tracker family (docs/BYTETRACK.md).  One JSON line per run on stdout.

  --mode kernel --streams S   k_byte_group alone: BASELINE configs[1]-like streams (1280x720, ~28 detections a frame, a share
                              of low scores, dropped sightings, false positives), 32-frame groups; wall time per call (events).
                              For the kernel's own time run it under `rocprofv3 --kernel-trace --stats -- python tools/byte_time.py ...`.
  --mode rates                YOLO.track() calls/s and track_stream frames/s, yolov8n (seeded random-init weights), bytetrack
                              mode beside the default StrongSORT (fp32 ReID) in the same process.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def kernel(S, groups, warmup):
    from strongsort_yolo_amd.config import ByteTrackConfig
    from strongsort_yolo_amd.engine import ByteTrackEngine
    from tests.test_bytetrack_cpu import byte_stream
    G = 32
    n = (groups + warmup) * G
    streams = [byte_stream(100 + s, n) for s in range(S)]
    dev = torch.device("cuda", 0)
    hd, hn = np.zeros((n, S, 128, 6), np.float32), np.zeros((n, S), np.int32)
    for f in range(n):
        for s in range(S):
            d = streams[s][f]
            hd[f, s, :len(d)], hn[f, s] = d, len(d)
    dets, nd = torch.from_numpy(hd).to(dev), torch.from_numpy(hn).to(dev)
    out = torch.zeros(G, S, 256, 8, device=dev)
    nout = torch.zeros(G, S, dtype=torch.int32, device=dev)
    eng = ByteTrackEngine(ByteTrackConfig(), S, 0)
    eng.use_current_stream()
    ms = []
    for g in range(groups + warmup):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.update_group(G, dets[g * G:(g + 1) * G], nd[g * G:(g + 1) * G], None, None, out, nout)
        b.record()
        b.synchronize()
        if g >= warmup:
            ms.append(a.elapsed_time(b))
    eng.check_errors()
    med = float(np.median(ms))
    return {"mode": "kernel", "streams": S, "group_frames": G, "groups": groups, "dets_per_frame": float(hn.mean()),
            "us_per_group_median": med * 1e3, "us_per_frame_per_stream": med * 1e3 / G,
            "us_per_group_min": float(np.min(ms)) * 1e3, "note": "host event pair around one launch (includes launch latency)"}


def rates(n_frames, batch):
    os.environ["SS_RANDOM_INIT"] = "1"
    from strongsort_yolo_amd.synth import make_stream
    from strongsort_yolo_amd.yolo import YOLO
    st = make_stream(0, 1280, 720, 28)
    frames = [st.frame_pixels(k).copy() for k in range(8)]
    res = {"mode": "rates", "weights": "yolov8n (seeded random init)", "frame": "1280x720", "batch": batch}
    for tt in ("bytetrack", "strongsort"):
        m = YOLO("yolov8n.pt", random_init_ok=True, tracker_type=tt)
        for k in range(10):
            m.track(frames[k % 8], persist=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for k in range(n_frames):
            m.track(frames[k % 8], persist=True)
        res[f"{tt}_track_calls_per_s"] = n_frames / (time.perf_counter() - t)
        src = [frames[k % 8] for k in range(n_frames)]
        for _ in m.track_stream(src[:2 * batch], batch=batch):
            pass
        t = time.perf_counter()
        for _ in m.track_stream(src, batch=batch):
            pass
        res[f"{tt}_track_stream_frames_per_s"] = n_frames / (time.perf_counter() - t)
        m.close()
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("kernel", "rates"), default="kernel")
    p.add_argument("--streams", type=int, default=1)
    p.add_argument("--groups", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--frames", type=int, default=256)
    p.add_argument("--batch", type=int, default=32)
    a = p.parse_args()
    r = kernel(a.streams, a.groups, a.warmup) if a.mode == "kernel" else rates(a.frames, a.batch)
    print(json.dumps(r))
