"""Timing of BoT-SORT's camera-motion estimators (docs/BYTETRACK.md §1b, §1f).  One JSON line per run on stdout.

  --mode kernel   ss_gmc_sparse_estimate and ss_cmc_estimate alone, called alternately on the same 32-frame groups of panning
                  1280x720 frames (--streams S streams): wall time per call (event pairs, launch latency included), median and
                  spread over --groups calls.  For the kernels' own times run it under
                  `rocprofv3 --kernel-trace --stats -- python tools/gmc_time.py --mode kernel` (no counters in that run).
  --mode rates    YOLO.track_stream frames/s, yolov8n (seeded random-init weights), tracker botsort: no GMC, gmc_method "ecc" and
                  "sparseOptFlow" in ONE process, --rounds repetitions of --frames frames each, the three legs interleaved.
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

from tools.byte_time import _pan_frames  # noqa: E402


def _spread(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(len(v))}


def kernel(S, groups, warmup):
    from strongsort_yolo_amd.engine import TrackerEngine
    G = 32
    dev = torch.device("cuda", 0)
    eng = TrackerEngine(n_streams=S)
    eng.use_current_stream()
    frames = torch.from_numpy(_pan_frames(G, S)).to(dev)
    w_sparse, w_ecc = eng.gmc_sparse_estimate(frames, G), eng.cmc_estimate(frames, G)      # size the buffers
    ms = {"sparse": [], "ecc": []}
    for g in range(groups + warmup):
        for leg, fn in (("sparse", lambda: eng.gmc_sparse_estimate(frames, G, w_sparse)), ("ecc", lambda: eng.cmc_estimate(frames, G, w_ecc))):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if g >= warmup:
                ms[leg].append(a.elapsed_time(b) * 1e3)
    ws, we = w_sparse.cpu().numpy(), w_ecc.cpu().numpy()
    st = eng.gmc_sparse_stages(5, 0)
    eng.close()
    res = {"mode": "kernel", "streams": S, "group_frames": G, "frame": "1280x720",
           "sparse_us_per_group": _spread(ms["sparse"]), "ecc_us_per_group": _spread(ms["ecc"]),
           "sparse_us_per_frame_per_stream_median": float(np.median(ms["sparse"])) / (G * S),
           "ecc_us_per_frame_per_stream_median": float(np.median(ms["ecc"])) / (G * S),
           "sparse_warps": int((ws[..., 6] >= 0).sum()), "sparse_inliers_mean": float(ws[..., 6][ws[..., 6] >= 0].mean()),
           "sparse_matches_mean": float(ws[..., 7].mean()), "corner_candidates_frame5": st["n_candidates"],
           "sparse_translation_median": [float(np.median(ws[1:, :, 2])), float(np.median(ws[1:, :, 5]))],
           "ecc_translation_median": [float(np.median(we[1:, :, 2])), float(np.median(we[1:, :, 5]))],
           "note": "host event pair around one call (includes launch latency); kernel times: rocprofv3 --kernel-trace --stats"}
    return res


def rates(n_frames, batch, rounds):
    from strongsort_yolo_amd.yolo import YOLO
    pan = _pan_frames(16, 1)
    frames = [pan[k].copy() for k in range(16)]
    frames += frames[::-1]                                  # back and forth: the sequence can repeat without a jump
    src = [frames[k % 32] for k in range(n_frames)]
    legs = {"botsort": {}, "botsort_ecc": {"camera_motion": True}, "botsort_sparse": {"camera_motion": True, "gmc_method": "sparseOptFlow"}}
    models = {k: YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", **kw) for k, kw in legs.items()}
    fps = {k: [] for k in legs}
    for m in models.values():                               # builds the pipelines and captures the graphs
        for _ in m.track_stream(src[:2 * batch], batch=batch):
            pass
    names = list(legs)
    for r in range(rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in models[k].track_stream(src, batch=batch):
                pass
            fps[k].append(n_frames / (time.perf_counter() - t))
    for m in models.values():
        m.close()
    res = {"mode": "rates", "weights": "yolov8n (seeded random init)", "frame": "1280x720", "batch": batch, "frames": n_frames, "rounds": rounds}
    for k, v in fps.items():
        res[f"{k}_track_stream_frames_per_s"] = _spread(v)
        res[f"{k}_all"] = [round(x, 1) for x in v]
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("kernel", "rates"), default="kernel")
    p.add_argument("--streams", type=int, default=1)
    p.add_argument("--groups", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--frames", type=int, default=256)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--rounds", type=int, default=5)
    a = p.parse_args()
    print(json.dumps(kernel(a.streams, a.groups, a.warmup) if a.mode == "kernel" else rates(a.frames, a.batch, a.rounds)))
