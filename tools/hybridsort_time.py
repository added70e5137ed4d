"""Timing of the Hybrid-SORT tracker (docs/HYBRIDSORT.md §6), in tools/ocsort_time.py's style.  One JSON line per run on stdout.

  --mode kernel --streams S   k_hybrid_group beside k_ocsort_group (the same use_byte) and k_byte_group (xyah) on the same rows in the
                              same run: tools/ocsort_time.py's streams (1280x720, ~28 detections a frame, a share of low scores,
                              dropped sightings, false positives), 32-frame groups, the three engines called alternately; wall time per
                              call (events).  For the kernels' own times run it under
                              `rocprofv3 --kernel-trace --stats -- python tools/hybridsort_time.py ...` (counters, if wanted, in a
                              run of their own).  --no-byte: both OC-SORT family trackers without their BYTE stage.
                              --steady: every object seen on every frame and no false positives (no gaps, so no ORU re-update).
  --mode rates                track_stream frames/s (and track() calls/s) of yolov8n (seeded random-init weights) with ocsort and
                              hybridsort: one leg per fresh process, the legs interleaved (--rounds each, default 2).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

LEGS = ("ocsort", "hybridsort")


def _steady_stream(seed, n):
    from strongsort_yolo_amd.synth import make_stream
    st = make_stream(seed, 1280, 720, 28)
    return [np.ascontiguousarray(st.next_frame().dets.astype(np.float32)[:128]) for _ in range(n)]


def kernel(S, groups, warmup, use_byte, steady):
    from strongsort_yolo_amd.config import ByteTrackConfig, HybridSortConfig, OCSortConfig
    from strongsort_yolo_amd.engine import ByteTrackEngine, HybridSortEngine, OCSortEngine
    from tests.test_bytetrack_cpu import byte_stream
    G = 32
    n = (groups + warmup) * G
    streams = [(_steady_stream if steady else byte_stream)(100 + s, n) for s in range(S)]
    dev = torch.device("cuda", 0)
    hd, hn = np.zeros((n, S, 128, 6), np.float32), np.zeros((n, S), np.int32)
    for f in range(n):
        for s in range(S):
            d = streams[s][f]
            hd[f, s, :len(d)], hn[f, s] = d, len(d)
    dets, nd = torch.from_numpy(hd).to(dev), torch.from_numpy(hn).to(dev)
    out = torch.zeros(G, S, 256, 8, device=dev)
    nout = torch.zeros(G, S, dtype=torch.int32, device=dev)
    engs = {"byte": ByteTrackEngine(ByteTrackConfig(), S, 0), "ocsort": OCSortEngine(OCSortConfig(use_byte=use_byte), S, 0),
            "hybrid": HybridSortEngine(HybridSortConfig(use_byte=use_byte), S, 0)}
    ms, tracks = {k: [] for k in engs}, {"ocsort": [], "hybrid": []}
    for e in engs.values():
        e.use_current_stream()
    for g in range(groups + warmup):
        sl = slice(g * G, (g + 1) * G)
        for leg, eng in engs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.update_group(G, dets[sl], nd[sl], None, None, out, nout)
            b.record()
            b.synchronize()
            if g >= warmup:
                ms[leg].append(a.elapsed_time(b))
        for k in tracks:
            tracks[k].append(engs[k].tracks(0)["n_tracks"])
    for e in engs.values():
        e.check_errors()
    med = {k: float(np.median(v)) * 1e3 for k, v in ms.items()}
    return {"mode": "kernel", "streams": S, "group_frames": G, "groups": groups, "use_byte": bool(use_byte), "steady": bool(steady),
            "dets_per_frame": float(hn.mean()), "ocsort_tracks_stream0_mean": float(np.mean(tracks["ocsort"])),
            "hybrid_tracks_stream0_mean": float(np.mean(tracks["hybrid"])),
            "byte_us_per_group_median": med["byte"], "ocsort_us_per_group_median": med["ocsort"], "hybrid_us_per_group_median": med["hybrid"],
            "hybrid_over_ocsort": med["hybrid"] / med["ocsort"], "hybrid_over_byte": med["hybrid"] / med["byte"],
            "note": "host event pair around one call (includes launch latency); kernel times: rocprofv3 --kernel-trace --stats"}


def rate_leg(leg, n_frames, batch):
    """One leg in this process: yolov8n with tracker_type `leg` on 1280x720 synthetic frames."""
    os.environ["SS_RANDOM_INIT"] = "1"
    from strongsort_yolo_amd.synth import make_stream
    from strongsort_yolo_amd.yolo import YOLO
    st = make_stream(0, 1280, 720, 28)
    frames = [st.frame_pixels(k).copy() for k in range(8)]
    m = YOLO("yolov8n.pt", random_init_ok=True, tracker_type=leg, **({"ocsort_use_byte": True} if leg == "ocsort" else {}))
    for k in range(10):
        m.track(frames[k % 8], persist=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for k in range(n_frames):
        m.track(frames[k % 8], persist=True)
    res = {"leg": leg, "track_calls_per_s": n_frames / (time.perf_counter() - t)}
    src = [frames[k % 8] for k in range(n_frames)]
    for _ in m.track_stream(src[:2 * batch], batch=batch):
        pass
    t = time.perf_counter()
    for _ in m.track_stream(src, batch=batch):
        pass
    res["track_stream_frames_per_s"] = n_frames / (time.perf_counter() - t)
    m.close()
    return res


def rates(n_frames, batch, rounds):
    legs = {k: [] for k in LEGS}
    for r in range(rounds):
        for leg in (LEGS if r % 2 == 0 else LEGS[::-1]):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--frames", str(n_frames), "--batch", str(batch)],
                               capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise RuntimeError(f"leg {leg} failed ({p.returncode}): {p.stderr[-2000:]}")
            legs[leg].append(json.loads(p.stdout.strip().splitlines()[-1]))
    res = {"mode": "rates", "weights": "yolov8n (seeded random init)", "frame": "1280x720", "batch": batch, "rounds": rounds,
           "note": "both legs with their BYTE stage"}
    for leg, rs in legs.items():
        for k in ("track_calls_per_s", "track_stream_frames_per_s"):
            res[f"{leg}_{k}_median"] = float(np.median([r[k] for r in rs]))
            res[f"{leg}_{k}_all"] = [round(r[k], 1) for r in rs]
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("kernel", "rates"), default="kernel")
    p.add_argument("--streams", type=int, default=1)
    p.add_argument("--groups", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--frames", type=int, default=256)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--rounds", type=int, default=2, help="rates: processes per leg")
    p.add_argument("--no-byte", action="store_true", help="kernel: OC-SORT and Hybrid-SORT without their BYTE stage")
    p.add_argument("--steady", action="store_true", help="kernel: streams without missed sightings or false positives")
    p.add_argument("--leg", choices=LEGS, default=None, help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.leg is not None:
        r = rate_leg(a.leg, a.frames, a.batch)
    elif a.mode == "kernel":
        r = kernel(a.streams, a.groups, a.warmup, not a.no_byte, a.steady)
    else:
        r = rates(a.frames, a.batch, a.rounds)
    print(json.dumps(r))
