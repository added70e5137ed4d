"""Segmentation results per frame: host masks (YOLO default: assemble_masks + mask_polygon when masks.xy is read) against device
masks (YOLO(device_masks=True), csrc/ss_mask.hip), and the same model with masks not read at all.  configs[1] geometry (480x640
frames, 384x640 network input, 32x96x160 prototypes), yolov8n-seg on seeded random-init weights with a low confidence threshold so
that every frame keeps max_det = 28 or 100 rows (the NMS then sees every anchor: all three paths pay that alike).

Every measurement ("leg") runs in a fresh process with the same warm-up (per-frame: 5 calls, stream: one whole call of `batch`
frames, each reading what the timed part reads); the legs are interleaved, their order rotated from one repetition to the next.
Prints one JSON line per leg and one summary line per (path, form, masks) with the median over the repetitions.

    python tools/mask_time.py [--reps 2] [--frames 32]
    python tools/mask_time.py --leg device_masks track 28      (one leg, used by the above)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = ("no_masks_read", "device_masks", "host_masks")
WARM = 5


def leg(path, form, n, nframes, batch=16):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    os.environ.setdefault("SS_RANDOM_INIT", "1")
    from strongsort_yolo_amd.yolo import YOLO
    m = YOLO("yolov8n-seg.pt", random_init_ok=True, device_masks=path == "device_masks")
    m.overrides.update(conf=0.05, iou=0.95, agnostic_nms=True, max_det=n)
    xy = path != "no_masks_read"
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(nframes)]

    def read(res):
        r = res[0]
        if xy and r.masks is not None:
            _ = r.masks.xy
        return 0 if r.masks is None else len(r.masks)

    if form == "track":
        for f in frames[:WARM]:
            read(m.track(f, persist=True))
        torch.cuda.synchronize()
        t0, kept = time.perf_counter(), 0
        for f in frames:
            kept += read(m.track(f, persist=True))
    else:
        for res in m.track_stream(iter(frames[:batch]), batch=batch):
            read(res)
        torch.cuda.synchronize()
        t0, kept = time.perf_counter(), 0
        for res in m.track_stream(iter(frames), batch=batch):
            kept += read(res)
    dt = (time.perf_counter() - t0) / len(frames)
    m.close()
    return {"path": path, "form": form if form == "track" else f"track_stream{batch}", "max_det": n,
            "masks_per_frame": round(kept / len(frames), 1), "ms_per_frame": round(dt * 1e3, 3), "frames_per_s": round(1.0 / dt, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--leg", nargs=3, default=None, metavar=("PATH", "FORM", "MAX_DET"))
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(leg(a.leg[0], a.leg[1], int(a.leg[2]), a.frames)), flush=True)
        return
    got = {}
    for rep in range(a.reps):
        for n in (28, 100):
            for form in ("track", "stream"):
                order = PATHS[rep % 3:] + PATHS[:rep % 3]
                for path in order:
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--frames", str(a.frames), "--leg", path, form, str(n)],
                                         capture_output=True, text=True, timeout=600)
                    if out.returncode != 0:
                        sys.stderr.write(out.stderr[-3000:])
                        raise SystemExit(f"leg {path} {form} {n}: exit {out.returncode}")
                    d = json.loads(out.stdout.strip().splitlines()[-1])
                    d["rep"] = rep
                    print(json.dumps(d), flush=True)
                    got.setdefault((d["path"], d["form"], n), []).append(d)
    for (path, form, n), ds in got.items():
        ms = statistics.median(d["ms_per_frame"] for d in ds)
        print(json.dumps({"summary": True, "path": path, "form": form, "max_det": n, "masks_per_frame": ds[0]["masks_per_frame"],
                          "median_ms_per_frame": round(ms, 3), "median_frames_per_s": round(1e3 / ms, 1),
                          "ms_per_frame_each": [d["ms_per_frame"] for d in ds]}), flush=True)


if __name__ == "__main__":
    main()
