"""Timing of the redaction (docs/REDACT.md §6), in tools/zones_time.py's style.  One JSON line per run on stdout.

  --mode kernel   32 resident frames of 1280x720 with about 28 boxes a frame (BASELINE configs[1]-like streams): `ss_redact` in place for
                  blur at r = 7, 15, 31, pixelate at 16 and fill, over boxes (and at r = 15 over the inscribed ellipses), the regions
                  already on the device; beside it, in the same rounds, `ss_overlay` drawing those boxes with their label plates on the
                  same frames, and a device-to-device copy of the batch — what a snapshot design would pay before it filters anything.
                  Event pairs around one call each, legs interleaved, medians and minima over --rounds after --warmup.  For the kernels'
                  own times: `rocprofv3 --kernel-trace --stats -- python tools/redact_time.py --mode kernel` (a run of its own).
  --mode rates    the CLI's process_video on `synthetic:N` (640x480) with yolov8n (seeded random-init weights), --tracker ocsort,
                  batch 32, --save clip.mjpeg --device-encode: frames/s without and with --redact blur, legs alternating in one process.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, B = 720, 1280, 32


def _boxes(rng, n):
    w, h = rng.integers(40, 140, n), rng.integers(90, 300, n)
    x0, y0 = rng.integers(-20, W - 60, n), rng.integers(-20, H - 100, n)
    return np.stack([x0, y0, x0 + w, y0 + h], 1)


def kernel(rounds, warmup):
    from strongsort_yolo_amd import redact
    from strongsort_yolo_amd.engine import TrackerEngine
    from strongsort_yolo_amd.overlay import CommandList, Overlay, bgr
    from strongsort_yolo_amd.overlay_font import ADVANCE
    dev = torch.device("cuda", 0)
    eng = TrackerEngine(None, 1, 0)
    ov = Overlay({}, eng)
    rng = np.random.default_rng(28)
    per = [_boxes(rng, int(rng.integers(24, 33))) for _ in range(B)]
    off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int32)
    d_off = torch.from_numpy(off).to(dev)
    d_verts = torch.zeros(1, 2, dtype=torch.int32, device=dev)

    def rows(kind):
        return torch.from_numpy(np.concatenate([np.concatenate([np.full((len(p), 1), kind), p, np.zeros((len(p), 3), int)], 1) for p in per]).astype(np.int32)).to(dev)

    d_rect, d_ell = rows(redact.RECT), rows(redact.ELLIPSE)
    lists = []
    for p in per:                                                          # what Overlay._box draws per box: outline, label plate, label
        cl = CommandList()
        for i, (x0, y0, x1, y1) in enumerate(p.tolist()):
            label = f" ID: {i} person 87.5%"
            cl.rect(x0, y0, x1, y1, bgr(0, 0, 225), 2); cl.fill(x0, y0, x0 + ADVANCE * len(label) + 2, y0 - 12, bgr(30, 30, 30)); cl.text(label, x0, y0 - 3, bgr(255, 255, 255))
        lists.append(cl)
    arr = [c.arrays() for c in lists]
    prims, coff, poff = [], 0, np.zeros(B + 1, np.int32)
    for i, (p, ch) in enumerate(arr):
        p = p.copy(); p[p[:, 0] == 4, 6] += coff; prims.append(p); poff[i + 1] = poff[i] + len(p); coff += len(ch)
    d_prims, d_poff = torch.from_numpy(np.concatenate(prims)).to(dev), torch.from_numpy(poff).to(dev)
    d_chars = torch.from_numpy(np.concatenate([ch for _, ch in arr])).to(dev)
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev)
    spare = torch.empty_like(frames)
    scratch = torch.empty(int(eng.L.ss_redact_scratch_bytes(B, H, W)), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def red(effect, strength, d_rows):
        return lambda: eng._ck(eng.L.ss_redact(eng.ctx, C.c_void_p(st.cuda_stream), ptr(frames), B, frames.stride(0), H, W, frames.stride(1), ptr(d_rows), ptr(d_off),
                                               ptr(d_verts), effect, strength, 0x203040, ptr(scratch), scratch.numel()))

    legs = {"blur_r7": red(0, 7, d_rect), "blur_r15": red(0, 15, d_rect), "blur_r31": red(0, 31, d_rect), "blur_r15_ellipse": red(0, 15, d_ell),
            "pixelate_16": red(1, 16, d_rect), "fill": red(2, 0, d_rect),
            "overlay": lambda: eng._ck(eng.L.ss_overlay(eng.ctx, C.c_void_p(st.cuda_stream), ptr(frames), B, frames.stride(0), H, W, frames.stride(1), ptr(d_prims),
                                                        ptr(d_poff), ptr(d_chars))),
            "copy": lambda: spare.copy_(frames)}
    ms = {k: [] for k in legs}
    for r in range(rounds + warmup):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):         # interleaved, the order alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); legs[k](); b.record(); b.synchronize()
            if r >= warmup:
                ms[k].append(a.elapsed_time(b))
    eng.close()
    med = {k: float(np.median(v)) * 1e3 for k, v in ms.items()}
    return {"mode": "kernel", "frames": B, "frame": f"{W}x{H}", "boxes_per_frame": float(np.mean([len(p) for p in per])), "rounds": rounds,
            **{f"{k}_us_median": round(v, 1) for k, v in med.items()}, **{f"{k}_us_min": round(float(np.min(v)) * 1e3, 1) for k, v in ms.items()},
            "blur_r15_over_copy_plus_overlay": round(med["blur_r15"] / (med["copy"] + med["overlay"]), 3), "batch_bytes": int(frames.numel()),
            "scratch_bytes": int(scratch.numel()), "note": "host event pair around one call (includes launch latency; ss_redact is a memset and three launches)"}


def rates(n_frames, rounds):
    os.environ["SS_RANDOM_INIT"] = "1"
    from strongsort_yolo_amd import cli
    from strongsort_yolo_amd.yolo import YOLO
    legs = {"plain": {}, "redact_blur": {"redact": "blur"}}
    fps, dev = {k: [] for k in legs}, torch.device("cuda", 0)
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="ocsort")
    model.overrides.update(conf=0.01, max_det=100)                         # seeded random-init weights: a low threshold, so that there are boxes to hide
    with tempfile.TemporaryDirectory() as tmp:
        base = {"source": f"synthetic:{n_frames}", "track": True, "count": False, "tracker": "ocsort", "batch": 32, "random_init": True, "outdir": tmp,
                "save": os.path.join(tmp, "clip.mjpeg"), "device_encode": True}
        cli.process_video(dict(base, source="synthetic:64", redact="blur"), model=model)        # warm-up: the pipeline and its kernels exist
        for r in range(rounds):
            for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
                torch.cuda.synchronize(dev)
                t = time.perf_counter()
                out = cli.process_video(dict(base, **legs[leg]), model=model)
                torch.cuda.synchronize(dev)
                fps[leg].append(out["frames"] / (time.perf_counter() - t))
    model.close()
    res = {"mode": "rates", "weights": "yolov8n (seeded random init, conf 0.01)", "frame": "640x480", "frames": n_frames, "batch": 32, "rounds": rounds,
           "sink": "clip.mjpeg, --device-encode"}
    for leg, v in fps.items():
        res[f"{leg}_frames_per_s_median"], res[f"{leg}_frames_per_s_all"] = float(np.median(v)), [round(x, 1) for x in v]
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("kernel", "rates"), default="kernel")
    p.add_argument("--rounds", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--frames", type=int, default=256)
    a = p.parse_args()
    print(json.dumps(kernel(a.rounds, a.warmup) if a.mode == "kernel" else rates(a.frames, a.rounds)))
