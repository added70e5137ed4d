"""Timing of the analytics stage (docs/ZONES.md §6), in tools/ocsort_time.py's style.  One JSON line per run on stdout.

  --mode kernel --streams S   per 32-frame group on BASELINE configs[1]-like streams (1280x720, ~28 rows a frame): OC-SORT's group
                              launch, then k_zone_update on its rows where they are (4 lines, 4 zones, heat "box" at 8 px, every
                              output; --grids: also, or only, without the per-frame heat grids), then k_zone_heat_blend over 32 resident 1280x720 frames with the group's per-frame grids, then
                              a device-to-device copy of the same frame bytes (the yardstick: it reads and writes what the blend
                              reads and writes).  Wall time per call from event pairs; for the kernels' own times run it under
                              `rocprofv3 --kernel-trace --stats -- python tools/zones_time.py --mode kernel`.
  --mode rates                the CLI's process_video on `synthetic:N` (640x480) with yolov8n (seeded random-init weights) and
                              --tracker ocsort, batch 32: frames/s without the flags, with --line / --zone, and with --heatmap box
                              too, the legs alternating in one process (--rounds each).
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HW = (720, 1280)
LINES = [[640, 0, 640, 720], [0, 360, 1280, 360], [200, 100, 1100, 650], [1100, 100, 200, 650]]
ZONES = [[[100, 100], [600, 100], [600, 600], [100, 600]], [[700, 100], [1200, 100], [1200, 600], [700, 600]],
         [[400, 200], [900, 200], [900, 500], [400, 500]], [[0, 0], [1280, 0], [1280, 720], [640, 400], [0, 720]]]


def kernel(S, groups, warmup, grids):
    from strongsort_yolo_amd import zones
    from strongsort_yolo_amd.config import OCSortConfig
    from strongsort_yolo_amd.engine import OCSortEngine
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
    out, nout = torch.zeros(G, S, 256, 8, device=dev), torch.zeros(G, S, dtype=torch.int32, device=dev)
    oc = OCSortEngine(OCSortConfig(), S, 0)
    oc.use_current_stream()
    zc = zones.ZoneCounter(zones.ZoneConfig(lines=LINES, zones=ZONES, heat="box", heat_cell=8), oc, frame_hw=HW)
    frames = torch.randint(0, 256, (G,) + HW + (3,), dtype=torch.uint8, device=dev)
    spare = torch.empty_like(frames)
    ms = {k: [] for k in ("ocsort", "zone_update", "zone_update_no_grids", "heat_blend", "copy")}
    twin = OCSortEngine(OCSortConfig(), S, 0)           # the same launch without the per-frame heat grids, on a state of its own
    twin.use_current_stream()
    zt = zones.ZoneCounter(zones.ZoneConfig(lines=LINES, zones=ZONES, heat="box", heat_cell=8), twin, frame_hw=HW)
    rows = []

    def timed(leg, fn, keep):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        if keep:
            ms[leg].append(a.elapsed_time(b))
        return r

    for g in range(groups + warmup):
        sl, keep = slice(g * G, (g + 1) * G), g >= warmup
        timed("ocsort", lambda: oc.update_group(G, dets[sl], nd[sl], None, None, out, nout), keep)
        o = None
        if grids in ("on", "both"):
            o = timed("zone_update", lambda: zc.update_group_device(out, nout, G, zones.OUTPUTS), keep)
        if grids in ("off", "both"):
            timed("zone_update_no_grids", lambda: zt.update_group_device(out, nout, G, zones.OUTPUTS[:5] + ("heat_max",)), keep)
        if o is not None:
            timed("heat_blend", lambda: zc.blend(frames, o["heat_frames"][:, 0], o["heat_max"][:, 0].contiguous(), 128), keep)
        else:
            timed("heat_blend", lambda: zt.blend(frames, alpha=128), keep)          # the cumulative grid for every frame
        timed("copy", lambda: spare.copy_(frames), keep)
        rows.append(float(nout.float().mean()))
    oc.check_errors()
    tot = (zc if grids != "off" else zt).totals(0)
    med = {k: float(np.median(v)) * 1e3 for k, v in ms.items() if v}
    return {"mode": "kernel", "streams": S, "group_frames": G, "groups": groups, "frame": "1280x720", "rows_per_frame": float(np.mean(rows)),
            "crossings_stream0": int(tot["line_totals"].sum()), "entries_stream0": int(tot["entries"].sum()), "heat_max_stream0": int(tot["heat_max"]),
            "grids": grids, **{f"{k}_us_per_group_median": v for k, v in med.items()}, "heat_blend_over_copy": med["heat_blend"] / med["copy"], "frame_bytes_per_group": int(frames.numel()),
            "note": "host event pair around one call (includes launch latency); kernel times: rocprofv3 --kernel-trace --stats"}


def rates(n_frames, rounds):
    os.environ["SS_RANDOM_INIT"] = "1"
    from strongsort_yolo_amd import cli
    from strongsort_yolo_amd.yolo import YOLO
    legs = {"plain": {}, "line_zone": {"lines": [[320, 0, 320, 480], [0, 240, 640, 240]], "zones": [[[100, 100], [540, 100], [540, 380], [100, 380]]]}}
    legs["line_zone_heat"] = dict(legs["line_zone"], heatmap="box")
    fps = {k: [] for k in legs}
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="ocsort")
    with tempfile.TemporaryDirectory() as tmp:
        base = {"source": f"synthetic:{n_frames}", "track": True, "count": False, "tracker": "ocsort", "batch": 32, "random_init": True, "outdir": tmp}
        cli.process_video(dict(base, source="synthetic:64"), model=model)                  # warm-up: the pipeline and its kernels exist
        for r in range(rounds):
            for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
                torch.cuda.synchronize()
                t = time.perf_counter()
                out = cli.process_video(dict(base, **legs[leg]), model=model)
                torch.cuda.synchronize()
                fps[leg].append(out["frames"] / (time.perf_counter() - t))
    model.close()
    res = {"mode": "rates", "weights": "yolov8n (seeded random init)", "frame": "640x480", "frames": n_frames, "batch": 32, "rounds": rounds}
    for leg, v in fps.items():
        res[f"{leg}_frames_per_s_median"], res[f"{leg}_frames_per_s_all"] = float(np.median(v)), [round(x, 1) for x in v]
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("kernel", "rates"), default="kernel")
    p.add_argument("--streams", type=int, default=1)
    p.add_argument("--groups", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--frames", type=int, default=256)
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--grids", choices=("both", "on", "off"), default="both",
                   help="kernel: k_zone_update with the per-frame heat grids (heat_frames), without them (the blend then takes the cumulative grid), or both "
                        "on twin states; under rocprofv3 run one at a time, so that the kernel's rows in the stats are of one kind")
    a = p.parse_args()
    print(json.dumps(kernel(a.streams, a.groups, a.warmup, a.grids) if a.mode == "kernel" else rates(a.frames, a.rounds)))
