"""Timing of the Deep OC-SORT tracker (docs/DEEPOCSORT.md §6), in tools/ocsort_time.py's style.  One JSON line per run on stdout.

  --mode all (default)        both measurements below in one run: the kernel leg as a child process under
                              `rocprofv3 --kernel-trace --stats` (a run of its own, no counters in it), its kernel statistics copied to
                              --stats-out, then the rate legs.
  --mode kernel --streams S   k_deepoc_group (and its pre-pass k_deepoc_feats) beside k_ocsort_group on the same rows in the same run:
                              tests/deepocsort_scenes.deep_stream (1280x720, ~25 rows a frame, identity features, dropped sightings,
                              false positives, a moving camera's warps for Deep OC-SORT), 32-frame groups, the two engines called
                              alternately; wall time per call (events).  --no-warps: Deep OC-SORT without the warps.
  --mode fill                 the rate legs' set-up looked into: 96 track() calls per tracker (deep_ocsort, botsort with with_reid, ocsort),
                              the rows a frame and the tracks in the table, then the tracker call alone on 32 copies of the last frame's
                              rows and features (host event pairs, ms per 32-frame group).
  --mode rates                track_stream frames/s (and track() calls/s) of yolov8n (seeded random-init weights) with deep_ocsort
                              beside botsort with with_reid: one leg per fresh process, the legs interleaved (--rounds each, default 2).
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

LEGS = ("botsort_reid", "deep_ocsort")


def kernel(S, groups, warmup, warps_on):
    from strongsort_yolo_amd.config import DeepOCSortConfig, OCSortConfig
    from strongsort_yolo_amd.engine import DeepOCSortEngine, OCSortEngine
    from tests.deepocsort_scenes import deep_stream
    G = 32
    n = (groups + warmup) * G
    streams = [deep_stream(100 + s, n) for s in range(S)]
    dev = torch.device("cuda", 0)
    hd, hn = np.zeros((n, S, 128, 6), np.float32), np.zeros((n, S), np.int32)
    hf, hw = np.zeros((n, S, 128, 512), np.float32), np.zeros((n, S, 8))
    for s, (frames, feats, warps) in enumerate(streams):
        hw[:, s] = warps
        for f in range(n):
            d = frames[f]
            hd[f, s, :len(d)], hn[f, s], hf[f, s, :len(d)] = d, len(d), feats[f]
    if not warps_on:
        hw[:, :, 6] = -1.0
    dets, nd, ft, wp = (torch.from_numpy(a).to(dev) for a in (hd, hn, hf, hw))
    out = torch.zeros(G, S, 256, 8, device=dev)
    nout = torch.zeros(G, S, dtype=torch.int32, device=dev)
    engs = {"ocsort": OCSortEngine(OCSortConfig(), S, 0), "deepoc": DeepOCSortEngine(DeepOCSortConfig(), S, 0)}
    ms, tracks = {k: [] for k in engs}, []
    for e in engs.values():
        e.use_current_stream()
    for g in range(groups + warmup):
        sl = slice(g * G, (g + 1) * G)
        for leg, eng in engs.items():
            if leg == "deepoc":
                eng.set_cmc(wp[sl])
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.update_group(G, dets[sl], nd[sl], ft[sl] if leg == "deepoc" else None, None, out, nout)
            b.record()
            b.synchronize()
            if g >= warmup:
                ms[leg].append(a.elapsed_time(b))
        tracks.append(engs["deepoc"].tracks(0)["n_tracks"])
    for e in engs.values():
        e.check_errors()
    med = {k: float(np.median(v)) * 1e3 for k, v in ms.items()}
    return {"mode": "kernel", "streams": S, "group_frames": G, "groups": groups, "warps": bool(warps_on), "dets_per_frame": float(hn.mean()),
            "deepoc_tracks_stream0_mean": float(np.mean(tracks)),
            "ocsort_us_per_group_median": med["ocsort"], "deepoc_us_per_group_median": med["deepoc"], "deepoc_over_ocsort": med["deepoc"] / med["ocsort"],
            "deepoc_us_per_frame_per_stream": med["deepoc"] / G,
            "note": "host event pair around one call (two launches for deepoc, includes launch latency); kernel times: rocprofv3 --kernel-trace --stats"}


def rate_leg(leg, n_frames, batch):
    """One leg in this process: yolov8n with the leg's tracker on 1280x720 synthetic frames."""
    os.environ["SS_RANDOM_INIT"] = "1"
    from strongsort_yolo_amd.synth import make_stream
    from strongsort_yolo_amd.yolo import YOLO
    st = make_stream(0, 1280, 720, 28)
    frames = [st.frame_pixels(k).copy() for k in range(8)]
    kw = dict(tracker_type="botsort", with_reid=True) if leg == "botsort_reid" else dict(tracker_type="deep_ocsort")
    m = YOLO("yolov8n.pt", random_init_ok=True, **kw)
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
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"leg {leg} failed ({p.returncode}): {p.stderr[-2000:]}")
            legs[leg].append(json.loads(p.stdout.strip().splitlines()[-1]))
    res = {"mode": "rates", "weights": "yolov8n, OSNet-x0.25 (seeded random init)", "frame": "1280x720", "batch": batch, "rounds": rounds}
    for leg, rs in legs.items():
        for k in ("track_calls_per_s", "track_stream_frames_per_s"):
            res[f"{leg}_{k}_median"] = float(np.median([r[k] for r in rs]))
            res[f"{leg}_{k}_all"] = [round(r[k], 1) for r in rs]
    return res


def fill():
    from strongsort_yolo_amd.synth import make_stream
    from strongsort_yolo_amd.yolo import YOLO
    st = make_stream(0, 1280, 720, 28)
    frames = [st.frame_pixels(k).copy() for k in range(8)]
    res = []
    for kw in (dict(tracker_type="deep_ocsort"), dict(tracker_type="botsort", with_reid=True), dict(tracker_type="ocsort")):
        m = YOLO("yolov8n.pt", random_init_ok=True, **kw)
        nd, nt = [], []
        for k in range(96):
            m.track(frames[k % 8], persist=True)
            p = m._pipe
            nd.append(int(p.ndets[0]))
            t = p.trk.tracks(0)
            nt.append(t["n_tracks"] if "n_tracks" in t else t["n_tracked"] + t["n_lost"])
        e, G = p.trk, 32
        d, n, f = p.b.dets6[:1].repeat(G, 1, 1).contiguous(), p.b.ndets[:1].repeat(G).contiguous(), p.b.feats_v[:1].repeat(G, 1, 1).contiguous()
        out, no = torch.zeros(G, 1, 256, 8, device=d.device), torch.zeros(G, 1, dtype=torch.int32, device=d.device)
        ms = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            e.update_group(G, d, n, f, None, out, no)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        res.append({"kw": kw, "rows_mean": float(np.mean(nd[32:])), "tracks_last": nt[-1], "tracks_mean_after_32": float(np.mean(nt[32:])),
                    "group_ms": [round(x, 2) for x in ms]})
        m.close()
    return {"mode": "fill", "legs": res}


def traced_kernel(S, groups, warmup, stats_out):
    """The kernel leg in a child process under the profiler's kernel trace (no counters); -> its JSON line and the kernels' rows."""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "--mode", "kernel", "--streams", str(S), "--groups", str(groups), "--warmup", str(warmup)],
                           capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise RuntimeError(f"traced kernel leg failed ({p.returncode}): {p.stderr[-2000:]}")
        line = json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise RuntimeError("the profiler wrote no kernel statistics")
        with open(found[0], newline="") as f:
            rows = [r for r in csv.DictReader(f) if any(k in r["Name"] for k in ("k_deepoc_group", "k_deepoc_feats", "k_ocsort_group"))]
        if stats_out:
            os.makedirs(os.path.dirname(os.path.abspath(stats_out)), exist_ok=True)
            shutil.copy(found[0], stats_out)
    line["kernel_trace"] = {r["Name"].split("(")[0]: {"calls": int(r["Calls"]), "mean_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                                                       "max_us": float(r["MaxNs"]) / 1e3} for r in rows}
    return line


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("all", "kernel", "rates", "fill"), default="all")
    p.add_argument("--streams", type=int, default=8)
    p.add_argument("--groups", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--frames", type=int, default=256)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--rounds", type=int, default=2, help="rates: processes per leg")
    p.add_argument("--no-warps", action="store_true", help="kernel: Deep OC-SORT without the camera's warps")
    p.add_argument("--stats-out", default=None, help="all: where the profiler's kernel statistics (CSV) are copied")
    p.add_argument("--leg", choices=LEGS, default=None, help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.leg is not None:
        print(json.dumps(rate_leg(a.leg, a.frames, a.batch)))
    elif a.mode == "kernel":
        print(json.dumps(kernel(a.streams, a.groups, a.warmup, not a.no_warps)))
    elif a.mode == "rates":
        print(json.dumps(rates(a.frames, a.batch, a.rounds)))
    elif a.mode == "fill":
        print(json.dumps(fill()))
    else:
        print(json.dumps(traced_kernel(a.streams, a.groups, a.warmup, a.stats_out)), flush=True)
        print(json.dumps(rates(a.frames, a.batch, a.rounds)))
