"""Timing of the BYTE tracker family (docs/BYTETRACK.md).  One JSON line per run on stdout.

  --mode kernel --streams S   k_byte_group alone: BASELINE configs[1]-like streams (1280x720, ~28 detections a frame, a share
                              of low scores, dropped sightings, false positives), 32-frame groups; wall time per call (events).
                              For the kernel's own time run it under `rocprofv3 --kernel-trace --stats -- python tools/byte_time.py ...`.
  --mode rates                YOLO.track() calls/s and track_stream frames/s, yolov8n (seeded random-init weights), bytetrack
                              mode beside the default StrongSORT (fp32 ReID) in the same process.
  --gmc                       BoT-SORT's camera-motion step (docs/BYTETRACK.md §1b).  kernel mode: two xywh engines on the same
                              streams, one with seeded synthetic warps installed (the GMC variant of k_byte_group) and one
                              without, called alternately; each group also runs ss_cmc_estimate on 32 panning 1280x720 frames
                              per stream (k_gray_small + k_ecc).  rates mode: botsort with and without camera_motion, one leg
                              per fresh process, the legs interleaved (--rounds each).
  --reid                      BoT-SORT's ReID branch (docs/BYTETRACK.md §1c).  kernel mode: two xywh engines on the same streams
                              with per-identity raw features (tests/test_gpu_botsort_reid.reid_stream), one with ReID (k_byte_feats +
                              the REID variant of k_byte_group) and one without, called alternately.  rates mode: botsort,
                              botsort with ReID and StrongSORT (fp32 ReID), one leg per fresh process, interleaved (--rounds each).
  --auto                      BoT-SORT's ReID with `model: auto` (docs/BYTETRACK.md §1d).  kernel mode: ss_native_feats alone on a
                              32-frame group of yolov8n head inputs at 1280x720 (f16 [32, 64|128|256, 48|24|12, 80|40|20],
                              --rows kept rows a frame); wall time per call (events), kernel time under rocprofv3.  rates mode:
                              botsort, botsort + OSNet fp32 ReID and botsort + `auto`, one leg per fresh process, interleaved.
  --pose                      BoT-SORT's keypoint term (docs/BYTETRACK.md §1e).  kernel mode: three xywh engines on the same seeded pose
                              streams (tests/test_botsort_pose_cpu.pose_stream), one with the term (k_byte_kpts + the POSE variant of
                              k_byte_group), one plain and one with ReID on seeded random features (the yardstick of the other opt-in
                              term), called alternately.  rates mode: yolo11n-pose with botsort and with botsort + with_pose, one leg
                              per fresh process, interleaved (--rounds each).
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


def _pan_frames(G, S, H=720, W=1280, seed=0):
    """G x S BGR frames cut from one seeded texture, panning 3 px right and 1 px down a frame ([F][S] order)."""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, ((H + 200) // 40, (W + 200) // 40, 3), dtype=np.uint8)
    canvas = np.repeat(np.repeat(small, 40, 0), 40, 1)          # 40 px blocks: 4 px in the 0.1x grey images ECC aligns
    out = np.zeros((G * S, H, W, 3), np.uint8)
    for f in range(G):
        for s in range(S):
            out[f * S + s] = canvas[f + 4 * s:f + 4 * s + H, 3 * f:3 * f + W]
    return out


def kernel_gmc(S, groups, warmup):
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
    rng = np.random.default_rng(7)                       # small seeded camera motions: tracks keep their detections
    th = rng.uniform(-2e-3, 2e-3, (n, S))
    w = np.zeros((n, S, 8))
    w[..., 0], w[..., 1], w[..., 3], w[..., 4] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    w[..., 2], w[..., 5], w[..., 6] = rng.uniform(-3, 3, (n, S)), rng.uniform(-3, 3, (n, S)), 5.0
    dets, nd, warps = torch.from_numpy(hd).to(dev), torch.from_numpy(hn).to(dev), torch.from_numpy(w).to(dev)
    frames = torch.from_numpy(_pan_frames(G, S)).to(dev)
    out = torch.zeros(G, S, 256, 8, device=dev)
    nout = torch.zeros(G, S, dtype=torch.int32, device=dev)
    cfg = ByteTrackConfig(kalman="xywh")
    plain, gmc = ByteTrackEngine(cfg, S, 0), ByteTrackEngine(cfg, S, 0)
    plain.use_current_stream()
    gmc.use_current_stream()
    ecc_warps = gmc.cmc_estimate(frames, G)              # sizes the small-frame buffer
    ms = {"plain": [], "gmc": [], "ecc": []}
    for g in range(groups + warmup):
        sl = slice(g * G, (g + 1) * G)
        gmc.set_cmc(warps[sl])
        for leg, fn in (("plain", lambda: plain.update_group(G, dets[sl], nd[sl], None, None, out, nout)),
                        ("gmc", lambda: gmc.update_group(G, dets[sl], nd[sl], None, None, out, nout)),
                        ("ecc", lambda: gmc.cmc_estimate(frames, G, ecc_warps))):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if g >= warmup:
                ms[leg].append(a.elapsed_time(b))
    plain.check_errors()
    gmc.check_errors()
    med = {k: float(np.median(v)) * 1e3 for k, v in ms.items()}
    return {"mode": "kernel_gmc", "streams": S, "group_frames": G, "groups": groups, "dets_per_frame": float(hn.mean()),
            "plain_us_per_group_median": med["plain"], "gmc_us_per_group_median": med["gmc"], "gmc_over_plain": med["gmc"] / med["plain"],
            "ecc_us_per_group_median": med["ecc"], "ecc_frame": "1280x720", "ecc_iterations_mean": float(ecc_warps[..., 6].float().mean()),
            "note": "host event pair around one call (includes launch latency); kernel times: rocprofv3 --kernel-trace --stats"}


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


def kernel_reid(S, groups, warmup):
    from strongsort_yolo_amd.config import ByteTrackConfig
    from strongsort_yolo_amd.engine import ByteTrackEngine
    from tests.test_gpu_botsort_reid import reid_stream
    G = 32
    n = (groups + warmup) * G
    streams = [reid_stream(100 + s, n) for s in range(S)]
    dev = torch.device("cuda", 0)
    hd, hn = np.zeros((n, S, 128, 6), np.float32), np.zeros((n, S), np.int32)
    hf = np.zeros((n, S, 128, 512), np.float32)
    for f in range(n):
        for s in range(S):
            d, ft = streams[s][f]
            hd[f, s, :len(d)], hf[f, s, :len(d)], hn[f, s] = d, ft, len(d)
    dets, nd, feats = torch.from_numpy(hd).to(dev), torch.from_numpy(hn).to(dev), torch.from_numpy(hf).to(dev)
    out = torch.zeros(G, S, 256, 8, device=dev)
    nout = torch.zeros(G, S, dtype=torch.int32, device=dev)
    plain = ByteTrackEngine(ByteTrackConfig(kalman="xywh"), S, 0)
    reid = ByteTrackEngine(ByteTrackConfig(kalman="xywh", with_reid=True), S, 0)
    plain.use_current_stream()
    reid.use_current_stream()
    ms = {"plain": [], "reid": []}
    for g in range(groups + warmup):
        sl = slice(g * G, (g + 1) * G)
        for leg, eng in (("plain", plain), ("reid", reid)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.update_group(G, dets[sl], nd[sl], feats[sl], None, out, nout)
            b.record()
            b.synchronize()
            if g >= warmup:
                ms[leg].append(a.elapsed_time(b))
    plain.check_errors()
    reid.check_errors()
    med = {k: float(np.median(v)) * 1e3 for k, v in ms.items()}
    return {"mode": "kernel_reid", "streams": S, "group_frames": G, "groups": groups, "dets_per_frame": float(hn.mean()),
            "plain_us_per_group_median": med["plain"], "reid_us_per_group_median": med["reid"], "reid_over_plain": med["reid"] / med["plain"],
            "note": "host event pair around one call (reid: k_byte_feats + k_byte_group, includes launch latency); kernel times: "
                    "rocprofv3 --kernel-trace --stats"}


def kernel_pose(S, groups, warmup):
    from strongsort_yolo_amd.config import ByteTrackConfig
    from strongsort_yolo_amd.engine import ByteTrackEngine
    from tests.test_botsort_pose_cpu import K, pose_stream
    G = 32
    n = (groups + warmup) * G
    streams = [pose_stream(100 + s, n) for s in range(S)]
    dev = torch.device("cuda", 0)
    hd, hn, hk = np.zeros((n, S, 128, 6), np.float32), np.zeros((n, S), np.int32), np.zeros((n, S, 128, K, 3), np.float32)
    for f in range(n):
        for s in range(S):
            d, kp = streams[s][f]
            hd[f, s, :len(d)], hk[f, s, :len(d)], hn[f, s] = d, kp, len(d)
    dets, nd, kpts = torch.from_numpy(hd).to(dev), torch.from_numpy(hn).to(dev), torch.from_numpy(hk).to(dev)
    feats = torch.randn(G, S, 128, 512, generator=torch.Generator().manual_seed(0)).to(dev)
    out = torch.zeros(G, S, 256, 8, device=dev)
    nout = torch.zeros(G, S, dtype=torch.int32, device=dev)
    engs = {"plain": ByteTrackEngine(ByteTrackConfig(kalman="xywh"), S, 0), "pose": ByteTrackEngine(ByteTrackConfig(kalman="xywh", with_pose=True), S, 0),
            "reid": ByteTrackEngine(ByteTrackConfig(kalman="xywh", with_reid=True), S, 0)}
    ms = {k: [] for k in engs}
    for e in engs.values():
        e.use_current_stream()
    for g in range(groups + warmup):
        sl = slice(g * G, (g + 1) * G)
        for leg, eng in engs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.update_group(G, dets[sl], nd[sl], feats, None, out, nout, kpts=kpts[sl])
            b.record()
            b.synchronize()
            if g >= warmup:
                ms[leg].append(a.elapsed_time(b))
    for e in engs.values():
        e.check_errors()
    med = {k: float(np.median(v)) * 1e3 for k, v in ms.items()}
    return {"mode": "kernel_pose", "streams": S, "group_frames": G, "groups": groups, "dets_per_frame": float(hn.mean()),
            "plain_us_per_group_median": med["plain"], "pose_us_per_group_median": med["pose"], "reid_us_per_group_median": med["reid"],
            "pose_over_plain": med["pose"] / med["plain"], "reid_over_plain": med["reid"] / med["plain"],
            "note": "host event pair around one call (pose: k_byte_kpts + k_byte_group, reid: k_byte_feats + k_byte_group, includes launch "
                    "latency); kernel times: rocprofv3 --kernel-trace --stats"}


def kernel_auto(groups, warmup, rows):
    from strongsort_yolo_amd.engine import TrackerEngine
    dev = torch.device("cuda", 0)
    eng = TrackerEngine(n_streams=1)
    g = torch.Generator().manual_seed(0)
    shapes = ((64, 48, 80), (128, 24, 40), (256, 12, 20))
    maps = [torch.randn(32, c, h, w, generator=g).half().to(dev).contiguous(memory_format=torch.channels_last) for c, h, w in shapes]
    A = sum(h * w for _, h, w in shapes)
    keep = torch.randint(0, A, (32, 128), generator=g, dtype=torch.int32).to(dev)
    cnt = torch.full((32,), rows, dtype=torch.int32, device=dev)
    out = torch.zeros(32, 128, 512, device=dev)
    ms = []
    for k in range(groups + warmup):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.native_feats(maps, keep, cnt, out)
        b.record()
        b.synchronize()
        if k >= warmup:
            ms.append(a.elapsed_time(b))
    eng.check_errors()
    eng.close()
    return {"mode": "kernel_auto", "group_frames": 32, "rows_per_frame": rows, "groups": groups, "us_per_group_median": float(np.median(ms)) * 1e3,
            "note": "host event pair around one ss_native_feats call (includes launch latency); kernel time: rocprofv3 --kernel-trace --stats"}


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


def rate_leg(leg, n_frames, batch):
    """One leg in this process: botsort with (leg "botsort_cmc") or without camera_motion, botsort with ReID ("botsort_reid": OSNet
    fp32, "botsort_auto": `model: auto`), StrongSORT with fp32 ReID ("strongsort"), yolo11n-pose with botsort ("pose_botsort") and with
    the keypoint term ("pose_botsort_pose"); 1280x720 frames panning 3 px a frame."""
    os.environ["SS_RANDOM_INIT"] = "1"
    from strongsort_yolo_amd.yolo import YOLO
    pan = _pan_frames(16, 1)
    frames = [pan[k].copy() for k in range(16)]
    frames += frames[::-1]                                  # back and forth: the sequence can repeat without a jump
    if leg == "strongsort":
        m = YOLO("yolov8n.pt", random_init_ok=True)
    elif leg in ("pose_botsort", "pose_botsort_pose"):      # the pose model under both legs: only the term differs
        m = YOLO("yolo11n-pose.pt", random_init_ok=True, tracker_type="botsort", with_pose=leg == "pose_botsort_pose")
    else:
        m = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", camera_motion=leg == "botsort_cmc",
                 with_reid=leg in ("botsort_reid", "botsort_auto"), reid_model="auto" if leg == "botsort_auto" else "osnet")
    for k in range(10):
        m.track(frames[k % 32], persist=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for k in range(n_frames):
        m.track(frames[k % 32], persist=True)
    res = {"leg": leg, "track_calls_per_s": n_frames / (time.perf_counter() - t)}
    src = [frames[k % 32] for k in range(n_frames)]
    for _ in m.track_stream(src[:2 * batch], batch=batch):
        pass
    t = time.perf_counter()
    for _ in m.track_stream(src, batch=batch):
        pass
    res["track_stream_frames_per_s"] = n_frames / (time.perf_counter() - t)
    m.close()
    return res


def rates_legs(n_frames, batch, rounds, names, mode):
    import subprocess
    legs = {k: [] for k in names}
    for r in range(rounds):
        for leg in (names if r % 2 == 0 else names[::-1]):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", "rates", "--leg", leg, "--frames", str(n_frames),
                                "--batch", str(batch)], capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise RuntimeError(f"leg {leg} failed ({p.returncode}): {p.stderr[-2000:]}")
            legs[leg].append(json.loads(p.stdout.strip().splitlines()[-1]))
    res = {"mode": mode, "weights": ("yolo11n-pose" if mode == "rates_pose" else "yolov8n") + " (seeded random init)", "frame": "1280x720", "batch": batch, "rounds": rounds}
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
    p.add_argument("--gmc", action="store_true", help="BoT-SORT GMC legs (see the module docstring)")
    p.add_argument("--rounds", type=int, default=3, help="rates --gmc: processes per leg")
    p.add_argument("--reid", action="store_true", help="BoT-SORT ReID legs (see the module docstring)")
    p.add_argument("--auto", action="store_true", help="BoT-SORT ReID with model: auto (see the module docstring)")
    p.add_argument("--rows", type=int, default=28, help="kernel --auto: kept rows a frame")
    p.add_argument("--pose", action="store_true", help="BoT-SORT keypoint-term legs (see the module docstring)")
    p.add_argument("--leg", choices=("botsort", "botsort_cmc", "botsort_reid", "botsort_auto", "strongsort", "pose_botsort", "pose_botsort_pose"), default=None, help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.leg is not None:
        r = rate_leg(a.leg, a.frames, a.batch)
    elif a.mode == "kernel":
        r = kernel_pose(a.streams, a.groups, a.warmup) if a.pose else kernel_auto(a.groups, a.warmup, a.rows) if a.auto else kernel_reid(a.streams, a.groups, a.warmup) if a.reid else kernel_gmc(a.streams, a.groups, a.warmup) if a.gmc else kernel(a.streams, a.groups, a.warmup)
    elif a.pose:
        r = rates_legs(a.frames, a.batch, a.rounds, ("pose_botsort", "pose_botsort_pose"), "rates_pose")
    elif a.auto:
        r = rates_legs(a.frames, a.batch, a.rounds, ("botsort", "botsort_reid", "botsort_auto"), "rates_auto")
    elif a.reid:
        r = rates_legs(a.frames, a.batch, a.rounds, ("botsort", "botsort_reid", "strongsort"), "rates_reid")
    elif a.gmc:
        r = rates_legs(a.frames, a.batch, a.rounds, ("botsort", "botsort_cmc"), "rates_gmc")
    else:
        r = rates(a.frames, a.batch)
    print(json.dumps(r))
