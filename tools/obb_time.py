"""Timing of the rotated NMS beside the axis-aligned one (docs/OBB.md §6), in tools/slice_time.py's style.  One JSON line on stdout.

  --mode kernel   32 resident head tensors [4 + 15 + 1][8400] (a 640 x 640 input), the same tensors for both legs, --cand candidates per
                  image in clusters of six near-copies.  Legs, each between an event pair (wall time per call, launch latency included):
                    nms       ss_nms_batch      (k_nms_filter + k_nms_rest; theta travels as one extra column)
                    nms_obb   ss_nms_obb_batch  (k_nms_filter + k_nms_obb_rest)
                    byte      ss_byte_update_group      (k_byte_group, xyah) on the envelopes of a 32-frame scene of 24 turning boxes
                    byte_obb  ss_byte_update_group_obb  (k_byte_group's OBB variant) on the same scene's rotated boxes
                  For the kernels' own times run it under `rocprofv3 --kernel-trace --stats -- python tools/obb_time.py --mode kernel`.
  --mode stream   YOLO.track_stream(batch=32) frames/s of yolov8n-obb against yolov8n, ByteTrack, synthetic heads filled from the same
                  scene (the networks run, their heads are replaced), 480 x 640 frames, the two legs alternating --rounds times.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

G, A, NC = 32, 8400, 15


def field(n_cand, rng):
    """[4 + NC + 1][A]: n_cand anchors above the threshold, clusters of six jittered copies of an elongated box, every third turned by pi/2"""
    pred = np.zeros((4 + NC + 1, A), np.float32)
    pred[4:4 + NC] = rng.uniform(0.0, 0.2, (NC, A))
    pred[:2], pred[2:4] = rng.uniform(0, 640, (2, A)), rng.uniform(10, 60, (2, A))
    anchors = rng.permutation(A)[:n_cand]
    ncl = (n_cand + 5) // 6
    ctr, wh = rng.uniform(40, 600, (ncl, 2)), np.stack([rng.uniform(60, 140, ncl), rng.uniform(8, 30, ncl)], 1)
    th, kc = rng.uniform(-np.pi / 4, np.pi / 4, ncl), rng.integers(0, NC, ncl)
    for q, a in enumerate(anchors):
        c = q // 6
        pred[:2, a], pred[2:4, a] = ctr[c] + rng.uniform(-3, 3, 2), wh[c] * rng.uniform(0.9, 1.1, 2)
        pred[4 + NC, a] = th[c] + rng.uniform(-0.08, 0.08) + (np.pi / 2 if q % 3 == 2 else 0.0)
        pred[4 + kc[c], a] = rng.uniform(0.3, 0.95)
    return pred


def scene(frames, n=24, hw=(480, 640)):
    """frames x [n, 11] rows (ss_nms_obb_batch's layout): elongated boxes that drift and turn inside the frame"""
    sys.path.insert(0, ROOT)
    from tests import obb_ref as R
    rng = np.random.default_rng(3)
    x0, y0 = rng.uniform(60, hw[1] - 60, n), rng.uniform(40, hw[0] - 40, n)
    vx, vy, th0, om = rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(0, np.pi, n), rng.uniform(-0.05, 0.05, n)
    out = []
    for f in range(frames):
        # the centres bounce between the margins: a box that left the frame would have an empty clipped envelope
        x, y = 60 + np.abs((x0 - 60 + vx * f) % (2 * (hw[1] - 120)) - (hw[1] - 120)), 40 + np.abs((y0 - 40 + vy * f) % (2 * (hw[0] - 80)) - (hw[0] - 80))
        b = np.stack([x, y, np.full(n, 60.0), np.full(n, 12.0), (th0 + om * f) % np.pi], 1).astype(np.float32)
        out.append(R.obb_rows(R.regularise(b), rng.uniform(0.3, 0.95, n).astype(np.float32), np.zeros(n, np.float32), hw[1], hw[0]))
    return out


def tracker_legs(dev):
    """the plain and the OBB group entry on the same 32-frame scene -> {name: callable} (each call restarts its stream first)"""
    from strongsort_yolo_amd.config import ByteTrackConfig
    from strongsort_yolo_amd.engine import ByteTrackEngine
    rows = np.stack(scene(32))                                          # [32, 24, 11]
    n = rows.shape[1]
    legs = {}
    for name, obb in (("byte", False), ("byte_obb", True)):
        eng = ByteTrackEngine(ByteTrackConfig(), 1, 0, obb=obb)
        ld = 11 if obb else 6
        d = torch.zeros(32, 1, 128, ld, device=dev)
        d[:, 0, :n] = torch.from_numpy(rows[:, :, :ld]).to(dev)
        nd = torch.full((32, 1), n, dtype=torch.int32, device=dev)
        out, nout = torch.zeros(32, 1, 256, 8, device=dev), torch.zeros(32, 1, dtype=torch.int32, device=dev)
        rb = torch.zeros(32, 1, 256, 5, device=dev)

        def call(eng=eng, d=d, nd=nd, out=out, nout=nout, rb=rb, obb=obb):
            eng.update_group(32, d, nd, None, None, out, nout, **({"rbox": rb} if obb else {}))
        legs[name] = (call, eng)
    return legs


def stream(rounds, frames=128):
    from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry
    from strongsort_yolo_amd.yolo import YOLO
    import time
    import warnings
    warnings.simplefilter("ignore")
    dev, hw = torch.device("cuda", 0), (480, 640)
    g = letterbox_geometry(*hw)
    gain, px, py = scale_geometry(g, *hw)
    A = sum((g.out_h // s) * (g.out_w // s) for s in (8, 16, 32))
    rows = scene(frames, hw=hw)
    imgs = [np.zeros(hw + (3,), np.uint8) for _ in range(frames)]
    models = {}
    for name, nc, obb in (("yolov8n", 80, False), ("yolov8n-obb", 15, True)):
        pred = np.zeros((frames, 4 + nc + (1 if obb else 0), A), np.float32)
        for k, r in enumerate(rows):
            n = len(r)
            if obb:
                b = r[:, 6:10] * np.float32(gain)
                pred[k, 4 + nc, :n] = r[:, 10]
            else:                                                        # the envelopes as xywh
                b = np.stack([(r[:, 0] + r[:, 2]) / 2, (r[:, 1] + r[:, 3]) / 2, r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]], 1) * np.float32(gain)
            b[:, 0] += np.float32(px)
            b[:, 1] += np.float32(py)
            pred[k, :4, :n], pred[k, 4, :n] = b.T, r[:, 4]
        m = YOLO(name + ".pt", tracker_type="bytetrack", random_init_ok=True)
        m._pipe_kw.update(det_source="synthetic")
        dp = torch.from_numpy(pred).to(dev)
        m._fill = lambda b, v, k, dp=dp: b.pred_in[v].copy_(dp[k % frames])
        models[name] = m
    fps, tracks = {k: [] for k in models}, {}
    for r in range(rounds + 1):                                          # round 0 builds and captures: not counted
        for name, m in models.items():
            m._frame_index = 0
            if m._stream_pipe is not None:
                m._stream_pipe.reset_tracker(-1)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res = list(m.track_stream(imgs, batch=32))
            dt = time.perf_counter() - t0
            tracks[name] = float(np.mean([len(x[0]) for x in res]))
            if r:
                fps[name].append(frames / dt)
    out = {"mode": "stream", "frames": frames, "frame_hw": list(hw), "batch": 32, "tracker": "bytetrack", "rounds": rounds,
           **{f"{k}_fps_median": float(np.median(v)) for k, v in fps.items()}, **{f"{k}_tracks_per_frame": v for k, v in tracks.items()},
           "obb_over_plain": float(np.median(fps["yolov8n-obb"]) / np.median(fps["yolov8n"])),
           "note": "host wall time of the whole generator, uploads and result hand-over included; legs alternate"}
    for m in models.values():
        m.close()
    return out


def kernel(rounds, warmup, cand):
    from strongsort_yolo_amd.config import DetectConfig
    from strongsort_yolo_amd.engine import TrackerEngine
    dev = torch.device("cuda", 0)
    eng, dcfg, rng = TrackerEngine(None, 1, 0), DetectConfig(), np.random.default_rng(0)
    d_pred = torch.from_numpy(np.stack([field(cand, rng) for _ in range(G)])).to(dev)
    geom = torch.tensor([[1.0, 0.0, 0.0, 640.0, 640.0]] * G, dtype=torch.float32, device=dev)
    R = 300
    rows7, rows11 = torch.zeros(G, R, 7, device=dev), torch.zeros(G, R, 11, device=dev)
    keep, cnt, cnt_obb = torch.zeros(G, R, dtype=torch.int32, device=dev), torch.zeros(G, dtype=torch.int32, device=dev), torch.zeros(G, dtype=torch.int32, device=dev)
    legs = {"nms": lambda: eng.nms_batch(d_pred, NC, dcfg, geom, n_extra=1, rows=rows7, keep=keep, count=cnt, max_det=R),
            "nms_obb": lambda: eng.nms_obb_batch(d_pred, NC, dcfg, geom, rows=rows11, keep=keep, count=cnt_obb, max_det=R)}
    trk = tracker_legs(dev)
    for k, (fn, _) in trk.items():
        legs[k] = fn
    ms = {k: [] for k in legs}
    for r in range(rounds + warmup):
        for k, fn in legs.items():
            if k in trk:
                trk[k][1].reset()                                        # synchronous, outside the event pair
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                ms[k].append(a.elapsed_time(b))
    eng.check_errors()
    med = {k: float(np.median(v)) * 1e3 for k, v in ms.items()}
    res = {"mode": "kernel", "images": G, "anchors": A, "nc": NC, "candidates_per_image": cand, "kept_rows_per_image": float(cnt.float().mean()),
           "kept_rows_per_image_obb": float(cnt_obb.float().mean()), **{f"{k}_us_median": v for k, v in med.items()},
           "nms_obb_over_nms": med["nms_obb"] / med["nms"], "byte_obb_over_byte": med["byte_obb"] / med["byte"],
           "byte_scene": "32 frames x 24 rows, one stream, one call", "rounds": rounds,
           "note": "host event pair around one call (includes launch latency); kernel times: rocprofv3 --kernel-trace --stats"}
    for _, e in trk.values():
        e.check_errors()
        e.close()
    eng.close()
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("kernel", "stream"), default="kernel")
    p.add_argument("--rounds", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--cand", type=int, default=60)
    a = p.parse_args()
    print(json.dumps(kernel(a.rounds, a.warmup, a.cand) if a.mode == "kernel" else stream(a.rounds)))
