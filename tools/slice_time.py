"""Timing of sliced inference (docs/SLICE.md §7), in tools/zones_time.py's style.  One JSON line per run on stdout.

  --mode kernel   32 resident 1280x720 frames, slice 640x640, overlap 0.2, the full frame: T = 7, f16 channels-last output.
                  Legs, each between an event pair (wall time per call, launch latency included):
                    slice_letterbox   k_slice_letterbox, one launch
                    letterbox_x7      T launches of the existing k_letterbox on offset pointers into the same frames (tile-major output)
                    copy              a device-to-device copy of the output's bytes
                    nms               ss_nms_batch (k_nms_filter + k_nms_rest) on the 32 x T synthetic head tensors
                    slice_merge       k_slice_merge on that call's rows
                  For the kernels' own times run it under `rocprofv3 --kernel-trace --stats -- python tools/slice_time.py --mode kernel`.
  --mode rates    track_stream (yolov8n, seeded random-init weights, ByteTrack, batch 32) on 1280x720 frames: frames/s without slicing
                  and with slice_hw=(640, 640), the legs alternating in one process (--rounds each).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HW, SLICE, OVERLAP, G = (720, 1280), (640, 640), 0.2, 32


def tile_heads(dets, table, tg, A, rng):
    """[T, 84, A] head tensors of one frame: every tile sees the scene's boxes it holds, clipped to it (tile pixels)."""
    from strongsort_yolo_amd.synth import synth_prediction
    out = np.zeros((len(table), 84, A), np.float32)
    for t, (x0, y0, tw, th) in enumerate(table[:, :4].tolist()):
        b = dets.copy()
        b[:, [0, 2]] = np.clip(b[:, [0, 2]] - x0, 0, tw)
        b[:, [1, 3]] = np.clip(b[:, [1, 3]] - y0, 0, th)
        b = b[((b[:, 2] - b[:, 0]) >= 8) & ((b[:, 3] - b[:, 1]) >= 8)]
        out[t], _ = synth_prediction(b, A, 80, float(tg[t, 0]), (float(tg[t, 1]), float(tg[t, 2])), rng)
    return out


def kernel(rounds, warmup, objects):
    from strongsort_yolo_amd import lib, slicing
    from strongsort_yolo_amd.config import DetectConfig
    from strongsort_yolo_amd.engine import TrackerEngine
    from strongsort_yolo_amd.synth import make_stream
    H, W = HW
    dev = torch.device("cuda", 0)
    eng = TrackerEngine(None, 1, 0)
    cfg = slicing.SliceConfig(SLICE, OVERLAP, True)
    g, table = slicing.canvas(H, W, cfg)
    T, R, dcfg = len(table), 128, DetectConfig()
    tg = slicing.nms_geometry(g, table)
    eng.slice_config(table, HW, (g.out_h, g.out_w), R)
    frames = torch.randint(0, 256, (G, H, W, 3), dtype=torch.uint8, device=dev)
    lb = torch.empty(G * T, 3, g.out_h, g.out_w, dtype=torch.float16, device=dev).contiguous(memory_format=torch.channels_last)
    lb2, spare = torch.empty_like(lb), torch.empty_like(lb)
    # the tiles' head tensors: a scene per frame, every tile sees the boxes it holds
    A = sum((g.out_h // s) * (g.out_w // s) for s in (8, 16, 32))
    rng = np.random.default_rng(0)
    st = make_stream(1, W, H, objects)
    pred = np.concatenate([tile_heads(st.next_frame().dets, table, tg, A, rng) for _ in range(G)])
    d_pred = torch.from_numpy(pred).to(dev)
    geom = eng.slice_nms_geom(G)
    rows, keep = torch.zeros(G * T, R, 6, device=dev), torch.zeros(G * T, R, dtype=torch.int32, device=dev)
    cnt = torch.zeros(G * T, dtype=torch.int32, device=dev)
    out, ocnt, osrc = torch.zeros(G, R, 6, device=dev), torch.zeros(G, dtype=torch.int32, device=dev), torch.zeros(G, R, dtype=torch.int32, device=dev)
    per = 3 * g.out_h * g.out_w * 2

    def letterbox_x7():
        for t, (x0, y0, tw, th, nw, nh, pl, pt) in enumerate(table.tolist()):
            src = frames.data_ptr() + y0 * frames.stride(1) + x0 * 3
            eng._ck(eng.L.ss_letterbox_batch(eng.ctx, C.c_void_p(src), G, frames.stride(0), th, tw, frames.stride(1), C.c_void_p(lb2.data_ptr() + t * G * per),
                                             lib.DST_F16 | lib.DST_HWC, g.out_h, g.out_w, nh, nw, pt, pl, 114))

    legs = {"slice_letterbox": lambda: eng.slice_letterbox_batch(frames, half=True, out=lb, channels_last=True), "letterbox_x7": letterbox_x7,
            "copy": lambda: spare.copy_(lb),
            "nms": lambda: eng.nms_batch(d_pred, 80, dcfg, geom, rows=rows, keep=keep, count=cnt, max_det=R),
            "slice_merge": lambda: eng.slice_merge(rows.view(G, T, R, 6), cnt.view(G, T), "nmm", "ios", 0.5, False, R, out, ocnt, osrc)}
    ms = {k: [] for k in legs}
    for r in range(rounds + warmup):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                ms[k].append(a.elapsed_time(b))
    eng.check_errors()
    same = bool(torch.equal(lb.permute(0, 2, 3, 1).reshape(G, T, -1), lb2.permute(0, 2, 3, 1).reshape(T, G, -1).transpose(0, 1)))
    med = {k: float(np.median(v)) * 1e3 for k, v in ms.items()}
    res = {"mode": "kernel", "frames": G, "frame": "1280x720", "tiles": T, "canvas": f"{g.out_w}x{g.out_h}", "output_bytes": int(lb.numel() * 2),
           "letterbox_equal": same, "tile_rows_per_frame": float(cnt.float().sum() / G), "merged_rows_per_frame": float(ocnt.float().mean()),
           **{f"{k}_us_median": v for k, v in med.items()}, "slice_letterbox_over_x7": med["slice_letterbox"] / med["letterbox_x7"],
           "slice_letterbox_over_copy": med["slice_letterbox"] / med["copy"], "rounds": rounds,
           "note": "host event pair around one call (includes launch latency); kernel times: rocprofv3 --kernel-trace --stats"}
    eng.close()
    return res


def rates(n_frames, rounds):
    # The networks run on seeded random-init weights (their load is real, their scores are not: every anchor of a 640 x 640 canvas would
    # pass the threshold), so the NMS reads synthetic head tensors of a 30-object scene, the same scene in both legs, 32 frames in a cycle.
    from strongsort_yolo_amd import slicing
    from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry
    from strongsort_yolo_amd.synth import make_stream, synth_prediction
    from strongsort_yolo_amd.yolo import YOLO
    H, W = HW
    dev = torch.device("cuda", 0)
    st, rng = make_stream(3, W, H, 30), np.random.default_rng(3)
    frames, dets = [], []
    for k in range(n_frames):
        d = st.next_frame().dets
        if k < G:
            dets.append(d)
        frames.append(st.frame_pixels(k).copy())
    models = {"plain": YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack"),
              "sliced": YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack", slice_hw=SLICE, slice_overlap=OVERLAP)}
    anchors = lambda g: sum((g.out_h // s) * (g.out_w // s) for s in (8, 16, 32))
    gp = letterbox_geometry(H, W)
    sp = scale_geometry(gp, H, W)
    gc, table = slicing.canvas(H, W, models["sliced"].slice)
    tg = slicing.nms_geometry(gc, table)
    heads = {"plain": torch.from_numpy(np.stack([synth_prediction(d, anchors(gp), 80, sp[0], (sp[1], sp[2]), rng)[0][None] for d in dets])).to(dev),
             "sliced": torch.from_numpy(np.stack([tile_heads(d, table, tg, anchors(gc), rng) for d in dets])).to(dev)}
    for leg, m in models.items():
        m._pipe_kw.update(det_source="synthetic")
        m._fill = (lambda hd: lambda b, v, k: b.pred_in[v * hd.shape[1]:(v + 1) * hd.shape[1]].copy_(hd[k % G]))(heads[leg])
    fps, rows = {k: [] for k in models}, {}
    for m in models.values():
        sum(1 for _ in m.track_stream(frames[:64], batch=G, conf=0.3))                  # warm-up: the pipeline and its graphs exist
    for r in range(rounds):
        for leg in (list(models) if r % 2 == 0 else list(models)[::-1]):
            torch.cuda.synchronize()
            t = time.perf_counter()
            n = sum(len(res[0].boxes) for res in models[leg].track_stream(frames, batch=G, conf=0.3))
            torch.cuda.synchronize()
            fps[leg].append(n_frames / (time.perf_counter() - t))
            rows[leg] = n / n_frames
    tiles = models["sliced"]._stream_pipe.T
    for m in models.values():
        m.close()
    res = {"mode": "rates", "weights": "yolov8n (seeded random init)", "frame": "1280x720", "frames": n_frames, "batch": G, "rounds": rounds, "tiles": tiles}
    for leg, v in fps.items():
        res[f"{leg}_frames_per_s_median"], res[f"{leg}_frames_per_s_all"], res[f"{leg}_track_rows_per_frame"] = float(np.median(v)), [round(x, 1) for x in v], rows[leg]
    res["plain_over_sliced"] = res["plain_frames_per_s_median"] / res["sliced_frames_per_s_median"]
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("kernel", "rates"), default="kernel")
    p.add_argument("--rounds", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--objects", type=int, default=30)
    p.add_argument("--frames", type=int, default=256)
    a = p.parse_args()
    print(json.dumps(kernel(a.rounds, a.warmup, a.objects) if a.mode == "kernel" else rates(a.frames, a.rounds)))
