"""COCO AP / AR of the f16 detector's rows against the fp32 detector's rows of the same frames (docs/DETEVAL.md §6).  One JSON line.

The set-up is bench.det_f16_vs_f32's: the same seeded, calibrated random-init network in both precisions (bench.calibrated_detector), 48
rendered frames at 1280x720, HIP letterbox and HIP NMS in both.  The fp32 rows are the ground truth, the f16 rows the detections,
scored by strongsort_yolo_amd.deteval on the device.  What the figure is: the agreement of two precisions on a synthetic network,
not accuracy on data.

    python tools/det_f16_ap.py [--preset c2] [--frames 48]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="c2")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--target", type=int, default=40)
    a = ap.parse_args()
    import torch
    import bench
    from strongsort_yolo_amd import deteval, fused
    from strongsort_yolo_amd.config import DetectConfig
    from strongsort_yolo_amd.pipeline import FramePipeline
    from strongsort_yolo_amd.synth import make_stream
    detector, W, H, n_ids, _ = bench.PRESETS[a.preset]
    dcfg = DetectConfig()
    kw = dict(device=0, reid_batch=32, dcfg=dcfg, det_source="detector", feat_source="injected", graph="none", seed=0)
    p16 = FramePipeline(detector, 1, (H, W), half=True, **kw)
    p32 = FramePipeline(detector, 1, (H, W), half=False, **kw)
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    det32, shift = bench.calibrated_detector(detector, W, H, n_ids, dcfg, p32, a.target)
    for p in (p16, p32):
        p.detector.load_state_dict(det32.state_dict())
        fused.clear_prepared(p.detector)
    st = make_stream(2025, W, H, n_ids)
    rows = {16: [], 32: []}
    with torch.no_grad():
        for k in range(a.frames):
            img = torch.from_numpy(st.render(st.next_frame())).to(p32.dev)
            for bits, p in ((16, p16), (32, p32)):
                p.frames[0].copy_(img)
                p.step(track=False)
                torch.cuda.synchronize(p.dev)
                n = int(p.ndets[0].item())
                d = p.dets[0, :n, :6].double().cpu().numpy()              # x1, y1, x2, y2, conf, cls
                r = np.zeros((n, 8))
                r[:, 0], r[:, 1], r[:, 2:6], r[:, 6], r[:, 7] = k, np.arange(n) if bits == 32 else -1, d[:, :4], d[:, 4], d[:, 5]
                rows[bits].append(r)
    gt, dt = np.concatenate(rows[32]), np.concatenate(rows[16])
    ok = lambda r: (r[:, 4] > r[:, 2]) & (r[:, 5] > r[:, 3])
    dropped = int((~ok(gt)).sum() + (~ok(dt)).sum())
    gt, dt = gt[ok(gt)], dt[ok(dt)]
    out = deteval.evaluate(gt, dt, p32.eng)
    p16.close(); p32.close()
    print(json.dumps({"preset": a.preset, "detector": detector, "frames": a.frames, "fp32_rows": len(gt), "f16_rows": len(dt), "empty_boxes_dropped": dropped,
                      "class_bias_shift": round(shift, 4), **{k: out[k] for k in deteval.FIGURES}, "classes_scored": len(out["classes"]),
                      "note": "f16 detector rows scored as detections against the fp32 detector's rows of the same frames as ground truth; seeded "
                              "calibrated random-init network: agreement of two precisions on a synthetic network, not accuracy on data"}))


if __name__ == "__main__":
    main()
