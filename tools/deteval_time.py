"""Timing of COCO AP / AR scoring (docs/DETEVAL.md).  One JSON line per leg on stdout.

  --mode time     (default) per leg wall ms of one deteval.evaluate call (host packing, the device call, the figures): the median of
                  --calls calls after --warmup warm-ups, with min and max; the share of that spent inside TrackerEngine.ap_eval; and,
                  in the same process, tests/deteval_ref.py on the host, once (skipped above --ref-rows detection rows and for the
                  dense leg: "not measured").
                  Legs: the golden cases mixed and sizes; a user's size, --images images of 1 .. --dets detections over --classes
                  classes, built from one-box cells whose detections are the box itself or a disjoint one (so the restatement's
                  loops stay short); and a dense leg of 200 images x 8 classes with up to 40 boxes and 100
                  detections a cell (jittered copies and strays).
  --mode kernel   a loop of --calls calls of the user's-size leg and of the dense leg and nothing else, for
                  `rocprofv3 --kernel-trace --stats -- python tools/deteval_time.py --mode kernel`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def stats(ms, calls):
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "calls": calls}


def device_leg(eng, gt, dt, calls, warmup):
    from strongsort_yolo_amd import deteval
    inner = []
    real = eng.ap_eval

    def timed(*a, **k):
        t0 = time.perf_counter()
        out = real(*a, **k)
        inner.append(1e3 * (time.perf_counter() - t0))
        return out

    eng.ap_eval = timed
    try:
        for _ in range(warmup):
            out = deteval.evaluate(gt, dt, eng)
        del inner[:]
        ms = []
        for _ in range(calls):
            t0 = time.perf_counter()
            out = deteval.evaluate(gt, dt, eng)
            ms.append(1e3 * (time.perf_counter() - t0))
    finally:
        del eng.ap_eval
    return out, stats(ms, calls), stats(inner, calls)


def host_leg(gt, dt):
    from tests import deteval_ref
    t0 = time.perf_counter()
    out = deteval_ref.evaluate(gt, dt)
    return out, 1e3 * (time.perf_counter() - t0)


def users_size(images, classes, dets, seed=0):
    """every image has 1 .. dets detections of random classes; 70 % of the (image, class) cells that hold a detection hold one
    ground-truth box as well; a cell's first detection is that box with probability 0.7 and every other detection is a box disjoint
    from everything, so every similarity is 1 or 0; scores with three decimals"""
    rng = np.random.default_rng(seed)
    img = np.repeat(np.arange(images), rng.integers(1, dets + 1, images)).astype(np.float64)
    n = len(img)
    cls = rng.integers(0, classes, n).astype(np.float64)
    cell, first, inv = np.unique(img * classes + cls, return_index=True, return_inverse=True)
    xy = np.round(rng.uniform(0, 500, (len(cell), 2)) * 8) / 8
    wh = np.round(rng.uniform(8, 160, (len(cell), 2)) * 8) / 8
    box = np.concatenate([xy, xy + wh], 1)
    has_gt = rng.random(len(cell)) < 0.7
    gt = np.zeros((int(has_gt.sum()), 8))
    gt[:, 0], gt[:, 2:6], gt[:, 6], gt[:, 7] = img[first[has_gt]], box[has_gt], 1.0, cls[first[has_gt]]
    dt = np.zeros((n, 8))
    dt[:, 0], dt[:, 1], dt[:, 2:6], dt[:, 6], dt[:, 7] = img, -1.0, box[inv.reshape(-1)], np.round(rng.random(n), 3), cls
    hit = np.zeros(n, bool)
    hit[first] = rng.random(len(cell)) < 0.7
    dt[~hit, 2:6] += 1000.0 + 200.0 * (np.arange(n) % 1000)[~hit, None]
    return gt, dt


def dense(seed=1):
    from tests import deteval_ref
    return deteval_ref.scene(np.random.default_rng(seed), 200, 8, 40, 100, crowd=0.05)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("time", "kernel"), default="time")
    p.add_argument("--images", type=int, default=5000)
    p.add_argument("--classes", type=int, default=80)
    p.add_argument("--dets", type=int, default=100)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--ref-rows", type=int, default=400000, help="the restatement runs on the host only up to this many detection rows")
    a = p.parse_args()
    from strongsort_yolo_amd import deteval
    from strongsort_yolo_amd.engine import TrackerEngine
    eng = TrackerEngine()
    big = users_size(a.images, a.classes, a.dets)
    legs = [(f"{a.images} images x {a.classes} classes, 1 .. {a.dets} detections an image, one-box cells",) + big + (len(big[1]) <= a.ref_rows,),
            ("200 images x 8 classes, up to 40 boxes x 100 detections a cell",) + dense() + (False,)]     # (its 10^8 loop steps are not for the host)
    if a.mode == "kernel":
        for _, g, d, _ in legs:
            for _ in range(a.calls):
                deteval.evaluate(g, d, eng)
        print(json.dumps({"leg": "kernel loop", "legs": [leg[0] for leg in legs], "calls": a.calls}))
        eng.close()
        return
    z = np.load(os.path.join(ROOT, "tests", "golden", "deteval_cases.npz"))
    legs = [(name, z[f"{name}_gt"], z[f"{name}_dt"], True) for name in ("mixed", "sizes")] + legs
    for name, g, d, on_host in legs:
        got, whole, inner = device_leg(eng, g, d, a.calls, a.warmup)
        line = {"leg": name, "gt_rows": len(g), "det_rows": len(d), "evaluate": whole, "of_which_ap_eval": inner}
        if on_host:
            want, host_ms = host_leg(g, d)
            line.update(restatement_host_ms=round(host_ms, 1), equal=json.dumps(got) == json.dumps(want))
        else:
            line.update(restatement_host_ms="not measured", equal="not measured")
        line.update(AP=got["AP"], AP50=got["AP50"], AR100=got["AR100"])
        print(json.dumps(line), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
