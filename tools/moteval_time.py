"""Timing of HOTA / CLEAR MOT scoring (docs/MOTEVAL.md).  One JSON line per leg on stdout.

  --mode time     (default) per leg wall ms of one moteval.evaluate call (host packing, the device call, the figures): the median of
                  --calls calls after --warmup warm-ups, with min and max; the share of that spent inside TrackerEngine.mot_eval;
                  and, in the same process, tests/moteval_ref.py (NumPy + SciPy's linear_sum_assignment) on the host, once per pair.
                  Legs: the golden cases id30 and id100, one pair of --frames frames x --ids ids (swaps every 25 frames, 10 % drops,
                  4 px jitter, one false positive a frame), and --pairs such pairs (different seeds of the perturbation) in one call.
  --mode kernel   a loop of --calls calls of the single large pair and of the --pairs-pair call and nothing else, for
                  `rocprofv3 --kernel-trace --stats -- python tools/moteval_time.py --mode kernel`.
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


def device_leg(eng, gt, trs, calls, warmup):
    from strongsort_yolo_amd import moteval
    inner = []
    real = eng.mot_eval

    def timed(*a, **k):
        t0 = time.perf_counter()
        out = real(*a, **k)
        inner.append(1e3 * (time.perf_counter() - t0))
        return out

    eng.mot_eval = timed
    try:
        for _ in range(warmup):
            out = moteval.evaluate(gt, trs, eng)
        del inner[:]
        ms = []
        for _ in range(calls):
            t0 = time.perf_counter()
            out = moteval.evaluate(gt, trs, eng)
            ms.append(1e3 * (time.perf_counter() - t0))
    finally:
        del eng.mot_eval
    return out, stats(ms, calls), stats(inner, calls)


def host_leg(gt, trs):
    from tests import moteval_ref
    t0 = time.perf_counter()
    out = [moteval_ref.evaluate(gt, t) for t in trs]
    return out, 1e3 * (time.perf_counter() - t0)


def large(frames, ids, pairs):
    from tests import moteval_ref
    gt = moteval_ref.synth_gt(1000, ids, frames)
    return gt, [moteval_ref.perturb(gt, np.random.default_rng(k), 25, 0.10, 4.0, 1.0) for k in range(pairs)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("time", "kernel"), default="time")
    p.add_argument("--frames", type=int, default=1000)
    p.add_argument("--ids", type=int, default=100)
    p.add_argument("--pairs", type=int, default=8)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    a = p.parse_args()
    from strongsort_yolo_amd import moteval
    from strongsort_yolo_amd.engine import TrackerEngine
    from tests.golden.make_moteval_golden import case_rows
    eng = TrackerEngine()
    gt, trs = large(a.frames, a.ids, a.pairs)
    if a.mode == "kernel":
        for sets in (trs[:1], trs):
            for _ in range(a.calls):
                moteval.evaluate(gt, sets, eng)
        print(json.dumps({"leg": "kernel loop", "frames": a.frames, "ids": a.ids, "pairs": [1, a.pairs], "calls": a.calls}))
        eng.close()
        return
    z = np.load(os.path.join(ROOT, "tests", "golden", "moteval_cases.npz"))
    legs = [(name, case_rows(z[f"{name}_gt"]), [case_rows(z[f"{name}_tr"])]) for name in ("id30", "id100")]
    legs += [(f"1 pair of {a.frames} frames x {a.ids} ids", gt, trs[:1]), (f"{a.pairs} such pairs in one call", gt, trs)]
    for name, g, t in legs:
        got, whole, inner = device_leg(eng, g, t, a.calls, a.warmup)
        want, host_ms = host_leg(g, t)
        print(json.dumps({"leg": name, "pairs": len(t), "gt_rows": len(g), "tracker_rows": [len(x) for x in t], "evaluate": whole, "of_which_mot_eval": inner,
                          "restatement_host_ms": round(host_ms, 1), "equal": json.dumps(got) == json.dumps(want), "HOTA": got[0]["HOTA"], "IDSW": got[0]["IDSW"]}),
              flush=True)
    eng.close()


if __name__ == "__main__":
    main()
