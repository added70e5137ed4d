"""Timing of HOTA / CLEAR MOT scoring (docs/MOTEVAL.md).  One JSON line per leg on stdout.

  --mode time     (default) per leg wall ms of one moteval.evaluate call (host packing, the device call, the figures): the median of
                  --calls calls after --warmup warm-ups, with min and max; the share of that spent inside TrackerEngine.mot_eval;
                  and, in the same process, tests/moteval_ref.py (NumPy + SciPy's linear_sum_assignment) on the host, once per pair.
                  Legs: the golden cases id30 and id100, one pair of --frames frames x --ids ids (swaps every 25 frames, 10 % drops,
                  4 px jitter, one false positive a frame), and --pairs such pairs (different seeds of the perturbation) in one call.
  --mode kernel   a loop of --calls calls of the single large pair and of the --pairs-pair call and nothing else, for
                  `rocprofv3 --kernel-trace --stats -- python tools/moteval_time.py --mode kernel`.
  --mode identity per leg wall ms of one moteval.identity call (IDF1, IDP, IDR: host packing, the device call, the figures), the same
                  statistics, the share inside TrackerEngine.mot_identity, and in the same process tests/identity_ref.py on the host:
                  the counts (pot_of), SciPy's linear_sum_assignment on the G x T reduction, and on the full (G+T)^2 matrix where
                  G + T < 1500.  Legs: those of --mode time, one dense tie-heavy pair of 1100 x 1030 ids (identity_ref.crowd, 24 frames
                  of 256 boxes a side), and two at the ids cap (4096 x 3072 ids in 40 frames, 4096 x 4096 in 20).
  --mode identity-kernel   --calls calls of the 1100 x 1030 pair, then of the 4096 x 3072 pair, and nothing else, for rocprofv3.
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


def identity_leg(eng, gt, trs, calls, warmup):
    from strongsort_yolo_amd import moteval
    inner = []
    real = eng.mot_identity

    def timed(*a, **k):
        t0 = time.perf_counter()
        out = real(*a, **k)
        inner.append(1e3 * (time.perf_counter() - t0))
        return out

    eng.mot_identity = timed
    try:
        for _ in range(warmup):
            out = moteval.identity(gt, trs, eng)
        del inner[:]
        ms = []
        for _ in range(calls):
            t0 = time.perf_counter()
            out = moteval.identity(gt, trs, eng)
            ms.append(1e3 * (time.perf_counter() - t0))
    finally:
        del eng.mot_identity
    return out, stats(ms, calls), stats(inner, calls)


def identity_host_leg(gt, trs):
    """-> (figures per pair, ms of the counts, ms of SciPy on the reduction, ms of SciPy on the full matrix or None)"""
    from tests import identity_ref
    out, t_pot, t_red, t_full = [], 0.0, 0.0, 0.0
    for t in trs:
        t0 = time.perf_counter()
        pot, p = identity_ref.pot_of(gt, t)
        t1 = time.perf_counter()
        w = identity_ref.reduced(pot)
        t2 = time.perf_counter()
        t_pot, t_red = t_pot + 1e3 * (t1 - t0), t_red + 1e3 * (t2 - t1)
        if t_full is not None and p.n_gid + p.n_tid < 1500:
            assert identity_ref.full(pot, p.cnt_g, p.cnt_t)[0] == w
            t_full += 1e3 * (time.perf_counter() - t2)
        else:
            t_full = None
        out.append(identity_ref.figures(w, len(p.gt), len(p.tr)))
    return out, t_pot, t_red, t_full


def crowds():
    from tests import identity_ref
    return [(f"crowd {g} x {t} ids, {f} frames",) + identity_ref.crowd(np.random.default_rng(g + f), g, t, f)
            for g, t, f in ((1100, 1030, 24), (4096, 3072, 40), (4096, 4096, 20))]


def large(frames, ids, pairs):
    from tests import moteval_ref
    gt = moteval_ref.synth_gt(1000, ids, frames)
    return gt, [moteval_ref.perturb(gt, np.random.default_rng(k), 25, 0.10, 4.0, 1.0) for k in range(pairs)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("time", "kernel", "identity", "identity-kernel"), default="time")
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
    if a.mode == "identity-kernel":
        legs = crowds()[:2]
        for _, g, t in legs:
            for _ in range(a.calls):
                moteval.identity(g, t, eng)
        print(json.dumps({"leg": "identity kernel loop", "legs": [n for n, _, _ in legs], "calls": a.calls}))
        eng.close()
        return
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
    if a.mode == "identity":
        for name, g, t in legs + [(n, cg, [ct]) for n, cg, ct in crowds()]:
            got, whole, inner = identity_leg(eng, g, t, a.calls, a.warmup)
            want, pot_ms, red_ms, full_ms = identity_host_leg(g, t)
            print(json.dumps({"leg": name, "pairs": len(t), "gt_rows": len(g), "tracker_rows": [len(x) for x in t], "identity": whole, "of_which_mot_identity": inner,
                              "host_counts_ms": round(pot_ms, 1), "scipy_reduction_ms": round(red_ms, 1), "scipy_full_ms": None if full_ms is None else round(full_ms, 1),
                              "equal": json.dumps(got) == json.dumps(want), "IDF1": got[0]["IDF1"], "IDTP": got[0]["IDTP"]}), flush=True)
        eng.close()
        return
    for name, g, t in legs:
        got, whole, inner = device_leg(eng, g, t, a.calls, a.warmup)
        want, host_ms = host_leg(g, t)
        print(json.dumps({"leg": name, "pairs": len(t), "gt_rows": len(g), "tracker_rows": [len(x) for x in t], "evaluate": whole, "of_which_mot_eval": inner,
                          "restatement_host_ms": round(host_ms, 1), "equal": json.dumps(got) == json.dumps(want), "HOTA": got[0]["HOTA"], "IDSW": got[0]["IDSW"]}),
              flush=True)
    eng.close()


if __name__ == "__main__":
    main()
