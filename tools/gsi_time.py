"""Timing of GSI's smoothing step (docs/GSI.md).  One JSON line per leg on stdout.

  --mode time     (default) a seeded clip of --tracks tracks of --rows rows plus --long tracks of 1024 rows with gaps, through
                  TrackerEngine.gsi_smooth: wall ms per call, the median of --calls calls after --warmup warm-ups, with min and
                  max; then, in the same process, the same tracks through scikit-learn's GaussianProcessRegressor(RBF(l, "fixed"),
                  alpha, optimizer=None) on the host (fit + predict per track, once), and the largest difference between the two.
                  Further legs: the short tracks alone, one 1024-row track alone (both on the device-memory path: 300 rows are
                  more than the 192 the LDS path takes) and --tracks tracks of --lds-rows rows (the LDS path by itself).
  --mode kernel   a loop of --calls gsi_smooth calls on the clip, then on the LDS-path tracks, and nothing else, for
                  `rocprofv3 --kernel-trace --stats -- python tools/gsi_time.py --mode kernel`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def clip(tracks, rows, long_, seed=0):
    """-> (offsets, frames, vals [rows, 4] tlwh, len_scale) of the seeded clip"""
    from strongsort_yolo_amd import gsi
    from tests import gsi_ref
    rng = np.random.default_rng(seed)
    t = [gsi_ref.make_track(rng, rows, False, tid=k + 1, start=int(rng.integers(0, 500))) for k in range(tracks)]
    t += [gsi_ref.make_track(rng, gsi.MAX_LEN, True, tid=tracks + k + 1) for k in range(long_)]
    lens = [len(x) for x in t]
    allr = np.concatenate(t, 0)
    return (np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), allr[:, 0].astype(np.int32), gsi_ref.tlwh(allr),
            np.array([gsi.length_scale(n) for n in lens]))


def device_leg(eng, c, calls, warmup):
    for _ in range(warmup):
        out, st = eng.gsi_smooth(*c)
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out, st = eng.gsi_smooth(*c)
        ms.append(1e3 * (time.perf_counter() - t0))
    return out, st, {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "calls": calls}


def sklearn_leg(c):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF
    off, frames, vals, ls = c
    out = np.empty_like(vals)
    t0 = time.perf_counter()
    for k in range(len(ls)):
        a, b = off[k], off[k + 1]
        X = frames[a:b].astype(np.float64).reshape(-1, 1)
        gp = GaussianProcessRegressor(RBF(ls[k], "fixed"), alpha=1e-10, optimizer=None).fit(X, vals[a:b])
        out[a:b] = gp.predict(X)
    return out, 1e3 * (time.perf_counter() - t0)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("time", "kernel"), default="time")
    p.add_argument("--tracks", type=int, default=64)
    p.add_argument("--rows", type=int, default=300)
    p.add_argument("--long", type=int, default=4)
    p.add_argument("--lds-rows", type=int, default=150)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    a = p.parse_args()
    from strongsort_yolo_amd.engine import TrackerEngine
    eng = TrackerEngine()
    c = clip(a.tracks, a.rows, a.long)
    what = {"tracks": a.tracks, "rows": a.rows, "long_1024": a.long}
    if a.mode == "kernel":
        lds = clip(a.tracks, a.lds_rows, 0)
        for cc in (c, lds):
            for _ in range(a.calls):
                eng.gsi_smooth(*cc)
        print(json.dumps({"leg": "kernel loop", **what, "calls": a.calls}))
        eng.close()
        return
    out, st, dev = device_leg(eng, c, a.calls, a.warmup)
    assert (st == 0).all()
    ref, host_ms = sklearn_leg(c)
    print(json.dumps({"leg": "clip", **what, "device": dev, "sklearn_host_ms": round(host_ms, 1),
                      "max_abs_diff_px": float(np.abs(out - ref).max())}), flush=True)
    for name, cc in (("short tracks alone", clip(a.tracks, a.rows, 0)), ("one 1024-row track alone", clip(0, a.rows, 1)),
                     (f"{a.tracks} tracks of {a.lds_rows} rows (LDS path)", clip(a.tracks, a.lds_rows, 0))):
        out, st, dev = device_leg(eng, cc, a.calls, a.warmup)
        ref, host_ms = sklearn_leg(cc)
        print(json.dumps({"leg": name, "tracks": len(cc[3]), "device": dev, "sklearn_host_ms": round(host_ms, 1),
                          "max_abs_diff_px": float(np.abs(out - ref).max())}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
