"""Timing of AFLink's cost step (docs/AFLINK.md §6).  One JSON line per leg on stdout.

  --mode time     (default) for every count of --pairs: seeded couples of tracklets that gate into exactly that many candidates
                  (tests/aflink_ref.couples) through aflink.costs (gate, inputs, network, copies): wall ms per call, the median
                  of --calls calls after --warmup warm-ups, with min and max, and the largest difference to the CPU float32
                  PyTorch network.  Then, in the same process on --threads CPU threads, the same pairs through the CPU float32
                  PyTorch network in batches of --batch, and pair at a time (the form upstream runs; --single pairs of them,
                  scaled to the whole set).
  --mode kernel   a loop of --calls aflink.costs calls for the largest count and nothing else, for
                  `rocprofv3 --kernel-trace --stats -- python tools/aflink_time.py --mode kernel`.
  --stats CSV     no device: reads a rocprofv3 kernel-stats CSV of a --mode kernel run and prints, per k_afl_gemm instantiation and
                  in total, the mean time per call and the fraction of the 157.3 TFLOP/s f32 MFMA peak from its FLOP count.
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PEAK_TFLOPS = 157.3
# 2 x rows x K x N per branch of the four wide layers, both branches: 32.6 MFLOP a pair (the first layer and the head add 0.1)
GEMM_FLOP = {"32, 64": 2 * 2 * 54 * 224 * 64, "64, 128": 2 * 2 * 36 * 448 * 128, "128, 256": 2 * 2 * 18 * 896 * 256, "256, 256": 2 * 2 * 6 * 768 * 256}


def stats(path, pairs, calls):
    total_ns, total_flop = 0.0, 0.0
    for row in csv.DictReader(open(path)):
        name = row["Name"]
        if "k_afl_gemm" not in name:
            continue
        key = next(k for k in GEMM_FLOP if f"<{k}," in name.replace("k_afl_gemm<", "<"))
        ns = float(row["TotalDurationNs"]) / calls
        flop = GEMM_FLOP[key] * pairs
        total_ns, total_flop = total_ns + ns, total_flop + flop
        print(json.dumps({"kernel": f"k_afl_gemm<{key}>", "us_per_call": round(ns / 1e3, 1), "tflops": round(flop / ns / 1e3, 2),
                          "of_f32_mfma_peak": round(flop / ns / 1e3 / PEAK_TFLOPS, 3)}))
    print(json.dumps({"kernel": "the four GEMM launches", "us_per_call": round(total_ns / 1e3, 1), "tflops": round(total_flop / total_ns / 1e3, 2),
                      "of_f32_mfma_peak": round(total_flop / total_ns / 1e3 / PEAK_TFLOPS, 3)}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("time", "kernel"), default="time")
    p.add_argument("--pairs", type=int, nargs="+", default=[256, 4096])
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--single", type=int, default=64)
    p.add_argument("--stats", default=None)
    a = p.parse_args()
    if a.stats:
        return stats(a.stats, max(a.pairs), a.calls)
    import torch
    from strongsort_yolo_amd import aflink
    from strongsort_yolo_amd.engine import TrackerEngine
    from tests import aflink_ref
    torch.set_num_threads(a.threads)
    model = aflink_ref.calibrated(0)
    eng = TrackerEngine()
    if a.mode == "kernel":
        rows = aflink_ref.couples(7, max(a.pairs))
        for _ in range(a.calls):
            aflink.costs(rows, eng, model)
        print(json.dumps({"leg": "kernel loop", "pairs": max(a.pairs), "calls": a.calls}))
        eng.close()
        return
    for n in a.pairs:
        rows = aflink_ref.couples(7, n)
        for _ in range(a.warmup):
            pi, pj, cost = aflink.costs(rows, eng, model)
        ms = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            pi, pj, cost = aflink.costs(rows, eng, model)
            ms.append(1e3 * (time.perf_counter() - t0))
        assert len(pi) == n
        _, offsets, _, feats = aflink_ref.tracklets(rows)
        x = torch.from_numpy(aflink_ref.transform(offsets, feats, pi, pj))
        with torch.no_grad():
            t0 = time.perf_counter()
            ref = torch.cat([1.0 - model(x[k:k + a.batch, 0:1], x[k:k + a.batch, 1:2])[:, 1] for k in range(0, n, a.batch)]).numpy()
            batched_ms = 1e3 * (time.perf_counter() - t0)
            k1 = min(a.single, n)
            t0 = time.perf_counter()
            for k in range(k1):
                model(x[k:k + 1, 0:1], x[k:k + 1, 1:2])
            single_ms = 1e3 * (time.perf_counter() - t0) / k1
        print(json.dumps({"leg": "aflink.costs", "pairs": n, "device": {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3),
                                                                         "ms_max": round(max(ms), 3), "calls": a.calls},
                          "cpu_f32_batched_ms": round(batched_ms, 1), "cpu_f32_pair_at_a_time_ms_per_pair": round(single_ms, 3),
                          "cpu_f32_pair_at_a_time_ms": round(single_ms * n, 1), "cpu_threads": a.threads,
                          "max_abs_diff_to_cpu_f32": float(np.abs(cost - ref).max())}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
