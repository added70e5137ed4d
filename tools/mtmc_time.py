"""Timing of the multi-camera linking (docs/MTMC.md §6).  One JSON line per leg on stdout.

  bank   one 32-frame group of a seeded 30-identity stream through TrackerEngine.update_group (StrongSORT's group call) and through
         the track bank's launch behind it: device time of each by HIP events, the median of --calls calls after --warmup warm-ups.
  link   for every count of --tracklets: seeded descriptors (clusters of two to four noisy sightings, four cameras, random
         intervals) through the engine call behind mtmc.link (upload, distances, constraints, clustering, download): wall ms per call, the median of
         --link-calls calls, with the merges made; then the same descriptors through SciPy's pdist + linkage(..., "average") +
         fcluster on the host (no constraints: SciPy has none).  No time here is a gate.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def tracklets(seed, T):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, 512))
    at = 0
    while at + 2 <= T:
        k = min(int(rng.integers(2, 5)), T - at)
        x[at + 1:at + k] = x[at] / np.linalg.norm(x[at]) + 0.02 * rng.standard_normal((k - 1, 512))
        at += k
    x = x[rng.permutation(T)]
    first = rng.integers(0, 2000, T)
    return {"desc": (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), "cam": np.sort(rng.integers(0, 4, T)), "first": first,
            "last": first + rng.integers(1, 200, T), "n": rng.integers(1, 200, T)}


def stat(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4), "max": round(float(max(ms)), 4), "calls": len(ms)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--tracklets", type=int, nargs="+", default=[256, 1024, 2048])
    p.add_argument("--calls", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--link-calls", type=int, default=5)
    a = p.parse_args()
    import torch
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import pdist
    from strongsort_yolo_amd import mtmc
    from strongsort_yolo_amd.engine import TrackerEngine
    from strongsort_yolo_amd.synth import make_stream
    dev = torch.device("cuda", 0)
    eng = TrackerEngine(None, 1, 0)
    bank = mtmc.TrackBank(eng, 4096)
    # ---- the bank launch beside the tracker's group launch
    F, st = 32, make_stream(3, 1280, 720, 30)
    hw = torch.tensor([[720, 1280]], dtype=torch.int32, device=dev)
    out, nout = torch.zeros(F, 1, 256, 8, device=dev), torch.zeros(F, 1, dtype=torch.int32, device=dev)
    t_trk, t_bank, rows = [], [], 0
    for call in range(a.warmup + a.calls):
        d, n, ft = np.zeros((F, 1, 128, 6), np.float32), np.zeros((F, 1), np.int32), np.zeros((F, 1, 128, 512), np.float32)
        for f in range(F):
            fr = st.next_frame()
            d[f, 0, :len(fr.dets)], n[f, 0], ft[f, 0, :len(fr.dets)] = fr.dets, len(fr.dets), fr.feats
        dd, dn, df = (torch.from_numpy(v).to(dev) for v in (d, n, ft))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        ev[0].record()
        eng.update_group(F, dd, dn, df, hw, out, nout)
        ev[1].record()
        bank.update_group_device(out, nout, df, F)
        ev[2].record()
        torch.cuda.synchronize()
        if call >= a.warmup:
            t_trk.append(ev[0].elapsed_time(ev[1]))
            t_bank.append(ev[1].elapsed_time(ev[2]))
            rows += int(nout.sum().item())
    eng.check_errors()
    print(json.dumps({"leg": "bank", "frames_per_group": F, "rows_per_group": round(rows / a.calls, 1), "ids_in_bank": int(len(bank.table(0)["ids"])),
                      "tracker_update_group_ms": stat(t_trk), "bank_update_group_ms": stat(t_bank)}), flush=True)
    # ---- the linking beside SciPy on the host
    for T in a.tracklets:
        t = tracklets(T, T)
        gid, merges = eng.mtmc_link(t["desc"], t["cam"], t["first"], t["last"], t["n"], 0.5, 1)       # warm-up: scratch growth
        ms = []
        for _ in range(a.link_calls):
            t0 = time.perf_counter()
            gid, merges = eng.mtmc_link(t["desc"], t["cam"], t["first"], t["last"], t["n"], 0.5, 1)
            ms.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        fc = fcluster(linkage(pdist(t["desc"].astype(np.float64), "cosine"), "average"), 0.5, "distance")
        scipy_ms = 1e3 * (time.perf_counter() - t0)
        print(json.dumps({"leg": "link", "tracklets": T, "merges": int(len(merges)), "clusters": int(gid.max()), "device_ms": stat(ms),
                          "scipy_unconstrained_ms": round(scipy_ms, 2), "scipy_clusters": int(fc.max())}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
