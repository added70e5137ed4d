"""Writes tests/golden/deteval_cases.npz: seeded inputs for the COCO AP / AR tests and what tests/deteval_ref.py computes on them.

    python tests/golden/make_deteval_golden.py

Boxes lie on a 1/8 px grid.  Per case `<name>_gt` and `<name>_dt`: float64 [n, 8] rows; `<name>_figures`: the restatement's twelve
figures, AP_class and classes as a JSON string; `<name>_precision`, `<name>_recall`: its arrays; `<name>_rank`, `<name>_kept_rows`,
`<name>_match` (int16), `<name>_ignored` (bool): its ranks and match record.
  mixed    16 images x 4 classes, up to 10 boxes and 16 detections a cell, 10 % crowd regions
  ties     12 images x 2 classes, scores rounded to one decimal: ties across images and within cells
  sizes    three classes of very different size: 1 image x 1 box, 4 images x up to 6, 12 images x up to 20
  sparse   mostly stray detections: recall never reaches 1, the precision rows end in zeros
Before anything is written the cases are checked to be deterministic for the restatement alone: no NaN, and no similarity of a kept
detection within 1e-12 of a threshold unless it equals a dyadic threshold (0.5, 0.75, 1.0: exact by construction)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import deteval_ref as ref  # noqa: E402

NAMES = ("mixed", "ties", "sizes", "sparse")


def make_case(name):
    rng = np.random.default_rng(sum(name.encode()))
    if name == "mixed":
        return ref.scene(rng, 16, 4, 10, 16, crowd=0.1)
    if name == "ties":
        return ref.scene(rng, 12, 2, 8, 14, score_decimals=1)
    if name == "sizes":
        parts = [ref.scene(rng, 1, 1, 1, 2), ref.scene(rng, 4, 1, 6, 8), ref.scene(rng, 12, 1, 20, 30)]
        for c, (g, d) in enumerate(parts):
            g[:, 7], d[:, 7] = c + 3, c + 3
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    if name == "sparse":
        gt, dt = ref.scene(rng, 5, 2, 10, 6, jitter=2.0)
        keep = rng.random(len(dt)) < 0.5
        return gt, dt[keep]
    raise KeyError(name)


def check_deterministic(name, gt, dt):
    thrs = ref.default_params()[0]
    for c in np.unique(gt[:, 7]):
        for im in np.unique(gt[:, 0]):
            g = gt[(gt[:, 7] == c) & (gt[:, 0] == im)]
            for d in dt[(dt[:, 7] == c) & (dt[:, 0] == im)]:
                s = ref.sim_iou(d[2:6], g[:, 2:6], g[:, 1] < 0)
                if np.isnan(s).any():
                    raise SystemExit(f"{name}: a NaN similarity")
                near = np.abs(s[:, None] - thrs[None, :]) < 1e-12
                exact = (s[:, None] == thrs[None, :]) & np.isin(thrs, (0.5, 0.75, 1.0))[None, :]
                if (near & ~exact).any():
                    raise SystemExit(f"{name}: a similarity within rounding of a threshold")


def main():
    out = {}
    for name in NAMES:
        gt, dt = make_case(name)
        check_deterministic(name, gt, dt)
        full = ref.evaluate_full(gt, dt)
        again = ref.evaluate_full(gt, dt)
        assert all(np.asarray(full[k]).tobytes() == np.asarray(again[k]).tobytes() for k in ("precision", "recall", "rank", "match", "ignored"))
        out[f"{name}_gt"], out[f"{name}_dt"] = gt, dt
        out[f"{name}_figures"] = np.array(json.dumps({k: full[k] for k in ref.FIGURES + ("AP_class", "classes")}))
        out[f"{name}_precision"], out[f"{name}_recall"] = full["precision"], full["recall"]
        out[f"{name}_rank"], out[f"{name}_kept_rows"] = full["rank"].astype(np.int32), full["kept_rows"].astype(np.int32)
        out[f"{name}_match"], out[f"{name}_ignored"] = full["match"].astype(np.int16), full["ignored"]
        print(f"{name}: {len(gt)} / {len(dt)} rows, " + " ".join(f"{k} {full[k]:.4f}" for k in ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR100")))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "deteval_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
