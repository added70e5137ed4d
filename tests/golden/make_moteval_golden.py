"""Writes tests/golden/moteval_cases.npz: seeded inputs for the HOTA / CLEAR MOT tests and what tests/moteval_ref.py computes on them.

    python tests/golden/make_moteval_golden.py

Ground truth comes from a seeded synth.SynthStream; the tracker rows are a perturbed copy (moteval_ref.perturb: id swaps every k
frames, dropped rows, Gaussian jitter, Poisson false positives with fresh ids).  All corners lie on a 1/8 px grid.  Per case
`<name>_gt` and `<name>_tr`: int16 [6, n] frame, id and 8 x1, 8 y1, 8 x2, 8 y2; `<name>_metrics`: the restatement's metrics as a JSON string; for
more_tr and b256 also `<name>_hota_idx`, `<name>_clear_idx`: int16 per ground-truth row by (frame, id), its matches.
  id6     6 ids / 24 frames, unperturbed                       id30    30 ids / 120 frames, swaps every 15, 10 % drops, 6 px, 0.5 FP a frame
  id100   100 ids / 60 frames, swaps every 5, 30 % drops, 10 px, 3 FP a frame
  more_tr 30 ids / 40 frames with 30 % of the GROUND TRUTH dropped and 3 FP a frame: more tracker than ground-truth boxes
  b256    three frames of 256 x 256 boxes
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import moteval_ref as ref  # noqa: E402

NAMES = ("id6", "id30", "id100", "more_tr", "b256")


def _grid(rows):
    rows[:, 2:6] = np.round(rows[:, 2:6] * 8) / 8
    return rows


def make_case(name):
    gt, tr = _make_case(name)
    return _grid(gt), _grid(tr)


def _make_case(name):
    rng = np.random.default_rng(sum(name.encode()))
    if name == "id6":
        gt = _grid(ref.synth_gt(6, 6, 24))
        return gt, gt.copy()
    if name == "id30":
        gt = _grid(ref.synth_gt(30, 30, 120))
        return gt, ref.perturb(gt, rng, 15, 0.10, 6.0, 0.5)
    if name == "id100":
        gt = _grid(ref.synth_gt(100, 100, 60))
        return gt, ref.perturb(gt, rng, 5, 0.30, 10.0, 3.0)
    if name == "more_tr":
        full = _grid(ref.synth_gt(31, 30, 40))
        tr = ref.perturb(full, rng, 10, 0.0, 4.0, 3.0)
        return full[rng.random(len(full)) >= 0.3], tr
    if name == "b256":
        return ref.random_frames(rng, [(256, 256)] * 3)
    raise KeyError(name)


def case_rows(a) -> np.ndarray:
    """int16 [6, n] of the file -> rows [n, 8] (conf 1, cls 0)"""
    a = np.asarray(a).T
    r = np.zeros((len(a), 8))
    r[:, :2], r[:, 2:6], r[:, 6] = a[:, :2], np.asarray(a[:, 2:6], np.float64) / 8.0, 1.0
    return r


def to_file(rows) -> np.ndarray:
    a = np.concatenate([rows[:, :2], rows[:, 2:6] * 8], 1)
    assert (a == np.round(a)).all() and np.abs(a).max() < 32768
    return np.ascontiguousarray(a.astype(np.int16).T)


def main():
    out = {}
    for name in NAMES:
        gt, tr = make_case(name)
        g32, t32 = to_file(gt), to_file(tr)
        assert (case_rows(g32)[:, :6] == gt[:, :6]).all() and (case_rows(t32)[:, :6] == tr[:, :6]).all(), name
        m, rec = ref.evaluate_full(case_rows(g32), case_rows(t32))
        out[f"{name}_gt"], out[f"{name}_tr"] = g32, t32
        if name in ("more_tr", "b256"):
            out[f"{name}_hota_idx"], out[f"{name}_clear_idx"] = rec["hota_idx"].astype(np.int16), rec["clear_idx"].astype(np.int16)
        out[f"{name}_metrics"] = np.array(json.dumps(m))
        p = rec["pair"]
        tall = sum(1 for f in range(len(p.frames)) if 0 < p.tr_off[f + 1] - p.tr_off[f] < p.gt_off[f + 1] - p.gt_off[f])
        print(f"{name}: {len(gt)} / {len(tr)} rows, {len(p.frames)} frames ({tall} with fewer tracker boxes), HOTA {m['HOTA']:.4f} DetA {m['DetA']:.4f} "
              f"AssA {m['AssA']:.4f} MOTA {m['MOTA']:.4f} IDSW {m['IDSW']} Frag {m['Frag']}")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "moteval_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
