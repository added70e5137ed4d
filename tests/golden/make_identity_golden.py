"""Writes tests/golden/identity_cases.npz: the identity figures of the five pairs of tests/golden/moteval_cases.npz, by the full
(G+T)² formulation of tests/identity_ref.py (`full`), at thr = 0.5.

    python tests/golden/make_identity_golden.py

Per case `<name>_identity`: the six figures IDTP, IDFN, IDFP, IDF1, IDP, IDR as a JSON string.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import identity_ref as iref  # noqa: E402
from tests.golden.make_moteval_golden import NAMES, case_rows  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def figures_by_full(gt, tr, thr: float = 0.5) -> dict:
    pot, p = iref.pot_of(gt, tr, thr)
    idtp, idfn, idfp = iref.full(pot, p.cnt_g, p.cnt_t)
    out = iref.figures(idtp, len(p.gt), len(p.tr))
    assert (out["IDFN"], out["IDFP"]) == (idfn, idfp)
    return out


def main():
    z = np.load(os.path.join(HERE, "moteval_cases.npz"))
    out = {}
    for name in NAMES:
        m = figures_by_full(case_rows(z[f"{name}_gt"]), case_rows(z[f"{name}_tr"]))
        out[f"{name}_identity"] = np.array(json.dumps(m))
        print(name, m)
    path = os.path.join(HERE, "identity_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
