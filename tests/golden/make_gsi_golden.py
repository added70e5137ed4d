"""Writes tests/golden/gsi_cases.npz: the long GSI cases, whose restatement (tests/gsi_ref.py) takes seconds each.

    python tests/golden/make_gsi_golden.py

Per case `<name>_frames` int32 [n], `<name>_xyxy` float32 [n, 4] (the corners a tracker would give, held exactly in float32) and,
for the two cases the device smooths, `<name>_out` float64 [n, 4]: the smoothed corners of gsi_ref.smooth at tau = 10, alpha = 1e-10.
  c1024  1024 contiguous frames          g1024  1024 rows with gaps of 20 .. 60 frames          p1025  1025 rows: status 2, passed through
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import gsi_ref  # noqa: E402

CASES = (("c1024", 1024, False), ("g1024", 1024, True), ("p1025", 1025, False))


def case_rows(frames, xyxy, tid=1) -> np.ndarray:
    r = np.zeros((len(frames), 8))
    r[:, 0], r[:, 1], r[:, 6] = frames, tid, 0.5
    r[:, 2:6] = np.asarray(xyxy, np.float64)
    return r


def main():
    rng = np.random.default_rng(1024)
    out = {}
    for name, n, gaps in CASES:
        t = gsi_ref.make_track(rng, n, gaps)
        frames, xyxy = t[:, 0].astype(np.int32), t[:, 2:6].astype(np.float32)
        out[f"{name}_frames"], out[f"{name}_xyxy"] = frames, xyxy
        rows, status = gsi_ref.smooth(case_rows(frames, xyxy))
        assert status == {1: 2 if n > gsi_ref.MAX_LEN else 0}, status
        if n <= gsi_ref.MAX_LEN:
            out[f"{name}_out"] = rows[:, 2:6].copy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gsi_cases.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
