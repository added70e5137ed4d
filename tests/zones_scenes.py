"""Seeded scenes for the analytics stage (docs/ZONES.md): walkers in the tracker's device layout (rows [F, S, 256, 8] float32 = x1, y1,
x2, y2, id, cls, conf, det; counts [F, S]) and geometry at the caps.

Not a conftest and not a test module: imported by tests/test_zones_cpu.py and tests/test_gpu_zones.py.
"""
import numpy as np

ROWS = 256
HW = (120, 160)                                    # small frames keep the heat grids of a 32-frame group small


def star(cx, cy, r_out, r_in, n=32):
    """A concave polygon of n integer vertices, alternating between two radii."""
    a = np.arange(n) * (2.0 * np.pi / n)
    r = np.where(np.arange(n) % 2 == 0, r_out, r_in)
    return [[int(round(cx + r[i] * np.cos(a[i]))), int(round(cy + r[i] * np.sin(a[i])))] for i in range(n)]


def geometry(n_lines=3, n_zones=3, verts=32, hw=HW, seed=1):
    """n_lines segments across the frame and n_zones star polygons of `verts` vertices, seeded."""
    rng = np.random.default_rng(seed)
    h, w = hw
    lines = []
    while len(lines) < n_lines:
        l = [int(v) for v in (rng.integers(0, w), rng.integers(0, h), rng.integers(0, w), rng.integers(0, h))]
        if l[:2] != l[2:]:
            lines.append(l)
    zones = [star(int(rng.integers(w // 4, 3 * w // 4)), int(rng.integers(h // 4, 3 * h // 4)), int(rng.integers(h // 4, h // 2)),
                  int(rng.integers(h // 12, h // 5)), verts) for _ in range(n_zones)]
    return lines, zones


def walkers(seed, F, S=1, n_tracks=40, hw=HW, id_step=1, life=None, births=0, p_miss=0.15, dirt=True, speed=9.0, id0=1):
    """F frames of S streams.  n_tracks walkers live from frame 0 (life None: for ever); `births` more are born every frame and live
    `life` frames, so ids churn.  A walker misses a frame with probability p_miss (gaps of any length).  dirt: now and then a second row
    of an id already in the frame, a row with a non-finite corner, a row with id 0.  Rows are shuffled; a frame holds at most 256."""
    rng = np.random.default_rng(seed)
    h, w = hw
    rows, counts = np.zeros((F, S, ROWS, 8), np.float32), np.zeros((F, S), np.int32)
    for s in range(S):
        tracks = []                                  # [id, x, y, vx, vy, bw, bh, cls, dies]
        nid = id0

        def born(f):
            nonlocal nid
            t = [nid, rng.uniform(-20, w + 20), rng.uniform(-20, h + 20), rng.uniform(-speed, speed), rng.uniform(-speed, speed),
                 rng.uniform(6, 40), rng.uniform(10, 60), int(rng.integers(0, 5)), (F + 1 if life is None else f + life)]
            nid += id_step
            return t
        tracks = [born(0) if life is None else born(int(rng.integers(-life + 1, 1))) for _ in range(n_tracks)]
        for f in range(F):
            tracks = [t for t in tracks if t[8] > f] + [born(f) for _ in range(births)]
            out = []
            for t in tracks:
                t[1] += t[3]; t[2] += t[4]
                if not -40 < t[1] < w + 40: t[3] = -t[3]
                if not -40 < t[2] < h + 40: t[4] = -t[4]
                if rng.random() < p_miss:
                    continue
                out.append([t[1] - t[5] / 2, t[2] - t[6], t[1] + t[5] / 2, t[2], t[0], t[7], rng.uniform(0.3, 0.99), len(out)])
            if dirt and out:
                k = int(rng.integers(0, len(out)))
                if rng.random() < 0.5:
                    out.append([out[k][0] + 31.5, out[k][1] - 17.25, out[k][2] + 31.5, out[k][3] - 17.25] + out[k][4:])   # the id twice
                if rng.random() < 0.3:
                    out.append([np.nan if rng.random() < 0.5 else np.inf, 1.0, 20.0, 30.0, 900000 + f, 0, 0.5, 0])
                if rng.random() < 0.3:
                    out.append([10.0, 10.0, 30.0, 50.0, 0, 1, 0.5, 0])
            out = np.asarray(out, np.float32).reshape(-1, 8)[:ROWS]
            out = out[rng.permutation(len(out))]
            rows[f, s, :len(out)], counts[f, s] = out, len(out)
    return rows, counts


def labels_rows(seed=3, F=40, n_tracks=12, hw=HW):
    """A labels array as gsi.py holds it ([N, 8]: frame, id, x1, y1, x2, y2, conf, cls) with integer corners, as a labels file records."""
    rows, counts = walkers(seed, F, 1, n_tracks, hw, dirt=False)
    out = []
    for f in range(F):
        for r in rows[f, 0, :counts[f, 0]]:
            out.append([f, r[4], *np.trunc(r[:4]), round(float(r[6]), 3), r[5]])
    return np.asarray(out, np.float64).reshape(-1, 8)
