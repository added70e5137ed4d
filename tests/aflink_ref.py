"""AFLink restated on the CPU (docs/AFLINK.md): the gate, the input transform, the merge and the dedupe in NumPy, the network as the
float64 form of aflink.PostLinker with its BatchNorms unfolded, the matching with SciPy both on the full compressed matrix (what
upstream solves) and component by component (what the device solves).  The project's own restatement: parity with upstream is
unpinned (docs/AFLINK.md §2)."""
import copy
import functools

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from strongsort_yolo_amd import aflink

LEN = 30
FILL = 1e5


# ---- tracklets, gate, transform ----------------------------------------------------------------------------------------------
def tracklets(rows):
    r = np.asarray(rows, np.float64).reshape(-1, 8)
    ids = sorted(set(r[:, 1].tolist()))
    tr = []
    for tid in ids:
        t = r[r[:, 1] == tid]
        tr.append(t[np.argsort(t[:, 0], kind="stable")])
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in tr])]).astype(np.int32)
    allr = np.concatenate(tr, 0) if tr else np.zeros((0, 8))
    return np.array(ids, np.float64), offsets, allr, np.ascontiguousarray(allr[:, [0, 2, 3]])


def gate(offsets, feats, thr_t=(0, 30), thr_s=75.0):
    n = len(offsets) - 1
    pi, pj = [], []
    for i in range(n):
        fi, xi, yi = feats[offsets[i + 1] - 1]
        for j in range(n):
            if i == j:
                continue
            fj, xj, yj = feats[offsets[j]]
            if (int(feats[offsets[i]][0]), i) > (int(fj), j):                # i starts first (ties: the smaller number): no cycles
                continue
            gap = int(fj) - int(fi)
            if not (thr_t[0] <= gap < thr_t[1]):
                continue
            dx, dy = xj - xi, yj - yi
            if np.sqrt(dx * dx + dy * dy) <= thr_s:
                pi.append(i)
                pj.append(j)
    return np.array(pi, np.int32), np.array(pj, np.int32)


def transform(offsets, feats, pi, pj):
    """-> [pairs, 2, 30, 3] float32: float64 arithmetic, rounded once."""
    out = np.zeros((len(pi), 2, LEN, 3), np.float32)
    for k, (i, j) in enumerate(zip(pi, pj)):
        a = feats[offsets[i]:offsets[i + 1]][-LEN:]
        b = feats[offsets[j]:offsets[j + 1]][:LEN]
        a = np.concatenate([np.zeros((LEN - len(a), 3)), a], 0)
        b = np.concatenate([b, np.zeros((LEN - len(b), 3))], 0)
        both = np.concatenate([a, b], 0)
        mn, mx = both.min(0), both.max(0)
        both = (both - (mx + mn) / 2.0) / ((mx - mn) / 2.0 + 1e-5)
        out[k, 0], out[k, 1] = both[:LEN], both[LEN:]
    return out


# ---- network -----------------------------------------------------------------------------------------------------------------
def net64(model):
    return copy.deepcopy(model).double().eval()


def net_costs(model, x, dtype=torch.float64, batch=128):
    """cost = 1 - p[1] of `model` (any dtype copy of it) on inputs x [pairs, 2, 30, 3]."""
    m = copy.deepcopy(model).to(dtype).eval()
    x = torch.from_numpy(np.asarray(x)).to(dtype)
    out = []
    with torch.no_grad():
        for k in range(0, len(x), batch):
            xb = x[k:k + batch]
            out.append(1.0 - m(xb[:, 0:1], xb[:, 1:2])[:, 1])
    return torch.cat(out).double().numpy() if out else np.zeros(0)


def couples(seed, n, lengths=None, spacing=3000.0):
    """n couples of tracklets -> rows [N, 8].  Couple k is tracklet 2k (the earlier) and 2k+1 (the later) by id; the couples sit
    `spacing` apart, so the gate passes exactly the n pairs (2k, 2k+1), in that order.  Half of the later tracklets continue the
    earlier one's motion, half start somewhere within the gate.  Coordinates are positive."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n):
        la, lb = (int(rng.integers(1, 61)), int(rng.integers(1, 61))) if lengths is None else lengths[k % len(lengths)]
        f0 = int(rng.integers(1, 400))
        pos = np.array([200.0 + spacing * k, float(rng.uniform(100, 900))])
        vel = rng.normal(0, 3.0, 2)
        fa = f0 + np.cumsum(rng.integers(1, 3, la))
        pa = pos + np.cumsum(vel + rng.normal(0, 1.0, (la, 2)), 0)
        gap = int(rng.integers(0, 30))
        if rng.random() < 0.5:
            start = pa[-1] + vel * gap + rng.normal(0, 2.0, 2)
        else:
            start, vel = pa[-1] + rng.uniform(-50, 50, 2), rng.normal(0, 3.0, 2)
        d = start - pa[-1]
        if np.hypot(*d) > 70.0:
            start = pa[-1] + d * (70.0 / np.hypot(*d))
        fb = fa[-1] + gap + np.concatenate([[0], np.cumsum(rng.integers(1, 3, lb - 1))])
        pb = start + np.concatenate([np.zeros((1, 2)), np.cumsum(vel + rng.normal(0, 1.0, (lb - 1, 2)), 0)], 0)
        for tid, f, p in ((2 * k + 1, fa, pa), (2 * k + 2, fb, pb)):
            p = np.abs(p) + 1.0
            blk = np.zeros((len(f), 8))
            blk[:, 0], blk[:, 1], blk[:, 2], blk[:, 3] = f, tid, p[:, 0], p[:, 1]
            blk[:, 4], blk[:, 5], blk[:, 6] = p[:, 0] + 40.0, p[:, 1] + 90.0, 0.9
            rows.append(blk)
    return np.concatenate(rows, 0)


def couple_inputs(seed, n):
    _, offsets, _, feats = tracklets(couples(seed, n))
    pi, pj = gate(offsets, feats)
    assert len(pi) == n
    return transform(offsets, feats, pi, pj)


@functools.lru_cache(maxsize=4)
def calibrated(seed=0):
    """A PostLinker whose costs spread over 0 .. 1 (a plain random initialisation puts every cost near 0.465): every BatchNorm's
    running statistics come from one training-mode pass with momentum 1 over 256 seeded pairs, fc2 is rescaled so the logit
    difference has a standard deviation of 4 on them and its bias centred on their median.  The pass runs in float64 and the
    result is rounded to the float32 parameters once."""
    model = aflink.PostLinker(seed)
    x = torch.from_numpy(couple_inputs(1000 + seed, 256)).double()
    m = net64(model)
    for mod in m.modules():
        if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
            mod.momentum = 1.0
    with torch.no_grad():
        m.train()
        m(x[:, 0:1], x[:, 1:2])
        m.eval()
        y = m.classifier(*m.features(x[:, 0:1], x[:, 1:2]))
        d = y[:, 1] - y[:, 0]
        s = 4.0 / float(d.std())
        m.classifier.fc2.weight.mul_(s)
        m.classifier.fc2.bias.mul_(s)
        m.classifier.fc2.bias[1] -= float((d * s).median())
    for mod in m.modules():
        if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
            mod.momentum = 0.1
    model.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in m.state_dict().items()})
    return model.eval()


# ---- matching ----------------------------------------------------------------------------------------------------------------
def _solve(pi, pj, cost, thr_p):
    rows, cols = np.unique(pi), np.unique(pj)
    m = np.full((len(rows), len(cols)), FILL)
    m[np.searchsorted(rows, pi), np.searchsorted(cols, pj)] = cost
    r, c = linear_sum_assignment(m)
    return [(int(rows[a]), int(cols[b]), float(m[a, b])) for a, b in zip(r, c) if m[a, b] < thr_p]


def match_full(n, pi, pj, cost, thr_p=0.05):
    """Upstream's matching: SciPy on the matrix of survivors (1e5 elsewhere) compressed to the rows and columns that have one.
    -> (successor [n], cost sum)."""
    pi, pj, cost = np.asarray(pi), np.asarray(pj), np.asarray(cost, np.float64)
    succ = np.full(n, -1, np.int32)
    s = cost < thr_p
    links = _solve(pi[s], pj[s], cost[s], thr_p) if s.any() else []
    for i, j, _ in links:
        succ[i] = j
    return succ, float(sum(c for _, _, c in links))


def match_components(n, pi, pj, cost, thr_p=0.05):
    """The same, one connected component of the survivor graph at a time, each with its own 1e5 fill."""
    pi, pj, cost = np.asarray(pi), np.asarray(pj), np.asarray(cost, np.float64)
    succ = np.full(n, -1, np.int32)
    s = cost < thr_p
    if not s.any():
        return succ, 0.0
    pi, pj, cost = pi[s], pj[s], cost[s]
    _, lab = connected_components(coo_matrix((np.ones(len(pi)), (pi, n + pj)), shape=(2 * n, 2 * n)), directed=False)
    total = 0.0
    for c in np.unique(lab[pi]):
        k = lab[pi] == c
        for i, j, v in _solve(pi[k], pj[k], cost[k], thr_p):
            succ[i] = j
            total += v
    return succ, total


# ---- merge ------------------------------------------------------------------------------------------------------------------
def merge(rows, ids, succ):
    """Follow predecessors to the head of the chain; where two rows share (frame, id) the one nearer the head stays.  A walk
    longer than the number of tracklets has met a cycle: refused."""
    pred = {int(j): i for i, j in enumerate(succ) if j >= 0}
    chain = {}
    for k in range(len(ids)):
        h, d = k, 0
        while h in pred:
            h, d = pred[h], d + 1
            if d > len(ids):
                raise ValueError(f"the links form a cycle through tracklet {k}")
        chain[k] = (h, d)
    r = np.asarray(rows, np.float64).reshape(-1, 8)
    index = {float(t): k for k, t in enumerate(ids)}
    best = {}
    for row in r:
        h, d = chain[index[float(row[1])]]
        key = (float(row[0]), float(ids[h]))
        if key not in best or d < best[key][0]:
            new = row.copy()
            new[1] = ids[h]
            best[key] = (d, new)
    out = np.array([best[k][1] for k in sorted(best)]).reshape(-1, 8)
    return out, {int(ids[k]): int(ids[h]) for k, (h, d) in chain.items() if h != k}


def link(rows, model, thr_t=(0, 30), thr_s=75.0, thr_p=0.05, cost=None):
    """End to end in float64 -> (rows, id_map, (pair_i, pair_j, cost))."""
    ids, offsets, r, feats = tracklets(rows)
    pi, pj = gate(offsets, feats, thr_t, thr_s)
    if cost is None:
        cost = net_costs(model, transform(offsets, feats, pi, pj))
    succ, _ = match_full(len(ids), pi, pj, cost, thr_p)
    out, id_map = merge(r, ids, succ)
    return out, id_map, (pi, pj, cost)


# ---- scenes of broken tracks -----------------------------------------------------------------------------------------------------
def scene(seed, objects=24, frames=160):
    """Objects on noisy straight paths, every track cut into fragments with gaps of 1 .. 40 frames, a fresh id per fragment
    (ids shuffled) -> rows [N, 8] by (frame, id)."""
    rng = np.random.default_rng(seed)
    frags = []
    for _ in range(objects):
        p = np.array([rng.uniform(50, 1800), rng.uniform(50, 1000)])
        v = rng.normal(0, 2.5, 2)
        f, f_end = int(rng.integers(1, 40)), int(rng.integers(frames // 2, frames))
        while f < f_end:
            n = int(rng.integers(3, 70))
            fr = np.arange(f, min(f + n, f_end + 1))
            path = p + np.cumsum(v + rng.normal(0, 0.8, (len(fr), 2)), 0)
            frags.append((fr, np.abs(path) + 1.0))
            gap = int(rng.integers(1, 41))
            p = path[-1] + v * gap
            f = int(fr[-1]) + gap
    tids = rng.permutation(len(frags)) + 1
    rows = []
    for tid, (fr, path) in zip(tids, frags):
        blk = np.zeros((len(fr), 8))
        blk[:, 0], blk[:, 1], blk[:, 2], blk[:, 3] = fr, tid, path[:, 0], path[:, 1]
        blk[:, 4], blk[:, 5], blk[:, 6] = path[:, 0] + 40.0, path[:, 1] + 90.0, np.round(rng.uniform(0.3, 1.0, len(fr)), 3)
        rows.append(blk)
    r = np.concatenate(rows, 0)
    return r[np.lexsort((r[:, 1], r[:, 0]))]


def scene_qualifies(rows, model, thr_ps=(0.05, 0.5), margin=1e-4, trials=16):
    """No float64 cost within `margin` of a thr_p, and the SciPy matching unchanged under `trials` seeded perturbations of
    +-margin: a device cost within the margin of the float64 one then gives the same links."""
    ids, offsets, r, feats = tracklets(rows)
    pi, pj = gate(offsets, feats)
    if len(pi) == 0:
        return False
    cost = net_costs(model, transform(offsets, feats, pi, pj))
    rng = np.random.default_rng(len(pi))
    for thr_p in thr_ps:
        if np.abs(cost - thr_p).min() <= margin:
            return False
        base, _ = match_full(len(ids), pi, pj, cost, thr_p)
        if not (base >= 0).any():
            return False
        for _ in range(trials):
            got, _ = match_full(len(ids), pi, pj, cost + rng.choice([-margin, margin], len(cost)), thr_p)
            if not np.array_equal(got, base):
                return False
    return True
