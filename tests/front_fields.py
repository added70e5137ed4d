"""Inputs and a plain reference for the front-end edge tests (tests/test_front_edges_cpu.py, tests/test_gpu_front_edges.py).

nms_field builds head tensors with a chosen number of candidates in clusters whose members are spread over the whole sorted order;
plain_nms is a float64 greedy NMS that shares nothing with oracle/csrc/ss_oracle.c (no class offset, no float32 box arithmetic);
known_answers are fields whose result follows from the definition of the operation; the crop box lists are the edge boxes of
tests/test_gpu_front.py::test_crop_norm_batch_bit_exact and a set for frames a few dozen pixels wide."""
import numpy as np

# (n_cand, per) of the clustered fields the CPU file pins against plain_nms; the GPU file takes `per` for its counts from PER_OF
FIELD_PAIRS = [(63, 5), (64, 5), (65, 5), (130, 5), (1024, 8), (1025, 8), (4095, 24), (4096, 24), (4097, 24), (8191, 24), (8192, 24),
               (8192, 5), (5000, 4)]
# seed of a field, where the default (0) leaves an IoU closer to the threshold than the float32 class offset can move it
SEEDS = {}


def PER_OF(n_cand):
    return 5 if n_cand < 1024 else 8 if n_cand <= 1025 else 24


def nms_field(n_cand, per, N=8400, nc=2, seed=0):
    """n_cand anchors above conf in clusters of ~per mutually overlapping boxes on a grid of centres 80 px apart
    (clusters never touch), classes alternating inside a cluster, a fifth of the scores tied; the rest of the N anchors score 0."""
    rng = np.random.default_rng([seed, n_cand, per])
    pred = np.zeros((4 + nc, N), np.float32)
    pred[0] = rng.uniform(0, 3000, N); pred[1] = rng.uniform(0, 3000, N)
    pred[2] = rng.uniform(10, 60, N); pred[3] = rng.uniform(10, 60, N)
    idx = rng.choice(N, n_cand, replace=False)
    C = max(1, -(-n_cand // per)); side = int(np.ceil(np.sqrt(C)))
    for j, a in enumerate(idx):
        c = j % C
        pred[0, a] = 100 + 80 * (c % side) + rng.uniform(-6, 6); pred[1, a] = 100 + 80 * (c // side) + rng.uniform(-6, 6)
        pred[2, a] = 40 + rng.uniform(-4, 4); pred[3, a] = 50 + rng.uniform(-4, 4)
        pred[4 + (j // C) % nc, a] = [0.9, 0.8, 0.7][j % 3] if j % 5 == 0 else rng.uniform(0.35, 0.95)
    return pred


def field(n_cand, per=None, **kw):
    """nms_field at the seed this module pins for (n_cand, per)"""
    per = PER_OF(n_cand) if per is None else per
    return nms_field(n_cand, per, seed=SEEDS.get((n_cand, per), 0), **kw)


def sorted_candidates(pred, nc, conf):
    """-> (anchors in the order the NMS visits them, their classes): best class per anchor (first maximum), score > float32(conf),
    descending score, ties to the lower anchor."""
    sc = pred[4:4 + nc]
    cls = sc.argmax(axis=0)                                          # first maximum = lowest class
    best = sc[cls, np.arange(sc.shape[1])]
    cand = np.nonzero(best > np.float32(conf))[0]
    order = cand[np.argsort(-best[cand].astype(np.float64), kind="stable")]
    return order, cls[order]


def plain_nms(pred, nc, conf, iou, agnostic, max_det):
    """float64 greedy NMS -> (kept anchors int32, smallest |IoU - iou| among the pairs it decided, inf when it decided none).
    A pair is decided when a kept box meets a later box that is still alive (and of its class, unless agnostic)."""
    order, cls = sorted_candidates(pred, nc, conf)
    p = pred[:4, order].astype(np.float64)
    x1, y1, x2, y2 = p[0] - p[2] / 2, p[1] - p[3] / 2, p[0] + p[2] / 2, p[1] + p[3] / 2
    area = (x2 - x1) * (y2 - y1)
    thr = float(np.float32(iou))
    alive = np.ones(len(order), bool)
    kept, margin = [], np.inf
    for i in range(len(order)):
        if len(kept) >= max_det:
            break
        if not alive[i]:
            continue
        kept.append(order[i])
        m = alive[i + 1:] if agnostic else alive[i + 1:] & (cls[i + 1:] == cls[i])
        j = i + 1 + np.nonzero(m)[0]
        if not len(j):
            continue
        iw = np.maximum(0.0, np.minimum(x2[i], x2[j]) - np.maximum(x1[i], x1[j]))
        ih = np.maximum(0.0, np.minimum(y2[i], y2[j]) - np.maximum(y1[i], y1[j]))
        inter = iw * ih
        with np.errstate(invalid="ignore", divide="ignore"):
            v = inter / (area[i] + area[j] - inter)                  # 0 / 0 (two empty boxes) is not above any threshold
        ok = np.isfinite(v)
        if ok.any():
            margin = min(margin, float(np.abs(v[ok] - thr).min()))
        alive[j[ok & (v > thr)]] = False
    return np.asarray(kept, np.int32), margin


def suppressed_past(pred, nc, conf, keep, max_det, rank=4096):
    """number of candidates of sorted rank >= `rank` the greedy pass dropped by suppression: not kept, and met while fewer than
    max_det were kept (everything behind the max_det-th kept box is cut off, not suppressed)."""
    order, _ = sorted_candidates(pred, nc, conf)
    pos = {int(a): r for r, a in enumerate(order)}
    stop = len(order) if len(keep) < max_det else pos[int(keep[-1])]
    kept = set(int(a) for a in keep)
    return sum(1 for r in range(rank, stop) if int(order[r]) not in kept)


# ---- known answers ---------------------------------------------------------------------------------------------------------------
KNOWN_N = 3200          # anchors of a known-answer field
KNOWN_CONF = 0.3
N_PAD = 70


def _blank(nc):
    return np.zeros((4 + nc, KNOWN_N), np.float32)


def known_answers():
    """-> list of dicts: name, pred, nc, conf, iou, keep (anchors in output order), cls (their classes).  Every answer follows from
    the definition of the operation, not from an implementation."""
    out = []
    half_lo = float(np.nextafter(np.float32(0.5), np.float32(0)))
    for c in (0, 1):                                                 # IoU exactly 0.5 in float32, with the class offset too
        pred = _blank(2)
        pred[:4, 10] = [1.5, 0.5, 3, 1]; pred[:4, 20] = [2.5, 0.5, 3, 1]
        pred[4 + c, 10] = 0.9; pred[4 + c, 20] = 0.8
        out.append(dict(name=f"iou_half_at_half_cls{c}", pred=pred, nc=2, conf=KNOWN_CONF, iou=0.5, keep=[10, 20], cls=[c, c]))
        out.append(dict(name=f"iou_half_below_half_cls{c}", pred=pred, nc=2, conf=KNOWN_CONF, iou=half_lo, keep=[10], cls=[c]))
    pred = _blank(2)                                                 # 70 identical empty boxes: 0 / 0 suppresses nothing
    pred[:4, 100:170] = np.array([[300.0], [200.0], [0.0], [40.0]], np.float32)
    pred[4, 100:170] = 0.9
    out.append(dict(name="zero_area", pred=pred, nc=2, conf=KNOWN_CONF, iou=0.4, keep=list(range(100, 170)), cls=[0] * 70))
    pred = _blank(2)                                                 # score == float32(conf) is no candidate, the next float is
    c32 = np.float32(KNOWN_CONF)
    for k, a in enumerate((5, 6, 7)):
        pred[:4, a] = [50.0 + 100 * k, 500.0, 20.0, 20.0]
    pred[4, 5] = c32; pred[5, 6] = np.nextafter(c32, np.float32(1)); pred[4, 7] = np.nextafter(c32, np.float32(0))
    out.append(dict(name="conf_edge", pred=pred, nc=2, conf=KNOWN_CONF, iou=0.4, keep=[6], cls=[1]))
    pred = _blank(3)                                                 # bit-equal best scores in two classes: the lower class
    pred[:4, 40] = [50.0, 700.0, 20.0, 20.0]; pred[:4, 41] = [150.0, 700.0, 20.0, 20.0]
    pred[4:7, 40] = [0.1, 0.8, 0.8]; pred[4:7, 41] = [0.7, 0.2, 0.7]
    out.append(dict(name="class_tie", pred=pred, nc=3, conf=KNOWN_CONF, iou=0.4, keep=[40, 41], cls=[1, 0]))
    pred = _blank(2)                                                 # 3000 identical boxes, equal scores: the lowest anchor
    pred[:4, :3000] = np.array([[100.0], [100.0], [50.0], [80.0]], np.float32)
    pred[4, :3000] = 0.9
    out.append(dict(name="identical_3000", pred=pred, nc=2, conf=KNOWN_CONF, iou=0.4, keep=[0], cls=[0]))
    return out


def padded(case):
    """the same field with N_PAD unrelated candidates far from everything else (the image then takes the workgroup path); they
    score below every score of the case, descending with the anchor, so all of them follow the case's own rows in anchor order."""
    pred = case["pred"].copy()
    pads = list(range(KNOWN_N - N_PAD, KNOWN_N))
    for k, a in enumerate(pads):
        pred[:4, a] = [1000.0 + 100.0 * (k % 20), 2000.0 + 100.0 * (k // 20), 10.0, 10.0]
        pred[4, a] = np.float32(0.39) - np.float32(0.001) * np.float32(k)
    lo = min(float(pred[4 + c, a]) for a, c in zip(case["keep"], case["cls"]))
    assert lo > 0.39 or case["name"] == "conf_edge"
    d = dict(case, name=case["name"] + "_padded", pred=pred)
    if case["name"] == "conf_edge":                                  # its one candidate scores below the pads
        d["keep"], d["cls"] = pads + case["keep"], [0] * N_PAD + case["cls"]
    else:
        d["keep"], d["cls"] = case["keep"] + pads, case["cls"] + [0] * N_PAD
    return d


# ---- crop boxes ------------------------------------------------------------------------------------------------------------------
def edge_boxes(W, H):
    """the boxes at which the crop kernels change path: clipped at each border, one pixel wide / high, sub-pixel, the full frame (no
    staging), the last bytes of the frame, tall boxes that stage 16 rows at a time, every byte alignment of the first column"""
    b = [[-5.0, -3.0, 20.5, 30.2], [W - 10.0, H - 12.0, W + 50.0, H + 50.0], [-8.0, H - 40.0, 60.0, H + 9.0], [W - 33.0, -4.0, W + 2.0, 70.0],
         [0.0, 0.0, W, H], [W - 3.0, H - 2.0, W, H], [101.0, 50.0, 102.5, 400.0], [30.0, 300.0, 500.0, 301.2], [100.0, 100.0, 100.4, 100.3],
         [300.0, 60.0, 520.0, 560.0], [701.0, 150.0, 990.0, H + 4.0]]
    b += [[200.0 + j, 100.0, 260.0 + 2 * j, 290.0] for j in range(2, 6)]
    return np.asarray(b, np.float32)


def packed_case(W=1280, H=720, B=4, cap=40, seed=77):
    """-> (dets [B, cap, 6] float32, counts): random boxes, the edge boxes spread over the images that have any (first rows, so
    every count covers them)"""
    rng = np.random.default_rng(seed)
    x1 = rng.uniform(-10, W - 40, (B, cap)); y1 = rng.uniform(-10, H - 60, (B, cap))
    bw = rng.uniform(0.3, 500, (B, cap)); bh = rng.uniform(0.3, 650, (B, cap))
    dets = np.stack([x1, y1, x1 + bw, y1 + bh, np.ones((B, cap)), np.zeros((B, cap))], 2).astype(np.float32)
    counts = [32, 0, 17, 40]
    e = edge_boxes(W, H)
    live = [i for i in range(B) if counts[i] > 0]
    for k, box in enumerate(e):
        dets[live[k % len(live)], k // len(live), :4] = box
    return dets, counts


def small_frame_boxes(W, H):
    """n = 8 boxes of a frame a few dozen pixels wide: the full frame, the last pixel, the first pixel, clipped, sub-pixel, every
    residue of x1 mod 4"""
    b = [[0.0, 0.0, W, H], [W - 1.0, H - 1.0, W, H], [0.0, 0.0, 1.0, 1.0], [-3.0, -2.0, 9.5, 11.0], [5.0, 7.0, 5.3, 7.2],
         [1.0, 3.0, W - 2.0, H - 1.0], [2.0, 0.0, 17.0, H], [3.0, 9.0, W + 5.0, 20.0]]
    d = np.zeros((8, 6), np.float32)
    d[:, :4] = np.asarray(b, np.float32); d[:, 4] = 1.0
    return d
