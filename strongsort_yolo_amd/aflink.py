"""AFLink, appearance-free tracklet linking: the network half of StrongSORT++'s post-processing (docs/AFLINK.md).

Rows are the float64 [N, 8] rows of `strongsort_yolo_amd.gsi`: frame, id, x1, y1, x2, y2, conf, cls.  A tracklet is the rows of one
id in rising frame order; tracklets are numbered 0 .. n-1 by rising id.  `costs` gates the n x n tracklet ends and runs the
PostLinker network on every candidate pair, `link` matches the pairs below thr_p and merges the linked tracklets; gate, input
transform, network and matching run on the device (csrc/ss_aflink.hip).  There is no CPU fallback: without the library or a
device both raise as the rest of the package does.  `PostLinker` is the CPU PyTorch form of the network and carries upstream's
parameter names, so `load` takes a trained checkpoint's state_dict; without one the network runs from its seeded random
initialisation like every network here.  tests/aflink_ref.py restates every step.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import lib as _lib
from .gsi import _sorted

LEN = 30                                # rows of a tracklet the network sees
THR_T, THR_S, THR_P = (0, 30), 75.0, 0.05
CHANNELS = (1, 32, 64, 128, 256)
MAX_COMPONENT = 256                     # ss_aflink_max_component()
BM = 64                                 # GEMM rows per workgroup (csrc/ss_aflink.hip): 54, 36, 18 and 6 rows a pair in the four wide layers
CHUNK = 1024                            # ss_op_set_option "aflink_chunk"


class TemporalBlock(nn.Module):
    """Conv2d(kernel (7, 1), no bias) along time, shared by the three columns; one BatchNorm1d per column; ReLU."""

    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, (7, 1), bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.bnf = nn.BatchNorm1d(cout)
        self.bnx = nn.BatchNorm1d(cout)
        self.bny = nn.BatchNorm1d(cout)

    def forward(self, x):
        x = self.conv(x)
        x = torch.stack([self.bnf(x[:, :, :, 0]), self.bnx(x[:, :, :, 1]), self.bny(x[:, :, :, 2])], 3)
        return self.relu(x)


class FusionBlock(nn.Module):
    """Conv2d(kernel (1, 3), no bias) across the three columns; BatchNorm2d; ReLU."""

    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, (1, 3), bias=False)
        self.bn = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.relu(self.bn(self.conv(x)))


class Classifier(nn.Module):
    def __init__(self, cin: int):
        super().__init__()
        self.fc1 = nn.Linear(cin * 2, cin // 2)
        self.relu = nn.ReLU(inplace=True)
        self.fc2 = nn.Linear(cin // 2, 2)

    def forward(self, x1, x2):
        return self.fc2(self.relu(self.fc1(torch.cat((x1, x2), 1))))


class PostLinker(nn.Module):
    """x1, x2: [B, 1, 30, 3] (frame, x1, y1 of the earlier and the later tracklet, normalised jointly) -> [B, 2]: logits while
    training, softmax probabilities in eval mode.  cost = 1 - p[:, 1]."""

    def __init__(self, seed: int | None = 0):
        super().__init__()
        if seed is not None:
            state = torch.random.get_rng_state()
            torch.manual_seed(seed)
        c = CHANNELS
        self.TemporalModule_1 = nn.Sequential(*[TemporalBlock(c[k], c[k + 1]) for k in range(4)])
        self.TemporalModule_2 = nn.Sequential(*[TemporalBlock(c[k], c[k + 1]) for k in range(4)])
        self.FusionBlock_1 = FusionBlock(c[4], c[4])
        self.FusionBlock_2 = FusionBlock(c[4], c[4])
        self.pooling = nn.AdaptiveAvgPool2d((1, 1))
        self.classifier = Classifier(c[4])
        if seed is not None:
            torch.random.set_rng_state(state)
        self.eval()

    def features(self, x1, x2):
        x1 = self.FusionBlock_1(self.TemporalModule_1(x1[:, :, :, :3]))
        x2 = self.FusionBlock_2(self.TemporalModule_2(x2[:, :, :, :3]))
        return self.pooling(x1).flatten(1), self.pooling(x2).flatten(1)

    def forward(self, x1, x2):
        y = self.classifier(*self.features(x1, x2))
        return y if self.training else torch.softmax(y, 1)


def load(path_or_state_dict, seed: int | None = 0) -> PostLinker:
    """A PostLinker with the weights of a checkpoint file (torch.load; a dict with a "state_dict" entry is unwrapped) or of a
    state_dict.  Strict: a missing, unexpected or misshapen key is a ValueError that names it."""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        sd = torch.load(sd, map_location="cpu", weights_only=True)
    if "state_dict" in sd and not any(k.startswith("TemporalModule_1") for k in sd):
        sd = sd["state_dict"]
    model = PostLinker(seed)
    want = model.state_dict()
    missing = [k for k in want if k not in sd]
    if missing:
        raise ValueError(f"aflink.load: missing key {missing[0]!r}" + (f" and {len(missing) - 1} more" if len(missing) > 1 else ""))
    extra = [k for k in sd if k not in want]
    if extra:
        raise ValueError(f"aflink.load: unexpected key {extra[0]!r}" + (f" and {len(extra) - 1} more" if len(extra) > 1 else ""))
    for k, v in want.items():
        if tuple(sd[k].shape) != tuple(v.shape):
            raise ValueError(f"aflink.load: key {k!r} has shape {tuple(sd[k].shape)}, not {tuple(v.shape)}")
    model.load_state_dict(sd, strict=True)
    return model.eval()


def _fold(bn):
    """BatchNorm with its running statistics as scale, bias in float64."""
    g, b = bn.weight.detach().double().numpy(), bn.bias.detach().double().numpy()
    m, v = bn.running_mean.detach().double().numpy(), bn.running_var.detach().double().numpy()
    scale = g / np.sqrt(v + bn.eps)
    return scale, b - m * scale


def parts(model: PostLinker) -> dict:
    """The folded network in float64, keyed as the blob is laid out (docs/AFLINK.md §3): per branch b = 0, 1 and temporal layer
    l = 1 .. 4 `w{l}_{b}` [cout, 7 * cin] (k = 7 taps x cin channels, tap-major) and `sb{l}_{b}` [2, 3, cout] (scale, bias per column);
    `wf_{b}` [256, 3 * 256] (column-major k) and `sbf_{b}` [2, 256]; `fc1t` [512, 128], `b1`, `fc2` [2, 128], `b2`."""
    out = {}
    for b, (tm, fb) in enumerate(((model.TemporalModule_1, model.FusionBlock_1), (model.TemporalModule_2, model.FusionBlock_2))):
        for l, blk in enumerate(tm, 1):
            w = blk.conv.weight.detach().double().numpy()[:, :, :, 0]                   # [cout, cin, 7]
            out[f"w{l}_{b}"] = np.ascontiguousarray(w.transpose(0, 2, 1)).reshape(w.shape[0], -1)
            out[f"sb{l}_{b}"] = np.stack([np.stack(c) for c in zip(*(_fold(bn) for bn in (blk.bnf, blk.bnx, blk.bny)))])
        w = fb.conv.weight.detach().double().numpy()[:, :, 0, :]                        # [cout, cin, 3]
        out[f"wf_{b}"] = np.ascontiguousarray(w.transpose(0, 2, 1)).reshape(w.shape[0], -1)
        out[f"sbf_{b}"] = np.stack(_fold(fb.bn))
    c = model.classifier
    out["fc1t"] = np.ascontiguousarray(c.fc1.weight.detach().double().numpy().T)
    out["b1"] = c.fc1.bias.detach().double().numpy()
    out["fc2"] = c.fc2.weight.detach().double().numpy()
    out["b2"] = c.fc2.bias.detach().double().numpy()
    return out


def _layout():
    keys = []
    for b in range(2):
        for l in range(1, 5):
            keys += [(f"w{l}_{b}", (CHANNELS[l], 7 * CHANNELS[l - 1])), (f"sb{l}_{b}", (2, 3, CHANNELS[l]))]
        keys += [(f"wf_{b}", (256, 768)), (f"sbf_{b}", (2, 256))]
    return keys + [("fc1t", (512, 128)), ("b1", (128,)), ("fc2", (2, 128)), ("b2", (2,))]


LAYOUT = _layout()
WEIGHT_FLOATS = sum(int(np.prod(s)) for _, s in LAYOUT)             # ss_aflink_weight_floats()


def pack(model: PostLinker) -> np.ndarray:
    """The weight blob of ss_aflink_set_weights: the BatchNorms folded in float64, everything rounded to float32 once."""
    p = parts(model)
    return np.concatenate([p[k].reshape(-1) for k, _ in LAYOUT]).astype(np.float32)


def unpack(blob) -> dict:
    """The arrays of `parts` back out of a blob (float32)."""
    blob = np.asarray(blob, np.float32).reshape(-1)
    if len(blob) != WEIGHT_FLOATS:
        raise ValueError(f"aflink.unpack: {len(blob)} floats, not {WEIGHT_FLOATS}")
    out, at = {}, 0
    for k, s in LAYOUT:
        n = int(np.prod(s))
        out[k] = blob[at:at + n].reshape(s)
        at += n
    return out


def folded_costs(p: dict, x) -> np.ndarray:
    """The folded network of `parts` / `unpack` on inputs x [pairs, 2, 30, 3] in float64 -> cost [pairs]: the arithmetic the device
    does, written with NumPy (a CPU check of the blob's layout, not a fallback: `costs` never calls it)."""
    x = np.asarray(x, np.float64)
    pooled = []
    for b in range(2):
        a = x[:, b].transpose(0, 2, 1)[..., None]                                       # [pairs, column, step, cin]
        for l in range(1, 5):
            t_out = a.shape[2] - 6
            win = np.concatenate([a[:, :, d:d + t_out] for d in range(7)], 3)             # k = tap-major
            sb = np.asarray(p[f"sb{l}_{b}"], np.float64)
            a = np.maximum(win @ np.asarray(p[f"w{l}_{b}"], np.float64).T * sb[0][None, :, None, :] + sb[1][None, :, None, :], 0.0)
        f = a.transpose(0, 2, 1, 3).reshape(len(x), a.shape[2], -1)                      # [pairs, step, column * 256 + c]
        sb = np.asarray(p[f"sbf_{b}"], np.float64)
        f = np.maximum(f @ np.asarray(p[f"wf_{b}"], np.float64).T * sb[0] + sb[1], 0.0)
        pooled.append(f.mean(1))
    h = np.maximum(np.concatenate(pooled, 1) @ np.asarray(p["fc1t"], np.float64) + np.asarray(p["b1"], np.float64), 0.0)
    y = h @ np.asarray(p["fc2"], np.float64).T + np.asarray(p["b2"], np.float64)
    e = np.exp(y - y.max(1, keepdims=True))
    return 1.0 - e[:, 1] / e.sum(1)


def tracklets(rows):
    """-> (ids rising, offsets [n + 1] int32, rows by (id, frame), feats [rows, 3] = frame, x1, y1)."""
    r = np.array(rows, np.float64, copy=True).reshape(-1, 8)
    r = r[np.lexsort((r[:, 0], r[:, 1]))]
    ids, counts = np.unique(r[:, 1], return_counts=True)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return ids, offsets, r, np.ascontiguousarray(r[:, [0, 2, 3]])


def _set_weights(engine, model):
    """Upload the model's blob unless the engine holds it already.  The key is the model and the version counter of every parameter
    and buffer, which PyTorch raises on each in-place change: a model that was loaded into or trained since (load_state_dict,
    an optimiser step) is packed and uploaded again; only writes that bypass autograd's counter (through .data or NumPy) are missed."""
    tensors = list(model.state_dict(keep_vars=True).values())
    key = (id(model), tuple(t.data_ptr() for t in tensors), tuple(t._version for t in tensors))
    if getattr(engine, "_aflink_key", None) != key:
        engine.aflink_set_weights(pack(model))
        engine._aflink_key = key


def costs(rows, engine, model: PostLinker, thr_t=THR_T, thr_s: float = THR_S):
    """-> (pair_i, pair_j, cost): the candidate pairs of tracklets (numbered by rising id), row-major, and the network's cost
    1 - p[1] of each, all on the device."""
    _, offsets, _, feats = tracklets(rows)
    if len(offsets) < 2:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)
    _set_weights(engine, model)
    return engine.aflink_cost(offsets, feats, thr_t, thr_s)


def chains(successor):
    """successor [n] (-1 or the tracklet linked behind) -> (head [n], depth [n]): the first tracklet of every tracklet's chain and
    its distance from it.  A successor out of range, a tracklet that is the successor of two others, or a cycle is a ValueError."""
    succ = np.asarray(successor, np.int64).reshape(-1)
    n = len(succ)
    linked = np.nonzero(succ >= 0)[0]
    if ((succ < -1) | (succ >= n)).any():
        raise ValueError("aflink.merge: a successor is out of range")
    if len(np.unique(succ[linked])) != len(linked):
        raise ValueError("aflink.merge: a tracklet is the successor of two others")
    pred = np.full(n, -1, np.int64)
    pred[succ[linked]] = linked
    head, depth, seen = np.arange(n), np.zeros(n, np.int64), pred < 0
    for k in np.nonzero(pred < 0)[0]:                                                   # walk every chain once, from its head
        h, d = int(k), 0
        while succ[h] >= 0:
            h, d = int(succ[h]), d + 1
            head[h], depth[h], seen[h] = k, d, True
    if not seen.all():                                                                  # no head leads here: the links run in a circle
        raise ValueError(f"aflink.merge: the links form a cycle through tracklet {int(np.nonzero(~seen)[0][0])}")
    return head, depth


def merge(rows, ids, successor):
    """Give every linked tracklet the id of the head of its chain, drop the later tracklet's row where two rows then share
    (frame, id) -> (rows by (frame, id), {id: head id} of the tracklets that changed).  The gate only links a tracklet to one
    that starts later (ties: the larger number), so its links have no cycle; a successor array that has one is refused."""
    ids = np.asarray(ids, np.float64)
    head, depth = chains(successor)
    if len(head) != len(ids):
        raise ValueError("aflink.merge: one successor per id")
    r = np.array(rows, np.float64, copy=True).reshape(-1, 8)
    idx = np.searchsorted(ids, r[:, 1])
    r[:, 1] = ids[head[idx]]
    # per (frame, id) keep the row of the tracklet nearest the head of its chain
    r = r[np.lexsort((depth[idx], r[:, 1], r[:, 0]))]
    keep = np.ones(len(r), bool)
    keep[1:] = (r[1:, 0] != r[:-1, 0]) | (r[1:, 1] != r[:-1, 1])
    return _sorted(r[keep]), {int(ids[k]): int(ids[head[k]]) for k in range(len(ids)) if head[k] != k}


def link(rows, engine, model: PostLinker, thr_t=THR_T, thr_s: float = THR_S, thr_p: float = THR_P, info: dict | None = None):
    """-> (rows by (frame, id), {id: the id it was given}).  `info`, when a dict, receives the counts `candidates` and `links`."""
    ids, offsets, r, feats = tracklets(rows)
    if len(ids) == 0:
        if info is not None:
            info.update(candidates=0, links=0)
        return r, {}
    _set_weights(engine, model)
    pi, pj, cost = engine.aflink_cost(offsets, feats, thr_t, thr_s)
    succ = engine.aflink_match(len(ids), pi, pj, cost, thr_p)
    if info is not None:
        info.update(candidates=int(len(pi)), links=int((succ >= 0).sum()))
    return merge(r, ids, succ)


def weight_floats() -> int:
    return int(_lib.load().ss_aflink_weight_floats())


def max_component() -> int:
    return int(_lib.load().ss_aflink_max_component())
