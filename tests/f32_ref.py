"""The fp32 operator kernels of csrc/ss_ops32.hip restated in float64 on the CPU (docs/F32_OPERATORS.md): every operator as a function,
operands on which every product and partial sum is exact in fp32 (so the kernel must EQUAL the reference, whatever order it adds in),
restatements of the launchers' choices of kernel form, the case lists of tests/test_gpu_nets32_exact.py and the ulp arithmetic its
Part B bounds the two transcendental epilogues with.  No GPU import; tests/test_f32_ref_cpu.py checks this file against itself.

Why equality is a fair demand: an fp32 value is m * 2^e with |m| < 2^24.  When every operand of a stage is an integer multiple of one
power of two q (the stage's quantum) and the sum of the ABSOLUTE values of its terms stays below 2^24 q, every partial sum - in any order
and grouping: MFMA blocks, K groups, FMA chains, wave shuffles - is a multiple of q below 2^24 q, hence an fp32 number, and no addition
rounds.  assert_exact() checks that on the ACTUAL tensors of a case and raises OutOfExactRange otherwise.

Tensors here are float64, NCHW; the GPU test lays them out the way each launcher wants.
"""
import numpy as np
import torch
import torch.nn.functional as F

LIMIT = 2.0 ** 24
LOOSE = 5e-6                    # the relative-to-maximum tolerance of tests/test_gpu_nets32.py the mutants are held against


class OutOfExactRange(ValueError):
    pass


# ---------------------------------------------------------------- the exact range
def assert_exact(abs_sum, quantum, what=""):
    """abs_sum: the sum of |term| per output element (or, for sums of non-negative terms, the sum itself)."""
    top = float(abs_sum.abs().max()) / quantum if abs_sum.numel() else 0.0
    if not top < LIMIT:
        raise OutOfExactRange(f"{what}: partial sums reach {top} quanta of {quantum}, past fp32's 2^24")


def assert_multiple(t, quantum, what=""):
    r = t / quantum
    if not bool((r == r.round()).all()) or not bool(torch.isfinite(t).all()):
        raise OutOfExactRange(f"{what}: operand is not an integer multiple of {quantum}")


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def exact_weights(g, s, *shape, density=0.5):
    """{-1, 0, 1} * 2^-s with about `density` of the entries kept."""
    w = _ints(g, -1, 1, *shape) * (torch.rand(*shape, generator=g) < density).double() * 2.0 ** -s
    return w + 0.0                                                       # (-0 -> +0)


def sparse_rows(g, s, rows, cols, nnz=3):
    """[rows, cols] with `nnz` entries of +-2^-s per row."""
    w = torch.zeros(rows, cols, dtype=torch.float64)
    for r in range(rows):
        idx = torch.randperm(cols, generator=g)[:nnz]
        w[r, idx] = (_ints(g, 0, 1, nnz) * 2 - 1) * 2.0 ** -s
    return w


def c1x1(x, w):
    return F.conv2d(x, w.view(w.shape[0], w.shape[1], 1, 1))


# ---------------------------------------------------------------- k32_pw
PW_PAIRS = [(16, 16), (16, 64), (64, 16), (64, 24), (64, 64), (64, 96), (96, 24), (96, 32), (96, 96), (96, 128), (128, 32), (128, 128)]
PW_MS = (105, 16, 64)           # three images of 35 pixels (six tiles and a ragged seventh), one tile, one workgroup exactly
PW_IMG_PX, PW_VALID = 35, 2     # with M = 105: a valid count of 2 cuts M at 70, inside the fifth tile
PW_TPW2 = dict(K=16, N=16, images=257, h=64, w=32)       # M = 526 336 pixels = 32 896 tiles: tiles / 4 = 8 224 > 8 192 -> tpw = 2


def pw_ref(x, w, bias, res=None, relu=True):
    """x [M, K], w [N, K] -> [relu](x w^T + bias (+ res))."""
    y = x @ w.t() + bias
    if res is not None:
        y = y + res
    return y.clamp_min(0) if relu else y


def pw_tpw(M):
    """Tiles per wave and grid of launch_pw32 (RESTATED from csrc/ss_ops32.hip: `while (tpw < 8 && tiles / (4 * tpw) > 8192) tpw *= 2`)."""
    tiles = (M + 15) // 16
    tpw = 1
    while tpw < 8 and tiles // (4 * tpw) > 8192:
        tpw *= 2
    return tpw, (tiles + 4 * tpw - 1) // (4 * tpw)


def exact_pw(K, N, M, s, loud=True):
    """x integers in [-2, 2], w {-1, 0, 1} 2^-s, bias and shortcut integers 2^-s; `loud`: bias[0] = 2^20 quanta, a channel five orders of
    magnitude above the rest - the element a max-relative comparison is scaled by."""
    g = _gen(1, K, N, M, s)
    q = 2.0 ** -s
    x, w = _ints(g, -2, 2, M, K), exact_weights(g, s, N, K)
    bias, res = _ints(g, -16, 16, N) * q, _ints(g, -8, 8, M, N) * q
    if loud:
        bias[0] = 2.0 ** 20 * q
    for t in (x, w, bias, res):
        assert_multiple(t, q, f"pw {(K, N, M, s)}")
    assert_exact(x.abs() @ w.abs().t() + bias.abs() + res.abs(), q, f"pw {(K, N, M, s)}")
    return dict(x=x, w=w, bias=bias, res=res, q=q)


# ---------------------------------------------------------------- the stem
STEM_WALKS = (-1, 1, 2, 4, 8, 16)
STEM_N, STEM_VALID = 3, 2


def stem_ref(x, w, bias, conv1=None):
    """relu(conv7x7/2 + b) -> max pool 3/2/1 (-inf padding); conv1 = (w1 [16, 16], b1): -> (y, relu(w1 y + b1))."""
    y = F.max_pool2d(F.relu(F.conv2d(x, w, bias, 2, 3)), 3, 2, 1)
    if conv1 is None:
        return y
    return y, F.relu(c1x1(y, conv1[0]) + conv1[1].view(1, -1, 1, 1))


def exact_stem(n, s):
    g = _gen(2, n, s)
    q = 2.0 ** -s
    x, w, bias = _ints(g, -2, 2, n, 3, 256, 128), exact_weights(g, s, 16, 3, 7, 7), _ints(g, -16, 16, 16) * q
    assert_exact(F.conv2d(x.abs(), w.abs(), bias.abs(), 2, 3), q, "stem 7x7")
    w1, b1 = exact_weights(g, s, 16, 16), _ints(g, -16, 16, 16) * q * q
    y, y1 = stem_ref(x, w, bias, (w1, b1))
    assert_multiple(y, q, "stem"); assert_multiple(y1, q * q, "stem conv1")
    assert_exact(c1x1(y.abs(), w1.abs()) + b1.abs().view(1, -1, 1, 1), q * q, "stem conv1")
    return dict(x=x, w=w, bias=bias, w1=w1, b1=b1), y, y1


# ---------------------------------------------------------------- the LightConv chains
DEPTHS = (1, 2, 3, 4)
CHAIN_MAPS = [(64, 32, 16), (32, 16, 24), (16, 8, 32)]                    # (H, W, C): the three OSNet-x0.25 stages
CHAIN_NS = (1, 2, 3, 5)
CHAIN_VALID = {(16, 8, 32): [(8, 5), (4, 3), (8, 6)],                     # (N, valid): four images per row-stream workgroup: ends inside a quad, and inside a wave's pair
               (64, 32, 16): [(4, 3), (8, 5)], (32, 16, 24): [(4, 3), (8, 5)]}      # two images per workgroup: ends inside a pair


def lightconv_ref(x, w1, w9, b):
    """w1 [C, C] (out, in; no bias), w9 [C, 3, 3] depthwise taps, b [C]: relu(dw3x3(w1 x) + b)."""
    c = x.shape[1]
    return F.relu(F.conv2d(c1x1(x, w1), w9.view(c, 1, 3, 3), b, 1, 1, 1, c))


def band_sums(y, bands):
    """[N, C, H, W] -> [N, bands, C]: channel sums over each band of H / bands rows, bands in row order."""
    n, c, h, w = y.shape
    return y.reshape(n, c, bands, h // bands, w).sum((3, 4)).permute(0, 2, 1)


def chains_ref(x1, w1, w9, b, bands):
    """The four chains (1, 2, 3, 4 layers; ten layers in that order: w1 [10, C, C], w9 [10, C, 3, 3], b [10, C]) ->
    ([y_1 .. y_4], psum [4, N, bands, C])."""
    ys, l = [], 0
    for t in DEPTHS:
        y = x1
        for _ in range(t):
            y = lightconv_ref(y, w1[l], w9[l], b[l])
            l += 1
        ys.append(y)
    return ys, torch.stack([band_sums(y, bands) for y in ys])


def exact_chains(n, h, w, c, s, bands):
    """x1 integers 0..3 (a ReLU output), 1x1 rows of three +-2^-s, taps {-1, 0, 1} at density 1/2, bias integers in quanta of the layer:
    a layer at depth d of its chain works in quanta of 2^-(s d).  Checked per layer on the actual tensors: |x| through |w1|, |mid| through
    |w9| plus |b|, and (non-negative terms: the sum itself) the channel sums per band and per image."""
    g = _gen(3, n, h, w, c, s)
    x1 = _ints(g, 0, 3, n, c, h, w)
    w1 = torch.stack([sparse_rows(g, s, c, c) for _ in range(10)])
    w9 = exact_weights(g, 0, 10, c, 3, 3)
    b = torch.zeros(10, c, dtype=torch.float64)
    what = f"chains {(n, h, w, c, s)}"
    l = 0
    for t in DEPTHS:
        y = x1
        for d in range(1, t + 1):
            q = 2.0 ** -(s * d)
            b[l] = _ints(g, -2, 2, c) * q
            assert_exact(c1x1(y.abs(), w1[l].abs()), q, what + f" layer {l} 1x1")
            mid = c1x1(y, w1[l])
            assert_exact(F.conv2d(mid.abs(), w9[l].abs().view(c, 1, 3, 3), b[l].abs(), 1, 1, 1, c), q, what + f" layer {l} 3x3")
            y = lightconv_ref(y, w1[l], w9[l], b[l])
            assert_multiple(y, q, what)
            l += 1
        assert_exact(y.sum((2, 3)), 2.0 ** -(s * t), what + f" chain {t} channel sums")
    ys, psum = chains_ref(x1, w1, w9, b, bands)
    for t, y in enumerate(ys):
        if float(y.max()) <= 0 or float((y > 0).double().mean()) < 0.10:
            raise OutOfExactRange(f"{what}: chain {t + 1} is (nearly) dead: {float((y > 0).double().mean()):.3f} positive")
    return dict(x1=x1, w1=w1, w9=w9, b=b), ys, psum


def chains_rows(H, W, C):
    """(rows per band, halo) of the LDS band forms (RESTATED from chains_rows in csrc/ss_ops32.hip; C32_THREADS = 768)."""
    if 2 * H * W * (C + 4) * 4 + 768 * 16 <= 150 * 1024:
        return H, 0
    R = H // 2
    while R >= 8:
        if H % R == 0 and 2 * (R + 8) * W * (C + 4) * 4 + 768 * 16 <= 150 * 1024:
            return R, 4
        R //= 2
    return -1, 4


def chains_form(N, H, W, C, form=2, min_n=128, pre=-1):
    """The kernel ss_op32_chains launches and its band count (RESTATED from chains_rowstream and the CH32C / CH32 lines of
    ss_op32_chains): ("R", C, W) k32_chainsR, ("c3", C, W, PRE) k32_chains3, ("c", C, W) k32_chains."""
    if form == 2 and N >= min_n and (C, W) in ((16, 32), (24, 16), (32, 8)) and H >= 9:
        return ("R", C, W), 1
    R, halo = chains_rows(H, W, C)
    bands = H // R
    if form >= 1 and (C, W) in ((16, 32), (24, 16)) and R + 2 * halo == (24 if C == 16 else 32):
        return ("c3", C, W, (C == 16) if pre < 0 else pre != 0), bands
    return ("c", C, W), bands


ALL_CHAIN_FORMS = frozenset([("R", 16, 32), ("R", 24, 16), ("R", 32, 8), ("c", 16, 32), ("c", 24, 16), ("c", 32, 8)] +
                            [("c3", c, w, p) for c, w in ((16, 32), (24, 16)) for p in (False, True)])


def chain_settings(H, W, C):
    """The (chains_form, chains_min_n, chains_pre) settings the GPU test runs a map under."""
    sets = [(2, 1, -1), (0, 128, -1)]
    if (C, W) != (32, 8):
        sets += [(1, 128, -1), (1, 128, 0), (1, 128, 1)]
    return sets


# ---------------------------------------------------------------- gates and tail
TAIL_INSTS = [(16, 64, 16, 16, False), (16, 64, 0, 64, True), (24, 96, 64, 24, False), (24, 96, 0, 96, True),
              (32, 128, 96, 32, False), (32, 128, 0, 128, False)]         # (MID, C2, C1, N2, POOL) of k32_tail
TAIL_MAP = {16: (64, 32), 24: (32, 16), 32: (16, 8)}
TAIL_N, TAIL_VALID, TAIL_WGS = 5, 3, (0, 1, 3, 7)
TAIL_BANDS = {16: 4, 24: 1, 32: 1}


def gates_ref(psum, hw, gw1, gb1, gw2, gb2):
    """sigmoid(fc2 relu(fc1 mean + b1) + b2) per chain and image: psum [4, N, bands, C] -> [4, N, C], ROUNDED TO FP32 (the gates workspace
    between k32_gates and k32_tail is an fp32 tensor: that is the contract)."""
    mean = psum.sum(2) / hw
    hid = F.relu(mean @ gw1.t() + gb1)
    return torch.sigmoid(hid @ gw2.t() + gb2).float().double()


def tail_ref(ys, gates, w3, b3, xin, down, w4, b4, pool):
    """x2 = sum_t gate_t y_t; o = relu(w3 x2 + b3 + shortcut), shortcut = xin or wd xin + bd (down = (wd, bd)); o2 = relu(w4 o + b4),
    averaged over 2x2 when pool -> (o, o2)."""
    x2 = sum(gates[t][:, :, None, None] * ys[t] for t in range(4))
    sc = xin if down is None else c1x1(xin, down[0]) + down[1].view(1, -1, 1, 1)
    o = F.relu(c1x1(x2, w3) + b3.view(1, -1, 1, 1) + sc)
    o2 = F.relu(c1x1(o, w4) + b4.view(1, -1, 1, 1))
    return o, (F.avg_pool2d(o2, 2, 2) if pool else o2)


def exact_gates(n, mid, h, w, bands, s):
    """Synthetic channel sums and gate weights whose gates are exactly 0, 0.5 or 1 in fp32.
    mean[t, i, c] = an integer 1..3, plus 8 on the (chain, image) pairs P_j[t, i] picks for hidden unit j; fc1 row j = four ones on channels
    of its own, b1 = -16: the hidden value is <= 12 - 16 < 0 -> 0 where P_j is off and >= 36 - 16 = 20 >= 2^-3 where it is on.  fc2 row c
    has ONE entry +-2^12 (or none), b2 = 0: every pre-sigmoid value is 0, >= 20 * 2^12 or <= -20 * 2^12, and 1 / (1 + expf(-v)) is 0.5,
    1 (1 + expf(-v) rounds to 1 from v = 17 on) or 0 (expf overflows to inf from -v = 89 on).  The band sums of a mean m are m H W / bands
    +- small integers that cancel over the bands (so a band left out or taken twice changes the mean)."""
    g = _gen(4, n, mid, s)
    hidden = max(mid // 16, 1)
    hw = h * w
    t_i = torch.arange(4).view(4, 1), torch.arange(n).view(1, n)
    # chains 0, 1: on at every other image (opposite phases); chains 2, 3: on for two images, off for two: four distinct rows, and any two
    # neighbouring images differ in every chain's row or in two of them
    P = [torch.where(t_i[0] < 2, (t_i[1] + t_i[0]) % 2 == 0, (t_i[1] // 2 + t_i[0]) % 2 == 0),
         ((t_i[0] // 2 + t_i[1] // 2) % 2 == 1)][:hidden]
    gw1 = torch.zeros(hidden, mid, dtype=torch.float64)
    mean = _ints(g, 1, 3, 4, n, mid)
    for j in range(hidden):
        ch = torch.arange(4) * hidden + j                                 # channels of hidden unit j
        gw1[j, ch] = 1.0
        mean[:, :, ch] += 8.0 * P[j].double().unsqueeze(-1)
    gb1 = torch.full((hidden,), -16.0, dtype=torch.float64)
    gw2 = torch.zeros(mid, hidden, dtype=torch.float64)
    for c in range(mid):
        k = c % (2 * hidden + 1)                                          # +unit 0, -unit 0, (+unit 1, -unit 1,) none
        if k < 2 * hidden:
            gw2[c, k // 2] = (1.0 if k % 2 == 0 else -1.0) * 2.0 ** 12
    gb2 = torch.zeros(mid, dtype=torch.float64)
    delta = _ints(g, -3, 3, 4, n, bands, mid)
    delta[:, :, bands - 1] = -delta[:, :, :bands - 1].sum(2)              # (one band: 0)
    psum = ((mean * hw / bands).unsqueeze(2) + delta) * 2.0 ** -s         # the chains' quantum 2^-s; fc1 (* 2^s) takes it back
    gw1 = gw1 * 2.0 ** s
    assert_multiple(psum, 2.0 ** -s, "gates psum")
    assert_exact(psum.abs().sum(2), 2.0 ** -s, "gates band sums")
    m = psum.sum(2) / hw
    assert_exact(m.abs() @ gw1.abs().t() + gb1.abs(), 1.0 / hw, "gates fc1")
    hid = F.relu(m @ gw1.t() + gb1)
    if not bool(((hid == 0) | (hid >= 0.125)).all()):
        raise OutOfExactRange("gates: a hidden value in (0, 2^-3)")
    pre = hid @ gw2.t() + gb2
    if not bool(((pre == 0) | (pre >= 32) | (pre <= -128)).all()):
        raise OutOfExactRange("gates: a pre-sigmoid value outside {0} u [32, inf) u (-inf, -128]")
    gates = gates_ref(psum, hw, gw1, gb1, gw2, gb2)
    if not bool(((gates == 0) | (gates == 0.5) | (gates == 1)).all()):
        raise OutOfExactRange("gates: a gate that is not 0, 0.5 or 1")
    return dict(psum=psum, gw1=gw1, gb1=gb1, gw2=gw2, gb2=gb2, hidden=hidden), gates


def gates_are_diverse(gates):
    """All three values occur, and the gates differ between the images of the batch, between the four chains and between channels:
    without that a tail that used another image's (or chain's) gates would still be right."""
    vals = set(gates.unique().tolist()) == {0.0, 0.5, 1.0}
    n = gates.shape[1]
    images = all(not torch.equal(gates[:, i], gates[:, i + 1]) for i in range(n - 1))
    chains = all(not torch.equal(gates[t], gates[u]) for t in range(4) for u in range(t))
    chans = all(len(gates[t, i].unique()) > 1 for t in range(4) for i in range(n) if bool((gates[t, i] != 0.5).any()))
    return vals and images and chains and chans and bool((gates != 0.5).any())


def exact_tail(inst, n, s, loud=True):
    """Synthetic chain outputs (integers 0..3) and channel sums (exact_gates: independent of the chain outputs, the tail takes them as two
    arguments) for one k32_tail instantiation.  Quanta: x2 in 2^-1, conv3 + shortcut in q3 = 2^-(s + 1), the following ConvBR in
    q4 = 2^-(2 s + 1), the 2x2 average in q4 / 4."""
    mid, c2, c1, n2, pool = inst
    h, w = TAIL_MAP[mid]
    g = _gen(5, mid, c2, c1, n2, n, s)
    gw, gates = exact_gates(n, mid, h, w, TAIL_BANDS[mid], s)
    ys = [_ints(g, 0, 3, n, mid, h, w) for _ in range(4)]
    q3, q4 = 2.0 ** -(s + 1), 2.0 ** -(2 * s + 1)
    w3, b3 = exact_weights(g, s, c2, mid), _ints(g, -8, 8, c2) * q3
    if loud:
        b3[0] = 2.0 ** 19 * q3
    what = f"tail {inst} n={n} s={s}"
    x2 = sum(gates[t][:, :, None, None] * ys[t] for t in range(4))
    if c1:
        xin, down = _ints(g, 0, 3, n, c1, h, w), (exact_weights(g, s, c2, c1), _ints(g, -8, 8, c2) * q3)
        sc_abs = c1x1(xin, down[0].abs()) + down[1].abs().view(1, -1, 1, 1)
    else:
        xin, down = _ints(g, 0, 3, n, c2, h, w), None
        sc_abs = xin
    assert_exact(c1x1(x2, w3.abs()) + b3.abs().view(1, -1, 1, 1) + sc_abs, q3, what + " conv3")
    w4, b4 = exact_weights(g, s, n2, c2, density=0.25), _ints(g, -8, 8, n2) * q4
    o, o2 = tail_ref(ys, gates, w3, b3, xin, down, w4, b4, False)
    assert_multiple(o, q3, what); assert_multiple(o2, q4, what)
    assert_exact(c1x1(o, w4.abs()) + b4.abs().view(1, -1, 1, 1), q4, what + " next ConvBR")
    if pool:
        assert_exact(4 * F.avg_pool2d(o2, 2, 2), q4, what + " 2x2 sum")
        o2 = F.avg_pool2d(o2, 2, 2)
    return dict(gw, ys=ys, w3=w3, b3=b3, xin=xin, down=down, w4=w4, b4=b4, gates=gates), o, o2


# ---------------------------------------------------------------- the head
HEAD_CASES = [(3, 512, None), (4, 512, None), (5, 200, None), (7, 512, None), (7, 200, 5), (5, 512, 1)]      # (N, F, valid): four images per workgroup


def head_ref(x, w, bias):
    return F.relu(x.mean((2, 3)) @ w.t() + bias)


def exact_head(n, f, s):
    g = _gen(6, n, f, s)
    x = _ints(g, -2, 2, n, 128, 16, 8)
    q = 2.0 ** -(7 + s)                                                   # the mean of 128 integers, through weights in 2^-s
    w, bias = exact_weights(g, s, f, 128), _ints(g, -64, 64, f) * q
    assert_exact(x.abs().sum((2, 3)), 1.0, "head sum")
    assert_exact(x.abs().mean((2, 3)) @ w.abs().t() + bias.abs(), q, "head fc")
    return dict(x=x, w=w, bias=bias), head_ref(x, w, bias)


# ---------------------------------------------------------------- k32_conv / k32_conv0
def conv_ref(x, w, bias, stride=1, act="none", res=None):
    """act(conv(x) + b) (+ res AFTER the activation); pad k // 2."""
    y = F.conv2d(x, w, bias, stride, w.shape[-1] // 2)
    if act == "silu":
        y = y * torch.sigmoid(y)
    return y if res is None else y + res


def _cv(ks, st, n, h, w, ci, co):
    return dict(ks=ks, st=st, n=n, h=h, w=w, ci=ci, co=co)


# G = ceil(ks^2 Cin / 64) groups of the K walk: 1 (a quarter-filled group), 2, odd, even > 2; 3x3 with Cin 16 / 48 / 80: a group spans four
# taps / straddles taps with 3 / 5 chunks per tap; M = 35: three tiles, one ragged, five (thirteen) idle waves; M = 128: eight waves exactly
CONV_CASES = [_cv(1, 1, 1, 5, 7, 16, 16), _cv(1, 1, 1, 5, 7, 128, 80), _cv(1, 1, 2, 8, 8, 16, 64), _cv(1, 1, 1, 17, 23, 128, 128),
              _cv(1, 1, 1, 17, 23, 256, 32),
              _cv(3, 1, 1, 5, 7, 16, 80), _cv(3, 1, 1, 17, 23, 48, 64), _cv(3, 1, 2, 8, 8, 80, 32), _cv(3, 1, 1, 17, 23, 16, 128),
              _cv(3, 1, 1, 5, 7, 48, 16),
              _cv(3, 2, 1, 17, 23, 16, 80), _cv(3, 2, 1, 17, 23, 48, 64), _cv(3, 2, 2, 16, 16, 80, 32), _cv(3, 2, 1, 9, 13, 16, 16),
              _cv(3, 2, 1, 17, 23, 80, 128)]
CONV_DEFAULTS = dict(conv_mt=0, conv_min=0, conv_waves=0, conv_wgs=1024)


def conv_id(c):
    return f"k{c['ks']}s{c['st']}-{c['n']}x{c['h']}x{c['w']}-{c['ci']}to{c['co']}"


def conv_dims(c):
    """(OH, OW, M, G)."""
    oh, ow = (c["h"] - 1) // c["st"] + 1, (c["w"] - 1) // c["st"] + 1
    return oh, ow, c["n"] * oh * ow, (c["ks"] ** 2 * c["ci"] // 16 + 3) // 4


def conv_settings(c):
    """The option states a case runs under: the default, both wave counts, every forced MT the channel count divides by (at both wave
    counts), a conv_min that reduces MT, and conv_wgs = 1 (the DEFAULT rule then picks eight waves from eight tiles on)."""
    sets = [dict(), dict(conv_waves=4), dict(conv_waves=8), dict(conv_min=1 << 20), dict(conv_wgs=1)]
    for mt in (1, 2, 4, 5):
        if c["co"] % (16 * mt) == 0:
            sets += [dict(conv_mt=mt, conv_waves=4), dict(conv_mt=mt, conv_waves=8)]
    return sets


def exact_conv(c, s, loud=True):
    g = _gen(7, c["ks"], c["st"], c["n"], c["h"], c["w"], c["ci"], c["co"], s)
    q = 2.0 ** -s
    x, w = _ints(g, -2, 2, c["n"], c["ci"], c["h"], c["w"]), exact_weights(g, s, c["co"], c["ci"], c["ks"], c["ks"])
    bias = _ints(g, -16, 16, c["co"]) * q
    if loud:
        bias[0] = 2.0 ** 20 * q
    oh, ow, _, _ = conv_dims(c)
    res = _ints(g, -8, 8, c["n"], c["co"], oh, ow) * q
    assert_exact(F.conv2d(x.abs(), w.abs(), bias.abs(), c["st"], c["ks"] // 2), q, f"conv {conv_id(c)} s={s}")
    return dict(x=x, w=w, bias=bias, res=res, q=q)


CONV0_CASES = [(2, 33, 47), (3, 2, 2)]                                    # (N, H, W)


def exact_conv0(n, h, w, s):
    g = _gen(8, n, h, w, s)
    q = 2.0 ** -s
    x, wt, bias = _ints(g, -3, 3, n, 3, h, w), exact_weights(g, s, 16, 3, 3, 3, density=0.8), _ints(g, -16, 16, 16) * q
    assert_exact(F.conv2d(x.abs(), wt.abs(), bias.abs(), 2, 1), q, "conv0")
    return dict(x=x, w=wt, bias=bias), conv_ref(x, wt, bias, 2)


# ---------------------------------------------------------------- upcat, SPPF (no arithmetic: any fp32 value is exact)
def upcat_ref(lo, hi, lo_first=True):
    up = F.interpolate(lo, scale_factor=2, mode="nearest")
    return torch.cat([up, hi] if lo_first else [hi, up], 1)


def sppf_ref(x, pad=float("-inf")):
    """cat(x, pool5 x, pool5^2 x, pool5^3 x); `pad`: what the pools see outside the map (-inf: the contract; 0: the mutant)."""
    outs = [x]
    for _ in range(3):
        outs.append(F.max_pool2d(F.pad(outs[-1], (2, 2, 2, 2), value=pad), 5, 1, 0))
    return torch.cat(outs, 1)


def negative_map(n, c, h, w, seed=0):
    """fp32 values in [-2^20, -2^-10]: all negative, spread over thirty binades."""
    g = _gen(9, n, c, h, w, seed)
    return -torch.exp2(_ints(g, -10, 20, n, c, h, w)) * (1 + _ints(g, 0, 7, n, c, h, w) / 8)


SPPF_CASES = [(2, 16, 4, 5), (1, 8, 12, 9), (2, 8, 1, 1), (1, 4, 15, 14)]    # (N, C, H, W): smaller than 13 in both axes; past it
UPCAT_CASES = [(2, 8, 16, 3, 5), (1, 4, 4, 1, 1), (3, 16, 8, 4, 7)]          # (N, Cl, Ch, h, w) of lo


# ---------------------------------------------------------------- the v8 decode
DECODE_LEVELS = ((12, 13), (6, 7), (3, 4))                                # A = 156 + 42 + 12 = 210: two 128-anchor blocks, the first level boundary inside the second
DECODE_STRIDES = (8, 16, 32)


def anchor_levels(levels, shift=0):
    """Per anchor a: (level, position in it) - the while loop of k32_v8_decode; `shift` moves every boundary (the mutant)."""
    out = []
    for a in range(sum(h * w for h, w in levels)):
        l, a0 = 0, 0
        while l < 2 and a >= a0 + levels[l][0] * levels[l][1] + shift:
            a0 += levels[l][0] * levels[l][1]
            l += 1
        out.append((l, min(max(a - a0, 0), levels[l][0] * levels[l][1] - 1)))
    return out


def v8_decode_ref(boxes, clss, strides, nc, ext=None, n_ext=0, ext_mode=0, offset=0.5, shift=0, stages=None):
    """boxes[l] [B, 64, H, W], clss[l] [B, >= nc, H, W], ext[l] [B, >= n_ext, H, W] -> pred [B, 4 + nc + n_ext, A].  DFL expectation over
    16 bins per side, dist2bbox around the anchor centre (x + offset, y + offset), times the stride; class sigmoid; ext rows raw (mode 0) or
    keypoint triplets (mode 1: (2 v + x) stride, (2 v + y) stride, sigmoid).  `stages`: receives d, x1, y1, x2, y2 per anchor [B, 4|1.., A]."""
    B = boxes[0].shape[0]
    levels = [tuple(t.shape[2:]) for t in boxes]
    rows = []
    for l, (h, w) in enumerate(levels):
        logit = boxes[l].reshape(B, 4, 16, h * w)
        p = torch.softmax(logit, 2)
        d = (p * torch.arange(16, dtype=torch.float64).view(1, 1, 16, 1)).sum(2)                  # [B, 4, HW]
        gx, gy = torch.arange(w, dtype=torch.float64).repeat(h), torch.arange(h, dtype=torch.float64).repeat_interleave(w)
        x1, y1, x2, y2 = gx + offset - d[:, 0], gy + offset - d[:, 1], gx + offset + d[:, 2], gy + offset + d[:, 3]
        st = float(strides[l])
        r = [(x1 + x2) * 0.5 * st, (y1 + y2) * 0.5 * st, (x2 - x1) * st, (y2 - y1) * st]
        r = [t.unsqueeze(1) for t in r] + [torch.sigmoid(clss[l][:, :nc].reshape(B, nc, h * w))]
        if n_ext:
            e = ext[l][:, :n_ext].reshape(B, n_ext, h * w)
            if ext_mode == 1:
                e = torch.stack([(e[:, k] * 2 + gx) * st if k % 3 == 0 else (e[:, k] * 2 + gy) * st if k % 3 == 1 else torch.sigmoid(e[:, k])
                                 for k in range(n_ext)], 1)
            r.append(e)
        rows.append((torch.cat(r, 1), torch.stack([d[:, 0], d[:, 1], d[:, 2], d[:, 3], x1, y1, x2, y2], 1)))
    idx = anchor_levels(levels, shift)
    if stages is not None:
        stages.append(torch.stack([rows[l][1][:, :, p] for l, p in idx], 2))
    return torch.stack([rows[l][0][:, :, p] for l, p in idx], 2)


def exact_decode(B, nc, n_ext, ext_mode, seed=0, loud=True):
    """One-hot DFL logits (one bin 0, the others -200: expf(-200) is exactly 0, so the expectation is the bin index), class logits in
    {0, 40, -200} (sigmoid exactly 0.5, 1, 0 in fp32), ext values k / 8 (mode 1: the x and y rows are exact; the confidence rows take
    logits in {0, 40, -200} too).  `loud` (mode 0): one raw ext value of 2^21."""
    g = _gen(10, B, nc, n_ext, ext_mode, seed)
    boxes, clss, ext = [], [], []
    pick = torch.tensor([0.0, 40.0, -200.0], dtype=torch.float64)
    for h, w in DECODE_LEVELS:
        bins = torch.randint(0, 16, (B, 4, 1, h, w), generator=g)
        b = torch.full((B, 4, 16, h, w), -200.0, dtype=torch.float64).scatter_(2, bins, 0.0)
        boxes.append(b.reshape(B, 64, h, w))
        clss.append(pick[torch.randint(0, 3, (B, nc + 3, h, w), generator=g)])                   # cls_ld = nc + 3 > nc
        if n_ext:
            e = _ints(g, -64, 64, B, n_ext + 1, h, w) / 8
            if ext_mode == 1:
                e[:, 2::3] = pick[torch.randint(0, 3, e[:, 2::3].shape, generator=g)]
            ext.append(e)
    if n_ext and ext_mode == 0 and loud:
        ext[0][0, 0, 0, 0] = 2.0 ** 21
    return boxes, clss, ext


# ---------------------------------------------------------------- Part B: the two transcendental epilogues
# expf: 1 ulp, the figure of the HIP documentation's math accuracy table ("Math API": expf, maximum ULP error 1) for a build without
# fast-math (csrc/Makefile: -fno-fast-math).  ROCm installs the runtime API reference but not that page: the figure is the published one.
# docs/F32_OPERATORS.md carries the sum.
EXPF_ULP = 1.0
ACT_B = 2.0 * (EXPF_ULP + 0.5 + 0.5)                # (expf + the add 1 + e + the correctly rounded divide), doubled for the binade edge: 4
FLT_MIN = 2.0 ** -126


def ulp32(t):
    """Spacing of the fp32 numbers at |t| (float64 tensor), 2^-149 below the smallest normal."""
    a = t.abs().clamp_min(FLT_MIN)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def act_bound(ref):
    """|kernel - ref| allowed for v / (1 + expf(-v)) and 1 / (1 + expf(-v)) on an exact v: relative errors 2^-23 (expf, 1 ulp; it enters
    1 + e scaled by e / (1 + e) <= 1) + 2^-24 (the add) + 2^-24 (the divide) = 2^-22 <= 4 ulp32(ref)."""
    return (ACT_B * ulp32(ref)).clamp_min(FLT_MIN)


def act_grid():
    """Pre-activations k / 8 in [-16, 16]: 257 values."""
    return torch.arange(-128, 129, dtype=torch.float64) / 8


def silu64(v):
    return v * torch.sigmoid(v)


def act_f32(v, silu):
    """The same formula in numpy float32 (what the CPU check of the bound evaluates)."""
    v = v.numpy().astype(np.float32)
    with np.errstate(over="ignore"):                                      # expf(89) = inf -> 1 / inf = 0: the kernel's arithmetic
        r = (v if silu else np.float32(1)) / (np.float32(1) + np.exp(-v).astype(np.float32))
    return torch.from_numpy(r.astype(np.float64))


DFL_REL = 40.0 * 2.0 ** -24


def dfl_logits(B, seed=0):
    """Box logits k / 8 in [-4, 4] per level."""
    g = _gen(11, B, seed)
    return [_ints(g, -32, 32, B, 64, h, w) / 8 for h, w in DECODE_LEVELS]


def decode_box_bound(st, strides, rel=DFL_REL):
    """Per element bound of the four box rows [B, 4, A] from the reference's own intermediates `st` [B, 8, A] = (d0..d3, x1, y1, x2, y2).
    d = sw / se with e_k = expf(v_k - max) (v_k - max exact, e_k 1 ulp: 2 * 2^-24 relative), se and sw 16-term sums of non-negative terms
    (15 roundings each, 2^-24 relative each; sw one more per product e_k * k), the quotient correctly rounded (2^-24):
    (2 + 15) + (2 + 1 + 15) + 1 = 36 units of 2^-24, taken as 40 for the second-order terms: |dd| <= DFL_REL d.
    x1 = ax - d0, x2 = ax + d2 and their sum / difference round once each: at most ulp32 of the reference value (a full ulp where half
    would do: the kernel's value may sit in the next binade); * 0.5 and * stride (a power of two) are exact."""
    d, p = st[:, :4], st[:, 4:]
    dd = rel * d                                                          # (rel: the half kernel re-derives it for __expf, tests/f16_ref.py)
    strides_a = torch.tensor([float(strides[l]) for l, _ in anchor_levels(DECODE_LEVELS)], dtype=torch.float64).view(1, 1, -1)
    ex = dd[:, 0] + dd[:, 2] + ulp32(p[:, 0]) + ulp32(p[:, 2])
    ey = dd[:, 1] + dd[:, 3] + ulp32(p[:, 1]) + ulp32(p[:, 3])
    b = torch.stack([(ex + ulp32(p[:, 0] + p[:, 2])) * 0.5, (ey + ulp32(p[:, 1] + p[:, 3])) * 0.5,
                     ex + ulp32(p[:, 2] - p[:, 0]), ey + ulp32(p[:, 3] - p[:, 1])], 1)
    return b * strides_a


def decode_boxes_f32(boxes, strides):
    """The box rows of k32_v8_decode in numpy float32, sums in bin order (the CPU check of decode_box_bound)."""
    f = np.float32
    B = boxes[0].shape[0]
    per = []
    for l, t in enumerate(boxes):
        h, w = t.shape[2:]
        v = t.reshape(B, 4, 16, h * w).numpy().astype(f)
        e = np.exp(v - v.max(2, keepdims=True)).astype(f)
        se, sw = np.zeros((B, 4, h * w), f), np.zeros((B, 4, h * w), f)
        for k in range(16):
            se = (se + e[:, :, k]).astype(f)
            sw = (sw + (e[:, :, k] * f(k)).astype(f)).astype(f)
        d = (sw / se).astype(f)
        gx, gy = np.tile(np.arange(w, dtype=f), h) + f(0.5), np.repeat(np.arange(h, dtype=f), w) + f(0.5)
        x1, y1, x2, y2 = gx - d[:, 0], gy - d[:, 1], gx + d[:, 2], gy + d[:, 3]
        st = f(strides[l])
        per.append(np.stack([(x1 + x2) * f(0.5) * st, (y1 + y2) * f(0.5) * st, (x2 - x1) * st, (y2 - y1) * st], 1).astype(np.float64))
    return torch.from_numpy(np.concatenate(per, 2))


# ---------------------------------------------------------------- what a max-relative comparison lets through
def hidden_from_loose(mut, ref, rel=LOOSE):
    """Elements where the mutant differs from the reference by no more than rel * max |ref|: what `max |got - ref| <= rel * max |ref|`
    does not see (when every differing element is such an element, that comparison passes the mutant whole)."""
    d = (mut - ref).abs()
    return (d > 0) & (d <= rel * float(ref.abs().max()))
