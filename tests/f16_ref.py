"""The f16 operator kernels of csrc/ss_ops.hip restated in float64 on the CPU (docs/F16_OPERATORS.md): the rounding chain of every
operator as a function, operands on which that chain is exact, a restatement of launch_pw's choice of kernel form, and the half-ulp
arithmetic the GPU tests bound their errors with.  No GPU import; tests/test_f16_ref_cpu.py checks this file against itself
(coverage of the forms, mutants), tests/test_gpu_nets_exact.py checks the kernels against it.

Notation: h(.) rounds to half (one rounding, to nearest even), acc is the kernel's fp32 sum of products.
    pointwise / conv3x3 / conv0 (pw_body, pw_splitk_body, k_conv0):
        c = h(acc); f = c + bias (+ res, when it is added before the activation); f = act(f); with res_after: f = h(f) + res; out = h(f)
    k_osnet_stem:   h(relu(h(conv7x7/2) + bias)), max pool 3/2/1; optional conv1: h(relu(h(pw(y)) + b1))
    k_lightconv:    mid = h(pw(x)); out = relu(h(bias + nine taps of mid in fp32))
    k_osnet_head:   m = h(sum_hw / HW); out = h(relu(h(fc(m)) + bias))
    k_avgpool2:     h((((a + b) + c) + d) / 4)  - ONE rounding to half, of the fp32 sum
    k_bias_act8/1:  h(act(x + bias (+ res)));  k_bias_act_place: the pointwise epilogue on an x that is already half
The depthwise 3x3, max pooling, the C2PSA attention, the half decode and the aggregation gate follow at the end of the file.
"""
import numpy as np
import torch
import torch.nn.functional as F

ACTS = ("none", "relu", "silu", "sigmoid")
LIPSCHITZ = {"none": 1.0, "relu": 1.0, "silu": 1.1, "sigmoid": 0.25}     # max |act'|: silu' peaks at 1.0998 (x = 2.4)


# ---------------------------------------------------------------- half arithmetic on float64 values
def h(t):
    """float64 tensor rounded to half and back, in ONE rounding (numpy's double -> half; torch goes through float, which rounds twice)."""
    return torch.from_numpy(t.contiguous().numpy().astype(np.float16).astype(np.float64))


def h_trunc(t):
    """float64 tensor rounded TOWARD ZERO to half (the rounding mutant of the oracle's own tests)."""
    a = t.contiguous().numpy()
    r = a.astype(np.float16)
    over = np.abs(r.astype(np.float64)) > np.abs(a)
    r[over] = np.nextafter(r[over], np.float16(0))
    return torch.from_numpy(r.astype(np.float64))


def ulp_h(t):
    """Spacing of the half numbers at |t| (2^-24 in the subnormal range), float64 tensor -> float64 tensor."""
    a = t.abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def near_tie(v):
    """Distance of each float64 value (numpy array) from the nearest boundary between two half roundings, i.e. from the nearest
    midpoint of neighbouring half numbers."""
    v = np.asarray(v, np.float64)
    r = v.astype(np.float16)
    up = np.nextafter(r, np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(r, np.float16(-np.inf)).astype(np.float64)
    r = r.astype(np.float64)
    return np.minimum(np.abs(v - (r + up) / 2), np.abs(v - (r + dn) / 2))


def act64(f, act):
    if act == "relu":
        return f.clamp_min(0)
    if act == "silu":
        return f * torch.sigmoid(f)
    if act == "sigmoid":
        return torch.sigmoid(f)
    assert act == "none", act
    return f


# ---------------------------------------------------------------- the contract
def epilogue(acc, bias, act="none", res=None, res_after=False, stages=None, hc=h):
    """The epilogue every convolution kernel shares, on an fp64 sum `acc` [B, N, H, W].  `stages` (a list) receives the unrounded value
    at every rounding point; `hc` is the rounding of the intermediate (the mutant swaps it)."""
    st = stages if stages is not None else []
    st.append(("conv", acc))
    f = hc(acc) + bias.view(1, -1, 1, 1)
    if res is not None and not res_after:
        f = f + res
    st.append(("pre", f))
    f = act64(f, act)
    if res is not None and res_after:
        st.append(("act", f))
        f = h(f) + res
    st.append(("out", f))
    return h(f)


def conv_acc(x, w, stride=1):
    """fp64 sum of a [N, K, k, k] convolution with pad k // 2 (k = 1: the pointwise product)."""
    return F.conv2d(x, w, None, stride, w.shape[-1] // 2)


def stem_ref(x, w, bias, conv1=None, stages=None):
    st = stages if stages is not None else []
    y = F.max_pool2d(epilogue(F.conv2d(x, w, None, 2, 3), bias, "relu", stages=st), 3, 2, 1)
    if conv1 is None:
        return y
    w1, b1 = conv1
    return y, epilogue(conv_acc(y, w1.view(16, 16, 1, 1)), b1, "relu", stages=st)


def lightconv_ref(x, w1, wd, bias, stages=None):
    """w1 [C, C] (out, in), wd [C, 3, 3] depthwise taps."""
    st = stages if stages is not None else []
    c = x.shape[1]
    acc = conv_acc(x, w1.view(c, c, 1, 1))
    st.append(("pointwise", acc))
    f = F.conv2d(h(acc), wd.view(c, 1, 3, 3), bias, 1, 1, 1, c)
    st.append(("out", f))
    return h(f).clamp_min(0)


def osnet_head_ref(x, w, bias, stages=None):
    """x [N, 128, H, W], w [F, 128] -> [N, F]."""
    st = stages if stages is not None else []
    m = x.sum((2, 3)) / (x.shape[2] * x.shape[3])
    st.append(("mean", m))
    fc = h(m) @ w.t()
    st.append(("fc", fc))
    f = (h(fc) + bias).clamp_min(0)
    st.append(("out", f))
    return h(f)


def avgpool2_ref(x):
    return h((x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2] + x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2]) / 4)


def bias_act_ref(x, bias, act="none", res=None, res_after=False, stages=None):
    """k_bias_act8 / k_bias_act1 / k_bias_act_place: x is a half tensor already, so the intermediate rounding is the identity."""
    return epilogue(x, bias, act, res, res_after, stages, hc=lambda t: t)


# ---------------------------------------------------------------- operands on which the chain is exact
def assert_half_exact(stages, what=""):
    """Every unrounded value at every rounding point is a half number already: the rounding there changes nothing, whichever way it goes."""
    for name, v in stages:
        bad = h(v) != v
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} values at rounding point '{name}' are not half numbers (max |v| = {float(v.abs().max())})"


def assert_any_order(abs_sum, unit, what=""):
    """abs_sum = sum of |products|, every product a multiple of `unit` (a power of two): when abs_sum / unit <= 2^24 every partial sum, in any
    order and grouping (MFMA shapes, split-K partial tiles), is an integer multiple of `unit` below 2^24 of them: exact in fp32."""
    top = float(abs_sum.max()) / unit
    assert top <= 2.0 ** 24, f"{what}: partial sums reach {top} units, past fp32's 2^24"


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def exact_weights(g, s, *shape):
    """{-1, 0, 1} * 2^-s, kept at density 1/2."""
    return _ints(g, -1, 1, *shape) * (torch.rand(*shape, generator=g) < 0.5).double() * 2.0 ** -s


def exact_conv_operands(seed, B, K, H, W, N, ksize, stride, s):
    """x integers in [-2, 2], weights {-1, 0, 1} * 2^-s at density 1/2, bias and shortcut small integers * 2^-s, for a k x k convolution
    (pad k // 2); asserts from the fp64 sums alone that no order of summation rounds in fp32."""
    g = torch.Generator().manual_seed(seed)
    x = _ints(g, -2, 2, B, K, H, W)
    w = exact_weights(g, s, N, K, ksize, ksize)
    bias = _ints(g, -16, 16, N) * 2.0 ** -s
    acc = conv_acc(x, w, stride)
    res = _ints(g, -8, 8, *acc.shape) * 2.0 ** -s
    assert_any_order(x.abs().max() * w.abs().sum((1, 2, 3)), 2.0 ** -s, f"conv {(B, K, H, W, N, ksize, stride, s)}")    # sum |x| |w| <= max |x| * sum |w|
    return dict(x=x, w=w, bias=bias, res=res, acc=acc)


VARIANTS = {"plain": (False, False), "res": (True, False), "res_after": (True, True)}
EXACT_ACTS = ("none", "relu")


def exact_conv_refs(ops, what=""):
    """{(variant, act): fp64 reference} for the three shortcut variants and the two exact activations, each asserted to be exact at every
    rounding point (assert_half_exact): a case that leaves the exact range fails here, before any kernel runs."""
    refs = {}
    for vname, (use_res, after) in VARIANTS.items():
        for act in EXACT_ACTS:
            st = []
            refs[vname, act] = epilogue(ops["acc"], ops["bias"], act, ops["res"] if use_res else None, after, st)
            assert_half_exact(st, f"{what} {vname} {act}")
    return refs


# ---------------------------------------------------------------- launch_pw's choice of kernel form, restated
def pw_form(M, K, N, conv3, aligned, pw_epilogue=1, pw_splitk=1):
    """The kernel ss_op_pointwise_f16 / ss_op_conv3x3_f16 launch for a problem of M pixels, K = Cin (1x1) or 9 * Cin (3x3) and N output
    channels: ("pw", BN, PT, CONV3, VEC_EPI) for k_pw<BN, PT, CONV3, VEC_EPI> or ("splitk", BN) for k_pw_splitk<BN, true>.  `aligned`:
    row pitch, c0 and cn multiples of 8 halfs and out / out2 / res on 16-byte addresses.

    This is a RESTATEMENT of launch_pw in strongsort_yolo_amd/csrc/ss_ops.hip and can drift from it: it follows `const bool vec = ...`
    (the vector epilogue), `if (splitk_allowed && vec && conv3 && K >= 512 && M <= 4096)` (split-K) and the four lines under
    `const bool big = M >= 32768;` (the tile).  When launch_pw changes, change this with it; the GPU tests do not read the form back from
    the library, they use it only to show that their cases reach every form."""
    vec = bool(pw_epilogue) and bool(aligned)
    if pw_splitk and vec and conv3 and K >= 512 and M <= 4096:
        return ("splitk", 32 if N <= 32 else 64)
    big = M >= 32768
    if N <= 32:
        bn = 32
    elif N == 80:
        bn = 80
    elif N <= 64 or not big:
        bn = 64
    else:
        bn = 128
    return ("pw", bn, 2 if big else 1, bool(conv3), vec)


# every form launch_pw can reach: k_pw<128, 1, ., .> is compiled for no launch (N > 64 at M < 32768 takes <64, 1>), so 7 tiles x 2 x 2 + 2
REACHABLE_FORMS = frozenset([("pw", bn, pt, c3, ve) for bn, pt in ((32, 1), (32, 2), (64, 1), (64, 2), (80, 1), (80, 2), (128, 2))
                             for c3 in (False, True) for ve in (False, True)] + [("splitk", 32), ("splitk", 64)])


# ---------------------------------------------------------------- the case list of tests/test_gpu_nets_exact.py, Part A
def _case(kind, B, K, H, W, N, stride=1, ss=(0, 3)):
    """kind "pw" (1x1) or "c3" (3x3, pad 1); K = input channels; ss = the weight shifts s the case runs with."""
    return dict(kind=kind, B=B, K=K, H=H, W=W, N=N, stride=stride, ss=ss)


def _pt1():
    out = []
    for kind in ("pw", "c3"):
        for n in (8, 24, 32, 40, 64, 72, 136, 80):                    # <32> | <64> one tile, two and three tiles with a ragged last | <80>
            out.append(_case(kind, 3, 24, 7, 9, n))                   # M = 189: three 64-pixel workgroups, the last ragged
        for n in (8, 64, 80):
            out.append(_case(kind, 2, 8, 3, 5, n))                    # M = 30: less than one workgroup, less than two waves
    return out


def _pt2():
    out = []
    for i, n in enumerate((16, 48, 80, 72, 128, 136)):                # <32, 2> <64, 2> <80, 2> <128, 2> x 3
        out.append(_case("pw", 1, 24 if n == 136 else 8, 181, 182, n, ss=(3 * (i % 2),)))       # M = 32942: ragged against 128 and 16
        out.append(_case("c3", 8, 8, 64, 64, n, ss=(3 * ((i + 1) % 2),)))                       # M = 32768: pixel tiles of eight images
    out.append(_case("c3", 1, 8, 181, 182, 136, ss=(0,)))            # 3x3 with a ragged last 128-pixel workgroup
    out.append(_case("c3", 2, 8, 258, 258, 48, 2, ss=(3,)))          # stride 2 at PT = 2: M = 2 * 129 * 129 = 33282
    return out


def _k_edges():
    out = [_case("pw", 3, k, 7, 9, 40) for k in (8, 40, 64, 72, 136, 512)]          # one chunk, ragged, exactly one, one + 8, three, eight
    out += [_case("c3", 3, c, 7, 9, 24) for c in (8, 24, 64, 72)]                   # Cin = 8: a 32-wide MFMA block spans four taps
    return out


def _geometry():
    return [_case("c3", 3, c, hh, ww, 40, st) for st in (1, 2) for (hh, ww), c in (((1, 1), 8), ((2, 1), 24), ((7, 9), 8), ((13, 11), 24))]


def _splitk():
    out = []
    for i, n in enumerate((8, 32, 40, 64, 80, 136)):                  # <32>: 8, 32; <64>: 40, 64, 80, 136 (three channel tiles, the last ragged)
        out.append(_case("c3", 1, (64, 72)[i % 2], 1, 17, n))         # M = 17: two 16-pixel workgroups; 9 chunks | 10 chunks with a ragged 8
    out += [_case("c3", 1, 64, 1, 1, 8), _case("c3", 1, 72, 1, 1, 64)]                           # M = 1
    out += [_case("c3", 4, 72, 32, 32, 32, ss=(0,)), _case("c3", 4, 64, 32, 32, 136, ss=(3,)),
            _case("c3", 4, 72, 64, 64, 80, 2, ss=(3,))]                                         # M = 4096, the last through stride 2
    out += [_case("c3", 1, 64, 17, 241, 32, ss=(3,)), _case("c3", 1, 72, 17, 241, 64, ss=(0,))]  # M = 4097: back on k_pw
    return out


PW_CASES = _pt1() + _pt2() + _k_edges() + _geometry() + _splitk()


def case_id(c):
    return f"{c['kind']}-{c['B']}x{c['K']}x{c['H']}x{c['W']}-n{c['N']}-s{c['stride']}"


def case_dims(c):
    """(M, K of the GEMM, OH, OW)."""
    st = c["stride"]
    oh, ow = (c["H"] - 1) // st + 1, (c["W"] - 1) // st + 1
    return c["B"] * oh * ow, c["K"] * (9 if c["kind"] == "c3" else 1), oh, ow


def case_settings(c):
    """The (pw_epilogue, pw_splitk) settings a case runs under: the default, the 8-byte epilogue, and - where the default takes the split-K
    form - the same case on k_pw."""
    M, K, _, _ = case_dims(c)
    sets = [(1, 1), (0, 1)]
    if pw_form(M, K, c["N"], c["kind"] == "c3", True)[0] == "splitk":
        sets.append((1, 0))
    return sets


def case_forms(c):
    """Every kernel form the GPU test of case `c` launches: its settings with aligned operands, and the default setting with the placement
    at c_off = 4 into N + 12 channels (not 16-byte aligned: the 8-byte epilogue without the option)."""
    M, K, _, _ = case_dims(c)
    c3 = c["kind"] == "c3"
    return [pw_form(M, K, c["N"], c3, True, e, sk) for e, sk in case_settings(c)] + [pw_form(M, K, c["N"], c3, False, 1, 1)]


def case_operands(c, s):
    ks = 3 if c["kind"] == "c3" else 1
    seed = (c["B"] * 7 + c["K"]) * 1000003 + c["H"] * 9176 + c["W"] * 131 + c["N"] * 17 + c["stride"] * 5 + s
    return exact_conv_operands(seed, c["B"], c["K"], c["H"], c["W"], c["N"], ks, c["stride"], s)


# ---------------------------------------------------------------- the other operators' exact cases
CONV0_CASES = [(1, 2, 128, 16), (2, 17, 128, 32), (1, 30, 256, 48)]                  # (B, H, W, co)
LIGHTCONV_CASES = [(2, 16, 5, 8), (3, 24, 16, 16), (2, 32, 20, 8), (1, 16, 20, 24), (2, 24, 5, 16), (1, 32, 16, 8)]   # H = 5, 20: a band's halo rows leave the image
STEM_CASES = [(2, 16), (1, 64)]                                                       # (N, H)
HEAD_CASES = [(1, 16, 8, 512), (13, 16, 8, 512), (9, 4, 4, 64)]                       # (N, H, W, F)


def exact_conv0(B, H, W, co, s):
    """Operands and {act: reference} of the detector's first convolution (3x3 / 2 / pad 1 on three channels)."""
    ops = exact_conv_operands(B * 100 + H + co + s, B, 3, H, W, co, 3, 2, s)
    refs = {}
    for act in EXACT_ACTS:
        st = []
        refs[act] = epilogue(ops["acc"], ops["bias"], act, stages=st)
        assert_half_exact(st, f"conv0 {(B, H, W, co, s)} {act}")
    return ops, refs


def exact_lightconv(n, c, hh, ww, s):
    g = torch.Generator().manual_seed(c * 100 + hh + s)
    x = _ints(g, -2, 2, n, c, hh, ww)
    w1, wd = exact_weights(g, s, c, c), exact_weights(g, s, c, 3, 3)
    bias = _ints(g, -16, 16, c) * 2.0 ** -(2 * s)
    assert_any_order(2 * w1.abs().sum(1), 2.0 ** -s, "lightconv pointwise")
    st = []
    ref = lightconv_ref(x, w1, wd, bias, st)
    assert_half_exact(st, f"lightconv {(n, c, hh, ww, s)}")
    mid = h(st[0][1])
    assert_any_order(mid.abs().max() * wd.abs().sum((1, 2)) + bias.abs(), 2.0 ** -(2 * s), "lightconv depthwise")
    return dict(x=x, w1=w1, wd=wd, bias=bias), ref


def exact_stem(n, hh, s):
    """x [n, 3, hh, 128]; 7x7 / 2 / pad 3 weights, the first OSBlock's conv1 (16 -> 16) behind the pool."""
    ops = exact_conv_operands(hh * 10 + s, n, 3, hh, 128, 16, 7, 2, s)
    g = torch.Generator().manual_seed(hh + 77 + s)
    w1, b1 = exact_weights(g, s, 16, 16), _ints(g, -16, 16, 16) * 2.0 ** -(2 * s)
    st = []
    y, y1 = stem_ref(ops["x"], ops["w"], ops["bias"], (w1, b1), st)
    assert_half_exact(st, f"stem {(n, hh, s)}")
    assert_any_order(y.abs().max() * w1.abs().sum(1), 2.0 ** -(2 * s), "stem conv1")
    return dict(ops, w1=w1, b1=b1), y, y1


def exact_head(n, hh, ww, f, s):
    """x integers in [-2, 2]: the sum over HW = 128 or 16 positions is an integer, the mean an integer / 2^7 or 2^4; fc weights {-1, 0, 1} *
    2^-s.  |sum| <= 2048 and |fc| * HW * 2^s <= 2048 follow from assert_half_exact on the mean and the fc stage."""
    g = torch.Generator().manual_seed(n * 31 + f + s)
    x = _ints(g, -2, 2, n, 128, hh, ww)
    w = exact_weights(g, s, f, 128)
    bias = _ints(g, -4, 4, f) * 2.0 ** -s                  # fc + bias stays below 16 * 2^-s, where the fc sum's unit 2^-7 * 2^-s is still a half step
    hw = hh * ww
    assert hw & (hw - 1) == 0
    st = []
    ref = osnet_head_ref(x, w, bias, st)
    assert_half_exact(st, f"osnet_head {(n, hh, ww, f, s)}")
    assert float(x.sum((2, 3)).abs().max()) <= 2048 and float(st[1][1].abs().max()) * hw * 2 ** s <= 2048
    assert_any_order(h(st[0][1]).abs().max() * w.abs().sum(1), 2.0 ** -s / hw, "osnet_head fc")
    return dict(x=x, w=w, bias=bias), ref


# ---------------------------------------------------------------- Part B: N(0,1) operands
def normal_conv_operands(seed, B, K, H, W, N, ksize, stride):
    """Half operands drawn as the existing tests draw them: x ~ N(0, 1), w ~ N(0, 1 / fan_in), bias and shortcut ~ N(0, 1), as fp64."""
    g = torch.Generator().manual_seed(seed)
    hf = lambda t: t.half().double()
    x = hf(torch.randn(B, K, H, W, generator=g))
    w = hf(torch.randn(N, K, ksize, ksize, generator=g) / (K * ksize * ksize) ** 0.5)
    bias = hf(torch.randn(N, generator=g))
    acc = conv_acc(x, w, stride)
    res = hf(torch.randn(*acc.shape, generator=g))
    acc32 = F.conv2d(x.float(), w.float(), None, stride, ksize // 2).double()
    return dict(x=x, w=w, bias=bias, res=res, acc=acc, acc32=acc32)


def elementwise_bound(stages, ref, act):
    """|kernel - ref| allowed per element, from the stages of the fp64 chain: one flip of the intermediate c, carried through the activation
    (Lipschitz constant L), and one flip of the output; with res_after one more flip, of the rounded activation a = h(act(f)) the shortcut is
    added to - its half step, not the output's: the shortcut may cancel most of a.    L * ulp_h(c) + ulp_h(ref) (+ ulp_h(a))"""
    d = dict(stages)
    if "conv" not in d:                             # a chain with ONE rounding point (k_dw3x3): no intermediate to flip
        return ulp_h(ref)
    b = LIPSCHITZ[act] * ulp_h(h(d["conv"])) + ulp_h(ref)
    return b + ulp_h(h(d["act"])) if "act" in d else b


def act_exempt(stages, act):
    """Elements the count of Part B leaves out - for sigmoid only: those whose fp64 value lies within act_delta (below) of a boundary of the
    rounding it meets first.  Cause: sigmoid(v) = 1/2 + v/4 - v^3/48 + ..., and the pre-activations c + bias near zero are multiples of
    2^-10 or 2^-11, for whose odd multiples 1/2 + v/4 is EXACTLY a midpoint between two half numbers (spacing 2^-12 below 1/2), so the
    true value sits v^3/48 (1e-8 .. 1e-12) from a rounding boundary: no fp32 evaluation resolves that, act_apply's v_exp_f32 / v_rcp_f32
    sequence least of all, and each such element is a coin toss.  Some 0.15 % of N(0,1)-driven elements are such structural ties; the kernels' raw count came out at 109 against the CPU's 7 of
    184320 (profiles/f16_exact_shares.txt), every excess element inside this zone.  The zone is derived from the instruction sequence, not
    from the counts, and is 0.2 - 0.5 % of the elements.  none, relu and silu (v/2 + v^2/4 + ...: v/2 is a half number, not a midpoint) exempt
    nothing: their raw counts are held to the bound."""
    d = dict(stages)
    a = d["act"] if "act" in d else d["out"]
    if act != "sigmoid":
        return torch.zeros(a.shape, dtype=torch.bool)
    return torch.from_numpy(near_tie(a.contiguous().numpy()) <= act_delta(d["pre"].contiguous().numpy(), act))


def share_bound(ref_count):
    """Elements not bit-equal to the fp64 chain a kernel may have, given the count of F.conv2d in fp32 on the CPU through the same chain:
    both are fp32 sums in some order, whose error is some 1e-3 of a half ulp, so their counts are of one order (factor 4); 20 for count noise
    on small outputs.  A truncating or half-accumulating kernel is at tens of percent."""
    return 4 * ref_count + 20


PARTB_CASES = [("c3", 2, 16, 24, 40, 32, 1), ("c3", 2, 64, 13, 11, 256, 2), ("c3", 2, 256, 12, 20, 64, 1),      # K = 144, 576, 2304
               ("pw", 3, 16, 24, 40, 64, 1), ("pw", 2, 512, 12, 20, 80, 1)]                                    # K = 16, 512
PARTB_CONV0 = [(2, 17, 128, 16), (1, 30, 256, 48)]


# ---------------------------------------------------------------- silu and sigmoid on a grid
def act_grid():
    """Pre-activations k / 8 in [-40, 40]: 641 half numbers."""
    return np.arange(-320, 321) / 8.0


def act_delta(v, act):
    """Bound on |act_apply(v) - act(v)| for the instruction sequence of act_apply, v a half number:
        t = -v * log2e      __expf's argument scaling: the fp32 constant is 0.22 * 2^-24 off, the product rounds by <= 2^-24: |dt| <= 1.22 * 2^-24 * |t|,
                            which exp2 turns into a relative error ln2 * |dt| = 1.22 * |v| * 2^-24 of e
        e = v_exp_f32(t)    1 ulp: 2 * 2^-24 relative
        d = 1 + e           1/2 ulp: 2^-24; e's relative error enters d scaled by e / (1 + e) <= 1
        r = v_rcp_f32(d)    1 ulp: 2 * 2^-24
        v * r               1/2 ulp: 2^-24 (silu only)
    sum: (1.22 |v| + 6) * 2^-24, taken as (1.25 |v| + 6) * 2^-24, relative to |act(v)|."""
    v = np.asarray(v, np.float64)
    sg = 1.0 / (1.0 + np.exp(-v))
    return (1.25 * np.abs(v) + 6.0) * 2.0 ** -24 * np.abs(v * sg if act == "silu" else sg)


def act_grid_ref(act):
    """(h(act64(v)) as half, exempt mask) over act_grid(): a point is exempt when the fp64 value lies within act_delta of a rounding boundary."""
    v = act_grid()
    sg = 1.0 / (1.0 + np.exp(-v))
    f = v * sg if act == "silu" else sg
    return f.astype(np.float16), near_tie(f) <= act_delta(v, act)


# ================================================================ the operators outside the convolution family
# (docs/F16_OPERATORS.md sections 6 - 11)
#    k_dw3x3:      out = h(act(bias + the in-image taps)), fp32 fma chain started at the bias, ONE rounding
#    k_maxpool:    the maximum of the in-image elements of the window (no arithmetic: equal to F.max_pool2d)
#    k_psa_attn:   S = scale * (q . k) in fp32; p = h(expf(S - max) / sum); o = sum_j p_j v_j in fp32; out = h(h(o) + pe) | h(o)
#    k_v8_decode:  f32_ref.v8_decode_ref on logit = tensor + bias (fp32 output, no half rounding)
#    the gate:     g_t = sigmoid(fc2(relu(fc1(mean_hw x_t)))) in fp32; out = h(sum_t g_t x_t)
from tests import f32_ref as R32

U32 = 2.0 ** -24                                                          # half an fp32 ulp, relative


# ---------------------------------------------------------------- depthwise 3x3
DW_CASES = [(1, 8, 1, 1),               # every tap but the centre is out of the image
            (1, 8, 1, 5), (1, 8, 5, 1),  # one row | one column
            (2, 24, 2, 2),              # every pixel a corner, two images
            (3, 72, 7, 9),              # C8 = 9 is no power of two; three images whose border rows differ
            (1, 128, 257, 256)]         # C8 * pixels = 1 052 672 > 4096 * 256 threads: the grid-stride loop's second pass
DW_PARTB = [(2, 64, 13, 11), (2, 80, 20, 12)]


def dw_taps(x, wd, leak=False):
    """fp64 (or fp32) sum of the nine in-image taps, x [N, C, H, W], wd [C, 3, 3], added in tap order.  `leak` (the mutant): the images are
    stacked into one tall map, so a tap above the first row of image n reads the last row of image n - 1."""
    n, c, hh, ww = x.shape
    src = x.permute(1, 0, 2, 3).reshape(1, c, n * hh, ww) if leak else x
    xp = F.pad(src, (1, 1, 1, 1))
    acc = torch.zeros_like(src)
    for dy in range(3):
        for dx in range(3):
            acc = acc + xp[:, :, dy:dy + src.shape[2], dx:dx + ww] * wd[:, dy, dx].view(1, c, 1, 1)
    return acc.reshape(c, n, hh, ww).permute(1, 0, 2, 3) if leak else acc


def dw_epilogue(acc, act="none", stages=None):
    """acc = bias + taps.  One rounding point."""
    st = stages if stages is not None else []
    st.append(("pre", acc))
    f = act64(acc, act)
    st.append(("out", f))
    return h(f)


def dw3x3_ref(x, wd, bias, act="none", stages=None, leak=False):
    return dw_epilogue(dw_taps(x, wd, leak) + bias.view(1, -1, 1, 1), act, stages)


def w9_of(wd):
    """[C, 3, 3] -> the kernel's [9, C] tap-major layout."""
    return wd.reshape(wd.shape[0], 9).t().contiguous()


def exact_dw(n, c, hh, ww, s):
    """x integers in [-2, 2] * 2^-s with no zero in the first and last row of an image (a tap that leaks across an image border then
    moves the sum wherever its weight is not 0), weights {-1, 0, 1} * 2^-s drawn per tap and channel, bias integers * 2^-2s."""
    g = torch.Generator().manual_seed(n * 1009 + c * 101 + hh * 7 + ww + s)
    x = _ints(g, -2, 2, n, c, hh, ww)
    for r in (0, hh - 1):
        x[:, :, r] = torch.where(x[:, :, r] == 0, torch.ones(()).double(), x[:, :, r])
    x = x * 2.0 ** -s
    wd = _ints(g, -1, 1, c, 3, 3) * 2.0 ** -s
    bias = _ints(g, -16, 16, c) * 2.0 ** -(2 * s)
    assert_any_order(x.abs().max() * wd.abs().sum((1, 2)) + bias.abs(), 2.0 ** -(2 * s), f"dw3x3 {(n, c, hh, ww, s)}")
    refs = {}
    for act in EXACT_ACTS:
        st = []
        refs[act] = dw3x3_ref(x, wd, bias, act, st)
        assert_half_exact(st, f"dw3x3 {(n, c, hh, ww, s)} {act}")
    return dict(x=x, wd=wd, bias=bias), refs


def dw_shifts(case):
    """The weight shifts a Part A case runs with: both, but one for the 17 MB case."""
    return (3,) if case[2] * case[3] > 4096 else (0, 3)


def normal_dw_operands(seed, n, c, hh, ww):
    """Half operands x ~ N(0, 1), taps ~ N(0, 1 / 9), bias ~ N(0, 1); acc = bias + taps in fp64, acc32 the same nine multiply-add steps in fp32
    on the CPU, started at the bias as the kernel starts them (the yardstick of the count)."""
    g = torch.Generator().manual_seed(seed)
    hf = lambda t: t.half().double()
    x, wd, bias = hf(torch.randn(n, c, hh, ww, generator=g)), hf(torch.randn(c, 3, 3, generator=g) / 3), hf(torch.randn(c, generator=g))
    acc = dw_taps(x, wd) + bias.view(1, -1, 1, 1)
    xp = F.pad(x.float(), (1, 1, 1, 1))
    a32 = bias.float().view(1, -1, 1, 1).expand(n, c, hh, ww).contiguous()
    for dy in range(3):
        for dx in range(3):
            a32 = torch.addcmul(a32, xp[:, :, dy:dy + hh, dx:dx + ww], wd.float()[:, dy, dx].view(1, c, 1, 1))
    return dict(x=x, wd=wd, bias=bias, acc=acc, acc32=a32.double())


# ---------------------------------------------------------------- max pooling
MAXPOOL_CASES = [(2, 8, 5, 7, 5, 1, 2),               # (N, C, H, W, k, stride, pad): SPPF's pool on a map smaller than two windows
                 (1, 24, 1, 1, 5, 1, 2),             # one pixel: 24 of the 25 window positions are padding
                 (2, 16, 7, 9, 3, 2, 1),             # odd sizes, the last window partly outside
                 (1, 8, 8, 8, 3, 2, 1),              # even sizes: the last window ends inside
                 (2, 8, 6, 10, 2, 2, 0),             # yolov7's MP
                 (1, 8, 13, 13, 13, 1, 6), (1, 8, 13, 13, 9, 1, 4),      # SPPCSPC
                 (1, 64, 41, 41, 5, 1, 2),           # H * W > 1024: the SPPF fall-back sppf_pools_ok refuses
                 (1, 8, 1030, 1030, 3, 1, 1)]        # 1 060 900 vector elements > 4096 * 256: the stride loop's second pass (17 MB)


def negative_half_map(n, c, hh, ww, seed=0):
    """Half numbers in [-2^14 * 15/8, -2^-10]: all negative, spread over twenty-five binades, so a pad of 0 wins every border window."""
    g = torch.Generator().manual_seed(seed * 7919 + n * 1009 + c * 101 + hh * 7 + ww)
    v = -torch.exp2(_ints(g, -10, 14, n, c, hh, ww)) * (1 + _ints(g, 0, 7, n, c, hh, ww) / 8)
    assert torch.equal(h(v), v) and float(v.max()) < 0
    return v


def maxpool_ref(x, k, stride, pad, fill=float("-inf")):
    """`fill`: what a window sees outside the map (-inf: the contract; 0: the mutant)."""
    return F.max_pool2d(F.pad(x, (pad, pad, pad, pad), value=fill), k, stride, 0)


# ---------------------------------------------------------------- C2PSA attention
PSA_CASES = [(1, 1, 1),                                   # (B, heads, N): one key
             (2, 2, 15), (1, 2, 16), (1, 2, 17),        # one wave: the first partial tile, the first full one, one query into the second
             (1, 2, 31), (1, 2, 32), (1, 2, 33),        # the NP padding step (keys are padded to a multiple of 32)
             (1, 2, 64), (1, 2, 65),                    # the second workgroup in x
             (3, 2, 240),                               # 640 x 384
             (1, 4, 255), (2, 4, 256),                  # the cap
             (1, 8, 60)]
PSA_PARTB = [(2, 2, 240), (1, 4, 256), (2, 2, 15)]
PSA_SCALE = float(np.float32(32.0 ** -0.5))               # the module's scale as the fp32 number the entry receives
PSA_GAP = 32.0                                            # exp(-32) < 2^-46: rounds to 0 in half, and 256 of them do not move an fp32 sum >= 1


def psa_split(qkv, heads):
    """[B, N, heads * 128] -> q, k [B, heads, N, 32], v [B, heads, N, 64]."""
    B, N, _ = qkv.shape
    t = qkv.reshape(B, N, heads, 128).permute(0, 2, 1, 3)
    return t[..., :32], t[..., 32:64], t[..., 64:]


def psa_ref(qkv, pe, heads, scale, stages=None, hp=h, mask=True, swap_pairs=False, f32=False):
    """qkv [B, N, heads * 128] (per head q 32 | k 32 | v 64), pe [B, N, heads * 64] or None -> [B, N, heads * 64].
    `hp`: the rounding of the probabilities.  The mutants: `mask` False - the keys padded up to a multiple of 32 (k = 0, v = 0) take part
    in the softmax with their score of 0; `swap_pairs` - the probabilities of key tile 2t meet the values of tile 2t + 1 and the other
    way round.  `f32`: every fp32 step of the kernel in float32 on the CPU (the yardstick of the count)."""
    st = stages if stages is not None else []
    B, N, _ = qkv.shape
    NP = (N + 31) // 32 * 32
    q, k, v = psa_split(qkv, heads)
    k, v = F.pad(k, (0, 0, 0, NP - N)), F.pad(v, (0, 0, 0, NP - N))
    if f32:
        S = ((q.float() @ k.float().transpose(2, 3)) * np.float32(scale))
    else:
        S = (q @ k.transpose(2, 3)) * scale
    if mask:
        S[..., N:] = float("-inf")
    p = torch.softmax(S, -1).double()
    st.append(("p", p))
    p = hp(p)
    if swap_pairs:
        p = p.reshape(B, heads, N, NP // 32, 2, 16).flip(4).reshape(B, heads, N, NP)
    o = (p.float() @ v.float()).double() if f32 else p @ v
    st.append(("o", o))
    o = h(o).permute(0, 2, 1, 3).reshape(B, N, heads * 64)
    if pe is None:
        return o
    st.append(("out", o + pe))
    return h(o + pe)


def _psa_code(j):
    """Key index -> its eight bits as +-1."""
    return torch.tensor([1.0 if (j >> b) & 1 else -1.0 for b in range(8)], dtype=torch.float64)


def _psa_assert_exact(qkv, pe, heads, scale, ref, what):
    """From the fp64 reference alone: the scores are integers any order of summation keeps; every key scores the row's maximum or at least
    PSA_GAP below it; the keys at the maximum are a power of two in number.  Then expf(S - max) is 1 or below 2^-46, the fp32 sum is that
    power of two exactly, p is 2^-k or rounds to 0 in half, and sum_j p_j v_j and its sum with pe are exact."""
    q, k, v = psa_split(qkv, heads)
    assert_any_order((q.abs() @ k.abs().transpose(2, 3)) * scale, scale, what)
    S = (q @ k.transpose(2, 3)) * scale
    top = S.max(-1, keepdim=True).values
    win = S == top
    assert bool((win | (S <= top - PSA_GAP)).all()), f"{what}: a score within {PSA_GAP} of the maximum"
    cnt = win.sum(-1, keepdim=True)
    assert bool(((cnt & (cnt - 1)) == 0).all()) and int(cnt.max()) <= 256, f"{what}: winners are no power of two"
    p = win.double() / cnt
    st = []
    again = psa_ref(qkv, pe, heads, scale, st)
    assert torch.equal(h(st[0][1])[..., :S.shape[-1]], p), f"{what}: h(softmax) is not the one-hot / uniform distribution"
    assert_half_exact(st[1:], what)
    assert_any_order(p @ v.abs(), float(1.0 / cnt.max()), what)
    assert torch.equal(again, ref)
    return S


def exact_psa_onehot(B, heads, N, with_pe, seed=0):
    """One key per query.  Key j: its index as eight +-1 in dims 0..7, 1 in dim 8; query i: 16 * code(pi(i)) and -256 in dim 8, scale 1:
    S = -128 - 32 * (bits in which j and pi(i) differ) - every real score negative, so an unmasked padded key (score 0) would win.
    Dims 9..15 of k and 16..31 of q carry integers that meet zeros of the other operand.  v, pe integers in [-8, 8]; pi, v, pe differ
    per head and image.  -> qkv [B, N, heads * 128], pe or None, ref, pi [B, heads, N]."""
    g = torch.Generator().manual_seed(seed * 31 + B * 100003 + heads * 1009 + N)
    codes = torch.stack([_psa_code(j) for j in range(N)])
    t = torch.zeros(B, heads, N, 128, dtype=torch.float64)
    pi = torch.stack([torch.stack([torch.randperm(N, generator=g) for _ in range(heads)]) for _ in range(B)])
    t[..., 0:8] = 16.0 * codes[pi]
    t[..., 8] = -256.0
    t[..., 16:32] = _ints(g, -2, 2, B, heads, N, 16)
    t[..., 32:40] = codes
    t[..., 40] = 1.0
    t[..., 41:48] = _ints(g, -2, 2, B, heads, N, 7)
    t[..., 64:] = _ints(g, -8, 8, B, heads, N, 64)
    qkv = t.permute(0, 2, 1, 3).reshape(B, N, heads * 128)
    pe = _ints(g, -8, 8, B, N, heads * 64) if with_pe else None
    ref = psa_ref(qkv, pe, heads, 1.0)
    S = _psa_assert_exact(qkv, pe, heads, 1.0, ref, f"psa one-hot {(B, heads, N)}")
    assert float(S.max()) == -128.0 and torch.equal(S.argmax(-1), pi)
    v = t[..., 64:]
    want = torch.gather(v, 2, pi.unsqueeze(-1).expand(-1, -1, -1, 64)).permute(0, 2, 1, 3).reshape(B, N, heads * 64)
    assert torch.equal(ref, want + pe if with_pe else want)
    return qkv, pe, ref


def exact_psa_uniform(B, heads, N, with_pe, seed=0):
    """Uniform over a subset.  Queries 1 or 2 in dim 0, keys 0 in dim 0 on a seeded subset of 2^k of the N positions and -64 elsewhere
    (k walks 0 .. log2 N over heads and images), scale 1: p = 2^-k on the subset, out = (sum of v over it) / 2^k; v integers in [-4, 4],
    pe in [-4, 4].  Dims 1..31 of q carry integers against zeros of k."""
    g = torch.Generator().manual_seed(seed * 37 + B * 100003 + heads * 1009 + N)
    kmax = min(8, N.bit_length() - 1)
    t = torch.zeros(B, heads, N, 128, dtype=torch.float64)
    t[..., 0] = _ints(g, 1, 2, B, heads, N)
    t[..., 1:32] = _ints(g, -2, 2, B, heads, N, 31)
    t[..., 32] = -64.0
    for b in range(B):
        for hd in range(heads):
            kk = (kmax - (b * heads + hd)) % (kmax + 1)
            t[b, hd, torch.randperm(N, generator=g)[:2 ** kk], 32] = 0.0
    t[..., 64:] = _ints(g, -4, 4, B, heads, N, 64)
    qkv = t.permute(0, 2, 1, 3).reshape(B, N, heads * 128)
    pe = _ints(g, -4, 4, B, N, heads * 64) if with_pe else None
    ref = psa_ref(qkv, pe, heads, 1.0)
    _psa_assert_exact(qkv, pe, heads, 1.0, ref, f"psa uniform {(B, heads, N)}")
    return qkv, pe, ref


def normal_psa_operands(B, heads, N, seed=0):
    g = torch.Generator().manual_seed(seed + B * 100003 + heads * 1009 + N)
    return torch.randn(B, N, heads * 128, generator=g).half().double(), torch.randn(B, N, heads * 64, generator=g).half().double()


MFMA_ADD = 2.0 * U32            # one accumulation step of the matrix cores: taken as a whole fp32 ulp of the partial sum (covers a truncating adder)


def psa_bound(qkv, pe, heads, scale, stages, ref):
    """|kernel - fp64 chain| allowed per element of the output [B, N, heads * 64], from the chain's rounding points and the fp32 steps
    between them.  u = 2^-24.
      scores   32 products of halves (exact) accumulated on the matrix cores, then * scale: |dS_j| <= (32 * 2 + 1) u A_j,
               A_j = scale * sum_d |q_d k_d|
      x = S - max    one fp32 subtraction: u |x| (softmax is shift invariant: the maximum's own error cancels)
      e = __expf(x)  (1.25 |x| + 6) u relative, as act_delta counts v_exp_f32 on x * log2e
      sum      N terms, none negative: (N - 1) u relative; inv = 1 / sum correctly rounded: u; e * inv: u
      => p~ = p (1 + r), |r| <= rel = 2 * max_j[65 A_j + (2.25 |x_j| + 6)] u + (N + 1) u   (numerator and denominator each carry the
         per-key term).  rel < 2^-11 (asserted), so p~ lies less than one half step from p and h(p~) is h(p) or its neighbour:
      p        |h(p~)_j - h(p)_j| <= ulp_h(h(p)_j)                                   (a flip; 2^-24 where h(p) is 0 or subnormal)
      o        NP accumulation steps on the matrix cores over sum_j h(p)_j |v_j|:  |o~ - o| <= E = sum_j ulp_h(h(p)_j) |v_j|
               + NP * 2 u * sum_j (h(p)_j + ulp_h(h(p)_j)) |v_j|
      out      h is monotone: |h(a) - h(b)| <= |a - b| + ulp_h(|b| + |a - b|).  Without pe: E + ulp_h(|o| + E).  With pe: the same for
               h(o), the sum with pe exact in fp32 (two halves), one more rounding: E1 = E + ulp_h(|o| + E), E1 + ulp_h(|h(o) + pe| + E1)."""
    B, N, _ = qkv.shape
    NP = (N + 31) // 32 * 32
    q, k, v = psa_split(qkv, heads)
    d = dict(stages)
    A = (q.abs() @ k.abs().transpose(2, 3)) * scale
    S = (q @ k.transpose(2, 3)) * scale
    x = (S - S.max(-1, keepdim=True).values).abs()
    rel = 2 * float((65 * A + 2.25 * x + 6).max()) * U32 + (N + 1) * U32
    assert rel < 2.0 ** -11, rel
    hp = h(d["p"])[..., :N]
    flip = ulp_h(hp)
    E = flip @ v.abs() + NP * MFMA_ADD * ((hp + flip) @ v.abs())
    o = d["o"]
    E1 = E + ulp_h(o.abs() + E)
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, N, heads * 64)
    if pe is None:
        return back(E1)
    E1 = back(E1)
    return E1 + ulp_h(d["out"].abs() + E1)


def psa_exempt(qkv, heads, stages):
    """Outputs the count of Part B leaves out: those a probability INSIDE fp32's own resolution of a rounding boundary can move.
    Cause: the midpoint between two half numbers is an fp32 number; a p whose fp64 value lies within half an fp32 ulp of one is, correctly
    rounded to fp32, that midpoint itself, and no fp32 evaluation - the kernel's, the CPU's - carries the side the fp64 chain rounds to:
    a coin toss.  Unlike a flip of an output element, one such flip reaches every channel of its query: output c of query i moves when
    the flip's ulp_h(h(p)_ij) v_jc carries o_ic over a rounding boundary of its own, which for the large p of a short key list (N = 15:
    p ~ 1/15, its half step a quarter of the output's) is a third of the query's 64 channels.  Measured: (2, 2, 15) without pe has one such p,
    0.008 * 2^-24 p from a midpoint (image 0, head 1, query 0, key 5); flipping it in the reference changes 26 outputs, the kernel
    differed in those and one more: 27 raw, against 4 * 1 + 20.  The zone follows from the two number formats, not from the count;
    tests/test_f16_ref_cpu.py caps it at 1 % of a tensor.  -> bool [B, N, heads * 64]."""
    B, N, _ = qkv.shape
    _, _, v = psa_split(qkv, heads)
    d = dict(stages)
    p = d["p"][..., :N]
    half_ulp32 = torch.exp2(torch.floor(torch.log2(p.clamp_min(R32.FLT_MIN))) - 24)
    zone = torch.from_numpy(near_tie(p.contiguous().numpy())) <= half_ulp32
    hp = h(p)
    step = torch.where(hp < p, 1.0, -1.0) * ulp_h(hp) * zone                          # to the half number on the other side of the midpoint
    contrib = step.unsqueeze(-1) * v.unsqueeze(2)                                     # [B, heads, N, N, 64]: what each flip adds to o_ic
    up, dn = contrib.clamp_min(0).sum(3), contrib.clamp_max(0).sum(3)                 # any subset of the flips moves o by something in [dn, up]
    o = d["o"]
    hit = (h(o + up) != h(o)) | (h(o + dn) != h(o))                                   # h is monotone: both ends unchanged, every subset unchanged
    return hit.permute(0, 2, 1, 3).reshape(B, N, heads * 64)


# ---------------------------------------------------------------- the v8 decode, half inputs, fp32 output
DECODE16_CASES = [(8, 8, 0, 0, 0),                  # (nc, cls_ld, n_ext, ext_ld, ext_mode): ss_op_v8_decode_f16, the vector class path
                  (80, 80, 0, 0, 0),
                  (5, 8, 0, 0, 0),                  # the scalar class path, class tensors padded to 8 channels
                  (1, 8, 51, 56, 1),                # the pose head: one class, seventeen keypoint triplets in 56 channels
                  (80, 80, 32, 32, 0)]              # the segmentation head: raw mask coefficients


def split_bias(g, total, hard=False):
    """total [B, C, H, W] -> (tensor, bias [C]) with tensor + bias == total: bias integers in [-8, 8] / 8-th of them for a dyadic total;
    `hard`: -200 more on half the channels, so the tensor alone has another maximum than the sum."""
    c = total.shape[1]
    bias = _ints(g, -8, 8, c)
    if hard:
        bias = bias - 200.0 * _ints(g, 0, 1, c)
    return total - bias.view(1, -1, 1, 1), bias


def exact_decode16(B, nc, cls_ld, n_ext, ext_ld, ext_mode, seed=0):
    """f32_ref.exact_decode's operands for the half kernel: one-hot DFL logits (0 | -200), class and confidence logits in {0, 40, -200},
    ext rows k / 8 and one raw value of 2^15 - each box and class logit split between the tensor and a per-level bias that is not zero
    and, for the boxes, moves the winner (split_bias).  Every tensor, every bias and every sum is an integer below 2048 in magnitude:
    a half number, and exact as the kernel's fp32 sum.  -> dict(boxes, clss, box_bias, cls_bias, ext, box_tot, cls_tot), ref [B, rows, A]."""
    g = torch.Generator().manual_seed(seed + nc * 1009 + n_ext * 17 + ext_mode)
    pick = torch.tensor([0.0, 40.0, -200.0], dtype=torch.float64)
    o = dict(boxes=[], clss=[], box_bias=[], cls_bias=[], ext=[], box_tot=[], cls_tot=[])
    for hh, ww in R32.DECODE_LEVELS:
        bins = torch.randint(0, 16, (B, 4, 1, hh, ww), generator=g)
        bt = torch.full((B, 4, 16, hh, ww), -200.0, dtype=torch.float64).scatter_(2, bins, 0.0).reshape(B, 64, hh, ww)
        ct = pick[torch.randint(0, 3, (B, cls_ld, hh, ww), generator=g)]
        b, bb = split_bias(g, bt, hard=True)
        c, cb = split_bias(g, ct)
        for t in (b, bb, c, cb):
            assert torch.equal(h(t), t) and float(t.abs().max()) < 2048
        assert len(bb.reshape(4, 16).unique(dim=1)[0]) > 1 and float(cb[:nc].abs().max()) > 0    # the box bias differs inside a side: softmax is shift invariant
        o["boxes"].append(b); o["box_bias"].append(bb); o["clss"].append(c); o["cls_bias"].append(cb)
        o["box_tot"].append(bt); o["cls_tot"].append(ct)
        if n_ext:
            e = _ints(g, -64, 64, B, ext_ld, hh, ww) / 8
            if ext_mode == 1:
                e[:, 2::3] = pick[torch.randint(0, 3, e[:, 2::3].shape, generator=g)]
            o["ext"].append(e)
    if n_ext and ext_mode == 0:
        o["ext"][0][0, 0, 0, 0] = 2.0 ** 15
    ref = R32.v8_decode_ref(o["box_tot"], o["cls_tot"], R32.DECODE_STRIDES, nc, o["ext"], n_ext, ext_mode)
    # the fp64 value is an fp32 number but for sigmoid(-200) = 1e-87 where fp32 (and the kernel: 1 / inf) has 0
    assert float((ref.float().double() - ref).abs().max()) < 2.0 ** -150, "decode: the reference is no fp32 tensor"
    ref = ref.float().double()
    assert set(ref[:, 4:4 + nc].unique().tolist()) == {0.0, 0.5, 1.0}
    return o, ref


# __expf(x) = v_exp_f32(x * log2e): (1.25 |x| + 6) u relative (act_delta's count); the DFL logits are k / 8 in [-4, 4], so |v_k - max| <= 8
EXPF16_TERM = 1.25 * 8 + 6                                               # 16 units of u per term
# se: 16 terms of EXPF16_TERM, 15 additions; sw: the same and one product e_k * k per term; the quotient correctly rounded:
# (16 + 15) + (16 + 1 + 15) + 1 = 64 units, taken as 72 for the second-order terms (f32_ref.DFL_REL takes 40 for 36)
DFL_REL16 = 72.0 * U32


def decode_box_bound16(st, strides):
    """f32_ref.decode_box_bound with the relative error of d re-derived for __expf: DFL_REL16 in place of DFL_REL."""
    return R32.decode_box_bound(st, strides, rel=DFL_REL16)


def act_bound16(v, ref):
    """|kernel - ref| allowed for 1 / (1 + __expf(-v)), v = tensor + bias exact: (1.25 |v| + 6) u for __expf (it enters 1 + e scaled by
    e / (1 + e) <= 1), u for the addition, u for the correctly rounded division - relative to the reference."""
    return ((1.25 * v.abs() + 8.0) * U32 * ref.abs()).clamp_min(R32.FLT_MIN)


# ---------------------------------------------------------------- OSNet's aggregation gate
GATE_CASES = [(2, 16, 16, 4, 1),                    # (N, C, HW, T, Cr)
              (3, 24, 32, 4, 1),                    # C8 = 3: 256 / C8 leaves an idle thread in k_gate_mean
              (2, 32, 128, 4, 2),
              (1, 256, 4, 1, 16),                   # one stream, the widest map, Cr at its cap
              (2, 16, 2048, 4, 1)]                  # 64 x 32: the apply loop strides, the mean loop runs 16 rounds
GATE_HW = {16: (4, 4), 32: (4, 8), 128: (8, 16), 4: (2, 2), 2048: (64, 32)}
GATE_PARTS = (1, 3, 8)


def gate_values(xs, w1, b1, w2, b2):
    """-> pre-sigmoid values a [T, N, C] of the gates, in fp64."""
    m = torch.stack([x.sum((2, 3)) / (x.shape[2] * x.shape[3]) for x in xs])          # [T, N, C]
    hid = (m @ w1.t() + b1).clamp_min(0)
    return hid @ w2.t() + b2


def gate_ref(xs, w1, b1, w2, b2, order=None, shift=0):
    """out = h(sum_t sigmoid(a_t) x_t).  The mutants: `order` - the stream whose gate multiplies x_t; `shift` - the gate of channel c
    read at channel c + shift."""
    g = torch.sigmoid(gate_values(xs, w1, b1, w2, b2))
    T = len(xs)
    order = list(range(T)) if order is None else order
    acc = 0
    for t in range(T):
        acc = acc + xs[t] * torch.roll(g[order[t]], -shift, 1).view(g.shape[1], g.shape[2], 1, 1)
    return h(acc)


def exact_gate(N, C, HW, T, Cr, seed=0):
    """Integer maps in [-4, 4] over a power-of-two HW (sums, means and psum parts exact), fc1 weights {-1, 0, 1} * HW (its outputs are
    integers: 0 or >= 1 after the relu, different per image and stream), and per channel one of five gate kinds:
        w2 = 0, b2 = 0: exactly 1/2 | b2 = +40: exactly 1 (1 + e^-40 is 1 in fp32 and fp64) | b2 = -40: 4e-18, which moves no sum of
        integers / 2 and alone rounds to 0 in half | w2 = +64 (-64) on one hidden unit, b2 = 0: 1 (about 0) where that unit is positive, else 1/2.
    Asserted from the fp64 values alone: every pre-sigmoid value is 0 or at least 40 in magnitude; with those gates read as 1/2, 1 and 0
    every product and partial sum is a multiple of 1/2 below 2^24 of them, and the sum is a half number; h of the true fp64 sum is that
    number.  -> operands, ref."""
    hh, ww = GATE_HW[HW]
    g = torch.Generator().manual_seed(seed + N * 100003 + C * 1009 + HW * 17 + T)
    pos = lambda xs, w1, b1: torch.stack([x.sum((2, 3)) / HW for x in xs]) @ w1.t() + b1 > 0            # [T, N, Cr]: the hidden units that fire
    for _ in range(64):                               # drawn again until the hidden units fire differently per stream and per image
        xs = [_ints(g, -4, 4, N, C, hh, ww) for _ in range(T)]
        w1 = _ints(g, -1, 1, Cr, C) * HW
        b1 = _ints(g, -2, 2, Cr)
        f = pos(xs, w1, b1)
        if T == 1 or (len(f.reshape(T, -1).unique(dim=0)) == T and (N == 1 or len(f.permute(1, 0, 2).reshape(N, -1).unique(dim=0)) == N)):
            break
    kind = torch.randint(0, 5, (C,), generator=g)
    unit = torch.randint(0, Cr, (C,), generator=g)
    w2, b2 = torch.zeros(C, Cr, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    b2[kind == 1], b2[kind == 2] = 40.0, -40.0
    w2[kind == 3, unit[kind == 3]] = 64.0
    w2[kind == 4, unit[kind == 4]] = -64.0
    for t in (w1, b1, w2, b2):
        assert torch.equal(h(t), t)
    a = gate_values(xs, w1, b1, w2, b2)
    assert bool(((a == 0) | (a.abs() >= 40)).all()), "gate: a pre-sigmoid value that is neither 0 nor saturated"
    m = torch.stack([x.sum((2, 3)) for x in xs])
    assert_any_order(torch.stack([x.abs().sum((2, 3)) for x in xs]), 1.0, "gate sums")
    assert_any_order((m.abs() / HW) @ w1.abs().t() + b1.abs(), 1.0, "gate fc1")
    hid = ((m / HW) @ w1.t() + b1).clamp_min(0)
    assert torch.equal(hid, hid.round()) and len(hid.unique()) > 1, "gate: fc1 is not integer, or the same everywhere"
    gs = torch.where(a == 0, 0.5, torch.where(a > 0, 1.0, 0.0)).double()                     # [T, N, C]
    if T > 1:
        assert not torch.equal(gs[0], gs[1]) and (N == 1 or not torch.equal(gs[:, 0], gs[:, 1])), "gate: the same for every stream or image"
    s = sum(xs[t] * gs[t].view(N, C, 1, 1) for t in range(T))
    assert_half_exact([("out", s)], f"gate {(N, C, HW, T, Cr)}")
    assert_any_order(sum(xs[t].abs() * gs[t].view(N, C, 1, 1) for t in range(T)), 0.5, "gate sum")
    ref = gate_ref(xs, w1, b1, w2, b2)
    assert torch.equal(ref, s), "gate: h(fp64 sum) is not the sum with the gates at 0, 1/2, 1"
    assert {0.0, 0.5, 1.0} <= set(gs.unique().tolist())
    return dict(xs=xs, w1=w1, b1=b1, w2=w2, b2=b2), ref


def gate_psum(xs, parts):
    """[T, N, parts, C] fp64: position p of the map counted in part p % parts - `parts` sums that add up to the map's."""
    T, (N, C) = len(xs), xs[0].shape[:2]
    out = torch.zeros(T, N, parts, C, dtype=torch.float64)
    for t, x in enumerate(xs):
        flat = x.reshape(N, C, -1)
        for p in range(parts):
            out[t, :, p] = flat[:, :, p::parts].sum(2)
    return out
