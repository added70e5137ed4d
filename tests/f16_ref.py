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
