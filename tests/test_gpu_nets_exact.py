"""The f16 operator kernels (csrc/ss_ops.hip) against their float64 restatement on the CPU (tests/f16_ref.py, docs/F16_OPERATORS.md).

Part A: operands on which every product, partial sum and rounding is exact - the kernel's output must EQUAL the fp64 reference cast to
half, for every kernel form launch_pw can choose (tests/test_f16_ref_cpu.py shows the case list reaches all 30), every epilogue variant
and the other operators.  Part B: N(0,1) operands and all four activations - an elementwise bound of one flip of the intermediate and
one of the output, and the count of elements not bit-equal to the fp64 chain held against the count of an fp32 CPU convolution.
Then silu and sigmoid on a grid of exact pre-activations.

The operators outside the convolution family follow in the same two parts (docs/F16_OPERATORS.md sections 6 - 10): the depthwise 3x3,
max pooling, the C2PSA attention, the v8 decode on half inputs and OSNet's aggregation gate."""
import contextlib

import numpy as np
import pytest
import torch

from tests import f16_ref as R

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _cl(t):
    """fp64 CPU tensor (half numbers) -> half on the device, channels-last for 4-d tensors."""
    t = t.to(_dev(), torch.float16)
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.contiguous()


@contextlib.contextmanager
def _options(pw_epilogue=1, pw_splitk=1):
    from strongsort_yolo_amd import fused
    fused.set_option("pw_epilogue", pw_epilogue)
    fused.set_option("pw_splitk", pw_splitk)
    try:
        yield
    finally:
        fused.set_option("pw_epilogue", 1)
        fused.set_option("pw_splitk", 1)


def _weights(kind, w):
    """[N, K, k, k] fp64 -> the layout the launcher takes: [N, K] or [N, 3 * 3 * K] tap-major."""
    n = w.shape[0]
    return _cl(w.reshape(n, -1) if kind == "pw" else w.permute(0, 2, 3, 1).reshape(n, -1))


def _run(kind, x, w, bias, stride, act, **kw):
    from strongsort_yolo_amd import fused
    return fused.pointwise(x, w, bias, act, **kw) if kind == "pw" else fused.conv3x3(x, w, bias, stride, act, **kw)


def _same(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} of {got.numel()} values differ, max |d| = {float((got.float() - ref.float()).abs().max())}"


# ================================================================ Part A: exact operands
@pytest.mark.parametrize("case", R.PW_CASES, ids=R.case_id)
def test_pointwise_and_conv3x3_equal_the_fp64_reference_on_exact_operands(case):
    """Every form of k_pw / k_pw_splitk: the case under the default options, under pw_epilogue = 0 (VEC_EPI = false), where it takes the
    split-K form also under pw_splitk = 0; no shortcut, shortcut before and after the activation, placement into a wider buffer with a
    dense mirror (out2) - 16-byte aligned, and at c_off = 4 into N + 12 channels, which takes the 8-byte epilogue without the option."""
    kind, N, stride = case["kind"], case["N"], case["stride"]
    B, (_, _, OH, OW) = case["B"], R.case_dims(case)
    for s in case["ss"]:
        ops = R.case_operands(case, s)
        refs = {k: _cl(v) for k, v in R.exact_conv_refs(ops, R.case_id(case)).items()}
        x, w, bias, res = _cl(ops["x"]), _weights(kind, ops["w"]), _cl(ops["bias"]), _cl(ops["res"])
        for epi, sk in R.case_settings(case):
            with _options(epi, sk):
                tag = f"{R.case_id(case)} s={s} pw_epilogue={epi} pw_splitk={sk}"
                for (vname, act), ref in refs.items():
                    use_res, after = R.VARIANTS[vname]
                    got = _run(kind, x, w, bias, stride, act, res=res if use_res else None, res_after=after)
                    assert got.is_contiguous(memory_format=torch.channels_last)
                    _same(got, ref, f"{tag} {vname} {act}")
                c0 = 8 * (N // 16)
                for vname, act in (("plain", "none"), ("res_after", "relu")):
                    use_res, after = R.VARIANTS[vname]
                    cat = torch.full((B, N + 24, OH, OW), 3.0, dtype=torch.float16, device=_dev()).contiguous(memory_format=torch.channels_last)
                    out2 = torch.full((B, N - c0, OH, OW), 5.0, dtype=torch.float16, device=_dev()).contiguous(memory_format=torch.channels_last)
                    _run(kind, x, w, bias, stride, act, res=res if use_res else None, res_after=after, out=cat, c_off=8, out2=out2, c0=c0)
                    _same(cat[:, 8:8 + N], refs[vname, act], f"{tag} placed {vname}")
                    _same(out2, refs[vname, act][:, c0:], f"{tag} mirror {vname}")
                    assert bool((cat[:, :8] == 3.0).all()) and bool((cat[:, 8 + N:] == 3.0).all()), f"{tag}: neighbours of the slice written"
        # the 8-byte epilogue without the option: a slice and a mirror that are 8-byte but not 16-byte aligned
        for vname, act in (("plain", "relu"), ("res", "none")):
            use_res, after = R.VARIANTS[vname]
            cat = torch.full((B, N + 12, OH, OW), 3.0, dtype=torch.float16, device=_dev()).contiguous(memory_format=torch.channels_last)
            out2 = torch.full((B, N - 4, OH, OW), 5.0, dtype=torch.float16, device=_dev()).contiguous(memory_format=torch.channels_last)
            _run(kind, x, w, bias, stride, act, res=res if use_res else None, res_after=after, out=cat, c_off=4, out2=out2, c0=4)
            _same(cat[:, 4:4 + N], refs[vname, act], f"{R.case_id(case)} s={s} c_off=4 {vname}")
            _same(out2, refs[vname, act][:, 4:], f"{R.case_id(case)} s={s} c_off=4 mirror {vname}")
            assert bool((cat[:, :4] == 3.0).all()) and bool((cat[:, 4 + N:] == 3.0).all())


def _conv_module(w, bias, stride, pad):
    conv = torch.nn.Conv2d(w.shape[1], w.shape[0], w.shape[2], stride, pad)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(bias)
    return conv.to(_dev(), torch.float16)


@pytest.mark.parametrize("B,H,W,co", R.CONV0_CASES)
def test_conv0_equals_the_fp64_reference_on_exact_operands(B, H, W, co):
    from strongsort_yolo_amd import fused
    for s in (0, 3):
        ops, refs = R.exact_conv0(B, H, W, co, s)
        conv, x = _conv_module(ops["w"], ops["bias"], 2, 1), _cl(ops["x"])
        assert fused.conv0_ok(x, conv)
        wp = fused.conv0_weight(torch.nn.Module(), conv)
        for act, ref in refs.items():
            _same(fused.conv0(x, wp, conv.bias, act), _cl(ref), f"conv0 {(B, H, W, co)} s={s} {act}")


@pytest.mark.parametrize("n,c,hh,ww", R.LIGHTCONV_CASES)
def test_lightconv_equals_the_fp64_reference_on_exact_operands(n, c, hh, ww):
    from strongsort_yolo_amd import fused
    for s in (0, 3):
        ops, ref = R.exact_lightconv(n, c, hh, ww, s)
        x = _cl(ops["x"])
        assert fused.lightconv_ok(x)
        got = fused.lightconv(x, _cl(ops["w1"]), _cl(ops["wd"].reshape(c, 9).t()), _cl(ops["bias"]))
        _same(got, _cl(ref), f"lightconv {(n, c, hh, ww)} s={s}")
        assert float(ref.max()) > 0


@pytest.mark.parametrize("n,hh", R.STEM_CASES)
def test_osnet_stem_equals_the_fp64_reference_on_exact_operands(n, hh):
    from strongsort_yolo_amd import fused
    for s in (0, 3):
        ops, y, y1 = R.exact_stem(n, hh, s)
        conv, x = _conv_module(ops["w"], ops["bias"], 2, 3), _cl(ops["x"])
        assert fused.stem_ok(x, conv)
        wp = fused.stem_weight(torch.nn.Module(), conv)
        _same(fused.osnet_stem(x, wp, conv.bias), _cl(y), f"stem {(n, hh)} s={s}")
        g, g1 = fused.osnet_stem(x, wp, conv.bias, (_cl(ops["w1"]), _cl(ops["b1"])))
        _same(g, _cl(y), f"stem with conv1 {(n, hh)} s={s}")
        _same(g1, _cl(y1), f"stem's conv1 {(n, hh)} s={s}")
        assert float(y.max()) > 0 and float(y1.max()) > 0


@pytest.mark.parametrize("n,hh,ww,f", R.HEAD_CASES)
def test_osnet_head_equals_the_fp64_reference_on_exact_operands(n, hh, ww, f):
    from strongsort_yolo_amd import fused
    for s in (0, 3):
        ops, ref = R.exact_head(n, hh, ww, f, s)
        fc = torch.nn.Linear(128, f)
        with torch.no_grad():
            fc.weight.copy_(ops["w"])
            fc.bias.copy_(ops["bias"])
        fc, x = fc.to(_dev(), torch.float16), _cl(ops["x"])
        assert fused.osnet_head_ok(x, fc)
        _same(fused.osnet_head(x, fc), _cl(ref), f"osnet_head {(n, hh, ww, f)} s={s}")


def test_avgpool2_equals_the_fp64_reference_on_exact_operands():
    from strongsort_yolo_amd import fused
    g = torch.Generator().manual_seed(2)
    for shape in [(2, 24, 6, 10), (1, 8, 2, 2), (3, 64, 16, 8)]:
        for s in (0, 3):
            x = torch.randint(-64, 65, shape, generator=g).double() * 2.0 ** -s
            ref = R.avgpool2_ref(x)
            R.assert_half_exact([("sum / 4", (x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2] + x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2]) / 4)], "avgpool2")
            got = fused.avgpool2(_cl(x))
            assert got.is_contiguous(memory_format=torch.channels_last)
            _same(got, _cl(ref), f"avgpool2 {shape} s={s}")


def _elementwise_operands(seed, B, C, H, W, s):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(-64, 65, (B, C, H, W), generator=g).double() * 2.0 ** -s
    bias = torch.randint(-16, 17, (C,), generator=g).double() * 2.0 ** -s
    res = torch.randint(-8, 9, (B, C, H, W), generator=g).double() * 2.0 ** -s
    return y, bias, res


@pytest.mark.parametrize("C", [32, 12])                                 # 16-byte vectors (k_bias_act8) | one element per thread (k_bias_act1)
def test_bias_act_equals_the_fp64_reference_on_exact_operands(C):
    from strongsort_yolo_amd import fused
    for s in (0, 3):
        y, bias, res = _elementwise_operands(C + s, 3, C, 5, 7, s)
        for act in R.EXACT_ACTS:
            for r in (None, res):
                st = []
                ref = R.bias_act_ref(y, bias, act, r, stages=st)
                R.assert_half_exact(st[1:], "bias_act_")
                got = fused.bias_act_(_cl(y).clone(), _cl(bias), act, res=None if r is None else _cl(r))
                _same(got, _cl(ref), f"bias_act_ C={C} s={s} {act} res={r is not None}")


def test_bias_act_place_equals_the_fp64_reference_on_exact_operands():
    from strongsort_yolo_amd import fused
    B, C, H, W, CT = 3, 32, 9, 13, 96
    for s in (0, 3):
        y, bias, res = _elementwise_operands(40 + s, B, C, H, W, s)
        for act in R.EXACT_ACTS:
            for vname, (use_res, after) in R.VARIANTS.items():
                st = []
                ref = _cl(R.bias_act_ref(y, bias, act, res if use_res else None, after, stages=st))
                R.assert_half_exact(st[1:], "bias_act_place")
                cat = torch.full((B, CT, H, W), 5.0, dtype=torch.float16, device=_dev()).contiguous(memory_format=torch.channels_last)
                out2 = torch.full((B, 16, H, W), 7.0, dtype=torch.float16, device=_dev()).contiguous(memory_format=torch.channels_last)
                fused.bias_act_place(_cl(y), _cl(bias), act, cat, 40, res=_cl(res) if use_res else None, res_after=after, out2=out2, c0=16)
                _same(cat[:, 40:72], ref, f"bias_act_place s={s} {act} {vname}")
                _same(out2, ref[:, 16:], f"bias_act_place mirror s={s} {act} {vname}")
                assert bool((cat[:, :40] == 5.0).all()) and bool((cat[:, 72:] == 5.0).all())


# ================================================================ Part B: N(0,1) operands, all four activations
def _partb_check(tag, got, chain, act):
    """chain(acc) -> (reference, stages) runs the fp64 epilogue on a convolution sum.  Prints the figures, then asserts the elementwise bound
    and the not-bit-equal count against the fp32 CPU convolution's; for sigmoid the count leaves out the elements inside
    f16_ref.act_exempt's zone (the cause is stated there), whose size and raw count are printed too."""
    ops, run = chain
    st = []
    ref, cpu32 = run(ops["acc"], st), run(ops["acc32"], [])
    got = got.double().cpu()
    bound, exempt = R.elementwise_bound(st, ref, act), R.act_exempt(st, act)
    worst = float(((got - ref).abs() / bound).max())
    raw, n_dev, n_ref = int((got != ref).sum()), int(((got != ref) & ~exempt).sum()), int((cpu32 != ref).sum())
    print(f"F16SHARE {tag}: elements {ref.numel()} device {n_dev} (raw {raw}, zone {int(exempt.sum())}) cpu_fp32 {n_ref} allowed {R.share_bound(n_ref)} "
          f"max_err/bound {worst:.3f}")
    assert bool(torch.isfinite(got).all()) and worst <= 1.0, (tag, worst)
    assert n_dev <= R.share_bound(n_ref), (tag, n_dev, raw, n_ref, ref.numel())


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("case", R.PARTB_CASES, ids=lambda c: "-".join(map(str, c)))
def test_pointwise_and_conv3x3_on_normal_operands_stay_within_one_flip_per_rounding(case, act):
    """Measured on the MI355X (profiles/f16_exact_shares.txt, docs/F16_OPERATORS.md section 5), over the 152 launches of this test and the
    next: the kernels differ from the fp64 chain in 2 .. 13 elements with none, 1 .. 9 with relu, 0 .. 30 with silu (at most 0.036 % of a
    tensor) where the fp32 CPU convolution differs in 1 .. 17, every one below 4 x the CPU's + 20 as it stands; the worst error is 1.000 of
    the elementwise bound.  With sigmoid the raw count is 4 .. 109 and passes the bound in one case (109 and 79 against 4 * 7 + 20 and
    4 * 6 + 20 of 184320 elements, K = 16): structural ties of sigmoid near v = 0, stated at f16_ref.act_exempt, whose derived zone the
    sigmoid count leaves out (counted: at most 11)."""
    kind, B, K, H, W, N, stride = case
    ops = R.normal_conv_operands(K * 1000 + N, B, K, H, W, N, 3 if kind == "c3" else 1, stride)
    c = dict(kind=kind, B=B, K=K, H=H, W=W, N=N, stride=stride)
    x, w, bias, res = _cl(ops["x"]), _weights(kind, ops["w"]), _cl(ops["bias"]), _cl(ops["res"])
    M, KK, _, _ = R.case_dims(c)
    for vname, (use_res, after) in R.VARIANTS.items():
        run = lambda acc, st, r=ops["res"] if use_res else None, after=after: R.epilogue(acc, ops["bias"], act, r, after, st)
        for epi, sk in R.case_settings(c):
            with _options(epi, sk):
                got = _run(kind, x, w, bias, stride, act, res=res if use_res else None, res_after=after)
            form = R.pw_form(M, KK, N, kind == "c3", True, epi, sk)
            _partb_check(f"{kind} {(B, K, H, W)}->{N}/s{stride} {act} {vname} {form}", got, (ops, run), act)


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("B,H,W,co", R.PARTB_CONV0)
def test_conv0_on_normal_operands_stays_within_one_flip_per_rounding(B, H, W, co, act):
    from strongsort_yolo_amd import fused
    ops = R.normal_conv_operands(H + co, B, 3, H, W, co, 3, 2)
    conv, x = _conv_module(ops["w"], ops["bias"], 2, 1), _cl(ops["x"])
    assert fused.conv0_ok(x, conv)
    got = fused.conv0(x, fused.conv0_weight(torch.nn.Module(), conv), conv.bias, act)
    _partb_check(f"conv0 {(B, H, W)}->{co} {act}", got, (ops, lambda acc, st: R.epilogue(acc, ops["bias"], act, stages=st)), act)


# ================================================================ silu and sigmoid on exact pre-activations
@pytest.mark.parametrize("act", ["silu", "sigmoid"])
def test_silu_and_sigmoid_on_the_exact_grid_equal_the_rounded_fp64_value(act):
    """Pre-activations k / 8 in [-40, 40] through act_apply - in k_bias_act8 and in k_pw's epilogue (a one-hot weight column makes the
    convolution sum the grid value itself): the output must be h(act64(v)) at every point whose fp64 value is further than
    f16_ref.act_delta from a rounding boundary (derivation there; tests/test_f16_ref_cpu.py caps the exempt points at 1 %)."""
    from strongsort_yolo_amd import fused
    want, exempt = R.act_grid_ref(act)
    v = np.zeros(648)
    v[:641] = R.act_grid()
    grid = torch.from_numpy(v).view(1, 81, 1, 8).permute(0, 3, 2, 1)                   # [1, 8, 1, 81]: 81 pixels x 8 channels hold the 648 values
    zero = torch.zeros(8, dtype=torch.float16, device=_dev())
    got = fused.bias_act_(_cl(grid).clone(), zero, act)
    a = got.permute(0, 3, 2, 1).reshape(-1)[:641].cpu().numpy()
    col = torch.zeros(1, 8, 1, 641, dtype=torch.float64)
    col[0, 0, 0] = torch.from_numpy(R.act_grid())
    wsel = torch.zeros(8, 8, dtype=torch.float64)
    wsel[:, 0] = 1.0
    b = fused.pointwise(_cl(col), _cl(wsel), zero, act)[0, 3, 0].cpu().numpy()
    for name, g in (("bias_act_", a), ("pointwise", b)):
        g = np.ascontiguousarray(g)
        differ = (g.view(np.uint16) != want.view(np.uint16)) & ~((g == 0) & (want == 0))
        print(f"F16GRID {act} {name}: differ {int(differ.sum())} exempt {int(exempt.sum())} differ-and-exempt {int((differ & exempt).sum())}")
        assert not (differ & ~exempt).any(), (name, R.act_grid()[differ & ~exempt], g[differ & ~exempt], want[differ & ~exempt])


# ================================================================ depthwise 3x3 (k_dw3x3)
@pytest.mark.parametrize("case", R.DW_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dwconv3x3_equals_the_fp64_reference_on_exact_operands(case):
    from strongsort_yolo_amd import fused
    for s in R.dw_shifts(case):
        ops, refs = R.exact_dw(*case, s)
        x, w9, bias = _cl(ops["x"]), _cl(R.w9_of(ops["wd"])), _cl(ops["bias"])
        for act, ref in refs.items():
            got = fused.dwconv3x3(x, w9, bias, act)
            assert got.is_contiguous(memory_format=torch.channels_last)
            _same(got, _cl(ref), f"dwconv3x3 {case} s={s} {act}")


def _grid_map():
    """act_grid()'s 641 values as an [1, 8, 1, 81] map (648 elements, the last seven 0) and the function that reads them back."""
    v = np.zeros(648)
    v[:641] = R.act_grid()
    return torch.from_numpy(v).view(1, 81, 1, 8).permute(0, 3, 2, 1), lambda t: np.ascontiguousarray(t.permute(0, 3, 2, 1).reshape(-1)[:641].cpu().numpy())


@pytest.mark.parametrize("act", ["silu", "sigmoid"])
def test_dwconv3x3_silu_and_sigmoid_on_the_exact_grid_equal_the_rounded_fp64_value(act):
    """A centre tap of 1, the other taps and the bias 0: the sum is the input value, k / 8 in [-40, 40]; the output must be h(act64(v))
    outside f16_ref.act_exempt's zone, as for the other epilogues."""
    from strongsort_yolo_amd import fused
    want, exempt = R.act_grid_ref(act)
    grid, back = _grid_map()
    w9 = torch.zeros(9, 8, dtype=torch.float16, device=_dev())
    w9[4] = 1.0
    g = back(fused.dwconv3x3(_cl(grid), w9, torch.zeros(8, dtype=torch.float16, device=_dev()), act))
    differ = (g.view(np.uint16) != want.view(np.uint16)) & ~((g == 0) & (want == 0))
    print(f"F16GRID {act} dwconv3x3: differ {int(differ.sum())} exempt {int(exempt.sum())} differ-and-exempt {int((differ & exempt).sum())}")
    assert not (differ & ~exempt).any(), (R.act_grid()[differ & ~exempt], g[differ & ~exempt], want[differ & ~exempt])


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("case", R.DW_PARTB, ids=lambda c: "x".join(map(str, c)))
def test_dwconv3x3_on_normal_operands_stays_within_one_flip(case, act):
    """One rounding point: |out - ref| <= ulp_h(ref), and the count of elements not bit-equal to the fp64 chain against the count of the
    same nine taps in fp32 on the CPU (figures: docs/F16_OPERATORS.md section 6)."""
    from strongsort_yolo_amd import fused
    ops = R.normal_dw_operands(case[1] * 100 + case[2], *case)
    got = fused.dwconv3x3(_cl(ops["x"]), _cl(R.w9_of(ops["wd"])), _cl(ops["bias"]), act)
    _partb_check(f"dw3x3 {case} {act}", got, (ops, lambda acc, st: R.dw_epilogue(acc, act, st)), act)


# ================================================================ max pooling (k_maxpool)
@pytest.mark.parametrize("case", R.MAXPOOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_maxpool_equals_torch_on_an_all_negative_map(case):
    """No arithmetic: equal to F.max_pool2d of the same half numbers in float64 on the CPU.  Every value is negative, so a window padded
    with 0 instead of -inf fails."""
    from strongsort_yolo_amd import fused
    n, c, hh, ww, k, stride, pad = case
    x = R.negative_half_map(n, c, hh, ww)
    ref = R.maxpool_ref(x, k, stride, pad)
    got = fused.maxpool(_cl(x), k, stride, pad)
    assert got.is_contiguous(memory_format=torch.channels_last)
    _same(got, _cl(ref), f"maxpool {case}")


# ================================================================ C2PSA attention (k_psa_attn)
def _psa(qkv, pe, heads, scale):
    """[B, N, heads * 128] (and pe [B, N, heads * 64]) fp64 -> the launch through fused.psa_attention on a 1 x N map -> [B, N, heads * 64]."""
    from strongsort_yolo_amd import fused
    as_map = lambda t: _cl(t.permute(0, 2, 1).unsqueeze(2))
    out = fused.psa_attention(as_map(qkv), None if pe is None else as_map(pe), heads, scale)
    assert out.shape == (qkv.shape[0], heads * 64, 1, qkv.shape[1]) and out.is_contiguous(memory_format=torch.channels_last)
    return out.squeeze(2).permute(0, 2, 1)


@pytest.mark.parametrize("with_pe", [False, True], ids=["plain", "pe"])
@pytest.mark.parametrize("case", R.PSA_CASES, ids=lambda c: "x".join(map(str, c)))
def test_psa_attention_equals_the_fp64_reference_on_exact_operands(case, with_pe):
    """One key per query (a seeded permutation per head and image; every real score negative, so a padded key left unmasked would win)
    and the uniform distribution over a seeded subset of 2^k keys: both rest on __expf(0) == 1 and must be EQUAL."""
    B, heads, N = case
    for make in (R.exact_psa_onehot, R.exact_psa_uniform):
        qkv, pe, ref = make(B, heads, N, with_pe)
        got = _psa(qkv, pe, heads, 1.0)
        _same(got, ref.to(_dev(), torch.float16), f"psa_attention {make.__name__} {case} pe={with_pe}")


def test_psa_attention_refuses_sizes_past_its_caps():
    from strongsort_yolo_amd import lib
    L = lib.load()
    buf = torch.zeros(257 * 128, dtype=torch.float16, device=_dev())
    for B, N, heads in ((1, 257, 1), (1, 16, 0), (1, 16, 65)):
        assert L.ss_op_psa_attention_f16(None, buf.data_ptr(), None, buf.data_ptr(), B, N, heads, 1.0) == lib.SS_ERR_INVALID, (B, N, heads)
    assert not bool(buf.any())


@pytest.mark.parametrize("with_pe", [False, True], ids=["plain", "pe"])
@pytest.mark.parametrize("case", R.PSA_PARTB, ids=lambda c: "x".join(map(str, c)))
def test_psa_attention_on_normal_operands_stays_within_its_derived_bound(case, with_pe):
    """N(0,1) q, k, v, pe, the module's scale: every element within f16_ref.psa_bound of the fp64 chain (p rounded to half, o rounded to
    half before pe, the sum rounded to half), and the count of elements not bit-equal held against the count of the same chain in
    float32 on the CPU (figures: docs/F16_OPERATORS.md section 8).  The count leaves out f16_ref.psa_exempt's zone - outputs that a
    probability within half an fp32 ulp of a rounding midpoint can move; the cause and the one measured case, 27 raw against 24 at
    (2, 2, 15), are stated there - and prints its size and the raw count, as _partb_check does for sigmoid."""
    B, heads, N = case
    qkv, pe = R.normal_psa_operands(B, heads, N)
    pe = pe if with_pe else None
    st = []
    ref = R.psa_ref(qkv, pe, heads, R.PSA_SCALE, st)
    cpu32 = R.psa_ref(qkv, pe, heads, R.PSA_SCALE, f32=True)
    bound = R.psa_bound(qkv, pe, heads, R.PSA_SCALE, st, ref)
    got = _psa(qkv, pe, heads, R.PSA_SCALE).double().cpu()
    worst = float(((got - ref).abs() / bound).max())
    exempt = R.psa_exempt(qkv, heads, st)
    raw, n_dev, n_ref = int((got != ref).sum()), int(((got != ref) & ~exempt).sum()), int((cpu32 != ref).sum())
    print(f"F16SHARE psa {case} pe={with_pe}: elements {ref.numel()} device {n_dev} (raw {raw}, zone {int(exempt.sum())}) cpu_fp32 {n_ref} "
          f"allowed {R.share_bound(n_ref)} max_err/bound {worst:.3f}")
    assert bool(torch.isfinite(got).all()) and worst <= 1.0, (case, worst)
    assert n_dev <= R.share_bound(n_ref), (case, n_dev, raw, n_ref, ref.numel())


# ================================================================ the v8 decode on half inputs (k_v8_decode)
def _decode16(o, nc, n_ext, mode, boxes=None, clss=None, box_bias=None, cls_bias=None):
    from strongsort_yolo_amd import fused
    pick = lambda k, v: [_cl(t) for t in (o[k] if v is None else v)]
    return fused.v8_decode(pick("boxes", boxes), pick("clss", clss), pick("box_bias", box_bias), pick("cls_bias", cls_bias),
                           R.R32.DECODE_STRIDES, nc, pick("ext", None) if n_ext else None, n_ext, mode)


@pytest.mark.parametrize("case", R.DECODE16_CASES, ids=lambda c: "-".join(map(str, c)))
def test_v8_decode_f16_equals_the_fp64_reference_on_one_hot_logits(case):
    """B = 2, A = 210 (two blocks of 128 anchors, the level borders at 156 and 198): every logit split between the tensor and a bias that
    is not zero - the box bias moves the winner of the tensor alone - and every row of pred equal."""
    nc, cls_ld, n_ext, ext_ld, mode = case
    o, ref = R.exact_decode16(2, *case)
    got = _decode16(o, nc, n_ext, mode)
    assert got.dtype == torch.float32
    _same(got, ref.to(_dev(), torch.float32), f"v8_decode f16 {case}")


def _ratio(got, ref, bound, what):
    r = (got.double().cpu() - ref).abs() / bound
    worst = float(r.max())
    print(f"F16SHARE {what}: worst err / bound = {worst:.4f} over {ref.numel()} elements")
    assert bool(torch.isfinite(got).all()) and worst <= 1.0, f"{what}: {int((r > 1).sum())} elements outside the bound, worst err / bound = {worst}"


def test_v8_decode_f16_sigmoid_and_dfl_stay_within_their_derived_bounds():
    """The fp32 kernel's test for the half one, whose __expf costs (1.25 |x| + 6) 2^-24 per term: class rows and keypoint confidences are
    sigmoids of multiples of 1/8 in [-16, 16] (f16_ref.act_bound16), box rows come from DFL logits k / 8 in [-4, 4]
    (f16_ref.decode_box_bound16), each logit split between the tensor and a bias; the dyadic keypoint x / y rows stay exact."""
    F32 = R.R32
    nc, n_ext, B = 5, 6, 2
    g = torch.Generator().manual_seed(5)
    v = F32.act_grid()
    o = dict(boxes=[], clss=[], box_bias=[], cls_bias=[], ext=[])
    box_tot, cls_tot = F32.dfl_logits(B), []
    for (hh, ww), bt in zip(F32.DECODE_LEVELS, box_tot):
        ct = v[torch.randint(0, len(v), (B, 8, hh, ww), generator=g)]
        bb, cb = torch.randint(-32, 33, (64,), generator=g).double() / 8, torch.randint(-32, 33, (8,), generator=g).double() / 8
        cls_tot.append(ct)
        o["boxes"].append(bt - bb.view(1, -1, 1, 1)); o["box_bias"].append(bb)
        o["clss"].append(ct - cb.view(1, -1, 1, 1)); o["cls_bias"].append(cb)
        e = torch.randint(-64, 65, (B, 8, hh, ww), generator=g).double() / 8
        e[:, 2::3] = v[torch.randint(0, len(v), e[:, 2::3].shape, generator=g)]
        o["ext"].append(e)
    st = []
    ref = F32.v8_decode_ref(box_tot, cls_tot, F32.DECODE_STRIDES, nc, o["ext"], n_ext, 1, stages=st)
    got = _decode16(o, nc, n_ext, 1)
    logits = lambda ts, rows: torch.stack([torch.cat([t[:, r].reshape(B, -1) for t in ts], 1) for r in rows], 1)      # [B, rows, A]
    conf = [k for k in range(n_ext) if k % 3 == 2]
    xy = [4 + nc + k for k in range(n_ext) if k % 3 != 2]
    _ratio(got[:, :4], ref[:, :4], R.decode_box_bound16(st[0], F32.DECODE_STRIDES), "decode f16 DFL box rows")
    _ratio(got[:, 4:4 + nc], ref[:, 4:4 + nc], R.act_bound16(logits(cls_tot, range(nc)), ref[:, 4:4 + nc]), "decode f16 class sigmoid")
    rows = [4 + nc + k for k in conf]
    _ratio(got[:, rows], ref[:, rows], R.act_bound16(logits(o["ext"], conf), ref[:, rows]), "decode f16 keypoint confidence sigmoid")
    _same(got[:, xy], ref[:, xy].to(_dev(), torch.float32), "decode f16 keypoint x / y rows")


# ================================================================ OSNet's aggregation gate (k_gate_mean, k_gate_apply)
@pytest.mark.parametrize("case", R.GATE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gate_sum_and_gate_apply_equal_the_fp64_reference_on_exact_operands(case):
    """Gates of exactly 1/2, 1 and (but for 4e-18) 0, different per channel, stream and image, on integer maps: gate_sum and gate_apply -
    the latter from psum in 1, 3 and 8 parts that add up to the same sums - must both equal the reference, and so each other."""
    from strongsort_yolo_amd import fused
    ops, ref = R.exact_gate(*case)
    xs = [_cl(x) for x in ops["xs"]]
    w = [_cl(ops[k]) for k in ("w1", "b1", "w2", "b2")]
    want = _cl(ref)
    _same(fused.gate_sum(xs, *w), want, f"gate_sum {case}")
    for parts in R.GATE_PARTS:
        psum = R.gate_psum(ops["xs"], parts).to(_dev(), torch.float32).contiguous()
        _same(fused.gate_apply(xs, psum, *w), want, f"gate_apply {case} parts={parts}")
