"""tests/f16_ref.py against itself, without a GPU: every case of tests/test_gpu_nets_exact.py builds inside the exact range, the case list
reaches every kernel form launch_pw can choose, and the oracle bites - three mutants of the fp64 reference are caught.  The same for the
depthwise 3x3, max pooling, the attention, the half decode and the gate: their cases stay exact, ten mutants differ on the listed cases,
the re-derived bounds hold for a float32 evaluation on the CPU, and the zones the counts leave out stay below 1 % of a tensor."""
import numpy as np
import pytest
import torch

from tests import f16_ref as R


@pytest.mark.parametrize("case", R.PW_CASES, ids=R.case_id)
def test_pointwise_and_conv3x3_cases_stay_in_the_exact_range(case):
    for s in case["ss"]:
        ops = R.case_operands(case, s)
        refs = R.exact_conv_refs(ops, R.case_id(case))                 # asserts half-exactness at every rounding point
        assert len(refs) == 6 and float(ops["acc"].abs().max()) * 2 ** s <= 2048
        assert torch.equal(R.conv_acc(ops["x"].float(), ops["w"].float(), case["stride"]).double(), ops["acc"])       # fp32 sums: exact too
        assert float(refs["plain", "none"].abs().max()) > 0


def test_other_operator_cases_stay_in_the_exact_range():
    for s in (0, 3):
        for c in R.CONV0_CASES:
            R.exact_conv0(*c, s)
        for c in R.LIGHTCONV_CASES:
            _, ref = R.exact_lightconv(*c, s)
            assert float(ref.max()) > 0
        for c in R.STEM_CASES:
            R.exact_stem(*c, s)
        for c in R.HEAD_CASES:
            _, ref = R.exact_head(*c, s)
            assert float(ref.max()) > 0


def test_a_case_outside_the_exact_range_fails_to_build():
    ops = R.exact_conv_operands(1, 1, 8, 3, 3, 8, 1, 1, 0)
    ops["acc"] = ops["acc"] + 2049.5                                   # not a half number
    with pytest.raises(AssertionError):
        R.exact_conv_refs(ops)
    with pytest.raises(AssertionError):
        R.assert_any_order(torch.tensor([2.0 ** 25]), 1.0)


def test_case_list_reaches_every_form_of_launch_pw():
    """k_pw<BN, PT, CONV3, VEC_EPI> over the seven (BN, PT) launch_pw chooses - <128, 1> is instantiated for no launch: N > 64 below 32768
    pixels takes <64, 1> - and k_pw_splitk<32 | 64, true>: 7 * 2 * 2 + 2 = 30 forms."""
    want = set()
    for bn, pt in ((32, 1), (32, 2), (64, 1), (64, 2), (80, 1), (80, 2), (128, 2)):
        want |= {("pw", bn, pt, False, False), ("pw", bn, pt, False, True), ("pw", bn, pt, True, False), ("pw", bn, pt, True, True)}
    want |= {("splitk", 32), ("splitk", 64)}
    assert len(want) == 30 and want == R.REACHABLE_FORMS
    got = {}
    for c in R.PW_CASES:
        for f in R.case_forms(c):
            got.setdefault(f, []).append(R.case_id(c))
    assert set(got) == want, (sorted(want - set(got)), sorted(set(got) - want))
    # the thresholds themselves
    assert R.pw_form(4096, 576, 64, True, True) == ("splitk", 64) and R.pw_form(4097, 576, 64, True, True) == ("pw", 64, 1, True, True)
    assert R.pw_form(4096, 504, 64, True, True) == ("pw", 64, 1, True, True) and R.pw_form(17, 576, 32, True, True) == ("splitk", 32)
    assert R.pw_form(17, 576, 32, True, False) == ("pw", 32, 1, True, False) and R.pw_form(17, 576, 32, True, True, 0) == ("pw", 32, 1, True, False)
    assert R.pw_form(17, 576, 32, True, True, 1, 0) == ("pw", 32, 1, True, True) and R.pw_form(17, 576, 32, False, True) == ("pw", 32, 1, False, True)
    assert R.pw_form(32767, 8, 72, False, True) == ("pw", 64, 1, False, True) and R.pw_form(32768, 8, 72, False, True) == ("pw", 128, 2, False, True)
    assert R.pw_form(32768, 8, 80, False, True) == ("pw", 80, 2, False, True) and R.pw_form(32768, 8, 64, False, True) == ("pw", 64, 2, False, True)


def _mutant_case(s):
    c = dict(kind="c3", B=2, K=16, H=7, W=9, N=24, stride=1, ss=(s,))
    return c, R.case_operands(c, s)


@pytest.mark.parametrize("s", [0, 3])
def test_mutant_one_tap_dropped_for_one_output_column_differs_on_exact_operands(s):
    c, ops = _mutant_case(s)
    ref = R.epilogue(ops["acc"], ops["bias"], "relu")
    w = ops["w"].clone()
    w[:, :, 0, 0] = 0
    acc = ops["acc"].clone()
    acc[:, :, :, 1] = R.conv_acc(ops["x"], w, 1)[:, :, :, 1]
    assert not torch.equal(R.epilogue(acc, ops["bias"], "relu"), ref)


@pytest.mark.parametrize("s", [0, 3])
def test_mutant_one_input_channel_dropped_at_one_tap_differs_on_exact_operands(s):
    c, ops = _mutant_case(s)
    ref = R.epilogue(ops["acc"], ops["bias"], "none")
    w = ops["w"].clone()
    w[:, c["K"] - 1, 2, 2] = 0
    assert not torch.equal(R.epilogue(R.conv_acc(ops["x"], w, 1), ops["bias"], "none"), ref)


@pytest.mark.parametrize("case", R.PARTB_CASES[:2] + R.PARTB_CASES[3:4])
@pytest.mark.parametrize("act", ["none", "silu", "sigmoid"])
def test_mutant_truncated_intermediate_exceeds_the_share_bound_on_normal_operands(case, act):
    """Part B's second assertion separates a correct fp32-accumulating kernel from one that rounds its intermediate toward zero: the
    fp32 CPU chain stays inside its own bound, the mutant is far outside, and the mutant also passes the old 4e-3 * max tolerance."""
    kind, B, K, H, W, N, stride = case
    ops = R.normal_conv_operands(K + N, B, K, H, W, N, 3 if kind == "c3" else 1, stride)
    st = []
    ref = R.epilogue(ops["acc"], ops["bias"], act, stages=st)
    cpu32 = R.epilogue(ops["acc32"], ops["bias"], act)
    mut = R.epilogue(ops["acc"], ops["bias"], act, hc=R.h_trunc)
    exempt = R.act_exempt(st, act)
    assert (int(exempt.sum()) == 0) if act != "sigmoid" else (0 < int(exempt.sum()) <= 0.01 * ref.numel())       # the zone stays a sliver
    n_ref, n_mut = int((cpu32 != ref).sum()), int(((mut != ref) & ~exempt).sum())
    assert n_ref <= R.share_bound(n_ref) and n_mut > R.share_bound(n_ref), (n_ref, n_mut, ref.numel())
    assert n_mut > (0.02 if act == "sigmoid" else 0.1) * ref.numel()                         # (sigmoid's slope of 1/4 absorbs most flips of c)
    assert bool(((cpu32 - ref).abs() <= R.elementwise_bound(st, ref, act)).all())
    assert float((mut - ref).abs().max()) <= 4e-3 * (float(ref.abs().max()) + 1.0)          # invisible to the scaled tolerance


def test_half_helpers():
    t = torch.tensor([1.0, 1.5, 2047.0, 2048.0, 0.75, 2.0 ** -14, 2.0 ** -20, 0.0, -3.0], dtype=torch.float64)
    assert R.ulp_h(t).tolist() == [2.0 ** -10, 2.0 ** -10, 1.0, 2.0, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -9]
    v = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -30, 2048.0, 2049.0 - 2.0 ** -20, 2.0 ** -25 + 2.0 ** -40, 0.0])
    assert np.allclose(R.near_tie(v), [2.0 ** -12, 0.0, 2.0 ** -30, 0.5, 2.0 ** -20, 2.0 ** -40, 2.0 ** -25], rtol=0, atol=0)
    x = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -30, -(1.0 + 2.0 ** -11 + 2.0 ** -30), 1.0 + 3 * 2.0 ** -11], dtype=torch.float64)
    assert R.h(x).tolist() == [1.0 + 2.0 ** -10, -(1.0 + 2.0 ** -10), 1.0 + 2.0 ** -9]       # one rounding (via float: 1.0), ties to even
    assert R.h_trunc(x).tolist() == [1.0, -1.0, 1.0 + 2.0 ** -10]


@pytest.mark.parametrize("act", ["silu", "sigmoid"])
def test_act_grid_exemptions_are_few_and_an_fp32_emulation_matches(act):
    """At most 1 % of the 641 grid points may lie within act_delta of a rounding boundary; act_apply's sequence emulated in fp32 (numpy's
    exp for v_exp_f32, a division for v_rcp_f32) equals h(act64(v)) at every point that is not exempt."""
    want, exempt = R.act_grid_ref(act)
    assert want.shape == (641,) and int(exempt.sum()) <= 6, int(exempt.sum())
    v = R.act_grid().astype(np.float32)
    r = np.float32(1) / (np.float32(1) + np.exp(-v))
    got = ((v * r) if act == "silu" else r).astype(np.float16)
    bad = (got.view(np.uint16) != want.view(np.uint16)) & ~exempt & ~((got == 0) & (want == 0))
    assert not bad.any(), R.act_grid()[bad]


# ================================================================ the operators outside the convolution family
def test_depthwise_maxpool_decode_and_gate_cases_stay_in_the_exact_range():
    for c in R.DW_CASES:
        for s in R.dw_shifts(c):
            ops, refs = R.exact_dw(*c, s)
            assert float(refs["relu"].max()) > 0 and float(refs["none"].min()) < 0
            assert torch.equal(R.dw_taps(ops["x"].float(), ops["wd"].float()).double(), R.dw_taps(ops["x"], ops["wd"]))      # fp32 sums: exact too
    assert R.DW_CASES[-1][1] // 8 * R.DW_CASES[-1][2] * R.DW_CASES[-1][3] > 4096 * 256                # the grid-stride loop's second pass
    for c in R.DECODE16_CASES:
        R.exact_decode16(2, *c)
    for c in R.GATE_CASES:
        ops, _ = R.exact_gate(*c)
        for parts in R.GATE_PARTS:
            ps = R.gate_psum(ops["xs"], parts)
            assert ps.shape[2] == parts and torch.equal(ps.sum(2), torch.stack([x.sum((2, 3)) for x in ops["xs"]]))
    n, c, hh, ww, k, st, p = R.MAXPOOL_CASES[-1]
    assert n * (c // 8) * ((hh + 2 * p - k) // st + 1) * ((ww + 2 * p - k) // st + 1) > 4096 * 256 and n * c * hh * ww * 2 < 18e6


@pytest.mark.parametrize("case", R.PSA_CASES, ids=lambda c: "x".join(map(str, c)))
def test_attention_cases_stay_in_the_exact_range(case):
    """Both constructions, with and without pe (asserted inside the generators), and the same operands in float32 on the CPU: exact too."""
    for make in (R.exact_psa_onehot, R.exact_psa_uniform):
        for with_pe in (False, True):
            qkv, pe, ref = make(*case, with_pe)
            assert torch.equal(R.psa_ref(qkv, pe, case[1], 1.0, f32=True), ref), (make.__name__, case, with_pe)


def test_mutants_of_the_depthwise_taps_differ_on_the_listed_cases():
    """A tap that leaks across an image border (the images read as one tall map) and a w9 laid out [C][9] where the kernel reads [9][C]."""
    leak_seen = 0
    for c in R.DW_CASES[:-1]:
        for s in R.dw_shifts(c):
            ops, refs = R.exact_dw(*c, s)
            leak = R.dw3x3_ref(ops["x"], ops["wd"], ops["bias"], "none", leak=True)
            assert torch.equal(leak, refs["none"]) == (c[0] == 1), c                # one image has no neighbour to leak from
            leak_seen += c[0] > 1
            ch = c[1]
            wt = R.w9_of(ops["wd"]).reshape(-1).reshape(ch, 9)                       # what a [C][9] reader finds in a [9][C] buffer
            if c[2] * c[3] > 1:                                                      # (on a 1 x 1 map only the centre tap is read)
                assert not torch.equal(R.dw3x3_ref(ops["x"], wt.reshape(ch, 3, 3), ops["bias"], "none"), refs["none"]), c
            mirrored = R.dw3x3_ref(ops["x"], ops["wd"].flip(2), ops["bias"], "none")
            assert torch.equal(mirrored, refs["none"]) == (c[3] == 1), c             # a mirrored tap shows wherever the map has two columns
    assert leak_seen >= 2


def test_mutant_max_pool_padded_with_zero_differs_on_every_padded_case():
    for n, c, hh, ww, k, st, p in R.MAXPOOL_CASES[:-1]:
        x = R.negative_half_map(n, c, hh, ww)
        ref = R.maxpool_ref(x, k, st, p)
        assert bool(torch.isfinite(ref).all()) and float(ref.max()) < 0
        assert torch.equal(R.maxpool_ref(x, k, st, p, 0.0), ref) == (p == 0), (n, c, hh, ww, k, st, p)


def test_mutants_of_the_attention_mask_and_key_pairing_differ_on_the_listed_cases():
    unmasked, swapped = [], []
    for case in R.PSA_CASES:
        qkv, pe, ref = R.exact_psa_onehot(*case, True)
        heads = case[1]
        if not torch.equal(R.psa_ref(qkv, pe, heads, 1.0, mask=False), ref):
            unmasked.append(case[2])
        if not torch.equal(R.psa_ref(qkv, pe, heads, 1.0, swap_pairs=True), ref):
            swapped.append(case[2])
        qkv, pe, ref = R.exact_psa_uniform(*case, False)
        if case[2] > 1:
            assert not torch.equal(R.psa_ref(qkv, pe, heads, 1.0, swap_pairs=True), ref), case
    assert unmasked == [c[2] for c in R.PSA_CASES if c[2] % 32], unmasked          # every size with a padded key sees the missing mask
    assert swapped == [c[2] for c in R.PSA_CASES], swapped


@pytest.mark.parametrize("case", R.PSA_PARTB, ids=lambda c: "x".join(map(str, c)))
def test_attention_bound_holds_in_float32_and_the_count_catches_unrounded_probabilities(case):
    """The derived bound holds for the same chain with every fp32 step in float32 on the CPU; a kernel that keeps p in fp32 (no rounding
    to half before the PV product) is far outside the count the fp32 chain sets, while it passes the old 1e-2 * (max + 1)."""
    B, heads, N = case
    qkv, pe = R.normal_psa_operands(B, heads, N)
    for use_pe in (None, pe):
        st = []
        ref = R.psa_ref(qkv, use_pe, heads, R.PSA_SCALE, st)
        cpu32 = R.psa_ref(qkv, use_pe, heads, R.PSA_SCALE, f32=True)
        bound = R.psa_bound(qkv, use_pe, heads, R.PSA_SCALE, st, ref)
        assert float(((cpu32 - ref).abs() / bound).max()) <= 1.0
        mut = R.psa_ref(qkv, use_pe, heads, R.PSA_SCALE, hp=lambda t: t.float().double())
        exempt = R.psa_exempt(qkv, heads, st)
        assert int(exempt.sum()) <= 0.01 * ref.numel(), (int(exempt.sum()), ref.numel())       # the zone stays a sliver: a condition
        n_ref, n_mut = int((cpu32 != ref).sum()), int(((mut != ref) & ~exempt).sum())
        assert n_mut > R.share_bound(n_ref) and n_mut > 0.02 * ref.numel(), (n_ref, n_mut, ref.numel())
        assert float((mut - ref).abs().max()) <= 1e-2 * (float(ref.abs().max()) + 1.0)
        assert float(bound.max()) < 0.1 * 1e-2 * (float(ref.abs().max()) + 1.0)      # every flip at once is still a tenth of the old tolerance


@pytest.mark.parametrize("case", R.DECODE16_CASES, ids=lambda c: "-".join(map(str, c)))
def test_mutants_of_the_decode_bias_and_anchor_offset_differ(case):
    nc, cls_ld, n_ext, ext_ld, mode = case
    o, ref = R.exact_decode16(2, *case)
    S = R.R32.DECODE_STRIDES
    no_box_bias = R.R32.v8_decode_ref(o["boxes"], o["cls_tot"], S, nc, o["ext"], n_ext, mode).float().double()
    no_cls_bias = R.R32.v8_decode_ref(o["box_tot"], o["clss"], S, nc, o["ext"], n_ext, mode).float().double()
    assert not torch.equal(no_box_bias[:, :4], ref[:, :4]) and torch.equal(no_box_bias[:, 4:], ref[:, 4:])
    assert not torch.equal(no_cls_bias[:, 4:4 + nc], ref[:, 4:4 + nc]) and torch.equal(no_cls_bias[:, :4], ref[:, :4])
    no_offset = R.R32.v8_decode_ref(o["box_tot"], o["cls_tot"], S, nc, o["ext"], n_ext, mode, offset=0.0).float().double()
    assert not torch.equal(no_offset[:, :2], ref[:, :2]) and torch.equal(no_offset[:, 2:], ref[:, 2:])


def test_mutants_of_the_gate_stream_order_and_channel_differ():
    for case in R.GATE_CASES:
        ops, ref = R.exact_gate(*case)
        T = case[3]
        if T > 1:
            assert not torch.equal(R.gate_ref(**ops, order=list(range(T))[::-1]), ref), case
        assert not torch.equal(R.gate_ref(**ops, shift=8), ref), case


def test_decode_bounds_rederived_for_expf_hold_in_float32():
    """The bounds of the half decode (__expf: (1.25 |x| + 6) 2^-24 per term) against the same formulas in numpy float32, and against the
    fp32 kernel's bounds: wider, by the factor the derivation gives and no more."""
    F32 = R.R32
    boxes = F32.dfl_logits(2)
    clss = [F32.act_grid()[torch.randint(0, 257, (2, 5, hh, ww), generator=torch.Generator().manual_seed(5))] for hh, ww in F32.DECODE_LEVELS]
    st = []
    ref = F32.v8_decode_ref(boxes, clss, F32.DECODE_STRIDES, 5, stages=st)
    b16, b32 = R.decode_box_bound16(st[0], F32.DECODE_STRIDES), F32.decode_box_bound(st[0], F32.DECODE_STRIDES)
    assert float(((F32.decode_boxes_f32(boxes, F32.DECODE_STRIDES) - ref[:, :4]).abs() / b16).max()) <= 1.0
    assert bool((b16 >= b32).all()) and float((b16 / b32).max()) <= R.DFL_REL16 / F32.DFL_REL == 1.8
    assert R.EXPF16_TERM == 16 and R.DFL_REL16 >= (2 * R.EXPF16_TERM + 15 + 16 + 1) * R.U32
    assert float(b16.max()) < 0.01                                                   # pixels: a hundredth, where the old test allows 0.512
    v = F32.act_grid()
    sg = torch.sigmoid(v)
    assert float(((F32.act_f32(v, False) - sg).abs() / R.act_bound16(v, sg)).max()) <= 1.0
    assert float((R.act_bound16(v, sg) / sg).max()) <= 28 * R.U32


@pytest.mark.parametrize("case", R.DW_PARTB)
@pytest.mark.parametrize("act", R.ACTS)
def test_depthwise_partb_zone_stays_a_sliver_and_the_count_catches_a_half_accumulator(case, act):
    """act_exempt leaves out at most 1 % of a tensor (sigmoid; nothing for the others) - a condition, checked here; the fp32 CPU chain stays
    inside the one-flip bound; a kernel that rounds its sum to half after every tap is far outside the count."""
    ops = R.normal_dw_operands(case[1] * 100 + case[2], *case)
    st = []
    ref = R.dw_epilogue(ops["acc"], act, st)
    cpu32 = R.dw_epilogue(ops["acc32"], act)
    exempt = R.act_exempt(st, act)
    assert (int(exempt.sum()) == 0) if act != "sigmoid" else (0 < int(exempt.sum()) <= 0.01 * ref.numel())
    assert bool(((cpu32 - ref).abs() <= R.elementwise_bound(st, ref, act)).all())
    x, wd, (n, c, hh, ww) = ops["x"], ops["wd"], case
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    a16 = ops["bias"].view(1, -1, 1, 1).expand(n, c, hh, ww)
    for dy in range(3):
        for dx in range(3):
            a16 = R.h(a16 + xp[:, :, dy:dy + hh, dx:dx + ww] * wd[:, dy, dx].view(1, c, 1, 1))
    n_ref, n_mut = int(((cpu32 != ref) & ~exempt).sum()), int(((R.dw_epilogue(a16, act) != ref) & ~exempt).sum())
    assert n_ref <= R.share_bound(n_ref) and n_mut > R.share_bound(n_ref) and n_mut > 0.05 * ref.numel(), (n_ref, n_mut, ref.numel())
