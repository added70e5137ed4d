"""tests/f16_ref.py against itself, without a GPU: every case of tests/test_gpu_nets_exact.py builds inside the exact range, the case list
reaches every kernel form launch_pw can choose, and the oracle bites - three mutants of the fp64 reference are caught."""
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
