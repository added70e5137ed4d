"""tests/f32_ref.py against itself and against the library's host-only entry points, without a GPU: every case of
tests/test_gpu_nets32_exact.py builds inside the exact range (and a case pushed outside raises), the case lists reach every launch form,
the restated launcher rules agree with the library, the Part B bounds hold for a numpy float32 evaluation of the same formulas, and the
oracle bites - seven mutants of the fp64 reference differ from it on the exact operands, in elements a comparison scaled to the tensor's
maximum lets through."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import f32_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(conv_mt=0, conv_min=0, conv_waves=0, conv_wgs=1024, chains_form=2, chains_pre=-1, chains_min_n=128)


@pytest.fixture(scope="module")
def L():
    from strongsort_yolo_amd import lib
    lib.build()
    return lib.load()


def _source():
    return open(os.path.join(ROOT, "strongsort_yolo_amd", "csrc", "ss_ops32.hip")).read()


# ---------------------------------------------------------------- the exact range
@pytest.mark.parametrize("case", R.CONV_CASES, ids=R.conv_id)
def test_conv_cases_stay_in_the_exact_range(case):
    for s in (0, 3):
        ops = R.exact_conv(case, s)
        ref = R.conv_ref(ops["x"], ops["w"], ops["bias"], case["st"], res=ops["res"])
        R.assert_multiple(ref, ops["q"])
        assert torch.equal(R.conv_ref(ops["x"].float(), ops["w"].float(), ops["bias"].float(), case["st"], res=ops["res"].float()).double(), ref)   # an fp32 sum: exact too
        assert float(ref.abs().max()) >= 2.0 ** 20 * ops["q"] > 1e3 * float(ref.abs().median())               # the loud channel: three orders above the rest


def test_other_operator_cases_stay_in_the_exact_range():
    for s in (0, 3):
        for K, N in R.PW_PAIRS:
            for M in R.PW_MS:
                R.exact_pw(K, N, M, s)
        for c in R.CONV0_CASES:
            R.exact_conv0(*c, s)
        _, y, y1 = R.exact_stem(R.STEM_N, s)
        assert float(y.max()) > 0 and float(y1.max()) > 0
        for n, f, _ in R.HEAD_CASES:
            _, ref = R.exact_head(n, f, s)
            assert float(ref.max()) > 0
    c = R.PW_TPW2
    R.exact_pw(c["K"], c["N"], c["images"] * c["h"] * c["w"], 3)


@pytest.mark.parametrize("h,w,c", R.CHAIN_MAPS)
def test_chain_cases_stay_in_the_exact_range_and_alive(h, w, c):
    """exact_chains raises when a layer leaves the range or a chain output has fewer than 10 % positive elements or a zero maximum."""
    for s in (0, 3):
        for n in sorted(set(R.CHAIN_NS) | {nn for nn, _ in R.CHAIN_VALID[(h, w, c)]}):
            for bands in {R.chains_form(n, h, w, c, f, m, p)[1] for f, m, p in R.chain_settings(h, w, c)}:
                _, ys, psum = R.exact_chains(n, h, w, c, s, bands)
                assert psum.shape == (4, n, bands, c) and torch.equal(psum.sum(2), torch.stack([y.sum((2, 3)) for y in ys]))
                assert all(float((y > 0).double().mean()) >= 0.10 and float(y.max()) > 0 for y in ys)


@pytest.mark.parametrize("inst", R.TAIL_INSTS, ids=lambda i: "tail-%d-%d-%d-%d-%d" % i)
def test_tail_cases_stay_in_the_exact_range_with_diverse_exact_gates(inst):
    for s in (0, 3):
        ops, o, o2 = R.exact_tail(inst, R.TAIL_N, s)
        g = ops["gates"]
        assert set(g.unique().tolist()) == {0.0, 0.5, 1.0}
        assert R.gates_are_diverse(g) and R.gates_are_diverse(g[:, :R.TAIL_VALID])
        assert not R.gates_are_diverse(g[:, :1].expand(4, 3, g.shape[2]))                  # the check itself: one image three times is not diverse
        assert float((o2 > 0).double().mean()) > 0.1 and float((o > 0).double().mean()) > 0.1
        # the gates in numpy float32, the kernel's formula: the same three values
        pre = (torch.relu(ops["psum"].sum(2) / (R.TAIL_MAP[inst[0]][0] * R.TAIL_MAP[inst[0]][1]) @ ops["gw1"].t() + ops["gb1"]) @ ops["gw2"].t() + ops["gb2"])
        assert torch.equal(R.act_f32(pre, False), g)


def test_a_case_outside_the_exact_range_fails_to_build(monkeypatch):
    with pytest.raises(R.OutOfExactRange):
        R.assert_exact(torch.tensor([2.0 ** 24]), 1.0)
    R.assert_exact(torch.tensor([2.0 ** 24 - 1]), 1.0)
    with pytest.raises(R.OutOfExactRange):
        R.assert_multiple(torch.tensor([0.375, 0.3]), 0.125)
    real = R._ints
    monkeypatch.setattr(R, "_ints", lambda g, lo, hi, *shape: real(g, lo, hi, *shape) * 2.0 ** 17)         # every operand 2^17 times larger
    for build in (lambda: R.exact_conv(R.CONV_CASES[6], 0), lambda: R.exact_pw(128, 128, 16, 0), lambda: R.exact_head(3, 512, 0),
                  lambda: R.exact_chains(1, 16, 8, 32, 0, 1), lambda: R.exact_tail(R.TAIL_INSTS[4], 2, 0), lambda: R.exact_stem(1, 0)):
        with pytest.raises(R.OutOfExactRange):
            build()


# ---------------------------------------------------------------- form coverage
def _set(L, **kw):
    for k, v in kw.items():
        assert L.ss_op32_set_option(k.encode(), v) == 0, (k, v)


def _plan(L, c):
    v = [C.c_int() for _ in range(4)]
    assert L.ss_op32_conv_plan(c["n"], c["h"], c["w"], c["ci"], c["co"], c["ks"], c["st"], *[C.byref(t) for t in v]) == 0
    return tuple(t.value for t in v)


def test_conv_case_list_reaches_all_24_instantiations(L):
    """(KS, STRIDE) x MT {1, 2, 4, 5} x WAVES {4, 8} through ss_op32_conv_plan (host only) under the option states the GPU test runs; the
    default rule alone reaches the 8-wave forms only through conv_wgs."""
    got, by_default = {}, set()
    try:
        for c in R.CONV_CASES:
            for opt in R.conv_settings(c):
                _set(L, **dict(R.CONV_DEFAULTS, **opt))
                mt, wv, gx, gy = _plan(L, c)
                got.setdefault((c["ks"], c["st"], mt, wv), []).append((R.conv_id(c), opt))
                if not opt:
                    by_default.add((c["ks"], c["st"], mt, wv))
                if opt == dict(conv_wgs=1):
                    assert wv == (8 if (R.conv_dims(c)[2] + 15) // 16 >= 8 else 4)
    finally:
        _set(L, **R.CONV_DEFAULTS)
    want = {(ks, st, mt, wv) for ks, st in ((1, 1), (3, 1), (3, 2)) for mt in (1, 2, 4, 5) for wv in (4, 8)}
    assert len(want) == 24 and set(got) == want, sorted(want - set(got))
    assert all(wv == 4 for _, _, _, wv in by_default)                     # what the older tests ran
    # the instantiation list of the launcher itself
    src = _source()
    assert re.search(r"#define CV32M\(KS_, ST_\) CV32\(KS_, ST_, 1, 4\) CV32\(KS_, ST_, 1, 8\) CV32\(KS_, ST_, 2, 4\) CV32\(KS_, ST_, 2, 8\) "
                     r"CV32\(KS_, ST_, 4, 4\) CV32\(KS_, ST_, 4, 8\) \\\s+CV32\(KS_, ST_, 5, 4\) CV32\(KS_, ST_, 5, 8\)", src)
    assert "CV32M(1, 1) CV32M(3, 1) CV32M(3, 2)" in src
    # shapes: the K walk leaves its double-buffered loop at G = 1, 2, odd and even > 2; channel counts; the pixel counts
    gs = {R.conv_dims(c)[3] for c in R.CONV_CASES}
    assert {1, 2} <= gs and any(g % 2 and g > 2 for g in gs) and any(g % 2 == 0 and g > 2 for g in gs)
    assert {c["co"] for c in R.CONV_CASES} == {16, 32, 64, 80, 128}
    for ks, st in ((1, 1), (3, 1), (3, 2)):
        ms = {R.conv_dims(c)[2] for c in R.CONV_CASES if (c["ks"], c["st"]) == (ks, st)}
        assert {35, 128} <= ms, (ks, st, ms)
    assert {(c["ks"], c["ci"]) for c in R.CONV_CASES} >= {(1, 16), (1, 128), (3, 16), (3, 48), (3, 80)}


def test_conv_plan_checks_its_arguments_like_the_launcher(L):
    v = [C.byref(C.c_int()) for _ in range(4)]
    assert L.ss_op32_conv_plan(1, 8, 8, 16, 16, 3, 1, *v) == 0
    for bad in ((0, 8, 8, 16, 16, 3, 1), (1, 8, 8, 8, 16, 3, 1), (1, 8, 8, 16, 24, 3, 1), (1, 8, 8, 16, 16, 5, 1), (1, 8, 8, 16, 16, 1, 2),
                (1, 8, 8, 16, 16, 3, 3)):
        assert L.ss_op32_conv_plan(*bad, *v) < 0, bad
    assert L.ss_op32_conv_plan(1, 8, 8, 16, 16, 3, 1, None, None, None, None) < 0
    assert L.ss_op32_conv(None, None, 16, None, None, None, 0, None, 16, 1, 8, 8, 16, 16, 3, 1, 0) < 0      # null tensors: no launch


def test_pointwise_cases_reach_all_twelve_pairs_and_two_tiles_per_wave():
    pairs = [(int(a), int(b)) for a, b in re.findall(r"PW32\((\d+), (\d+)\)", _source())]
    assert len(pairs) == 12 and sorted(pairs) == sorted(R.PW_PAIRS)
    assert "while (tpw < 8 && tiles / (4 * tpw) > 8192) tpw *= 2;" in _source()            # what pw_tpw restates
    c = R.PW_TPW2
    M = c["images"] * c["h"] * c["w"]
    assert R.pw_tpw(M) == (2, 4112) and R.pw_tpw(M - c["h"] * c["w"])[0] == 1 and R.pw_tpw(105) == (1, 2)
    assert (c["K"], c["N"]) in R.PW_PAIRS and 2 * M * 16 * 4 < 72e6                           # x and out: under 70 MB
    assert (R.PW_VALID * R.PW_IMG_PX) % 16 != 0 and R.PW_VALID * R.PW_IMG_PX < max(R.PW_MS)   # the valid count cuts M inside a tile


def test_chain_cases_reach_every_form_and_agree_with_the_library(L):
    """ss_op32_chains_bands is host-only: the restated form choice must give its band count under every setting; the case list reaches
    k32_chainsR and k32_chains on all three maps and k32_chains3 with both PRE_ values on the two maps it is instantiated for."""
    got = set()
    try:
        for h, w, c in R.CHAIN_MAPS:
            for n in (1, 5, 127, 128, 300):
                for form in (0, 1, 2):
                    for min_n in (1, 128):
                        _set(L, chains_form=form, chains_min_n=min_n)
                        assert L.ss_op32_chains_bands(n, h, w, c) == R.chains_form(n, h, w, c, form, min_n)[1], (h, w, c, n, form, min_n)
            for n in R.CHAIN_NS:
                for form, min_n, pre in R.chain_settings(h, w, c):
                    got.add(R.chains_form(n, h, w, c, form, min_n, pre)[0])
    finally:
        _set(L, chains_form=2, chains_min_n=128)
    assert got == R.ALL_CHAIN_FORMS and len(got) == 10
    assert R.chains_form(127, 64, 32, 16)[0] == ("c3", 16, 32, True) and R.chains_form(128, 64, 32, 16)[0] == ("R", 16, 32)
    assert R.chains_form(5, 32, 16, 24, 1)[0] == ("c3", 24, 16, False) and R.chains_form(5, 16, 8, 32, 1)[0] == ("c", 32, 8)
    assert R.chains_form(5, 16, 8, 32, 2, 1)[0] == ("R", 32, 8)          # the 16 x 8 maps do take the row-stream form
    src = _source()
    assert "CHR(16, 32, false) CHR(24, 16, true) CHR(32, 8, true)" in src
    assert "CH32C(16, 32, true) CH32C(16, 32, false) CH32C(24, 16, true) CH32C(24, 16, false)" in src and "CH32(16, 32) CH32(24, 16) CH32(32, 8)" in src
    # valid counts that end inside a workgroup's images: two per workgroup (four on the 8-wide map, two per wave)
    for (h, w, c), cases in R.CHAIN_VALID.items():
        ipw = 4 if w == 8 else 2
        assert any(nv % ipw for _, nv in cases) and all(nv < n for n, nv in cases)
    assert any(nv % 4 == 1 for _, nv in R.CHAIN_VALID[(16, 8, 32)]) and any(nv % 4 == 3 for _, nv in R.CHAIN_VALID[(16, 8, 32)])


def test_tail_cases_are_the_six_instantiations():
    insts = [(int(a), int(b), int(c), int(d), e == "true") for a, b, c, d, e in re.findall(r"TL32\((\d+), (\d+), (\d+), (\d+), (true|false)\);", _source())]
    assert len(insts) == 6 and sorted(insts) == sorted(R.TAIL_INSTS)
    assert R.TAIL_WGS == (0, 1, 3, 7) and R.TAIL_N == 5 and R.TAIL_VALID == 3
    for mid, (h, w) in R.TAIL_MAP.items():
        assert R.chains_form(R.TAIL_N, h, w, mid)[1] == R.TAIL_BANDS[mid]            # the band count the default chains hand the tail
        assert (h * w) & (h * w - 1) == 0                                             # 1 / (H W) is a power of two


# ---------------------------------------------------------------- Part B: the bounds hold for a float32 evaluation on the CPU
def test_partb_bounds_hold_for_numpy_float32():
    assert R.ACT_B == 4.0
    v = R.act_grid()
    assert len(v) == 257 and float(v.min()) == -16 and float(v.max()) == 16
    for silu in (True, False):
        ref = R.silu64(v) if silu else torch.sigmoid(v)
        bound = R.act_bound(ref)
        assert float(bound.min()) >= R.FLT_MIN and float(((R.act_f32(v, silu) - ref).abs() / bound).max()) <= 1.0
        assert float((bound / ref.abs().clamp_min(1e-30))[ref != 0].max()) <= 2.0 ** -21      # the bound itself: at most 4 ulp = 2^-21 relative
    boxes = R.dfl_logits(2)
    st = []
    clss = [torch.zeros(2, 5, h, w, dtype=torch.float64) for h, w in R.DECODE_LEVELS]
    ref = R.v8_decode_ref(boxes, clss, R.DECODE_STRIDES, 5, stages=st)[:, :4]
    bound = R.decode_box_bound(st[0], R.DECODE_STRIDES)
    err = (R.decode_boxes_f32(boxes, R.DECODE_STRIDES) - ref).abs()
    assert float((err / bound).max()) <= 1.0
    assert float(bound.max()) < 5e-3                                      # thousandths of a pixel on boxes of hundreds of pixels: no licence
    assert float(R.ulp32(torch.tensor([1.0, 1.5, 2.0, 0.0], dtype=torch.float64))[0]) == 2.0 ** -23 and float(R.ulp32(torch.tensor([2.0], dtype=torch.float64))) == 2.0 ** -22


# ---------------------------------------------------------------- mutants of the reference
def _hidden(mut, ref):
    h = R.hidden_from_loose(mut, ref)
    assert bool(h.any()), f"the mutant differs in {int((mut != ref).sum())} elements, none of them within {R.LOOSE} x max"
    return int(h.sum()), int((mut != ref).sum())


def test_mutant_one_tap_dropped_at_a_border_column():
    c = R.CONV_CASES[6]                                                   # 3x3, 17 x 23, 48 -> 64
    for s in (0, 3):
        ops = R.exact_conv(c, s)
        ref = R.conv_ref(ops["x"], ops["w"], ops["bias"], c["st"])
        w_tap = torch.zeros_like(ops["w"]); w_tap[:, :, 1, 0] = ops["w"][:, :, 1, 0]
        mut = ref.clone()
        mut[..., -1] -= torch.nn.functional.conv2d(ops["x"], w_tap, None, 1, 1)[..., -1]       # the left neighbour of the last column, not added
        _hidden(mut, ref)


def test_mutant_one_16_channel_chunk_dropped_at_one_tap():
    for c in (R.CONV_CASES[6], R.CONV_CASES[14], R.CONV_CASES[3]):
        ops = R.exact_conv(c, 3)
        ref = R.conv_ref(ops["x"], ops["w"], ops["bias"], c["st"])
        w2 = ops["w"].clone(); w2[:, -16:, -1, -1] = 0                    # the last chunk of the last tap: the end of the K walk
        _hidden(R.conv_ref(ops["x"], w2, ops["bias"], c["st"]), ref)


@pytest.mark.parametrize("inst", R.TAIL_INSTS, ids=lambda i: "tail-%d-%d-%d-%d-%d" % i)
def test_mutant_the_previous_images_gates(inst):
    """Image i's gates used for image i + 1: what a wave's stale gate table does when a workgroup walks on to its next image."""
    ops, o, o2 = R.exact_tail(inst, R.TAIL_N, 3)
    stale = ops["gates"].clone(); stale[:, 1:] = ops["gates"][:, :-1]
    mo, mo2 = R.tail_ref(ops["ys"], stale, ops["w3"], ops["b3"], ops["xin"], ops["down"], ops["w4"], ops["b4"], inst[4])
    assert torch.equal(mo[0], o[0]) and not torch.equal(mo[1], o[1])
    _hidden(mo, o)
    assert not torch.equal(mo2, o2)


def test_mutant_the_second_image_of_a_row_stream_pair_skipped():
    """The skipped image keeps what the buffer held.  With outputs that start as a sentinel the mutant differs in every element of the
    image; with a buffer that still holds an earlier launch's result for the same batch (torch.empty in a loop over the forms hands back
    the block just freed) it EQUALS the reference - no tolerance is involved, which is why the GPU test fills every output first.  (Not
    shown: a difference below 5e-6 x max.  The chain outputs and their band sums share one exact range, which leaves no room for an
    element 2e5 times louder than the quantum.)"""
    n, (h, w, c) = 4, (16, 8, 32)
    _, ys, psum = R.exact_chains(n, h, w, c, 3, 1)
    for prev, equal in ((-7777.25, False), (None, True)):
        for y in ys + [psum.permute(1, 0, 2, 3)]:
            mut = y.clone()
            mut[1::2] = y[1::2] if prev is None else prev
            assert torch.equal(mut, y) == equal


def test_mutant_zero_padding_in_the_sppf_pools():
    for n, c, h, w in R.SPPF_CASES:
        x = R.negative_map(n, c, h, w)
        ref, mut = R.sppf_ref(x), R.sppf_ref(x, 0.0)
        assert float(ref.max()) < 0 and float(mut.max()) == 0.0
        _hidden(mut, ref)


def test_mutants_of_the_decode_anchor_offset_and_level_boundary():
    boxes, clss, ext = R.exact_decode(2, 5, 5, 0)
    ref = R.v8_decode_ref(boxes, clss, R.DECODE_STRIDES, 5, ext, 5, 0)
    assert float(ref.abs().max()) == 2.0 ** 21
    no_offset = R.v8_decode_ref(boxes, clss, R.DECODE_STRIDES, 5, ext, 5, 0, offset=0.0)
    assert torch.equal(no_offset[:, 2:], ref[:, 2:]) and bool((no_offset[:, :2] != ref[:, :2]).all())      # centres only, every anchor
    _hidden(no_offset, ref)
    for shift in (1, -1):
        moved = R.v8_decode_ref(boxes, clss, R.DECODE_STRIDES, 5, ext, 5, 0, shift=shift)
        cols = ((moved != ref).any(1).any(0)).nonzero().flatten().tolist()
        assert cols and set(cols) <= ({156, 198} if shift == 1 else {155, 197}), cols
        _hidden(moved, ref)
    a = R.anchor_levels(R.DECODE_LEVELS)
    assert a[155] == (0, 155) and a[156] == (1, 0) and a[197] == (1, 41) and a[198] == (2, 0) and a[209] == (2, 11) and len(a) == 210
