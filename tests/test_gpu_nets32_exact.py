"""The fp32 operator kernels (csrc/ss_ops32.hip) against their float64 restatement on the CPU (tests/f32_ref.py, docs/F32_OPERATORS.md).

Part A: operands on which every product and partial sum is exact in fp32 - the kernel's output must EQUAL the fp64 reference cast to
float, for every launch form the launchers can choose (tests/test_f32_ref_cpu.py shows the case lists reach them) and every option that
changes a form.  Every output starts as a sentinel: what a launch must not write (images past a valid count, the neighbours of a channel
slice) keeps it, and a valid-count run is bit-equal to the full run on the images it covers.  The entry points are called through the C
ABI directly, so the outputs (and the tail's gate workspace) are the test's own tensors.
Part B: SiLU and sigmoid on a grid of exact pre-activations and the DFL expectation on dyadic logits, held per element to bounds derived
from the instruction sequence (f32_ref.act_bound, f32_ref.decode_box_bound); each case prints its worst err / bound
(profiles/f32_exact_ratios.txt)."""
import contextlib
import ctypes as C

import pytest
import torch

from tests import f32_ref as R

pytestmark = pytest.mark.gpu

SENT = -7777.25                                       # no reference holds it: the references are small dyadic numbers or 2^k
DEFAULTS = dict(conv_mt=0, conv_min=0, conv_waves=0, conv_wgs=1024, tail_wgs=0, stem_walk=0, chains_form=2, chains_pre=-1, chains_min_n=128)


def _dev():
    return torch.device("cuda", 0)


def _lib():
    from strongsort_yolo_amd import lib
    return lib.load()


def _g(t):
    """fp64 CPU tensor -> dense fp32 on the device (the values are fp32 numbers: the cast is exact)."""
    assert bool((t.float().double() == t).all())
    return t.to(_dev(), torch.float32).contiguous()


def _nhwc(t):
    return _g(t.permute(0, 2, 3, 1))


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off) if t is not None else C.c_void_p(0)


def _st():
    return C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _sent(*shape):
    return torch.full(shape, SENT, dtype=torch.float32, device=_dev())


def _nv(k):
    return torch.tensor([k], dtype=torch.int32, device=_dev())


def _ok(rc, what):
    assert rc == 0, f"{what}: the launcher returned {rc}"


@contextlib.contextmanager
def _options(**kw):
    L = _lib()
    try:
        for k, v in kw.items():
            _ok(L.ss_op32_set_option(k.encode(), int(v)), f"set_option {k}={v}")
        yield
    finally:
        for k in kw:
            L.ss_op32_set_option(k.encode(), DEFAULTS[k])


def _same(got, ref, what):
    """Equality (torch.equal: -0 == 0, which a ReLU output needs; a NaN is unequal to everything)."""
    ref = ref.to(got.device, torch.float32)                               # the fp64 reference cast to float
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if not torch.equal(got, ref):
        bad = got != ref
        first = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} values differ, first at {first}: {float(got[tuple(first)])} != "
                             f"{float(ref[tuple(first)])}, max |d| = {float((got.double() - ref.double()).abs().max())}")


def _untouched(t, what):
    assert bool((t == SENT).all()), f"{what}: {int((t != SENT).sum())} values written that the launch must leave alone"


# ================================================================ Part A: k32_conv
def _plan(c):
    mt, wv, gx, gy = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _ok(_lib().ss_op32_conv_plan(c["n"], c["h"], c["w"], c["ci"], c["co"], c["ks"], c["st"], C.byref(mt), C.byref(wv), C.byref(gx), C.byref(gy)), "plan")
    return mt.value, wv.value, gx.value, gy.value


def _conv(c, x, xs, w, bias, res, rs, out, os_, act=0):
    return _lib().ss_op32_conv(_st(), x, xs, _p(w), _p(bias), res, rs, out, os_, c["n"], c["h"], c["w"], c["ci"], c["co"], c["ks"], c["st"], act)


@pytest.mark.parametrize("case", R.CONV_CASES, ids=R.conv_id)
def test_conv_equals_the_fp64_reference_on_exact_operands_under_every_option(case):
    """Dense operands under every option state of f32_ref.conv_settings (default, conv_waves 4 / 8, every conv_mt the channel count divides
    by, a conv_min that reduces MT, conv_wgs = 1), with and without the shortcut; then input, output and shortcut as channel slices of wider
    tensors, whose other channels keep their values.  The plan of every launch is read from ss_op32_conv_plan and checked against the
    option that forces it."""
    c = case
    oh, ow, M, _ = R.conv_dims(c)
    n, ci, co = c["n"], c["ci"], c["co"]
    for s in (0, 3):
        ops = R.exact_conv(c, s)
        refs = {False: _nhwc(R.conv_ref(ops["x"], ops["w"], ops["bias"], c["st"])),
                True: _nhwc(R.conv_ref(ops["x"], ops["w"], ops["bias"], c["st"], res=ops["res"]))}
        x, w, bias, res = _nhwc(ops["x"]), _g(ops["w"].permute(0, 2, 3, 1)), _g(ops["bias"]), _nhwc(ops["res"])
        for opt in R.conv_settings(c):
            with _options(**opt):
                mt, wv, gx, gy = _plan(c)
                tag = f"{R.conv_id(c)} s={s} {opt} plan mt={mt} waves={wv} grid={gx}x{gy}"
                assert mt in (1, 2, 4, 5) and wv in (4, 8) and co % (16 * mt) == 0 and gx == ((M + 15) // 16 + wv - 1) // wv and gy == co // (16 * mt), tag
                assert opt.get("conv_waves", wv) == wv and opt.get("conv_mt", mt) == mt, tag
                if "conv_min" in opt:
                    assert mt == 1, tag                               # 2^20 workgroups are never there: reduced all the way
                if "conv_wgs" in opt:
                    assert wv == (8 if (M + 15) // 16 >= 8 else 4), tag
                for use_res in (False, True):
                    out = _sent(n, oh, ow, co)
                    _ok(_conv(c, _p(x), ci, w, bias, _p(res if use_res else None), co if use_res else 0, _p(out), co), tag)
                    _same(out, refs[use_res], f"{tag} res={use_res}")
        # channel slices: x at channel 4 of ci + 8, out at 4 of co + 8, the shortcut at 8 of co + 12
        xw = torch.full((n, c["h"], c["w"], ci + 8), 9.0, dtype=torch.float32, device=_dev())
        xw[..., 4:4 + ci] = x
        rw = torch.full((n, oh, ow, co + 12), 9.0, dtype=torch.float32, device=_dev())
        rw[..., 8:8 + co] = res
        for opt in (dict(), dict(conv_waves=8), dict(conv_mt=1, conv_waves=4)):
            with _options(**opt):
                for use_res in (False, True):
                    wide = _sent(n, oh, ow, co + 8)
                    tag = f"{R.conv_id(c)} s={s} {opt} slices res={use_res} plan={_plan(c)}"
                    _ok(_conv(c, _p(xw, 4), ci + 8, w, bias, _p(rw, 8) if use_res else _p(None), co + 12 if use_res else 0, _p(wide, 4), co + 8), tag)
                    _same(wide[..., 4:4 + co], refs[use_res], tag)
                    _untouched(wide[..., :4], tag); _untouched(wide[..., 4 + co:], tag)
        assert bool((xw[..., :4] == 9.0).all()) and bool((xw[..., 4 + ci:] == 9.0).all()) and bool((rw[..., :8] == 9.0).all())


@pytest.mark.parametrize("n,h,w", R.CONV0_CASES)
def test_conv0_equals_the_fp64_reference_on_exact_operands(n, h, w):
    for s in (0, 3):
        ops, ref = R.exact_conv0(n, h, w, s)
        oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        x, wt, bias = _nhwc(ops["x"]), _g(ops["w"].permute(0, 2, 3, 1)), _g(ops["bias"])
        out = _sent(n, oh, ow, 16)
        _ok(_lib().ss_op32_conv0(_st(), _p(x), _p(wt), _p(bias), _p(out), 16, n, h, w, 0), "conv0")
        _same(out, _nhwc(ref), f"conv0 {(n, h, w)} s={s}")
        wide = _sent(n, oh, ow, 24)
        _ok(_lib().ss_op32_conv0(_st(), _p(x), _p(wt), _p(bias), _p(wide, 4), 24, n, h, w, 0), "conv0 slice")
        _same(wide[..., 4:20], _nhwc(ref), f"conv0 slice {(n, h, w)} s={s}")
        _untouched(wide[..., :4], "conv0 slice"); _untouched(wide[..., 20:], "conv0 slice")


# ================================================================ Part A: k32_pw
def _pw(x, w, bias, res, out, M, K, N, relu, nv=None, img_px=0):
    return _lib().ss_op32_pointwise(_st(), _p(x), _p(w), _p(bias), _p(res), _p(out), M, K, N, int(relu), _p(nv), img_px)


@pytest.mark.parametrize("K,N", R.PW_PAIRS)
def test_pointwise_equals_the_fp64_reference_on_exact_operands(K, N):
    """All twelve instantiations at M = 105, 16 and 64, ReLU and shortcut on and off; at M = 105 = 3 images of 35 pixels with a valid count
    of 2, which cuts M at 70 - inside the fifth tile: rows from 70 on keep the sentinel, the rest is the full run bit for bit."""
    for s in (0, 3):
        for M in R.PW_MS:
            ops = R.exact_pw(K, N, M, s)
            x, w, bias, res = _g(ops["x"]), _g(ops["w"]), _g(ops["bias"]), _g(ops["res"])
            for relu in (True, False):
                for use_res in (False, True):
                    tag = f"pw {K}->{N} M={M} s={s} relu={relu} res={use_res}"
                    ref = R.pw_ref(ops["x"], ops["w"], ops["bias"], ops["res"] if use_res else None, relu)
                    out = _sent(M, N)
                    _ok(_pw(x, w, bias, res if use_res else None, out, M, K, N, relu), tag)
                    _same(out, ref, tag)
                    if M == 105:
                        part = _sent(M, N)
                        _ok(_pw(x, w, bias, res if use_res else None, part, M, K, N, relu, _nv(R.PW_VALID), R.PW_IMG_PX), tag)
                        cut = R.PW_VALID * R.PW_IMG_PX
                        assert torch.equal(part[:cut], out[:cut]), tag + " valid count"
                        _untouched(part[cut:], tag + " valid count")


def test_pointwise_with_two_tiles_per_wave_equals_the_fp64_reference():
    """257 images of 64 x 32: 32 896 tiles, more than 4 x 8 192 -> tpw = 2 (f32_ref.pw_tpw restates the rule); then a valid count of 129
    images of 2 047 pixels, which cuts M inside a tile: every row past the cut keeps the sentinel."""
    c = R.PW_TPW2
    K, N, px = c["K"], c["N"], c["h"] * c["w"]
    M = c["images"] * px
    assert R.pw_tpw(M)[0] == 2
    ops = R.exact_pw(K, N, M, 3)
    x, w, bias, res = _g(ops["x"]), _g(ops["w"]), _g(ops["bias"]), _g(ops["res"])
    ref = _g(R.pw_ref(ops["x"], ops["w"], ops["bias"], ops["res"], True))
    out = _sent(M, N)
    _ok(_pw(x, w, bias, res, out, M, K, N, True), "pw tpw=2")
    _same(out, ref, "pw tpw=2")
    out.fill_(SENT)
    nv = 129
    _ok(_pw(x, w, bias, res, out, M, K, N, True, _nv(nv), px - 1), "pw tpw=2 valid")      # img_px = 2047: M is cut at 264 063, inside a tile
    cut = nv * (px - 1)
    _same(out[:cut], ref[:cut], "pw tpw=2 valid")
    _untouched(out[cut:], "pw tpw=2 valid")


# ================================================================ Part A: the stem
def test_stem_equals_the_fp64_reference_at_every_walk():
    """k32_stem (stem_walk -1) and k32_stemW<false> at 1, 2, 4, 8 and 16 bands per workgroup, alone and with the first block's conv1 in
    the launch, full and with a valid count of 2 of 3 crops."""
    L = _lib()
    n, nv = R.STEM_N, R.STEM_VALID
    for s in (0, 3):
        ops, y, y1 = R.exact_stem(n, s)
        x, bias, w1, b1 = _nhwc(ops["x"]), _g(ops["bias"]), _g(ops["w1"]), _g(ops["b1"])
        wk = torch.zeros(16, 148, dtype=torch.float32, device=_dev())
        wk[:, :147] = _g(ops["w"].permute(0, 2, 3, 1).reshape(16, 147))
        ry, ry1 = _nhwc(y), _nhwc(y1)
        for walk in R.STEM_WALKS:
            with _options(stem_walk=walk):
                for valid in (None, nv):
                    tag = f"stem s={s} walk={walk} valid={valid}"
                    k = n if valid is None else valid
                    cnt = None if valid is None else _nv(valid)
                    out = _sent(n, 64, 32, 16)
                    _ok(L.ss_op32_stem(_st(), _p(x), _p(wk), _p(bias), _p(out), n, 256, 128, _p(cnt)), tag)
                    _same(out[:k], ry[:k], tag)
                    _untouched(out[k:], tag)
                    out, out1 = _sent(n, 64, 32, 16), _sent(n, 64, 32, 16)
                    _ok(L.ss_op32_stem_conv1(_st(), _p(x), 0, _p(wk), _p(bias), _p(out), _p(w1), _p(b1), _p(out1), n, 256, 128, _p(cnt)), tag)
                    _same(out[:k], ry[:k], tag + " +conv1: y")
                    _same(out1[:k], ry1[:k], tag + " +conv1: y1")
                    _untouched(out[k:], tag); _untouched(out1[k:], tag)


# ================================================================ Part A: the chains
def _chains(ops_g, n, h, w, c, nv=None):
    L = _lib()
    bands = L.ss_op32_chains_bands(n, h, w, c)
    assert bands >= 1
    ys = [_sent(n, h, w, c) for _ in range(4)]
    psum = _sent(4, n, bands, c)
    arr = (C.c_void_p * 4)(*[y.data_ptr() for y in ys])
    x1, w1, w9, b = ops_g
    _ok(L.ss_op32_chains(_st(), _p(x1), _p(w1), _p(w9), _p(b), arr, _p(psum), n, h, w, c, _p(nv)), "chains")
    return ys, psum, bands


@pytest.mark.parametrize("h,w,c", R.CHAIN_MAPS)
def test_chains_equal_the_fp64_reference_in_every_form(h, w, c):
    """k32_chainsR (chains_form 2 with chains_min_n 1), k32_chains3 (form 1, chains_pre -1 / 0 / 1) and k32_chains (form 0) on the three
    maps, at 1, 2, 3 and 5 images, ys and psum both; then valid counts that end inside a row-stream workgroup's pair / quad of images:
    the images past the count keep the sentinel in ys and psum, the others are the full run bit for bit."""
    for s in (0, 3):
        built = {}
        for n in sorted(set(R.CHAIN_NS) | {nn for nn, _ in R.CHAIN_VALID[(h, w, c)]}):
            for form, min_n, pre in R.chain_settings(h, w, c):
                with _options(chains_form=form, chains_min_n=min_n, chains_pre=pre):
                    want, bands = R.chains_form(n, h, w, c, form, min_n, pre)
                    if (n, bands) not in built:
                        ops, rys, rps = R.exact_chains(n, h, w, c, s, bands)
                        built[n, bands] = ((_nhwc(ops["x1"]), _g(ops["w1"]), _g(ops["w9"].reshape(10, c, 9).permute(0, 2, 1)), _g(ops["b"])),
                                           [_nhwc(y) for y in rys], _g(rps))
                    ops_g, rys, rps = built[n, bands]
                    tag = f"chains {h}x{w}x{c} n={n} s={s} form={form} min_n={min_n} pre={pre} -> {want}"
                    ys, psum, got_bands = _chains(ops_g, n, h, w, c)
                    assert got_bands == bands, tag
                    for t in range(4):
                        _same(ys[t], rys[t], f"{tag} y{t + 1}")
                    _same(psum, rps, tag + " psum")
                    for nn, nv in R.CHAIN_VALID[(h, w, c)]:
                        if nn != n:
                            continue
                        pys, pps, _ = _chains(ops_g, n, h, w, c, _nv(nv))
                        for t in range(4):
                            assert torch.equal(pys[t][:nv], ys[t][:nv]), f"{tag} valid {nv}: y{t + 1}"
                            _untouched(pys[t][nv:], f"{tag} valid {nv}: y{t + 1}")
                        assert torch.equal(pps[:, :nv], psum[:, :nv]), f"{tag} valid {nv}: psum"
                        _untouched(pps[:, nv:], f"{tag} valid {nv}: psum")


# ================================================================ Part A: gates and tail
@pytest.mark.parametrize("inst", R.TAIL_INSTS, ids=lambda i: "tail-%d-%d-%d-%d-%d" % i)
def test_gates_and_tail_equal_the_fp64_reference_when_a_workgroup_walks_several_images(inst):
    """Every k32_tail instantiation on synthetic exact chain outputs and channel sums (independent of the chain kernels), five images, the
    persistent grid at its default size and at 1, 3 and 7 workgroups - with 1 and 3 a workgroup walks several images and changes image in
    the middle of its share, refilling its waves' gate tables - then the same with a valid count of 3.  The gate workspace is the test's
    own tensor, so k32_gates is compared by itself too: gates exactly 0, 0.5 and 1 that differ between images, chains and channels."""
    L = _lib()
    mid, c2, c1, n2, pool = inst
    h, w = R.TAIL_MAP[mid]
    n, nv = R.TAIL_N, R.TAIL_VALID
    for s in (0, 3):
        ops, o, o2 = R.exact_tail(inst, n, s)
        assert R.gates_are_diverse(ops["gates"]) and R.gates_are_diverse(ops["gates"][:, :nv])
        ys = [_nhwc(y) for y in ops["ys"]]
        arr = (C.c_void_p * 4)(*[y.data_ptr() for y in ys])
        psum = _g(ops["psum"])
        gw = [_g(ops[k]) for k in ("gw1", "gb1", "gw2", "gb2")]
        w3, b3, xin, w4, b4 = _g(ops["w3"]), _g(ops["b3"]), _nhwc(ops["xin"]), _g(ops["w4"]), _g(ops["b4"])
        wd, bd = (_g(ops["down"][0]), _g(ops["down"][1])) if c1 else (None, None)
        ro, ro2, rg = _nhwc(o), _nhwc(o2), _g(ops["gates"])
        oh, ow = (h // 2, w // 2) if pool else (h, w)
        for wgs in R.TAIL_WGS:
            with _options(tail_wgs=wgs):
                for valid in (None, nv):
                    for want_out in (True, False):
                        tag = f"tail {inst} s={s} tail_wgs={wgs} valid={valid} out={want_out}"
                        k = n if valid is None else valid
                        out, out2, gates = _sent(n, h, w, c2), _sent(n, oh, ow, n2), _sent(4, n, mid)
                        _ok(L.ss_op32_tail(_st(), arr, _p(psum), psum.shape[2], _p(gw[0]), _p(gw[1]), _p(gw[2]), _p(gw[3]), ops["hidden"], _p(gates),
                                           _p(w3), _p(b3), _p(xin), c1, _p(wd), _p(bd), _p(out if want_out else None), _p(w4), _p(b4), _p(out2), int(pool),
                                           n, h, w, mid, c2, n2, _p(None if valid is None else _nv(valid))), tag)
                        _same(gates[:, :k], rg[:, :k], tag + " gates")
                        _untouched(gates[:, k:], tag + " gates")
                        _same(out2[:k], ro2[:k], tag + " out2")
                        _untouched(out2[k:], tag + " out2")
                        if want_out:
                            _same(out[:k], ro[:k], tag + " out")
                            _untouched(out[k:], tag + " out")
                        else:
                            _untouched(out, tag + " out (not asked for)")


# ================================================================ Part A: the head
@pytest.mark.parametrize("n,f,valid", R.HEAD_CASES)
def test_head_equals_the_fp64_reference_on_exact_operands(n, f, valid):
    for s in (0, 3):
        ops, ref = R.exact_head(n, f, s)
        x, w, bias = _nhwc(ops["x"]), _g(ops["w"]), _g(ops["bias"])
        out = _sent(n, f)
        k = n if valid is None else valid
        _ok(_lib().ss_op32_head(_st(), _p(x), _p(w), _p(bias), _p(out), n, 128, 128, f, _p(None if valid is None else _nv(valid))), "head")
        _same(out[:k], ref[:k], f"head {(n, f, valid)} s={s}")
        _untouched(out[k:], f"head {(n, f, valid)} s={s}")
        assert float(ref.max()) > 0


# ================================================================ Part A: upcat, SPPF
@pytest.mark.parametrize("n,cl,ch,h,w", R.UPCAT_CASES)
def test_upcat_equals_cat_of_interpolate(n, cl, ch, h, w):
    g = torch.Generator().manual_seed(cl * 10 + h)
    lo, hi = torch.randn(n, cl, h, w, generator=g).double(), torch.randn(n, ch, 2 * h, 2 * w, generator=g).double()
    lod, hid = _nhwc(lo), _nhwc(hi)
    low = torch.full((n, h, w, cl + 8), 9.0, dtype=torch.float32, device=_dev()); low[..., 4:4 + cl] = lod
    hiw = torch.full((n, 2 * h, 2 * w, ch + 12), 9.0, dtype=torch.float32, device=_dev()); hiw[..., 8:8 + ch] = hid
    for lo_first in (1, 0):
        ref = _nhwc(R.upcat_ref(lo, hi, bool(lo_first)))
        for sliced in (False, True):
            out = _sent(n, 2 * h, 2 * w, cl + ch)
            args = (_p(low, 4), cl + 8, cl, _p(hiw, 8), ch + 12, ch) if sliced else (_p(lod), cl, cl, _p(hid), ch, ch)
            _ok(_lib().ss_op32_upcat(_st(), *args, _p(out), n, 2 * h, 2 * w, lo_first), "upcat")
            _same(out, ref, f"upcat {(n, cl, ch, h, w)} lo_first={lo_first} sliced={sliced}")


@pytest.mark.parametrize("n,c,h,w", R.SPPF_CASES)
def test_sppf_equals_the_max_pool_cascade_on_an_all_negative_map(n, c, h, w):
    """All values negative: a pool that pads with zero instead of -inf returns 0 along the border."""
    x = R.negative_map(n, c, h, w)
    ref = _nhwc(R.sppf_ref(x))
    assert float(ref.max()) < 0
    xd = _nhwc(x)
    xw = torch.full((n, h, w, c + 8), 9.0, dtype=torch.float32, device=_dev()); xw[..., 4:4 + c] = xd
    for sliced in (False, True):
        out = _sent(n, h, w, 4 * c)
        _ok(_lib().ss_op32_sppf_pools(_st(), _p(xw, 4) if sliced else _p(xd), c + 8 if sliced else c, _p(out), n, h, w, c), "sppf")
        _same(out, ref, f"sppf {(n, c, h, w)} sliced={sliced}")


# ================================================================ the v8 decode
def _decode(boxes, clss, ext, nc, n_ext, ext_mode):
    B = boxes[0].shape[0]
    A = sum(h * w for h, w in R.DECODE_LEVELS)
    bx, cl = [_nhwc(t) for t in boxes], [_nhwc(t) for t in clss]
    ex = [_nhwc(t) for t in ext] if n_ext else None
    arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
    ints = lambda v: (C.c_int * 3)(*v)
    pred = _sent(B, 4 + nc + n_ext, A)
    _ok(_lib().ss_op32_v8_decode(_st(), arr(bx), arr(cl), arr(ex) if n_ext else None, n_ext, ex[0].shape[3] if n_ext else 0, ext_mode,
                                 ints([h for h, _ in R.DECODE_LEVELS]), ints([w for _, w in R.DECODE_LEVELS]), ints(R.DECODE_STRIDES), B, nc,
                                 cl[0].shape[3], _p(pred)), "v8_decode")
    return pred


@pytest.mark.parametrize("n_ext,ext_mode", [(0, 0), (5, 0), (6, 1)])
def test_v8_decode_equals_the_fp64_reference_on_one_hot_logits(n_ext, ext_mode):
    """B = 2, A = 210 (two blocks, level boundaries at anchors 156 and 198): boxes from one-hot DFL logits, class scores and keypoint
    confidences from logits whose sigmoid is exactly 0, 0.5 or 1, raw / dyadic ext rows: every row of pred equal."""
    nc = 5
    boxes, clss, ext = R.exact_decode(2, nc, n_ext, ext_mode)
    ref = R.v8_decode_ref(boxes, clss, R.DECODE_STRIDES, nc, ext, n_ext, ext_mode)
    assert bool((ref[:, :4].float().double() == ref[:, :4]).all()) and set(ref[:, 4:4 + nc].float().unique().tolist()) == {0.0, 0.5, 1.0}
    _same(_decode(boxes, clss, ext, nc, n_ext, ext_mode), ref, f"v8_decode n_ext={n_ext} mode={ext_mode}")


# ================================================================ Part B
def _ratio(got, ref, bound, what):
    r = ((got.double().cpu() - ref).abs() / bound)
    worst = float(r.max())
    print(f"PARTB {what}: worst err / bound = {worst:.4f} over {ref.numel()} elements")
    assert torch.isfinite(got).all() and worst <= 1.0, f"{what}: {int((r > 1).sum())} elements outside the bound, worst err / bound = {worst}"


def _grid_columns(count, channels):
    """[count + ..] grid values spread so that channel c of position p holds grid[(p + 16 c) % 257]."""
    v = R.act_grid()
    idx = (torch.arange(count).view(-1, 1) + 16 * torch.arange(channels).view(1, -1)) % len(v)
    return v[idx]                                                       # [count, channels]


def test_silu_of_conv_on_the_exact_grid_stays_within_four_ulps():
    """k32_conv with a one-hot weight per output channel and zero bias: the pre-activation IS the input value, a multiple of 1/8 in
    [-16, 16]; 1x1 and 3x3 (centre tap), both wave counts."""
    v = _grid_columns(257, 16)                                           # pixel p, channel c
    ref = R.silu64(v)
    x = _g(v.view(1, 1, 257, 16))
    for ks in (1, 3):
        w = torch.zeros(16, ks, ks, 16, dtype=torch.float64)
        w[torch.arange(16), ks // 2, ks // 2, torch.arange(16)] = 1.0
        c = dict(ks=ks, st=1, n=1, h=1, w=257, ci=16, co=16)
        for waves in (4, 8):
            with _options(conv_waves=waves):
                out = _sent(1, 1, 257, 16)
                _ok(_conv(c, _p(x), 16, _g(w), torch.zeros(16, device=_dev()), _p(None), 0, _p(out), 16, act=1), "conv silu")
                _ratio(out.view(257, 16), ref, R.act_bound(ref), f"silu k32_conv {ks}x{ks} waves={waves}")


def test_silu_of_conv0_on_the_exact_grid_stays_within_four_ulps():
    v = _grid_columns(257, 3)                                            # output pixel ox reads input pixel 2 ox
    xin = torch.zeros(1, 2, 514, 3, dtype=torch.float64)
    xin[0, 0, 0::2] = v
    w = torch.zeros(16, 3, 3, 3, dtype=torch.float64)
    w[torch.arange(16), 1, 1, torch.arange(16) % 3] = 1.0
    ref = R.silu64(v[:, torch.arange(16) % 3])
    out = _sent(1, 1, 257, 16)
    x, wt, bias = _g(xin), _g(w), torch.zeros(16, device=_dev())          # (named: a tensor passed as _p(_g(..)) is freed before the launch)
    _ok(_lib().ss_op32_conv0(_st(), _p(x), _p(wt), _p(bias), _p(out), 16, 1, 2, 514, 1), "conv0 silu")
    _ratio(out.view(257, 16), ref, R.act_bound(ref), "silu k32_conv0")


def test_decode_sigmoid_and_dfl_stay_within_their_derived_bounds():
    """Class rows and keypoint confidences: sigmoid of multiples of 1/8 in [-16, 16], 4 ulps.  Box rows: DFL logits k / 8 in [-4, 4], the
    bound of f32_ref.decode_box_bound per element; the keypoint x / y rows (dyadic) stay exact."""
    nc, n_ext, B = 5, 6, 2
    boxes = R.dfl_logits(B)
    v = R.act_grid()
    g = torch.Generator().manual_seed(5)
    clss = [v[torch.randint(0, len(v), (B, nc, h, w), generator=g)] for h, w in R.DECODE_LEVELS]
    ext = []
    for h, w in R.DECODE_LEVELS:
        e = torch.randint(-64, 65, (B, n_ext, h, w), generator=g).double() / 8
        e[:, 2::3] = v[torch.randint(0, len(v), e[:, 2::3].shape, generator=g)]
        ext.append(e)
    st = []
    ref = R.v8_decode_ref(boxes, clss, R.DECODE_STRIDES, nc, ext, n_ext, 1, stages=st)
    got = _decode(boxes, clss, ext, nc, n_ext, 1)
    _ratio(got[:, :4], ref[:, :4], R.decode_box_bound(st[0], R.DECODE_STRIDES), "decode DFL box rows")
    _ratio(got[:, 4:4 + nc], ref[:, 4:4 + nc], R.act_bound(ref[:, 4:4 + nc]), "decode class sigmoid")
    conf = [4 + nc + k for k in range(n_ext) if k % 3 == 2]
    xy = [4 + nc + k for k in range(n_ext) if k % 3 != 2]
    _ratio(got[:, conf], ref[:, conf], R.act_bound(ref[:, conf]), "decode keypoint confidence sigmoid")
    _same(got[:, xy], ref[:, xy], "decode keypoint x / y rows")
