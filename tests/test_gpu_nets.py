"""Fused NHWC-half glue operators (csrc/ss_ops.hip) vs the plain torch modules they replace."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _fp32_on_cpu(m, x):
    """The same module in float32 on the CPU, on the same half weights and input: no kernel of this project runs there."""
    import copy
    from strongsort_yolo_amd import fused
    ref = copy.deepcopy(m).float().cpu()
    fused.ENABLED = False
    try:
        with torch.no_grad():
            out = ref(x.float().cpu())
    finally:
        fused.ENABLED = True
    return out


def _by_row_group(name, m, fused_out, plain_out, ref32):
    """Box rows, class rows and ext rows of pred [B, 4 + nc + n_ext, A] (the embedding for OSNet) each on their own scale: the error of
    the fused path against the float32 reference at most twice the error of the library's half path against the same reference, in the
    maximum and in the root mean square.  The yardstick is the library path, never the fused path against itself; the factor 2 allows for
    rounding points that sit in different places (measured ratios: docs/F16_OPERATORS.md section 11)."""
    from strongsort_yolo_amd import nets
    det = [mod for mod in m.modules() if isinstance(mod, nets.Detect)]
    groups = {"embedding": slice(None)} if not det else {"box": slice(0, 4), "class": slice(4, 4 + det[0].nc)}
    if det and fused_out.shape[1] > 4 + det[0].nc:
        groups["ext"] = slice(4 + det[0].nc, None)
    for g, rows in groups.items():
        r = ref32.double()[:, rows]
        ef, ep = (fused_out.double().cpu()[:, rows] - r).abs(), (plain_out.double().cpu()[:, rows] - r).abs()
        mx, rms = (float(ef.max()), float(ep.max())), (float(ef.pow(2).mean().sqrt()), float(ep.pow(2).mean().sqrt()))
        print(f"F16NET {name} {g}: max fused {mx[0]:.3e} plain {mx[1]:.3e} ratio {mx[0] / mx[1]:.3f}; rms fused {rms[0]:.3e} plain {rms[1]:.3e} "
              f"ratio {rms[0] / rms[1]:.3f}; max |ref| {float(r.abs().max()):.3e}")
        assert mx[0] <= 2 * mx[1], (name, g, "max", mx)
        assert rms[0] <= 2 * rms[1], (name, g, "rms", rms)


@pytest.mark.parametrize("name,shape", [("yolov8n", (1, 3, 384, 640)), ("osnet", (8, 3, 256, 128)), ("yolov8n-pose", (2, 3, 128, 160)),
                                        ("yolov8s", (2, 3, 192, 320)), ("yolov5n", (2, 3, 128, 160)), ("yolov7", (1, 3, 192, 320)),
                                        ("yolo11n", (2, 3, 192, 320)), ("yolo11n-pose", (1, 3, 384, 640))])
def test_fused_ops_match_torch_modules(name, shape):
    from strongsort_yolo_amd import fused, nets
    dev = torch.device("cuda", 0)
    m = (nets.build_reid() if name == "osnet" else nets.build_detector(name)).to(dev, torch.float16).to(memory_format=torch.channels_last)
    x = torch.randn(*shape, device=dev, dtype=torch.float16).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        fused.ENABLED = True
        a = m(x).float()
        fused.ENABLED = False
        b = m(x).float()
        fused.ENABLED = True
    assert a.shape == b.shape and torch.isfinite(a).all()
    scale = b.abs().max().item() + 1e-6
    assert (a - b).abs().max().item() <= 2e-2 * scale, ((a - b).abs().max().item(), scale)
    _by_row_group(name, m, a, b, _fp32_on_cpu(m, x))


@pytest.mark.parametrize("name,shape", [("yolov8n-seg", (2, 3, 192, 320)), ("yolo11n-seg", (1, 3, 128, 160))])
def test_segmentation_head_fused_matches_torch_modules(name, shape):
    """Segment head (yolo_multi_model.py:14 names 'yolov8n-seg.pt'): rows [B, 4+nc+32, A] with the raw mask coefficients last,
    prototypes [B, 32, H/4, W/4]; the fused convolutions under it against the plain torch modules."""
    from strongsort_yolo_amd import fused, nets
    dev = torch.device("cuda", 0)
    m = nets.build_detector(name).to(dev, torch.float16).to(memory_format=torch.channels_last)
    x = torch.randn(*shape, device=dev, dtype=torch.float16).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        fused.ENABLED = True
        a = m(x)
        fused.ENABLED = False
        b = m(x)
        fused.ENABLED = True
    B, _, H, W = shape
    A = sum((H // s) * (W // s) for s in (8, 16, 32))
    assert a[0].shape == b[0].shape == (B, 4 + 80 + 32, A) and a[1].shape == b[1].shape == (B, 32, H // 4, W // 4)
    for u, v in zip(a, b):
        u, v = u.float(), v.float()
        scale = v.abs().max().item() + 1e-6
        assert torch.isfinite(u).all() and (u - v).abs().max().item() <= 2e-2 * scale, ((u - v).abs().max().item(), scale)
    ref = _fp32_on_cpu(m, x)
    _by_row_group(name, m, a[0].float(), b[0].float(), ref[0])
    _by_row_group(name + " prototypes", torch.nn.Identity(), a[1].float(), b[1].float(), ref[1])


@pytest.mark.parametrize("shape", [(3, 16, 64, 32), (2, 24, 32, 16), (5, 32, 16, 8), (1, 16, 20, 24), (2, 32, 7, 8)])
def test_lightconv_matches_pointwise_plus_depthwise(shape):
    """Fused LightConv3x3 (MFMA pointwise -> LDS -> depthwise+bias+ReLU) vs the two-step form: the pointwise
    product rounded to half (as the GEMM writes it), then the depthwise in fp32.  Covers bands whose halo rows
    fall outside the image (H not a multiple of the 16-row band, H < band)."""
    import torch.nn.functional as F
    from strongsort_yolo_amd import fused
    n, c, h, w = shape
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(c * 100 + h)
    x = torch.randn(n, c, h, w, generator=g).to(dev, torch.float16).contiguous(memory_format=torch.channels_last)
    w1 = (torch.randn(c, c, generator=g) / c ** 0.5).to(dev, torch.float16)
    wd = (torch.randn(c, 9, generator=g) / 3).to(dev, torch.float16)
    b = torch.randn(c, generator=g).to(dev, torch.float16)
    assert fused.lightconv_ok(x)
    got = fused.lightconv(x, w1, wd.t().contiguous(), b).float()
    mid = F.conv2d(x.float(), w1.float().view(c, c, 1, 1)).half().float()
    ref = F.relu(F.conv2d(mid, wd.float().view(c, 1, 3, 3), b.float(), padding=1, groups=c))
    ref = ref.half().float()
    err = (got - ref).abs().max().item()
    # one half-ulp flip of an intermediate can move an output by ~|w| * ulp(mid); outputs themselves are half
    assert err <= 2e-2 * (ref.abs().max().item() + 1e-6), err
    assert (got != ref).float().mean().item() < 0.02       # and nearly every element is bit-identical


def test_bias_act_place_matches_torch():
    """Placement epilogue of the C2f blocks: slice of a wider NHWC buffer + dense mirror + post-activation shortcut."""
    import torch.nn.functional as F
    from strongsort_yolo_amd import fused
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(7)
    B, C, H, W, CT = 3, 32, 9, 13, 96
    mk = lambda *s: torch.randn(*s, generator=g).to(dev, torch.float16)
    y = mk(B, C, H, W).contiguous(memory_format=torch.channels_last)
    res = mk(B, C, H, W).contiguous(memory_format=torch.channels_last)
    bias = mk(C)
    cat = torch.full((B, CT, H, W), 5.0, dtype=torch.float16, device=dev).contiguous(memory_format=torch.channels_last)
    out2 = torch.empty((B, 16, H, W), dtype=torch.float16, device=dev).contiguous(memory_format=torch.channels_last)
    fused.bias_act_place(y, bias, "silu", cat, 40, res=res, res_after=True, out2=out2, c0=16)
    ref = (F.silu(y.float() + bias.float().view(1, C, 1, 1)).half().float() + res.float()).half()
    assert torch.equal(cat[:, 40:72], ref) or (cat[:, 40:72].float() - ref.float()).abs().max().item() <= 2e-3
    assert torch.equal(out2, cat[:, 56:72])
    assert (cat[:, :40] == 5.0).all() and (cat[:, 72:] == 5.0).all()      # neighbours of the slice untouched
    cat2 = torch.zeros_like(cat)
    fused.bias_act_place(y, bias, "silu", cat2, 0)
    ref2 = F.silu(y.float() + bias.float().view(1, C, 1, 1)).half()
    assert (cat2[:, :C].float() - ref2.float()).abs().max().item() <= 2e-3 and (cat2[:, C:] == 0).all()


def test_v8_decode_matches_float_reference():
    from strongsort_yolo_amd import fused
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(3)
    B, nc, sizes, strides = 3, 80, [(12, 20), (6, 10), (3, 5)], (8, 16, 32)
    mk = lambda *s: torch.randn(*s, generator=g).to(dev, torch.float16)
    boxes = [(2 * mk(B, 64, h, w)).contiguous(memory_format=torch.channels_last) for h, w in sizes]
    clss = [(2 * mk(B, nc, h, w)).contiguous(memory_format=torch.channels_last) for h, w in sizes]
    bb, cb = [mk(64) for _ in sizes], [mk(nc) for _ in sizes]
    got = fused.v8_decode(boxes, clss, bb, cb, strides, nc)
    A = sum(h * w for h, w in sizes)
    assert got.shape == (B, 4 + nc, A) and got.dtype == torch.float32
    box = torch.cat([(t.float() + b.float().view(1, -1, 1, 1)).reshape(B, 64, -1) for t, b in zip(boxes, bb)], 2)
    cls = torch.cat([(t.float() + b.float().view(1, -1, 1, 1)).reshape(B, nc, -1) for t, b in zip(clss, cb)], 2)
    pts, st = [], []
    for (h, w), s in zip(sizes, strides):
        yy, xx = torch.meshgrid(torch.arange(h, device=dev) + 0.5, torch.arange(w, device=dev) + 0.5, indexing="ij")
        pts.append(torch.stack((xx, yy), 0).view(2, -1)); st.append(torch.full((1, h * w), float(s), device=dev))
    anchors, st = torch.cat(pts, 1).unsqueeze(0), torch.cat(st, 1).unsqueeze(0)
    d = (box.view(B, 4, 16, A).softmax(2) * torch.arange(16, device=dev, dtype=torch.float32).view(1, 1, 16, 1)).sum(2)
    x1y1, x2y2 = anchors - d[:, :2], anchors + d[:, 2:]
    ref = torch.cat((torch.cat(((x1y1 + x2y2) / 2, x2y2 - x1y1), 1) * st, cls.sigmoid()), 1)
    assert (got - ref).abs().max().item() <= 1e-3 * 32 * 16         # __expf-level error on coordinates up to stride*16
    assert (got[:, 4:] - ref[:, 4:]).abs().max().item() <= 1e-5


@pytest.mark.parametrize("B,dim,H,W", [(3, 128, 12, 20), (2, 256, 6, 10), (1, 128, 16, 16), (2, 128, 3, 5), (32, 128, 12, 20)])
def test_psa_attention_launch_matches_the_module(B, dim, H, W):
    """nets.Attention (v11 C2PSA: heads of key_dim 32 / head_dim 64 over the H*W positions, depthwise positional term on v) through
    the one-launch kernel against the module's torch path in fp32 on the same half weights and input."""
    from strongsort_yolo_amd import fused, nets
    dev = torch.device("cuda", 0)
    torch.manual_seed(dim + H)
    att = nets.Attention(dim, num_heads=dim // 64, attn_ratio=0.5).to(dev, torch.float16)
    x = (torch.randn(B, dim, H, W) * 0.7).to(dev, torch.float16).contiguous(memory_format=torch.channels_last)
    assert fused.psa_ok(x, att.num_heads, att.key_dim, att.head_dim)
    with torch.no_grad():
        got = att(x).float()
        old = fused.ENABLED
        fused.ENABLED = False
        try:
            ref = att.float()(x.float())
        finally:
            fused.ENABLED = old
            att.half()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    assert err <= 1e-2 * (scale + 1.0), (err, scale)


@pytest.mark.parametrize("nc,cls_ld,n_ext,ext_ld,mode", [(1, 8, 51, 56, 1), (80, 80, 32, 32, 0), (1, 8, 0, 0, 0), (3, 8, 6, 8, 1)])
def test_v8_decode_extra_rows_match_float_reference(nc, cls_ld, n_ext, ext_ld, mode):
    """The decode launch with a third branch (ss_op_v8_decode_ext_f16): keypoint triplets as Ultralytics Pose.kpts_decode — x, y =
    (2 v + cell index) * stride, visibility = sigmoid(v) — or raw mask coefficients in rows 4 + nc .. of the prediction, class
    tensors padded past nc channels (a one-class head padded to 8 rows); rows 0 .. 4 + nc equal the plain decode."""
    from strongsort_yolo_amd import fused
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(nc + n_ext)
    B, sizes, strides = 2, [(12, 20), (6, 10), (3, 5)], (8, 16, 32)
    mk = lambda *s: torch.randn(*s, generator=g).to(dev, torch.float16)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    boxes = [cl(2 * mk(B, 64, h, w)) for h, w in sizes]
    clss = [cl(2 * mk(B, cls_ld, h, w)) for h, w in sizes]
    ext = [cl(mk(B, ext_ld, h, w)) for h, w in sizes] if n_ext else None
    z = torch.zeros(max(64, cls_ld), dtype=torch.float16, device=dev)
    got = fused.v8_decode(boxes, clss, [z] * 3, [z] * 3, strides, nc, ext, n_ext, mode)
    A = sum(h * w for h, w in sizes)
    assert got.shape == (B, 4 + nc + n_ext, A) and got.dtype == torch.float32
    base = fused.v8_decode(boxes, [cl(t[:, :nc].contiguous()) for t in clss] if nc % 8 == 0 else clss, [z] * 3, [z] * 3, strides, nc)
    assert torch.equal(got[:, :4 + nc], base[:, :4 + nc])
    cls = torch.cat([t[:, :nc].float().reshape(B, nc, -1) for t in clss], 2)
    assert (got[:, 4:4 + nc] - cls.sigmoid()).abs().max().item() <= 1e-5
    if n_ext:
        e = torch.cat([t[:, :n_ext].float().reshape(B, n_ext, -1) for t in ext], 2)              # [B, n_ext, A]
        if mode == 0:
            assert torch.equal(got[:, 4 + nc:], e)
        else:
            col = torch.cat([torch.arange(w, device=dev, dtype=torch.float32).repeat(h) for h, w in sizes])
            row = torch.cat([torch.arange(h, device=dev, dtype=torch.float32).repeat_interleave(w) for h, w in sizes])
            st = torch.cat([torch.full((h * w,), float(s), device=dev) for (h, w), s in zip(sizes, strides)])
            k = e.view(B, n_ext // 3, 3, A)
            ref = torch.stack(((k[:, :, 0] * 2.0 + col) * st, (k[:, :, 1] * 2.0 + row) * st, k[:, :, 2].sigmoid()), 2).view(B, n_ext, A)
            assert (got[:, 4 + nc:] - ref).abs().max().item() <= 1e-4 * (ref.abs().max().item() + 1.0)
            assert torch.equal(got[:, 4 + nc::3][:, :n_ext // 3], ref[:, 0::3]) and torch.equal(got[:, 5 + nc::3][:, :n_ext // 3], ref[:, 1::3])   # the affine rows: exact


@pytest.mark.parametrize("M_hw,K,N,act", [((8, 48, 80), 64, 32, "silu"), ((2, 12, 20), 384, 128, "silu"), ((64, 64, 32), 16, 64, "relu"),
                                          ((3, 7, 9), 24, 96, "none"), ((5, 16, 8), 128, 128, "relu"), ((1, 5, 5), 512, 256, "silu"),
                                          ((40, 64, 32), 16, 16, "relu"), ((2, 3, 5), 8, 8, "sigmoid"),
                                          ((8, 48, 80), 64, 80, "none"), ((2, 12, 20), 80, 80, "silu"), ((3, 24, 40), 128, 80, "silu")])
def test_pointwise_matches_conv_bias_act(M_hw, K, N, act):
    """MFMA 1x1 conv kernel vs conv2d (fp32 accumulate, rounded to half as the library conv writes it) + bias + act,
    with and without the shortcut (before / after the activation), over every tile configuration and ragged M."""
    import torch.nn.functional as F
    from strongsort_yolo_amd import fused
    B, H, W = M_hw
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(K * 1000 + N)
    mk = lambda *s: torch.randn(*s, generator=g).to(dev, torch.float16)
    x = mk(B, K, H, W).contiguous(memory_format=torch.channels_last)
    w = (mk(N, K).float() / K ** 0.5).half()
    bias, res = mk(N), mk(B, N, H, W).contiguous(memory_format=torch.channels_last)
    f = {"silu": F.silu, "relu": F.relu, "none": lambda t: t, "sigmoid": torch.sigmoid}[act]
    conv = F.conv2d(x.float(), w.float().view(N, K, 1, 1)).half().float() + bias.float().view(1, N, 1, 1)
    tol = lambda ref: 4e-3 * (ref.abs().max().item() + 1.0)
    got = fused.pointwise(x, w, bias, act)
    assert got.shape == (B, N, H, W) and got.is_contiguous(memory_format=torch.channels_last)
    assert (got.float() - f(conv)).abs().max().item() <= tol(f(conv))
    got = fused.pointwise(x, w, bias, act, res=res)
    assert (got.float() - f(conv + res.float())).abs().max().item() <= tol(f(conv + res.float()))
    got = fused.pointwise(x, w, bias, act, res=res, res_after=True)
    assert (got.float() - (f(conv).half().float() + res.float())).abs().max().item() <= tol(f(conv) + res.float())
    if N % 16 == 0:                                          # placement into a wider buffer + dense mirror of the upper half
        cat = torch.full((B, N + 24, H, W), 3.0, dtype=torch.float16, device=dev).contiguous(memory_format=torch.channels_last)
        out2 = torch.empty((B, N // 2, H, W), dtype=torch.float16, device=dev).contiguous(memory_format=torch.channels_last)
        fused.pointwise(x, w, bias, act, out=cat, c_off=8, out2=out2, c0=N // 2)
        assert torch.equal(cat[:, 8:8 + N], fused.pointwise(x, w, bias, act))
        assert torch.equal(out2, cat[:, 8 + N // 2:8 + N]) and (cat[:, :8] == 3.0).all() and (cat[:, 8 + N:] == 3.0).all()


@pytest.mark.parametrize("shape", [(3, 16, 64, 32), (2, 24, 32, 16), (4, 32, 16, 8), (2, 16, 40, 24), (1, 32, 5, 8), (5, 16, 37, 32), (3, 32, 19, 16),
                                   (2, 16, 7, 16), (1, 24, 64, 16),
                                   # >= 96 images: the register-stream form (bands chosen from the image count)
                                   (96, 16, 64, 32), (130, 16, 37, 32), (200, 24, 32, 16), (97, 32, 19, 16), (100, 16, 7, 16), (512, 16, 64, 32),
                                   # 8-wide maps in the register-stream form: two images per 16-lane tile (odd counts: the last wave has one)
                                   (97, 32, 16, 8), (200, 32, 16, 8), (131, 16, 11, 8), (96, 24, 5, 8), (1024, 32, 16, 8)])
def test_osnet_streams_equal_layerwise_chains(shape):
    """Chain-fused kernel (intermediates in LDS, shrinking halo) vs the same ten layers run one launch each: outputs
    bit-identical (same arithmetic per layer), band sums equal the float sum of the outputs; then the gate built on
    those sums vs the two-pass gate."""
    from strongsort_yolo_amd import fused
    n, c, h, w = shape
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(c * 7 + h)
    x = torch.randn(n, c, h, w, generator=g).to(dev, torch.float16).contiguous(memory_format=torch.channels_last)
    w1 = (torch.randn(10, c, c, generator=g) / c ** 0.5).to(dev, torch.float16)
    w9 = (torch.randn(10, 9, c, generator=g) / 3).to(dev, torch.float16)
    b = (torch.randn(10, c, generator=g) / 2).to(dev, torch.float16)
    assert fused.streams_ok(x)
    ys, psum = fused.osnet_streams(x, w1, w9, b)
    L, ref = 0, []
    for t in range(1, 5):
        cur = x
        for _ in range(t):
            cur = fused.lightconv(cur, w1[L], w9[L], b[L]); L += 1
        ref.append(cur)
    for t in range(4):
        assert torch.equal(ys[t], ref[t]), t
        tot = ref[t].float().sum((2, 3))                                     # [n, c]
        assert (psum[t].sum(1) - tot).abs().max().item() <= 1e-3 * (tot.abs().max().item() + 1.0)
    cr = max(c // 16, 1)
    gw = [(torch.randn(cr, c, generator=g) / c ** 0.5).to(dev, torch.float16), torch.randn(cr, generator=g).to(dev, torch.float16),
          torch.randn(c, cr, generator=g).to(dev, torch.float16), torch.randn(c, generator=g).to(dev, torch.float16)]
    a, r = fused.gate_apply(ys, psum, *gw), fused.gate_sum(ref, *gw)
    assert (a.float() - r.float()).abs().max().item() <= 2e-3 * (r.float().abs().max().item() + 1.0)


@pytest.mark.parametrize("n,mid,c2,n2,h,w,pool,want", [(3, 16, 64, 16, 64, 32, False, True), (2, 16, 64, 64, 64, 32, True, False),
                                                       (3, 24, 96, 24, 32, 16, False, True), (2, 24, 96, 96, 32, 16, True, False),
                                                       (5, 32, 128, 32, 16, 8, False, True), (4, 32, 128, 128, 16, 8, False, False),
                                                       (2, 16, 64, 64, 64, 32, False, True), (1, 24, 96, 96, 16, 16, True, True)])
def test_osnet_tail_equals_separate_kernels(n, mid, c2, n2, h, w, pool, want):
    """gate + conv3 + shortcut + ReLU + following 1x1 ConvBR (+ 2x2 average) in one launch == gate_apply, pointwise, pointwise,
    avgpool2 run one after the other, bit for bit."""
    from strongsort_yolo_amd import fused
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(mid * 131 + n2 + h)
    rnd = lambda *sh, s=1.0: (torch.randn(*sh, generator=g) * s).to(dev, torch.float16)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    ys = [cl(rnd(n, mid, h, w).relu_()) for _ in range(4)]
    bands = (h + 15) // 16                                  # any partition of the rows will do: the tail only adds the parts up
    psum = torch.stack([torch.stack([y[:, :, bnd * 16:(bnd + 1) * 16].float().sum((2, 3)) for bnd in range(bands)], 1) for y in ys]).contiguous()
    cr = max(mid // 16, 1)
    gw = (rnd(cr, mid, s=mid ** -0.5), rnd(cr), rnd(mid, cr), rnd(mid))
    w3, b3, idn = rnd(c2, mid, s=mid ** -0.5), rnd(c2, s=0.5), cl(rnd(n, c2, h, w))
    w4, b4 = rnd(n2, c2, s=c2 ** -0.5), rnd(n2, s=0.5)
    assert fused.tail_ok(mid, c2, n2, h, w, pool)
    out, o2 = fused.osnet_tail(ys, psum, gw, w3, b3, idn, want, w4, b4, pool)
    x2 = fused.gate_apply(ys, psum, *gw)
    r1 = fused.pointwise(x2, w3, b3, "relu", res=idn)
    r2 = fused.pointwise(r1, w4, b4, "relu")
    if pool:
        r2 = fused.avgpool2(r2)
    assert (out is None) == (not want)
    if want:
        assert torch.equal(out, r1)
    assert o2.shape == r2.shape and torch.equal(o2, r2)
    assert r2.float().abs().max().item() > 0.1                           # not a comparison of zeros


@pytest.mark.parametrize("n,c1,mid,c2,h,w", [(3, 16, 16, 64, 64, 32), (2, 64, 24, 96, 32, 16), (5, 96, 32, 128, 16, 8)])
def test_osnet_tail_with_down_shortcut_equals_separate_kernels(n, c1, mid, c2, h, w):
    """First block of a stage: the tail computes the shortcut down(x) itself == pointwise(down) + gate_apply + pointwise + pointwise."""
    from strongsort_yolo_amd import fused
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(c1 * 7 + h)
    rnd = lambda *sh, s=1.0: (torch.randn(*sh, generator=g) * s).to(dev, torch.float16)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    ys = [cl(rnd(n, mid, h, w).relu_()) for _ in range(4)]
    psum = torch.stack([y.float().sum((2, 3)).unsqueeze(1) for y in ys]).contiguous()          # one part per image
    cr = max(mid // 16, 1)
    gw = (rnd(cr, mid, s=mid ** -0.5), rnd(cr), rnd(mid, cr), rnd(mid))
    x = cl(rnd(n, c1, h, w))
    wd, bd = rnd(c2, c1, s=c1 ** -0.5), rnd(c2, s=0.5)
    w3, b3 = rnd(c2, mid, s=mid ** -0.5), rnd(c2, s=0.5)
    w4, b4 = rnd(mid, c2, s=c2 ** -0.5), rnd(mid, s=0.5)
    assert fused.tail_ok(mid, c2, mid, h, w, False) and fused.tail_down_ok(c1, mid, c2, mid)
    out, o2 = fused.osnet_tail(ys, psum, gw, w3, b3, x, True, w4, b4, False, down=(wd, bd))
    idn = fused.pointwise(x, wd, bd, "none")
    r1 = fused.pointwise(fused.gate_apply(ys, psum, *gw), w3, b3, "relu", res=idn)
    r2 = fused.pointwise(r1, w4, b4, "relu")
    assert torch.equal(out, r1) and torch.equal(o2, r2)
    assert r2.float().abs().max().item() > 0.1


@pytest.mark.parametrize("name,B", [("yolov8n", 16), ("yolov8n", 1), ("yolov8s", 2)])
def test_detect_head_grouped_launches_equal_separate_launches(name, B):
    """The detect head's six branches as three grouped launches (one per depth) vs 18 separate launches: same kernels' bodies,
    identical predictions."""
    from strongsort_yolo_amd import fused, nets
    dev = torch.device("cuda", 0)
    m = nets.build_detector(name).to(dev).half().to(memory_format=torch.channels_last)
    x = torch.randn(B, 3, 384, 640, generator=torch.Generator().manual_seed(5)).to(dev, torch.float16).contiguous(memory_format=torch.channels_last)
    old = fused.set_flags(HEAD=False)                               # (k_head would take the head before the grouped form is asked)
    try:
        with torch.no_grad():
            fused.set_flags(GROUP=False)
            ref = m(x)
            fused.set_flags(GROUP=True)
            got = m(x)
    finally:
        fused.set_flags(GROUP=True, **old)
    assert got.shape == ref.shape and torch.equal(got, ref)
    assert ref[:, 4:].float().max().item() > 0.0


def test_osnet_with_fused_tails_equals_blockwise_path():
    """The whole OSNet: block tails fused with the following 1x1 convolution vs one launch per operator — identical embeddings,
    for every place a frame pipeline may cut the backbone."""
    from strongsort_yolo_amd import fused, nets
    dev = torch.device("cuda", 0)
    m = nets.build_reid().to(dev).half()
    x = torch.randn(6, 3, 256, 128, generator=torch.Generator().manual_seed(3)).to(dev, torch.float16).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        ref_flag, fused.TAIL = fused.TAIL, False
        try:
            ref = m(x)
        finally:
            fused.TAIL = ref_flag
        assert fused.TAIL
        for split in range(0, m.N_PARTS + 1):
            st = m.forward_a(x, split)
            assert isinstance(st, tuple) == (split in (1, 2, 3, 5, 6, 8, 9)), split       # 1: (stem output, first block's conv1)
            assert torch.equal(m.forward_b(st, split), ref), split


@pytest.mark.parametrize("shape,N,stride,act", [((2, 16, 48, 80), 16, 1, "silu"), ((8, 16, 96, 160), 32, 2, "silu"), ((2, 64, 24, 40), 64, 1, "silu"),
                                                ((3, 128, 12, 20), 128, 1, "relu"), ((1, 32, 7, 9), 64, 2, "none"), ((2, 64, 13, 11), 256, 2, "silu"),
                                                ((1, 8, 5, 5), 8, 1, "sigmoid"), ((4, 24, 17, 16), 40, 1, "silu"),
                                                # 80-channel tiles (class branch): 64- and 128-pixel workgroups, split-K
                                                ((6, 64, 24, 40), 80, 1, "silu"), ((2, 64, 24, 40), 80, 1, "silu"), ((9, 80, 48, 80), 80, 1, "silu"),
                                                # detector-sized layers on the same implicit-GEMM kernel (k_pw<., ., true, .>; there is no separate tiled form):
                                                # 128-pixel workgroups from 32768 pixels up, 64-pixel ones below, every channel tile but <128, 2>, 16-channel
                                                # inputs (two taps per 32-wide MFMA block), stride 2, several K chunks, ragged tiles
                                                ((32, 16, 96, 160), 16, 1, "silu"), ((32, 32, 96, 160), 64, 2, "silu"), ((32, 64, 48, 80), 64, 1, "silu"),
                                                ((32, 64, 48, 80), 80, 1, "silu"), ((16, 128, 24, 40), 128, 1, "relu"), ((16, 128, 24, 40), 64, 1, "silu"),
                                                ((5, 32, 37, 53), 48, 1, "none"), ((5, 32, 37, 53), 48, 2, "silu"), ((20, 256, 12, 20), 64, 1, "silu"),
                                                ((32, 64, 48, 80), 128, 2, "silu"), ((32, 32, 96, 160), 32, 1, "silu"), ((12, 128, 24, 40), 256, 2, "silu"),
                                                ((32, 80, 48, 80), 80, 1, "silu"), ((8, 48, 30, 44), 32, 2, "relu")])
def test_conv3x3_matches_conv2d_bias_act(shape, N, stride, act):
    """Implicit-GEMM 3x3 kernel vs conv2d (pad 1) + bias + act, shortcut before/after, placement; odd sizes and stride 2."""
    import torch.nn.functional as F
    from strongsort_yolo_amd import fused
    B, K, H, W = shape
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(K * 100 + N + stride)
    mk = lambda *s: torch.randn(*s, generator=g).to(dev, torch.float16)
    x = mk(B, K, H, W).contiguous(memory_format=torch.channels_last)
    w = (mk(N, K, 3, 3).float() / (9 * K) ** 0.5).half()
    w9 = w.permute(0, 2, 3, 1).reshape(N, -1).contiguous()
    bias = mk(N)
    f = {"silu": F.silu, "relu": F.relu, "none": lambda t: t, "sigmoid": torch.sigmoid}[act]
    conv = F.conv2d(x.float(), w.float(), None, stride, 1).half().float() + bias.float().view(1, N, 1, 1)
    OH, OW = conv.shape[2:]
    res = mk(B, N, OH, OW).contiguous(memory_format=torch.channels_last)
    tol = lambda ref: 4e-3 * (ref.abs().max().item() + 1.0)
    got = fused.conv3x3(x, w9, bias, stride, act)
    assert got.shape == (B, N, OH, OW) and got.is_contiguous(memory_format=torch.channels_last)
    assert (got.float() - f(conv)).abs().max().item() <= tol(f(conv))
    got = fused.conv3x3(x, w9, bias, stride, act, res=res, res_after=True)
    assert (got.float() - (f(conv).half().float() + res.float())).abs().max().item() <= tol(f(conv) + res.float())
    if N % 16 == 0:
        cat = torch.full((B, N + 16, OH, OW), 3.0, dtype=torch.float16, device=dev).contiguous(memory_format=torch.channels_last)
        out2 = torch.empty((B, N, OH, OW), dtype=torch.float16, device=dev).contiguous(memory_format=torch.channels_last)
        fused.conv3x3(x, w9, bias, stride, act, out=cat, c_off=16, out2=out2, c0=0)
        assert torch.equal(cat[:, 16:], fused.conv3x3(x, w9, bias, stride, act)) and torch.equal(out2, cat[:, 16:])
        assert (cat[:, :16] == 3.0).all()


@pytest.mark.parametrize("B,C,H,W,add", [(32, 16, 96, 160, True), (32, 32, 48, 80, True), (32, 64, 24, 40, True), (3, 32, 48, 80, False),
                                          (2, 64, 13, 21, True), (1, 16, 7, 5, False), (5, 16, 37, 53, True), (32, 64, 24, 40, False),
                                          (32, 128, 12, 20, True), (3, 128, 9, 11, False),
                                          # the 8 x 16 tile (B * H * W / 128 >= 512, C <= 64) hanging over both edges
                                          (1, 16, 250, 263, True), (1, 64, 251, 262, False)])
def test_bottleneck_launch_is_bit_identical_to_its_two_convolutions(B, C, H, W, add):
    """k_bneck (3x3 + SiLU -> LDS -> 3x3 + SiLU + shortcut, placed into a concat slice) == the two ss_op_conv3x3_f16 launches,
    every bit; tiles that hang over the right / bottom edge (of either tile size), images smaller than a tile, both tile sizes."""
    from strongsort_yolo_amd import fused, nets
    dev = torch.device("cuda", 0)
    torch.manual_seed(C * 1000 + H)
    m = nets.Bottleneck(C, C, shortcut=add, e=1.0).to(dev, torch.float16)
    assert fused.bottleneck_ok(m) and m.add == add
    x = torch.randn(B, C, H, W).to(dev, torch.float16).contiguous(memory_format=torch.channels_last)
    a, b = m.cv1.conv, m.cv2.conv
    fused.set_option("pw_splitk", 0)                                 # (the split-K form of small 64-channel layers sums in another order)
    try:
        t = fused.conv3x3(x, fused.weight_n9k(m.cv1, a), a.bias, 1, "silu")
        ref = fused.conv3x3(t, fused.weight_n9k(m.cv2, b), b.bias, 1, "silu", res=x if add else None, res_after=True)
    finally:
        fused.set_option("pw_splitk", 1)
    cat = torch.full((B, 3 * C, H, W), 3.0, dtype=torch.float16, device=dev).contiguous(memory_format=torch.channels_last)
    out2 = torch.empty_like(x)
    fused.bottleneck(x, m, cat, 2 * C, out2=out2)
    assert torch.equal(cat[:, 2 * C:], ref) and torch.equal(out2, ref) and (cat[:, :2 * C] == 3.0).all()
    fused.bottleneck(x, m, cat, C)                                   # no dense copy, another slice
    assert torch.equal(cat[:, C:2 * C], ref) and (cat[:, :C] == 3.0).all()


@pytest.mark.parametrize("B,cin,H,W,nc,tile16", [(32, 64, 48, 80, 80, False), (32, 128, 24, 40, 80, False), (32, 256, 12, 20, 80, False),
                                                  (3, 64, 48, 80, 80, True), (2, 64, 13, 21, 16, False), (2, 64, 13, 21, 16, True),
                                                  (1, 128, 7, 5, 80, False), (5, 256, 9, 11, 8, False)])
def test_head_level_launch_is_bit_identical_to_its_six_layers(B, cin, H, W, nc, tile16):
    """k_head (per branch 3x3 + SiLU -> LDS -> 3x3 + SiLU -> per-wave LDS tile -> 1x1 + bias; both branches of a level in one launch)
    == ss_op_conv3x3_f16 x 2 + ss_op_pointwise_f16 per branch, every bit (the non-split-K form of the small layers: the split-K form
    adds the K chunks in another order); tiles hanging over the edges, maps smaller than a tile, both tile sizes, class counts < 80;
    and close to the fp32 convolutions."""
    import torch.nn.functional as F
    from strongsort_yolo_amd import fused, nets
    dev = torch.device("cuda", 0)
    torch.manual_seed(cin * 100 + H)
    det = nets.Detect(80, (64, 128, 256))
    lvl = {64: 0, 128: 1, 256: 2}[cin]
    if nc != 80:                                                     # fewer output channels than mid channels in both branches
        det.cv3[lvl][2] = torch.nn.Conv2d(80, nc, 1)
        det.cv2[lvl][2] = torch.nn.Conv2d(64, 8 + nc, 1)
    det = det.to(dev, torch.float16)
    box, cls = det.cv2[lvl], det.cv3[lvl]
    x = torch.randn(B, cin, H, W).to(dev, torch.float16).contiguous(memory_format=torch.channels_last)
    old_flags = fused.set_flags(HEAD=True)
    assert fused.head_level_ok(x, box, cls)
    fused.set_flags(**old_flags)
    fused.set_option("pw_splitk", 0)
    try:
        refs = []
        for seq in (box, cls):
            t = fused.conv3x3(x, fused.weight_n9k(seq[0], seq[0].conv), seq[0].conv.bias, 1, "silu")
            t = fused.conv3x3(t, fused.weight_n9k(seq[1], seq[1].conv), seq[1].conv.bias, 1, "silu")
            refs.append(fused.pointwise(t, fused.weight_nk(seq[2], seq[2]), seq[2].bias))
    finally:
        fused.set_option("pw_splitk", 1)
    got = fused.head_level(x, box, cls, tile16=tile16)
    for g, r, seq in zip(got, refs, (box, cls)):
        assert g.shape == r.shape and torch.equal(g, r), f"{int((g != r).sum())} of {g.numel()} values differ"
        f32 = seq.float()(x.float())
        assert (g.float() - f32).abs().max().item() <= 2e-2 * (f32.abs().max().item() + 1.0)
        seq.half()


def test_detector_with_head_level_launches_equals_grouped_launches():
    """yolov8n at the benchmark batch: the whole detector with k_head == with the grouped head launches (at 32 frames no level takes the
    split-K form), bit for bit."""
    from strongsort_yolo_amd import fused, nets
    dev = torch.device("cuda", 0)
    m = nets.build_detector("yolov8n").to(dev).half().to(memory_format=torch.channels_last)
    x = torch.randn(32, 3, 384, 640, generator=torch.Generator().manual_seed(7)).to(dev, torch.float16).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        old = fused.set_flags(HEAD=False)
        try:
            ref = m(x)
            fused.set_flags(HEAD=True)
            got = m(x)
        finally:
            fused.set_flags(**old)
    assert got.shape == ref.shape and torch.equal(got, ref) and ref[:, 4:].float().max().item() > 0.0


@pytest.mark.parametrize("N,H", [(3, 256), (2, 64), (1, 16)])
def test_osnet_stem_matches_conv_relu_pool(N, H):
    import torch.nn.functional as F
    from strongsort_yolo_amd import fused, nets
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(H)
    x = torch.randn(N, 3, H, 128, generator=g).to(dev, torch.float16).contiguous(memory_format=torch.channels_last)
    conv = torch.nn.Conv2d(3, 16, 7, 2, 3).to(dev, torch.float16)
    assert fused.stem_ok(x, conv)
    holder = torch.nn.Module()
    got = fused.osnet_stem(x, fused.stem_weight(holder, conv), conv.bias)
    c = F.conv2d(x.float(), conv.weight.float(), None, 2, 3).half().float() + conv.bias.float().view(1, 16, 1, 1)
    ref = F.max_pool2d(F.relu(c).half().float(), 3, 2, 1)
    assert got.shape == ref.shape == (N, 16, H // 4, 32)
    assert (got.float() - ref).abs().max().item() <= 4e-3 * (ref.abs().max().item() + 1.0)
    assert (got.float() != ref).float().mean().item() < 0.02
    # the first OSBlock's conv1 from the same launch == the pointwise kernel on the stem output, bit for bit
    w1 = (torch.randn(16, 16, generator=g) / 4).to(dev, torch.float16)
    b1 = torch.randn(16, generator=g).to(dev, torch.float16)
    y, y1 = fused.osnet_stem(x, fused.stem_weight(holder, conv), conv.bias, (w1, b1))
    assert torch.equal(y, got) and torch.equal(y1, fused.pointwise(got, w1, b1, "relu"))


@pytest.mark.parametrize("b,c1,c2,h,w,lo_first", [(16, 256, 128, 12, 20, True), (3, 128, 64, 24, 40, True), (2, 8, 24, 5, 7, False), (1, 64, 64, 1, 1, False)])
def test_upcat_equals_interpolate_plus_cat(b, c1, c2, h, w, lo_first):
    import torch.nn.functional as F
    from strongsort_yolo_amd import fused
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(c1 + h)
    lo = torch.randn(b, c1, h, w, generator=g).to(dev, torch.float16).contiguous(memory_format=torch.channels_last)
    hi = torch.randn(b, c2, 2 * h, 2 * w, generator=g).to(dev, torch.float16).contiguous(memory_format=torch.channels_last)
    assert fused.upcat_ok(lo, hi)
    up = F.interpolate(lo, scale_factor=2.0, mode="nearest")
    ref = torch.cat((up, hi) if lo_first else (hi, up), 1)
    got = fused.upcat(lo, hi, lo_first)
    assert got.is_contiguous(memory_format=torch.channels_last) and torch.equal(got, ref)


@pytest.mark.parametrize("b,c,h,w", [(16, 128, 12, 20), (2, 256, 20, 20), (1, 8, 3, 2), (3, 64, 32, 32), (2, 16, 1, 9)])
def test_sppf_pools_equal_the_pool_cascade(b, c, h, w):
    import torch.nn.functional as F
    from strongsort_yolo_amd import fused
    dev = torch.device("cuda", 0)
    x = torch.randn(b, c, h, w, generator=torch.Generator().manual_seed(c + w)).to(dev, torch.float16).contiguous(memory_format=torch.channels_last)
    assert fused.sppf_pools_ok(x)
    y = [x]
    for _ in range(3):
        y.append(F.max_pool2d(y[-1], 5, 1, 2))
    assert torch.equal(fused.sppf_pools(x), torch.cat(y, 1))


@pytest.mark.parametrize("B,H,W,co", [(16, 384, 640, 16), (2, 384, 640, 32), (1, 30, 128, 48), (3, 17, 256, 16)])
def test_conv0_matches_conv_bias_silu(B, H, W, co):
    import torch.nn.functional as F
    from strongsort_yolo_amd import fused
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(co + H)
    x = torch.randn(B, 3, H, W, generator=g).to(dev, torch.float16).contiguous(memory_format=torch.channels_last)
    conv = torch.nn.Conv2d(3, co, 3, 2, 1).to(dev, torch.float16)
    assert fused.conv0_ok(x, conv)
    got = fused.conv0(x, fused.conv0_weight(torch.nn.Module(), conv), conv.bias, "silu")
    ref = F.silu(F.conv2d(x.float(), conv.weight.float(), None, 2, 1).half().float() + conv.bias.float().view(1, co, 1, 1))
    assert got.shape == ref.shape
    assert (got.float() - ref).abs().max().item() <= 4e-3 * (ref.abs().max().item() + 1.0)
    assert (got.float() - ref).abs().mean().item() <= 2e-4


def test_avgpool2_equals_torch():
    import torch.nn.functional as F
    from strongsort_yolo_amd import fused
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(1)
    for shape in [(3, 64, 64, 32), (2, 96, 32, 16), (1, 8, 2, 2)]:
        x = torch.randn(*shape, generator=g).to(dev, torch.float16).contiguous(memory_format=torch.channels_last)
        got, ref = fused.avgpool2(x), F.avg_pool2d(x, 2, 2)
        assert got.shape == ref.shape and got.is_contiguous(memory_format=torch.channels_last)
        assert (got.float() - ref.float()).abs().max().item() <= 1e-3 * (ref.float().abs().max().item() + 1e-6)


def test_valid_image_counts_belong_to_their_stream():
    """ss_op_set_valid_images is per (thread, stream): two pipelines in one process with different packed-batch counts do not
    see each other's setting (ADVICE r2 / VERDICT r2 item 9), and a stream without a setting computes every image."""
    from strongsort_yolo_amd import fused
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(5)
    B, K, N, H, W = 8, 16, 16, 4, 8
    x = torch.randn(B, K, H, W, generator=g).to(dev, torch.float16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(N, K, generator=g) / 4).to(dev, torch.float16)
    bias = torch.randn(N, generator=g).to(dev, torch.float16)
    ref = fused.pointwise(x, w, bias, "relu")
    na, nb = torch.tensor([2], dtype=torch.int32, device=dev), torch.tensor([5], dtype=torch.int32, device=dev)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    mk = lambda: torch.full((B, N, H, W), 7.0, dtype=torch.float16, device=dev).contiguous(memory_format=torch.channels_last)
    oa, ob, oc = mk(), mk(), mk()
    torch.cuda.synchronize()
    with torch.cuda.stream(sa):
        ctx_a = fused.valid_images(na, B); ctx_a.__enter__()
    with torch.cuda.stream(sb):
        ctx_b = fused.valid_images(nb, B); ctx_b.__enter__()
    with torch.cuda.stream(sa):
        fused.pointwise(x, w, bias, "relu", out=oa)
    with torch.cuda.stream(sb):
        fused.pointwise(x, w, bias, "relu", out=ob)
    fused.pointwise(x, w, bias, "relu", out=oc)                 # the default stream holds no setting
    with torch.cuda.stream(sb):
        ctx_b.__exit__(None, None, None)
    with torch.cuda.stream(sa):
        fused.pointwise(x, w, bias, "relu", out=ob[:0] if False else mk())          # stream a still limited after b's exit
        ctx_a.__exit__(None, None, None)
    torch.cuda.synchronize()
    assert torch.equal(oa[:2], ref[:2]) and (oa[2:] == 7.0).all()
    assert torch.equal(ob[:5], ref[:5]) and (ob[5:] == 7.0).all()
    assert torch.equal(oc, ref)
    with torch.cuda.stream(sa):
        od = mk(); fused.pointwise(x, w, bias, "relu", out=od)
    torch.cuda.synchronize()
    assert torch.equal(od, ref)


@pytest.mark.parametrize("N,H,W,F", [(13, 16, 8, 512), (1, 16, 8, 512), (1024, 16, 8, 512), (9, 4, 4, 64)])
def test_osnet_head_launch_matches_mean_fc_relu(N, H, W, F):
    """relu(fc(mean_hw(x))) in one launch against torch on the same half tensors (means rounded to half, fp32 accumulation)."""
    from strongsort_yolo_amd import fused
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(N + F)
    x = torch.randn(N, 128, H, W, generator=g).to(dev, torch.float16).contiguous(memory_format=torch.channels_last)
    fc = torch.nn.Linear(128, F).to(dev, torch.float16)
    assert fused.osnet_head_ok(x, fc)
    got = fused.osnet_head(x, fc).float()
    m = x.float().mean((2, 3)).half().float()
    ref = torch.relu((m @ fc.weight.float().t()).half().float() + fc.bias.float()).half().float()
    assert got.shape == ref.shape == (N, F)
    assert (got - ref).abs().max().item() <= 2e-3 * (ref.abs().max().item() + 1.0)
    assert (got != ref).float().mean().item() < 0.05
