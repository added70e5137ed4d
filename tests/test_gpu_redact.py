"""Redaction on the device (csrc/ss_redact.hip, docs/REDACT.md): whole buffers, row padding included, equal tests/redact_ref.py byte for
byte — every effect over every shape at the tile and frame borders, frames smaller than the radius, order, overlap and splitting,
a batch at the caps, a reused scratch, a captured call, and the way through Overlay.annotate_resident and the command line."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.overlay_np import rasterise
from strongsort_yolo_amd import cli, overlay, redact
from strongsort_yolo_amd.overlay_font import font_table
from tests import redact_ref as R
from tests.gpu_util import engine

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EFFECTS = [("blur", 1), ("blur", 2), ("blur", 7), ("blur", 31), ("pixelate", 4), ("pixelate", 8), ("pixelate", 32), ("fill", 0)]
FILL = (17, 200, 99)


@pytest.fixture(scope="module")
def eng():
    e = engine(debug=False)
    yield e
    e.close()


def _buffers(rng, B, H, W, pad_cols=5, pad_rows=0):
    """-> host buffer uint8 [B, H + pad_rows, 3 W + pad_cols]: the frames are its [:, :H, :3 W]"""
    return rng.integers(0, 256, (B, H + pad_rows, 3 * W + pad_cols), dtype=np.uint8)


def _frames(d_buf, H, W):
    return d_buf[:, :H, :3 * W].unflatten(2, (W, 3))


def _device(eng, buf, H, W, regions, effect, strength):
    d_buf = torch.from_numpy(buf).to(DEV)
    rd = redact.Redactor(redact.RedactConfig(effect=effect, strength=strength or None, fill_color=FILL), eng)
    rd.apply_regions_device(_frames(d_buf, H, W), regions)
    torch.cuda.synchronize(DEV)
    return d_buf.cpu().numpy()


def _want(buf, H, W, regions, effect, strength):
    out = buf.copy()
    for b, (rows, verts) in enumerate(regions):
        out[b, :H, :3 * W] = R.redact(buf[b, :H, :3 * W].reshape(H, W, 3), rows, verts, effect, strength, FILL).reshape(H, 3 * W)
    return out


def _same(got, want, what):
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), f"{what}: {int((got != want).sum())} bytes differ"


def _region(shape, x0, y0, x1, y1, voff=0):
    """One region of `shape` filling the box -> (row, its vertices)"""
    if shape != R.POLY:
        return [shape, x0, y0, x1, y1, 0, 0, 0], np.zeros((0, 2), np.int32)
    xm, ym = (x0 + x1) // 2, (y0 + y1) // 2
    q = np.int32([[x0, y0], [xm, ym], [x1, y0], [x1, y1], [xm, y1 - (y1 - y0) // 3], [x0, y1]])      # a concave hexagon; a point when the box is one
    return [R.POLY, int(q[:, 0].min()), int(q[:, 1].min()), int(q[:, 0].max()), int(q[:, 1].max()), voff, len(q), 0], q


def _pack(items):
    """[(row, vertices)] -> (rows [n, 8], vertices [m, 2]) with running vertex offsets"""
    rows, verts, off = [], [], 0
    for row, q in items:
        row = list(row)
        if row[0] == R.POLY:
            row[5] = off
        off += len(q)
        rows.append(row)
        verts.append(np.asarray(q, np.int32).reshape(-1, 2))
    return np.asarray(rows, np.int32).reshape(-1, 8), (np.concatenate(verts) if verts else np.zeros((0, 2), np.int32))


# W = 97, H = 75: tiles of 64 x 32 meet at x = 64 and y = 32, 64; neither side is a tile or a cell multiple
BOXES = {"inside one tile": (5, 4, 40, 20), "across a tile corner": (50, 20, 80, 45), "left border": (0, 10, 6, 30), "right border": (88, 5, 96, 25),
         "over the right border": (85, 50, 120, 60), "top border": (30, -5, 45, 3), "bottom border": (20, 66, 60, 74), "over the bottom": (3, 70, 30, 90),
         "wholly outside, above left": (-30, -30, -3, -3), "wholly outside, right": (100, 10, 130, 30), "one pixel": (70, 60, 70, 60),
         "the corner pixel": (96, 74, 96, 74), "the whole frame": (0, 0, 96, 74), "more than the frame": (-9, -7, 200, 150), "corners swapped": (40, 45, 12, 33)}


@pytest.mark.parametrize("shape", [R.RECT, R.ELLIPSE, R.POLY], ids=["rect", "ellipse", "poly"])
@pytest.mark.parametrize("effect,strength", EFFECTS)
def test_every_effect_over_every_shape_at_tile_and_frame_borders(eng, shape, effect, strength):
    H, W = 75, 97
    buf = _buffers(np.random.default_rng(7), 1, H, W)
    for what, box in BOXES.items():
        reg = [_pack([_region(shape, *box)])]
        _same(_device(eng, buf, H, W, reg, effect, strength), _want(buf, H, W, reg, effect, strength), what)
    reg = [_pack([_region(shape, *box) for box in BOXES.values()])]
    _same(_device(eng, buf, H, W, reg, effect, strength), _want(buf, H, W, reg, effect, strength), "all of them")
    outside = [_pack([_region(shape, *BOXES[k]) for k in ("wholly outside, above left", "wholly outside, right")])]
    _same(_device(eng, buf, H, W, outside, effect, strength), buf, "regions outside the frame write nothing")


@pytest.mark.parametrize("hw", [(9, 20), (1, 1)])
def test_frames_smaller_than_the_radius(eng, hw):
    H, W = hw
    buf = _buffers(np.random.default_rng(H), 1, H, W)
    for effect, strength in (("blur", 31), ("blur", 7), ("pixelate", 32), ("pixelate", 4), ("fill", 0)):
        for shape in (R.RECT, R.ELLIPSE, R.POLY):
            reg = [_pack([_region(shape, 0, 0, W - 1, H - 1)])]
            _same(_device(eng, buf, H, W, reg, effect, strength), _want(buf, H, W, reg, effect, strength), (effect, strength, shape))


def _seeded(rng, n, H, W):
    items = [_region(R.RECT, 30, 20, 150, 90)]                               # the rectangle that is split below
    for _ in range(n - 1):
        x0, y0 = int(rng.integers(-20, W)), int(rng.integers(-20, H))
        items.append(_region(int(rng.integers(0, 3)), x0, y0, x0 + int(rng.integers(0, 90)), y0 + int(rng.integers(0, 70))))
    return items


@pytest.mark.parametrize("effect,strength", [("blur", 7), ("blur", 31), ("pixelate", 8), ("fill", 0)])
def test_order_overlap_and_splitting_change_no_byte(eng, effect, strength):
    """Every output pixel is a function of the untouched input: the test that catches an in-place hazard."""
    H, W = 120, 200
    rng = np.random.default_rng(40)
    buf = _buffers(rng, 1, H, W)
    items = _seeded(rng, 40, H, W)
    split = [_region(R.RECT, 30, 20, 97, 90), _region(R.RECT, 98, 20, 150, 90)] + items[1:]
    want = _want(buf, H, W, [_pack(items)], effect, strength)
    assert (want != buf).sum() > 1000 or effect == "fill"
    for what, lst in (("the list", items), ("its reverse", items[::-1]), ("one rectangle split in two", split)):
        _same(_device(eng, buf, H, W, [_pack(lst)], effect, strength), want, what)


@pytest.mark.parametrize("effect,strength", [("blur", 15), ("pixelate", 16), ("fill", 0)])
def test_a_batch_with_5_0_and_1024_regions_and_a_polygon_at_the_vertex_cap(eng, effect, strength):
    H, W, B = 75, 97, 3
    rng = np.random.default_rng(50)
    buf = _buffers(rng, B, H, W, pad_cols=7, pad_rows=2)                     # frame_batch_stride = (H + 2) * row_stride
    nv = eng.L.ss_redact_max_vertices()
    assert nv == R.MAX_VERTICES and eng.L.ss_redact_max_regions() == R.MAX_REGIONS
    t = np.arange(nv) * (2 * np.pi / nv)
    ring = np.int32(np.stack([48 + (30 + 6 * np.sin(9 * t)) * np.cos(t), 37 + (24 + 5 * np.sin(7 * t)) * np.sin(t)], 1))
    five = _seeded(rng, 4, H, W)[1:] + [([R.POLY, int(ring[:, 0].min()), int(ring[:, 1].min()), int(ring[:, 0].max()), int(ring[:, 1].max()), 0, nv, 0], ring),
                                        _region(R.POLY, 70, 50, 96, 74)]
    many = []
    for _ in range(R.MAX_REGIONS):
        x0, y0 = int(rng.integers(-5, W)), int(rng.integers(-5, H))
        many.append(_region(int(rng.integers(0, 3)), x0, y0, x0 + int(rng.integers(0, 9)), y0 + int(rng.integers(0, 7))))
    regions = [_pack(five), _pack([]), _pack(many)]
    assert [len(r[0]) for r in regions] == [5, 0, 1024]
    got, want = _device(eng, buf, H, W, regions, effect, strength), _want(buf, H, W, regions, effect, strength)
    _same(got, want, "batch")
    assert np.array_equal(got[1], buf[1]) and (got[0] != buf[0]).any() and (got[2] != buf[2]).any()
    rd = redact.Redactor(redact.RedactConfig(effect=effect, strength=strength or None), eng)
    with pytest.raises(ValueError, match="1025 regions"):
        rd.apply_regions_device(_frames(torch.from_numpy(buf).to(DEV), H, W), [_pack(five), _pack([]), _pack(many + many[:1])])


def _raw_call(eng, frames, d_rows, d_off, d_verts, effect, strength, scratch, stream):
    eng._ck(eng.L.ss_redact(eng.ctx, C.c_void_p(stream.cuda_stream), C.c_void_p(frames.data_ptr()), frames.shape[0], frames.stride(0), frames.shape[1],
                            frames.shape[2], frames.stride(1), C.c_void_p(d_rows.data_ptr()), C.c_void_p(d_off.data_ptr()), C.c_void_p(d_verts.data_ptr()),
                            R.EFFECTS[effect], strength, FILL[0] | FILL[1] << 8 | FILL[2] << 16, C.c_void_p(scratch.data_ptr()), scratch.numel()))


@pytest.mark.parametrize("effect,strength", [("blur", 7), ("pixelate", 4)])
def test_two_calls_on_one_scratch_and_a_captured_call_equal_plain_launches(eng, effect, strength):
    H, W, B = 120, 200, 2
    rng = np.random.default_rng(60)
    buf_a, buf_b = _buffers(rng, B, H, W), _buffers(rng, B, H, W)
    reg_a = [_pack(_seeded(rng, 12, H, W)), _pack(_seeded(rng, 3, H, W))]
    reg_b = [_pack(_seeded(rng, 2, H, W)), _pack(_seeded(rng, 30, H, W))]
    want_a, want_b = _want(buf_a, H, W, reg_a, effect, strength), _want(buf_b, H, W, reg_b, effect, strength)
    _same(_device(eng, buf_a, H, W, reg_a, effect, strength), want_a, "plain launch a")
    _same(_device(eng, buf_b, H, W, reg_b, effect, strength), want_b, "plain launch b")

    def upload(regs):
        rows, off, verts, vo = [], [0], [], 0
        for rw, vt in regs:
            rw = rw.copy()
            rw[rw[:, 0] == R.POLY, 5] += vo
            rows.append(rw); verts.append(vt); off.append(off[-1] + len(rw)); vo += len(vt)
        verts = np.concatenate(verts + [np.zeros((1, 2), np.int32)])
        return [torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV) for a in (np.concatenate(rows), np.asarray(off), verts)]

    scratch = torch.empty(int(eng.L.ss_redact_scratch_bytes(B, H, W)), dtype=torch.uint8, device=DEV)
    d_a, d_b = torch.from_numpy(buf_a).to(DEV), torch.from_numpy(buf_b).to(DEV)
    up_a, up_b = upload(reg_a), upload(reg_b)
    st = torch.cuda.current_stream(DEV)
    _raw_call(eng, _frames(d_a, H, W), *up_a, effect, strength, scratch, st)                # back to back: the second call takes the scratch
    _raw_call(eng, _frames(d_b, H, W), *up_b, effect, strength, scratch, st)                # in stream order, behind the first one's store
    torch.cuda.synchronize(DEV)
    _same(d_a.cpu().numpy(), want_a, "first of two calls on one scratch")
    _same(d_b.cpu().numpy(), want_b, "second of two calls on one scratch")

    d_c = torch.from_numpy(buf_a).to(DEV)
    frames_c = _frames(d_c, H, W)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(st)
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):                                          # one linear capture: memset, three launches
            _raw_call(eng, frames_c, *up_a, effect, strength, scratch, side)
    torch.cuda.synchronize(DEV)
    _same(d_c.cpu().numpy(), buf_a, "a capture runs nothing")
    graph.replay()
    torch.cuda.synchronize(DEV)
    _same(d_c.cpu().numpy(), want_a, "replayed")
    d_c.copy_(torch.from_numpy(buf_b))                                                      # other pixels under the same regions
    torch.cuda.synchronize(DEV)
    graph.replay()
    torch.cuda.synchronize(DEV)
    _same(d_c.cpu().numpy(), _want(buf_b, H, W, reg_a, effect, strength), "replayed on new pixels")
    del graph


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _composed(frame, results, cfg, ov_ref, counts, fps_text, font):
    rows, verts = R.regions_of(results, region=cfg.region, classes=cfg.classes, pad=cfg.pad, head_scale=cfg.head_scale, head_frac=cfg.head_frac)
    red = R.redact(frame, rows, verts, cfg.effect, cfg.strength, cfg.fill_color)
    return rasterise(red, *ov_ref.commands(results, counts, fps_text).arrays(), font), len(rows)


@pytest.mark.parametrize("kw", [dict(effect="blur", strength=9), dict(effect="pixelate", region="ellipse", pad=0.1), dict(effect="fill", region="head", fill_color=(1, 2, 3)),
                                dict(effect="blur", classes=[2])], ids=["blur-box", "pixelate-ellipse-pad", "fill-head", "blur-class-2"])
def test_annotate_resident_equals_reference_redaction_then_the_oracle_rasteriser(eng, kw):
    from tests.test_overlay_cpu import _results
    names = {0: "person", 2: "car"}
    cfg = redact.RedactConfig(**kw)
    ov, ov_ref, rd = overlay.Overlay(names, eng), overlay.Overlay(names), redact.Redactor(cfg, eng)
    frame = np.random.default_rng(2).integers(0, 256, (240, 320, 3), dtype=np.uint8)
    font = font_table()
    for k in range(2):
        want, n = _composed(frame, _results(), cfg, ov_ref, {"person": 1}, "FPS: 9.00", font)
        got = ov.draw(frame, _results(), counts={"person": 1}, fps_text="FPS: 9.00", redact=rd)
        assert n > 0 and got.tobytes() == want.tobytes(), int((got != want).sum())
    plain, plain_ref = overlay.Overlay(names, eng), overlay.Overlay(names)
    got = plain.draw(frame, _results(), redact=None)
    assert got.tobytes() == rasterise(frame, *plain_ref.commands(_results()).arrays(), font).tobytes()        # None keeps the bytes


def test_cli_run_with_redact_pixelate_equals_the_composed_reference_and_keeps_the_labels(tmp_path, monkeypatch):
    from strongsort_yolo_amd.yolo import YOLO
    seen = []
    real = overlay.Overlay.annotate_resident

    def spy(self, dev_frame, results, counts=None, fps_text="", stream=None, zones=None, redact=None):
        torch.cuda.synchronize(DEV)
        seen.append((dev_frame.cpu().numpy().copy(), results, counts, fps_text, redact))
        return real(self, dev_frame, results, counts, fps_text, stream, zones, redact)

    monkeypatch.setattr(overlay.Overlay, "annotate_resident", spy)
    base = {"source": "synthetic:8", "track": True, "count": False, "tracker": "ocsort", "batch": 4, "random_init": True}

    def run(tag, **more):                                                   # a model of its own per run: the track ids start at 1 in both
        model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="ocsort")
        model.overrides.update(conf=0.01, max_det=100)                      # seeded random-init weights: a low threshold, so that there are boxes to hide
        try:
            return cli.process_video(dict(base, outdir=str(tmp_path / tag), save=str(tmp_path / f"{tag}.npy"), **more), model=model), dict(model.names)
        finally:
            model.close()

    out_a, names = run("a")
    n_plain = len(seen)
    out_b, _ = run("b", redact="pixelate", redact_region="box")
    assert out_a["frames"] == out_b["frames"] == 8 and n_plain == 8 and len(seen) == 16
    assert all(s[4] is None for s in seen[:8]) and all(isinstance(s[4], redact.Redactor) for s in seen[8:])
    labels_a, labels_b = (open(tmp_path / d / "synthetic:8_labels.txt", "rb").read() for d in "ab")
    assert labels_a == labels_b                                             # the labels never see the redaction
    cfg = cli.redact_config({"redact": "pixelate"})
    assert (cfg.effect, cfg.strength, cfg.region) == ("pixelate", 16, "box")
    got, font, ov_ref, hidden = np.load(tmp_path / "b.npy"), font_table(), overlay.Overlay(names), 0
    assert got.shape == (8, 480, 640, 3)
    for k, (frame, results, counts, fps_text, _) in enumerate(seen[8:]):
        want, n = _composed(frame, results, cfg, ov_ref, counts, fps_text, font)
        hidden += n
        assert got[k].tobytes() == want.tobytes(), (k, int((got[k] != want).sum()))
    print(f"regions hidden over the run: {hidden}; labels file: {len(labels_a)} bytes")
    assert hidden > 0
    assert not np.array_equal(got, np.load(tmp_path / "a.npy"))
