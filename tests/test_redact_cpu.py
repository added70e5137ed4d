"""Redaction without a GPU (docs/REDACT.md): tests/redact_ref.py against SciPy's mirror correlation and a brute-force loop, its
coverage rules against the overlay's, the region builder of strongsort_yolo_amd/redact.py against the reference's on crafted Results,
csrc/ss_redact_div.h proven exact by a host program, every refusal of ss_redact with a NULL context, and the command line."""
import argparse
import ctypes
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from strongsort_yolo_amd import cli, lib, overlay, redact
from strongsort_yolo_amd.yolo import OBB, Boxes, Keypoints, Results
from tests import redact_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the reference itself -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (1, 9), (5, 4), (20, 9)])
@pytest.mark.parametrize("r", [1, 7, 31])
def test_reference_blur_sums_equal_scipy_mirror_correlation(hw, r):
    ndimage = pytest.importorskip("scipy.ndimage")
    x = np.random.default_rng(hw[0] * 100 + hw[1] + r).integers(0, 256, hw, dtype=np.uint8)
    k = 2 * r + 1
    want = ndimage.correlate(x.astype(np.int64), np.ones((k, k), np.int64), mode="mirror")
    assert np.array_equal(R.blur_sums(x, r), want)


def _walk(i, n):
    if n == 1:
        return 0
    pos, d = 0, 1
    for _ in range(abs(i)):
        if not 0 <= pos + d < n:
            d = -d
        pos += d
    return pos


def test_reference_equals_a_brute_force_loop_on_a_7x6_frame():
    rng = np.random.default_rng(3)
    H, W = 6, 7
    x = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rows = np.array([[R.RECT, 1, 1, 4, 3, 0, 0, 0], [R.ELLIPSE, 6, 5, 2, 0, 0, 0, 0], [R.POLY, 0, 2, 3, 5, 0, 3, 0]], np.int32)
    verts = np.array([[0, 2], [3, 5], [0, 5]], np.int32)
    cov = np.zeros((H, W), bool)
    for y in range(H):
        for xx in range(W):
            cov[y, xx] |= 1 <= xx <= 4 and 1 <= y <= 3
            cov[y, xx] |= 2 <= xx <= 6 and (2 * xx - 8) ** 2 * 36 + (2 * y - 5) ** 2 * 25 <= 25 * 36
    assert np.array_equal(cov, R.cover(rows[:2], verts, H, W))
    full = R.cover(rows, verts, H, W)
    assert full[5, 0] and full[2, 0] and full[4, 2] and not full[0, 0]          # vertices, an edge pixel
    for r in (1, 2, 7):
        got = R.redact(x, rows, verts, "blur", r)
        k = 2 * r + 1
        for y in range(H):
            for xx in range(W):
                for c in range(3):
                    s = sum(int(x[_walk(y + dy, H), _walk(xx + dx, W), c]) for dy in range(-r, r + 1) for dx in range(-r, r + 1))
                    assert got[y, xx, c] == ((s + k * k // 2) // (k * k) if full[y, xx] else x[y, xx, c])
    got = R.redact(x, rows, verts, "pixelate", 4)
    for y in range(H):
        for xx in range(W):
            cell = x[y // 4 * 4:y // 4 * 4 + 4, xx // 4 * 4:xx // 4 * 4 + 4].astype(int)
            n = cell.shape[0] * cell.shape[1]
            for c in range(3):
                assert got[y, xx, c] == ((int(cell[..., c].sum()) + n // 2) // n if full[y, xx] else x[y, xx, c])
    got = R.redact(x, rows, verts, "fill", 0, (9, 8, 7))
    assert np.array_equal(got[full], np.tile(np.uint8([9, 8, 7]), (int(full.sum()), 1))) and np.array_equal(got[~full], x[~full])


def test_reference_polygon_interior_equals_the_overlays_polygon_mask():
    rng = np.random.default_rng(5)
    for k in (3, 5, 9, 14):
        q = rng.integers(-5, 45, (k, 2))
        want = overlay.polygon_mask(torch.from_numpy(q), 0, 0, 33, 41).numpy()
        assert np.array_equal(R.polygon_interior(q, 33, 41), want)
    assert not R.polygon_interior([[1, 1], [5, 5]], 8, 8).any()
    rows, verts = np.array([[R.POLY, 1, 1, 5, 5, 0, 2, 0]], np.int32), np.array([[1, 1], [5, 5]], np.int32)
    assert not R.cover(rows, verts, 8, 8).any()                                   # a degenerate region covers nothing, its edge included


def test_reference_ellipse_is_symmetric_and_small_rectangles_are_whole():
    H, W = 40, 50
    m = R.region_mask([R.ELLIPSE, 7, 30, 39, 4, 0, 0, 0], None, H, W)
    box = m[4:31, 7:40]
    assert np.array_equal(box, box[::-1]) and np.array_equal(box, box[:, ::-1]) and not m[:4].any() and not m[:, 40:].any()
    assert box[13, 0] and box[13, -1] and box[0, 16] and box[-1, 16] and not box[0, 0]
    assert R.region_mask([R.ELLIPSE, 3, 3, 3, 3, 0, 0, 0], None, H, W).sum() == 1
    assert R.region_mask([R.ELLIPSE, 3, 3, 4, 3, 0, 0, 0], None, H, W).sum() == 2
    assert np.array_equal(R.region_mask([R.ELLIPSE, -20, -10, 9, 9, 0, 0, 0], None, H, W),
                          R.region_mask([R.ELLIPSE, 0, 0, 9, 9, 0, 0, 0], None, H, W))                 # inscribed in the CLIPPED rectangle
    assert not R.region_mask([R.RECT, -9, -9, -1, 50, 0, 0, 0], None, H, W).any()


# ---- the region builder ---------------------------------------------------------------------------------------------------
def _boxes(xyxy, cls):
    return Boxes(torch.tensor(xyxy, dtype=torch.float32), torch.full((len(xyxy),), 0.9), torch.tensor(cls, dtype=torch.float32), None)


def _both(results, **kw):
    cfg = redact.RedactConfig(effect="fill", **kw)
    got = redact.regions_of(results, cfg, R.MAX_REGIONS, R.MAX_VERTICES)
    want = R.regions_of(results, region=cfg.region, classes=cfg.classes, pad=cfg.pad, head_scale=cfg.head_scale, head_frac=cfg.head_frac)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[0].shape[1:] == (8,) and got[1].shape[1:] == (2,)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    return got


def test_builder_boxes_pad_and_class_filter():
    res = [Results(None, {}, _boxes([[10.7, 20.2, 50.9, 90.99], [-3.5, 4.5, 12.25, 30.0], [100.0, 100.0, 100.0, 100.0]], [0, 2, 0]))]
    rows, _ = _both(res)
    assert rows[:, :5].tolist() == [[R.RECT, 10, 20, 50, 90], [R.RECT, -3, 4, 12, 30], [R.RECT, 100, 100, 100, 100]]      # int(): the drawn rectangle
    rows, _ = _both(res, region="ellipse", pad=0.1)
    assert rows[0, :5].tolist() == [R.ELLIPSE, 6, 13, 54, 97]
    rows, _ = _both(res, classes=[2])
    assert rows[:, :5].tolist() == [[R.RECT, -3, 4, 12, 30]]
    assert len(_both([None, Results(None, {}, None)])[0]) == 0


def test_builder_heads_from_five_two_one_and_no_face_keypoints():
    kp = torch.zeros(4, 17, 3)
    kp[0, :5, :2] = torch.tensor([[50.5, 40.0], [54.0, 36.5], [47.0, 36.0], [59.0, 38.0], [42.5, 38.5]])
    kp[1, 1, :2], kp[1, 3, :2] = torch.tensor([150.0, 30.0]), torch.tensor([151.0, 30.5])           # two close points: the floor box_w / 6 rules
    kp[2, 4, :2] = torch.tensor([250.25, 44.0])
    kp[3, 9, :2] = torch.tensor([300.0, 100.0])                                                     # a wrist is no face keypoint
    res = [Results(None, {}, _boxes([[30, 20, 70, 140], [120, 10, 180, 200], [230.5, 20, 275, 160], [290, 50, 330.9, 171.5]], [0, 0, 0, 0]), Keypoints(kp))]
    rows, _ = _both(res, region="head")
    assert rows[:, 0].tolist() == [R.ELLIPSE, R.ELLIPSE, R.ELLIPSE, R.RECT]
    d = float(np.hypot(59.0 - 42.5, 38.0 - 38.5))
    cx, cy = (50.5 + 54.0 + 47.0 + 59.0 + 42.5) / 5, (40.0 + 36.5 + 36.0 + 38.0 + 38.5) / 5
    assert rows[0, 1:5].tolist() == [int(np.floor(cx - .75 * d)), int(np.floor(cy - 1.25 * .75 * d)), int(np.floor(cx + .75 * d)), int(np.floor(cy + 1.25 * .75 * d))]
    assert rows[1, 1:5].tolist() == [143, 20, 158, 39]                           # a = 0.75 * 60 / 6 = 7.5 about (150.5, 30.25)
    assert rows[3, 1:5].tolist() == [290, 50, 330, 50 + 24]                      # the top fifth of the box: fails closed
    rows2, _ = _both(res, region="head", head_scale=1.0, head_frac=0.5)
    assert rows2[3, 4] == 50 + 60 and rows2[1, 1:5].tolist() == [140, 17, 160, 42]


def test_builder_masks_with_two_polygons_and_obb_rows():
    a = np.float32([[10.9, 10.1], [40.5, 12.0], [30.0, 44.7], [12.2, 40.0]])
    b = np.float32([[60, 60], [70, 60.5], [65.5, 75]])
    masks = SimpleNamespace(xy=[[a, b], np.float32([[1, 1], [2, 2]]), np.zeros((0, 2), np.float32)])
    res = [Results(None, {}, _boxes([[10, 10, 70, 75], [0, 0, 5, 5], [1, 1, 2, 2]], [0, 0, 0]), None, masks)]
    rows, verts = _both(res, region="mask")
    assert rows.tolist() == [[R.POLY, 10, 10, 40, 44, 0, 4, 0], [R.POLY, 60, 60, 70, 75, 4, 3, 0]]
    assert verts.tolist() == np.int32(a).tolist() + np.int32(b).tolist()
    obb = OBB(torch.tensor([[50.0, 40.0, 30.0, 10.0, 0.5], [20.0, 20.0, 8.0, 4.0, 0.0]]), torch.zeros(2, 4), torch.tensor([0.9, 0.8]), torch.tensor([1.0, 3.0]))
    res = [Results(None, {}, None, obb=obb)]
    rows, verts = _both(res, region="ellipse")
    assert rows[:, 0].tolist() == [R.POLY, R.POLY] and rows[:, 5:7].tolist() == [[0, 4], [4, 4]]
    assert verts.tolist() == np.int32(obb.xyxyxyxy.numpy()).reshape(-1, 2).tolist()
    assert len(_both(res, classes=[3])[0]) == 1


def test_builder_raises_on_caps_and_refuses_head_and_mask_by_name():
    many = [Results(None, {}, _boxes([[i, 0, i + 5, 9] for i in range(9)], [0] * 9))]
    cfg = redact.RedactConfig(effect="blur")
    assert len(redact.regions_of(many, cfg, 9, 16)[0]) == 9
    with pytest.raises(ValueError, match="9 regions .* cap of 8"):
        redact.regions_of(many, cfg, 8, 16)
    with pytest.raises(ValueError, match="cap of 8"):
        R.regions_of(many, max_regions=8)
    ring = np.float32([[i, (i * 7) % 13] for i in range(17)])
    res = [Results(None, {}, _boxes([[0, 0, 9, 9]], [0]), None, SimpleNamespace(xy=[ring]))]
    with pytest.raises(ValueError, match="17 vertices .* cap of 16"):
        redact.regions_of(res, redact.RedactConfig(effect="blur", region="mask"), 9, 16)
    with pytest.raises(ValueError, match="17 vertices"):
        R.regions_of(res, region="mask", max_vertices=16)
    far = [Results(None, {}, _boxes([[0, 0, 9, 9]], [0]), None, SimpleNamespace(xy=[np.float32([[0, 0], [20000, 5], [3, 9]])]))]
    with pytest.raises(ValueError, match="outside -8192 .. 16383"):
        redact.regions_of(far, redact.RedactConfig(effect="blur", region="mask"), 9, 16)
    plain = [Results(None, {}, _boxes([[0, 0, 9, 9]], [0]))]
    with pytest.raises(ValueError, match="'head' needs keypoints: use a pose model"):
        redact.regions_of(plain, redact.RedactConfig(effect="blur", region="head"), 9, 16)
    with pytest.raises(ValueError, match="'mask' needs masks: use a segmentation model"):
        redact.regions_of(plain, redact.RedactConfig(effect="blur", region="mask"), 9, 16)
    obb = [Results(None, {}, None, obb=OBB(torch.tensor([[5.0, 5.0, 4.0, 2.0, 0.1]]), torch.zeros(1, 4), torch.tensor([0.9]), torch.tensor([0.0])))]
    with pytest.raises(ValueError, match="'head' is not available on an oriented-box model"):
        redact.regions_of(obb, redact.RedactConfig(effect="blur", region="head"), 9, 16)
    for bad in (dict(effect="smear"), dict(effect="blur", strength=0), dict(effect="blur", strength=32), dict(effect="pixelate", strength=5),
                dict(effect="fill", region="face"), dict(effect="fill", fill_color=(0, 0, 256)), dict(effect="fill", pad=-0.1)):
        with pytest.raises(ValueError, match="redact"):
            redact.RedactConfig(**bad)
    assert redact.RedactConfig(effect="blur").strength == 15 and redact.RedactConfig(effect="pixelate").strength == 16


# ---- the divider, the library's checks ------------------------------------------------------------------------------------
def test_multiply_shift_divider_is_exact_for_every_radius_and_sum(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "clang++"
    exe = str(tmp_path / "redact_div_host")
    subprocess.check_call([cxx, "-O2", "-std=c++17", os.path.join(HERE, "redact_div_host_main.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, check=True, text=True).stdout.split()
    assert out == ["ok", str(sum(255 * (2 * r + 1) ** 2 + 1 for r in range(1, 32)))]


def test_getters_and_every_refusal_of_ss_redact_with_a_null_context():
    lib.build()
    L = lib.load()
    assert (L.ss_redact_max_regions(), L.ss_redact_max_vertices(), L.ss_redact_max_radius()) == (R.MAX_REGIONS, R.MAX_VERTICES, R.MAX_RADIUS)
    assert redact.caps() == {"regions": 1024, "vertices": 4096, "radius": 31}
    from strongsort_yolo_amd.yolo import YOLO
    assert L.ss_redact_max_vertices() >= YOLO.MASK_CAP
    tiles = lambda b, h, w: b * ((w + 63) // 64) * ((h + 31) // 32)
    for b, h, w in ((1, 1, 1), (3, 75, 97), (32, 720, 1280), (1, 8192, 8192)):
        n = tiles(b, h, w)
        assert L.ss_redact_scratch_bytes(b, h, w) == 256 + (4 * n + 255) // 256 * 256 + n * (64 * 32 * 3 + 256)
    for b, h, w in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 0), (1, 8193, 4), (1, 4, 8193), (-1, 4, 4)):
        assert L.ss_redact_scratch_bytes(b, h, w) < 0
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    big = 1 << 40

    def call(frames=p, batch=2, stride=75 * 300, h=75, w=97, rs=300, regs=p, off=p, verts=p, effect=0, strength=7, fill=0, scratch=p, nbytes=big):
        rc = L.ss_redact(None, None, frames, batch, stride, h, w, rs, regs, off, verts, effect, strength, fill, scratch, nbytes)
        return rc, (L.ss_last_error(None) or b"").decode()

    assert call() == (lib.SS_ERR_INVALID, "ss_redact: null context")               # every argument is sound: only the context is missing
    for bad, why in ((dict(frames=None), "null pointer"), (dict(regs=None), "null pointer"), (dict(off=None), "null pointer"),
                     (dict(verts=None), "null pointer"), (dict(scratch=None), "null pointer"),
                     (dict(batch=0), "batch"), (dict(batch=-2), "batch"), (dict(batch=65536), "batch"),
                     (dict(h=0), "frame size"), (dict(w=0), "frame size"), (dict(h=-5), "frame size"), (dict(h=8193, stride=big), "frame size"),
                     (dict(w=8193, rs=3 * 8193), "frame size"), (dict(rs=3 * 97 - 1), "row_stride"), (dict(stride=75 * 300 - 1), "overlap"),
                     (dict(effect=-1), "effect"), (dict(effect=3), "effect"), (dict(strength=0), "radius"), (dict(strength=32), "radius"),
                     (dict(effect=1, strength=7), "cell"), (dict(effect=1, strength=64), "cell"), (dict(effect=1, strength=0), "cell"),
                     (dict(fill=-1), "fill colour"), (dict(fill=1 << 24), "fill colour"), (dict(scratch=p + 4), "aligned"),
                     (dict(nbytes=L.ss_redact_scratch_bytes(2, 75, 97) - 1), "scratch_bytes"), (dict(nbytes=0), "scratch_bytes")):
        rc, msg = call(**bad)
        assert rc == lib.SS_ERR_INVALID and msg.startswith("ss_redact: ") and why in msg and "null context" not in msg, (bad, msg)
    for ok in (dict(effect=2, strength=0), dict(effect=2, strength=99), dict(effect=1, strength=32), dict(batch=1, stride=0),
               dict(nbytes=L.ss_redact_scratch_bytes(2, 75, 97)), dict(h=8192, w=8192, rs=3 * 8192, stride=3 * 8192 * 8192)):
        assert call(**ok)[1] == "ss_redact: null context", ok


# ---- the command line -----------------------------------------------------------------------------------------------------
def _ns(**kw):
    base = dict(redact=None, redact_region="box", redact_strength=None, redact_classes=None, redact_pad=0.0, redact_color=None, save=None, weights="yolov8n-pose.pt")
    return argparse.Namespace(**dict(base, **kw))


def test_cli_refuses_redact_without_save_and_round_trips_the_flags(capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["--redact", "blur"])
    assert e.value.code == 2 and "--redact hides people in the annotated output: it needs --save" in capsys.readouterr().err
    for argv, why in ((["--redact-strength", "9"], "are options of --redact"), (["--redact-region", "head", "--save", "x.npy"], "are options of --redact"),
                      (["--redact", "blur", "--save", "x.npy", "--redact-strength", "40"], "radius must be 1 .. 31"),
                      (["--redact", "pixelate", "--save", "x.npy", "--redact-strength", "5"], "one of 4, 8, 16, 32"),
                      (["--redact", "blur", "--save", "x.npy", "--redact-color", "1", "2", "3"], "colour of --redact fill"),
                      (["--redact", "fill", "--save", "x.npy", "--redact-color", "1", "2", "300"], "0 .. 255"),
                      (["--redact", "blur", "--save", "x.npy", "--redact-region", "head", "--weights", "yolov8n.pt"], "needs a pose model"),
                      (["--redact", "blur", "--save", "x.npy", "--redact-region", "mask", "--weights", "yolov8n.pt"], "needs a segmentation model")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and why in capsys.readouterr().err, argv
    assert cli.redact_refusal(_ns()) is None and cli.redact_config(vars(_ns())) is None
    a = _ns(redact="pixelate", redact_region="head", redact_strength=8, redact_classes=[0, 2], redact_pad=0.25, save="out.npy")
    assert cli.redact_refusal(a) is None
    cfg = cli.redact_config(vars(a))
    assert (cfg.effect, cfg.strength, cfg.region, cfg.classes, cfg.pad, cfg.fill_color) == ("pixelate", 8, "head", (0, 2), 0.25, (0, 0, 0))
    cfg = cli.redact_config(vars(_ns(redact="fill", redact_color=[1, 2, 3], save="o.npy")))
    assert (cfg.effect, cfg.fill_color, cfg.region) == ("fill", (1, 2, 3), "box")
    assert cli.redact_config(vars(_ns(redact="blur", save="o.npy"))).strength == 15
