"""BoT-SORT's `model: auto` ReID features (docs/BYTETRACK.md §1d) without a GPU: tests/native_feats_ref.py against Ultralytics'
get_obj_feats expression, and the argument surface of YOLO, FramePipeline, BYTETracker and the CLI."""
import os

import numpy as np
import pytest
import torch

from tests.native_feats_ref import FEAT_DIM, anchor_pixel, native_feats, native_row, ultralytics_obj_feats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((8, 10), (4, 5), (2, 3))          # three levels of a 64 x 80 letterbox: 80 + 20 + 6 anchors


def _maps(chans, dtype, seed, B=2, wide=0):
    """Random maps [B, C_l, H_l, W_l]; wide > 0: each a channel slice [wide : wide + C_l] of a wider channels-last tensor."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for c, (h, w) in zip(chans, SHAPES):
        x = (torch.randn(B, c + 2 * wide, h, w, generator=g) * 3).to(dtype).contiguous(memory_format=torch.channels_last)
        out.append(x[:, wide:wide + c] if wide else x)
    return out


def _boundary_anchors():
    A = [h * w for h, w in SHAPES]
    e0, e1, e2 = A[0], A[0] + A[1], sum(A)
    return [0, 1, e0 - 1, e0, e0 + 1, e1 - 1, e1, e1 + 1, e2 - 1, 37]


def _ulps32(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def _ulps16(a, b):
    ia, ib = a.view(np.int16).astype(np.int64), b.view(np.int16).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("chans", [(16, 32, 64), (24, 48, 72), (16, 48, 64), (32, 32, 32)])     # g = (1,2,4), (1,2,3), (1,3,4), (1,1,1)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("wide", [0, 8])
def test_restatement_equals_ultralytics_expression(chans, dtype, wide):
    maps = _maps(chans, dtype, seed=sum(chans) + wide, wide=wide)
    s = min(chans)
    anchors = _boundary_anchors()
    keep = np.array([anchors, anchors[::-1]], np.int32)
    ours = native_feats(maps, np.pad(keep, ((0, 0), (0, 128 - len(anchors)))), np.array([len(anchors)] * 2, np.int32))
    ult = ultralytics_obj_feats(maps, [torch.as_tensor(k, dtype=torch.long) for k in keep])
    for b in range(2):
        u = ult[b].numpy()
        assert u.dtype == (np.float32 if dtype == torch.float32 else np.float16)        # N-02: Ultralytics keeps the map's dtype
        o = ours[b, :len(anchors)]
        assert not o[:, s:].any()                                                     # N-03: zero padding to 512
        for r, a in enumerate(keep[b]):
            lv = anchor_pixel(SHAPES, int(a))[0]
            g = chans[lv] // s
            if dtype == torch.float32:
                d = _ulps32(o[r, :s], u[r])
                assert d.max() == 0 if g == 1 else d.max() <= 1, (b, r, g, d.max())
            else:                        # our f32 value rounded to f16 against Ultralytics' f16 mean
                d = _ulps16(o[r, :s].astype(np.float16), u[r])
                assert d.max() == 0 if g == 1 else d.max() <= 1, (b, r, g, d.max())
                if g == 1:
                    assert o[r, :s].tobytes() == u[r].astype(np.float32).tobytes()     # g = 1: the map's value itself


def test_restatement_order_and_divide():
    """N-01 by hand: g = 3, the sum from the first term in channel order, then one correctly rounded divide."""
    m0 = torch.zeros(1, 64, 1, 1)
    m1 = torch.zeros(1, 192, 1, 1)
    m2 = torch.zeros(1, 128, 1, 1)
    trio = np.array([1e8, 1.0, -1e8], np.float32)               # (1e8 + 1) - 1e8 = 0 in f32; another order gives 1
    m1[0, :3, 0, 0] = torch.from_numpy(trio)
    m1[0, 3:6, 0, 0] = torch.tensor([1.0, 1.0, 0.5])
    row = native_row([m0, m1, m2], 0, 1)                        # anchor 1 = the only pixel of P4
    assert row[0] == np.float32(0.0)
    assert row[1] == np.float32(2.5) / np.float32(3)
    assert row.shape == (FEAT_DIM,) and not row[64:].any()
    with pytest.raises(ValueError):                             # C_l % s != 0
        native_row([m0, m1, torch.zeros(1, 100, 1, 1)], 0, 0)
    with pytest.raises(ValueError):                             # s > 512
        native_row([torch.zeros(1, 1024, 1, 1)] * 3, 0, 0)


def test_rows_past_the_count_are_left_alone():
    maps = _maps((16, 32, 64), torch.float32, 3)
    out = np.full((2, 128, FEAT_DIM), np.nan, np.float32)
    keep = np.zeros((2, 128), np.int32)
    keep[:, :3] = [[0, 80, 105], [5, 6, 7]]
    native_feats(maps, keep, np.array([3, 0], np.int32), out=out)
    assert np.isfinite(out[0, :3]).all() and np.isnan(out[0, 3:]).all() and np.isnan(out[1]).all()


# ---- argument surface ----------------------------------------------------------------------------------------------------------
def test_reid_model_arguments():
    from strongsort_yolo_amd.config import REID_MODELS, check_reid_model
    from strongsort_yolo_amd.yolo import YOLO
    assert REID_MODELS == ("osnet", "auto")
    assert check_reid_model("osnet", False) == "osnet" and check_reid_model("auto", True) == "auto"
    m = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", with_reid=True, reid_model="auto")
    assert m._pipe_kw["reid_model"] == "auto" and m._pipe_kw["with_reid"] is True and m.reid_model == "auto"
    m = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", with_reid=True)
    assert "reid_model" not in m._pipe_kw and m.reid_model == "osnet"                  # the default: today's pipeline keywords
    m = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", with_reid=True, reid_model="auto", half=False)
    assert m._pipe_kw["half"] is False
    with pytest.raises(ValueError):
        YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", with_reid=True, reid_model="resnet")
    for t in ("botsort", "bytetrack", "strongsort"):                                   # auto without with_reid
        with pytest.raises(ValueError):
            YOLO("yolov8n.pt", random_init_ok=True, tracker_type=t, reid_model="auto")
    with pytest.raises(ValueError):                                                     # auto with an OSNet weights file
        YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", with_reid=True, reid_model="auto", reid_weights="osnet.pth")


def test_pipeline_and_tracker_refuse_auto_without_reid():
    """Checked before any device work, so these raise on a machine without a GPU too."""
    from strongsort_yolo_amd.config import ByteTrackConfig
    from strongsort_yolo_amd.pipeline import FramePipeline, OverlappedPipeline
    from strongsort_yolo_amd.tracker import BYTETracker
    for kw in ({"tracker": "botsort", "reid_model": "auto"}, {"tracker": "botsort", "with_reid": True, "reid_model": "x"},
               {"tracker": "strongsort", "reid_model": "auto"}):
        with pytest.raises(ValueError):
            FramePipeline("yolov8n", **kw)
        with pytest.raises(ValueError):
            OverlappedPipeline("yolov8n", **kw)
    with pytest.raises(ValueError):
        BYTETracker(ByteTrackConfig(kalman="xywh"), reid_model="auto")
    with pytest.raises(ValueError):
        BYTETracker(ByteTrackConfig(kalman="xywh", with_reid=True), reid_model="auto", reid_weights="osnet.pth")


def test_cli_reid_model_flag(monkeypatch):
    from strongsort_yolo_amd import cli
    monkeypatch.setattr(cli, "process_video", lambda job: job)
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--tracker", "botsort", "--with-reid", "--reid-model", "auto"])
    assert job["reid_model"] == "auto" and job["with_reid"] is True
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--tracker", "botsort", "--with-reid"])
    assert job["reid_model"] == "osnet"
    for argv in (["--tracker", "botsort", "--reid-model", "auto"], ["--tracker", "botsort", "--with-reid", "--reid-model", "resnet"],
                 ["--tracker", "botsort", "--with-reid", "--reid-model", "auto", "--reid-weights", "osnet.pth"]):
        with pytest.raises(SystemExit):
            cli.main(["--source", "synthetic:3", "--track"] + argv)


def test_cli_passes_reid_model_to_the_model(monkeypatch):
    from strongsort_yolo_amd import cli, yolo
    seen = {}

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(yolo, "YOLO", fake)
    with pytest.raises(Stop):
        cli.process_video({"source": "synthetic:2", "track": True, "count": False, "tracker": "botsort", "with_reid": True,
                           "reid_model": "auto"})
    assert seen["reid_model"] == "auto" and seen["with_reid"] is True


def test_native_entry_point_is_declared_exported_and_checks_arguments():
    """ss_native_feats is in the header, the export list and the binding; a bad call returns SS_ERR_INVALID before the device
    is touched (a NULL context included)."""
    from strongsort_yolo_amd import lib
    src = open(os.path.join(ROOT, "include", "strongsort_hip.h")).read()
    assert "int ss_native_feats(ss_ctx* ctx, int n_img, int half, const ss_native_map* maps, int s," in src
    body = src[src.index("typedef struct ss_native_map {"):src.index("} ss_native_map;")]
    assert [f for f, _ in lib.ss_native_map._fields_] == ["data", "img_stride", "row_stride", "pix_stride", "channels", "height", "width"]
    for f in ("data", "img_stride", "row_stride", "pix_stride", "channels", "height", "width"):
        assert f in body
    lib.build()
    L = lib.load()
    assert "ss_native_feats" in lib.EXPORTS and L.ss_native_feats.argtypes is not None
    maps = (lib.ss_native_map * 3)()
    for m, (c, h, w) in zip(maps, ((64, 8, 8), (128, 4, 4), (256, 2, 2))):
        m.data, m.channels, m.height, m.width = 256, c, h, w
        m.pix_stride, m.row_stride, m.img_stride = c, c * w, c * w * h
    assert L.ss_native_feats(None, 1, 1, maps, 64, 256, 128, 256, 256) == lib.SS_ERR_INVALID
