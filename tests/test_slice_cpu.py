"""Sliced inference without a GPU: the tile grid and canvas, the reference merge on hand-made cases, the refusals of YOLO(...), of the
library (argument checks only) and of the command line, and that the fields tests/test_gpu_slice.py uses are not vacuous."""
import ctypes as C

import numpy as np
import pytest

from strongsort_yolo_amd import cli, lib, slicing
from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry
from tests import slice_fields as sf, slice_ref as ref

F = np.float32


# ---- grid and canvas --------------------------------------------------------------------------------------------------------
def test_grid_known_answer():
    tiles = slicing.grid(720, 1280, (640, 640), 0.2)
    assert len(tiles) == 7 and tiles[-1] == (0, 0, 1280, 720)
    assert sorted({t[0] for t in tiles[:6]}) == [0, 512, 640] and sorted({t[1] for t in tiles[:6]}) == [0, 80]
    assert [t[:2] for t in tiles[:6]] == [(0, 0), (512, 0), (640, 0), (0, 80), (512, 80), (640, 80)]          # row-major
    assert all(t[2:] == (640, 640) for t in tiles[:6])


def test_grid_edges():
    assert slicing.grid(128, 192, (64, 64), 0.0, full=False) == [(x, y, 64, 64) for y in (0, 64) for x in (0, 64, 128)]
    assert slicing.grid(96, 160, (96, 160), 0.2, full=False) == [(0, 0, 160, 96)]                               # slice == frame: one tile
    assert len(slicing.grid(96, 160, (96, 160), 0.2)) == 2
    t = slicing.grid(100, 150, (64, 64), (0.25, 0.5), full=False)                                              # a border shift on both axes
    assert sorted({q[1] for q in t}) == [0, 36] and sorted({q[0] for q in t}) == [0, 32, 64, 86]
    assert all(q[0] + 64 <= 150 and q[1] + 64 <= 100 for q in t)
    assert len(slicing.grid(96, 160, (64, 64), 0.25)) == 7


def test_grid_refusals():
    with pytest.raises(ValueError, match="height"):
        slicing.grid(96, 160, (97, 64))
    with pytest.raises(ValueError, match="width"):
        slicing.grid(96, 160, (64, 161))
    with pytest.raises(ValueError, match="at most 64"):
        slicing.grid(512, 512, (64, 64), 0.0)                      # 64 cut tiles and the full frame
    assert len(slicing.grid(512, 512, (64, 64), 0.0, full=False)) == 64
    for bad in (dict(overlap=1.0), dict(overlap=(-0.1, 0.2)), dict(merge="soft"), dict(metric="giou"), dict(thr=float("nan"))):
        with pytest.raises(ValueError):
            slicing.SliceConfig((64, 64), **bad)
    with pytest.raises(ValueError):
        slicing.SliceConfig((0, 64))
    assert slicing.rows_per_tile(128, 7) == 128 and slicing.rows_per_tile(1024, 7) == 1024 and slicing.rows_per_tile(1024, 64) == 128


def test_canvas_and_geometry():
    cfg = slicing.SliceConfig((640, 640), 0.2)
    g, table = slicing.canvas(720, 1280, cfg)
    assert (g.out_h, g.out_w) == (640, 640) and table.shape == (7, 8) and table.dtype == np.int32
    assert table[0].tolist() == [0, 0, 640, 640, 640, 640, 0, 0]                       # the identity tile
    # the whole frame in the same canvas: r = 0.5, 640 x 360, centred with the round(x - 0.1) rule
    assert table[6].tolist() == [0, 0, 1280, 720, 640, 360, 0, 140]
    geom = slicing.nms_geometry(g, table)
    assert geom[0].tolist() == [1.0, 0.0, 0.0, 640.0, 640.0] and geom[6].tolist() == [0.5, 0.0, 140.0, 1280.0, 720.0]
    assert slicing.SliceConfig((64, 64)).key() != slicing.SliceConfig((64, 64), thr=0.4).key()


# ---- the reference merge on hand-made cases ---------------------------------------------------------------------------------
def _tiles(*per_tile, ld=6):
    """per_tile: lists of rows -> (rows [T, R, ld], counts)."""
    R = max(max((len(p) for p in per_tile), default=1), 1)
    rows, counts = np.zeros((len(per_tile), R, ld), F), np.zeros(len(per_tile), np.int32)
    for t, p in enumerate(per_tile):
        for r, row in enumerate(p):
            rows[t, r, :len(row)] = row
        counts[t] = len(p)
    return rows, counts, R


def test_box_split_over_two_tiles_becomes_its_union():
    # an object spanning x 40..90: tile 0 (origin 0, 64 wide) sees 40..64, tile 1 (origin 48) sees 48..90 as 0..42
    rows, counts, R = _tiles([[40, 10, 64, 30, 0.9, 2]], [[0, 10, 42, 30, 0.8, 2]])
    out, m, src = ref.merge(rows, counts, [(0, 0), (48, 0)], R, "nmm", "ios", 0.5)
    assert m == 1 and out[0].tolist() == [40, 10, 90, 30, F(0.9), 2] and src.tolist() == [0]
    out, m, src = ref.merge(rows, counts, [(0, 0), (48, 0)], R, "nms", "ios", 0.5)
    assert m == 1 and out[0, :4].tolist() == [40, 10, 64, 30]                              # nms: the duplicate is dropped, the box stays


def test_chain_grows_only_through_the_recheck():
    # A = 0..8, B = 0..10 (ios(A, B) = 1), C = 4..12: ios(A, C) = 32 / 64 = 0.5 exactly -> C is removed by A (>=) but the strict test
    # against A itself fails; against A u B = 0..10 it is 48 / 64 = 0.75 > 0.5, so C joins only because the box is re-checked as merged
    rows, counts, R = _tiles([[0, 0, 8, 8, 0.9, 0]], [[0, 0, 10, 8, 0.8, 0]], [[4, 0, 12, 8, 0.7, 0]])
    org = [(0, 0)] * 3
    out, m, src, st = ref.merge(rows, counts, org, R, "nmm", "ios", 0.5, want_stats=True)
    assert m == 1 and out[0, :4].tolist() == [0, 0, 12, 8] and st["rechecks"] == 1
    # without B the chain does not start: C stays removed and unmerged
    rows2, counts2, R2 = _tiles([[0, 0, 8, 8, 0.9, 0]], [[4, 0, 12, 8, 0.7, 0]])
    out, m, src = ref.merge(rows2, counts2, org[:2], R2, "nmm", "ios", 0.5)
    assert m == 1 and out[0, :4].tolist() == [0, 0, 8, 8]


def test_ge_against_gt_at_a_representable_threshold():
    # ios exactly 0.5: removed (>=) in both modes; one ulp above the threshold it is not even removed
    rows, counts, R = _tiles([[0, 0, 8, 8, 0.9, 0]], [[4, 0, 12, 8, 0.7, 0]])
    org = [(0, 0)] * 2
    assert ref.merge(rows, counts, org, R, "nms", "ios", 0.5)[1] == 1
    assert ref.merge(rows, counts, org, R, "nms", "ios", np.nextafter(F(0.5), F(1)))[1] == 2
    out, m, _ = ref.merge(rows, counts, org, R, "nmm", "ios", np.nextafter(F(0.5), F(0)))  # just below: strictly above now, merged
    assert m == 1 and out[0, :4].tolist() == [0, 0, 12, 8]


def test_equal_scores_across_tiles_order_by_tile_then_row():
    rows, counts, R = _tiles([[0, 0, 10, 10, 0.5, 0], [50, 0, 60, 10, 0.5, 0]], [[0, 0, 10, 10, 0.5, 0]], [[20, 0, 30, 10, 0.5, 0]])
    out, m, src = ref.merge(rows, counts, [(0, 0), (100, 0), (0, 0)], R, "nmm", "iou", 0.5)
    assert src.tolist() == [0, 1, 2, 4] and out[:, 0].tolist() == [0, 50, 100, 20]          # source index = tile * R + row, R = 2
    # a tie between duplicates: the lower tile keeps, the higher is merged into it
    out, m, src = ref.merge(rows, counts, [(0, 0), (0, 0), (0, 0)], R, "nmm", "iou", 0.5)
    assert src.tolist() == [0, 1, 4]


def test_classes_agnostic_and_not():
    rows, counts, R = _tiles([[0, 0, 10, 10, 0.9, 1]], [[0, 0, 10, 10, 0.8, 2]])
    org = [(0, 0)] * 2
    assert ref.merge(rows, counts, org, R, "nmm", "ios", 0.5, agnostic=False)[1] == 2
    out, m, _ = ref.merge(rows, counts, org, R, "nmm", "ios", 0.5, agnostic=True)
    assert m == 1 and out[0, 5] == 1


def test_zero_area_box_matches_nothing():
    rows, counts, R = _tiles([[5, 5, 5, 9, 0.9, 0]], [[5, 5, 5, 9, 0.8, 0]], [[0, 0, 10, 10, 0.7, 0]])
    for metric in ("ios", "iou"):
        assert ref.merge(rows, counts, [(0, 0)] * 3, R, "nmm", metric, 0.5)[1] == 3         # 0 / 0 is NaN, 0 / area is 0: neither matches


def test_counts_are_clamped_and_out_cap_cuts():
    rows, counts, R = _tiles([[0, 0, 10, 10, 0.9, 0], [20, 0, 30, 10, 0.8, 0]], [[40, 0, 50, 10, 0.7, 0], [60, 0, 70, 10, 0.95, 0]])
    counts[0], counts[1] = 7, -2
    out, m, src = ref.merge(rows, counts, [(0, 0)] * 2, R, "nmm", "ios", 0.5)
    assert m == 2 and src.tolist() == [0, 1]
    assert ref.merge(rows, [2, 2], [(0, 0)] * 2, R, "nmm", "ios", 0.5, out_cap=3)[2].tolist() == [3, 0, 1]


def test_keypoints_against_a_hand_computation():
    rows, counts, R = _tiles([], [[8, 8, 40, 40, 0.9, 0, 33.0, 70.0, 0.6, 12.5, 90.25, 0.3, 7.0]], ld=13)
    tg = np.array([[2.0, 0.0, 0.0], [2.0, 4.0, 6.0]], F)
    out, m, _ = ref.merge(rows, counts, [(0, 0), (48, 16)], R, "nmm", "ios", 0.5, n_kpt=2, tile_geom=tg, frame_geom=(0.5, 3.0, 20.0))
    # ((33 - 4) / 2 + 48) * 0.5 + 3 = 34.25;  ((70 - 6) / 2 + 16) * 0.5 + 20 = 44;  ((12.5 - 4) / 2 + 48) * 0.5 + 3 = 29.125;  ((90.25 - 6) / 2 + 16) * .5 + 20 = 49.0625
    assert out[0, 6:].tolist() == [34.25, 44.0, F(0.6), 29.125, 49.0625, F(0.3), 7.0]
    assert out[0, :4].tolist() == [56, 24, 88, 56]


@pytest.mark.parametrize("name", [n for n in sf.CASES if sf.CASES[n][6] >= 63])
def test_gpu_fields_are_not_vacuous(name):
    """What tests/test_gpu_slice.py asserts again on its own fields, shown here on the reference alone (seed 7)."""
    su = sf.setup(name)
    rows, counts, seen = sf.field(su, 7)
    assert int(counts.sum()) == su["total"] and counts.max() <= su["R"]
    assert (seen >= 2).mean() >= 1 / 3
    for metric in ("ios", "iou"):
        out, m, src, st = ref.merge(rows, counts, su["table"][:, :2], su["R"], "nmm", metric, 0.5, False, su["T"] * su["R"], want_stats=True)
        assert m < su["total"] and st["rechecks"] >= 1
        assert len(set(src.tolist())) == m


# ---- refusals: Python, library, command line --------------------------------------------------------------------------------
def test_yolo_refusals():
    from strongsort_yolo_amd.yolo import YOLO
    with pytest.raises(ValueError, match="segmentation"):
        YOLO("yolov8n-seg.pt", random_init_ok=True, slice_hw=(64, 64))
    with pytest.raises(ValueError, match="auto"):
        YOLO("yolov8n.pt", random_init_ok=True, tracker_type="botsort", with_reid=True, reid_model="auto", slice_hw=(64, 64))
    with pytest.raises(ValueError, match="overlap"):
        YOLO("yolov8n.pt", random_init_ok=True, slice_hw=(64, 64), slice_overlap=1.0)
    with pytest.raises(ValueError, match="slice_merge"):
        YOLO("yolov8n.pt", random_init_ok=True, slice_hw=(64, 64), slice_merge="wbf")
    m = YOLO("yolov8n.pt", random_init_ok=True, slice_hw=(64, 64), slice_thr=0.4)
    assert m._pipe_kw["slice_cfg"].thr == 0.4 and m._state_key((96, 160), 0)[-1] == m.slice.key()
    assert YOLO("yolov8n.pt", random_init_ok=True)._state_key((96, 160), 0)[-1] is None and "slice_cfg" not in YOLO("yolov8n.pt", random_init_ok=True)._pipe_kw


def test_library_refuses_before_it_touches_a_context():
    lib.build()
    L = lib.load()
    assert L.ss_slice_max_tiles() == slicing.MAX_TILES == 64 and L.ss_slice_max_candidates() == slicing.MAX_CANDIDATES == 8192
    pi = C.POINTER(C.c_int)

    def config(table, T=None, fh=96, fw=160, ch=64, cw=64, R=128, nx=0, nk=0, kg=1.0):
        t = np.ascontiguousarray(table, np.int32)
        return L.ss_slice_config(None, t.ctypes.data_as(pi), len(t) if T is None else T, fh, fw, ch, cw, R, nx, nk, kg, 0.0, 0.0), L.ss_last_error(None).decode()

    ok = [[0, 0, 64, 64, 64, 64, 0, 0]]
    assert config(ok) == (lib.SS_ERR_INVALID, "ss_slice_config: null context")             # every argument passed the checks
    for kw, word in ((dict(T=65), "65 tiles"), (dict(T=0), "0 tiles"), (dict(R=0), "rows_per_tile"), (dict(fh=0), "frame size"),
                     (dict(ch=0), "canvas size"), (dict(nx=3, nk=2), "keypoint triples"), (dict(nx=3, nk=1, kg=0.0), "keypoint geometry")):
        rc, msg = config(ok * max(kw.get("T", 1), 1), **kw)
        assert rc == lib.SS_ERR_INVALID and word in msg, (kw, msg)
    rc, msg = config(ok * 64, R=129)
    assert rc == lib.SS_ERR_INVALID and "8192" in msg                                         # T * rows_per_tile > 8192
    assert config(ok * 64, R=128)[1].endswith("null context")
    rc, msg = config(ok + [[100, 0, 64, 64, 64, 64, 0, 0]])
    assert rc == lib.SS_ERR_INVALID and "tile 1" in msg and "frame" in msg
    rc, msg = config([[0, 0, 64, 64, 64, 60, 0, 5]])
    assert rc == lib.SS_ERR_INVALID and "tile 0" in msg and "canvas" in msg
    assert L.ss_slice_config(None, None, 1, 96, 160, 64, 64, 8, 0, 0, 1.0, 0.0, 0.0) == lib.SS_ERR_INVALID and b"null tile table" in L.ss_last_error(None)
    # the launches: arguments first, then the context
    one = C.c_void_p(16)
    assert L.ss_slice_letterbox_batch(None, None, 1, 0, 480, one, 0, 114) == lib.SS_ERR_INVALID and b"null pointer" in L.ss_last_error(None)
    for args, word in (((one, 70000, 0, 480, one, 0, 114), b"batch"), ((one, 1, 0, 480, one, 4, 114), b"dst_flags"), ((one, 1, 0, 480, one, 0, 256), b"pad_value"),
                       ((one, 1, 0, 480, C.c_void_p(18), 0, 114), b"aligned"), ((one, 1, 0, 480, one, 0, 114), b"null context")):
        assert L.ss_slice_letterbox_batch(None, *args) == lib.SS_ERR_INVALID and word in L.ss_last_error(None), word
    good = dict(rows=one, counts=one, batch=1, ld=6, ts=768, fs=5376, mode=1, metric=1, thr=0.5, ag=0, cap=128, out=one, old=6, ofs=768, cnt=one, src=one, sfs=128)
    for kw, word in ((dict(rows=None), b"null pointer"), (dict(batch=-1), b"batch"), (dict(ld=5), b"row_stride"), (dict(mode=2), b"mode"), (dict(metric=-1), b"metric"),
                     (dict(thr=float("inf")), b"finite"), (dict(ag=2), b"agnostic"), (dict(cap=0), b"out_cap"), (dict(cap=8193), b"out_cap"), (dict(old=4), b"out_row_stride"),
                     (dict(batch=2, ofs=100), b"overlap"), ({}, b"null context")):
        assert L.ss_slice_merge(None, *{**good, **kw}.values()) == lib.SS_ERR_INVALID and word in L.ss_last_error(None), word
    assert L.ss_slice_nms_geom(None, None, 1) == lib.SS_ERR_INVALID and L.ss_slice_nms_geom(None, one, 1) == lib.SS_ERR_INVALID


def test_cli_flags():
    assert cli.slice_kwargs({}) == {}
    kw = cli.slice_kwargs({"slice": [640, 512], "slice_overlap": 0.3, "slice_merge": "nms", "slice_metric": "iou", "slice_thr": 0.6, "no_slice_full": True})
    assert kw == dict(slice_hw=(640, 512), slice_overlap=0.3, slice_full=False, slice_merge="nms", slice_metric="iou", slice_thr=0.6)
    for argv in (["--slice", "0", "64"], ["--slice-thr", "0.3"], ["--no-slice-full"], ["--slice", "64", "64", "--slice-overlap", "1.0"],
                 ["--slice", "64", "64", "--slice-merge", "wbf"], ["--slice", "64"], ["--slice", "64", "64", "--weights", "yolov8n-seg.pt"],
                 ["--slice", "64", "64", "--track", "--tracker", "botsort", "--with-reid", "--reid-model", "auto"]):
        with pytest.raises(SystemExit) as ei:
            cli.main(argv)
        assert ei.value.code == 2, argv
