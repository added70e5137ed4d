"""The analytics stage without a GPU (docs/ZONES.md): hand-made cases of tests/zones_ref.py with known answers, the reference's group
invariance, the library's argument checks, the colour table, the blend formula, the CLI flags and the `_zones.json` document."""
import ctypes as C
import json

import numpy as np
import pytest

from strongsort_yolo_amd import cli, lib, zones
from tests import zones_ref, zones_scenes
from tests.zones_ref import ZoneRef

LINE = [50, 0, 50, 100]             # a -> b straight down x = 50: s >= 0 (side 1, "in") is x <= 50
SQUARE = [[0, 0], [100, 0], [100, 100], [0, 100]]
# a U of 32 vertices: the square with a notch x 40..60, y 40..100 cut in from the y = 100 edge, and 24 collinear vertices on the y = 0 edge
U32 = [[0, 0]] + [[4 * k, 0] for k in range(1, 25)] + [[100, 0], [100, 100], [60, 100], [60, 40], [40, 40], [40, 100], [0, 100]]


def at(x, y, tid, cls=0):
    """A box whose bottom-centre AND centre-free anchors are exact: bottom anchor (x, y)."""
    return [x - 5, y - 20, x + 5, y, tid, cls, 0.9, 0]


def centred(x, y, tid, cls=0):
    return [x - 5, y - 5, x + 5, y + 5, tid, cls, 0.9, 0]


def run(ref, frames):
    """frames: a list of row lists (stream 0) -> the reference's outputs for the whole list as one group call per frame."""
    outs = []
    for fr in frames:
        rows, counts = np.zeros((1, 1, 256, 8), np.float32), np.zeros((1, 1), np.int32)
        rows[0, 0, :len(fr)], counts[0, 0] = np.asarray(fr, np.float32).reshape(-1, 8), len(fr)
        outs.append(ref.update_group(rows, counts))
    return outs


def test_u32_is_what_the_docstring_says():
    assert len(U32) == 32 and len({tuple(p) for p in U32}) == 32


def test_one_crossing_out_then_back_in():
    ref = ZoneRef(lines=[LINE])
    o = run(ref, [[at(30, 50, 1, 2)], [at(70, 50, 1, 2)], [at(30, 50, 1, 3)]])
    assert [int(x["events"][0, 0, 0]) for x in o] == [0, 1 << 16, 1 << 0]
    assert o[1]["line_totals"][0, 0, 0].tolist() == [0, 1] and o[2]["line_totals"][0, 0, 0].tolist() == [1, 1]
    t = ref.totals()
    assert t["line_class"][0, 1, 2] == 1 and t["line_class"][0, 0, 3] == 1 and t["line_class"].sum() == 2       # the class of the row at f1


def test_a_path_beyond_the_segments_end_does_not_count():
    ref = ZoneRef(lines=[LINE])
    o = run(ref, [[at(30, 150, 1)], [at(70, 150, 1)], [at(30, 99, 1)], [at(70, 99, 1)]])
    assert int(o[1]["events"][0, 0, 0]) == 0                      # meets x = 50 at y = 150, beyond b = (50, 100)
    assert int(o[2]["events"][0, 0, 0]) == 0                      # (70, 150) -> (30, 99) meets x = 50 at y = 124.5: still beyond b
    assert int(o[3]["events"][0, 0, 0]) == 1 << 16                # at y = 99 it is on the segment
    assert ref.totals()["line_totals"][0].tolist() == [0, 1]


def test_anchor_exactly_on_the_line_and_a_stationary_track():
    ref = ZoneRef(lines=[LINE])
    o = run(ref, [[at(30, 50, 1), at(70, 20, 2)], [at(50, 50, 1), at(70, 20, 2)], [at(70, 50, 1), at(70, 20, 2)]])
    assert zones_ref.side(100.0, 0.0, 100.0, 200.0, 100.0, 100.0) == 1          # s == 0 is side 1
    assert [int(x["events"][0, 0, 0]) for x in o] == [0, 0, 1 << 16]           # onto the line: still side 1; off it: outward
    assert [int(x["events"][0, 0, 1]) for x in o] == [0, 0, 0]                 # the stationary track never crosses


def test_gap_of_max_gap_counts_and_one_more_does_not():
    for gap, want in ((3, 1 << 16), (4, 0)):
        ref = ZoneRef(lines=[LINE], zones=[SQUARE], max_gap=3)
        o = run(ref, [[at(30, 50, 1)]] + [[]] * (gap - 1) + [[at(70, 50, 1)]])
        assert int(o[-1]["events"][0, 0, 0]) == want
        # after expiry the reappearance is a first appearance: inside the square it is a second entry, and no exit was counted
        assert ref.totals()["entries"][0] == (1 if want else 2) and ref.totals()["exits"][0] == 0
        assert int(o[-1]["dwell"][0, 0, 0]) == (gap + 1 if want else 1)


def test_concave_zone_with_the_anchor_on_a_vertex_and_on_horizontal_edges():
    ref = ZoneRef(zones=[U32], anchor="centre")
    pts = [(50, 20, 1), (50, 70, 0), (20, 70, 1), (40, 40, 0), (50, 40, 0), (20, 100, 0), (50, 0, 1), (0, 0, 1), (100, 50, 0)]
    o = run(ref, [[centred(x, y, i + 1) for i, (x, y, _) in enumerate(pts)]])[0]
    assert o["inside"][0, 0, :len(pts)].tolist() == [w for _, _, w in pts]
    assert int(o["occupancy"][0, 0, 0]) == sum(w for _, _, w in pts)


def test_enter_exit_and_dwell_with_a_track_first_seen_inside():
    ref = ZoneRef(zones=[SQUARE])
    o = run(ref, [[at(50, 50, 1)], [at(60, 50, 1)], [at(150, 50, 1)], [at(50, 50, 1), at(20, 20, 2)], []])
    assert [int(x["dwell"][0, 0, 0]) for x in o[:4]] == [1, 2, 0, 1]
    assert [int(x["occupancy"][0, 0, 0]) for x in o] == [1, 1, 0, 2, 0]
    t = ref.totals()
    assert (t["entries"][0], t["exits"][0], t["dwell_sum"][0], t["longest"][0], t["peak"][0]) == (3, 1, 2, 2, 2)
    # both tracks vanish while inside: that is no exit


def test_duplicate_id_non_finite_row_and_id_zero():
    ref = ZoneRef(zones=[SQUARE], heat="anchor", cell=8, frame_hw=(120, 160))
    fr = [at(50, 50, 7), at(60, 60, 7), [np.nan, 0, 10, 10, 8, 0, .5, 0], [0, 0, np.inf, 10, 9, 0, .5, 0], at(20, 20, 0), at(20, 20, -3)]
    o = run(ref, [fr])[0]
    assert o["inside"][0, 0, :6].tolist() == [1, 0, 0, 0, 0, 0] and o["dwell"][0, 0, :6].tolist() == [1, 0, 0, 0, 0, 0]
    assert int(o["occupancy"][0, 0, 0]) == 1 and int(ref.heatmap().sum()) == 1 and ref.heatmap()[50 >> 3, 50 >> 3] == 1


def test_heat_box_across_every_border_and_outside():
    ref = ZoneRef(heat="box", cell=8, frame_hw=(20, 30))               # grid 3 x 4: w is no multiple of the cell
    boxes = [[-5.5, -3.0, 4.2, 6.7], [25.5, 15.2, 40.0, 30.0], [40.0, 5.0, 50.0, 10.0], [-10.0, -10.0, -1.0, -1.0], [8.0, 8.0, 16.0, 16.0],
             [10.0, -4.0, 12.0, 3.0], [-3.0, 18.0, 2.0, 25.0]]
    o = run(ref, [[b + [i + 1, 0, .9, 0] for i, b in enumerate(boxes)]])[0]
    want = np.zeros((3, 4), np.int32)
    want[0, 0] += 1                    # the top-left corner: pixels x 0..4, y 0..6
    want[1:3, 3] += 1                  # the bottom-right corner: x 25..29, y 15..19
    want[1, 1] += 1                    # x 8..15, y 8..15: ceil(16) - 1 = 15 stays in cell 1
    want[0, 1] += 1                    # over the top border: x 10..11, y 0..2
    want[2, 0] += 1                    # over the left and bottom borders: x 0..1, y 18..19
    assert ref.heatmap().tolist() == want.tolist() and o["heat_frames"][0, 0].tolist() == want.tolist() and int(o["heat_max"][0, 0]) == 1


def test_heat_anchor_sums_to_the_counted_rows():
    rng = np.random.default_rng(5)
    ref = ZoneRef(heat="anchor", cell=4, frame_hw=(120, 160))
    n = 0
    for f in range(6):
        fr = [at(float(rng.uniform(6, 150)), float(rng.uniform(21, 119)), i + 1) for i in range(20)] + [at(30, 30, 3)]      # id 3 twice
        run(ref, [fr])
        n += 20
    assert int(ref.heatmap().sum()) == n and ref.totals()["heat_max"] == int(ref.heatmap().max())


@pytest.mark.parametrize("group", [1, 7, 32])
def test_the_reference_does_not_depend_on_the_grouping(group):
    rows, counts = zones_scenes.walkers(11, 64, 2, 30, births=2, life=9)
    lines, zs = zones_scenes.geometry()
    kw = dict(lines=lines, zones=zs, max_gap=4, heat="box", frame_hw=zones_scenes.HW, n_streams=2)
    whole, parts = ZoneRef(**kw), ZoneRef(**kw)
    a = [whole.update_group(rows[g:g + 64], counts[g:g + 64]) for g in range(0, 64, 64)]
    b = [parts.update_group(rows[g:g + group], counts[g:g + group]) for g in range(0, 64, group)]
    for k in a[0]:
        assert np.concatenate([x[k] for x in b]).tobytes() == a[0][k].tobytes(), k
    for s in range(2):
        ta, tb = whole.totals(s), parts.totals(s)
        assert all(np.asarray(ta[k]).tobytes() == np.asarray(tb[k]).tobytes() for k in ta)
        assert ta["line_totals"].sum() > 0 and ta["exits"].sum() > 0        # the scene exercises what it compares


# ---- the library's argument checks: no context, no device ------------------------------------------------------------------------
def _create(cfg=None, lines=(), zs=()):
    L = lib.load()
    c = lib.ss_zone_config(*(cfg or (1, 30, 80, 0, 3, 0, 0)))
    ln = np.asarray(lines, np.int32).reshape(-1, 4)
    xy = np.concatenate([np.asarray(z, np.int32).reshape(-1, 2) for z in zs], 0) if zs else np.zeros((0, 2), np.int32)
    off = np.concatenate([[0], np.cumsum([len(z) for z in zs])]).astype(np.int32)
    pi = C.POINTER(C.c_int)
    rc = L.ss_zone_create(None, C.byref(c), ln.ctypes.data_as(pi), len(ln), xy.ctypes.data_as(pi), off.ctypes.data_as(pi), len(zs))
    return rc, L.ss_last_error(None).decode()


def test_library_refuses_bad_arguments_without_a_context():
    L = lib.load()
    assert (L.ss_zone_max_lines(), L.ss_zone_max_zones(), L.ss_zone_max_vertices(), L.ss_zone_max_live()) == (16, 16, 32, 1024)
    rc, msg = _create(lines=[LINE])
    assert rc == lib.SS_ERR_INVALID and "null context" in msg                 # good arguments: only the context is missing
    for kw, word in ((dict(lines=[LINE] * 17), "17 lines"), (dict(zs=[SQUARE[:2]]), "zone 0: 2 vertices"), (dict(zs=[SQUARE, SQUARE[:2]]), "zone 1"),
                     (dict(lines=[LINE, [0, 0, 40000, 5]]), "line 1: coordinate 40000"), (dict(lines=[[3, 3, 3, 3]]), "line 0"),
                     (dict(zs=[[[0, 0], [5, -40000], [9, 9]]]), "zone 0: coordinate -40000"), (dict(zs=[SQUARE] * 17), "17 zones"),
                     (dict(cfg=(1, 0, 80, 0, 3, 0, 0)), "max_gap 0"), (dict(cfg=(1, 33, 80, 0, 3, 0, 0)), "max_gap 33"),
                     (dict(cfg=(1, 30, 129, 0, 3, 0, 0)), "n_classes 129"), (dict(cfg=(2, 30, 80, 0, 3, 0, 0)), "anchor"),
                     (dict(cfg=(1, 30, 80, 2, 0, 300, 300)), "90000 cells"), (dict(cfg=(1, 30, 80, 1, 7, 64, 64)), "heat_cell_log2 7")):
        rc, msg = _create(**kw)
        assert rc == lib.SS_ERR_INVALID and word in msg and "null context" not in msg, (kw, msg)
    assert L.ss_zone_update_group(None, 0, None, None, None, None, None, None, None, None, None) == lib.SS_ERR_INVALID
    assert "n_frames 0" in L.ss_last_error(None).decode()
    assert L.ss_zone_update_group(None, 33, None, None, None, None, None, None, None, None, None) == lib.SS_ERR_INVALID
    assert L.ss_zone_heat_blend(None, None, None, 1, 0, 4, 4, 12, None, 0, None, 0, 128) == lib.SS_ERR_INVALID
    assert "null pointer" in L.ss_last_error(None).decode()
    assert L.ss_zone_reset(None, 0) == lib.SS_ERR_INVALID and L.ss_zone_destroy(None) == lib.SS_ERR_INVALID
    assert L.ss_zone_get_totals(None, 0, None, None, None, None, None, None, None, None, None) == lib.SS_ERR_INVALID


def test_config_refuses_by_name_what_the_library_refuses():
    for kw, word in ((dict(lines=[LINE] * 17), "17 lines"), (dict(zones=[SQUARE[:2]]), "zone 0"), (dict(lines=[[0, 0, 40000, 1]]), "line 0"),
                     (dict(max_gap=0), "max_gap 0"), (dict(max_gap=33), "max_gap 33"), (dict(heat="box", heat_cell=3), "heat_cell 3")):
        with pytest.raises(ValueError, match=word):
            zones.ZoneConfig(**kw).validate()
    with pytest.raises(ValueError, match="90000 cells"):
        zones.ZoneConfig(heat="box", heat_cell=1).validate((300, 300))


# ---- colour table and blend ---------------------------------------------------------------------------------------------------
def test_colormap_bytes():
    t = zones.colormap()
    assert t.dtype == np.uint8 and t.shape == (256, 3) and t.tobytes() == zones_ref.colormap().tobytes()
    assert t[0].tolist() == [127, 0, 0] and t[255].tolist() == [0, 0, 127] and t[64].tolist() == [255, 128, 0] and t[128].tolist() == [125, 255, 129]
    for i in range(256):                                                         # the formula, once more, in plain integers
        assert t[i].tolist() == [min(max(382 - abs(4 * i - c), 0), 255) for c in (255, 510, 765)]


def test_blend_formula_at_its_ends():
    rng = np.random.default_rng(2)
    frame = rng.integers(0, 256, (23, 37, 3), dtype=np.uint8)
    heat = rng.integers(0, 4, (6, 10)).astype(np.int32)
    lut = zones_ref.colormap()
    assert zones_ref.blend(frame, heat, 3, 2, lut, 0).tobytes() == frame.tobytes()
    full = zones_ref.blend(frame, heat, 3, 2, lut, 256)
    v = np.kron(heat, np.ones((4, 4), np.int32))[:23, :37]
    assert (full[v > 0] == lut[(v[v > 0] * 255 + 1) // 3]).all() and (full[v == 0] == frame[v == 0]).all()
    half = zones_ref.blend(frame, heat, 3, 2, lut, 77)
    y, x = np.argwhere(v > 0)[0]
    assert half[y, x].tolist() == [(int(frame[y, x, c]) * 179 + int(lut[(v[y, x] * 255 + 1) // 3][c]) * 77 + 128) >> 8 for c in range(3)]
    assert zones_ref.blend(frame, np.zeros_like(heat), 0, 2, lut, 256).tobytes() == frame.tobytes()      # an all-zero grid, max 0


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------
def test_cli_parsing():
    assert zones.parse_line("1,2,3,-4") == [1, 2, 3, -4]
    assert zones.parse_zone("0,0,10,0,10,10") == [[0, 0], [10, 0], [10, 10]]
    for fn, text, word in ((zones.parse_line, "1,2,3", "four numbers"), (zones.parse_line, "1,2,1,2", "same point"), (zones.parse_line, "1,2,x,2", "integer"),
                           (zones.parse_line, "0,0,40000,1", "40000"), (zones.parse_zone, "0,0,1,1", "3 to 32"), (zones.parse_zone, "0,0,1,1,2", "3 to 32"),
                           (zones.parse_zone, ",".join(["1,1"] * 33), "3 to 32")):
        with pytest.raises(ValueError, match=word):
            fn(text)


@pytest.mark.parametrize("argv,word", [(["--line", "1,2,3"], "four numbers"), (["--zone", "0,0,5,5"], "3 to 32"), (["--line", "0,0,40000,1"], "40000"),
                                       (["--line", "0,0,1,1", "--zone-gap", "33"], "max_gap 33"), (["--heatmap", "box", "--heat-cell", "3"], "heat_cell 3"),
                                       (["--heatmap", "box", "--heat-alpha", "1.5"], "heat-alpha"), (["--line", "0,0,1,1"] * 17, "17 lines")])
def test_cli_refuses_bad_geometry_at_argument_time(argv, word, capsys):
    with pytest.raises(SystemExit):
        cli.main(["--track"] + argv)
    assert word in capsys.readouterr().err


def test_cli_flags_without_track_print_the_hint(tmp_path, capsys):
    from tests.test_cli_host import StubModel
    out = cli.process_video({"source": "synthetic:3", "track": False, "count": False, "outdir": str(tmp_path), "lines": [LINE]}, StubModel())
    assert out["frames"] == 1 and "work only when objects are tracking" in capsys.readouterr().out
    assert not (tmp_path / "synthetic:3_zones.json").exists()


def test_zones_json_schema_from_the_reference(tmp_path):
    rows = zones_scenes.labels_rows()
    path = tmp_path / "seq_labels.txt"
    from strongsort_yolo_amd import gsi, moteval
    gsi.write_labels(str(path), rows)
    back = moteval.read_labels(str(path))
    lines, zs = zones_scenes.geometry(2, 2, 8)
    cfg = zones.ZoneConfig(lines=lines, zones=zs, max_gap=5, n_classes=5)
    ref = ZoneRef(lines=lines, zones=zs, max_gap=5, n_classes=5)
    F = int(back[:, 0].max()) + 1
    buf, cnt = np.zeros((F, 1, 256, 8), np.float32), np.zeros((F, 1), np.int32)
    for r in back:
        f = int(r[0])
        buf[f, 0, cnt[f, 0]] = [r[2], r[3], r[4], r[5], r[1], r[7], r[6], 0]
        cnt[f, 0] += 1
    ref.update_group(buf, cnt)
    doc = zones.write_summary(str(tmp_path / "seq_zones.json"), ref.totals(), cfg, {0: "person", 2: "car"})
    assert json.load(open(tmp_path / "seq_zones.json")) == doc
    assert set(doc) == {"frames", "anchor", "max_gap", "lines", "zones"} and doc["frames"] == F and len(doc["lines"]) == 2 and len(doc["zones"]) == 2
    for l in doc["lines"]:
        assert set(l) == {"line", "in", "out", "in_by_class", "out_by_class"}
        assert sum(l["in_by_class"].values()) == l["in"] and sum(l["out_by_class"].values()) == l["out"]
        assert all(k in ("person", "1", "car", "3", "4") for k in l["in_by_class"])
    for z in doc["zones"]:
        assert set(z) == {"polygon", "entries", "exits", "peak_occupancy", "mean_dwell", "longest_dwell"}
        assert (z["mean_dwell"] is None) == (z["exits"] == 0) and z["entries"] >= z["exits"]
    assert sum(l["in"] + l["out"] for l in doc["lines"]) > 0 and sum(z["exits"] for z in doc["zones"]) > 0
