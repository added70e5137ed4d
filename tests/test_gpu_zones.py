"""The analytics stage on the device (csrc/ss_zone.hip, docs/ZONES.md): every output array and every total equals tests/zones_ref.py byte
for byte, at the caps, across group boundaries, under capture, on a tracker's own device rows, through the blend and through the CLI."""
import json

import numpy as np
import pytest
import torch

from strongsort_yolo_amd import cli, lib, zones
from strongsort_yolo_amd.engine import OCSortEngine, TrackerEngine
from tests import zones_ref, zones_scenes
from tests.zones_ref import ZoneRef

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HW = zones_scenes.HW


def _pair(S, lines, zs, **kw):
    """A ZoneCounter on a fresh engine and the reference, configured alike."""
    eng = TrackerEngine(None, S, 0)
    heat, cell = kw.get("heat"), kw.get("cell", 8)
    cfg = zones.ZoneConfig(lines=lines, zones=zs, anchor=kw.get("anchor", "bottom"), max_gap=kw.get("max_gap", 30), n_classes=kw.get("n_classes", 5),
                           heat=heat, heat_cell=cell)
    zc = zones.ZoneCounter(cfg, eng, frame_hw=kw.get("hw", HW) if heat else None)
    ref = ZoneRef(lines=lines, zones=zs, anchor=cfg.anchor, max_gap=cfg.max_gap, n_classes=cfg.n_classes, heat=heat, cell=cell,
                  frame_hw=kw.get("hw", HW), n_streams=S)
    return eng, zc, ref


def _same_outputs(got, want, what, streams=None):
    for k in got:
        g, w = (got[k], want[k]) if streams is None else (got[k][:, streams], want[k][:, streams])
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: {k} differs in {int((g != w).sum())} places"


def _same_totals(zc, ref, S, heat, what, streams=None):
    for s in range(S) if streams is None else streams:
        tg, tr = zc.totals(s), ref.totals(s)
        assert set(tg) == set(tr)
        for k in tr:
            assert np.asarray(tg[k]).astype(np.int64).tobytes() == np.asarray(tr[k]).astype(np.int64).tobytes(), f"{what}: total {k} of stream {s}"
        if heat:
            assert zc.heatmap(s).tobytes() == ref.heatmap(s).tobytes(), f"{what}: heat grid of stream {s}"


def _run(zc, ref, rows, counts, group, what, S, heat):
    for g in range(0, len(counts), group):
        got, want = zc.update_group(rows[g:g + group], counts[g:g + group]), ref.update_group(rows[g:g + group], counts[g:g + group])
        _same_outputs(got, {k: want[k] for k in got}, f"{what}, frames from {g}")
    zc.eng.check_errors()
    _same_totals(zc, ref, S, heat, what)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("F", [1, 5, 32])
def test_every_output_and_total_equals_the_reference(S, F):
    lines, zs = zones_scenes.geometry()
    eng, zc, ref = _pair(S, lines, zs, max_gap=4, heat="box")
    rows, counts = zones_scenes.walkers(100 + 10 * S + F, 2 * F + 1, S, 30, births=2, life=9)
    _run(zc, ref, rows, counts, F, f"S {S} F {F}", S, True)          # two full groups and a rest: the state crosses the calls
    t = ref.totals(0)
    assert F == 1 or (t["line_totals"].sum() > 0 and t["entries"].sum() > 0)
    eng.close()


def test_a_frame_of_256_rows_with_the_centre_anchor_and_anchor_heat():
    lines, zs = zones_scenes.geometry(4, 4, 7, seed=3)
    eng, zc, ref = _pair(1, lines, zs, anchor="centre", heat="anchor", cell=4, max_gap=2)
    rows, counts = zones_scenes.walkers(7, 6, 1, 256, dirt=False, p_miss=0.0)
    rows2, counts2 = zones_scenes.walkers(8, 6, 1, 300, dirt=True)        # more than fit: the first 256 rows of each frame
    assert counts.max() == 256 and counts2.max() == 256
    _run(zc, ref, np.concatenate([rows, rows2]), np.concatenate([counts, counts2]), 6, "256 rows", 1, True)
    eng.close()


def test_sixteen_lines_and_sixteen_zones_of_32_vertices_at_cell_1():
    lines, zs = zones_scenes.geometry(16, 16, 32, seed=5)
    eng, zc, ref = _pair(2, lines, zs, heat="box", cell=1, hw=(48, 61), max_gap=32)
    rows, counts = zones_scenes.walkers(9, 10, 2, 50, hw=(48, 61))
    _run(zc, ref, rows, counts, 5, "caps", 2, True)
    assert ref.totals(0)["line_totals"].min() >= 0 and (ref.totals(0)["line_totals"].sum(1) > 0).sum() >= 8
    eng.close()


def test_ids_that_collide_in_the_table():
    lines, zs = zones_scenes.geometry()
    eng, zc, ref = _pair(1, lines, zs, max_gap=3)
    rows, counts = zones_scenes.walkers(12, 24, 1, 70, id_step=lib.load().ss_zone_max_live(), id0=1024, births=3, life=5)
    _run(zc, ref, rows, counts, 8, "colliding ids", 1, False)
    eng.close()


def test_churn_of_more_ids_than_the_table_holds_reuses_its_slots():
    lines, zs = zones_scenes.geometry()
    eng, zc, ref = _pair(1, lines, zs, max_gap=3)
    rows, counts = zones_scenes.walkers(13, 64, 1, 20, births=22, life=6)
    assert len(np.unique(rows[..., 4])) > 1100 + 1
    _run(zc, ref, rows, counts, 32, "churn", 1, False)                  # check_errors inside: the live set stays far below the cap
    eng.close()


def test_1025_live_ids_report_capacity_and_leave_the_other_stream_alone():
    lines, zs = zones_scenes.geometry()
    eng, zc, ref = _pair(2, lines, zs, max_gap=32)
    rows, counts = zones_scenes.walkers(14, 5, 2, 30)
    ids = np.arange(1, 1026, dtype=np.float32).reshape(5, 205)           # stream 0: 205 new ids a frame, all alive at the fifth
    rows[:, 0] = 0
    rows[:, 0, :205, 0:4] = [10, 10, 30, 50]
    rows[:, 0, :205, 4] = ids
    counts[:, 0] = 205
    got, want = zc.update_group(rows, counts), ref.update_group(rows, counts)
    _same_outputs(got, {k: want[k] for k in got}, "beside a full stream", streams=[1])
    _same_totals(zc, ref, 2, False, "beside a full stream", streams=[1])
    with pytest.raises(lib.SSError) as ei:
        eng.check_errors()
    assert ei.value.code == lib.SS_ERR_CAPACITY and "stream 0" in str(ei.value)
    zc.reset()
    eng.check_errors()
    ref.reset()
    rows, counts = zones_scenes.walkers(15, 6, 2, 30)
    _run(zc, ref, rows, counts, 6, "after reset", 2, False)
    eng.close()


def test_one_group_equals_single_frames_equals_5_plus_27():
    lines, zs = zones_scenes.geometry()
    rows, counts = zones_scenes.walkers(16, 32, 2, 40, births=2, life=7)
    eng = TrackerEngine(None, 2, 0)
    cfg = zones.ZoneConfig(lines=lines, zones=zs, max_gap=3, n_classes=5, heat="box")
    runs = []
    for cuts in ([32], [1] * 32, [5, 27]):
        zc = zones.ZoneCounter(cfg, eng, frame_hw=HW)                   # replaces the state before it
        outs, g = [], 0
        for n in cuts:
            outs.append(zc.update_group(rows[g:g + n], counts[g:g + n]))
            g += n
        tot = [zc.totals(s) for s in range(2)]
        runs.append(({k: np.concatenate([o[k] for o in outs]) for k in outs[0]}, tot, [zc.heatmap(s) for s in range(2)]))
    for other in runs[1:]:
        _same_outputs(other[0], runs[0][0], "cut differently")
        for s in range(2):
            assert all(np.asarray(other[1][s][k]).tobytes() == np.asarray(runs[0][1][s][k]).tobytes() for k in runs[0][1][s])
            assert other[2][s].tobytes() == runs[0][2][s].tobytes()
    eng.close()


def test_captured_update_equals_the_plain_launch():
    lines, zs = zones_scenes.geometry()
    eng, zc, ref = _pair(2, lines, zs, max_gap=4, heat="box")
    rows, counts = zones_scenes.walkers(17, 16, 2, 30)
    G = 8
    names = zones.OUTPUTS
    d_rows, d_counts = torch.zeros(G, 2, 256, 8, device=DEV), torch.full((G, 2), -1, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        eng.use_current_stream()
        zc.update_group_device(d_rows, d_counts, G, names)              # warm-up (every stream sits it out): the buffers exist before the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):                      # one linear capture: the one launch
            eng.use_current_stream()
            out = zc.update_group_device(d_rows, d_counts, G, names)
    torch.cuda.synchronize(DEV)
    eng.use_current_stream()
    for g in range(0, 16, G):
        d_rows.copy_(torch.from_numpy(rows[g:g + G])); d_counts.copy_(torch.from_numpy(counts[g:g + G]))
        torch.cuda.synchronize(DEV)
        graph.replay()
        torch.cuda.synchronize(DEV)
        want = ref.update_group(rows[g:g + G], counts[g:g + G])
        got = {k: v.cpu().numpy().view(want[k].dtype) for k, v in out.items()}
        _same_outputs(got, want, f"replayed group at {g}")
    eng.check_errors()
    _same_totals(zc, ref, 2, True, "replayed")
    del graph
    eng.close()


def test_rows_of_the_ocsort_engine_go_straight_in():
    from tests.ocsort_scenes import box
    S, F = 2, 12
    oc = OCSortEngine(None, S, 0)
    rng = np.random.default_rng(18)
    dets, nd = np.zeros((F, S, 128, 6), np.float32), np.zeros((F, S), np.int32)
    for s in range(S):
        x0 = rng.uniform(40, 50, 10)                                     # slow walkers in rows of their own: odd ones go right over x = 60, even ones left over it
        for f in range(F):
            d = np.asarray([box(x0[i] + (2 + 0.3 * i) * f if i % 2 else x0[i] + 25 - (2 + 0.3 * i) * f, 5 + 11 * i, 14, 10, 0.9, i % 3) for i in range(10)], np.float32)
            dets[f, s, :10], nd[f, s] = d, 10
    out, nout = torch.zeros(F, S, 256, 8, device=DEV), torch.zeros(F, S, dtype=torch.int32, device=DEV)
    oc.update_group(F, torch.from_numpy(dets).to(DEV), torch.from_numpy(nd).to(DEV), None, None, out, nout)
    lines, zs = [[60, 0, 60, 120], [100, 119, 100, 0]], [zones_scenes.star(80, 60, 50, 20, 12)]
    cfg = zones.ZoneConfig(lines=lines, zones=zs, max_gap=5, n_classes=3)
    zc = zones.ZoneCounter(cfg, oc)
    dev_out = {k: v.cpu().numpy() for k, v in zc.update_group_device(out, nout, F).items()}      # the tracker's tensors, in place
    oc.check_errors()
    dev_tot = zc.totals(0), zc.totals(1)
    h_rows, h_counts = out.cpu().numpy(), nout.cpu().numpy()
    assert h_counts.sum() > 100
    zc.reset()
    host = zc.update_group(h_rows, h_counts)
    ref = ZoneRef(lines=lines, zones=zs, max_gap=5, n_classes=3, n_streams=S)
    want = ref.update_group(h_rows, h_counts)
    for k in dev_out:
        assert dev_out[k].tobytes() == host[k].tobytes() == want[k].tobytes(), k
    for s in range(S):
        assert all(np.asarray(dev_tot[s][k]).tobytes() == np.asarray(zc.totals(s)[k]).tobytes() for k in dev_tot[s])
    assert ref.totals(0)["line_totals"].sum() > 0
    oc.close()


# ---- blend -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("alpha", [0, 77, 256])
def test_blend_equals_the_numpy_formula(batch, alpha):
    h, w = 23, 37                                                       # 111 bytes a row: no multiple of 16, so every row starts at another alignment
    rng = np.random.default_rng(20 + batch)
    eng = TrackerEngine(None, 1, 0)
    lut = zones.colormap()
    for cell, stride, mx in ((4, 3 * w, None), (1, 3 * w + 9, None), (8, 3 * w + 16, 1), (4, 3 * w, 0)):
        zc = zones.ZoneCounter(zones.ZoneConfig(heat="box", heat_cell=cell), eng, frame_hw=(h, w))
        gh, gw = zc.grid
        k = cell.bit_length() - 1
        heat = (rng.integers(0, 6, (batch, gh, gw)) * (rng.random((batch, gh, gw)) < 0.6)).astype(np.int32)
        if mx is not None:
            heat = np.minimum(heat, mx)                                 # heat max 1, and the all-zero grid
        maxes = heat.reshape(batch, -1).max(1).astype(np.int32)
        buf = rng.integers(0, 256, (batch, h, stride), dtype=np.uint8)
        d_buf = torch.from_numpy(buf).to(DEV)
        frames = d_buf[:, :, :3 * w].unflatten(2, (w, 3))               # row_stride > 3 w: the padding must come back untouched
        zc.blend(frames, torch.from_numpy(np.ascontiguousarray(heat)).to(DEV), torch.from_numpy(maxes).to(DEV), alpha)
        got = d_buf.cpu().numpy()
        want = buf.copy()
        for b in range(batch):
            want[b, :, :3 * w] = zones_ref.blend(buf[b, :, :3 * w].reshape(h, w, 3), heat[b], maxes[b], k, lut, alpha).reshape(h, 3 * w)
        assert got.tobytes() == want.tobytes(), (cell, stride, mx, int((got != want).sum()))
    # the stream's own cumulative grid, one grid for every frame of the batch
    rows, counts = zones_scenes.walkers(21, 4, 1, 20, hw=(h, w))
    zc.update_group(rows, counts)
    buf = rng.integers(0, 256, (batch, h, w, 3), dtype=np.uint8)
    d = torch.from_numpy(buf).to(DEV)
    zc.blend(d, alpha=alpha)
    grid, m = zc.heatmap(0), zc.totals(0)["heat_max"]
    assert m == grid.max() > 0
    assert d.cpu().numpy().tobytes() == np.stack([zones_ref.blend(buf[b], grid, m, 2, lut, alpha) for b in range(batch)]).tobytes()
    eng.close()


# ---- CLI -------------------------------------------------------------------------------------------------------------------------------
def test_cli_run_writes_what_replay_gives_on_its_own_labels(tmp_path):
    from strongsort_yolo_amd import moteval
    from strongsort_yolo_amd.yolo import YOLO
    argv_lines, argv_zones = ["320,0,320,480", "0,240,640,240"], ["100,100,540,100,540,380,100,380"]
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="ocsort")
    args = {"source": "synthetic:12", "track": True, "count": False, "tracker": "ocsort", "batch": 4, "random_init": True, "outdir": str(tmp_path),
            "lines": [zones.parse_line(t) for t in argv_lines], "zones": [zones.parse_zone(t) for t in argv_zones], "heatmap": "box",
            "save": str(tmp_path / "out.npy")}
    out = cli.process_video(args, model=model)
    assert out["frames"] == 12
    name = "synthetic:12"
    doc = json.load(open(tmp_path / f"{name}_zones.json"))
    assert doc == out["zones"] and np.load(tmp_path / "out.npy").shape == (12, 480, 640, 3)
    cfg = cli.zone_config(args, len(model.names))
    labels = moteval.read_labels(str(tmp_path / f"{name}_labels.txt"))
    eng = model.overlay().eng
    tot, heat = zones.replay(labels, cfg, eng, (480, 640))
    # the run ended with the last processed frame; the file's last frame is the last that had a row
    tot["frames"] = doc["frames"]
    assert zones.summary(tot, cfg, model.names) == doc
    assert np.load(tmp_path / f"{name}_heat.npy").tobytes() == heat.tobytes() and (len(labels) == 0 or heat.sum() > 0)
    model.close()
