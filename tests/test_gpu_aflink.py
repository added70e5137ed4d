"""AFLink on the MI355X (csrc/ss_aflink.hip, docs/AFLINK.md) against its CPU restatement (tests/aflink_ref.py), through the C ABI:
the gate and the network inputs byte for byte, the costs within the float bounds of docs/AFLINK.md §5, the matching link for link."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from strongsort_yolo_amd import aflink, cli, lib
from tests import aflink_ref as R
from tests import gsi_ref
from tests.gpu_util import engine

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = json.load(open(os.path.join(GOLD, "aflink_scenes.json")))
TOL = 1e-4                                  # the float-distance tolerance of the project's north star


@pytest.fixture(scope="module")
def model():
    return R.calibrated(SCENES["model_seed"])


@pytest.fixture(scope="module")
def eng(model):
    e = engine(debug=False)
    e.aflink_set_weights(aflink.pack(model))
    yield e
    e.close()


@pytest.fixture(scope="module")
def big(model):
    """The 512-pair set, its float64 costs and the CPU float32 PyTorch costs: computed once, shared, never changed."""
    rows = R.couples(7, 512)
    _, offsets, _, feats = R.tracklets(rows)
    pi, pj = R.gate(offsets, feats)
    x = R.transform(offsets, feats, pi, pj)
    c64, c32 = R.net_costs(model, x), R.net_costs(model, x, torch.float32)
    for a in (x, c64, c32):
        a.setflags(write=False)
    return offsets, feats, pi, pj, x, c64, c32


def _device_and_ref(eng, rows, thr_t=(0, 30), thr_s=75.0):
    _, offsets, _, feats = R.tracklets(rows)
    got = eng.aflink_cost(offsets, feats, thr_t, thr_s, want_inputs=True)
    pi, pj = R.gate(offsets, feats, thr_t, thr_s)
    return got, (pi, pj, R.transform(offsets, feats, pi, pj))


def _same_gate_and_inputs(got, ref, what):
    assert got[0].tolist() == ref[0].tolist() and got[1].tolist() == ref[1].tolist(), f"{what}: pair list"
    assert got[3].dtype == np.float32 and got[3].shape == ref[2].shape and got[3].tobytes() == ref[2].tobytes(), f"{what}: inputs"


def _tracklet(tid, frames, x, y):
    frames = np.asarray(frames, np.float64)
    blk = np.zeros((len(frames), 8))
    blk[:, 0], blk[:, 1], blk[:, 2], blk[:, 3] = frames, tid, x, y
    blk[:, 4], blk[:, 5], blk[:, 6] = blk[:, 2] + 40.0, blk[:, 3] + 90.0, 0.9
    return blk


def _crowd(seed, n):
    """n tracklets of mixed lengths whose ends fall near one another in time and space: many candidates per row."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        ln = int(rng.choice([1, 2, 29, 30, 31, 45, 60]))
        f0 = int(rng.integers(1, 120))
        p = rng.uniform(100, 400, 2)
        path = p + np.cumsum(rng.normal(0, 1.5, (ln, 2)), 0)
        out.append(_tracklet(k + 1, f0 + np.arange(ln), np.abs(path[:, 0]) + 1.0, np.abs(path[:, 1]) + 1.0))
    return np.concatenate(out, 0)


# ---- gate and inputs: byte equality ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_gate_and_inputs_equal_the_restatement(eng, n):
    rows = _crowd(n, n)
    got, ref = _device_and_ref(eng, rows)
    if n == 1:
        assert len(got[0]) == 0 and len(ref[0]) == 0
        return
    assert n < 65 or len(ref[0]) > n, "the crowd should give more candidates than tracklets"
    _same_gate_and_inputs(got, ref, f"n={n}")
    assert np.isfinite(got[2]).all() and ((got[2] >= 0) & (got[2] <= 1)).all()


def test_gate_edges_of_the_frame_gap_and_the_distance(eng):
    t0, t1 = 2, 30
    up = np.nextafter(560.0, np.inf)
    rows = np.concatenate([
        _tracklet(1, np.arange(90, 101), 500.0, 500.0),                     # ends at frame 100 in (500, 500)
        _tracklet(2, 100 + t0 + np.arange(5), 510.0, 500.0),                # gap thrT0: kept
        _tracklet(3, 100 + t0 - 1 + np.arange(5), 510.0, 500.0),            # gap thrT0 - 1: dropped
        _tracklet(4, 100 + t1 - 1 + np.arange(5), 510.0, 500.0),            # gap thrT1 - 1: kept
        _tracklet(5, 100 + t1 + np.arange(5), 510.0, 500.0),                # gap thrT1: dropped
        _tracklet(6, 110 + np.arange(40), 545.0, 560.0),                    # dx = 45, dy = 60: distance exactly thrS, kept
        _tracklet(7, 110 + np.arange(40), 545.0, up),                       # the next y above: dropped
        _tracklet(8, 110 + np.arange(3), 455.0, 440.0),                     # the same distance the other way
    ], 0)
    rows = rows[np.random.default_rng(0).permutation(len(rows))]            # the caller's row order does not matter
    got, ref = _device_and_ref(eng, rows, (t0, t1), 75.0)
    from_first = [int(j) for i, j in zip(ref[0], ref[1]) if i == 0]
    assert from_first == [1, 3, 5, 7], "the restatement keeps exactly the edge cases the definition keeps"
    _same_gate_and_inputs(got, ref, "edges")


def test_tracklets_that_start_on_one_frame_gate_one_way_only(eng):
    # one-row tracklets on one frame have gap 0 both ways; a longer one that starts with them ends later.  Only (first frame, number)
    # rising is a candidate, so no matching of the candidates links in a circle
    rows = np.concatenate([_tracklet(4, [50], 900.0, 900.0), _tracklet(2, [50], 905.0, 900.0), _tracklet(7, [50], 910.0, 905.0),
                           _tracklet(5, [50, 51, 52], 300.0, 300.0), _tracklet(6, [52], 310.0, 300.0), _tracklet(3, [52, 53], 305.0, 300.0)], 0)
    got, ref = _device_and_ref(eng, rows)                                   # numbers by rising id: 2 -> 0, 3 -> 1, 4 -> 2, 5 -> 3, 6 -> 4, 7 -> 5
    assert list(zip(ref[0].tolist(), ref[1].tolist())) == [(0, 2), (0, 5), (2, 5), (3, 1), (3, 4)]
    _same_gate_and_inputs(got, ref, "one frame")


def test_inputs_for_every_length_on_either_side_and_a_constant_column(eng):
    lens = list(itertools.product([1, 29, 30, 31, 60], repeat=2))
    rows = R.couples(3, len(lens), lengths=lens)
    got, ref = _device_and_ref(eng, rows)
    assert len(ref[0]) == len(lens) and (rows[:, 2:4] > 0).all()             # all positive: the padding's zero is the minimum
    short = [k for k, (a, b) in enumerate(lens) if a < 30 or b < 30]
    assert all(ref[2][k].min(axis=(0, 1)).tolist() == pytest.approx([-1.0] * 3, abs=1e-6) for k in short)
    _same_gate_and_inputs(got, ref, "lengths")
    # a constant column over all 60 rows: the divisor is the 1e-5 alone and every value is 0
    rows = np.concatenate([_tracklet(1, np.arange(1, 41), 300.0, np.linspace(200, 260, 40)), _tracklet(2, np.arange(45, 80), 300.0, np.linspace(262, 300, 35))], 0)
    got, ref = _device_and_ref(eng, rows)
    assert len(ref[0]) == 1 and (ref[2][0, :, :, 1] == 0.0).all() and np.abs(ref[2][0, :, :, 2]).max() > 0.9
    _same_gate_and_inputs(got, ref, "constant column")


# ---- costs ---------------------------------------------------------------------------------------------------------------------
# a workgroup of the GEMM owns aflink.BM = 64 rows; a pair is 54, 36, 18 and 6 rows in the four wide layers: 1 pair (one ragged tile),
# 3 | 4 pairs (54 | 72 rows of layer 4), 10 | 11 pairs (60 | 66 rows of the fusion layer) sit either side of the tile boundary
@pytest.mark.parametrize("n", [1, 3, 4, 10, 11])
def test_costs_within_the_float_tolerance(eng, model, n):
    assert aflink.BM == 64
    rows = R.couples(20 + n, n)
    got, ref = _device_and_ref(eng, rows)
    _same_gate_and_inputs(got, ref, f"{n} pairs")
    c64 = R.net_costs(model, ref[2])
    err = np.abs(got[2] - c64).max()
    print(f"{n} pairs: max |device - f64| = {err:.3e}")
    assert err <= TOL


def test_costs_in_several_chunks(eng, model):
    rows = R.couples(41, 19)
    L = lib.load()
    one, ref = _device_and_ref(eng, rows)
    assert L.ss_op_set_option(b"aflink_chunk", 8) == 0
    try:
        got, _ = _device_and_ref(eng, rows)                                  # 8 + 8 + 3 pairs
    finally:
        assert L.ss_op_set_option(b"aflink_chunk", aflink.CHUNK) == 0
    _same_gate_and_inputs(got, ref, "chunks of 8")
    err = np.abs(got[2] - R.net_costs(model, ref[2])).max()
    print(f"19 pairs in chunks of 8: max |device - f64| = {err:.3e}")
    assert err <= TOL
    assert got[2].tobytes() == one[2].tobytes(), "a pair's cost does not depend on the chunk it travels in"


def test_costs_of_the_512_pair_set(eng, big):
    offsets, feats, pi, pj, x, c64, c32 = big
    got = eng.aflink_cost(offsets, feats, want_inputs=True)
    _same_gate_and_inputs(got, (pi, pj, x), "512 pairs")
    q = np.percentile(c64, [25, 50, 75])
    assert q[0] < 0.2 and q[2] > 0.8, "the calibrated network spreads its costs"
    cpu32 = np.abs(c32 - c64).max()
    err = np.abs(got[2] - c64).max()
    print(f"512 pairs: max |device - f64| = {err:.3e}, max |CPU f32 - f64| = {cpu32:.3e}, bound {8 * cpu32:.3e}")
    assert err <= TOL
    assert err <= 8 * cpu32


# ---- matching on costs the test supplies ---------------------------------------------------------------------------------------------
def _block(seed, rows, cols, thr_p, density=0.6, decimals=None):
    """One dense bipartite block: earlier tracklets 0 .. rows-1, later ones rows .. rows+cols-1; survivors with probability `density`,
    the other pairs cost more than thr_p."""
    rng = np.random.default_rng(seed)
    pi, pj = np.divmod(np.arange(rows * cols), cols)
    pj = pj + rows
    cost = np.where(rng.random(rows * cols) < density, rng.uniform(0.0, thr_p, rows * cols), rng.uniform(thr_p, 1.0, rows * cols))
    if density > 0:
        cost[0] = min(cost[0], 0.4 * thr_p)                                 # at least one survivor
    if decimals is not None:
        cost = np.round(cost, decimals)
    return rows + cols, pi.astype(np.int32), pj.astype(np.int32), cost


@pytest.mark.parametrize("rows,cols", [(1, 1), (40, 65), (70, 30), (180, 200), (256, 256)])
def test_matching_equals_scipy_on_tie_free_costs(eng, rows, cols):
    n, pi, pj, cost = _block(rows * 1000 + cols, rows, cols, 0.05)
    ref, total = R.match_full(n, pi, pj, cost, 0.05)
    got = eng.aflink_match(n, pi, pj, cost, 0.05)
    assert got.tolist() == ref.tolist()
    assert (got >= 0).sum() > 0


def test_matching_of_a_path_component_and_of_a_chain_of_links(eng):
    # a path in the survivor graph: 0-2', 3-2', 3-4', 5-4': one component of 3 x 2
    pi, pj = np.array([0, 3, 3, 5], np.int32), np.array([2, 2, 4, 4], np.int32)
    cost = np.array([0.03, 0.01, 0.04, 0.02])
    ref, _ = R.match_full(6, pi, pj, cost, 0.05)
    assert eng.aflink_match(6, pi, pj, cost, 0.05).tolist() == ref.tolist() == [-1, -1, -1, 2, -1, 4]
    # links 0 -> 1 -> 2 -> 3: three components of 1 x 1 (a tracklet as the earlier and as the later one are two nodes)
    pi, pj = np.array([0, 1, 2], np.int32), np.array([1, 2, 3], np.int32)
    assert eng.aflink_match(4, pi, pj, np.array([0.01, 0.02, 0.03]), 0.05).tolist() == [1, 2, 3, -1]


def test_matching_with_ties_has_scipys_count_and_cost_sum(eng):
    n, pi, pj, cost = _block(5, 60, 90, 0.05, decimals=2)
    assert len(np.unique(cost[cost < 0.05])) <= 5
    ref, total = R.match_full(n, pi, pj, cost, 0.05)
    got = eng.aflink_match(n, pi, pj, cost, 0.05)
    linked = got >= 0
    lookup = {(int(i), int(j)): c for i, j, c in zip(pi, pj, cost)}
    got_total = sum(lookup[(i, int(got[i]))] for i in np.nonzero(linked)[0])
    assert linked.sum() == (ref >= 0).sum() and got_total == pytest.approx(total, abs=1e-9)
    assert len(set(got[linked].tolist())) == linked.sum() and all(lookup[(i, int(got[i]))] < 0.05 for i in np.nonzero(linked)[0])


def test_matching_without_survivors_and_at_the_threshold(eng):
    n, pi, pj, cost = _block(2, 5, 7, 0.05, density=0.0)
    assert eng.aflink_match(n, pi, pj, cost, 0.05).tolist() == [-1] * n
    cost[3] = 0.05                                                          # a cost equal to thr_p is left out
    assert eng.aflink_match(n, pi, pj, cost, 0.05).tolist() == [-1] * n
    cost[3] = np.nextafter(0.05, 0.0)
    assert eng.aflink_match(n, pi, pj, cost, 0.05).tolist() == R.match_full(n, pi, pj, cost, 0.05)[0].tolist() != [-1] * n
    assert eng.aflink_match(3, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), 0.05).tolist() == [-1] * 3


def test_a_component_of_257_is_refused_and_the_context_stays_usable(eng):
    assert aflink.max_component() == aflink.MAX_COMPONENT == 256
    pi, pj = np.zeros(257, np.int32), np.arange(1, 258, dtype=np.int32)
    with pytest.raises(lib.SSError, match="1 x 257") as e:
        eng.aflink_match(258, pi, pj, np.full(257, 0.01), 0.05)
    assert e.value.code == lib.SS_ERR_CAPACITY
    n, pi, pj, cost = _block(9, 12, 9, 0.05)
    assert eng.aflink_match(n, pi, pj, cost, 0.05).tolist() == R.match_full(n, pi, pj, cost, 0.05)[0].tolist()
    eng.check_errors()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SCENES["scenes"])
def test_link_and_the_cli_files_equal_the_restatement(eng, model, seed, tmp_path):
    rows = R.scene(seed)
    assert R.scene_qualifies(rows, model, SCENES["thr_p"], SCENES["margin"], SCENES["trials"]), "a committed scene seed must qualify"
    cost = None
    for thr_p in SCENES["thr_p"]:
        ref, ref_map, (pi, pj, cost) = R.link(rows, model, thr_p=thr_p, cost=cost)
        assert ref_map, "the scene should have links at every thr_p"
        info = {}
        got, got_map = aflink.link(rows, eng, model, thr_p=thr_p, info=info)
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes() and got_map == ref_map
        assert info == {"candidates": len(pi), "links": len(ref_map)}
        summary, outdir = {}, str(tmp_path / f"p{thr_p}")
        with_gsi = seed == SCENES["scenes"][0] and thr_p == SCENES["thr_p"][0]
        cli.aflink_post(rows, eng, {"aflink": model, "aflink_thr_p": thr_p, "gsi": with_gsi}, outdir, "scene", summary)
        assert open(os.path.join(outdir, "scene_labels_aflink.txt")).read() == gsi_ref.label_lines(ref)
        assert summary == {"aflink_candidates": len(pi), "aflink_links": len(ref_map)}
        assert os.path.exists(os.path.join(outdir, "scene_labels_aflink_gsi.txt")) == with_gsi
        if with_gsi:
            assert open(os.path.join(outdir, "scene_labels_aflink_gsi.txt")).read() == gsi_ref.label_lines(gsi_ref.gsi(ref)[0])


class _Boxes:
    def __init__(self, r):
        self.id, self.xyxy, self.conf, self.cls = r[:, 1].copy(), r[:, 2:6].copy(), r[:, 6].copy(), r[:, 7].copy()

    def __len__(self):
        return len(self.id)

    def __iter__(self):
        return iter([self])


class _Result:
    def __init__(self, r, img):
        self.boxes, self.orig_img = (_Boxes(r) if len(r) else None), img


class _Replay:
    """Stands where the detector and tracker stand in cli.process_video and replays a scene's rows frame by frame (frame = index in
    the stream), so the stream's tracked rows are rows that gate; the post-processing runs on a real engine."""
    names = {0: "object"}

    def __init__(self, rows, eng):
        self.rows, self.eng = rows, eng

    def overlay(self):
        return self

    def track_stream(self, src, batch=1, device=0, **kw):
        for k, frame in enumerate(src):
            yield [_Result(self.rows[self.rows[:, 0] == k], frame)]


def test_cli_writes_the_linked_labels_beside_the_untouched_labels(eng, model, tmp_path):
    import json as _json
    rows = R.scene(SCENES["scenes"][1])
    n_frames = int(rows[:, 0].max()) + 1
    src, ckpt = tmp_path / "seq.npy", tmp_path / "aflink.pth"
    np.save(src, np.zeros((n_frames, 8, 8, 3), np.uint8))
    torch.save(model.state_dict(), ckpt)
    with pytest.raises(SystemExit):
        cli.main(["--source", str(src), "--aflink", str(ckpt)])              # needs --track
    replay = _Replay(rows, eng)
    names = ("", "_gsi", "_aflink", "_aflink_gsi")
    labels, outs = {}, {}
    for run, extra in (("a", {}), ("b", {"aflink": str(ckpt), "aflink_thr_p": 0.5, "gsi": True}),
                       ("c", {"aflink": str(ckpt), "aflink_thr_p": 0.5, "gsi": True, "eval_gt": str(tmp_path / "a" / "seq_labels.txt")})):
        outs[run] = cli.process_video({"source": str(src), "track": True, "count": False, "batch": 4, "outdir": str(tmp_path / run), **extra}, model=replay)
        assert outs[run]["frames"] == n_frames
        labels[run] = [(tmp_path / run / f"seq_labels{k}.txt").read_bytes() if (tmp_path / run / f"seq_labels{k}.txt").exists() else None for k in names]
    assert labels["a"][0] == labels["b"][0] == labels["c"][0] and labels["a"][0] and labels["a"][1:] == [None, None, None]
    assert labels["a"][0].decode() == gsi_ref.label_lines(rows)                  # the stream's rows are the scene's
    assert "aflink_links" not in outs["a"] and all(v is not None for v in labels["b"]) and labels["b"] == labels["c"]
    ref, ref_map, (pi, pj, cost) = R.link(rows, model, thr_p=0.5)
    assert len(pi) > 0 and len(ref_map) > 0, "the replayed scene gates and links"
    assert outs["b"]["aflink_candidates"] == len(pi) and outs["b"]["aflink_links"] == len(ref_map)
    assert labels["b"][2].decode() == gsi_ref.label_lines(ref)
    assert labels["b"][1].decode() == gsi_ref.label_lines(gsi_ref.gsi(rows)[0])   # the GSI file is what it is without --aflink
    assert labels["b"][3].decode() == gsi_ref.label_lines(gsi_ref.gsi(ref)[0])    # AFLink, then GSI
    # --eval-gt: every file is a pair of the one scoring call, a key of the metrics file and a suffix of the summary's figures
    metrics = _json.load(open(tmp_path / "c" / "seq_metrics.json"))
    assert sorted(metrics) == ["labels", "labels_aflink", "labels_aflink_gsi", "labels_gsi"]
    for k in ("", "_gsi", "_aflink", "_aflink_gsi"):
        assert outs["c"]["HOTA" + k] == metrics["labels" + k]["HOTA"] and "MOTA" + k in outs["c"] and "IDSW" + k in outs["c"]
    assert metrics["labels"]["IDSW"] == 0 and metrics["labels"]["MOTA"] == 1.0    # the ground truth is the labels file itself
    assert len(set(ref[:, 1])) < len(set(rows[:, 1])) and "HOTA_aflink" not in outs["b"]


# ---- guards ------------------------------------------------------------------------------------------------------------------
def test_cost_without_weights_is_refused(model):
    e = engine(debug=False)
    try:
        _, offsets, _, feats = R.tracklets(R.couples(1, 2))
        with pytest.raises(lib.SSError, match="no weights") as err:
            e.aflink_cost(offsets, feats)
        assert err.value.code == lib.SS_ERR_INVALID
        with pytest.raises(lib.SSError, match="floats"):
            e.aflink_set_weights(np.zeros(10, np.float32))
        e.aflink_set_weights(aflink.pack(model))
        assert len(e.aflink_cost(offsets, feats)[2]) == 2
    finally:
        e.close()


def test_a_generous_cap_gives_the_same_pairs_and_a_small_one_is_refused(eng):
    import ctypes as C
    _, offsets, _, feats = R.tracklets(R.couples(61, 6))
    want = eng.aflink_cost(offsets, feats)
    pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
    L, count = lib.load(), C.c_longlong(0)
    for cap, rc in ((1 << 22, lib.SS_OK), (6, lib.SS_OK), (5, lib.SS_ERR_CAPACITY)):       # room is made for min(cap, n (n - 1) / 2) = 66 at most
        i, j, c = np.full(8, -1, np.int32), np.full(8, -1, np.int32), np.zeros(8)
        got = L.ss_aflink_cost(eng.ctx, 12, offsets.ctypes.data_as(pi), feats.ctypes.data_as(pd), 0, 30, 75.0, cap, i.ctypes.data_as(pi), j.ctypes.data_as(pi),
                               c.ctypes.data_as(pd), None, C.byref(count))
        assert got == rc and count.value == 6
        if rc == lib.SS_OK:
            assert i[:6].tolist() == want[0].tolist() and j[:6].tolist() == want[1].tolist() and c[:6].tobytes() == want[2].tobytes()
        else:
            assert "6 candidates, cap 5" in L.ss_last_error(eng.ctx).decode()


def test_scratch_reuse_and_determinism(eng, model):
    large, small = R.couples(51, 40), R.couples(52, 5)
    first, ref_l = _device_and_ref(eng, large)
    got_s, ref_s = _device_and_ref(eng, small)                                # a smaller call after a larger one: the scratch is reused
    again, _ = _device_and_ref(eng, large)
    _same_gate_and_inputs(got_s, ref_s, "small after large")
    assert np.abs(got_s[2] - R.net_costs(model, ref_s[2])).max() <= TOL
    assert np.abs(first[2] - R.net_costs(model, ref_l[2])).max() <= TOL
    for a, b in zip(first, again):                                           # two identical calls: the same bytes
        assert a.tobytes() == b.tobytes()
    with pytest.raises(lib.SSError, match="tracklet 1: frames must increase"):
        eng.aflink_cost([0, 2, 4], np.array([[1, 5, 5], [2, 5, 5], [9, 5, 5], [9, 5, 5.0]]))
    after, _ = _device_and_ref(eng, small)
    assert after[2].tobytes() == got_s[2].tobytes()
    eng.check_errors()
