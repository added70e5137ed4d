"""AFLink without a GPU: the restatement (tests/aflink_ref.py) against literal forms of itself, the Python side of
strongsort_yolo_amd.aflink (pack / unpack / load / merge), the library's host-only entry points and the CLI's argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from strongsort_yolo_amd import aflink, cli, lib
from tests import aflink_ref as R


@pytest.fixture(scope="module")
def model():
    return R.calibrated(0)


def test_transform_against_a_literal_per_pair_form():
    rows = R.couples(5, 6, lengths=[(1, 60), (29, 31), (30, 30), (60, 1), (12, 40), (31, 29)])
    _, offsets, _, feats = R.tracklets(rows)
    pi, pj = R.gate(offsets, feats)
    assert pi.tolist() == [0, 2, 4, 6, 8, 10] and pj.tolist() == [1, 3, 5, 7, 9, 11]
    x = R.transform(offsets, feats, pi, pj)
    for k, (i, j) in enumerate(zip(pi, pj)):
        a, b = feats[offsets[i]:offsets[i + 1]], feats[offsets[j]:offsets[j + 1]]
        stack = [[0.0, 0.0, 0.0]] * max(30 - len(a), 0) + a[-30:].tolist() + b[:30].tolist() + [[0.0, 0.0, 0.0]] * max(30 - len(b), 0)
        assert len(stack) == 60
        for c in range(3):
            col = [r[c] for r in stack]
            lo, hi = min(col), max(col)
            for t in range(60):
                want = np.float32((col[t] - (hi + lo) / 2.0) / ((hi - lo) / 2.0 + 1e-5))
                assert x[k, t // 30, t % 30, c] == want


def test_gate_is_row_major_and_keeps_the_exact_distance():
    rows = np.zeros((4, 8))
    rows[:, 0], rows[:, 1] = [10, 12, 12, 39], [1, 2, 3, 4]
    rows[:, 2], rows[:, 3] = [500, 545, 545, 500], [500, 560, np.nextafter(560.0, np.inf), 500]
    _, offsets, _, feats = R.tracklets(rows)
    pi, pj = R.gate(offsets, feats)
    # (0, 2) and (2, 3) are a hair over 75 and dropped, (0, 1) and (1, 3) exactly 75 and kept; gap 29 of (0, 3) is kept; 1 and 2 share
    # frame 12 (gap 0): the smaller number is the earlier one, (2, 1) is no candidate
    assert list(zip(pi.tolist(), pj.tolist())) == [(0, 1), (0, 3), (1, 2), (1, 3)]
    assert R.gate(offsets, feats, (0, 29))[0].tolist() == [0, 1, 1]                      # gap 29 of (0, 3) is now thrT1


def test_two_one_row_tracklets_on_one_frame_link_one_way_and_a_cycle_is_refused():
    rows = np.zeros((2, 8))
    rows[:, 0], rows[:, 1], rows[:, 2] = [5, 5], [1, 2], [100, 110]
    ids, offsets, r, feats = R.tracklets(rows)
    pi, pj = R.gate(offsets, feats)
    assert (pi.tolist(), pj.tolist()) == ([0], [1])                                      # not (1, 0) as well: both costs could survive
    succ, _ = R.match_full(2, pi, pj, np.array([0.01]), 0.05)
    assert succ.tolist() == [1, -1]
    for merge in (R.merge, aflink.merge):
        out, id_map = merge(r, ids, succ)
        assert id_map == {2: 1} and out[:, [0, 1, 2]].tolist() == [[5.0, 1.0, 100.0]]  # one row a (frame, id): the earlier tracklet's
        with pytest.raises(ValueError, match="cycle"):
            merge(r, ids, np.array([1, 0], np.int32))
    rows3 = np.zeros((3, 8))
    rows3[:, 0], rows3[:, 1] = [5, 5, 5], [1, 2, 3]
    with pytest.raises(ValueError, match="cycle"):
        aflink.merge(rows3, np.array([1.0, 2.0, 3.0]), np.array([1, 2, 0], np.int32))
    with pytest.raises(ValueError, match="cycle"):
        R.merge(rows3, np.array([1.0, 2.0, 3.0]), np.array([1, 2, 0], np.int32))
    with pytest.raises(ValueError, match="successor of two"):
        aflink.merge(rows3, np.array([1.0, 2.0, 3.0]), np.array([2, 2, -1], np.int32))
    with pytest.raises(ValueError, match="out of range"):
        aflink.merge(rows3, np.array([1.0, 2.0, 3.0]), np.array([3, -1, -1], np.int32))


def _problem(rng, n, pairs, decimals=None):
    ij = rng.permutation(n * n)[:pairs]
    pi, pj = np.divmod(np.sort(ij), n)
    keep = pi != pj
    cost = rng.uniform(0.0, 0.1, pairs)
    if decimals is not None:
        cost = np.round(cost, decimals)
    return pi[keep].astype(np.int32), pj[keep].astype(np.int32), cost[keep]


def test_component_matching_equals_the_full_matching():
    rng = np.random.default_rng(0)
    for trial in range(40):
        n = int(rng.integers(2, 120))
        pi, pj, cost = _problem(rng, n, int(rng.integers(1, 4 * n)))
        full, comp = R.match_full(n, pi, pj, cost), R.match_components(n, pi, pj, cost)
        assert full[0].tolist() == comp[0].tolist() and full[1] == pytest.approx(comp[1], abs=1e-12)
    for trial in range(20):                                                  # tie-heavy: the same count and cost sum
        n = int(rng.integers(10, 80))
        pi, pj, cost = _problem(rng, n, 6 * n, decimals=2)
        full, comp = R.match_full(n, pi, pj, cost), R.match_components(n, pi, pj, cost)
        assert (full[0] >= 0).sum() == (comp[0] >= 0).sum() and full[1] == pytest.approx(comp[1], abs=1e-9)


def _rows_of(spans):
    """{id: (first frame, last frame)} -> rows, x1 = 100 id so a row's origin stays visible."""
    out = []
    for tid, (a, b) in spans.items():
        blk = np.zeros((b - a + 1, 8))
        blk[:, 0], blk[:, 1], blk[:, 2] = np.arange(a, b + 1), tid, 100.0 * tid
        out.append(blk)
    return np.concatenate(out, 0)


@pytest.mark.parametrize("merge", [R.merge, aflink.merge])
def test_chains_merge_to_their_head_and_the_predecessors_row_stays(merge):
    # ids 7 -> 3 -> 9 (tracklets 1 -> 0 -> 2 by rising id); 3 starts on 7's last frame, 9 on 3's last: two duplicates
    rows = _rows_of({3: (10, 14), 7: (1, 10), 9: (14, 20), 11: (5, 6)})
    ids = np.array([3.0, 7.0, 9.0, 11.0])
    succ = np.array([2, 0, -1, -1], np.int32)
    out, id_map = merge(rows, ids, succ)
    assert id_map == {3: 7, 9: 7}
    assert sorted(set(out[:, 1].tolist())) == [7.0, 11.0] and len(out) == len(rows) - 2
    assert np.array_equal(out, out[np.lexsort((out[:, 1], out[:, 0]))])
    chain = out[out[:, 1] == 7.0]
    assert chain[:, 0].tolist() == list(range(1, 21))
    assert chain[chain[:, 0] == 10, 2].item() == 700.0 and chain[chain[:, 0] == 14, 2].item() == 300.0      # the predecessor's row
    # a one-row tracklet between two others on the same frame: the head's row stays
    rows = _rows_of({1: (1, 5), 2: (5, 5), 3: (5, 8)})
    out, id_map = merge(rows, np.array([1.0, 2.0, 3.0]), np.array([1, 2, -1], np.int32))
    assert id_map == {2: 1, 3: 1} and out[out[:, 0] == 5, 2].tolist() == [100.0]


def test_both_merges_agree_whatever_the_order_of_the_links():
    rng = np.random.default_rng(4)
    rows = R.scene(11, objects=8)
    ids, offsets, r, feats = R.tracklets(rows)
    pi, pj = R.gate(offsets, feats)
    succ, _ = R.match_full(len(ids), pi, pj, rng.uniform(0, 0.06, len(pi)), 0.05)
    assert (succ >= 0).sum() >= 3
    a, amap = R.merge(r, ids, succ)
    b, bmap = aflink.merge(r[rng.permutation(len(r))], ids, succ)
    assert a.tobytes() == b.tobytes() and amap == bmap


def test_pack_then_unpack_reproduces_the_folded_network(model):
    blob = aflink.pack(model)
    assert blob.dtype == np.float32 and len(blob) == aflink.WEIGHT_FLOATS == 1068482
    p32, p64 = aflink.unpack(blob), aflink.parts(model)
    assert all(np.array_equal(p32[k], p64[k].astype(np.float32)) for k, _ in aflink.LAYOUT)
    x = R.couple_inputs(9, 24)
    ref = R.net_costs(model, x)                                              # float64, BatchNorms unfolded
    assert np.abs(aflink.folded_costs(p64, x) - ref).max() <= 1e-12          # the folding itself, in float64
    # the blob's float32 rounding: 2^-24 relative per weight, scale and bias, through six layers into a logit difference whose
    # standard deviation the calibration sets to 4 and whose slope into the cost is at most 1/4: well below 1e-5
    assert np.abs(aflink.folded_costs(p32, x) - ref).max() <= 1e-5


def test_weights_are_uploaded_again_after_an_in_place_change():
    class Engine:
        uploads = 0

        def aflink_set_weights(self, blob):
            self.uploads += 1

    e, a, b = Engine(), aflink.PostLinker(0), aflink.PostLinker(1)
    aflink._set_weights(e, a)
    aflink._set_weights(e, a)
    assert e.uploads == 1
    a.load_state_dict(b.state_dict())
    aflink._set_weights(e, a)
    assert e.uploads == 2
    with torch.no_grad():
        a.classifier.fc2.bias.mul_(2.0)
    aflink._set_weights(e, a)
    aflink._set_weights(e, b)
    aflink._set_weights(e, b)
    assert e.uploads == 4


def test_load_is_strict_and_names_the_key(model, tmp_path):
    sd = model.state_dict()
    path = tmp_path / "aflink.pth"
    torch.save(sd, path)
    x = torch.from_numpy(R.couple_inputs(9, 4))
    for src in (str(path), sd, {"state_dict": sd}):
        got = aflink.load(src)
        with torch.no_grad():
            assert torch.equal(got(x[:, 0:1], x[:, 1:2]), model(x[:, 0:1], x[:, 1:2]))
    assert "TemporalModule_1.0.bnf.running_mean" in sd and "FusionBlock_2.conv.weight" in sd and "classifier.fc2.bias" in sd
    short = {k: v for k, v in sd.items() if k != "TemporalModule_2.3.bny.running_var"}
    with pytest.raises(ValueError, match="missing key 'TemporalModule_2.3.bny.running_var'"):
        aflink.load(short)
    with pytest.raises(ValueError, match="unexpected key 'extra.weight'"):
        aflink.load({**sd, "extra.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match=r"'classifier.fc1.weight' has shape \(128, 256\)"):
        aflink.load({**sd, "classifier.fc1.weight": torch.zeros(128, 256)})


def test_host_only_entry_points_check_their_arguments_without_a_context():
    lib.build()
    L = lib.load()
    assert L.ss_aflink_weight_floats() == aflink.WEIGHT_FLOATS and L.ss_aflink_max_component() == aflink.MAX_COMPONENT
    pi, pd, pf = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float)
    count = C.c_longlong(0)

    def cost(offsets, feats, t=(0, 30), s=75.0, cap=0):
        offsets, feats = np.asarray(offsets, np.int32), np.asarray(feats, np.float64)
        rc = L.ss_aflink_cost(None, len(offsets) - 1, offsets.ctypes.data_as(pi), feats.ctypes.data_as(pd), t[0], t[1], s, cap, None, None, None, None, C.byref(count))
        return rc, L.ss_last_error(None).decode()

    good = [[1, 5, 5], [2, 5, 5], [9, 5, 5], [10, 5, 5]]
    assert cost([0, 2, 4], good) == (lib.SS_ERR_INVALID, "ss_aflink_cost: null context")       # the arguments pass: the context is next
    for args, why in ((([0, 2, 4], [[1, 5, 5], [2, 5, 5], [9, 5, 5], [9, 5, 5]]), "tracklet 1: frames must increase"),
                      (([0, 2, 2], good), "tracklet 1: no rows"), (([1, 2, 4], good), "offsets"),
                      (([0, 2, 4], [[1, 5, 5], [2.5, 5, 5], [9, 5, 5], [10, 5, 5]]), "not an integer"),
                      (([0, 2, 4], [[1, 5, np.nan], [2, 5, 5], [9, 5, 5], [10, 5, 5]]), "NaN"),
                      (([0, 2, 4], good, (30, 30)), "thr_t0 < thr_t1"), (([0, 2, 4], good, (0, 30), -1.0), "thr_s"),
                      (([0, 2, 4], good, (0, 30), 75.0, 5), "cap")):
        rc, msg = cost(*args)
        assert rc == lib.SS_ERR_INVALID and why in msg, (args, msg)
    assert L.ss_aflink_set_weights(None, np.zeros(8, np.float32).ctypes.data_as(pf), 8) == lib.SS_ERR_INVALID
    assert "ss_aflink_weight_floats" in L.ss_last_error(None).decode()
    succ = np.zeros(3, np.int32)
    i, j = np.array([0, 1], np.int32), np.array([1, 2], np.int32)

    def match(i, j, c, thr=0.05):
        c = np.asarray(c, np.float64)
        return L.ss_aflink_match(None, 3, len(i), i.ctypes.data_as(pi), j.ctypes.data_as(pi), c.ctypes.data_as(pd), thr, succ.ctypes.data_as(pi))

    succ[:] = 7
    assert match(i, j, [0.5, 0.05]) == lib.SS_OK and succ.tolist() == [-1, -1, -1]            # no survivor: settled on the host
    assert match(i, j, [0.01, 0.5]) == lib.SS_ERR_INVALID and "null context" in L.ss_last_error(None).decode()
    assert match(i[::-1].copy(), j[::-1].copy(), [0.5, 0.5]) == lib.SS_ERR_INVALID and "row-major" in L.ss_last_error(None).decode()
    assert match(i, np.array([1, 1], np.int32), [0.5, 0.5]) == lib.SS_ERR_INVALID              # i == j
    assert match(i, j, [0.5, np.nan]) == lib.SS_ERR_INVALID
    assert L.ss_op_set_option(b"aflink_chunk", 0) == lib.SS_ERR_INVALID and L.ss_op_set_option(b"aflink_chunk", aflink.CHUNK) == lib.SS_OK


@pytest.mark.parametrize("argv,why", [
    (["--aflink", "{ckpt}"], "needs --track"),
    (["--track", "--aflink", "{ckpt}.missing"], "no such file"),
    (["--track", "--aflink", "{ckpt}", "--aflink-thr-t", "30", "30"], "0 <= A < B"),
    (["--track", "--aflink", "{ckpt}", "--aflink-thr-t", "-1", "30"], "0 <= A < B"),
    (["--track", "--aflink", "{ckpt}", "--aflink-thr-s", "-2"], "--aflink-thr-s"),
    (["--track", "--aflink", "{ckpt}", "--aflink-thr-p", "0"], "--aflink-thr-p"),
    (["--track", "--aflink", "{ckpt}", "--aflink-thr-p", "1.5"], "--aflink-thr-p"),
])
def test_cli_argument_errors(argv, why, tmp_path, capsys):
    ckpt = tmp_path / "aflink.pth"
    ckpt.write_bytes(b"")
    with pytest.raises(SystemExit):
        cli.main([a.replace("{ckpt}", str(ckpt)) for a in argv])
    assert why in capsys.readouterr().err
