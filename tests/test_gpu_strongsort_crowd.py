"""The StrongSORT chain on crowds (tests/strongsort_crowd.py): 129 - 256 tracks, 128 detections a frame, k_frame's one-wave LSAP in
each of its forms and orientations on a cost matrix in LDS or read back from cost_spill — against the oracle, bit for bit: rows,
cosine, Mahalanobis, gate, both cost matrices, both assignment lists, the candidate and column lists of every frame, the track
tables at the end.  What each scene reaches is fixed on the CPU (tests/test_strongsort_crowd_cpu.py); here the device's debug record
must also name the path (shortcut / LSAP) that the reference predicts for every frame and stage."""
import numpy as np
import pytest

from tests.gpu_util import engine
from tests.strongsort_crowd import EDGE_SIZES, H, W, edge_args, reference, solver_form
from tests.test_gpu_sequence import _compare_frame, _compare_table

pytestmark = pytest.mark.gpu

STAGINGS = [0, 1, 2, 4, 5, 104]                      # the assoc_stage values of test_assoc_operand_staging_variants


def _check_frame(eng, run, got, k, s, f, seen):
    """Frame k of `run` at position f of its group on stream s: everything _compare_frame compares, the stage B assignment list and
    the path of both stages; the LSAP shapes of the device's own record go to `seen`."""
    last = run.lasts[k]
    _compare_frame(eng, None, got, run.rows[k], k, s, f, last)
    dbg = eng.debug(s, f)
    pb = np.full(len(last["cand"]), -1, np.int32)
    for r, c in last["pairs_b"]:
        pb[r] = c
    assert np.array_equal(dbg["pairs_b"], pb), f"frame {k}: stage B assignment"
    (ra, ca, pa), (rb, cb, pbth) = run.stages[k]
    assert (dbg["n_conf"], dbg["n_dets"], dbg["path_a"]) == (ra, ca, pa), f"frame {k}: stage A shape / path"
    assert (dbg["n_cand"], dbg["n_cols"], dbg["path_b"]) == (rb, cb, pbth), f"frame {k}: stage B shape / path"
    if dbg["path_a"] == 2:
        seen[0].append((dbg["n_conf"], dbg["n_dets"]))
    if dbg["path_b"] == 2:
        seen[1].append((dbg["n_cand"], dbg["n_cols"]))


def _largest(shapes):
    return max(shapes, key=lambda s: (s[0] * s[1], s)) if shapes else None


def _run(cases, F, opts=None, capacity=False):
    """The scenes `cases` (reference() arguments, equally many frames each) side by side on the streams of one context, fed in groups of
    F frames; every frame and the final track tables against the cached reference.  capacity: SS_ERR_CAPACITY is expected to be
    pending after the groups (the rows are compared all the same)."""
    import torch
    from strongsort_yolo_amd import lib
    runs = [reference(*c) for c in cases]
    S, n = len(runs), len(runs[0].frames)
    assert all(len(r.frames) == n and r.cfg == runs[0].cfg for r in runs)
    eng = engine(runs[0].cfg, n_streams=S, debug=True)
    for name, value in (opts or {}).items():
        eng.set_option(name, value)
    dev = eng.device
    hw = torch.tensor([[H, W]] * S, dtype=torch.int32, device=dev)
    out, nout = torch.zeros(F, S, 256, 8, device=dev), torch.zeros(F, S, dtype=torch.int32, device=dev)
    seen = [([], []) for _ in range(S)]
    for k0 in range(0, n, F):
        nf = min(F, n - k0)
        hd, hf, hn = np.zeros((F, S, 128, 6), np.float32), np.zeros((F, S, 128, 512), np.float32), np.zeros((F, S), np.int32)
        for f in range(nf):
            for s, r in enumerate(runs):
                d, ft = r.frames[k0 + f]
                hd[f, s, :len(d)], hf[f, s, :len(d)], hn[f, s] = d, ft, len(d)
        eng.update_group(nf, torch.from_numpy(hd).to(dev), torch.from_numpy(hn).to(dev), torch.from_numpy(hf).to(dev), hw, out, nout)
        if not capacity:
            eng.check_errors()
        ho, hno = out.cpu().numpy(), nout.cpu().numpy()
        for f in range(nf):
            for s, r in enumerate(runs):
                _check_frame(eng, r, ho[f, s, :hno[f, s]], k0 + f, s, f, seen[s])
    if capacity:
        with pytest.raises(lib.SSError) as ei:
            eng.check_errors()
        assert ei.value.code == lib.SS_ERR_CAPACITY
    for s, r in enumerate(runs):
        _compare_table(eng, r.orc, s)
        a, b = _largest(seen[s][0]), _largest(seen[s][1])
        print(f"LSAP on the device: {r.name}{r.args} F={F} {opts or ''} stream {s}: stage A {a}"
              f"{'' if a is None else ' form %d' % solver_form(*a)}, stage B {b}{'' if b is None else ' form %d' % solver_form(*b)}")
    eng.close()
    return seen


@pytest.mark.parametrize("F", [1, 4, 32])
@pytest.mark.parametrize("case", [("two_crowds", 0), ("dense_crowd", 0), ("churn", 0, 5), ("churn", 0, 6)], ids=lambda c: "-".join(str(x) for x in c))
def test_scene_frame_by_frame_and_in_groups(case, F):
    """Every scene with one frame a call, in groups of 4 and as one call of up to 32 frames (tracks are born, confirmed and lost inside
    the group): two_crowds (256 tracks: the transposed 256 x 128 stage A from the spill on lsap_wave_regs<4>, the spilled 128 x 128
    stage B on lsap_wave_regs<2>), dense_crowd (an LSAP in both stages of a frame, tall and wide spilled matrices), churn (255 tracks;
    slots freed one frame before, or in the frame of, 85 births)."""
    seen = _run([case], F)
    if case[0] == "two_crowds":
        assert _largest(seen[0][0]) == (256, 128) and _largest(seen[0][1]) == (128, 128)


@pytest.mark.parametrize("size", EDGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edge_sizes(size):
    """A stage A LSAP of exactly n_tracks x d with an exact tie between two tracks: the last LDS-resident size (96 x 128 = 12288
    entries) and the first spilled one, both sides of the 64 and 128 edges between the solver's three forms in both orientations,
    256 x 128, and 3 detections against 200 tracks."""
    seen = _run([("edge_scene", *edge_args(*size))], 4)
    assert _largest(seen[0][0]) == size


@pytest.mark.parametrize("opts", [{"frame_caps": 16}, {"frame_caps": 112}, {"pred_ahead": 0}, {"pred_ahead": 1}, {"chain_merge": 0}, {"chain_merge": 1},
                                  {"assoc_pack": 0}, {"assoc_pack": 1}] + [{"assoc_stage": v % 100, "assoc_xcd_map": v // 100} for v in STAGINGS],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_two_crowds_under_each_option(opts):
    """256 tracks under every form of the chain: the track-indexed work arrays from frame_scratch (frame_caps: 256 tracks exceed any
    cap), the prediction ahead or inside k_frame, k_postnew or two launches, packed or per-frame columns, every operand staging."""
    _run([("two_crowds", 0)], 4, opts)


def test_crowd_beside_a_sparse_stream():
    """Stream 1's crowd spills and uses the scratch while stream 0 runs 12 identities: the per-stream offsets of cost_spill and
    frame_scratch."""
    _run([("sparse", 5), ("two_crowds", 0)], 4)


def test_two_crowds_side_by_side():
    """Two different crowds, both spilling in the same launches."""
    _run([("two_crowds", 0), ("two_crowds", 1)], 32)


@pytest.mark.parametrize("F", [1, 32])
def test_overflow_starts_the_lowest_detections_that_fit(F):
    """200 coasting tracks and 100 unmatched detections: the 56 of lowest index start tracks, SS_ERR_CAPACITY is pending, and the
    chain goes on as OracleStrongSort(max_tracks=256) does — every frame and the final table."""
    _run([("overflow", 0)], F, capacity=True)


@pytest.mark.parametrize("graph", [1, 0])
def test_chain_graph_replay_on_two_crowds(graph):
    """`track_graph` on 256 tracks, with the fixed caller buffers of test_chain_graph_replay_equals_oracle: groups of 2 frames (captured
    at the second call, replayed at the third and fourth, a partial last group) == plain launches == the oracle."""
    import torch
    run = reference("two_crowds", 0)
    F, n = 2, len(run.frames)
    eng = engine(run.cfg, debug=False)
    eng.set_option("track_graph", graph)
    dev = eng.device
    bd, bf, bn = torch.zeros(F, 1, 128, 6, device=dev), torch.zeros(F, 1, 128, 512, device=dev), torch.zeros(F, 1, dtype=torch.int32, device=dev)
    hw = torch.tensor([[H, W]], dtype=torch.int32, device=dev)
    out, nout = torch.zeros(F, 1, 256, 8, device=dev), torch.zeros(F, 1, dtype=torch.int32, device=dev)
    for k0 in range(0, n, F):
        nf = min(F, n - k0)
        hd, hf, hn = np.zeros((F, 1, 128, 6), np.float32), np.zeros((F, 1, 128, 512), np.float32), np.zeros((F, 1), np.int32)
        for f in range(nf):
            d, ft = run.frames[k0 + f]
            hd[f, 0, :len(d)], hf[f, 0, :len(d)], hn[f, 0] = d, ft, len(d)
        bd.copy_(torch.from_numpy(hd)); bf.copy_(torch.from_numpy(hf)); bn.copy_(torch.from_numpy(hn))
        eng.update_group(nf, bd, bn, bf, hw, out, nout)
        eng.check_errors()
        ho, hno = out.cpu().numpy(), nout.cpu().numpy()
        for f in range(nf):
            got, ref = ho[f, 0, :hno[f, 0]], run.rows[k0 + f]
            assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), f"frame {k0 + f}"
    _compare_table(eng, run.orc)
    eng.close()
