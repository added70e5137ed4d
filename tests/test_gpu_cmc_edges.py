"""The ECC camera-motion estimator (csrc/ss_cmc.hip: k_gray_small, k_ecc, k_cmc_roll) on the MI355X against the oracle, bit for
bit, where tests/test_gpu_cmc.py does not go: rotations and gain / bias, non-integer scales, strided views, fewer pixels than
threads, the 64-sample cut, every exit of the iteration, n_valid, full groups of three streams, size changes, resets, refusals and
graph capture.  tests/cmc_ref.py makes the inputs and keeps the books; tests/test_cmc_ref_cpu.py checks both without a GPU.
Every case also asserts, on the reference, the property that makes it meaningful."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import cexact
from tests import cmc_ref as R
from tests.test_cmc_ref_cpu import CAP_PAIR, EXIT_SEED, SEED, _pair, tiny

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ID = R.IDENTITY


def _make(S):
    from strongsort_yolo_amd.engine import TrackerEngine
    return TrackerEngine(n_streams=S, debug=False), R.EccRef(S)


@pytest.fixture(scope="module")
def one():
    eng, ref = _make(1)
    yield eng, ref
    eng.close()


@pytest.fixture(scope="module")
def three():
    eng, ref = _make(3)
    yield eng, ref
    eng.close()


def _device_frames(frames, padded):
    """[F, S, H, W, 3] on the device as [F * S, H, W, 3]: contiguous, or the corner of a buffer 7 rows taller and 5 pixels wider
    whose padding holds 255 (row_stride > 3 W, frame_stride > H * row_stride)."""
    F, S, H, W = frames.shape[:4]
    d = torch.from_numpy(np.ascontiguousarray(frames).reshape(F * S, H, W, 3)).to(DEV)
    if not padded:
        return d
    buf = torch.full((F * S, H + 7, W + 5, 3), 255, dtype=torch.uint8, device=DEV)
    buf[:, :H, :W] = d
    view = buf[:, :H, :W]
    assert view.stride(1) > 3 * W and view.stride(0) > H * view.stride(1)
    return view


def _equal(got, exp, what):
    for f in range(exp.shape[0]):
        for s in range(exp.shape[1]):
            assert np.array_equal(got[f, s, :7], exp[f, s, :7]), f"{what} frame {f} stream {s}: got {got[f, s, :7]}, expected {exp[f, s, :7]}"


def _run(pair, frames, what, n_valid=None, padded=False):
    """One ss_cmc_estimate call on the engine and on its reference (both move on, whatever the comparison says)."""
    eng, ref = pair
    F = frames.shape[0]
    nv = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int32, device=DEV)
    got = eng.cmc_estimate(_device_frames(frames, padded), F, n_valid=nv).cpu().numpy()
    exp = ref.estimate(frames, n_valid)
    _equal(got, exp, what)
    return got, exp


def _check_smalls(pair, what):
    """Frames 1..F of the last call and the remembered predecessor (frame 0), byte for byte."""
    eng, ref = pair
    for f, row in enumerate(ref.smalls):
        for s, img in enumerate(row):
            got = eng.cmc_small(f + 1, s)
            assert got.shape == img.shape and np.array_equal(got, img), f"{what}: small image of frame {f} stream {s}"
    for s, img in enumerate(ref.prev):
        if img is not None:
            assert np.array_equal(eng.cmc_small(0, s), img), f"{what}: remembered small image of stream {s}"


def _angle(w8):
    return np.arctan2(w8[..., 3], w8[..., 0])


# ---- 1. the down-scale alone --------------------------------------------------------------------------------------------------
# (337, 517): both scales non-integer; (330, 510), (120, 160): scale 10; (20, 20): the smallest frame, a 2 x 2 image; (21, 29): 2 x 2
# at scales 10.5 and 14.5
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("hw", [(337, 517), (330, 510), (120, 160), (20, 20), (21, 29)])
def test_small_images_equal_oracle(one, hw, padded):
    H, W = hw
    hs, ws = R.small_hw(H, W)
    rng = np.random.default_rng(H * W + padded)
    last = None
    for call in range(2):
        frames = rng.integers(0, 256, (2, 1, H, W, 3), dtype=np.uint8)
        _run(one, frames, f"{hw} call {call}", padded=padded)
        _check_smalls(one, f"{hw} call {call}")
        assert one[1].smalls[0][0].shape == (hs, ws) and np.array_equal(one[1].prev[0], cexact.gray_small(frames[1, 0], hs, ws))
        assert last is None or not np.array_equal(one[1].prev[0], last)          # the predecessor did move on
        last = one[1].prev[0]
    if padded:                                                                 # a read of the padding would have shown
        dark = np.zeros((1, 1, H, W, 3), np.uint8)
        _run(one, dark, f"{hw} dark", padded=True)
        assert not one[0].cmc_small(1, 0).any()


# ---- 2. rotation, shift and gain / bias ---------------------------------------------------------------------------------------
_ROT = {}


def _rotation_frames(H, W):
    """still, motion 1, still, motion 2, still, motion 3 of one scene (cmc_ref.MOTIONS, shifts scaled to the frame)"""
    if (H, W) not in _ROT:
        hs, ws = R.small_hw(H, W)
        sc = R.scene(H, W, SEED)
        still = R.warped(sc, 0, 0, 0)
        fr = []
        for theta, tx, ty, gain, bias in R.MOTIONS:
            fr += [still, R.warped(sc, theta, tx * W / ws, ty * H / hs, gain, bias)]
        _ROT[H, W] = np.stack(fr)[:, None]
    return _ROT[H, W]


# (120, 160): 192 small pixels, so 13 of k_ecc's 16 waves add nothing
@pytest.mark.parametrize("hw", [(720, 1280), (480, 640), (337, 517), (120, 160)])
def test_rotation_shift_gain_equal_oracle(one, hw):
    H, W = hw
    frames = _rotation_frames(H, W)
    for padded in (False, True):
        got, exp = _run(one, frames, f"{hw} padded {padded}", padded=padded)
        for k, (theta, tx, ty, _, _) in enumerate(R.MOTIONS):
            fwd, back = exp[2 * k + 1, 0], exp[2 * k + 2, 0] if k < 2 else None
            assert 2 <= fwd[6] <= 20 and abs(_angle(fwd)) > 0.01 and abs(_angle(fwd) - theta) < 0.005, (hw, theta, fwd)
            assert back is None or (back[6] >= 2 and abs(_angle(back) + theta) < 0.005), (hw, theta, back)
            assert tx == 0 or abs(fwd[2] / (W / R.small_hw(H, W)[1]) - tx) < 0.1, (hw, theta, fwd)
    _check_smalls(one, f"{hw}")


# ---- 3. three streams, full groups --------------------------------------------------------------------------------------------
def test_three_streams_32_frames(three):
    F, S, H, W = 32, 3, 120, 160
    rng = np.random.default_rng(11)
    scs = [R.scene(H, W, 10 * s) for s in range(S)]
    # (call, frame, stream): a flat frame gets no warp and gives none to its successor; a jump of half the frame gets none (the way
    # back may find one, or run into the iteration cap: it is compared, not judged)
    flat, jump = {(1, 5, 0)}, {(0, 9, 1): (0, 100, 0), (2, 20, 2): (0, 80, 60)}
    three[0].reset(-1); three[1].reset()
    for call in range(3):
        frames = np.zeros((F, S, H, W, 3), np.uint8)
        for f in range(F):
            for s in range(S):
                pose = jump.get((call, f, s), (rng.uniform(-0.03, 0.03), rng.uniform(-6, 6), rng.uniform(-6, 6)))
                frames[f, s] = 90 if (call, f, s) in flat else R.warped(scs[s], *pose)
        got, exp = _run(three, frames, f"call {call}")
        it = exp[..., 6]
        special = np.zeros((F, S), bool)
        for c, f, s in list(flat) + list(jump):
            if c == call:
                special[f, s] = special[f + 1, s] = True
                assert it[f, s] == -1 and ((c, f, s) in jump or it[f + 1, s] == -1), (call, f, s, it[f, s], it[f + 1, s])
        if call == 0:
            special[0] = True
            assert (it[0] == -1).all()
        assert (it[~special] >= 2).all() and (np.abs(_angle(exp[~special])) > 0.01).sum() > F       # ordinary pairs, most of them rotated
    _check_smalls(three, "call 2")


# ---- 4. the pixel-count edge and the exits ------------------------------------------------------------------------------------
def _exit_frames():
    """33 x 51 small images through blocks(): the pairs test_cmc_ref_cpu reaches every exit with, between ordinary pairs"""
    T, I = _pair(33, 51, EXIT_SEED, 0.03, 15, -10)
    cap = _pair(33, 51, EXIT_SEED, *CAP_PAIR)[1]
    flat = np.full_like(T, 90)
    seq = [T, I, 255 - I, 255 - T, T, cap, T, I, flat, T, I]
    return np.stack([R.blocks(x) for x in seq])[:, None]


def test_pixel_count_edge(one):
    a, b, c = tiny(8, 8)[:, :8], tiny(7, 9)[:, :9], tiny(8, 9)
    _, exp = _run(one, np.stack([R.blocks(a)] * 3)[:, None], "8 x 8")                   # exactly 64 samples
    assert exp[0, 0, 6] == -1 and (exp[1:, 0, 6] == 2).all()
    _check_smalls(one, "8 x 8")
    _, exp = _run(one, np.stack([R.blocks(b)] * 3)[:, None], "7 x 9")                   # 63
    assert (exp[:, 0, 6] == -1).all()
    c0, c1 = R.blocks(c[:, :9]), R.blocks(c[:, 1:10])                                    # 72, and a shift by one small pixel
    _, exp = _run(one, np.stack([c0, c0, c1, c1, c0, c0])[:, None], "8 x 9")
    assert list(exp[:, 0, 6]) == [-1, 2, -1, 2, -1, 2]                                   # the pair after a -1 is not affected
    _check_smalls(one, "8 x 9")


def test_exits_between_ordinary_pairs(one):
    _, exp = _run(one, _exit_frames(), "exits")
    it = exp[:, 0, 6]
    assert it[1] >= 2 and abs(_angle(exp[1, 0]) - 0.03) < 0.005                          # an ordinary pair
    assert it[2] == -1 and it[4] == -1                                                   # inverted: no positive scale
    assert it[3] >= 2 and abs(_angle(exp[3, 0]) + 0.03) < 0.005                          # both inverted: ordinary again
    assert it[5] == 100 and not np.array_equal(exp[5, 0, :6], ID[:6])                    # the cap: the last iterate
    assert it[8] == -1 and it[9] == -1                                                   # flat image, flat template
    assert np.array_equal(exp[7, 0], exp[1, 0]) and np.array_equal(exp[10, 0], exp[1, 0])      # the same pair after a cap and after a -1
    big = _pair(72, 128, EXIT_SEED, 0.6, 100, 100)                                       # an over-large jump
    _, exp = _run(one, np.stack([R.blocks(big[0]), R.blocks(big[1]), R.blocks(big[0])])[:, None], "jump")
    assert exp[1, 0, 6] == -1


# ---- 5. n_valid -----------------------------------------------------------------------------------------------------------------
def test_n_valid(three):
    F, S, H, W = 4, 3, 120, 160
    eng, ref = three
    rng = np.random.default_rng(21)
    scs, other = [R.scene(H, W, 40 + s) for s in range(S)], R.scene(H, W, 99)
    eng.reset(-1); ref.reset()
    stale = None
    for call, nv in enumerate([4, 3, 0, 1, 5, None]):
        n = F if nv is None else min(nv, F)
        frames = np.zeros((F, S, H, W, 3), np.uint8)
        for f in range(F):
            for s in range(S):                                   # stale: first an older view of the stream's scene, then another scene
                frames[f, s] = R.warped(scs[s] if f <= n else other, rng.uniform(-0.03, 0.03), rng.uniform(-6, 6), rng.uniform(-6, 6))
        before = [eng.cmc_small(0, s) for s in range(S)] if call else None
        got, exp = _run(three, frames, f"call {call} n_valid {nv}", n_valid=nv)
        assert np.array_equal(got[n:, :, :7], np.tile(ID[:7], (F - n, S, 1))) and (exp[n:, :, 6] == -1).all()
        assert (exp[1:n, :, 6] >= 2).all() and (call == 0 or n == 0 or (exp[0, :, 6] >= 2).all())
        _check_smalls(three, f"call {call} n_valid {nv}")
        hs, ws = R.small_hw(H, W)
        for s in range(S):
            if n < F:                                           # the first stale frame would have aligned with its predecessor
                assert R.pair_warp(ref.smalls[n - 1][s] if n else ref.prev[s], ref.smalls[n][s], H, W)[6] >= 2
            if n == 0:
                assert np.array_equal(eng.cmc_small(0, s), before[s]), f"call {call}: a group without real frames moved the predecessor"
            else:
                assert np.array_equal(eng.cmc_small(0, s), cexact.gray_small(frames[n - 1, s], hs, ws))
                if stale is not None:                           # aligned with the stale last frame, the warp would differ
                    assert not np.array_equal(R.pair_warp(stale[s], ref.smalls[0][s], H, W)[:7], exp[0, s, :7])
        if n > 0:                                               # what a roll of the whole buffer would have remembered
            stale = [cexact.gray_small(frames[F - 1, s], hs, ws) for s in range(S)] if n < F else None


# ---- 6. state ---------------------------------------------------------------------------------------------------------------------
def _moving(H, W, F, S, seed):
    rng = np.random.default_rng(seed)
    scs = [R.scene(H, W, seed + s) for s in range(S)]
    return np.stack([np.stack([R.warped(scs[s], rng.uniform(-0.03, 0.03), rng.uniform(-6, 6), rng.uniform(-6, 6)) for s in range(S)])
                     for _ in range(F)])


def test_frame_size_change_forgets_predecessors(one):
    _run(one, _moving(120, 160, 2, 1, 50), "before")
    for call, hw in enumerate([(330, 510), (120, 160), (330, 510)]):
        _, exp = _run(one, _moving(*hw, 2, 1, 60), f"call {call} {hw}")
        assert exp[0, 0, 6] == -1 and exp[1, 0, 6] >= 2
        _check_smalls(one, f"call {call} {hw}")
    _, exp = _run(one, _moving(330, 510, 2, 1, 60), "same size again")
    assert (exp[:, 0, 6] >= 2).all()


def test_reset_of_one_stream(three):
    fr = _moving(120, 160, 6, 3, 70)
    _run(three, fr[:2], "before")
    three[0].reset(1); three[1].reset(1)
    _, exp = _run(three, fr[2:4], "after reset(1)")
    assert exp[0, 1, 6] == -1 and exp[0, 0, 6] >= 2 and exp[0, 2, 6] >= 2 and (exp[1, :, 6] >= 2).all()
    three[0].reset(-1); three[1].reset()
    _, exp = _run(three, fr[4:], "after reset(-1)")
    assert (exp[0, :, 6] == -1).all() and (exp[1, :, 6] >= 2).all()


def test_refusals_leave_the_engine_usable(one):
    from strongsort_yolo_amd import lib
    eng = one[0]
    good = _moving(120, 160, 2, 1, 80)
    _run(one, good, "before")
    z = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device=DEV)
    overlapping = torch.as_strided(z(1, 40, 40, 3), (1, 40, 40, 3), (40 * 40 * 3, 3 * 39, 3, 1))      # rows 3 * (W - 1) bytes apart
    assert overlapping.stride(1) < 3 * 40
    for what, frames, F in [("H = 19", z(1, 19, 40, 3), 1), ("W = 19", z(1, 40, 19, 3), 1), ("row stride", overlapping, 1),
                            ("33 frames", z(33, 20, 20, 3), 33)]:
        with pytest.raises(lib.SSError) as ei:
            eng.cmc_estimate(frames, F)
        assert ei.value.code == lib.SS_ERR_INVALID, what
    with pytest.raises(lib.SSError) as ei:                        # read-back refusals: a frame past the last call's, a stream past S
        eng.cmc_small(3, 0)
    assert ei.value.code == lib.SS_ERR_INVALID
    with pytest.raises(lib.SSError) as ei:
        eng.cmc_small(0, 1)
    assert ei.value.code == lib.SS_ERR_INVALID
    buf, hs, ws = np.zeros(12 * 16 - 1, np.uint8), C.c_int(0), C.c_int(0)
    rc = eng.L.ss_cmc_get_small(eng.ctx, 1, 0, buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size, C.byref(hs), C.byref(ws))
    assert rc == lib.SS_ERR_INVALID and (hs.value, ws.value) == (12, 16)                                  # cap one byte short
    _, exp = _run(one, good[::-1].copy(), "after the refusals")    # the size, the predecessor and the context are as they were
    assert (exp[:, 0, 6] >= 2).all()
    eng.check_errors()


def test_read_back_before_the_first_estimate():
    from strongsort_yolo_amd import lib
    eng, _ = _make(1)
    with pytest.raises(lib.SSError) as ei:
        eng.cmc_small(0, 0)
    assert ei.value.code == lib.SS_ERR_INVALID
    eng.close()


# ---- 7. capture -----------------------------------------------------------------------------------------------------------------
def test_captured_estimate_equals_reference():
    from strongsort_yolo_amd import lib
    F, S, H, W = 4, 1, 120, 160
    pair = _make(S)
    eng, ref = pair
    fr = _moving(H, W, 4 * F, S, 90).reshape(4, F, S, H, W, 3)
    buf = torch.zeros(F * S, H, W, 3, dtype=torch.uint8, device=DEV)
    nv = torch.tensor([F], dtype=torch.int32, device=DEV)
    warps = torch.zeros(F, S, 8, dtype=torch.float64, device=DEV)
    side = torch.cuda.Stream(DEV)
    fresh, _ = _make(S)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        _run(pair, fr[0], "eager")                                 # the first call of the size allocates: outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            eng.cmc_estimate(buf, F, warps=warps, n_valid=nv)
            with pytest.raises(lib.SSError) as ei:                 # a fresh context: its first call of a size is refused here
                fresh.cmc_estimate(buf, F, warps=warps, n_valid=nv)
    assert ei.value.code == lib.SS_ERR_INVALID and "capture" in str(ei.value)
    torch.cuda.synchronize(DEV)
    for k, n in enumerate([4, 2, 4]):
        buf.copy_(torch.from_numpy(fr[k + 1].reshape(F * S, H, W, 3)))
        nv.fill_(n)
        torch.cuda.synchronize(DEV)
        graph.replay()
        torch.cuda.synchronize(DEV)
        exp = ref.estimate(fr[k + 1], n)
        _equal(warps.cpu().numpy(), exp, f"replay {k} n_valid {n}")
        assert (exp[:n, :, 6] >= 2).all() and (exp[n:, :, 6] == -1).all()
        _check_smalls(pair, f"replay {k}")
    eng.check_errors()
    del graph
    fresh.close()
    eng.close()
