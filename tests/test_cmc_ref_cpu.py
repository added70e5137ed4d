"""The ECC oracle (oracle.cexact.ecc, the definition of ss_cmc_estimate's result, DECISIONS D-18) against known camera motion,
every exit of the iteration reached with the oracle alone, and tests/cmc_ref.py (inputs and group bookkeeping of the GPU tests)
against calls written out by hand.  No GPU."""
import numpy as np
import pytest

from oracle import cexact
from tests import cmc_ref as R
from tests.test_oracle_cmc import _texture

SEED = 7                     # the scenes of the rotation test
EXIT_SEED = 1                # the scenes of the exit tests (test_gpu_cmc_edges uses the same pairs)
CAP_PAIR = (0.25, 10.0, 0.0) # (theta, tx, ty), full-frame pixels at 330 x 510, scene EXIT_SEED: runs into the iteration cap

# largest errors of the oracle measured with this generator over cmc_ref.MOTIONS, per small-image size: (angle [rad], shift [px])
MEASURED = {(72, 128): (3.4e-5, 0.0059), (48, 64): (1.0e-4, 0.0114), (33, 51): (3.4e-4, 0.0143)}


def _pair(hs, ws, seed, theta, tx, ty, gain=1.0, bias=0.0):
    """small images (previous, current) of a 10 hs x 10 ws scene whose camera moved by (theta, tx, ty), full-frame pixels"""
    sc = R.scene(10 * hs, 10 * ws, seed)
    return cexact.gray_small(R.warped(sc, 0, 0, 0), hs, ws), cexact.gray_small(R.warped(sc, theta, tx, ty, gain, bias), hs, ws)


def test_still_view_and_blocks_are_exact():
    sc = R.scene(120, 160, 3)
    assert sc.shape == (320, 360, 3) and sc.dtype == np.uint8
    assert np.array_equal(R.warped(sc, 0, 0, 0), sc[R.MARGIN:-R.MARGIN, R.MARGIN:-R.MARGIN])
    assert np.array_equal(R.warped(sc, 0, 7, -5), sc[R.MARGIN + 5:R.MARGIN + 125, R.MARGIN - 7:R.MARGIN + 153])     # the scene moves with the shift
    g = R.warped(sc, 0, 0, 0, gain=0.5, bias=200.0)
    assert g.max() == 255 and np.array_equal(g, np.clip(np.floor(sc[100:-100, 100:-100] * 0.5 + 200.5), 0, 255))
    rng = np.random.default_rng(0)
    for hs, ws in ((7, 9), (8, 8), (33, 51)):
        s = rng.integers(0, 256, (hs, ws)).astype(np.uint8)
        b = R.blocks(s)
        assert b.shape == (10 * hs, 10 * ws, 3) and b.dtype == np.uint8 and b.flags.c_contiguous
        assert np.array_equal(cexact.gray_small(b, hs, ws), s)


@pytest.mark.parametrize("hs,ws", list(MEASURED))
def test_oracle_recovers_rotation_shift_and_photometric_change(hs, ws):
    """Measured with this generator (scene seed 7, the three motions of cmc_ref.MOTIONS, the last with gain 0.7 and bias 20):
        72 x 128: angle error up to 3.3e-5 rad, shift error up to 0.0059 px, 4 to 6 iterations
        48 x 64:  angle error up to 9.9e-5 rad, shift error up to 0.0114 px, 4 to 5 iterations
        33 x 51:  angle error up to 3.3e-4 rad, shift error up to 0.0143 px, 4 to 5 iterations
    The bound is three times the size's figure (the factor absorbs another interpolation of the synthetic input, not the solver),
    never above 2e-3 rad and 0.05 px.  The truth is the full-frame motion seen from the small image (cmc_ref.small_motion: the
    small pixels sit at 10 x + 4.5, so a rotation about the frame's origin also shifts the small image by up to 0.03 px here)."""
    a_bound, t_bound = min(3 * MEASURED[hs, ws][0], 2e-3), min(3 * MEASURED[hs, ws][1], 0.05)
    sc = R.scene(10 * hs, 10 * ws, SEED)
    T = cexact.gray_small(R.warped(sc, 0, 0, 0), hs, ws)
    for theta, tx, ty, gain, bias in R.MOTIONS:
        I = cexact.gray_small(R.warped(sc, theta, 10 * tx, 10 * ty, gain, bias), hs, ws)
        w, it = cexact.ecc(T, I)
        eth, etx, ety = R.small_motion(theta, 10 * tx, 10 * ty)
        ang = np.arctan2(w[1, 0], w[0, 0])
        print(f"{hs}x{ws} theta {theta}: it {it}, angle error {abs(ang - eth):.2e}, shift error {abs(w[0, 2] - etx):.4f} {abs(w[1, 2] - ety):.4f}")
        assert 2 <= it <= 20, (theta, it)
        assert abs(ang - eth) < a_bound, (theta, ang - eth)
        assert abs(w[0, 2] - etx) < t_bound and abs(w[1, 2] - ety) < t_bound, (theta, w[0, 2] - etx, w[1, 2] - ety)
        assert w[0, 0] == w[1, 1] and w[0, 1] == -w[1, 0] and abs(w[0, 0] ** 2 + w[1, 0] ** 2 - 1) < 1e-12      # a rotation matrix


def test_sincos_over_the_range_runs_wander_in():
    for t in np.linspace(-1.2, 1.2, 49):
        s, c = cexact.sincos(t)
        assert abs(s - np.sin(t)) < 1e-13 and abs(c - np.cos(t)) < 1e-13, t


def tiny(hs, ws, seed=0):
    """An hs x (ws + 1) grey texture to cut hs x ws small images from."""
    return _texture(hs, ws + 1, seed)[:hs, :ws + 1].astype(np.uint8)


def test_every_exit_is_reachable():
    a = tiny(8, 8)
    assert cexact.ecc(a[:, :8], a[:, :8])[1] == 2                 # exactly 64 samples: converged at the second look
    b = tiny(7, 9)
    assert cexact.ecc(b[:, :9], b[:, :9])[1] == -1                # 63 samples
    c = tiny(8, 9)
    assert cexact.ecc(c[:, :9], c[:, :9])[1] == 2                 # 72 samples ...
    assert cexact.ecc(c[:, :9], c[:, 1:10])[1] == -1              # ... and fewer than 64 after the first update of a one-pixel shift
    T, I = _pair(72, 128, EXIT_SEED, 0.03, 15, -10)
    assert cexact.ecc(T, I)[1] >= 2 and cexact.ecc(255 - T, 255 - I)[1] >= 2
    assert cexact.ecc(T, 255 - T)[1] == -1 and cexact.ecc(T, 255 - I)[1] == -1       # anti-correlated: no positive scale
    T, I = _pair(72, 128, EXIT_SEED, 0.6, 100, 100)               # (10, 10) small pixels and 0.6 rad: out of reach
    assert cexact.ecc(T, I)[1] == -1
    flat = np.full((72, 128), 90, np.uint8)
    assert cexact.ecc(T, flat)[1] == -1 and cexact.ecc(flat, T)[1] == -1
    T, I = _pair(33, 51, EXIT_SEED, *CAP_PAIR)
    w, it = cexact.ecc(T, I)
    assert it == 100 and not np.array_equal(w, [[1, 0, 0], [0, 1, 0]])               # the cap: the last iterate is returned


def _by_hand(prev, cur):
    """test_gpu_cmc._oracle_warp, written out again"""
    H, W = cur.shape[:2]
    hs, ws = int(H * 0.1), int(W * 0.1)
    w, it = cexact.ecc(cexact.gray_small(prev, hs, ws), cexact.gray_small(cur, hs, ws))
    out = np.array([1.0, 0, 0, 0, 1, 0, -1, 0])
    if it >= 0:
        out[:6], out[6] = w.reshape(6), it
        out[2] *= W / ws; out[5] *= H / hs
    return out


def test_eccref_bookkeeping():
    F, S, H, W = 4, 2, 120, 160
    ID = np.array([1.0, 0, 0, 0, 1, 0, -1, 0])
    rng = np.random.default_rng(5)
    scs = [R.scene(H, W, 30 + s) for s in range(S)]

    def group(h=H, w=W, scenes=scs):
        return np.stack([np.stack([R.warped(scenes[s], rng.uniform(-0.03, 0.03), rng.uniform(-6, 6), rng.uniform(-6, 6))[:h, :w]
                                   for s in range(S)]) for _ in range(F)])

    ref = R.EccRef(S)
    a = group()
    out = ref.estimate(a)                                         # the first call: no predecessor
    assert out.shape == (F, S, 8)
    for s in range(S):
        assert np.array_equal(out[0, s], ID)
        for f in range(1, F):
            assert np.array_equal(out[f, s], _by_hand(a[f - 1, s], a[f, s]))
    assert (out[1:, :, 6] >= 2).all()
    b = group()
    out = ref.estimate(b, n_valid=F - 1)                          # the last frame is stale
    for s in range(S):
        assert np.array_equal(out[0, s], _by_hand(a[F - 1, s], b[0, s])) and out[0, s, 6] >= 2
        assert np.array_equal(out[2, s], _by_hand(b[1, s], b[2, s])) and np.array_equal(out[F - 1, s], ID)
    c = group()
    out = ref.estimate(c, n_valid=0)                              # no real frame: nothing estimated, nothing forgotten
    assert np.array_equal(out, np.tile(ID, (F, S, 1)))
    d = group()
    out = ref.estimate(d, n_valid=1)
    for s in range(S):
        assert np.array_equal(out[0, s], _by_hand(b[F - 2, s], d[0, s])) and out[0, s, 6] >= 2
        assert np.array_equal(out[1:, s], np.tile(ID, (F - 1, 1)))
    e = group()
    out = ref.estimate(e, n_valid=F + 1)                          # more than the call holds: all of it
    for s in range(S):
        assert np.array_equal(out[0, s], _by_hand(d[0, s], e[0, s]))
        assert np.array_equal(out[F - 1, s], _by_hand(e[F - 2, s], e[F - 1, s]))
    g = group()
    out = ref.estimate(g, n_valid=F)
    for s in range(S):
        assert np.array_equal(out[0, s], _by_hand(e[F - 1, s], g[0, s])) and np.array_equal(out[1, s], _by_hand(g[0, s], g[1, s]))
    assert np.array_equal(ref.prev[1], cexact.gray_small(g[F - 1, 1], 12, 16)) and np.array_equal(ref.smalls[2][0], cexact.gray_small(g[2, 0], 12, 16))
    ref.reset(1)                                                  # one stream of two
    h = group()
    out = ref.estimate(h)
    assert np.array_equal(out[0, 0], _by_hand(g[F - 1, 0], h[0, 0])) and out[0, 0, 6] >= 2 and np.array_equal(out[0, 1], ID)
    assert np.array_equal(out[1, 1], _by_hand(h[0, 1], h[1, 1]))
    i = group(100, 130)                                           # another frame size: every predecessor is forgotten
    out = ref.estimate(i)
    assert np.array_equal(out[0], np.tile(ID, (S, 1))) and np.array_equal(out[1, 0], _by_hand(i[0, 0], i[1, 0]))
    j = group()
    out = ref.estimate(j)                                         # and back
    assert np.array_equal(out[0], np.tile(ID, (S, 1))) and np.array_equal(out[1, 1], _by_hand(j[0, 1], j[1, 1]))
    ref.reset()
    assert np.array_equal(ref.estimate(group())[0], np.tile(ID, (S, 1)))
