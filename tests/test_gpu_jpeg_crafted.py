"""The device JPEG decoder (csrc/ss_jpeg.hip: k_jpeg_idct, k_jpeg_pixels, k_jpeg_huff, k_jpeg_dc) on input no encoder writes.

Crafted files (tests/jpeg_crafted.py): coefficients whose IDCT wraps int32 and reaches all four zones of the range limit, and
blocks whose padding samples do not repeat the edge.  The expectation is tests/jpeg_ref.py (pixels, int32) and the blocks the files
were written from, never the device's own output.  Damaged scans (tests/golden/jpeg_damaged.npz): the cause, the surviving
neighbours, the rounds and the coefficients, against tests/jpeg_huff_ref.py's stored word and the host decoder."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from strongsort_yolo_amd import fused, jpeg, lib
from tests import jpeg_crafted as jc
from tests import jpeg_ref
from tests.gpu_util import engine

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
STAGES = [("host", 32), ("device", 4), ("device", 32)]                      # (entropy stage, jpeg_subseq_words)
WRAPPING = ("b_max", "d_negative", "f_seed1", "f_seed2", "f_seed3")          # (c_zrl and e_zero hold next to nothing: they stay inside int32)


@pytest.fixture(scope="module")
def eng():
    e = engine(debug=False)
    yield e
    e.close()


@pytest.fixture
def words():
    """Sets the dwords of scan per lane; 32, the default, afterwards."""
    yield lambda w: fused.set_option("jpeg_subseq_words", w)
    fused.set_option("jpeg_subseq_words", 32)


@pytest.fixture(scope="module")
def extreme():
    """The extreme files, after checking that they test what they claim."""
    cases = jc.extreme()
    zones = set()
    for c in cases:
        y = jpeg_ref.prelimit(c.data)
        v = y & 1023
        zones |= set(np.unique(np.select([v < 128, v < 512, v < 896], [0, 1, 2], 3)).tolist())
        if c.name.split("_q")[0] in WRAPPING and "_q1_" in c.name:
            assert not np.array_equal(jc.expect(c).rgb, jpeg_ref.decode(c.data, dtype=np.int64)), f"{c.name}: nothing wraps"
            assert ((y < -512) | (y > 511)).any(), c.name                      # (beyond the span in which the four zones are a plain clamp)
    assert zones == {0, 1, 2, 3}
    return cases


def _differ(eng, cases, entropy, rgb):
    """Names of the cases (one size) whose batch decode differs from tests/jpeg_ref.py, with the count of differing bytes."""
    got = jpeg.decode(eng, [jpeg.EncodedFrame(c.data) for c in cases], rgb=rgb, entropy=entropy).cpu().numpy()
    eng.check_errors()
    bad = []
    for k, c in enumerate(cases):
        want = jc.expect(c).rgb if rgb else jc.expect(c).rgb[:, :, ::-1]
        if not np.array_equal(got[k], want):
            bad.append((c.name, "rgb" if rgb else "bgr", len(cases), int((got[k] != want).sum())))
    return bad


@pytest.mark.parametrize("entropy,W", STAGES)
def test_extreme_coefficients_wrap_and_pass_the_range_limit_like_the_reference(eng, words, extreme, entropy, W):
    words(W)
    assert len(extreme) == 63 and len({(c.hm, c.vm) for c in extreme}) == 3
    bad = []
    for rgb in (False, True):
        bad += _differ(eng, extreme, entropy, rgb)                           # all 63 in one call: three samplings side by side
        for c in extreme:
            bad += _differ(eng, [c], entropy, rgb)
    assert not bad, f"{len(bad)} decodes differ ({entropy}, W = {W}): {bad[:8]}"


@pytest.mark.parametrize("entropy,W", STAGES)
def test_padding_that_does_not_repeat_the_edge_is_never_read(eng, words, entropy, W):
    words(W)
    cases = jc.padding()
    assert len(cases) == 30
    bad = []
    for k in range(0, 30, 3):
        trio = cases[k:k + 3]
        assert len({(c.W, c.H) for c in trio}) == 1 and len({(c.hm, c.vm) for c in trio}) == 3
        for rgb in (False, True):
            bad += _differ(eng, trio, entropy, rgb)                          # one size, three samplings in one call
            for c in trio:
                bad += _differ(eng, [c], entropy, rgb)
    assert not bad, f"{len(bad)} decodes differ ({entropy}, W = {W}): {bad[:8]}"


@pytest.mark.parametrize("entropy,W", STAGES)
def test_crafted_files_at_an_unaligned_out_frame_stride(eng, words, entropy, W):
    words(W)
    for w, h in ((61, 45), (3, 5)):
        trio = [c for c in jc.padding() if (c.W, c.H) == (w, h)]
        each = h * w * 3
        for extra in (64, 5):                                                # 5: frames that are not dword-aligned take the byte stores
            buf = torch.full((3, each + extra), 0xA5, dtype=torch.uint8, device=DEV)
            dst = buf[:, :each].view(3, h, w, 3)
            assert dst.stride(0) == each + extra
            eng.jpeg_decode_batch(dst, [jpeg.EncodedFrame(c.data) for c in trio], entropy=entropy)
            out = buf.cpu().numpy()
            eng.check_errors()
            assert (out[:, each:] == 0xA5).all()
            for k, c in enumerate(trio):
                assert np.array_equal(out[k, :each].reshape(h, w, 3), jc.expect(c).rgb[:, :, ::-1]), (c.name, extra)


@pytest.mark.parametrize("W", [4, 32])
def test_device_coefficients_equal_the_reference_and_the_blocks_the_files_were_written_from(eng, words, extreme, W):
    words(W)
    for c in extreme + jc.padding():
        coef, rounds = jpeg.device_coefficients(eng, c.data)
        assert np.array_equal(coef, jc.expect(c).coef), (c.name, W)
        for k, got, want in jc.known_answer(c, coef):                        # the known answer, at every real block
            assert np.array_equal(got, want), (c.name, W, k)


# ---- damaged scans ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def damaged():
    """([(name, source, bytes, cause, {W: rounds}, rgb or None)], {source: (bytes, rgb)})."""
    z = np.load(os.path.join(GOLD, "jpeg_damaged.npz"))
    cases = [(str(n), str(z["sources"][i]), z[f"bytes_{i}"].tobytes(), str(z["causes"][i]), {4: z[f"rounds4_{i}"].tolist(), 32: z[f"rounds32_{i}"].tolist()},
              z[f"rgb_{i}"] if f"rgb_{i}" in z.files else None) for i, n in enumerate(z["names"])]
    r = np.load(os.path.join(GOLD, "jpeg_refused.npz"))
    sound = {"good": (r["good"].tobytes(), r["good_rgb"])}
    for f in ("jpeg_entropy_cases.npz", "jpeg_cases.npz"):
        s = np.load(os.path.join(GOLD, f))
        for i, n in enumerate(s["names"]):
            if str(n) in {c[1] for c in cases}:
                sound[str(n)] = (s[f"bytes_{i}"].tobytes(), s[f"rgb_{i}"])
    assert {c[1] for c in cases} == set(sound)
    return cases, sound


def _host_coefficients(data, size):
    coef, quant = np.zeros(size, np.int16), np.zeros((4, 64), np.uint16)
    rc = lib.load().ss_jpeg_coefficients(data, len(data), coef.ctypes.data_as(C.POINTER(C.c_short)), size, quant.ctypes.data_as(C.POINTER(C.c_ushort)))
    assert rc == lib.SS_OK
    return coef


@pytest.mark.parametrize("W", [4, 32])
def test_damaged_scans_name_their_cause_or_decode_to_the_stored_pixels(eng, words, damaged, W):
    words(W)
    cases, sound = damaged
    seen = set()
    for name, src, data, cause, rounds, rgb in cases:
        good, good_rgb = sound[src]
        frames = [jpeg.EncodedFrame(good), jpeg.EncodedFrame(data), jpeg.EncodedFrame(good)]
        out = jpeg.decode(eng, frames, rgb=True, entropy="device")            # the headers are sound: nothing is refused here
        if cause:
            with pytest.raises(lib.SSError, match=re.escape("image 1: " + cause)) as e:
                eng.check_errors()
            assert e.value.code == lib.SS_ERR_INVALID, name
            eng.check_errors()                                               # reported once
            got = out.cpu().numpy()
            assert (got[1] == got[1][0, 0]).all(), name                      # every block empty: one flat colour
            with pytest.raises(lib.SSError, match=re.escape(cause)):
                jpeg.device_coefficients(eng, data)
            again = jpeg.decode(eng, frames[:1], rgb=True, entropy="device").cpu().numpy()
            eng.check_errors()                                               # the next call succeeds
            assert np.array_equal(again[0], good_rgb), name
        else:
            eng.check_errors()
            got = out.cpu().numpy()
            assert np.array_equal(got[1], rgb), (name, W, int((got[1] != rgb).sum()))
            coef, got_rounds = jpeg.device_coefficients(eng, data)
            assert np.array_equal(coef, _host_coefficients(data, coef.size)), (name, W)
            assert got_rounds == rounds[W], (name, W, got_rounds, rounds[W])
        assert np.array_equal(got[0], good_rgb) and np.array_equal(got[2], good_rgb), name
        seen.add(cause)
    assert len(seen) == 6                                                    # five causes, and files that decode


def test_the_host_stage_refuses_the_same_files_with_the_same_cause_before_any_launch(eng, damaged):
    cases, sound = damaged
    for name, src, data, cause, rounds, rgb in cases:
        good, good_rgb = sound[src]
        h, w = good_rgb.shape[:2]
        frames = [jpeg.EncodedFrame(good), jpeg.EncodedFrame(data), jpeg.EncodedFrame(good)]
        out = torch.full((3, h, w, 3), 0x5A, dtype=torch.uint8, device=DEV)
        if cause:
            with pytest.raises(lib.SSError, match=re.escape("image 1: " + cause)) as e:
                eng.jpeg_decode_batch(out, frames, rgb=True, entropy="host")
            assert e.value.code == lib.SS_ERR_INVALID, name
            torch.cuda.synchronize()
            assert bool((out == 0x5A).all()), name
        else:
            eng.jpeg_decode_batch(out, frames, rgb=True, entropy="host")
            got = out.cpu().numpy()
            assert np.array_equal(got[1], rgb) and np.array_equal(got[0], good_rgb) and np.array_equal(got[2], good_rgb), name
    eng.check_errors()


@pytest.mark.parametrize("W", [4, 32])
def test_of_two_damaged_images_the_lower_index_is_named(eng, words, damaged, W):
    words(W)
    cases, sound = damaged
    pairs = 0
    for src, (good, good_rgb) in sound.items():
        first = {}
        for c in cases:
            if c[1] == src and c[3]:
                first.setdefault(c[3], c)
        for a, b in zip(list(first.values()), list(first.values())[1:]):     # neighbours in the order of first appearance: different causes
            for x, y in ((a, b), (b, a)):
                out = jpeg.decode(eng, [jpeg.EncodedFrame(good), jpeg.EncodedFrame(x[2]), jpeg.EncodedFrame(y[2])], rgb=True, entropy="device")
                with pytest.raises(lib.SSError, match=re.escape("image 1: " + x[3])):
                    eng.check_errors()
                eng.check_errors()
                assert np.array_equal(out[0].cpu().numpy(), good_rgb), (x[0], y[0])
            pairs += 1
    assert pairs >= 4
