"""The device entropy stage of the JPEG decoder without a GPU (docs/JPEG.md §12): its NumPy restatement (tests/jpeg_huff_ref.py)
against the host decoder's coefficients on every fixture, the host's scan cut (ss_jpeg_scan_segments) against the restatement's,
the derived entry bound, the refusals and the argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from strongsort_yolo_amd import cli, jpeg, lib
from tests import jpeg_huff_ref as ref
from tests.jpeg_ref import Refused

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ("jpeg_cases.npz", "jpeg_sequence.npz", "jpeg_entropy_cases.npz")


def _load(name):
    z = np.load(os.path.join(GOLD, name))
    n = len([k for k in z.files if k.startswith("bytes_")])
    names = [str(x) for x in z["names"]] if "names" in z.files else [f"{name} {i}" for i in range(n)]
    return [(names[i], z[f"bytes_{i}"].tobytes()) for i in range(n)]


@pytest.fixture(scope="module")
def L():
    lib.build()
    return lib.load()


@pytest.fixture(scope="module")
def refused():
    z = np.load(os.path.join(GOLD, "jpeg_refused.npz"))
    return z["good"].tobytes(), {k: (z[k].tobytes(), v) for k, v in (str(c).split("=") for c in z["causes"])}


def _host_coefficients(L, data):
    h, w, nc, (hs, vs) = jpeg.probe(data)
    cap = -(-w // (8 * hs)) * -(-h // (8 * vs)) * 64 * (1 if nc == 1 else hs * vs + 2)
    coef, quant = np.zeros(cap, np.int16), np.zeros((4, 64), np.uint16)
    rc = L.ss_jpeg_coefficients(data, len(data), coef.ctypes.data_as(C.POINTER(C.c_short)), cap, quant.ctypes.data_as(C.POINTER(C.c_ushort)))
    assert rc == lib.SS_OK, L.ss_last_error(None)
    return coef


_ratio = {}


@pytest.mark.parametrize("fname", FILES)
def test_reference_equals_the_host_decoder_and_its_rounds_stay_below_the_lanes(L, fname):
    worst = (0.0, "")
    for name, data in _load(fname):
        want = _host_coefficients(L, data)
        for W in (4, 32):
            st = ref.stream(data, W)
            coef, rounds, status = ref.finish(st)
            assert status is None and np.array_equal(coef, want), (name, W, status)
            raw, segs = ref.cut(data)
            lanes = sum(max(1, -(-s[1] // (4 * W))) for s in segs)
            assert len(rounds) == -(-lanes // ref.LANES), (name, W)
            for t, r in enumerate(rounds):
                assert 1 <= r <= min(ref.LANES, lanes - t * ref.LANES), (name, W, t, r)
            entries, bound = ref.entry_count(st)                              # an AC entry costs at least 2 bits of scan
            assert entries <= bound == len(want) // 64 + 4 * sum(s[1] for s in segs), (name, entries, bound)
            worst = max(worst, (entries / bound, name))
    print(f"{fname}: largest entries / bound {worst[0]:.3f} ({worst[1]})")


def test_a_small_tile_carries_state_blocks_and_entries_into_the_next(L):
    """Tiles of 7 and 64 lanes on files with and without restart markers: the carry is the same code path as 1024 lanes."""
    picks = [c for c in _load("jpeg_cases.npz") if c[0].startswith(("33x31_noise", "61x45_photo"))][:12] + _load("jpeg_entropy_cases.npz")[1:]
    assert any("_rst" in n for n, _ in picks)
    for name, data in picks:
        want = _host_coefficients(L, data)
        for lanes in (7, 64):
            coef, rounds, status = ref.decode(data, 4, lanes)
            assert status is None and np.array_equal(coef, want), (name, lanes)


@pytest.mark.parametrize("fname", FILES)
def test_scan_segments_equal_the_reference_cut(fname):
    for name, data in _load(fname):
        raw, segs, hdr = jpeg.scan_segments(data)
        want_raw, want_segs = ref.cut(data)
        assert raw == want_raw, name
        assert np.array_equal(segs, np.array(want_segs, np.uint32).reshape(-1, 4)), name
        h, w, nc, (hs, vs) = jpeg.probe(data)
        assert hdr[0] == nc and (hdr[1], hdr[2]) == (hs, vs) and hdr[17] == len(want_segs), name
        assert hdr[4] == sum(s[3] for s in want_segs) and all(s[0] % 4 == 0 for s in want_segs), name


def test_entropy_fixtures_are_what_they_promise():
    cases = dict(_load("jpeg_entropy_cases.npz"))
    raw, segs = ref.cut(cases["noise_224x160_444_q100"])
    assert len(segs) == 1 and segs[0][1] > 4 * 32 * ref.LANES                   # more than one tile at W = 32
    for n in ("rst1_61x45_420_q50", "rst1_61x45_grey_q90"):
        raw, segs = ref.cut(cases[n])
        assert len(segs) > 1 and max(s[1] for s in segs) < 4 * 32               # every segment shorter than a subsequence
    info = ref.parse(cases["opt_48x32_444_q100"])
    assert max(ln for t in list(info["dc"].values()) + list(info["ac"].values()) for (ln, _) in t) > 9


def test_refusals(L, refused):
    good, bad = refused
    for name, (data, cause) in bad.items():
        if name == "cut_scan":                                               # sound headers, sound cut: only decoding shows it
            raw, segs, hdr = jpeg.scan_segments(data)
            assert (raw, [tuple(s) for s in segs.tolist()]) == ref.cut(data)
            coef, rounds, status = ref.decode(data)
            assert status == cause == "data ends before the last MCU" and not coef.any()
            continue
        with pytest.raises(ValueError, match=re.escape(cause)):
            jpeg.scan_segments(data)
        with pytest.raises(Refused, match=re.escape(cause)):
            ref.cut(data)
    used, nseg = C.c_size_t(), C.c_int()
    assert L.ss_jpeg_scan_segments(None, 0, None, 0, C.byref(used), None, 0, C.byref(nseg), None) == lib.SS_ERR_INVALID
    buf = np.zeros(8, np.uint8)
    seg = np.zeros(4, np.uint32)
    assert L.ss_jpeg_scan_segments(good, len(good), buf.ctypes.data, 8, C.byref(used), seg.ctypes.data, 1, C.byref(nseg), None) == lib.SS_ERR_INVALID
    assert b"too small" in L.ss_last_error(None) and not buf.any()


def test_damaged_scans_take_the_total_continuations(refused):
    """Every byte-wise truncation and a few overwritten scans of a small file: the restatement ends, within its round bound, with
    a status or with coefficients; the causes are the documented ones."""
    good = refused[0]
    info = ref.parse(good)
    rng = np.random.default_rng(7)
    seen = set()
    for k in range(12):
        bad = bytearray(good)
        at = info["scan"] + int(rng.integers(0, len(good) - info["scan"] - 2))
        for q in range(at, min(at + 6, len(good) - 2)):
            bad[q] = int(rng.integers(0, 255))                                # (never FF: the cut stays the same shape)
        coef, rounds, status = ref.decode(bytes(bad), 4)
        seen.add(status)
        assert status is None or (status in ref.CAUSES.values() and not coef.any())
    for cutat in range(info["scan"] + 1, len(good) - 2, 37):
        coef, rounds, status = ref.decode(good[:cutat], 4)
        assert status == "data ends before the last MCU", cutat
    assert len(seen) > 1


def test_argument_errors(tmp_path, monkeypatch, capsys):
    with pytest.raises(ValueError, match="entropy"):
        jpeg.decode(None, [], entropy="gpu")
    from strongsort_yolo_amd.engine import TrackerEngine
    with pytest.raises(ValueError, match="entropy"):
        TrackerEngine.jpeg_decode_batch(None, None, [], entropy="gpu")
    from strongsort_yolo_amd.yolo import YOLO
    with pytest.raises(ValueError, match="jpeg_entropy"):
        next(YOLO.track_stream(None, [], jpeg_entropy="gpu"))
    monkeypatch.setattr(cli, "process_video", lambda job: job)
    d = tmp_path / "frames"
    d.mkdir()
    for i, (_, data) in enumerate(_load("jpeg_sequence.npz")[:2]):
        (d / f"{i:03d}.jpg").write_bytes(data)
    (job,) = cli.main(["--source", str(d), "--track", "--tracker", "bytetrack", "--device-decode", "--device-entropy"])
    assert job["device_decode"] is True and job["device_entropy"] is True
    (job,) = cli.main(["--source", str(d), "--track", "--tracker", "bytetrack", "--device-decode"])
    assert job["device_entropy"] is False
    with pytest.raises(SystemExit):
        cli.main(["--source", str(d), "--track", "--device-entropy"])
    assert "--device-decode" in capsys.readouterr().err


def test_option_and_exports(L):
    for w in (4, 8, 16, 32):
        assert L.ss_op_set_option(b"jpeg_subseq_words", w) == lib.SS_OK
    for w in (0, 3, 64, -4):
        assert L.ss_op_set_option(b"jpeg_subseq_words", w) == lib.SS_ERR_INVALID
    src = open(os.path.join(os.path.dirname(GOLD), "..", "include", "strongsort_hip.h")).read()
    for name, nargs in (("ss_jpeg_decode_batch_device", 11), ("ss_jpeg_scan_segments", 9), ("ss_jpeg_device_coefficients", 5), ("ss_jpeg_device_rounds", 3)):
        assert re.search(r"\bint %s\(" % name, src) and name in lib.EXPORTS
        assert len(getattr(L, name).argtypes) == nargs
    assert L.ss_jpeg_decode_batch_device(None, None, None, None, 1, 8, 8, None, 192, 0, 1) == lib.SS_ERR_INVALID
    assert L.ss_jpeg_device_coefficients(None, b"ab", 2, None, 0) == lib.SS_ERR_INVALID
