"""The JPEG front door without a GPU: the NumPy restatement of docs/JPEG.md §2 (tests/jpeg_ref.py) against Pillow's stored and
live decodes, the library's host entropy stage against the restatement, the stream splitter, the Python surface and the CLI."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from strongsort_yolo_amd import cli, jpeg, lib
from tests import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def cases():
    z = np.load(os.path.join(GOLD, "jpeg_cases.npz"))
    return [(str(n), z[f"bytes_{i}"].tobytes(), z[f"rgb_{i}"]) for i, n in enumerate(z["names"])]


@pytest.fixture(scope="module")
def sequence():
    z = np.load(os.path.join(GOLD, "jpeg_sequence.npz"))
    return [(z[f"bytes_{i}"].tobytes(), z[f"rgb_{i}"]) for i in range(12)]


@pytest.fixture(scope="module")
def refused():
    z = np.load(os.path.join(GOLD, "jpeg_refused.npz"))
    return z["good"].tobytes(), z["good_rgb"], {k: (z[k].tobytes(), v) for k, v in (str(c).split("=") for c in z["causes"])}


@pytest.fixture(scope="module")
def L():
    lib.build()
    return lib.load()


def test_case_matrix_is_the_one_the_fixtures_promise(cases):
    names = [c[0] for c in cases]
    for size in ("1x1", "8x8", "3x5", "4x9", "17x9", "33x31", "61x45", "130x70"):
        for kind in ("photo", "noise", "flat", "synth"):
            for sub in ("444", "422", "420", "grey"):
                assert any(n.startswith(f"{size}_{kind}_{sub}_") for n in names)
    for tag in ("_q30", "_q90", "_q100", "_opt", "_rst"):
        assert sum(tag in n for n in names) >= 20
    for f in ("jpeg_cases.npz", "jpeg_sequence.npz", "jpeg_refused.npz"):
        assert os.path.getsize(os.path.join(GOLD, f)) <= 1 << 20


def test_reference_equals_every_stored_array_in_int32_and_int64(cases, sequence):
    for name, data, rgb in cases + [(f"sequence {i}", d, a) for i, (d, a) in enumerate(sequence)]:
        got = jpeg_ref.decode(data)
        assert np.array_equal(got, rgb), name
        assert np.array_equal(jpeg_ref.decode(data, dtype=np.int64), got), name        # no intermediate leaves int32
        assert np.array_equal(jpeg_ref.decode(data, rgb=False), rgb[:, :, ::-1]), name


def test_reference_equals_pillow_live_on_a_wider_matrix():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(77)
    sizes = [(w, h) for w in (2, 3, 4, 5, 6, 7) for h in (1, 2, 7, 18)] + [(16, 16), (24, 8), (31, 33), (47, 29), (64, 48), (99, 35)]
    n = 0
    for k, (w, h) in enumerate(sizes):
        smooth = np.clip(np.add.outer(np.arange(h) * 5.0, np.arange(w) * 3.0)[:, :, None] + rng.normal(0, 12, (h, w, 3)) + [20, 90, 160], 0, 255).astype(np.uint8)
        for arr in (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), smooth):
            for sub in ("4:4:4", "4:2:2", "4:2:0", "grey"):
                q = (30, 90, 100, 75)[n % 4]
                kw = {} if sub == "grey" else {"subsampling": sub}
                if n % 3 == 1:
                    kw["restart_marker_blocks"] = 1 + n % 4
                buf = io.BytesIO()
                (Image.fromarray(arr).convert("L") if sub == "grey" else Image.fromarray(arr)).save(buf, "JPEG", quality=q, optimize=n % 2 == 1, **kw)
                data = buf.getvalue()
                want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
                got = jpeg_ref.decode(data)
                assert np.array_equal(got, want), (w, h, sub, q, kw)
                assert np.array_equal(jpeg_ref.decode(data, dtype=np.int64), got)
                n += 1
    assert n == len(sizes) * 8


def _coefficients(L, data, cap):
    coef, quant = np.full(cap, 12345, np.int16), np.zeros((4, 64), np.uint16)
    rc = L.ss_jpeg_coefficients(data, len(data), coef.ctypes.data_as(C.POINTER(C.c_short)), cap, quant.ctypes.data_as(C.POINTER(C.c_ushort)))
    return rc, coef, quant


def test_library_coefficients_and_tables_equal_the_reference(L, cases, sequence):
    for name, data, _ in cases + [(f"sequence {i}", d, a) for i, (d, a) in enumerate(sequence)]:
        coefs, quant, _ = jpeg_ref.coefficients(data)
        want = np.concatenate([c.reshape(-1) for c in coefs])
        rc, coef, q = _coefficients(L, data, want.size)
        assert rc == lib.SS_OK, (name, L.ss_last_error(None))
        assert np.array_equal(coef, want) and np.array_equal(q, quant), name
    _, data, _ = cases[-1]
    rc, coef, _ = _coefficients(L, data, 64)                                   # too small a buffer: refused, nothing written
    assert rc == lib.SS_ERR_INVALID and b"too small" in L.ss_last_error(None) and (coef == 12345).all()


def test_probe_values(cases):
    sampling = {"444": (3, (1, 1)), "422": (3, (2, 1)), "420": (3, (2, 2)), "grey": (1, (1, 1))}
    for name, data, rgb in cases:
        h, w, nc, hv = jpeg.probe(data)
        assert (h, w) == rgb.shape[:2] and (nc, hv) == sampling[name.split("_")[2]], name


def test_every_refusal_names_its_cause(L, refused):
    good, good_rgb, bad = refused
    assert jpeg.probe(good) == (48, 64, 3, (2, 1))
    for name, (data, cause) in bad.items():
        with pytest.raises(jpeg_ref.Refused, match=re.escape(cause)):
            jpeg_ref.decode(data)
        rc, _, _ = _coefficients(L, data, 1 << 16)
        assert rc == lib.SS_ERR_INVALID and cause.encode() in L.ss_last_error(None), name
        if name in ("cut_scan", "bad_restart"):                                # the headers are fine: only the scan shows it
            assert jpeg.probe(data)[:2] == (48, 64)
        else:
            with pytest.raises(ValueError, match=re.escape(cause)):
                jpeg.probe(data)
    for data, cause in ((b"", "null argument"), (b"\x00\x01\x02\x03\x04", "no SOI"), (good[:30], "no scan|truncated")):
        with pytest.raises(ValueError, match=cause):
            jpeg.probe(data)
    hacked = bytearray(good)                                                   # an extended-sequential frame header, 12-bit samples
    sof = good.index(b"\xff\xc0")
    hacked[sof + 4] = 12
    with pytest.raises(ValueError, match="12-bit"):
        jpeg.probe(bytes(hacked))
    hacked = bytearray(good)
    hacked[sof + 1] = 0xC1
    with pytest.raises(ValueError, match="extended sequential"):
        jpeg.probe(bytes(hacked))
    dht = good.index(b"\xff\xc4")                                              # drop the first Huffman table: a missing table
    ln = (good[dht + 2] << 8) | good[dht + 3]
    with pytest.raises(ValueError, match="missing DC Huffman table 0"):
        jpeg.probe(good[:dht] + good[dht + 2 + ln:])


def test_null_arguments_without_a_context(L):
    n = C.c_int()
    assert L.ss_jpeg_probe(None, 10, n, n, n, n, n) == lib.SS_ERR_INVALID
    assert L.ss_jpeg_probe(b"abc", 3, None, n, n, n, n) == lib.SS_ERR_INVALID
    assert L.ss_jpeg_coefficients(None, 0, None, 0, None) == lib.SS_ERR_INVALID
    assert L.ss_jpeg_decode_batch(None, None, None, None, 1, 8, 8, None, 192, 0, 1) == lib.SS_ERR_INVALID
    assert b"ss_jpeg_decode_batch" in L.ss_last_error(None)


def test_declarations_exports_and_argtypes(L):
    src = open(os.path.join(ROOT, "include", "strongsort_hip.h")).read()
    for name, nargs in (("ss_jpeg_probe", 7), ("ss_jpeg_coefficients", 5), ("ss_jpeg_decode_batch", 11)):
        assert re.search(r"\bint %s\(" % name, src) and name in lib.EXPORTS
        fn = getattr(L, name)
        assert len(fn.argtypes) == nargs and fn.restype is C.c_int


def test_encoded_frame(cases, refused):
    name, data, rgb = cases[-1]
    f = jpeg.EncodedFrame(np.frombuffer(data, np.uint8))
    assert f.shape == rgb.shape and f.data == data and len(f) == len(data) and isinstance(f.data, bytes)
    with pytest.raises(ValueError, match="progressive"):
        jpeg.EncodedFrame(refused[2]["progressive"][0])


def test_split_mjpeg(tmp_path, sequence, refused):
    good = refused[0]
    soi = good[:2]
    tricky = soi + b"\xff\xe1\x00\x08" + b"ab\xff\xd9cd" + b"\xff\xfe\x00\x06\xff\xd8\xff\xd9" + good[2:]     # FFD9 / FFD8 inside APP1 and COM data
    assert jpeg.probe(tricky) == jpeg.probe(good)
    files = [d for d, _ in sequence[:3]] + [tricky, sequence[3][0]]
    blob = b"".join(files)
    got = list(jpeg.split_mjpeg(blob))
    assert [g.data for g in got] == files
    path = tmp_path / "clip.mjpeg"
    path.write_bytes(b"junk" + blob + b"\xff\xd8\xff\xe0")                                                   # a cut last frame is dropped
    assert [g.data for g in jpeg.split_mjpeg(str(path))] == files
    assert list(jpeg.split_mjpeg(b"")) == []


def _jpeg_dir(tmp_path, sequence, n=5):
    d = tmp_path / "frames"
    d.mkdir()
    for i in range(n):
        (d / f"f_{i:03d}.jpg").write_bytes(sequence[i][0])
    return d


def test_frame_source_encoded(tmp_path, sequence):
    d = _jpeg_dir(tmp_path, sequence)
    got = list(cli.frame_source(str(d), encoded=True))
    assert all(isinstance(g, jpeg.EncodedFrame) for g in got) and [g.data for g in got] == [s[0] for s in sequence[:5]]
    assert len(list(cli.frame_source(str(d), 2, encoded=True))) == 2
    clip = tmp_path / "clip.mjpg"
    clip.write_bytes(b"".join(s[0] for s in sequence[:4]))
    assert [g.data for g in cli.frame_source(str(clip), encoded=True, limit=3)] == [s[0] for s in sequence[:3]]
    (d / "extra.png").write_bytes(b"not a jpeg")
    with pytest.raises(ValueError, match="only"):
        list(cli.frame_source(str(d), encoded=True))
    with pytest.raises(ValueError, match="neither"):
        list(cli.frame_source("synthetic:3", encoded=True))


def test_mjpeg_source_without_the_flag_decodes_through_pillow(tmp_path, sequence):
    pytest.importorskip("PIL")
    clip = tmp_path / "clip.mjpeg"
    clip.write_bytes(b"".join(s[0] for s in sequence[:3]))
    got = list(cli.frame_source(str(clip)))
    assert len(got) == 3 and all(np.array_equal(g, s[1][:, :, ::-1]) for g, s in zip(got, sequence))


def test_cli_flag(tmp_path, sequence, refused, monkeypatch, capsys):
    monkeypatch.setattr(cli, "process_video", lambda job: job)
    d = _jpeg_dir(tmp_path, sequence)
    (job,) = cli.main(["--source", str(d), "--track", "--tracker", "bytetrack", "--device-decode"])
    assert job["device_decode"] is True
    (job,) = cli.main(["--source", str(d), "--track"])
    assert job["device_decode"] is False
    for argv in (["--source", str(d), "--device-decode"],                                    # no --track
                 ["--source", str(d), "--track", "--batch", "1", "--device-decode"],
                 ["--source", "synthetic:3", "--track", "--device-decode"]):
        with pytest.raises(SystemExit):
            cli.main(argv)
    capsys.readouterr()
    bad = tmp_path / "bad"
    bad.mkdir()
    (bad / "a.jpg").write_bytes(refused[2]["progressive"][0])
    with pytest.raises(SystemExit):
        cli.main(["--source", str(bad), "--track", "--device-decode"])
    err = capsys.readouterr().err
    assert "a.jpg" in err and "progressive" in err


def test_track_and_predict_refuse_encoded_frames(sequence):
    from strongsort_yolo_amd.yolo import YOLO
    model = YOLO("yolov8n.pt", random_init_ok=True, tracker_type="bytetrack")
    f = jpeg.EncodedFrame(sequence[0][0])
    for call in (lambda x: model.track(x, tracker="bytetrack.yaml"), model.predict):
        with pytest.raises(TypeError, match="track_stream.*jpeg.decode"):
            call(f)


def _segment(data, marker, nth=0):
    """(offset of the FF, segment length field) of the nth `marker` segment before the scan."""
    at = -1
    for _ in range(nth + 1):
        at = data.index(bytes([0xFF, marker]), at + 1)
    return at, (data[at + 2] << 8) | data[at + 3]


def _malformed(good):
    """Hand-made malformed headers of the fixture `good` (4:2:2, two DQT, four DHT segments) and the cause each must be refused with."""
    out = {}
    dht, ln = _segment(good, 0xC4, 1)                                  # the first AC table
    assert good[dht + 4] == 0x10
    for name, counts in (("dht_162_codes_of_length_1", [162] + [0] * 15), ("dht_3_codes_of_length_1", [3] + [0] * 15),
                         ("dht_5_codes_of_length_2", [0, 5] + [0] * 14), ("dht_kraft_excess_at_length_9", [1, 1, 1, 1, 1, 1, 1, 1, 3] + [0] * 7)):
        syms = bytes(range(sum(counts)))
        out[name] = (good[:dht + 2] + (19 + len(syms)).to_bytes(2, "big") + b"\x10" + bytes(counts) + syms + good[dht + 2 + ln:], "bad Huffman table")
    out["dht_counts_beyond_the_segment"] = (good[:dht + 5] + bytes([255]) + good[dht + 6:], "bad Huffman table")
    out["dht_class_2"] = (good[:dht + 4] + b"\x20" + good[dht + 5:], "bad Huffman table")
    out["dht_table_7"] = (good[:dht + 4] + b"\x17" + good[dht + 5:], "bad Huffman table")
    out["dht_short_segment"] = (good[:dht + 2] + (10).to_bytes(2, "big") + good[dht + 4:dht + 12] + good[dht + 2 + ln:], "bad Huffman table")
    dqt, ln = _segment(good, 0xDB)
    out["dqt_table_5"] = (good[:dqt + 4] + b"\x05" + good[dqt + 5:], "bad quantisation table")
    out["dqt_short_segment"] = (good[:dqt + 2] + (40).to_bytes(2, "big") + good[dqt + 4:dqt + 42] + good[dqt + 2 + ln:], "bad quantisation table")
    out["segment_length_1"] = (good[:dqt + 2] + b"\x00\x01" + good[dqt + 4:], "truncated header")
    out["segment_length_past_the_end"] = (good[:dqt + 2] + b"\xff\xf0" + good[dqt + 4:], "truncated header")
    sof, ln = _segment(good, 0xC0)
    out["sof_zero_width"] = (good[:sof + 7] + b"\x00\x00" + good[sof + 9:], "sides must be")
    out["sof_height_9000"] = (good[:sof + 5] + (9000).to_bytes(2, "big") + good[sof + 7:], "sides must be")
    out["sof_component_count_mismatch"] = (good[:sof + 9] + b"\x02" + good[sof + 10:], "bad frame header")
    out["sof_table_4"] = (good[:sof + 12] + b"\x04" + good[sof + 13:], "missing quantisation table 4")
    out["sof_twice"] = (good[:sof] + good[sof:sof + 2 + ln] + good[sof:], "two frame headers")
    sos, ln = _segment(good, 0xDA)
    assert ln == 12 and good[sos + 11:sos + 14] == b"\x00\x3f\x00"
    out["sos_before_sof"] = (good[:sof] + good[sof + 2 + _segment(good, 0xC0)[1]:], "scan before the frame header")
    out["sos_two_components"] = (good[:sos + 2] + b"\x00\x0a\x02" + good[sos + 5:sos + 9] + good[sos + 11:], "several scans")
    out["sos_huffman_table_3"] = (good[:sos + 6] + b"\x33" + good[sos + 7:], "missing DC Huffman table 3")
    out["sos_se_62"] = (good[:sos + 12] + b"\x3e" + good[sos + 13:], "not a baseline one")
    out["sos_ss_1"] = (good[:sos + 11] + b"\x01" + good[sos + 12:], "not a baseline one")
    out["sos_al_1"] = (good[:sos + 13] + b"\x01" + good[sos + 14:], "not a baseline one")
    out["sos_components_swapped"] = (good[:sos + 5] + good[sos + 7:sos + 9] + good[sos + 5:sos + 7] + good[sos + 9:], "scan components out of order")
    dri = b"\xff\xdd\x00\x05\x00\x00\x04"
    out["dri_length_5"] = (good[:sos] + dri + good[sos:], "bad restart interval")
    out["no_scan_at_all"] = (good[:sos] + b"\xff\xd9", "no scan")
    return out


def test_malformed_headers_are_refused_by_the_library_and_the_reference(L, refused):
    """Headers an encoder never writes.  The first cases are Huffman tables with more codes of a length than the code space holds:
    the look-up table must not be written before that is seen (162 codes of length 1 would index it 80 kB past its end)."""
    good = refused[0]
    cases = _malformed(good)
    assert len(cases) == 26
    for name, (data, cause) in cases.items():
        with pytest.raises(ValueError, match=re.escape(cause)):
            jpeg.probe(data)
        rc, coef, _ = _coefficients(L, data, 1 << 16)
        assert rc == lib.SS_ERR_INVALID and cause.encode() in L.ss_last_error(None), (name, L.ss_last_error(None))
        with pytest.raises(jpeg_ref.Refused, match=re.escape(cause)):
            jpeg_ref.parse(data)
    assert jpeg.probe(good) == (48, 64, 3, (2, 1))                     # and the library goes on working
    rc, _, _ = _coefficients(L, good, 1 << 16)
    assert rc == lib.SS_OK


def test_scan_data_that_no_table_explains_is_refused(L, refused):
    """A valid but sparse table (one 1-bit code) over real scan data: codes that do not exist, or indices beyond 63; and every
    byte-wise truncation of a small file is refused or decoded, never anything else."""
    good = refused[0]
    dht, ln = _segment(good, 0xC4, 1)
    data = good[:dht + 2] + (20).to_bytes(2, "big") + b"\x10" + bytes([1] + [0] * 15) + b"\x11" + good[dht + 2 + ln:]
    assert jpeg.probe(data)[:2] == (48, 64)
    rc, _, _ = _coefficients(L, data, 1 << 16)
    msg = L.ss_last_error(None)
    assert rc == lib.SS_ERR_INVALID and (b"does not exist" in msg or b"beyond 63" in msg or b"data ends" in msg), msg
    with pytest.raises(jpeg_ref.Refused):
        jpeg_ref.coefficients(data)
    for cut in range(0, len(good), 7):
        rc, _, _ = _coefficients(L, good[:cut] or b"\x00", 1 << 16)
        assert rc == lib.SS_ERR_INVALID, cut
