"""The JPEG encoder without a GPU (docs/JPEG.md "Encoding"): the NumPy reference (tests/jpeg_enc_ref.py) against Pillow's stored and
live files, the library's entropy stage and header against the same files, the refusals that need no device, the capacity bound,
the reciprocal the kernel divides with, the sink's kinds and the CLI's flags."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from strongsort_yolo_amd import cli, lib
from tests import jpeg_enc_ref as ref
from tests import jpeg_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def cases():
    return ref.load_cases()


@pytest.fixture(scope="module")
def L():
    lib.build()
    return lib.load()


def _lib_coefficients(L, data, blocks):
    coef, quant = (C.c_short * (blocks * 64))(), (C.c_ushort * 256)()
    assert L.ss_jpeg_coefficients(data, len(data), coef, blocks * 64, quant) == lib.SS_OK, L.ss_last_error(None)
    return coef


def _lib_entropy(L, coef, q, w, h, hs, vs):
    cap = L.ss_jpeg_encode_bound(w, h, hs, vs)
    out, size = (C.c_ubyte * cap)(), C.c_size_t()
    rc = L.ss_jpeg_entropy_encode(coef, q, w, h, hs, vs, out, cap, C.byref(size))
    assert rc == lib.SS_OK, L.ss_last_error(None)
    return bytes(out[:size.value])


def _mcu_blocks(w, h, hs, vs):
    return -(-w // (8 * hs)) * -(-h // (8 * vs)) * (hs * vs + 2)


def test_the_fixture_holds_what_the_issue_lists(cases):
    sizes = {c[1].shape[:2] for c in cases}
    assert sizes == {(1, 1), (8, 8), (3, 2), (23, 17), (24, 20), (20, 36), (31, 33), (45, 61), (75, 100), (70, 130)}       # (H, W)
    for s in ref.SAMPLING:
        assert {c[2] for c in cases if c[3] == s} == {10, 75, 85, 100}
        assert {c[1].shape[:2] for c in cases if c[3] == s} == sizes
    assert {c[0].split("_")[1] for c in cases} == {"noise", "noise2", "ramp", "flat", "checker", "synth"}
    assert sum(c[5] is not None for c in cases) >= 4


def _check_reference(bgr, q, s, data):
    rgb = bgr[:, :, ::-1]
    want, _, info = jpeg_ref.coefficients(data)
    got = ref.coefficients(rgb, q, s)
    diff = sum(int((g != w[:g.shape[0], :g.shape[1]]).sum()) for g, w in zip(got, want))          # real blocks only
    assert diff == 0
    assert np.array_equal(ref.quant_tables(q), jpeg_ref.parse(data)["quant"][:2])
    assert ref.encode(rgb, q, s) == data


def test_reference_equals_pillow_on_every_stored_case(cases):
    for name, bgr, q, s, data, _ in cases:
        _check_reference(bgr, q, s, data)
        hs, vs = ref.SAMPLING[s]
        assert np.array_equal(ref.coefficients(bgr[:, :, ::-1], q, s, np.int64)[0], ref.coefficients(bgr[:, :, ::-1], q, s)[0]), name      # nothing wraps


def test_reference_equals_live_pillow_on_random_sizes():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(77)
    for k in range(12):
        h, w = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        s, q = list(ref.SAMPLING)[k % 3], int(rng.integers(1, 101))
        bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if k % 2 else np.clip(
            np.add.outer(np.arange(h) * 3, np.arange(w) * 2)[:, :, None] + rng.integers(-4, 5, (h, w, 3)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, "JPEG", quality=q, subsampling=s)
        _check_reference(bgr, q, s, buf.getvalue())


def test_entropy_stage_reproduces_every_stored_file(L, cases):
    for name, bgr, q, s, data, _ in cases:
        h, w = bgr.shape[:2]
        hs, vs = ref.SAMPLING[s]
        coef = _lib_coefficients(L, data, _mcu_blocks(w, h, hs, vs))
        assert _lib_entropy(L, coef, q, w, h, hs, vs) == data, name


def test_entropy_stage_does_not_read_dummy_blocks(L, cases):
    name, bgr, q, s, data, _ = next(c for c in cases if c[0].startswith("20x24_noise_420"))
    coef = np.frombuffer(_lib_coefficients(L, data, _mcu_blocks(20, 24, 2, 2)), np.int16).copy()
    y = coef[:16 * 64].reshape(4, 4, 64)
    assert y[3, 0, 0] == y[2, 1, 0] and y[0, 3, 0] == y[0, 2, 0] and not y[3, :, 1:].any()      # what the decoder saw there: the DC before, no AC
    y[3, :, :] = 1234                                                                          # column 3 and row 3 are dummies
    y[:, 3, :] = -77
    assert _lib_entropy(L, coef.ctypes.data_as(C.POINTER(C.c_short)), q, 20, 24, 2, 2) == data


def _standard_tables(data):
    """True when the file's DHT segments are the four Annex K tables in the writer's order."""
    segs, p = [], 2
    while p + 4 <= len(data) and data[p] == 0xFF and data[p + 1] != 0xDA:
        ln = (data[p + 2] << 8) | data[p + 3]
        if data[p + 1] == 0xC4:
            segs.append(data[p + 4:p + 2 + ln])
        p += 2 + ln
    want = [bytes([t] + c + sy) for t, c, sy in ((0, ref.DC_COUNTS[0], ref.DC_SYMS[0]), (0x10, ref.AC_COUNTS[0], ref.AC_SYMS[0]),
                                                 (1, ref.DC_COUNTS[1], ref.DC_SYMS[1]), (0x11, ref.AC_COUNTS[1], ref.AC_SYMS[1]))]
    return segs == want


def test_entropy_stage_reproduces_the_decoders_fixtures(L):
    """jpeg_cases.npz entries that are 3-component, written with the standard tables and without restart markers: their quality follows
    from the name, and the file made from their own coefficients is the file."""
    z = np.load(os.path.join(GOLD, "jpeg_cases.npz"))
    done = 0
    for i, n in enumerate(str(x) for x in z["names"]):
        data = z[f"bytes_{i}"].tobytes()
        info = jpeg_ref.parse(data)
        if len(info["comps"]) != 3 or info["ri"] or not _standard_tables(data):
            continue
        w, h, hs, vs = info["width"], info["height"], info["hmax"], info["vmax"]
        q = int(n.split("_q")[1].split("_")[0])
        coef = _lib_coefficients(L, data, _mcu_blocks(w, h, hs, vs))
        assert _lib_entropy(L, coef, q, w, h, hs, vs) == data, n
        done += 1
    assert done >= 20


def test_bound_covers_every_stored_file(L, cases):
    for name, bgr, q, s, data, _ in cases:
        hs, vs = ref.SAMPLING[s]
        assert L.ss_jpeg_encode_bound(bgr.shape[1], bgr.shape[0], hs, vs) >= len(data), name
    # header + per block 20 bits of DC and 63 x 26 bits of AC, every byte stuffed
    assert L.ss_jpeg_encode_bound(16, 16, 2, 2) >= 625 + 6 * 2 * ((20 + 63 * 26 + 7) // 8)
    assert L.ss_jpeg_encode_bound(16, 16, 2, 2) < L.ss_jpeg_encode_bound(17, 16, 2, 2)


def test_refusals_that_need_no_device(L):
    coef, out, size = (C.c_short * (6 * 64))(), (C.c_ubyte * 65536)(), C.c_size_t()
    good = (coef, 85, 16, 16, 2, 2, out, 65536, C.byref(size))
    assert L.ss_jpeg_entropy_encode(*good) == lib.SS_OK

    def refused(cause, **kw):
        names = ("coef", "quality", "width", "height", "h_samp", "v_samp", "out", "out_cap", "out_size")
        args = [kw.get(n, g) for n, g in zip(names, good)]
        assert L.ss_jpeg_entropy_encode(*args) == lib.SS_ERR_INVALID
        assert cause in L.ss_last_error(None).decode(), L.ss_last_error(None)
    refused("null", coef=None)
    refused("null", out=None)
    refused("null", out_size=None)
    for q in (0, 101, -5):
        refused("quality", quality=q)
    for side in (0, 8193, -1):
        refused("sides", width=side)
        refused("sides", height=side)
    for hs, vs in ((1, 2), (2, 4), (4, 1), (0, 0), (3, 1)):
        refused("sampling", h_samp=hs, v_samp=vs)
    refused("below the bound", out_cap=L.ss_jpeg_encode_bound(16, 16, 2, 2) - 1)
    assert L.ss_jpeg_encode_bound(0, 16, 2, 2) < 0 and L.ss_jpeg_encode_bound(16, 16, 1, 2) < 0 and L.ss_jpeg_encode_bound(16, 9000, 1, 1) < 0
    coef[0] = 3000                                             # a DC difference of 12 bits: no baseline category
    refused("categories")
    # the batch call checks everything before it touches the device: a context is the first thing it needs
    one = (C.c_void_p * 1)(C.addressof(out))
    cap = (C.c_size_t * 1)(65536)
    assert L.ss_jpeg_encode_batch(None, None, C.c_void_p(4096), 768, 1, 16, 16, 0, 85, 2, 2, 1, one, cap, C.byref(size)) == lib.SS_ERR_INVALID


def test_the_reciprocal_divides_exactly():
    """The kernel quantises with (a * r) >> 32, r = floor(2^32 / qv) + 1: equal to a // qv for every a = |c| + qv / 2 with |c| below the bound
    the reference asserts, and every qv = 8 q, q = 1 .. 255."""
    c = np.arange(ref.MAX_COEF, dtype=np.uint64)
    for q in range(1, 256):
        qv = np.uint64(8 * q)
        a = c + (qv >> np.uint64(1))
        r = ref.reciprocal(qv)
        assert r < (1 << 32)
        assert np.array_equal((a * r) >> np.uint64(32), a // qv), q


def test_sink_kinds(tmp_path):
    S = cli.FrameSink
    assert S.encoded_kind("a/clip.mjpeg") == "mjpeg" and S.encoded_kind("clip.MJPG") == "mjpeg"
    assert S.encoded_kind(str(tmp_path)) == "jpgdir" and S.encoded_kind("new_dir/") == "jpgdir"
    assert S.encoded_kind("x.npy") is None and S.encoded_kind("x.bgr") is None and S.encoded_kind(str(tmp_path / "absent")) is None
    s = S(str(tmp_path / "c.mjpeg"), device_encode=True)
    assert s.kind == "mjpeg"
    with pytest.raises(RuntimeError, match="engine"):
        s.write(np.zeros((4, 4, 3), np.uint8))
    s.close()
    assert (tmp_path / "c.mjpeg").read_bytes() == b""
    s = S(str(tmp_path / "frames") + "/", device_encode=True, quality=70, subsampling="4:4:4")
    assert s.kind == "jpgdir" and (tmp_path / "frames").is_dir() and (s.quality, s.subsampling) == (70, "4:4:4")
    with pytest.raises(ValueError, match="mjpeg"):
        S(str(tmp_path / "x.npy"), device_encode=True)
    # without device encoding nothing changes: the same paths select what they always did
    assert S(str(tmp_path / "x.npy")).kind == "npy" and S(str(tmp_path / "x.bgr")).kind == "bgr" and S(str(tmp_path / "pngs")).kind == "dir"
    with pytest.raises(ValueError, match="host frames"):
        S(str(tmp_path / "y.npy")).write_device(None)


def test_cli_flags(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(cli, "process_video", lambda job: job)
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--save", str(tmp_path / "o.mjpeg"), "--device-encode"])
    assert job["device_encode"] is True and job["save_quality"] == 85 and job["save_subsampling"] == "4:2:0"
    (job,) = cli.main(["--source", "synthetic:3", "--save", str(tmp_path) + "/", "--device-encode", "--save-quality", "60", "--save-subsampling", "4:2:2"])
    assert (job["save_quality"], job["save_subsampling"], job["save"]) == (60, "4:2:2", str(tmp_path) + "/")
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--save", str(tmp_path / "o.npy")])
    assert job["device_encode"] is False
    import argparse
    two = argparse.Namespace(source=["a", "b"], save=str(tmp_path) + "/", device_encode=True)                   # several sources: a directory each
    assert cli._save_path(two, 1) == os.path.join(str(tmp_path), "stream_1", "") and cli.FrameSink.encoded_kind(cli._save_path(two, 1)) == "jpgdir"
    two.save = str(tmp_path / "o.mjpeg")
    assert cli._save_path(two, 1) == str(tmp_path / "o_1.mjpeg")
    for argv, word in ((["--source", "synthetic:3", "--device-encode"], "--save"),
                       (["--source", "synthetic:3", "--save", str(tmp_path / "o.npy"), "--device-encode"], ".mjpeg"),
                       (["--source", "synthetic:3", "--save", str(tmp_path / "o.bgr"), "--device-encode"], ".mjpeg"),
                       (["--source", "synthetic:3", "--save", str(tmp_path / "absent_dir"), "--device-encode"], "directory"),
                       (["--source", "synthetic:3", "--save", str(tmp_path / "o.mjpeg"), "--device-encode", "--save-quality", "0"], "--save-quality"),
                       (["--source", "synthetic:3", "--save", str(tmp_path / "o.mjpeg"), "--device-encode", "--save-subsampling", "4:1:1"], "4:1:1")):
        with pytest.raises(SystemExit):
            cli.main(argv)
        assert word in capsys.readouterr().err, argv
