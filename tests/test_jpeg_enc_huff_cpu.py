"""The encoder's device entropy stage without a GPU (docs/JPEG.md §13): the NumPy restatement of its data-parallel steps
(tests/jpeg_enc_huff_ref.py) against Pillow's stored files and against the sequential reference, the CLI's flags, the keyword's check."""
import ctypes as C
import re

import numpy as np
import pytest

from strongsort_yolo_amd import cli, jpeg, lib
from tests import jpeg_enc_huff_ref as href
from tests import jpeg_enc_ref as ref


HEADER = 623                                                         # SOI .. SOS; with EOI the 625 bytes every file carries besides its scan


@pytest.fixture(scope="module")
def cases():
    return ref.load_cases()


def test_restatement_reproduces_every_stored_scan(cases):
    stuffed_files, ends_in_ff = 0, 0
    for name, bgr, q, s, data, _ in cases:
        h, w = bgr.shape[:2]
        hm, vm = ref.SAMPLING[s]
        st = href.stages(ref.coefficients(bgr[:, :, ::-1], q, s), w, h, hm, vm)
        assert data[:HEADER] == ref.header(w, h, hm, vm, ref.quant_tables(q)) and data[-2:] == b"\xff\xd9", name
        assert st["stuffed"] == data[HEADER:-2], name
        # the stage values the GPU tests rely on are consistent with each other
        assert len(st["unstuffed"]) == -(-st["bits"] // 8) and len(st["stuffed"]) == len(st["unstuffed"]) + st["unstuffed"].count(b"\xff")
        assert st["pos"][0] == 0 and np.array_equal(np.diff(st["pos"]), st["lens"][:-1]) and st["pos"][-1] + st["lens"][-1] == st["bits"]
        assert st["stuffed"].replace(b"\xff\x00", b"\xff") == st["unstuffed"]
        stuffed_files += b"\xff" in st["unstuffed"]
        ends_in_ff += st["unstuffed"].endswith(b"\xff")
    assert len(cases) == 180 and stuffed_files == 103 and ends_in_ff == 1


@pytest.mark.parametrize("w,h", [(1, 1), (2, 3), (8, 8), (36, 20), (20, 24), (17, 23)])
@pytest.mark.parametrize("s", list(ref.SAMPLING))
def test_predecessor_closed_form_equals_a_search(w, h, s):
    """The edge shapes of the fixture: every branch of the closed form (first block, same row of the MCU, row above, MCU before with a
    narrower or lower set of real blocks) against the sequential rule, and dummies exactly where the real-block extents end."""
    hm, vm = ref.SAMPLING[s]
    lay = href.layout(w, h, hm, vm)
    extent = [(-(-h // 8), -(-w // 8))] + [(-(-(-(-h // vm)) // 8), -(-(-(-w // hm)) // 8))] * 2
    last = {}
    for p in range(len(lay["comp"])):
        c = int(lay["comp"][p])
        assert bool(lay["real"][p]) == (lay["by"][p] < extent[c][0] and lay["bx"][p] < extent[c][1])
        if lay["real"][p]:
            assert lay["prev"][p] == last.get(c, -1), (p, c)
            last[c] = p
    assert lay["real"][0] and not (lay["comp"] > 0)[~lay["real"]].any()


def test_dummy_and_maximum_block_lengths():
    flat = [np.zeros((1, 1, 64), np.int16)] * 3
    st = href.stages(flat, 1, 1, 2, 2)                               # 1 x 1 at 4:2:0: one real luma block, three dummies, two chroma
    assert list(st["lens"]) == [6, 6, 6, 6, 4, 4] and list(st["layout"]["real"]) == [True, False, False, False, True, True]
    assert st["bits"] == 32 and len(st["unstuffed"]) == 4            # a whole flat 4:2:0 MCU is one 32-bit word
    st = href.stages(href.crafted("b_max"), href.CRAFT_W, href.CRAFT_H, 1, 1)
    assert st["lens"].max() == href.MAX_BLOCK_BITS == 1658 and (st["lens"] == 1658).sum() == 6      # the luma blocks with a category-11 difference
    assert 3_100_000 * href.MAX_BLOCK_BITS > 1 << 32                 # why the positions are 64-bit


@pytest.mark.parametrize("name", href.CRAFTED)
def test_restatement_agrees_with_the_sequential_reference_on_crafted_coefficients(name):
    coefs = href.crafted(name)
    q = ref.quant_tables(href.CRAFT_Q)
    want = ref.entropy_encode(coefs, href.CRAFT_W, href.CRAFT_H, 1, 1, q)
    assert href.encode_file(coefs, href.CRAFT_W, href.CRAFT_H, 1, 1, q) == want
    scan = want[HEADER:-2]
    if name == "b_max":
        assert len(scan) == 6866 and len(re.findall(rb"(?:\xff\x00)+", scan)) == 1516 and b"\xff\x00\xff\x00" in scan      # the issue's figures
    if name == "c_zrl":
        st = href.stages(coefs, href.CRAFT_W, href.CRAFT_H, 1, 1)
        assert st["lens"][0] == 3 + 3 + 3 * 11 + 16 + 1              # DC category 3, three ZRL, run 15 / size 1 (16 bits), no EOB


def test_the_library_host_writer_agrees_on_crafted_coefficients():
    """What the GPU tests compare against: ss_jpeg_entropy_encode on the library's layout of the same arrays."""
    lib.build()
    L = lib.load()
    cap = L.ss_jpeg_encode_bound(href.CRAFT_W, href.CRAFT_H, 1, 1)
    for name in href.CRAFTED:
        coefs = href.crafted(name)
        flat = href.library_layout(coefs, href.CRAFT_W, href.CRAFT_H, 1, 1)
        out, size = (C.c_ubyte * cap)(), C.c_size_t()
        assert L.ss_jpeg_entropy_encode(flat.ctypes.data_as(C.POINTER(C.c_short)), href.CRAFT_Q, href.CRAFT_W, href.CRAFT_H, 1, 1, out, cap, C.byref(size)) == lib.SS_OK
        assert bytes(out[:size.value]) == href.encode_file(coefs, href.CRAFT_W, href.CRAFT_H, 1, 1, ref.quant_tables(href.CRAFT_Q)), name


def test_the_issues_pixel_cases_hold_consecutive_stuffed_bytes():
    for seed, s in ((11, "4:4:4"), (12, "4:2:0")):
        rgb = np.random.default_rng(seed).integers(0, 256, (31, 33, 3), dtype=np.uint8)
        hm, vm = ref.SAMPLING[s]
        st = href.stages(ref.coefficients(rgb, 100, s), 33, 31, hm, vm)
        assert b"\xff\x00\xff\x00" in st["stuffed"], seed
        assert ref.header(33, 31, hm, vm, ref.quant_tables(100)) + st["stuffed"] + b"\xff\xd9" == ref.encode(rgb, 100, s)


def test_cli_flags(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(cli, "process_video", lambda job: job)
    save = str(tmp_path / "o.mjpeg")
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--save", save, "--device-encode", "--device-encode-entropy"])
    assert job["device_encode"] is True and job["device_encode_entropy"] is True and job["device_entropy"] is False
    (job,) = cli.main(["--source", "synthetic:3", "--track", "--save", save, "--device-encode"])
    assert job["device_encode"] is True and job["device_encode_entropy"] is False
    for argv, word in ((["--source", "synthetic:3", "--save", save, "--device-encode-entropy"], "--device-encode"),
                       (["--source", "synthetic:3", "--device-encode-entropy"], "--device-encode"),
                       (["--source", "synthetic:3", "--save", save, "--device-encode", "--device-encode-entropy", "--device-entropy"], "--device-decode"),
                       (["--source", "synthetic:3", "--device-entropy"], "--device-decode")):
        with pytest.raises(SystemExit):
            cli.main(argv)
        assert word in capsys.readouterr().err, argv


def test_sink_passes_the_entropy_stage_on(tmp_path, monkeypatch):
    seen = []
    monkeypatch.setattr(jpeg, "encode", lambda engine, frames, quality, subsampling, **kw: seen.append(kw) or [])
    for flag, want in ((False, "host"), (True, "device")):
        s = cli.FrameSink(str(tmp_path / "c.mjpeg"), device_encode=True, device_entropy=flag)
        assert s.entropy == want
        s._held, s.n, s._buf = 1, 1, np.zeros((1, 4, 4, 3), np.uint8)
        s.flush()
        s.close()
    assert seen == [{"entropy": "host"}, {"entropy": "device"}]
    assert cli.FrameSink(str(tmp_path / "d.mjpeg"), device_encode=True).entropy == "host"


def test_entropy_keyword_is_checked_before_a_device_is_touched():
    frames = np.zeros((1, 8, 8, 3), np.uint8)
    for bad in ("gpu", "", None, "Device"):
        with pytest.raises(ValueError, match="entropy"):
            jpeg.encode(None, frames, entropy=bad)                   # (no engine: anything that reached for one would fail differently)
    with pytest.raises(ValueError, match=r'entropy \'gpu\' \("host" or "device"\)'):
        jpeg.encode(None, frames, entropy="gpu")
    assert "ss_jpeg_encode_batch_device" in lib.EXPORTS and "ss_jpeg_entropy_encode_device" in lib.EXPORTS
