"""The crafted JPEG files of tests/jpeg_crafted.py and the damaged scans of tests/golden/jpeg_damaged.npz without a GPU: the files
are what they claim, tests/jpeg_ref.py equals Pillow where the two are meant to (docs/JPEG.md §2), the host decoder reads the blocks
they were written from, and host decoder, its restatement and the device stage's restatement name one and the same cause."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from strongsort_yolo_amd import jpeg, lib
from tests import jpeg_crafted as jc
from tests import jpeg_huff_ref as huff
from tests import jpeg_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WRAPPING = ("b_max", "d_negative", "f_seed1", "f_seed2", "f_seed3")


@pytest.fixture(scope="module")
def L():
    lib.build()
    return lib.load()


def _host(L, data):
    """(coefficients, "") or (None, the cause) by the library's host decoder."""
    h, w, nc, (hs, vs) = jpeg.probe(data)
    cap = -(-w // (8 * hs)) * -(-h // (8 * vs)) * 64 * (1 if nc == 1 else hs * vs + 2)
    coef, quant = np.zeros(cap, np.int16), np.zeros((4, 64), np.uint16)
    rc = L.ss_jpeg_coefficients(data, len(data), coef.ctypes.data_as(C.POINTER(C.c_short)), cap, quant.ctypes.data_as(C.POINTER(C.c_ushort)))
    if rc == lib.SS_OK:
        return coef, ""
    assert rc == lib.SS_ERR_INVALID
    return None, L.ss_last_error(None).decode().split(": ", 1)[1]


def _outside(y):
    return int(((y < -512) | (y > 511)).sum())


def test_extreme_files_wrap_int32_and_reach_every_zone_of_the_range_limit():
    cases = jc.extreme()
    assert len(cases) == 63
    zones, wrapped = set(), {}
    for c in cases:
        y = jpeg_ref.prelimit(c.data)
        v = y & 1023
        zones |= set(np.unique(np.select([v < 128, v < 512, v < 896], [0, 1, 2], 3)).tolist())
        if c.name.split("_q")[0] in WRAPPING and "_q1_" in c.name:
            wrapped[c.name] = int((jc.expect(c).rgb != jpeg_ref.decode(c.data, dtype=np.int64)).sum())
            assert wrapped[c.name] > 0 and _outside(y) > 0, c.name
    assert zones == {0, 1, 2, 3}
    assert (wrapped["b_max_q1_444"], wrapped["d_negative_q1_444"], wrapped["f_seed1_q1_444"]) == (396, 416, 547)     # the counts of the first CPU study
    assert (wrapped["f_seed1_q1_420"], wrapped["f_seed1_q1_422"]) == (680, 660)


def test_padding_files_hold_samples_that_do_not_repeat_the_edge():
    """Beside the last real chroma column (and below the last real row) of the 2:1 planes lie samples far from the edge's: a tap
    that reads s[cw] instead of clamping to cw - 1 changes pixels."""
    cols = rows = 0
    for c in jc.padding():
        coefs, quant, info = jpeg_ref.coefficients(c.data)
        cw, ch = -(-c.W // c.hm), -(-c.H // c.vm)
        for k in (1, 2):
            s = jpeg_ref.idct_blocks(coefs[k], quant[info["comps"][k][3]])
            s = s.transpose(0, 2, 1, 3).reshape(s.shape[0] * 8, s.shape[1] * 8).astype(np.int32)
            if c.hm == 2 and cw > 2 and cw % 8:
                cols += int((np.abs(s[:ch, cw] - s[:ch, cw - 1]) > 4).sum())
            if c.vm == 2 and cw > 2 and ch % 8:
                rows += int((np.abs(s[ch, :cw] - s[ch - 1, :cw]) > 4).sum())
    assert cols > 100 and rows > 100, (cols, rows)


def test_the_host_decoder_reads_the_blocks_the_files_were_written_from(L):
    for c in jc.extreme() + jc.padding():
        coef, cause = _host(L, c.data)
        assert cause == "" and np.array_equal(coef, jc.expect(c).coef), c.name
        for k, got, want in jc.known_answer(c, coef):
            assert np.array_equal(got, want), (c.name, k)
        for W in (4, 32):                                                    # and so does the device stage's restatement
            got, rounds, status = huff.decode(c.data, W)
            assert status is None and np.array_equal(got, coef), (c.name, W)


def test_reference_equals_pillow_where_no_sample_leaves_the_table_and_only_there():
    Image = pytest.importorskip("PIL.Image")
    for c in jc.padding():
        assert _outside(jpeg_ref.prelimit(c.data)) == 0, c.name             # inside -512 .. 511 the C table and a saturating IDCT agree
        pil = np.asarray(Image.open(io.BytesIO(c.data)).convert("RGB"))
        assert np.array_equal(pil, jc.expect(c).rgb), (c.name, int((pil != jc.expect(c).rgb).sum()))
    # the extreme files leave that span; nothing about them is compared with Pillow (docs/JPEG.md §2)
    assert sum(_outside(jpeg_ref.prelimit(c.data)) > 0 for c in jc.extreme()) >= 30


# ---- damaged scans ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def damaged():
    z = np.load(os.path.join(GOLD, "jpeg_damaged.npz"))
    return z, [str(n) for n in z["names"]]


def test_damaged_fixture_is_what_the_restatements_say_now_and_the_three_decoders_name_one_cause(L, damaged):
    z, names = damaged
    differ = []
    for i, name in enumerate(names):
        data, cause = z[f"bytes_{i}"].tobytes(), str(z["causes"][i])
        for col, W in enumerate((4, 32)):
            st = huff.stream(data, W)                                        # (asserts that every table store stays inside its segment)
            coef, rounds, got = huff.finish(st)
            assert (got or "") == cause, (name, W, got, cause)
            assert rounds == z[f"rounds{W}_{i}"].tolist(), (name, W)
            assert (-1 if st[4] is None else (st[4] >> 3) - 1) == z["lanes"][i][col], (name, W)
            entries, cap = huff.entry_count(st)
            assert entries <= cap, (name, W)
        host_coef, host_cause = _host(L, data)
        try:
            ref_cause = ""
            ref_coef = jc.library_layout(jpeg_ref.coefficients(data)[0])
        except jpeg_ref.Refused as e:
            ref_cause = str(e)
        if not (host_cause == ref_cause == cause):
            differ.append((name, host_cause, ref_cause, cause))
        elif not cause:
            assert np.array_equal(host_coef, ref_coef) and np.array_equal(host_coef, coef), name
            assert np.array_equal(z[f"rgb_{i}"], jpeg_ref.decode(data)), name
    assert not differ, f"{len(differ)} of {len(names)} files: (name, host, its restatement, the device's restatement) {differ}"


def test_damaged_fixture_covers_what_it_promises(damaged):
    z, names = damaged
    causes = [str(c) for c in z["causes"]]
    for k in range(1, 6):
        assert causes.count(huff.CAUSES[k]) >= 2, huff.CAUSES[k]
    assert huff.CAUSES[6] not in causes
    sound = {"good": np.load(os.path.join(GOLD, "jpeg_refused.npz"))["good"].tobytes()}
    for f in ("jpeg_entropy_cases.npz", "jpeg_cases.npz"):
        s = np.load(os.path.join(GOLD, f))
        sound.update({str(n): s[f"bytes_{i}"].tobytes() for i, n in enumerate(s["names"]) if str(n) in set(z["sources"].tolist())})
    other = 0
    for i, name in enumerate(names):
        data, src = z[f"bytes_{i}"].tobytes(), sound[str(z["sources"][i])]
        assert len(data) == len(src) and data.count(0xFF) == src.count(0xFF), name       # no FF made, none touched
        assert jpeg.probe(data) == jpeg.probe(src), name                                  # sound headers, the source's size
        if not causes[i]:
            other += not np.array_equal(z[f"rgb_{i}"], jpeg_ref.decode(src))
    assert other >= 8
    late = [i for i, n in enumerate(names) if "_late" in n]
    assert len(late) == 3
    for i in late:                                                           # found in a later tile at W = 4, by a lane beyond the first 1024
        assert causes[i] and z["lanes"][i][0] >= huff.LANES and len(z[f"rounds4_{i}"]) > 1
        a, b = np.frombuffer(z[f"bytes_{i}"].tobytes(), np.uint8), np.frombuffer(sound[str(z["sources"][i])], np.uint8)
        assert np.flatnonzero(a != b)[0] >= jpeg_ref.parse(b.tobytes())["scan"] + 16384
    assert os.path.getsize(os.path.join(GOLD, "jpeg_damaged.npz")) < 512 * 1000


def test_truncations_under_a_table_whose_all_zero_code_carries_a_run_name_one_cause(L, monkeypatch):
    """With the all-zero code meaning (run 1, size 1), zero bits read beyond a cut scan march the index past 63.  A symbol that
    starts beyond the last real bit is not judged: host decoder, its restatement and the device's restatement all say that the data
    ends (the host decoder used to say "coefficient index beyond 63" on 121 of these 817 cuts)."""
    from tests import jpeg_enc_huff_ref as wr
    from tests import jpeg_enc_ref as er
    syms = [list(t) for t in er.AC_SYMS]
    i, j = syms[0].index(0x01), syms[0].index(0x11)
    syms[0][i], syms[0][j] = 0x11, 0x01
    monkeypatch.setattr(er, "AC_SYMS", syms)
    monkeypatch.setattr(wr, "AC", [er._codes(er.AC_COUNTS[t], syms[t]) for t in range(2)])
    rng = np.random.default_rng(1)
    coefs = [np.where(rng.random((2, 4, 64)) < 0.3, rng.integers(-20, 21, (2, 4, 64)), 0).astype(np.int16) for _ in range(3)]
    data = wr.encode_file(coefs, 32, 16, 1, 1, er.quant_tables(90))
    coef, cause = _host(L, data)
    assert cause == "" and np.array_equal(coef, jc.library_layout(coefs))
    scan = jpeg_ref.parse(data)["scan"]
    seen = set()
    for cut in range(scan + 1, len(data) - 2):
        if data[cut - 1] == 0xFF:
            continue
        bad = data[:cut] + b"\xff\xd9"
        with pytest.raises(jpeg_ref.Refused) as e:
            jpeg_ref.coefficients(bad)
        causes = (_host(L, bad)[1], str(e.value), huff.decode(bad, 4)[2])
        assert len(set(causes)) == 1, (cut - scan, causes)
        seen.add(causes[0])
    assert "data ends before the last MCU" in seen and len(seen) > 1, seen
