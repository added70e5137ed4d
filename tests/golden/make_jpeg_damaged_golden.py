"""Writes the fixture of damaged scans for the device entropy stage (NumPy only, no Pillow; run by hand, never at test time):

    python tests/golden/make_jpeg_damaged_golden.py

    jpeg_damaged.npz   names [N], sources [N] (the sound file a case was made from: `good` of jpeg_refused.npz or a case name of
                       jpeg_entropy_cases.npz / jpeg_cases.npz), causes [N] (what tests/jpeg_huff_ref.py reports, the same at W = 4 and
                       W = 32; "" when the file decodes), lanes [N, 2] (the status word's lane at W = 4 and 32, -1 without a cause);
                       per case i: bytes_i (uint8, the file), rounds4_i and rounds32_i (the rounds of every tile),
                       rgb_i (uint8 [H,W,3], tests/jpeg_ref.py's decode) when there is no cause

The cases, all with sound headers, so that only decoding the scan shows the damage:

  <source>_m<k>      seeded mutations of the scan of four small files: one flipped bit, six random bytes, or three FE bytes.  No
                     mutation creates an FF or touches an FF or the byte behind it, so the scan is cut into the same segments.
                     Of the mutations that are refused or decode to other coefficients than their source's, the first
                     five per source and cause are kept.  rst1_61x45_grey_q90_m2, _m12 and _m23 end a segment in a code that
                     reaches beyond its last real bit and carries the index past 63 (docs/JPEG.md §12: judged, not "data ends").
  good_dc16          bit 4 set in every symbol of the first DC table of `good`: "bad DC category", in the first lane
  good_dc16_cat5     the same in the symbol of category 5 alone: found by a later lane
  130x70_..._late<k> 130x70_noise_444_q100 with the damage beyond byte 16 384 of the scan: at W = 4 the error is found in a later
                     tile than the first, by a lane above 1024

The restatement asserts that every block-table store stays inside the lane's segment; here every entry total is checked against
the capacity (cause 6 does not occur).
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

SEED = 2
PER_FILE = 60
PER_CLASS = 5                                    # mutations kept per (source, cause): the first ones; the fixture stays under 512 kB
SMALL = ("good", "rst1_61x45_420_q50", "rst1_61x45_grey_q90", "opt_48x32_444_q100")
LATE = "130x70_noise_444_q100"


def sources():
    out = {"good": np.load(os.path.join(HERE, "jpeg_refused.npz"))["good"].tobytes()}
    for f, want in (("jpeg_entropy_cases.npz", SMALL[1:]), ("jpeg_cases.npz", (LATE,))):
        z = np.load(os.path.join(HERE, f))
        for i, n in enumerate(z["names"]):
            if str(n) in want:
                out[str(n)] = z[f"bytes_{i}"].tobytes()
    return out


def scan_span(data):
    from tests.jpeg_ref import parse
    return parse(data)["scan"], data.rindex(b"\xff\xd9")


def mutate(data, rng, lo=None, kind=None):
    """One mutation of the scan's bytes from `lo` on: a flipped bit (kind 0), six random bytes (1) or three FE bytes (2)."""
    start, end = scan_span(data)
    lo = start if lo is None else lo
    free = [p for p in range(lo, end) if data[p] != 0xFF and data[p - 1] != 0xFF]      # neither an FF nor the 00 / RSTn behind one
    bad = bytearray(data)
    kind = int(rng.integers(0, 3)) if kind is None else kind
    at = int(rng.integers(0, len(free)))
    if kind == 0:
        while True:
            v = bad[free[at]] ^ (1 << int(rng.integers(0, 8)))
            if v != 0xFF:
                break
        bad[free[at]] = v
    else:
        for p in free[at:at + (6 if kind == 1 else 3)]:
            bad[p] = int(rng.integers(0, 255)) if kind == 1 else 0xFE                 # (never FF)
    assert len(bad) == len(data) and bad.count(0xFF) == data.count(0xFF)
    return bytes(bad)


def expectations(data):
    """(cause or "", (lane at W = 4, lane at W = 32), rounds at 4, rounds at 32, dense coefficients or None) by tests/jpeg_huff_ref.py."""
    from tests import jpeg_huff_ref as ref
    got = []
    for W in (4, 32):
        st = ref.stream(data, W)
        entries, cap = ref.entry_count(st)
        assert entries <= cap, (entries, cap)
        coef, rounds, cause = ref.finish(st)
        assert (st[4] is None) == (cause is None) and (cause is None or st[4] & 7 != 6)
        got.append((cause or "", -1 if st[4] is None else (st[4] >> 3) - 1, rounds, coef))
    assert got[0][0] == got[1][0], (got[0][0], got[1][0])                            # the cause does not depend on W
    assert got[0][0] or np.array_equal(got[0][3], got[1][3])
    return got[0][0], (got[0][1], got[1][1]), got[0][2], got[1][2], None if got[0][0] else got[0][3]


def corpus():
    """[(name, source, bytes)] before selection."""
    src = sources()
    rng = np.random.default_rng(SEED)
    out = []
    for s in SMALL:
        out += [(f"{s}_m{k}", s, mutate(src[s], rng)) for k in range(PER_FILE)]
    good = src["good"]
    dht = good.index(b"\xff\xc4")
    assert good[dht + 4] == 0x00                                                     # the first table is DC table 0
    n = sum(good[dht + 5:dht + 21])
    for name, which in (("good_dc16", range(n)), ("good_dc16_cat5", (5,))):
        patched = bytearray(good)
        for k in which:
            patched[dht + 21 + k] |= 0x10
        out.append((name, "good", bytes(patched)))
    start, _ = scan_span(src[LATE])
    out += [(f"{LATE}_late{k}", LATE, mutate(src[LATE], rng, start + 16384 + 2048 * k, (2, 1, 2)[k])) for k in range(3)]
    return out, src


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same file."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    from tests import jpeg_huff_ref as ref
    from tests import jpeg_ref
    cases, src = corpus()
    sound = {s: ref.decode(d, 32)[0] for s, d in src.items()}
    keep = []
    for name, s, data in cases:
        cause, lanes, r4, r32, coef = expectations(data)
        if not cause and np.array_equal(coef, sound[s]):
            continue                                                                  # the damage fell on bits that decide nothing
        if "_m" in name and sum(1 for c in keep if (c[1], c[3]) == (s, cause)) >= PER_CLASS:
            continue
        keep.append((name, s, data, cause, lanes, r4, r32))
    causes = [c[3] for c in keep]
    for k in range(1, 6):
        assert causes.count(ref.CAUSES[k]) >= 2, (ref.CAUSES[k], causes.count(ref.CAUSES[k]))
    assert causes.count("") >= 8, causes.count("")
    by_name = {c[0]: c for c in keep}
    assert by_name["good_dc16"][3] == by_name["good_dc16_cat5"][3] == "bad DC category" and by_name["good_dc16"][4] == (0, 0) and by_name["good_dc16_cat5"][4][0] > 0
    late = [c for c in keep if c[1] == LATE]
    assert len(late) == 3 and all(c[3] and c[4][0] >= ref.LANES and len(c[5]) > 1 for c in late), [(c[3], c[4]) for c in late]
    out = {"names": np.array([c[0] for c in keep]), "sources": np.array([c[1] for c in keep]), "causes": np.array(causes),
           "lanes": np.array([c[4] for c in keep], np.int32)}
    for i, (name, s, data, cause, lanes, r4, r32) in enumerate(keep):
        out[f"bytes_{i}"] = np.frombuffer(data, np.uint8)
        out[f"rounds4_{i}"], out[f"rounds32_{i}"] = np.array(r4, np.int32), np.array(r32, np.int32)
        if not cause:
            out[f"rgb_{i}"] = jpeg_ref.decode(data)
    path = os.path.join(HERE, "jpeg_damaged.npz")
    save_npz(path, out)
    assert os.path.getsize(path) < 512 * 1000
    print(path, os.path.getsize(path), "bytes;", len(keep), "of", len(cases), "cases;", {c: causes.count(c) for c in sorted(set(causes))})


if __name__ == "__main__":
    main()
