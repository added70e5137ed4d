"""NumPy restatement of docs/JPEG.md "Encoding" (pixels -> baseline JPEG file, the arithmetic of libjpeg-turbo's defaults: JDCT_ISLOW,
the Annex K tables, no optimisation).  The specification in executable form; not a test module.

    q = quant_tables(quality)                      uint16 [2, 64] natural order: luma, chroma
    coefs = coefficients(rgb, quality, sampling)   per component int16 [bh, bw, 64] natural-order blocks, REAL blocks only
    data = encode(rgb, quality, sampling)          the whole file; sampling "4:2:0" | "4:2:2" | "4:4:4"
    reciprocal(qv)                                 the multiplier the device divides by 8 q with

    load_cases()                                   the stored fixtures (tests/golden/make_jpeg_encode_golden.py)

`rgb` is uint8 [H, W, 3] in R, G, B order.
"""
import os

import numpy as np

from tests.jpeg_ref import ZIGZAG

SAMPLING = {"4:2:0": (2, 2), "4:2:2": (2, 1), "4:4:4": (1, 1)}
MAX_COEF = 1 << 14          # |8 x coefficient| stays below this: a true DCT coefficient of samples in -128 .. 127 is at most 1024 in magnitude
                            # (the DC term), 8 x that is 2^13, and the integer passes are off by a few units at most; asserted in fdct()

BASE = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32], np.int64)

# Annex K.3.3 - K.3.6 as the DHT segments carry them: 16 code counts, then the symbols
DC_COUNTS = [[0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]]
DC_SYMS = [list(range(12)), list(range(12))]
AC_COUNTS = [[0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]]
AC_SYMS = [list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")), list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6"
    "c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))]


def quant_tables(quality: int) -> np.ndarray:
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((BASE * s + 50) // 100, 1, 255).astype(np.uint16)


def reciprocal(qv):
    """(a * reciprocal(qv)) >> 32 == a // qv for every a < MAX_COEF + qv / 2 and qv in 8, 16 .. 2040 (proved in test_jpeg_encode_cpu.py)."""
    return (1 << 32) // np.asarray(qv, np.uint64) + 1


def _ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16
    return y, cb, cr


def component_planes(rgb, hm, vm):
    """Y, Cb, Cr as int32 planes padded to whole 8 x 8 blocks of each component (not to whole MCUs), by the edge rule of the document."""
    H, W = rgb.shape[:2]
    y, cb, cr = _ycc(rgb)
    yy = np.minimum(np.arange(-(-H // 8) * 8), H - 1)
    xx = np.minimum(np.arange(-(-W // 8) * 8), W - 1)
    out = [y[yy][:, xx]]
    cw, ch = -(-W // hm), -(-H // vm)
    cyp = np.minimum(np.arange(-(-ch // 8) * 8), ch - 1)              # the DOWNSAMPLED last row is replicated
    cx = np.arange(-(-cw // 8) * 8)                                    # no clamp of cx: the full-size last column is replicated
    for c in (cb, cr):
        acc = np.zeros((len(cyp), len(cx)), np.int32)
        for j in range(vm):
            rows = np.minimum(vm * cyp + j, H - 1)
            for i in range(hm):
                acc += c[rows][:, np.minimum(hm * cx + i, W - 1)]
        if (hm, vm) == (2, 2):
            acc = (acc + 1 + (cx & 1)[None, :]) >> 2
        elif (hm, vm) == (2, 1):
            acc = (acc + (cx & 1)[None, :]) >> 1
        out.append(acc)
    return out


def _pass(d, first, dtype):
    d0, d1, d2, d3, d4, d5, d6, d7 = d
    s = 11 if first else 15
    r = dtype(1 << (s - 1))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    if first:
        o0, o4 = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o0, o4 = (t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2
    z1 = (t12 + t13) * 4433
    o2, o6 = (z1 + t13 * 6270 + r) >> s, (z1 - t12 * 15137 + r) >> s
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    return [o0, (t7 + z1 + z4 + r) >> s, o2, (t6 + z2 + z3 + r) >> s, o4, (t5 + z2 + z4 + r) >> s, o6, (t4 + z1 + z3 + r) >> s]


def fdct(plane, dtype=np.int32):
    """plane [8 bh, 8 bw] samples -> [bh, bw, 8, 8], 8 x the DCT coefficients of sample - 128."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    d = (plane.astype(dtype) - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
    d = np.stack(_pass([d[..., j] for j in range(8)], True, dtype), axis=-1)        # along each row
    d = np.stack(_pass([d[..., i, :] for i in range(8)], False, dtype), axis=-2)    # down each column
    assert int(np.abs(d).max()) < MAX_COEF
    return d


def quantise(c, q):
    """c [..., 64] (8 x coefficients), q [64] -> int16."""
    qv = q.astype(np.int64) << 3
    t = (np.abs(c.astype(np.int64)) + (qv >> 1)) // qv
    return np.where(c < 0, -t, t).astype(np.int16)


def coefficients(rgb, quality, sampling="4:2:0", dtype=np.int32):
    hm, vm = SAMPLING[sampling]
    q = quant_tables(quality)
    out = []
    for k, p in enumerate(component_planes(np.asarray(rgb), hm, vm)):
        d = fdct(p, dtype)
        out.append(quantise(d.reshape(d.shape[:2] + (64,)), q[1 if k else 0]))
    return out


def _codes(counts, syms):
    t, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            t[syms[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return t


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, ln):
        self.acc = (self.acc << ln) | code
        self.n += ln
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def value(self, v):
        s = int(abs(v)).bit_length()
        self.put((v - 1 if v < 0 else v) & ((1 << s) - 1), s)


def header(W, H, hm, vm, q):
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    for t in range(2):
        out += seg(0xDB, bytes([t]) + bytes(int(v) for v in q[t][ZIGZAG]))
    out += seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, hm << 4 | vm, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for t in range(2):
        out += seg(0xC4, bytes([t] + DC_COUNTS[t] + DC_SYMS[t])) + seg(0xC4, bytes([0x10 | t] + AC_COUNTS[t] + AC_SYMS[t]))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def entropy_encode(coefs, W, H, hm, vm, q) -> bytes:
    """coefs: per component [bh, bw, 64] natural order over (at least) its real blocks."""
    dc = [_codes(DC_COUNTS[t], DC_SYMS[t]) for t in range(2)]
    ac = [_codes(AC_COUNTS[t], AC_SYMS[t]) for t in range(2)]
    mcux, mcuy = -(-W // (8 * hm)), -(-H // (8 * vm))
    real = [(-(-H // 8), -(-W // 8))] + [(-(-(-(-H // vm)) // 8), -(-(-(-W // hm)) // 8))] * 2
    b = _Bits()
    pred = [0, 0, 0]
    for my in range(mcuy):
        for mx in range(mcux):
            for ci in range(3):
                h, v = (hm, vm) if ci == 0 else (1, 1)
                t = 1 if ci else 0
                for by in range(my * v, my * v + v):
                    for bx in range(mx * h, mx * h + h):
                        if by >= real[ci][0] or bx >= real[ci][1]:         # a dummy block: the DC before it, nothing else
                            b.put(*dc[t][0])
                            b.put(*ac[t][0])
                            continue
                        zz = [int(x) for x in coefs[ci][by, bx][ZIGZAG]]
                        diff, pred[ci] = zz[0] - pred[ci], zz[0]
                        b.put(*dc[t][abs(diff).bit_length()])
                        b.value(diff)
                        run = 0
                        last = max([k for k in range(1, 64) if zz[k]], default=0)
                        for k in range(1, last + 1):
                            if zz[k] == 0:
                                run += 1
                                continue
                            while run > 15:
                                b.put(*ac[t][0xF0])
                                run -= 16
                            b.put(*ac[t][run << 4 | abs(zz[k]).bit_length()])
                            b.value(zz[k])
                            run = 0
                        if last < 63:
                            b.put(*ac[t][0])
    if b.n:
        b.put((1 << (8 - b.n)) - 1, 8 - b.n)
    return header(W, H, hm, vm, q) + bytes(b.out) + b"\xff\xd9"


def encode(rgb, quality=85, sampling="4:2:0") -> bytes:
    rgb = np.asarray(rgb)
    hm, vm = SAMPLING[sampling]
    return entropy_encode(coefficients(rgb, quality, sampling), rgb.shape[1], rgb.shape[0], hm, vm, quant_tables(quality))


def load_cases():
    """tests/golden/jpeg_encode_cases.npz as [(name, BGR input, quality, sampling, Pillow's bytes, Pillow's decode of them or None)]."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_encode_cases.npz"))
    off, blob, dec = z["offsets"], z["blob"], set(int(i) for i in z["decoded"])
    inputs = {}
    out = []
    for i, n in enumerate(z["names"]):
        j = int(z["input"][i])
        if j not in inputs:
            inputs[j] = z[f"in_{j}"]
        out.append((str(n), inputs[j], int(z["quality"][i]), str(z["sampling"][i]), blob[off[i]:off[i + 1]].tobytes(), z[f"rgb_{i}"] if i in dec else None))
    return out
