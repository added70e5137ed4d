"""NumPy restatement of docs/JPEG.md §2 (baseline JPEG -> pixels, the arithmetic of libjpeg-turbo's defaults: JDCT_ISLOW, fancy
upsampling).  The specification in executable form; not a test module.

    info = parse(data)                       headers: width, height, components, tables, where the scan starts
    coefs, quant, info = coefficients(data)  per component [bh, bw, 64] int16 natural-order blocks; quant [4, 64] uint16 natural order
    rgb = decode(data)                       uint8 [H, W, 3] (RGB; rgb=False: BGR); dtype=np.int64 runs the same arithmetic without wrap
    y = prelimit(data)                       every IDCT result before the range limit (which zones of the limit does the file reach?)

Everything the device refuses raises Refused with the same cause.
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class Refused(ValueError):
    pass


def parse(data: bytes) -> dict:
    d = bytes(data)
    if len(d) < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise Refused("no SOI marker")
    p, n = 2, len(d)
    info = {"quant": np.zeros((4, 64), np.uint16), "have_q": [False] * 4, "dc": {}, "ac": {}, "ri": 0, "jfif": False, "adobe": None}
    sof = None
    while True:
        while p < n and d[p] != 0xFF:
            p += 1
        while p < n and d[p] == 0xFF:
            p += 1
        if p >= n:
            raise Refused("no scan")
        m = d[p]
        p += 1
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise Refused("no scan")
        if p + 2 > n:
            raise Refused("truncated header")
        L = (d[p] << 8) | d[p + 1]
        if L < 2 or p + L > n:
            raise Refused("truncated header")
        seg = d[p + 2:p + L]
        if m == 0xC0:
            if sof is not None:
                raise Refused("two frame headers")
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                raise Refused("bad frame header")
            if seg[0] != 8:
                raise Refused("12-bit samples")
            sof = {"height": (seg[1] << 8) | seg[2], "width": (seg[3] << 8) | seg[4],
                   "comps": [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])]}
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise Refused({0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless"}.get(m, "arithmetic or differential") + " JPEG (SOF%d)" % (m - 0xC0))
        elif m == 0xCC:
            raise Refused("arithmetic coding")
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                if pq != 0:
                    raise Refused("16-bit quantisation table")
                if tq > 3 or q + 65 > len(seg):
                    raise Refused("bad quantisation table")
                info["quant"][tq][ZIGZAG] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                info["have_q"][tq] = True
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    raise Refused("bad Huffman table")
                tc, th = seg[q] >> 4, seg[q] & 15
                counts = list(seg[q + 1:q + 17])
                tot = sum(counts)
                if tc > 1 or th > 3 or tot > 256 or q + 17 + tot > len(seg):
                    raise Refused("bad Huffman table")
                syms = seg[q + 17:q + 17 + tot]
                table, code, k = {}, 0, 0
                for ln in range(1, 17):
                    if counts[ln - 1] > (1 << ln) - code:            # more codes of this length than the code space has left
                        raise Refused("bad Huffman table")
                    for _ in range(counts[ln - 1]):
                        table[(ln, code)] = syms[k]
                        code += 1
                        k += 1
                    code <<= 1
                info["ac" if tc else "dc"][th] = table
                q += 17 + tot
        elif m == 0xDD:
            if len(seg) != 2:
                raise Refused("bad restart interval")
            info["ri"] = (seg[0] << 8) | seg[1]
        elif m == 0xE0 and seg[:5] == b"JFIF\0":
            info["jfif"] = True
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            info["adobe"] = seg[11]
        elif m == 0xDA:
            if sof is None:
                raise Refused("scan before the frame header")
            break
        p += L
    info.update(sof)
    H, W, comps = info["height"], info["width"], info["comps"]
    if not (1 <= H <= 8192 and 1 <= W <= 8192):
        raise Refused("sides must be 1 ... 8192")
    if len(comps) not in (1, 3):
        raise Refused("%d components (1 or 3 are decoded)" % len(comps))
    if info["adobe"] == 0 and len(comps) == 3:
        raise Refused("Adobe marker with transform 0 (RGB)")
    if len(comps) == 3 and not info["jfif"] and info["adobe"] is None and [c[0] for c in comps] == [82, 71, 66]:
        raise Refused("component ids R, G, B (RGB)")
    if len(comps) == 1:
        comps[0] = (comps[0][0], 1, 1, comps[0][3])              # a one-component scan is not interleaved: the factors do not matter
    else:
        if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            raise Refused("sampling factors " + " ".join("%dx%d" % (c[1], c[2]) for c in comps) + " (4:4:4, 4:2:2 and 4:2:0 are decoded)")
    if len(seg) < 1 or seg[0] != len(comps) or len(seg) != 4 + 2 * seg[0]:
        raise Refused("several scans")
    if tuple(seg[-3:]) != (0, 63, 0):
        raise Refused("scan header is not a baseline one (Ss 0, Se 63, Ah / Al 0)")
    sel = []
    for i in range(seg[0]):
        if seg[1 + 2 * i] != comps[i][0]:
            raise Refused("scan components out of order")
        sel.append((seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15))
    for (cid, h, v, tq), (td, ta) in zip(comps, sel):
        if tq > 3 or not info["have_q"][tq]:
            raise Refused("missing quantisation table %d" % tq)
        if td not in info["dc"]:
            raise Refused("missing DC Huffman table %d" % td)
        if ta not in info["ac"]:
            raise Refused("missing AC Huffman table %d" % ta)
    info["sel"] = sel
    info["scan"] = p + L
    info["hmax"], info["vmax"] = comps[0][1], comps[0][2]
    info["mcux"] = -(-W // (8 * info["hmax"]))
    info["mcuy"] = -(-H // (8 * info["vmax"]))
    return info


class _Bits:
    """The entropy-coded segment from `pos` to the next marker, FF00 unstuffed, as a bit array."""

    def __init__(self, d, pos):
        out = bytearray()
        n = len(d)
        while pos < n:
            b = d[pos]
            if b == 0xFF:
                if pos + 1 < n and d[pos + 1] == 0:
                    out.append(0xFF)
                    pos += 2
                    continue
                break
            out.append(b)
            pos += 1
        self.end = pos                                        # at the marker's FF (or the end of the data)
        self.bits = np.unpackbits(np.frombuffer(bytes(out), np.uint8)).tolist()
        self.i = 0

    def sym(self, table):
        """The next code.  One that starts inside the data and reaches beyond it is completed with zero bits and judged like any
        other, as the host decoder's bit reader does; one that starts beyond the data is read the same way, but `past` tells the
        caller not to judge its symbol.  Whoever consumed such bits finds `i` beyond the data at the end of the block."""
        code, bits, i = 0, self.bits, self.i
        self.past = i >= len(bits)
        for ln in range(1, 17):
            code = (code << 1) | (bits[i] if i < len(bits) else 0)
            i += 1
            s = table.get((ln, code))
            if s is not None:
                self.i = i
                return s
        raise Refused("data ends before the last MCU" if len(bits) - self.i < 16 else "Huffman code that does not exist")

    def receive_extend(self, s):
        if s == 0:
            return 0
        v = 0
        got = self.bits[self.i:self.i + s]
        for b in got + [0] * (s - len(got)):                      # (zero bits beyond the data, as in sym)
            v = (v << 1) | b
        self.i += s
        return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def coefficients(data: bytes):
    info = parse(data)
    d = bytes(data)
    comps, sel = info["comps"], info["sel"]
    mcux, mcuy = info["mcux"], info["mcuy"]
    coefs = [np.zeros((mcuy * v, mcux * h, 64), np.int16) for (_, h, v, _) in comps]
    br = _Bits(d, info["scan"])
    pred = [0] * len(comps)
    ri, rst = info["ri"], 0
    for m in range(mcux * mcuy):
        if ri and m and m % ri == 0:
            if len(br.bits) - br.i >= 8 or br.end + 1 >= len(d) or d[br.end] != 0xFF or d[br.end + 1] != 0xD0 + (rst & 7):
                raise Refused("bad restart marker")
            rst += 1
            br = _Bits(d, br.end + 2)
            pred = [0] * len(comps)
        my, mx = divmod(m, mcux)
        for ci, (_, h, v, _) in enumerate(comps):
            dc, ac = info["dc"][sel[ci][0]], info["ac"][sel[ci][1]]
            for by in range(v):
                for bx in range(h):
                    blk = coefs[ci][my * v + by, mx * h + bx]
                    s = br.sym(dc)
                    if s > 15:
                        raise Refused("data ends before the last MCU" if br.past else "bad DC category")
                    pred[ci] = (pred[ci] + br.receive_extend(s) + 32768) % 65536 - 32768
                    blk[0] = pred[ci]
                    k = 1
                    while k < 64:
                        rs = br.sym(ac)
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        if k > 63:
                            raise Refused("data ends before the last MCU" if br.past else "coefficient index beyond 63")
                        blk[ZIGZAG[k]] = br.receive_extend(s)
                        k += 1
                    if br.i > len(br.bits):                       # the block took bits that are not there
                        raise Refused("data ends before the last MCU")
    return coefs, info["quant"].copy(), info


_A, _B, _C, _D, _E, _F, _G, _H, _I, _J, _K, _L = 2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172


def _pass(x, s):
    """One 1-D ISLOW pass on x[0..7] (arrays), descale shift s."""
    x0, x1, x2, x3, x4, x5, x6, x7 = x
    r = 1 << (s - 1)
    z1 = (x2 + x6) * _C
    t2 = z1 - x6 * _H
    t3 = z1 + x2 * _D
    t0 = (x0 + x4) << 13
    t1 = (x0 - x4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = x7, x5, x3, x1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * _F
    o0, o1, o2, o3 = o0 * _A, o1 * _J, o2 * _L, o3 * _G
    z1, z2, z3, z4 = -z1 * _E, -z2 * _K, -z3 * _I + z5, -z4 * _B + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    return [(t10 + o3 + r) >> s, (t11 + o2 + r) >> s, (t12 + o1 + r) >> s, (t13 + o0 + r) >> s,
            (t13 - o0 + r) >> s, (t12 - o1 + r) >> s, (t11 - o2 + r) >> s, (t10 - o3 + r) >> s]


def idct_prelimit(coef, q, dtype=np.int32):
    """coef [..., 64] int16 natural order, q [64] -> the second pass's results [..., 8, 8] before the range limit."""
    d = (coef.astype(dtype) * q.astype(dtype)).reshape(coef.shape[:-1] + (8, 8))
    ws = np.stack(_pass([d[..., i, :] for i in range(8)], 11), axis=-2)          # down the columns
    return np.stack(_pass([ws[..., :, j] for j in range(8)], 18), axis=-1)       # along the rows


def idct_blocks(coef, q, dtype=np.int32):
    """coef [..., 64] int16 natural order, q [64] -> samples [..., 8, 8] uint8."""
    v = idct_prelimit(coef, q, dtype) & 1023
    return np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896))).astype(np.uint8)


def prelimit(data: bytes, dtype=np.int32):
    """Every sample of every block of the file before the range limit (padding blocks included), as one flat array."""
    coefs, quant, info = coefficients(data)
    return np.concatenate([idct_prelimit(c, quant[tq], dtype).reshape(-1) for c, (_, _, _, tq) in zip(coefs, info["comps"])])


def planes(data: bytes, dtype=np.int32):
    """The component planes cw x ch (padding dropped), and info."""
    coefs, quant, info = coefficients(data)
    H, W, hm, vm = info["height"], info["width"], info["hmax"], info["vmax"]
    out = []
    for c, (_, h, v, tq) in zip(coefs, info["comps"]):
        s = idct_blocks(c, quant[tq], dtype)
        bh, bw = s.shape[:2]
        s = s.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        out.append(s[:-(-H * v // vm), :-(-W * h // hm)])
    return out, info


def upsample(s, hs, vs, dtype=np.int32):
    """A chroma plane [ch, cw] -> [vs * ch, hs * cw] (hs 1 or 2, vs 1 or 2; 1x2 does not occur)."""
    if hs == 1:
        return s
    ch, cw = s.shape
    if cw <= 2:                                                       # libjpeg turns fancy upsampling off there
        return np.repeat(np.repeat(s, vs, axis=0), 2, axis=1)
    s = s.astype(dtype)
    lo = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    hi = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    if vs == 1:
        out = np.empty((ch, 2 * cw), dtype)
        out[:, 0::2] = (3 * s + lo + 1) >> 2
        out[:, 1::2] = (3 * s + hi + 2) >> 2
        return out
    out = np.empty((2 * ch, 2 * cw), dtype)
    for p in (0, 1):
        oth = np.clip(np.arange(ch) + (1 if p else -1), 0, ch - 1)
        c = 3 * s + s[oth]
        cl = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
        cr = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
        out[p::2, 0::2] = (3 * c + cl + 8) >> 4
        out[p::2, 1::2] = (3 * c + cr + 7) >> 4
    return out


def decode(data: bytes, rgb: bool = True, dtype=np.int32) -> np.ndarray:
    pl, info = planes(data, dtype)
    H, W = info["height"], info["width"]
    y = pl[0].astype(dtype)
    if len(pl) == 1:
        return np.repeat(y.astype(np.uint8)[:, :, None], 3, axis=2)
    hs, vs = info["hmax"], info["vmax"]
    cb = upsample(pl[1], hs, vs, dtype).astype(dtype)[:H, :W] - 128
    cr = upsample(pl[2], hs, vs, dtype).astype(dtype)[:H, :W] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    ch = (r, g, b) if rgb else (b, g, r)
    return np.stack([np.clip(c, 0, 255) for c in ch], axis=2).astype(np.uint8)
