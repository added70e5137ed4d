"""NumPy restatement of docs/JPEG.md §13, "Entropy coding on the device": the encoder's entropy stage as the data-parallel steps the
kernels take (csrc/ss_jpeg_enc.hip: k_jpegenc_hlen, k_jpegenc_hwrite, k_jpegenc_ffcount, k_jpegenc_stuff).  Not a test module.

    lay = layout(W, H, hm, vm)                     per scan position: component, block row / column, real?, DC predecessor (closed form)
    st = stages(coefs, W, H, hm, vm)               every stage's values: lens, pos, bits, unstuffed, ff_before, stuffed
    data = encode_file(coefs, W, H, hm, vm, q)     header + stuffed scan + FFD9
    coefs = crafted(name)                          the coefficient sets of the known-answer tests (32 x 16, 4:4:4)
    flat = library_layout(coefs, W, H, hm, vm)     the same blocks as ss_jpeg_coefficients lays them out

`coefs`: per component int16 [rows, columns, 64] natural-order blocks over at least its real blocks (jpeg_enc_ref.coefficients' form).
"""
import numpy as np

from tests import jpeg_enc_ref as ref
from tests.jpeg_ref import ZIGZAG

DC = [ref._codes(ref.DC_COUNTS[t], ref.DC_SYMS[t]) for t in range(2)]
AC = [ref._codes(ref.AC_COUNTS[t], ref.AC_SYMS[t]) for t in range(2)]
MAX_BLOCK_BITS = 20 + 63 * 26

CRAFT_W, CRAFT_H, CRAFT_Q, CRAFT_S = 32, 16, 100, "4:4:4"
CRAFTED = ("b_max", "c_zrl", "d_negative", "e_zero", "f_seed1", "f_seed2", "f_seed3")


def layout(W, H, hm, vm):
    """Step 1.  Arrays over the scan positions: comp, by, bx, real (bool), prev (scan position of the nearest earlier real block of the
    component, -1 for none; meaningless for a dummy).  The predecessor is the closed form the kernel uses, not a search."""
    mcux, mcuy = -(-W // (8 * hm)), -(-H // (8 * vm))
    bw, bh = -(-W // 8), -(-H // 8)
    assert -(-(-(-W // hm)) // 8) == mcux and -(-(-(-H // vm)) // 8) == mcuy           # chroma: every position is a real block
    nl, bpm = hm * vm, hm * vm + 2
    n = mcux * mcuy * bpm
    comp, by, bx, real, prev = (np.zeros(n, np.int64) for _ in range(5))
    for s in range(n):
        mcu, j = divmod(s, bpm)
        my, mx = divmod(mcu, mcux)
        if j >= nl:
            comp[s], by[s], bx[s], real[s], prev[s] = 1 + j - nl, my, mx, 1, s - bpm if mcu else -1
            continue
        jy, jx = divmod(j, hm)
        rw, rh = min(hm, bw - mx * hm), min(vm, bh - my * vm)                          # the MCU's real luma blocks: the left rw x rh
        assert rw >= 1 and rh >= 1
        by[s], bx[s] = my * vm + jy, mx * hm + jx
        real[s] = jx < rw and jy < rh
        if jx > 0:
            prev[s] = s - 1
        elif jy > 0:
            prev[s] = mcu * bpm + (jy - 1) * hm + rw - 1
        elif mcu > 0:
            pmy, pmx = divmod(mcu - 1, mcux)
            prev[s] = (mcu - 1) * bpm + (min(vm, bh - pmy * vm) - 1) * hm + min(hm, bw - pmx * hm) - 1
        else:
            prev[s] = -1
    return {"comp": comp, "by": by, "bx": bx, "real": real.astype(bool), "prev": prev, "mcux": mcux, "mcuy": mcuy}


def _value_bits(v, s):
    return (v - 1 if v < 0 else v) & ((1 << s) - 1)


def lane_codes(zz, diff, t):
    """Step 2 per lane, as the kernel's 64 lanes see a block: [(bits, length)] * 64.  Lane 0: the DC difference; lane k: a non-zero AC
    with the ZRLs of the zero run in front of it; lane 63 with a zero: EOB; every other lane nothing."""
    out = [(0, 0)] * 64
    s = abs(diff).bit_length()
    code, ln = DC[t][s]
    out[0] = (code << s | _value_bits(diff, s), ln + s)
    last = 0                                                                           # the last lane before k that holds a non-zero AC (0: none)
    for k in range(1, 64):
        v = zz[k]
        if v:
            run = k - 1 - last
            bits, n = 0, 0
            for _ in range(run >> 4):
                bits, n = bits << AC[t][0xF0][1] | AC[t][0xF0][0], n + AC[t][0xF0][1]
            s = abs(v).bit_length()
            code, ln = AC[t][(run & 15) << 4 | s]
            out[k] = ((bits << ln | code) << s | _value_bits(v, s), n + ln + s)
            last = k
        elif k == 63:
            out[k] = AC[t][0]
    return out


def stages(coefs, W, H, hm, vm):
    lay = layout(W, H, hm, vm)
    n = len(lay["comp"])
    zz = np.zeros((n, 64), np.int64)
    for s in range(n):
        if lay["real"][s]:
            zz[s] = coefs[lay["comp"][s]][lay["by"][s], lay["bx"][s]][ZIGZAG]
    codes = []
    for s in range(n):
        t = 1 if lay["comp"][s] else 0
        if not lay["real"][s]:
            codes.append(lane_codes([0] * 64, 0, t))                                   # a dummy: difference 0, EOB
            continue
        p = lay["prev"][s]
        assert p < s and (p < 0 or (lay["real"][p] and lay["comp"][p] == lay["comp"][s]))
        codes.append(lane_codes([int(x) for x in zz[s]], int(zz[s, 0]) - (int(zz[p, 0]) if p >= 0 else 0), t))
    lens = np.array([sum(c[1] for c in cs) for cs in codes], np.int64)
    assert lens.max() <= MAX_BLOCK_BITS
    pos = np.cumsum(lens) - lens                                                       # step 3 (Python ints / int64: no 32-bit positions)
    bits = int(lens.sum())
    stream = ["0"] * (-(-bits // 8) * 8)                                               # step 4: zero-initialised, every block at its position
    for s in range(n):
        text = "".join(format(c, f"0{ln}b") for c, ln in codes[s] if ln)
        assert len(text) == lens[s]
        stream[pos[s]:pos[s] + lens[s]] = text
    stream[bits:] = "1" * (len(stream) - bits)                                         # the last byte's padding
    unstuffed = np.packbits(np.array([ch == "1" for ch in stream], np.uint8)) if stream else np.zeros(0, np.uint8)
    ff = (unstuffed == 0xFF).astype(np.int64)                                          # step 5
    ff_before = np.cumsum(ff) - ff
    stuffed = np.zeros(len(unstuffed) + int(ff.sum()), np.uint8)
    stuffed[np.arange(len(unstuffed)) + ff_before] = unstuffed
    return {"lens": lens, "pos": pos, "bits": bits, "unstuffed": unstuffed.tobytes(), "ff_before": ff_before, "stuffed": stuffed.tobytes(), "layout": lay}


def encode_file(coefs, W, H, hm, vm, q) -> bytes:
    return ref.header(W, H, hm, vm, q) + stages(coefs, W, H, hm, vm)["stuffed"] + b"\xff\xd9"


def crafted(name):
    """Per component int16 [2, 4, 64] natural-order blocks for the 32 x 16 4:4:4 grid of the known-answer tests."""
    c = np.zeros((3, 2, 4, 64), np.int16)
    nat = np.asarray(ZIGZAG)                                                           # zig-zag index -> natural index
    if name == "b_max":                                                                # every AC part the maximum; DC differences of category 11 inside a block row
        c[...] = 1023
        for by in range(2):
            for bx in range(4):
                c[:, by, bx, 0] = 1023 if (bx + by) & 1 else -1023
    elif name == "c_zrl":                                                              # three ZRL, no EOB
        c[..., 0] = 5
        c[..., nat[63]] = 1
    elif name == "d_negative":
        c[...] = -1023
        c[..., 0] = 0
    elif name == "e_zero":
        pass
    elif name.startswith("f_seed"):
        rng = np.random.default_rng(int(name[6:]))
        cat = rng.integers(0, 11, c.shape)
        mag = np.where(cat > 0, rng.integers(0, 1 << 30, c.shape) % np.maximum(1 << np.maximum(cat - 1, 0), 1) + (1 << np.maximum(cat - 1, 0)), 0)
        mag = np.where(rng.random(c.shape) < 0.25, mag, 0)                             # sparse
        c[...] = np.where(rng.integers(0, 2, c.shape) == 1, -mag, mag)
    else:
        raise KeyError(name)
    return [c[0], c[1], c[2]]


def library_layout(coefs, W, H, hm, vm):
    """ss_jpeg_coefficients' layout: component after component, each one's blocks in raster order over its whole-MCU grid (zeros where the
    grid has no real block)."""
    mcux, mcuy = -(-W // (8 * hm)), -(-H // (8 * vm))
    out = []
    for k, c in enumerate(coefs):
        rows, cols = (mcuy * vm, mcux * hm) if k == 0 else (mcuy, mcux)
        g = np.zeros((rows, cols, 64), np.int16)
        r, w = min(rows, c.shape[0]), min(cols, c.shape[1])
        g[:r, :w] = c[:r, :w]
        out.append(g.reshape(-1))
    return np.concatenate(out)
