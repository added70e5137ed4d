"""Baseline files written from chosen coefficient blocks (tests/jpeg_enc_huff_ref.encode_file, NumPy only), for what no encoder-made
file reaches: IDCT results far outside a sample's range, and padding samples inside the last blocks that do not repeat the edge.
Not a test module; made once per process from fixed seeds.

    extreme()    the CRAFTED sets of jpeg_enc_huff_ref at 32 x 16, with the tables of quality 1, 50 and 100, at 4:4:4, 4:2:2, 4:2:0
    padding()    sparse random blocks (density 0.2, AC within +-20, quality-90 tables) over every real block, at ten sizes x 3 samplings

Both return [Case]: name, data (the file), W, H, hm, vm, coefs (the blocks it was written from, per component [rows, cols, 64]).
`expect(case)` is tests/jpeg_ref.py's word on the file: its RGB pixels (int32 arithmetic) and its coefficients in the library's layout.
"""
import functools
from collections import namedtuple

import numpy as np

from tests import jpeg_enc_huff_ref as wr
from tests import jpeg_ref
from tests.jpeg_enc_ref import SAMPLING, quant_tables

Case = namedtuple("Case", "name data W H hm vm coefs")
Expect = namedtuple("Expect", "rgb coef")

EXTREME_QUALITIES = (1, 50, 100)
PADDING_SIZES = ((1, 1), (2, 3), (3, 5), (9, 8), (17, 23), (20, 24), (33, 31), (36, 20), (61, 45), (130, 70))      # (W, H)
PADDING_DENSITY, PADDING_AC, PADDING_DC, PADDING_QUALITY = 0.2, 20, 40, 90


def real_blocks(W, H, hm, vm):
    """Per component (rows, columns) of the blocks that hold samples of the image."""
    cw, ch = -(-W // hm), -(-H // vm)
    return [(-(-H // 8), -(-W // 8))] + [(-(-ch // 8), -(-cw // 8))] * 2


@functools.lru_cache(maxsize=None)
def extreme():
    out = []
    for name in wr.CRAFTED:
        coefs = wr.crafted(name)
        for q in EXTREME_QUALITIES:
            for sub, (hm, vm) in SAMPLING.items():
                real = real_blocks(wr.CRAFT_W, wr.CRAFT_H, hm, vm)
                use = [c[:r, :w] for c, (r, w) in zip(coefs, real)]
                out.append(Case(f"{name}_q{q}_{sub.replace(':', '')}", wr.encode_file(use, wr.CRAFT_W, wr.CRAFT_H, hm, vm, quant_tables(q)),
                                wr.CRAFT_W, wr.CRAFT_H, hm, vm, use))
    return out


@functools.lru_cache(maxsize=None)
def padding():
    out = []
    q = quant_tables(PADDING_QUALITY)
    for k, (W, H) in enumerate(PADDING_SIZES):
        for j, (sub, (hm, vm)) in enumerate(SAMPLING.items()):
            rng = np.random.default_rng(2000 + 10 * k + j)             # (seeds under which no IDCT result leaves -512 .. 511)
            coefs = []
            for (r, w) in real_blocks(W, H, hm, vm):
                c = np.where(rng.random((r, w, 64)) < PADDING_DENSITY, rng.integers(-PADDING_AC, PADDING_AC + 1, (r, w, 64)), 0)
                c[..., 0] = rng.integers(-PADDING_DC, PADDING_DC + 1, (r, w))
                coefs.append(c.astype(np.int16))
            out.append(Case(f"pad_{W}x{H}_{sub.replace(':', '')}", wr.encode_file(coefs, W, H, hm, vm, q), W, H, hm, vm, coefs))
    return out


def library_layout(coefs):
    """jpeg_ref.coefficients' per-component blocks (whole-MCU grids) as ss_jpeg_coefficients lays them out."""
    return np.concatenate([c.reshape(-1) for c in coefs])


@functools.lru_cache(maxsize=None)
def _expect(data):
    return Expect(jpeg_ref.decode(data), library_layout(jpeg_ref.coefficients(data)[0]))


def expect(case):
    return _expect(case.data)


def known_answer(case, flat):
    """[(component, the blocks of `flat` (library layout) at the component's real blocks, the blocks the file was written from)]."""
    mcux, mcuy = -(-case.W // (8 * case.hm)), -(-case.H // (8 * case.vm))
    out, at = [], 0
    for k, c in enumerate(case.coefs):
        rows, cols = (mcuy * case.vm, mcux * case.hm) if k == 0 else (mcuy, mcux)
        grid = flat[at:at + rows * cols * 64].reshape(rows, cols, 64)
        at += rows * cols * 64
        out.append((k, grid[:c.shape[0], :c.shape[1]], c))
    assert at == flat.size
    return out
