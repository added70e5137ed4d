"""Writes the fixtures of the device entropy stage (needs Pillow 12.2; run by hand, never at test time):

    python tests/golden/make_jpeg_entropy_golden.py

    jpeg_entropy_cases.npz   names [N]; per case i: bytes_i (uint8, the file) and rgb_i (uint8 [H,W,3], Pillow's decode)

      noise_224x160_444_q100     the unstuffed scan is longer than one tile of 1024 subsequences of 32 dwords (131 072 bytes)
      rst1_61x45_420_q50         restart_marker_blocks=1: every segment is shorter than a subsequence
      rst1_61x45_grey_q90
      opt_48x32_444_q100         optimised tables whose DHT holds codes longer than 9 bits: the second-level look-up
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))


def encode(arr, sub, quality, **kw):
    im = Image.fromarray(arr)
    if sub == "grey":
        im = im.convert("L")
    else:
        kw["subsampling"] = sub
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def dht_lengths(data):
    """The code lengths that occur in the file's Huffman tables."""
    p, seen = 2, set()
    while data[p + 1] != 0xDA:
        L = (data[p + 2] << 8) | data[p + 3]
        if data[p + 1] == 0xC4:
            q = p + 4
            while q < p + 2 + L:
                counts = data[q + 1:q + 17]
                seen |= {i + 1 for i, c in enumerate(counts) if c}
                q += 17 + sum(counts)
        p += 2 + L
    return seen


def main():
    from tests.jpeg_huff_ref import cut
    rng = np.random.default_rng(2024)
    cases = []
    noise = encode(rng.integers(0, 256, (160, 224, 3), dtype=np.uint8), "4:4:4", 100)
    raw, segs = cut(noise)
    assert len(segs) == 1 and segs[0][1] > 131072, segs[0][1]
    assert len(noise) < (1 << 20)
    cases.append(("noise_224x160_444_q100", noise))
    from strongsort_yolo_amd.synth import make_stream
    small = np.ascontiguousarray(make_stream(0, 640, 480, 8).frame_pixels(2)[5:50, 9:70, ::-1])     # a rendered frame: short MCUs
    for sub, q in (("4:2:0", 50), ("grey", 90)):
        data = encode(small, sub, q, restart_marker_blocks=1)
        raw, segs = cut(data)
        assert len(segs) > 1 and max(s[1] for s in segs) < 4 * 32
        cases.append((f"rst1_61x45_{sub.replace(':', '')}_q{q}", data))
    opt = encode(rng.integers(0, 256, (32, 48, 3), dtype=np.uint8), "4:4:4", 100, optimize=True)
    assert max(dht_lengths(opt)) > 9, dht_lengths(opt)
    cases.append(("opt_48x32_444_q100", opt))
    out = {}
    for i, (name, data) in enumerate(cases):
        out[f"bytes_{i}"] = np.frombuffer(data, np.uint8)
        out[f"rgb_{i}"] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    path = os.path.join(HERE, "jpeg_entropy_cases.npz")
    np.savez_compressed(path, names=np.array([c[0] for c in cases]), **out)
    print(path, os.path.getsize(path), [(n, len(d)) for n, d in cases])


if __name__ == "__main__":
    main()
