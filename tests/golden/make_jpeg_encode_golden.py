"""Writes the JPEG encoder's fixtures (needs Pillow; run by hand, never at test time):

    python tests/golden/make_jpeg_encode_golden.py

    jpeg_encode_cases.npz   in_<j>          the distinct BGR input arrays, uint8 [H, W, 3]
                            names [N]       "<W>x<H>_<content>_<sampling>_q<quality>"
                            input [N], quality [N], sampling [N]   the case's input array, quality and "4:2:0" | "4:2:2" | "4:4:4"
                            blob, offsets [N + 1]   what Pillow writes, Image.save(..., "JPEG", quality=q, subsampling=s): case i's file is
                                            blob[offsets[i]:offsets[i + 1]]
                            rgb_<i>         Pillow's decode of those bytes, for the few cases named in `decoded`
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

SIZES = [(1, 1), (8, 8), (2, 3), (17, 23), (20, 24), (36, 20), (33, 31), (61, 45), (100, 75), (130, 70)]       # (W, H)
BATCH_SIZES = [(33, 31), (61, 45), (130, 70)]              # five contents at one sampling and quality each, so batches can be formed
SUBS = ["4:2:0", "4:2:2", "4:4:4"]
QUALITIES = [10, 75, 85, 100]


def contents(w, h, k):
    """BGR arrays: noise, a second noise, a smooth ramp with small noise, a flat colour, a 0 / 255 pixel checkerboard, a rendered frame."""
    from strongsort_yolo_amd.synth import make_stream
    rng = np.random.default_rng(2000 + k)
    yy, xx = np.mgrid[0:h, 0:w]
    out = {"noise": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "noise2": rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
           "ramp": np.clip(np.stack([2 * yy + xx, 3 * xx, 255 - yy - xx], 2) + rng.integers(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8),
           "flat": np.broadcast_to(np.array([(53 * k + 20) % 256, (97 * k + 130) % 256, (11 * k + 240) % 256], np.uint8), (h, w, 3)).copy(),
           "checker": np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2),
           "synth": np.ascontiguousarray(make_stream(0, 640, 480, 8).frame_pixels(k)[40:40 + h, 60:60 + w])}
    return out


def pillow_bytes(bgr, quality, sub):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, "JPEG", quality=quality, subsampling=sub)
    return buf.getvalue()


def main():
    out, names, inp, qual, samp, decoded, files = {}, [], [], [], [], [], []
    n_in = 0
    for k, (w, h) in enumerate(SIZES):
        arrs = contents(w, h, k)
        index = {}
        for si, sub in enumerate(SUBS):
            r = k + si
            # (noise at quality 100 is the largest file by far: at the two largest sizes the checkerboard alone carries that quality)
            plan = [("noise", QUALITIES[r % 4] if w * h < 5000 else QUALITIES[r % 3]), ("ramp", QUALITIES[(r + 1) % 4]), ("flat", QUALITIES[(r + 2) % 4]), ("checker", 100), ("synth", 85)]
            if (w, h) in BATCH_SIZES:
                plan += [(kind, 85) for kind in ("noise", "noise2", "ramp", "flat") if (kind, 85) not in plan]
            for kind, q in plan:
                i = len(names)
                if kind not in index:
                    out[f"in_{n_in}"] = arrs[kind]
                    index[kind] = n_in
                    n_in += 1
                data = pillow_bytes(arrs[kind], q, sub)
                names.append(f"{w}x{h}_{kind}_{sub.replace(':', '')}_q{q}")
                inp.append(index[kind]); qual.append(q); samp.append(sub)
                files.append(data)
                if kind == "synth" and (w, h) in ((17, 23), (36, 20), (61, 45), (130, 70)):
                    out[f"rgb_{i}"] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
                    decoded.append(i)
    path = os.path.join(HERE, "jpeg_encode_cases.npz")
    np.savez_compressed(path, names=np.array(names), input=np.array(inp, np.int32), quality=np.array(qual, np.int32), sampling=np.array(samp),
                        decoded=np.array(decoded, np.int32), blob=np.frombuffer(b"".join(files), np.uint8),
                        offsets=np.cumsum([0] + [len(f) for f in files]).astype(np.int64), **out)
    print(path, os.path.getsize(path), "bytes;", len(names), "cases,", n_in, "inputs")


if __name__ == "__main__":
    main()
