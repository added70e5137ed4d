"""Writes the JPEG fixtures (needs Pillow; run by hand, never at test time):

    python tests/golden/make_jpeg_golden.py --image <a photograph, e.g. the reference's testing.jpg>

    jpeg_cases.npz     names [N]; per case i: bytes_i (uint8, the file) and rgb_i (uint8 [H,W,3], Pillow's decode)
    jpeg_sequence.npz  12 rendered 160 x 128 frames, 4:2:0 quality 85: bytes_i and rgb_i
    jpeg_refused.npz   streams the decoder refuses: <name> (uint8, the file) and the cause it must name in `causes`
"""
import argparse
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

SIZES = [(1, 1), (8, 8), (3, 5), (4, 9), (17, 9), (33, 31), (61, 45), (130, 70)]          # (W, H)
SUBS = ["4:4:4", "4:2:2", "4:2:0", "grey"]
QUALITIES = [30, 90, 100]


def encode(arr, sub, quality, optimize=False, restart=0, **kw):
    im = Image.fromarray(arr)
    if sub == "grey":
        im = im.convert("L")
        kw2 = {}
    else:
        kw2 = {"subsampling": sub}
    if restart:
        kw2["restart_marker_blocks"] = restart
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=quality, optimize=optimize, **kw2, **kw)
    return buf.getvalue()


def pil_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def contents(photo, w, h, k):
    from strongsort_yolo_amd.synth import make_stream
    rng = np.random.default_rng(1000 + k)
    py, px = (37 * k) % (photo.shape[0] - h), (91 * k) % (photo.shape[1] - w)
    yield "photo", photo[py:py + h, px:px + w]
    yield "noise", rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yield "flat", np.broadcast_to(np.array([(53 * k + 20) % 256, (97 * k + 130) % 256, (11 * k + 240) % 256], np.uint8), (h, w, 3)).copy()
    yield "synth", np.ascontiguousarray(make_stream(0, 640, 480, 8).frame_pixels(k)[5:5 + h, 9:9 + w, ::-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", required=True)
    a = ap.parse_args()
    photo = np.asarray(Image.open(a.image).convert("RGB"))
    out, names, n = {}, [], 0
    for k, (w, h) in enumerate(SIZES):
        for kind, arr in contents(photo, w, h, k):
            for sub in SUBS:
                # the three qualities at the small sizes; one each, in turn, at the two largest (the file stays under 1 MiB)
                for q in (QUALITIES if w * h < 2000 else [QUALITIES[n % 3]]):
                    opt, rst = n % 4 == 1, 3 if n % 5 == 2 else 0
                    data = encode(arr, sub, q, opt, rst)
                    names.append(f"{w}x{h}_{kind}_{sub.replace(':', '')}_q{q}" + ("_opt" if opt else "") + ("_rst" if rst else ""))
                    out[f"bytes_{n}"] = np.frombuffer(data, np.uint8)
                    out[f"rgb_{n}"] = pil_decode(data)
                    n += 1
    np.savez_compressed(os.path.join(HERE, "jpeg_cases.npz"), names=np.array(names), **out)

    from strongsort_yolo_amd.synth import make_stream
    st = make_stream(3, 640, 512, 6)                            # rendered at 640 x 512, every fourth pixel kept
    seq = {}
    for i in range(12):
        data = encode(np.ascontiguousarray(st.render(st.next_frame())[::4, ::4, ::-1]), "4:2:0", 85)
        seq[f"bytes_{i}"] = np.frombuffer(data, np.uint8)
        seq[f"rgb_{i}"] = pil_decode(data)
    np.savez_compressed(os.path.join(HERE, "jpeg_sequence.npz"), **seq)

    arr = photo[100:148, 200:264]
    good = encode(arr, "4:2:2", 90)
    ref = {"progressive": encode(arr, "4:2:0", 90, progressive=True)}
    buf = io.BytesIO()
    Image.fromarray(arr).convert("CMYK").save(buf, "JPEG", quality=90)
    ref["cmyk"] = buf.getvalue()
    sof = good.index(b"\xff\xc0")
    assert good[sof + 11] == 0x21
    ref["s440"] = good[:sof + 11] + b"\x12" + good[sof + 12:]                       # luma 1x2: 4:4:0
    sos = good.index(b"\xff\xda")
    ref["cut_scan"] = good[:sos + (len(good) - sos) // 2] + b"\xff\xd9"
    rst = encode(arr, "4:2:0", 90, restart=2)
    at = rst.index(b"\xff\xd1", rst.index(b"\xff\xda"))
    ref["bad_restart"] = rst[:at + 1] + b"\xd5" + rst[at + 2:]
    dqt = good.index(b"\xff\xdb")
    ln = (good[dqt + 2] << 8) | good[dqt + 3]
    assert ln == 67 and good[dqt + 4] >> 4 == 0
    wide = bytes([0x10 | good[dqt + 4]]) + b"".join(bytes([0, v]) for v in good[dqt + 5:dqt + 69])
    ref["dqt16"] = good[:dqt + 2] + bytes([0, 131]) + wide + good[dqt + 2 + ln:]
    causes = {"progressive": "progressive", "cmyk": "4 components", "s440": "sampling factors", "cut_scan": "data ends before the last MCU",
              "bad_restart": "bad restart marker", "dqt16": "16-bit quantisation table"}
    np.savez_compressed(os.path.join(HERE, "jpeg_refused.npz"), good=np.frombuffer(good, np.uint8), good_rgb=pil_decode(good),
                        causes=np.array([f"{k}={v}" for k, v in causes.items()]), **{k: np.frombuffer(v, np.uint8) for k, v in ref.items()})
    for f in ("jpeg_cases.npz", "jpeg_sequence.npz", "jpeg_refused.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes;", n, "cases")


if __name__ == "__main__":
    main()
