"""Command line of the reference script, kept: `--source ... --track --count` (yolo_multi_model.py:341-354).

What is kept is the per-stream loop (:244-339), the labels file (:34-39, :165-169), the class-count analytics
(:284-305) — as an incremental per-id majority-class counter instead of re-reading the whole CSV every frame
 — and, with `--save`, the annotated output (:58-162, :311-331): the drawing runs as an overlay kernel
on the device (overlay.py, N2) on the frame that is ALREADY there (the throughput path keeps a device copy of every frame
of a group: one upload and one download per frame) and the frames go to a sink (N3).  Frame sources (N3): `synthetic[:N]`,
a `.npy` stack [T,H,W,3], a directory of images (Pillow; with `--device-decode` a JPEG directory or a raw `.mjpeg` file stays encoded and is decoded on the
device, docs/JPEG.md) and — when OpenCV is importable — a video file or a camera index
through `cv2.VideoCapture` (:252); sinks: `.npy`, raw BGR24, a PNG directory, with `--device-encode` a raw `.mjpeg` file or a JPEG directory whose frames
are encoded on the device (docs/JPEG.md "Encoding") and — with OpenCV — `cv2.VideoWriter` (:256-260).
OpenCV is optional: this environment has none, there the video branches raise a clear error (no GUI: imshow is out of scope).
"""
from __future__ import annotations

import argparse
import os
import time
from collections import Counter, defaultdict
from typing import Iterator, Optional

import numpy as np


# ---- frame sources (N3) --------------------------------------------------------------------------------
JPEG_EXT, MJPEG_EXT = (".jpg", ".jpeg"), (".mjpeg", ".mjpg")


def _image_names(spec: str):
    return sorted(f for f in os.listdir(spec) if f.lower().endswith((".jpg", ".jpeg", ".png", ".bmp")))


def _pil():
    """Pillow's Image module, if this interpreter has it."""
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


def encoded_source_error(spec: str) -> Optional[str]:
    """Why `spec` cannot feed --device-decode (None: it can): a directory of .jpg / .jpeg files or a raw .mjpeg / .mjpg file whose
    first frame the device decoder accepts (baseline JPEG, docs/JPEG.md)."""
    from .jpeg import probe, split_mjpeg
    if os.path.isdir(spec):
        names = _image_names(spec)
        if not names or not all(f.lower().endswith(JPEG_EXT) for f in names):
            return f"--device-decode: '{spec}' must hold .jpg / .jpeg images only"
        first = os.path.join(spec, names[0])
        try:
            with open(first, "rb") as f:
                probe(f.read())
        except ValueError as e:
            return f"--device-decode: '{first}': {e}"
        return None
    if spec.lower().endswith(MJPEG_EXT) and os.path.isfile(spec):
        try:
            if next(split_mjpeg(spec), None) is None:
                return f"--device-decode: '{spec}' holds no JPEG frame"
        except ValueError as e:
            return f"--device-decode: '{spec}': {e}"
        return None
    return f"--device-decode: '{spec}' is neither a directory of .jpg / .jpeg images nor a .mjpeg / .mjpg file"


def frame_source(spec: str, limit: Optional[int] = None, encoded: bool = False) -> Iterator[np.ndarray]:
    """BGR uint8 frames of a source; encoded=True (JPEG directories and raw MJPEG files only): jpeg.EncodedFrames, still encoded."""
    if encoded:
        from .jpeg import EncodedFrame, split_mjpeg
        why = encoded_source_error(spec)
        if why:
            raise ValueError(why)
        if os.path.isdir(spec):
            for k, f in enumerate(_image_names(spec)):
                if limit is not None and k >= limit:
                    break
                with open(os.path.join(spec, f), "rb") as fh:
                    yield EncodedFrame(fh.read())
        else:
            for k, fr in enumerate(split_mjpeg(spec)):
                if limit is not None and k >= limit:
                    break
                yield fr
    elif spec.startswith("synthetic"):
        from .synth import make_stream
        n = int(spec.split(":")[1]) if ":" in spec else 100
        st = make_stream(0, 640, 480, 8)
        for k in range(n if limit is None else min(n, limit)):
            yield st.frame_pixels(k).copy()
    elif spec.endswith(".npy"):
        arr = np.load(spec, mmap_mode="r")
        for k in range(len(arr) if limit is None else min(len(arr), limit)):
            yield np.ascontiguousarray(arr[k])
    elif os.path.isdir(spec):
        from PIL import Image
        for k, f in enumerate(_image_names(spec)):
            if limit is not None and k >= limit:
                break
            yield np.asarray(Image.open(os.path.join(spec, f)).convert("RGB"))[:, :, ::-1].copy()   # BGR like cv2
    elif spec.lower().endswith(MJPEG_EXT) and os.path.isfile(spec) and _pil() is not None:
        import io
        from .jpeg import split_bytes
        with open(spec, "rb") as fh:
            buf = fh.read()
        for k, seg in enumerate(split_bytes(buf)):
            if limit is not None and k >= limit:
                break
            yield np.asarray(_pil().open(io.BytesIO(seg)).convert("RGB"))[:, :, ::-1].copy()
    else:
        yield from _video_source(spec, limit)


VIDEO_EXT = (".mp4", ".avi", ".mov", ".mkv", ".m4v", ".webm", ".mpg", ".mpeg", ".wmv")


def _cv2():
    """OpenCV, if this interpreter has it (it is not a dependency: decoding / encoding video is the only use)."""
    try:
        import cv2
        return cv2
    except ImportError:
        return None


def _video_source(spec: str, limit: Optional[int]) -> Iterator[np.ndarray]:
    """A video file, a stream URL or a camera index through cv2.VideoCapture — the reference's only source kind
    (`cv2.VideoCapture(int(source) if source == '0' else source)`, yolo_multi_model.py:252; here every all-digit source is a
    camera index, App. C notes that the reference's '1' stays a path)."""
    is_cam = spec.isdigit()
    if not (is_cam or "://" in spec or spec.lower().endswith(VIDEO_EXT)):
        raise ValueError(f"cannot open source '{spec}' (synthetic[:N] | stack.npy | image directory | video file / camera index with OpenCV)")
    cv2 = _cv2()
    if cv2 is None:
        raise RuntimeError(f"source '{spec}' is a video / camera: that needs OpenCV (`import cv2` failed in this interpreter); "
                           f"decode it to a .npy stack or an image directory instead")
    cap = cv2.VideoCapture(int(spec) if is_cam else spec)
    try:
        if not cap.isOpened():                               # the reference checks this after creating its writer (:262)
            raise RuntimeError(f"cv2.VideoCapture could not open '{spec}'")
        k = 0
        while limit is None or k < limit:
            ok, frame = cap.read()                           # BGR uint8 [H,W,3], :272
            if not ok:
                break
            yield np.ascontiguousarray(frame)
            k += 1
    finally:
        cap.release()


# ---- frame sink (N3) ------------------------------------------------------------------------------------------
class FrameSink:
    """Where annotated frames go — the reference writes `output/<name>_output.mp4` with cv2.VideoWriter at 15 fps
    (yolo_multi_model.py:258-260, :331); there is no encoder in this environment, so the sink writes
      *.npy      one uint8 stack [T,H,W,3] (BGR), saved at close
      *.bgr      raw BGR24 frames appended as they arrive + `<path>.json` {width, height, fps, frames} (ffmpeg -f rawvideo
                 -pix_fmt bgr24 -s WxH -r fps turns it into the reference's mp4)
      directory  frame_000000.png ... (Pillow)
    and, with device_encode=True (the CLI's --device-encode), baseline JPEG encoded on the device (jpeg.encode, docs/JPEG.md; with
    device_entropy=True, --device-encode-entropy, its Huffman coding too):
      *.mjpeg / *.mjpg   the frames' files concatenated (jpeg.split_mjpeg and --device-decode read it back)       kind "mjpeg"
      directory          frame_000000.jpg ... (the path ends in a separator or is an existing directory)          kind "jpgdir"
    These two take frames that are still on the device (`write_device`); `write` uploads a host frame into the same path.  Frames
    are collected in a device buffer and encoded a group (up to GROUP) at a time, on flush() and close()."""
    GROUP = 32

    @staticmethod
    def encoded_kind(path: str) -> Optional[str]:
        """The device-encoded kind a --save path selects, None when it selects neither."""
        if path.lower().endswith(MJPEG_EXT):
            return "mjpeg"
        if path.endswith(("/", os.sep)) or os.path.isdir(path):
            return "jpgdir"
        return None

    def __init__(self, path: str, fps: int = 15, device_encode: bool = False, engine=None, quality: int = 85, subsampling: str = "4:2:0",
                 device_entropy: bool = False):
        self.path, self.fps, self.n, self.shape = path, fps, 0, None
        self.engine, self.quality, self.subsampling = engine, quality, subsampling
        self.entropy = "device" if device_entropy else "host"   # jpeg.encode's entropy: Huffman coding on the device too (docs/JPEG.md §13)
        self._buf, self._held = None, 0                      # device frames waiting for their group's encode
        if device_encode:
            self.kind = self.encoded_kind(path)
            if self.kind is None:
                raise ValueError(f"sink '{path}': device encoding writes a .mjpeg / .mjpg file or a directory of .jpg files")
        else:
            self.kind = ("npy" if path.endswith(".npy") else "bgr" if path.endswith((".bgr", ".raw")) else
                         "video" if path.lower().endswith(VIDEO_EXT) else "dir")
        self._writer = None
        if self.kind == "video" and _cv2() is None:
            raise RuntimeError(f"sink '{path}' is a video file: that needs OpenCV (`import cv2` failed); use .bgr (raw BGR24 + .json), .npy or a directory")
        if self.kind in ("dir", "jpgdir"):
            os.makedirs(path, exist_ok=True)
        else:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self._frames = []
        self._f = open(path, "wb") if self.kind in ("bgr", "mjpeg") else None

    def _slot(self, shape):
        """The next free frame of the device buffer (encoding what it holds first when it is full or of another size)."""
        import torch
        if self.engine is None:
            raise RuntimeError(f"sink '{self.path}' encodes on the device: it needs an engine (FrameSink(..., engine=...))")
        if self._buf is not None and (self._held == self.GROUP or tuple(self._buf.shape[1:]) != tuple(shape)):
            self.flush()
        if self._buf is None or tuple(self._buf.shape[1:]) != tuple(shape):
            self._buf = torch.empty((self.GROUP,) + tuple(shape), dtype=torch.uint8, device=self.engine.device)
        self._held += 1
        self.n += 1
        self.shape = tuple(shape)
        return self._buf[self._held - 1]

    def write_device(self, dev_frame):
        """A frame on the device (uint8 [H,W,3], BGR): copied into the sink's buffer there — the caller may reuse its tensor."""
        if self.kind not in ("mjpeg", "jpgdir"):
            raise ValueError(f"sink '{self.path}' ({self.kind}) takes host frames: write()")
        self._slot(dev_frame.shape).copy_(dev_frame)

    def flush(self):
        """Encode and write the device frames collected so far (the device-encoded kinds; nothing to do for the others)."""
        if not self._held:
            return
        from .jpeg import encode
        files = encode(self.engine, self._buf[:self._held], self.quality, self.subsampling, entropy=self.entropy)
        first, self._held = self.n - self._held, 0
        for k, data in enumerate(files):
            if self.kind == "mjpeg":
                self._f.write(data)
            else:
                with open(os.path.join(self.path, f"frame_{first + k:06d}.jpg"), "wb") as f:
                    f.write(data)

    def write(self, frame: np.ndarray):
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        if self.kind in ("mjpeg", "jpgdir"):
            slot = self._slot(frame.shape)
            self.engine.upload(slot, frame)
            return
        self.shape = frame.shape
        if self.kind == "npy":
            self._frames.append(frame.copy())
        elif self.kind == "bgr":
            self._f.write(frame.tobytes())
        elif self.kind == "video":
            if self._writer is None:                         # cv2.VideoWriter(path, mp4v, 15 fps, (w, h)), yolo_multi_model.py:258-260
                cv2 = _cv2()
                self._writer = cv2.VideoWriter(self.path, cv2.VideoWriter_fourcc(*"mp4v"), self.fps, (frame.shape[1], frame.shape[0]))
            self._writer.write(frame)
        else:
            from PIL import Image
            Image.fromarray(frame[:, :, ::-1]).save(os.path.join(self.path, f"frame_{self.n:06d}.png"))
        self.n += 1

    def close(self):
        self.flush()
        if self.kind == "mjpeg":
            self._f.close()
        if self.kind == "video" and self._writer is not None:
            self._writer.release()
        if self.kind == "npy":
            np.save(self.path, np.stack(self._frames) if self._frames else np.zeros((0, 0, 0, 3), np.uint8))
        elif self.kind == "bgr":
            self._f.close()
            import json
            h, w = (self.shape or (0, 0, 3))[:2]
            json.dump({"width": int(w), "height": int(h), "fps": self.fps, "frames": self.n, "pix_fmt": "bgr24"}, open(self.path + ".json", "w"))


# ---- labels file + counting (N1) -------------------------------------------------------------------------
class LabelsWriter:
    """`frameId cls id conf x1 y1 x2 y2 -1 -1 -1 -1` per tracked box (yolo_multi_model.py:165-169).
    compat=True reproduces the reference's quirks (frameId always 0, :32; append mode, :39)."""

    def __init__(self, path: str, compat: bool = False, obb: bool = False):
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        self.f = open(path, "a" if compat else "w")
        self.compat = compat
        # an oriented-box model (docs/OBB.md §5): the labels file holds the envelopes, <name>_labels_obb.txt beside it the rotated boxes
        self.f_obb = open(path[:-4] + "_obb.txt", "a" if compat else "w") if obb else None

    def write(self, frame_id: int, results) -> int:
        n = 0
        for r in results:
            b = None if r is None else r.boxes if r.boxes is not None else getattr(r, "obb", None)
            if b is None or b.id is None:
                continue
            if self.f_obb is not None and b is not r.boxes:                     # frame cls id conf cx cy w h theta
                for conf, cls, id_, q in zip(b.conf, b.cls, b.id, b.xywhr.tolist()):
                    self.f_obb.write(f"{0 if self.compat else frame_id} {int(cls)} {int(id_)} {round(float(conf), 3)} "
                                     f"{q[0]:.2f} {q[1]:.2f} {q[2]:.2f} {q[3]:.2f} {q[4]:.5f}\n")
            for bbox in b:
                for conf, cls, xyxy, id_ in zip(bbox.conf, bbox.cls, bbox.xyxy, bbox.id):
                    x1, y1, x2, y2 = (int(v) for v in xyxy)                 # reference :166 int() box corners
                    fid = 0 if self.compat else frame_id
                    self.f.write(f"{fid} {int(cls)} {int(id_)} {round(float(conf), 3)} {x1} {y1} {x2} {y2} -1 -1 -1 -1\n")
                    n += 1
        self.f.flush()
        if self.f_obb is not None:
            self.f_obb.flush()
        return n

    def close(self):
        self.f.close()
        if self.f_obb is not None:
            self.f_obb.close()


class DetsWriter:
    """--eval-det-gt: every frame's boxes in the labels file's line format with id -1, `frame cls -1 conf x1 y1 x2 y2 -1 -1 -1 -1`,
    tracked or not; with an oriented-box model also `<name>_dets_obb.txt`: `frame cls -1 conf cx cy w h theta` (docs/DETEVAL.md §4)."""

    def __init__(self, path: str, obb: bool = False):
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        self.f = open(path, "w")
        self.f_obb = open(path[:-4] + "_obb.txt", "w") if obb else None

    def write(self, frame_id: int, results) -> int:
        n = 0
        for r in results:
            b = None if r is None else r.boxes if r.boxes is not None else getattr(r, "obb", None)
            if b is None or len(b) == 0:
                continue
            if self.f_obb is not None and b is not r.boxes:
                for conf, cls, q in zip(b.conf, b.cls, b.xywhr.tolist()):
                    self.f_obb.write(f"{frame_id} {int(cls)} -1 {round(float(conf), 3)} {q[0]:.2f} {q[1]:.2f} {q[2]:.2f} {q[3]:.2f} {q[4]:.5f}\n")
            for conf, cls, xyxy in zip(b.conf, b.cls, b.xyxy):
                x1, y1, x2, y2 = (int(v) for v in xyxy)
                self.f.write(f"{frame_id} {int(cls)} -1 {round(float(conf), 3)} {x1} {y1} {x2} {y2} -1 -1 -1 -1\n")
                n += 1
        self.f.flush()
        if self.f_obb is not None:
            self.f_obb.flush()
        return n

    def close(self):
        self.f.close()
        if self.f_obb is not None:
            self.f_obb.close()


def eval_det_post(args: dict, eng, outdir: str, name: str, obb: bool, summary: dict) -> None:
    """--eval-det-gt after the stream: <name>_dets.txt (an oriented-box model: <name>_dets_obb.txt by ProbIoU, against the ground
    truth's own `_obb` file) scored on the device into <name>_det_metrics.json; AP, AP50, AR100 into the summary."""
    from . import deteval
    gt_path = args["eval_det_gt"]
    if obb:
        gt_path = gt_path if gt_path.endswith("_obb.txt") else gt_path[:-4] + "_obb.txt"
        if not os.path.isfile(gt_path):
            raise ValueError(f"--eval-det-gt: an oriented-box model is scored against the rotated ground truth: no such file: {gt_path}")
        gt, dt = deteval.read_labels_obb(gt_path), deteval.read_labels_obb(os.path.join(outdir, f"{name}_dets_obb.txt"))
        ok = lambda r: (r[:, 4] > 0) & (r[:, 5] > 0)
    else:
        gt, dt = deteval.read_labels(gt_path), deteval.read_labels(os.path.join(outdir, f"{name}_dets.txt"))
        ok = lambda r: (r[:, 4] > r[:, 2]) & (r[:, 5] > r[:, 3])
    dropped = int(np.count_nonzero(~ok(gt)) + np.count_nonzero(~ok(dt)))       # int() corners can close a box of less than a pixel
    gt, dt = gt[ok(gt)], dt[ok(dt)]
    kw = {"max_dets": tuple(args["eval_det_max_dets"])} if args.get("eval_det_max_dets") else {}
    if args.get("eval_det_classes"):
        kw["classes"] = list(args["eval_det_classes"])
    m = deteval.evaluate(gt, dt, eng, similarity="probiou" if obb else "iou", **kw)
    m.update(gt_rows=len(gt), det_rows=len(dt), dropped_rows=dropped, similarity="probiou" if obb else "iou")
    deteval.write_metrics(os.path.join(outdir, f"{name}_det_metrics.json"), m)
    for fig in ("AP", "AP50", "AR100"):
        summary[fig] = m[fig]


class ClassCounter:
    """Objects per class = number of track ids whose majority class is that class (yolo_multi_model.py:293-300),
    maintained incrementally: O(boxes) per frame instead of O(file)."""

    def __init__(self, names):
        self.names = names
        self.votes = defaultdict(Counter)

    def update(self, results):
        for r in results:
            b = None if r is None else r.boxes if r.boxes is not None else getattr(r, "obb", None)
            if b is None or b.id is None:
                continue
            for cls, id_ in zip(b.cls, b.id):
                self.votes[int(id_)][int(cls)] += 1

    def counts(self) -> dict:
        c = Counter()
        for votes in self.votes.values():
            top = max(votes.values())
            c[min(k for k, v in votes.items() if v == top)] += 1     # ties -> lowest class id (pandas mode()[0])
        # the plate's order is the reference's: sorted by class NAME (yolo_multi_model.py:305; testing.jpg shows {'backpack': 1, 'bicycle': 4, ...})
        return dict(sorted(((self.names.get(k, str(k)), v) for k, v in c.items()), key=lambda item: item[0]))


DEFAULT_WEIGHTS = "yolo11n-pose.pt"       # the model file the reference loads (/root/reference/yolo_multi_model.py:17)


def slice_kwargs(args: dict) -> dict:
    """--slice and its companions as YOLO(...)'s keywords ({} without --slice); a ValueError names what is wrong."""
    hw = args.get("slice")
    given = [f for f, d in (("slice_overlap", 0.2), ("slice_merge", "nmm"), ("slice_metric", "ios"), ("slice_thr", 0.5), ("no_slice_full", False))
             if args.get(f, d) != d]
    if hw is None:
        if given:
            raise ValueError(f"--{given[0].replace('_', '-')} is an option of sliced inference: it needs --slice H W")
        return {}
    from .slicing import SliceConfig
    if "seg" in os.path.basename(str(args.get("weights", ""))):
        raise ValueError("--slice cannot run a segmentation model (a row's mask coefficients belong to its tile's prototypes)")
    if args.get("reid_model", "osnet") == "auto":
        raise ValueError("--slice cannot feed --reid-model auto (the detector's anchor indices are per tile)")
    kw = dict(slice_hw=tuple(hw), slice_overlap=args.get("slice_overlap", 0.2), slice_full=not args.get("no_slice_full", False),
              slice_merge=args.get("slice_merge", "nmm"), slice_metric=args.get("slice_metric", "ios"), slice_thr=args.get("slice_thr", 0.5))
    SliceConfig(kw["slice_hw"], kw["slice_overlap"], kw["slice_full"], kw["slice_merge"], kw["slice_metric"], kw["slice_thr"])
    return kw


# ---- per-stream loop ------------------------------------------------------------------------------------------
def process_video(args: dict, model=None) -> dict:
    """One stream (yolo_multi_model.py:244-339).  Returns a summary instead of showing a window."""
    source, track, count = args["source"], args["track"], args["count"]
    if model is None:
        from .yolo import YOLO
        model = YOLO(args.get("weights", DEFAULT_WEIGHTS), random_init_ok=args.get("random_init", False), reid_weights=args.get("reid_weights"),
                     reid_fp32=not args.get("reid_f16", False), half=not args.get("fp32", False),
                     device_masks=args.get("device_masks", False), tracker_type=args.get("tracker", "strongsort"),
                     camera_motion=args.get("camera_motion", False), with_reid=args.get("with_reid", False),
                     reid_model=args.get("reid_model", "osnet"), with_pose=args.get("with_pose", False),
                     gmc_method=args.get("gmc_method", "ecc"), ocsort_use_byte=args.get("ocsort_use_byte", False), **slice_kwargs(args),
                     **({"hybrid_asso": args.get("hybrid_asso", "hmiou"), "hybrid_use_byte": not args.get("hybrid_no_byte", False)}
                        if args.get("tracker") == "hybridsort" else {}),
                     **({"track_bank": True} if args.get("mtmc") and track else {}))
        model.overrides.update(conf=0.3, iou=0.4, agnostic_nms=False, max_det=1000)      # :18-21
    name = os.path.splitext(os.path.basename(str(source)))[0] or "stream"
    writer = LabelsWriter(os.path.join(args.get("outdir", "output"), f"{name}_labels.txt"), args.get("compat", False),
                          obb=getattr(model, "_obb", False))
    counter = ClassCounter(model.names)
    det_writer = (DetsWriter(os.path.join(args.get("outdir", "output"), f"{name}_dets.txt"), obb=getattr(model, "_obb", False))
                  if args.get("eval_det_gt") else None)                   # --eval-det-gt: the boxes of every frame, tracked or not (docs/DETEVAL.md)
    frames, t0, fps = 0, time.time(), 0.0
    batch = int(args.get("batch", 16))
    src = frame_source(str(source), args.get("limit"), encoded=bool(args.get("device_decode", False)))
    sink = (FrameSink(args["save"], device_encode=bool(args.get("device_encode", False)), quality=int(args.get("save_quality", 85)),
                      subsampling=args.get("save_subsampling", "4:2:0"), device_entropy=bool(args.get("device_encode_entropy", False)))
            if args.get("save") else None)       # annotated output (N2 + N3), off by default
    on_device = sink is not None and sink.kind in ("mjpeg", "jpgdir")
    overlay, fps_str = None, ""
    gsi_on, gsi_rows = bool(args.get("gsi", False)) and track, []         # --gsi: every frame's tracked rows, smoothed after the stream (docs/GSI.md)
    aflink_on = bool(args.get("aflink")) and track                        # --aflink: the same rows, linked after the stream (docs/AFLINK.md)
    keep_rows = gsi_on or aflink_on
    if keep_rows:
        from .gsi import rows_of
    # --line / --zone / --heatmap: crossings, occupancy, dwell and heat counted on the device, frame by frame, on the rows the labels file records (docs/ZONES.md)
    zone_cfg, zc, zf = zone_config(args, len(model.names)) if track else None, None, None
    zone_asked = bool(args.get("lines") or args.get("zones") or args.get("heatmap"))
    redact_cfg, redactor = (redact_config(args) if sink is not None else None), None      # --redact: the saved frames only (docs/REDACT.md)

    def emit(frame, res):
        """labels, counts and (with --save) the annotated frame of one processed frame; reference :284-331"""
        nonlocal frames, t0, fps, overlay, fps_str, zc, zf, redactor
        if det_writer is not None:
            det_writer.write(frames, res)
        if track:
            writer.write(frames, res)
            if keep_rows:
                gsi_rows.append(rows_of(res, frames))
            if count:
                counter.update(res)
            if zone_cfg is not None:
                from . import zones
                if zc is None:
                    overlay = overlay or model.overlay()
                    zc = zones.ZoneCounter(zone_cfg, overlay.eng, frame_hw=frame.shape[:2])
                zf = zc.update(zones.label_rows(res))
        frames += 1
        if frames % 10 == 0:                     # reference :321-326 (10-frame window)
            fps = 10 / max(time.time() - t0, 1e-9)
            fps_str = f"FPS: {fps:.2f}"
            t0 = time.time()
        if sink is not None:
            if overlay is None:
                overlay = model.overlay()
            if sink.engine is None:
                sink.engine = overlay.eng
            cnt = counter.counts() if (count and track) else None
            zkw = {"zones": zf} if zf is not None else {}     # the heat blended on the resident frame, then the lines and zones drawn with the rest
            if redact_cfg is not None:                       # the people are hidden first, on the device; labels, dets and metrics never see it
                if redactor is None:
                    from .redact import Redactor
                    redactor = Redactor(redact_cfg, overlay.eng)
                zkw["redact"] = redactor
            dev_frame = getattr(res[0], "orig_img_device", None) if res else None
            if dev_frame is not None and on_device:  # drawn and encoded where it is: only the sparse coefficients of its JPEG come back
                sink.write_device(overlay.annotate_resident(dev_frame, res, cnt, fps_str, **zkw))
            elif dev_frame is not None:              # the frame is still on the device: draw there, ONE download, no second upload
                sink.write(overlay.draw_resident(dev_frame, res, cnt, fps_str, **zkw))
            else:
                sink.write(overlay.draw(frame, res, cnt, fps_str, **zkw))

    if track and batch > 1 and hasattr(model, "track_stream"):
        # a file / synthetic source can supply frames ahead: groups of `batch` frames through the overlapped pipeline
        # (same rows as frame-by-frame model.track; --batch 1 keeps the reference's per-frame call, :41)
        kw = {"keep_device_frames": True} if sink is not None else {}
        if args.get("device_entropy", False):
            kw["jpeg_entropy"] = "device"
        for res in model.track_stream(src, batch=batch, device=args.get("device", 0), **kw):
            emit(res[0].orig_img, res)
        src = ()
    for frame in src:
        if track:
            res = model.track(frame, verbose=False, device=args.get("device", 0), persist=True, tracker=f"{args.get('tracker', 'strongsort')}.yaml")
        else:
            res = model.predict(frame, verbose=False, device=args.get("device", 0))
            if count:                                # reference :280-282: counting needs tracking
                print("[INFO] count works only when objects are tracking.. so use both flags (--track --count)")
                frames += 1
                break
            if zone_asked:
                print("[INFO] lines, zones and the heat map work only when objects are tracking.. so use them with --track")
                frames += 1
                break
        emit(frame, res)
    if sink is not None:
        sink.close()
    writer.close()
    if det_writer is not None:
        det_writer.close()
    summary = {"source": str(source), "frames": frames, "fps": fps, "counts": counter.counts() if count and track else {}}
    if zc is not None:
        from . import zones
        outdir = args.get("outdir", "output")
        summary["zones"] = zones.write_summary(os.path.join(outdir, f"{name}_zones.json"), zc.totals(0), zone_cfg, model.names)
        if zone_cfg.heat:
            np.save(os.path.join(outdir, f"{name}_heat.npy"), zc.heatmap(0))
        zone_hw = zc.frame_hw
        zc.close()
    if args.get("mtmc") and track and frames:
        # --mtmc: this stream's track bank beside its labels file; the parent links the streams' tables after all of them (docs/MTMC.md)
        from . import mtmc
        mtmc.save_table(os.path.join(args.get("outdir", "output"), f"{name}_bank.npz"), model.track_bank())
    if gsi_on:
        # GSI post-processing of the whole run on the device context the overlay uses; the labels file above stays as it is
        from . import gsi
        eng = (overlay or model.overlay()).eng
        rows = np.concatenate(gsi_rows, 0) if gsi_rows else np.zeros((0, 8))
        rows, status = gsi.gsi(rows, eng, interval=int(args.get("gsi_interval", gsi.INTERVAL)), tau=float(args.get("gsi_tau", gsi.TAU)))
        summary["gsi_rows"] = gsi.write_labels(os.path.join(args.get("outdir", "output"), f"{name}_labels_gsi.txt"), rows)
        summary["gsi_status"] = {k: sum(1 for v in status.values() if v == k) for k in (0, 1, 2)}
        if zc is not None:                       # the same counts over the smoothed rows as their file records them
            from . import moteval, zones
            tot, _ = zones.replay(moteval.read_labels(os.path.join(args.get("outdir", "output"), f"{name}_labels_gsi.txt")), zone_cfg, eng, zone_hw)
            zones.write_summary(os.path.join(args.get("outdir", "output"), f"{name}_zones_gsi.json"), tot, zone_cfg, model.names)
    if aflink_on:
        eng = (overlay or model.overlay()).eng
        rows = np.concatenate(gsi_rows, 0) if gsi_rows else np.zeros((0, 8))
        aflink_post(rows, eng, args, args.get("outdir", "output"), name, summary)
    if args.get("eval_gt") and track:
        # HOTA and CLEAR MOT of the files just written against the ground truth (docs/MOTEVAL.md): the labels file holds int()
        # corners, so the file is what is scored; with --gsi its file is a second pair of the same device call
        from . import moteval
        eng = (overlay or model.overlay()).eng
        outdir = args.get("outdir", "output")
        names = ["labels"] + (["labels_gsi"] if gsi_on else []) + (["labels_aflink"] if aflink_on else []) + (["labels_aflink_gsi"] if aflink_on and gsi_on else [])
        with_identity = bool(args.get("eval_identity"))            # IDF1, IDP, IDR: a second device call for the same pairs
        scored = moteval.evaluate(moteval.read_labels(args["eval_gt"]), [moteval.read_labels(os.path.join(outdir, f"{name}_{k}.txt")) for k in names],
                                  eng, thr=float(args.get("eval_thr", 0.5)), **({"identity": True} if with_identity else {}))
        moteval.write_metrics(os.path.join(outdir, f"{name}_metrics.json"), dict(zip(names, scored)) if len(names) > 1 else scored[0])
        for k, m in zip(names, scored):
            for fig in ("HOTA", "MOTA", "IDSW") + (("IDF1",) if with_identity else ()):
                summary[fig + k[len("labels"):]] = m[fig]
    if det_writer is not None and frames:
        pipe = model._stream_pipe or model._pipe or model._pred_pipe      # (a detection-only run has no overlay to borrow the context from)
        eval_det_post(args, overlay.eng if overlay is not None else pipe.eng, args.get("outdir", "output"), name, getattr(model, "_obb", False), summary)
    return summary


def redact_config(args: dict):
    """--redact and its options -> redact.RedactConfig, None without --redact; ValueError names a bad value."""
    if not args.get("redact"):
        return None
    from .redact import RedactConfig
    return RedactConfig(effect=args["redact"], strength=args.get("redact_strength"), region=args.get("redact_region", "box"),
                        classes=args.get("redact_classes"), pad=float(args.get("redact_pad", 0.0)),
                        fill_color=tuple(args.get("redact_color") or (0, 0, 0)))


def redact_refusal(a) -> Optional[str]:
    """Why the parsed --redact flags cannot be used, None when they can."""
    opts = a.redact_region != "box" or a.redact_strength is not None or a.redact_classes is not None or a.redact_pad != 0.0 or a.redact_color is not None
    if opts and not a.redact:
        return "--redact-region, --redact-strength, --redact-classes, --redact-pad and --redact-color are options of --redact"
    if a.redact and not a.save:
        return "--redact hides people in the annotated output: it needs --save"
    if a.redact == "fill" and a.redact_strength is not None:
        return "--redact-strength does not apply to --redact fill"
    if a.redact_color is not None and a.redact != "fill":
        return "--redact-color is the colour of --redact fill"
    base = os.path.basename(a.weights)
    if a.redact and a.redact_region == "head" and "pose" not in base:
        return "--redact-region head needs a pose model (--weights ...-pose.pt): this detector has no keypoint columns"
    if a.redact and a.redact_region == "mask" and "seg" not in base:
        return "--redact-region mask needs a segmentation model (--weights ...-seg.pt): this detector has no masks"
    if a.redact and a.redact_region in ("head", "mask") and "obb" in base:
        return f"--redact-region {a.redact_region} is not available on an oriented-box model"
    return None


def zone_config(args: dict, n_names: int):
    """The ZoneConfig the flags ask for (None: none of --line, --zone, --heatmap was given)."""
    if not (args.get("lines") or args.get("zones") or args.get("heatmap")):
        return None
    from .zones import ZoneConfig
    cfg = ZoneConfig(lines=list(args.get("lines") or []), zones=list(args.get("zones") or []), anchor=args.get("zone_anchor", "bottom"),
                     max_gap=int(args.get("zone_gap", 30)), n_classes=min(max(int(n_names), 1), 128), heat=args.get("heatmap"),
                     heat_cell=int(args.get("heat_cell", 8)), heat_alpha=int(round(float(args.get("heat_alpha", 0.5)) * 256)))
    cfg.validate()
    return cfg


def aflink_post(rows, eng, args: dict, outdir: str, name: str, summary: dict):
    """--aflink: the tracked rows of a finished run linked on the device (docs/AFLINK.md) into <name>_labels_aflink.txt; with --gsi
    the StrongSORT++ order, AFLink then GSI, into <name>_labels_aflink_gsi.txt.  The other labels files stay as they are."""
    from . import aflink, gsi
    model = args["aflink"] if isinstance(args["aflink"], aflink.PostLinker) else aflink.load(args["aflink"])
    info = {}
    linked, _ = aflink.link(rows, eng, model, thr_t=tuple(args.get("aflink_thr_t", aflink.THR_T)), thr_s=float(args.get("aflink_thr_s", aflink.THR_S)),
                            thr_p=float(args.get("aflink_thr_p", aflink.THR_P)), info=info)
    os.makedirs(outdir, exist_ok=True)
    gsi.write_labels(os.path.join(outdir, f"{name}_labels_aflink.txt"), linked)
    summary["aflink_candidates"], summary["aflink_links"] = info["candidates"], info["links"]
    if args.get("gsi", False):
        both, _ = gsi.gsi(linked, eng, interval=int(args.get("gsi_interval", gsi.INTERVAL)), tau=float(args.get("gsi_tau", gsi.TAU)))
        gsi.write_labels(os.path.join(outdir, f"{name}_labels_aflink_gsi.txt"), both)
    return linked


def source_name(source) -> str:
    """The name a source's output files carry (process_video)."""
    return os.path.splitext(os.path.basename(str(source)))[0] or "stream"


def mtmc_refusal(track: bool, sources, tracker: str, with_reid: bool, reid_model: str, weights: str) -> Optional[str]:
    """Why --mtmc cannot run with these flags (None: it can)."""
    if not track:
        return "--mtmc links tracked ids across sources: it needs --track"
    if len(sources) < 2:
        return "--mtmc links ids across cameras: it needs at least two --source"
    names = [source_name(s) for s in sources]
    if len(set(names)) != len(names):
        return "--mtmc: two sources share the output name '" + next(n for n in names if names.count(n) > 1) + "'"
    from .mtmc import bank_refusal
    from .nets import OBB_DETECTORS
    why = bank_refusal(tracker, with_reid, reid_model, os.path.basename(str(weights)).lower().replace(".pt", "") in OBB_DETECTORS)
    return f"--mtmc: {why}" if why else None


def mtmc_post(sources, outdir: str, engine, thr: float, min_rows: int = 1) -> dict:
    """--mtmc, after every stream has finished: the streams' <name>_bank.npz tables linked on the device (docs/MTMC.md), per source
    <name>_labels_mtmc.txt = the labels file with global ids in the id column, and mtmc.json.  Every other file stays as it is."""
    from . import mtmc
    names = [source_name(s) for s in sources]
    tables = [mtmc.load_table(os.path.join(outdir, f"{n}_bank.npz")) for n in names]
    info = {}
    maps = mtmc.link(tables, engine, thr=thr, min_rows=min_rows, info=info)
    for n, m in zip(names, maps):
        mtmc.rewrite_labels(os.path.join(outdir, f"{n}_labels.txt"), os.path.join(outdir, f"{n}_labels_mtmc.txt"), m)
    return mtmc.write_summary(os.path.join(outdir, "mtmc.json"), [str(s) for s in sources], tables, maps, info)


def _save_path(a, i: int) -> Optional[str]:
    """--save of source i: the path itself for one source, `<root>_<i><ext>` for several (a JPEG directory: `<directory>/stream_<i>/`)."""
    if not a.save or len(a.source) == 1:
        return a.save
    if a.device_encode and FrameSink.encoded_kind(a.save) == "jpgdir":
        return os.path.join(a.save, f"stream_{i}", "")
    root, ext = os.path.splitext(a.save)
    return f"{root}_{i}{ext}"


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--source", nargs="+", type=str, default=["synthetic:30"], help="frame sources")
    p.add_argument("--track", action="store_true")
    p.add_argument("--count", action="store_true")
    p.add_argument("--weights", default=DEFAULT_WEIGHTS, help="detector weights; the reference's default model file (yolo_multi_model.py:17)")
    p.add_argument("--reid-fp32", action="store_true", help="(the default since round 6) ReID crops + OSNet in fp32 on the fp32 kernels: float distances within 1e-4 of a CPU fp32 network")
    p.add_argument("--reid-f16", action="store_true", help="throughput mode: ReID crops + OSNet with f16 activations (1.7x the stream rate; appearance distances off by up to 3e-2)")
    p.add_argument("--fp32", action="store_true", help="every network operation in fp32 (the reference passes no half=): detector on the fp32 convolution kernels too — NMS keep lists equal the CPU fp32 network's; about 0.39x the f16 throughput")
    p.add_argument("--reid-weights", default=None, help="OSNet-x0.25 state_dict for the tracker's appearance features (required with --track unless --random-init; "
                                                          "used by --tracker botsort only with --with-reid, by deep_ocsort always, not by bytetrack or ocsort)")
    p.add_argument("--tracker", choices=("strongsort", "bytetrack", "botsort", "ocsort", "deep_ocsort", "hybridsort"), default="strongsort",
                   help="strongsort (default): OSNet appearance + NSA Kalman; bytetrack / botsort: the BYTE family on IoU and scores, no ReID network (docs/BYTETRACK.md); "
                        "ocsort: OC-SORT, motion only, no ReID network (docs/OCSORT.md); deep_ocsort: Deep OC-SORT, OC-SORT with OSNet appearance and, "
                        "with --camera-motion, compensated filters and observations (docs/DEEPOCSORT.md; needs --reid-weights or --random-init)")
    p.add_argument("--hybrid-asso", choices=("hmiou", "iou"), default="hmiou",
                   help="--tracker hybridsort only: the association value, height-modulated IoU (default) or plain IoU (docs/HYBRIDSORT.md)")
    p.add_argument("--hybrid-no-byte", action="store_true",
                   help="--tracker hybridsort only: without its BYTE stage, the second association on the rows scoring between 0.1 and 0.25")
    p.add_argument("--ocsort-use-byte", action="store_true",
                   help="--tracker ocsort only: OC-SORT's BYTE stage, a second association on the rows scoring between 0.1 and 0.25")
    p.add_argument("--camera-motion", action="store_true",
                   help="ECC camera-motion compensation on the device: StrongSORT moves its track boxes, botsort applies BoT-SORT's GMC "
                        "(docs/BYTETRACK.md §1b); not with --tracker bytetrack")
    p.add_argument("--gmc-method", choices=("ecc", "sparseOptFlow"), default="ecc",
                   help="--camera-motion with --tracker botsort only: ecc (default) or sparseOptFlow, the estimator Ultralytics' botsort.yaml "
                        "names (corners, pyramidal Lucas-Kanade, RANSAC similarity on the device; docs/BYTETRACK.md §1f)")
    p.add_argument("--with-reid", action="store_true",
                   help="--tracker botsort only: BoT-SORT's ReID branch, OSNet-x0.25 appearance beside IoU (docs/BYTETRACK.md §1c; needs --reid-weights or --random-init)")
    p.add_argument("--reid-model", choices=("osnet", "auto"), default="osnet",
                   help="--with-reid only: osnet (default) runs OSNet-x0.25 on the crops; auto reads the features from the detector's own "
                        "head inputs (Ultralytics' model: auto, docs/BYTETRACK.md §1d) — no second weights file, not with --reid-weights")
    p.add_argument("--with-pose", action="store_true",
                   help="--tracker botsort on a pose model only: the keypoint (OKS) term beside IoU (docs/BYTETRACK.md §1e); not with --with-reid")
    p.add_argument("--limit", type=int, default=None)
    p.add_argument("--save", default=None, help="write annotated frames: stack.npy | video.bgr (raw BGR24 + .json) | directory of PNGs | video.mp4 (needs OpenCV) | "
                                                "with --device-encode: clip.mjpeg (raw concatenated JPEG) or a directory of .jpg files")
    p.add_argument("--device-encode", action="store_true",
                   help="encode the annotated frames as baseline JPEG on the device (colour, DCT and quantisation in csrc/ss_jpeg_enc.hip, Huffman on host "
                        "threads; the same bytes as Pillow, docs/JPEG.md); needs --save clip.mjpeg / clip.mjpg or --save <directory>/")
    p.add_argument("--device-encode-entropy", action="store_true",
                   help="--device-encode: Huffman-code the frames on the device too (docs/JPEG.md §13); only the files' own bytes come back, the same bytes")
    p.add_argument("--save-quality", type=int, default=85, help="--device-encode: JPEG quality 1 .. 100")
    p.add_argument("--save-subsampling", choices=("4:2:0", "4:2:2", "4:4:4"), default="4:2:0", help="--device-encode: chroma subsampling")
    p.add_argument("--batch", type=int, default=16, help="frames per group on the throughput path (1: per-frame model.track calls as in the reference)")
    p.add_argument("--random-init", action="store_true", help="run seeded random-init networks when the weights file is missing")
    p.add_argument("--device-decode", action="store_true",
                   help="JPEG directories and raw .mjpeg files: decode baseline JPEG on the device (Huffman on host threads, the rest in "
                        "csrc/ss_jpeg.hip; same pixels as Pillow, docs/JPEG.md); needs --track and --batch > 1")
    p.add_argument("--device-entropy", action="store_true",
                   help="--device-decode: decode the Huffman code on the device too (docs/JPEG.md §12); the host only parses headers and copies the scans")
    p.add_argument("--device-masks", action="store_true", help="segmentation models: assemble masks and trace their outlines on the device (csrc/ss_mask.hip) instead of on the host")
    p.add_argument("--gsi", action="store_true",
                   help="--track only: after the stream, GSI post-processing (StrongSORT++'s gap interpolation + Gaussian-process smoothing on the "
                        "device, docs/GSI.md) of the tracked rows into <name>_labels_gsi.txt beside the labels file; any --tracker")
    p.add_argument("--gsi-interval", type=int, default=20, help="--gsi: gaps shorter than this many frames are filled")
    p.add_argument("--gsi-tau", type=float, default=10.0, help="--gsi: the length scale adapts as tau ln(tau^3 / track length)")
    p.add_argument("--aflink", default=None, metavar="WEIGHTS",
                   help="--track only: after the stream, AFLink (StrongSORT++'s tracklet linking, docs/AFLINK.md) of the tracked rows on the device "
                        "with the PostLinker checkpoint WEIGHTS, into <name>_labels_aflink.txt; with --gsi also AFLink then GSI into "
                        "<name>_labels_aflink_gsi.txt; any --tracker")
    p.add_argument("--aflink-thr-t", type=int, nargs=2, default=[0, 30], metavar=("A", "B"), help="--aflink: a pair needs A <= frame gap < B")
    p.add_argument("--aflink-thr-s", type=float, default=75.0, help="--aflink: a pair needs at most this distance between the tracklet ends")
    p.add_argument("--aflink-thr-p", type=float, default=0.05, help="--aflink: a pair is linked only if its cost is below this, in (0, 1]")
    p.add_argument("--eval-gt", nargs="+", default=None, metavar="PATH",
                   help="--track only: ground-truth labels files (the labels file's line format), one per source; after the stream "
                        "<name>_labels.txt (with --gsi / --aflink also their files) is scored against it on the device, HOTA and CLEAR MOT "
                        "(docs/MOTEVAL.md), into <name>_metrics.json")
    p.add_argument("--eval-thr", type=float, default=0.5, help="--eval-gt: CLEAR MOT's similarity threshold, in (0, 1]")
    p.add_argument("--eval-identity", action="store_true",
                   help="--eval-gt only: also the identity metrics IDTP, IDFN, IDFP, IDF1, IDP, IDR at --eval-thr, into the same <name>_metrics.json")
    p.add_argument("--eval-det-gt", nargs="+", default=None, metavar="PATH",
                   help="ground-truth labels files (the labels file's line format; id < 0 marks a crowd region), one per source; with or without "
                        "--track every frame's boxes go to <name>_dets.txt with id -1 and after the stream are scored against it on the device, "
                        "COCO AP and AR (docs/DETEVAL.md), into <name>_det_metrics.json; an -obb model is scored by ProbIoU from the _obb files")
    p.add_argument("--eval-det-max-dets", type=int, nargs="+", default=None, metavar="N", help="--eval-det-gt: the detections kept per image and class, rising (1 10 100)")
    p.add_argument("--eval-det-classes", type=int, nargs="+", default=None, metavar="CLS", help="--eval-det-gt: score only these classes")
    p.add_argument("--line", action="append", default=[], metavar="X0,Y0,X1,Y1",
                   help="--track only, repeatable (up to 16): count the tracks that cross the directed segment a -> b, inward (onto its s >= 0 side) "
                        "and outward, by class, on the device (docs/ZONES.md) into <name>_zones.json; any --tracker")
    p.add_argument("--zone", action="append", default=[], metavar="X0,Y0,X1,Y1,...",
                   help="--track only, repeatable (up to 16): a polygon of 3 to 32 vertices; entries, exits, peak occupancy and dwell into <name>_zones.json")
    p.add_argument("--zone-anchor", choices=("bottom", "centre"), default="bottom", help="--line / --zone: the point of a box that is tested")
    p.add_argument("--zone-gap", type=int, default=30, help="--line / --zone: a track unseen for more frames than this starts anew (1 .. 32)")
    p.add_argument("--heatmap", choices=("anchor", "box"), default=None,
                   help="--track only: a cumulative heat map of the anchors or of the boxes on the device into <name>_heat.npy; with --save it is blended over the frames")
    p.add_argument("--heat-cell", type=int, default=8, help="--heatmap: pixels a side of a heat cell, a power of two from 1 to 64")
    p.add_argument("--heat-alpha", type=float, default=0.5, help="--heatmap with --save: weight of the heat colour, 0 .. 1")
    p.add_argument("--mtmc", action="store_true",
                   help="--track with two or more --source only: every stream keeps one pooled OSNet descriptor per track id on the device, and after "
                        "all streams the tracklets are linked across the sources (docs/MTMC.md) into <name>_labels_mtmc.txt (the labels file with "
                        "global ids) and mtmc.json; needs a tracker with OSNet features (strongsort, deep_ocsort, botsort --with-reid)")
    p.add_argument("--mtmc-thr", type=float, default=0.2, help="--mtmc: clusters merge while their average cosine distance is below this")
    p.add_argument("--mtmc-min-rows", type=int, default=1, help="--mtmc: a track with fewer rows than this keeps a global id of its own")
    p.add_argument("--slice", type=int, nargs=2, default=None, metavar=("H", "W"),
                   help="sliced inference (docs/SLICE.md): run the detector on overlapping H x W tiles of every frame and merge their rows on the device; the detector costs T times as much")
    p.add_argument("--slice-overlap", type=float, default=0.2, help="--slice: overlap of neighbouring tiles as a ratio of the tile, in [0, 1)")
    p.add_argument("--slice-merge", choices=("nmm", "nms"), default="nmm", help="--slice: merge duplicates into their union (SAHI's GREEDYNMM) or drop them")
    p.add_argument("--slice-metric", choices=("ios", "iou"), default="ios", help="--slice: intersection over the smaller area, or over the union")
    p.add_argument("--slice-thr", type=float, default=0.5, help="--slice: the match threshold")
    p.add_argument("--no-slice-full", action="store_true", help="--slice: do not add the whole frame as one more tile")
    p.add_argument("--redact", choices=("blur", "pixelate", "fill"), default=None,
                   help="--save only: hide the detected objects in the saved frames on the device before anything is drawn (csrc/ss_redact.hip, docs/REDACT.md); "
                        "labels, dets, zones and metrics files are unchanged")
    p.add_argument("--redact-region", choices=("box", "ellipse", "head", "mask"), default="box",
                   help="--redact: the box, the ellipse inscribed in it, the head from a pose model's face keypoints, or a segmentation model's silhouette")
    p.add_argument("--redact-strength", type=int, default=None, help="--redact: blur radius 1 .. 31 (default 15) or pixelate cell 4, 8, 16, 32 (default 16)")
    p.add_argument("--redact-classes", type=int, nargs="+", default=None, metavar="CLS", help="--redact: only these classes (default: every class)")
    p.add_argument("--redact-pad", type=float, default=0.0, help="--redact with box / ellipse: this fraction of the box side is added on each side")
    p.add_argument("--redact-color", type=int, nargs=3, default=None, metavar=("B", "G", "R"), help="--redact fill: the colour (default 0 0 0)")
    a = p.parse_args(argv)
    from . import zones as _zones
    try:
        slice_kwargs(vars(a))
        a.line, a.zone = [_zones.parse_line(t) for t in a.line], [_zones.parse_zone(t) for t in a.zone]
        if not 0.0 <= a.heat_alpha <= 1.0:
            raise ValueError("--heat-alpha must be 0 .. 1")
        zone_config({"lines": a.line, "zones": a.zone, "heatmap": a.heatmap, "zone_anchor": a.zone_anchor, "zone_gap": a.zone_gap,
                     "heat_cell": a.heat_cell, "heat_alpha": a.heat_alpha}, 80)
        why = redact_refusal(a)
        if why:
            raise ValueError(why)
        redact_config(vars(a))
    except ValueError as e:
        p.error(str(e))
    if a.mtmc:
        why = mtmc_refusal(a.track, a.source, a.tracker, a.with_reid, a.reid_model, a.weights)
        if why:
            p.error(why)
        if not (a.mtmc_thr == a.mtmc_thr and abs(a.mtmc_thr) < float("inf")) or a.mtmc_min_rows < 0:
            p.error("--mtmc-thr must be finite and --mtmc-min-rows >= 0")
    elif a.mtmc_thr != 0.2 or a.mtmc_min_rows != 1:
        p.error("--mtmc-thr and --mtmc-min-rows are options of --mtmc")
    if a.eval_identity and not a.eval_gt:
        p.error("--eval-identity adds to what --eval-gt scores: it needs --eval-gt")
    if a.eval_gt and not a.track:
        p.error("--eval-gt scores tracked rows: it needs --track")
    if a.eval_gt and len(a.eval_gt) != len(a.source):
        p.error("--eval-gt takes one ground-truth file per --source")
    for path in a.eval_gt or ():
        if not os.path.isfile(path):
            p.error(f"--eval-gt: no such file: {path}")
    if a.eval_gt and not 0.0 < a.eval_thr <= 1.0:
        p.error("--eval-thr must be in (0, 1]")
    if (a.eval_det_max_dets or a.eval_det_classes) and not a.eval_det_gt:
        p.error("--eval-det-max-dets and --eval-det-classes are options of detection scoring: each needs --eval-det-gt")
    if a.eval_det_gt and len(a.eval_det_gt) != len(a.source):
        p.error("--eval-det-gt takes one ground-truth file per --source")
    for path in a.eval_det_gt or ():
        if not os.path.isfile(path):
            p.error(f"--eval-det-gt: no such file: {path}")
    if a.eval_det_max_dets and (min(a.eval_det_max_dets) < 1 or any(y <= x for x, y in zip(a.eval_det_max_dets, a.eval_det_max_dets[1:]))):
        p.error("--eval-det-max-dets must be positive and rising")
    if a.gsi and not a.track:
        p.error("--gsi post-processes tracked rows: it needs --track")
    if a.gsi and (a.gsi_interval < 1 or not a.gsi_tau > 0):
        p.error("--gsi-interval must be >= 1 and --gsi-tau > 0")
    if a.aflink and not a.track:
        p.error("--aflink post-processes tracked rows: it needs --track")
    if a.aflink and not os.path.isfile(a.aflink):
        p.error(f"--aflink: no such file: {a.aflink}")
    if a.aflink and not 0 <= a.aflink_thr_t[0] < a.aflink_thr_t[1]:
        p.error("--aflink-thr-t A B must satisfy 0 <= A < B")
    if a.aflink and not (a.aflink_thr_s >= 0 and a.aflink_thr_s < float("inf")):
        p.error("--aflink-thr-s must be finite and >= 0")
    if a.aflink and not 0.0 < a.aflink_thr_p <= 1.0:
        p.error("--aflink-thr-p must be in (0, 1]")
    if a.tracker == "ocsort":
        for flag, on in (("--camera-motion", a.camera_motion), ("--with-reid", a.with_reid), ("--with-pose", a.with_pose)):
            if on:
                p.error(f"{flag} is not available with --tracker ocsort (OC-SORT is motion only, docs/OCSORT.md)")
    if a.tracker == "hybridsort":
        for flag, on in (("--camera-motion", a.camera_motion), ("--with-reid", a.with_reid), ("--with-pose", a.with_pose),
                         ("--ocsort-use-byte", a.ocsort_use_byte)):
            if on:
                p.error(f"{flag} is not available with --tracker hybridsort (Hybrid-SORT is motion only and its BYTE stage is its own, docs/HYBRIDSORT.md)")
        if a.reid_model != "osnet":
            p.error("--reid-model auto is BoT-SORT's: --tracker hybridsort reads no features")
        if a.gmc_method != "ecc":
            p.error("--gmc-method is a camera-motion estimator: --tracker hybridsort has no camera-motion compensation")
        if "-obb" in os.path.basename(a.weights):
            p.error("--tracker hybridsort associates on axis-aligned boxes: an oriented-box model needs --tracker bytetrack or botsort")
    elif a.hybrid_asso != "hmiou" or a.hybrid_no_byte:
        p.error("--hybrid-asso and --hybrid-no-byte are Hybrid-SORT's: they need --tracker hybridsort")
    if a.tracker == "deep_ocsort":
        for flag, on in (("--with-reid", a.with_reid), ("--with-pose", a.with_pose), ("--ocsort-use-byte", a.ocsort_use_byte)):
            if on:
                p.error(f"{flag} is not available with --tracker deep_ocsort (its appearance branch is its own and it has no BYTE stage, docs/DEEPOCSORT.md)")
        if a.reid_model != "osnet":
            p.error("--reid-model auto is BoT-SORT's: --tracker deep_ocsort reads OSNet features")
    if a.ocsort_use_byte and a.tracker != "ocsort":
        p.error("--ocsort-use-byte is OC-SORT's BYTE stage: it needs --tracker ocsort")
    if a.camera_motion and a.tracker == "bytetrack":
        p.error("--camera-motion needs --tracker strongsort or botsort (ByteTrack has no GMC)")
    if a.gmc_method != "ecc" and not a.camera_motion:
        p.error("--gmc-method is a camera-motion estimator: it needs --camera-motion")
    if a.gmc_method != "ecc" and a.tracker not in ("botsort", "deep_ocsort"):
        p.error("--gmc-method sparseOptFlow is BoT-SORT's GMC: it needs --tracker botsort")
    if a.with_reid and a.tracker != "botsort":
        p.error("--with-reid is BoT-SORT's ReID branch: it needs --tracker botsort")
    if a.with_pose and a.tracker != "botsort":
        p.error("--with-pose is BoT-SORT's keypoint term: it needs --tracker botsort")
    if a.with_pose and a.with_reid:
        p.error("--with-pose and --with-reid cannot be combined")
    if a.with_pose and "pose" not in os.path.basename(a.weights):
        p.error("--with-pose needs a pose model (--weights ...-pose.pt): this detector has no keypoint columns")
    if a.reid_model != "osnet" and not a.with_reid:
        p.error("--reid-model is a model for BoT-SORT's ReID branch: it needs --with-reid")
    if a.reid_model == "auto" and a.reid_weights:
        p.error("--reid-model auto reads the detector's own features: --reid-weights does not apply")
    if a.device_entropy and not a.device_decode:
        p.error("--device-entropy is a stage of the device JPEG decoder: it needs --device-decode")
    if a.device_decode:
        if not a.track or a.batch <= 1:
            p.error("--device-decode feeds the grouped tracking path: it needs --track and --batch > 1")
        for src in a.source:
            why = encoded_source_error(src)
            if why:
                p.error(why)
    if a.device_encode_entropy and not a.device_encode:
        p.error("--device-encode-entropy is a stage of the device JPEG encoder: it needs --device-encode")
    if a.device_encode:
        if not a.save:
            p.error("--device-encode encodes the annotated output: it needs --save")
        if FrameSink.encoded_kind(a.save) is None:
            p.error(f"--device-encode: --save '{a.save}' must be a .mjpeg / .mjpg file or a directory (a path ending in '/' or an existing directory)")
        if not 1 <= a.save_quality <= 100:
            p.error("--save-quality must be 1 .. 100")
    jobs = [{"source": s, "track": a.track, "count": a.count, "weights": a.weights, "reid_weights": a.reid_weights, "limit": a.limit, "device": i, "random_init": a.random_init, "batch": a.batch, "reid_f16": a.reid_f16, "fp32": a.fp32, "device_masks": a.device_masks, "tracker": a.tracker, "camera_motion": a.camera_motion, "with_reid": a.with_reid, "reid_model": a.reid_model, "with_pose": a.with_pose, "gmc_method": a.gmc_method, "ocsort_use_byte": a.ocsort_use_byte, "hybrid_asso": a.hybrid_asso, "hybrid_no_byte": a.hybrid_no_byte, "device_decode": a.device_decode, "device_entropy": a.device_entropy,
             "device_encode": a.device_encode, "device_encode_entropy": a.device_encode_entropy, "save_quality": a.save_quality, "save_subsampling": a.save_subsampling,
             "gsi": a.gsi, "gsi_interval": a.gsi_interval, "gsi_tau": a.gsi_tau, "eval_gt": a.eval_gt[i] if a.eval_gt else None, "eval_thr": a.eval_thr, "eval_identity": a.eval_identity,
             "eval_det_gt": a.eval_det_gt[i] if a.eval_det_gt else None, "eval_det_max_dets": a.eval_det_max_dets, "eval_det_classes": a.eval_det_classes,
             "aflink": a.aflink, "aflink_thr_t": tuple(a.aflink_thr_t), "aflink_thr_s": a.aflink_thr_s, "aflink_thr_p": a.aflink_thr_p,
             "lines": a.line, "zones": a.zone, "zone_anchor": a.zone_anchor, "zone_gap": a.zone_gap, "heatmap": a.heatmap, "heat_cell": a.heat_cell, "heat_alpha": a.heat_alpha,
             "slice": a.slice, "slice_overlap": a.slice_overlap, "slice_merge": a.slice_merge, "slice_metric": a.slice_metric, "slice_thr": a.slice_thr, "no_slice_full": a.no_slice_full,
             "redact": a.redact, "redact_region": a.redact_region, "redact_strength": a.redact_strength, "redact_classes": a.redact_classes, "redact_pad": a.redact_pad,
             "redact_color": a.redact_color, "mtmc": a.mtmc, "save": _save_path(a, i)}
            for i, s in enumerate(a.source)]
    import torch
    ngpu = max(torch.cuda.device_count(), 1)
    for j in jobs:
        j["device"] %= ngpu                          # stream i -> GPU i mod N (the reference pins device 0, :41)
    if len(jobs) == 1:
        out = [process_video(jobs[0])]
    else:
        import torch.multiprocessing as mp
        with mp.get_context("spawn").Pool(processes=len(jobs)) as pool:      # :353-354
            out = pool.map(process_video, jobs)
        if a.mtmc:
            # the workers have exited: one more process opens the device, links the tables and leaves
            from .engine import TrackerEngine
            eng = TrackerEngine(n_streams=1, device=0)
            try:
                s = mtmc_post(a.source, "output", eng, a.mtmc_thr, a.mtmc_min_rows)
            finally:
                eng.close()
            out.append({"mtmc": {k: s[k] for k in ("cameras", "tracklets", "clusters")}})
    for o in out:
        print(o)
    return out


if __name__ == "__main__":
    main()
