"""`YOLO(weights)` — the model object the reference script drives.

Mirrors exactly what /root/reference/yolo_multi_model.py touches:
  :17     model = YOLO("yolo11n-pose.pt")
  :18-21  model.overrides['conf'|'iou'|'agnostic_nms'|'max_det'] (+ optional 'classes' :22)
  :23     model.names
  :41     model.track(image, verbose=False, device=0, persist=True, tracker="botsort.yaml") -> [Results]
  :173    model.predict(image, verbose=False, device=0)                                       -> [Results]
and the Results duck type consumed at :45-169 / :175-237 (boxes.id/.conf/.cls/.xyxy as 1-row tensors
per box, keypoints[i].xy, masks[i].xy, names).  The frame -> rows path runs on the MI355X
(pipeline.FramePipeline); this file is host glue only.
"""
from __future__ import annotations

import os
from typing import List, Optional

import numpy as np
import torch

from .config import DetectConfig, StrongSortConfig, byte_config, ocsort_config, deep_ocsort_config, hybridsort_config, check_reid_model, check_gmc_method

COCO_NAMES = ("person bicycle car motorcycle airplane bus train truck boat traffic_light fire_hydrant stop_sign "
              "parking_meter bench bird cat dog horse sheep cow elephant bear zebra giraffe backpack umbrella handbag tie "
              "suitcase frisbee skis snowboard sports_ball kite baseball_bat baseball_glove skateboard surfboard "
              "tennis_racket bottle wine_glass cup fork knife spoon bowl banana apple sandwich orange broccoli carrot "
              "hot_dog pizza donut cake chair couch potted_plant bed dining_table toilet tv laptop mouse remote keyboard "
              "cell_phone microwave oven toaster sink refrigerator book clock vase scissors teddy_bear hair_drier "
              "toothbrush").split()


def _row(i, n):
    """An int index as a one-row slice (negative indices count from the end, as on a tensor); anything else unchanged."""
    if isinstance(i, (int, np.integer)):
        i = int(i)
        if not -n <= i < n:
            raise IndexError(f"index {i} out of range for {n} rows")
        i %= n
        return slice(i, i + 1)
    return i


class Boxes:
    """Rows of [x1,y1,x2,y2,(id),conf,cls]; iterating yields 1-row Boxes (yolo_multi_model.py:73,126)."""

    def __init__(self, xyxy, conf, cls, ids=None):
        self.xyxy, self.conf, self.cls, self.id = xyxy, conf, cls, ids

    def __len__(self):
        return self.xyxy.shape[0]

    def __getitem__(self, i):
        i = _row(i, len(self))
        return Boxes(self.xyxy[i], self.conf[i], self.cls[i], None if self.id is None else self.id[i])

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    @property
    def is_track(self):
        return self.id is not None


# DOTA v1's 15 classes in the order of Ultralytics' DOTAv1.yaml (the -obb models), spelt with underscores like COCO_NAMES
DOTA_NAMES = ("plane ship storage_tank baseball_diamond tennis_court basketball_court ground_track_field harbor bridge large_vehicle "
              "small_vehicle helicopter roundabout soccer_ball_field swimming_pool").split()


class OBB:
    """Oriented boxes (docs/OBB.md): `xywhr` [n,5] = cx, cy, w, h, theta in original-image pixels (w >= h, theta in [0, pi)), `xyxy` [n,4]
    the axis-aligned envelope, `conf`, `cls`, `id` (None unless tracked).  `OBB.from_rows` reads the rows ss_nms_obb_batch writes.
    Length, indexing and iteration as Boxes."""

    def __init__(self, xywhr, xyxy, conf, cls, ids=None):
        self.xywhr, self.xyxy, self.conf, self.cls, self.id = xywhr, xyxy, conf, cls, ids

    @classmethod
    def from_rows(cls, rows, ids=None):
        """rows [n, >= 11] = x1, y1, x2, y2, conf, cls, cx, cy, w, h, theta (TrackerEngine.nms_obb_batch, the first `count` rows of an image)"""
        rows = torch.as_tensor(rows)
        if rows.dim() != 2 or rows.shape[1] < 11:
            raise ValueError("OBB.from_rows: rows [n, 11] = x1, y1, x2, y2, conf, cls, cx, cy, w, h, theta")
        return cls(rows[:, 6:11], rows[:, :4], rows[:, 4], rows[:, 5], ids)

    @property
    def xyxyxyxy(self):
        """[n,4,2]: the corners ctr + v1 + v2, ctr + v1 - v2, ctr - v1 - v2, ctr - v1 + v2 with v1 = (w/2)(cos, sin), v2 = (h/2)(-sin, cos)"""
        ctr, w, h, t = self.xywhr[:, :2], self.xywhr[:, 2:3], self.xywhr[:, 3:4], self.xywhr[:, 4:5]
        cos, sin = torch.cos(t), torch.sin(t)
        v1, v2 = torch.cat((w / 2 * cos, w / 2 * sin), 1), torch.cat((-h / 2 * sin, h / 2 * cos), 1)
        return torch.stack((ctr + v1 + v2, ctr + v1 - v2, ctr - v1 - v2, ctr - v1 + v2), 1)

    def __len__(self):
        return self.xywhr.shape[0]

    def __getitem__(self, i):
        i = _row(i, len(self))
        return OBB(self.xywhr[i], self.xyxy[i], self.conf[i], self.cls[i], None if self.id is None else self.id[i])

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    @property
    def is_track(self):
        return self.id is not None


class Keypoints:
    def __init__(self, data):                    # [n,17,3]
        self.data = data
        self.xy = data[..., :2]
        self.conf = data[..., 2]

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, i):
        return Keypoints(self.data[_row(i, len(self))])

    def __iter__(self):
        return (self[i] for i in range(len(self)))


def assemble_masks(proto, coef, boxes_in, in_hw):
    """Instance masks at the network-input resolution from a frame's prototypes [nm, mh, mw], the kept rows' coefficients [n, nm]
    and their DETECTION boxes in input pixels [n, 4] (the published Ultralytics recipe `process_mask(..., upsample=True)`: linear
    combination, cropped to the box on the prototype grid, bilinear up to the input size, > 0).  Host arithmetic in float32:
    the device hands over prototypes and coefficients, nothing of this is on the timed path.  -> bool [n, ih, iw]"""
    import torch.nn.functional as F
    c, mh, mw = proto.shape
    ih, iw = in_hw
    n = coef.shape[0]
    if n == 0:
        return torch.zeros(0, ih, iw, dtype=torch.bool)
    m = (coef.float() @ proto.float().reshape(c, -1)).view(n, mh, mw)
    b = boxes_in.float().clone()
    b[:, [0, 2]] *= mw / iw
    b[:, [1, 3]] *= mh / ih
    x1, y1, x2, y2 = (b[:, i].view(n, 1, 1) for i in range(4))
    col = torch.arange(mw, dtype=torch.float32).view(1, 1, mw)
    row = torch.arange(mh, dtype=torch.float32).view(1, mh, 1)
    m = m * ((col >= x1) & (col < x2) & (row >= y1) & (row < y2))
    return F.interpolate(m[None], (ih, iw), mode="bilinear", align_corners=False)[0] > 0.0


_RING = ((-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1), (0, 1), (-1, 1))      # (dx, dy) clockwise from west, y down


def trace_outline(comp: np.ndarray) -> np.ndarray:
    """Outer boundary of ONE 8-connected component (bool [h, w]) by Moore-neighbour tracing, clockwise from its first pixel in
    raster order, runs of equal chain direction reduced to their end points (what cv2.CHAIN_APPROX_SIMPLE keeps).  cv2 is not
    installed and its border-following order is not restated: the polygon is the same closed pixel chain, the start point
    and orientation are this function's.  -> int32 [k, 2] (x, y)"""
    h, w = comp.shape
    ys, xs = np.nonzero(comp)
    if len(ys) == 0:
        return np.zeros((0, 2), np.int32)
    sx, sy = int(xs[0]), int(ys[0])                       # np.nonzero is row-major: top-most row, left-most pixel
    inside = lambda x, y: 0 <= x < w and 0 <= y < h and comp[y, x]
    pts, x, y, back = [(sx, sy)], sx, sy, 0               # back: ring index of a background neighbour (west of the start pixel)
    first = None
    for _ in range(4 * (h * w + 4)):
        nxt = None
        for k in range(1, 9):
            j = (back + k) % 8
            qx, qy = x + _RING[j][0], y + _RING[j][1]
            if inside(qx, qy):
                bx, by = x + _RING[(j - 1) % 8][0], y + _RING[(j - 1) % 8][1]      # the background pixel scanned just before
                nxt = (qx, qy, _RING.index((bx - qx, by - qy)))
                break
        if nxt is None:                                   # an isolated pixel
            break
        if (x, y) == (sx, sy) and first is not None and nxt[:2] == first:          # back at the start, leaving as the first time
            pts.pop()
            break
        if first is None:
            first = nxt[:2]
        x, y, back = nxt
        pts.append((x, y))
    p = np.asarray(pts, np.int32)
    if len(p) < 3:
        return p
    d_in, d_out = p - np.roll(p, 1, 0), np.roll(p, -1, 0) - p
    return p[(d_in != d_out).any(1)]


def mask_polygon(mask: np.ndarray) -> np.ndarray:
    """The polygon Ultralytics' `masks2segments(strategy="largest")` stands for: the outline with the most points among the
    mask's 8-connected components (the 16 largest are traced).  -> float32 [k, 2] in the mask's pixel coordinates."""
    from scipy import ndimage
    lab, n = ndimage.label(mask, structure=np.ones((3, 3), np.int8))
    if n == 0:
        return np.zeros((0, 2), np.float32)
    order = np.argsort(-np.bincount(lab.ravel(), minlength=n + 1)[1:], kind="stable")[:16] + 1
    best = max((trace_outline(lab == int(i)) for i in order), key=len)
    return best.astype(np.float32)


def unpack_masks(bits: np.ndarray, iw: int) -> torch.Tensor:
    """Bit-packed masks uint32 / int32 [n, ih, ceil(iw/32)] (bit x % 32 of word x / 32 = pixel (y, x), csrc/ss_mask.hip) -> bool [n, ih, iw]."""
    b = np.ascontiguousarray(bits).view(np.uint8)
    return torch.from_numpy(np.unpackbits(b, axis=-1, bitorder="little")[..., :iw].astype(bool))


class Masks:
    """Instance masks of one frame: the part of Ultralytics' `Masks` the reference touches (/root/reference/yolo_multi_model.py
    :71-72 iterates them in step with the boxes, :112-121 draws `masks.xy`).  `data`: bool [n, ih, iw] at the network-input size,
    `xy`: one float32 [k, 2] polygon per mask in ORIGINAL-image pixels, `xyn`: the same normalised.  Assembled lazily on the host
    from the frame's prototypes and the kept rows' coefficients (`assemble_masks`) — or, from a YOLO(device_masks=True), unpacked
    from the device's bit-packed masks (`_bits`) with the device's polygons in mask pixels (`_polys`; None for a mask whose
    polygon was longer than the device's capacity: traced on the host)."""

    def __init__(self, proto, coef, boxes_in, in_hw, orig_shape, gain, pad_xy, _data=None, _bits=None, _polys=None):
        self._proto, self._coef, self._boxes, self._in_hw = proto, coef, boxes_in, tuple(int(v) for v in in_hw)
        self.orig_shape, self._gain, self._pad = tuple(int(v) for v in orig_shape[:2]), float(gain), (float(pad_xy[0]), float(pad_xy[1]))
        self._data, self._xy = _data, None
        self._bits, self._polys = _bits, _polys

    @property
    def data(self):
        if self._data is None:
            if self._bits is not None:
                self._data = unpack_masks(self._bits, self._in_hw[1])
            else:
                self._data = assemble_masks(self._proto, self._coef, self._boxes, self._in_hw)
        return self._data

    def _scale(self, p):
        H, W = self.orig_shape
        if len(p):
            p = (p - np.float32(self._pad)) / np.float32(self._gain)       # scale_coords: un-pad, un-scale, clip
            p[:, 0], p[:, 1] = p[:, 0].clip(0, W), p[:, 1].clip(0, H)
        return p.astype(np.float32)

    @property
    def xy(self):
        if self._xy is None:
            if self._polys is not None:
                self._xy = [self._scale(mask_polygon(self.data[i].numpy()) if p is None else p) for i, p in enumerate(self._polys)]
            else:
                self._xy = [self._scale(mask_polygon(m)) for m in self.data.numpy()]
        return self._xy

    @property
    def xyn(self):
        H, W = self.orig_shape
        return [p / np.float32((W, H)) for p in self.xy]

    def __len__(self):
        return self._coef.shape[0]

    def __getitem__(self, i):
        i = _row(i, len(self))
        sel = np.arange(len(self))[i.numpy() if isinstance(i, torch.Tensor) else i]
        return Masks(self._proto, self._coef[i], self._boxes[i], self._in_hw, self.orig_shape, self._gain, self._pad,
                     None if self._data is None else self._data[i], None if self._bits is None else self._bits[sel],
                     None if self._polys is None else [self._polys[k] for k in sel])

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class Results:
    def __init__(self, orig_img, names, boxes: Optional[Boxes], keypoints: Optional[Keypoints] = None, masks: Optional[Masks] = None,
                 obb: Optional[OBB] = None):
        self.orig_img, self.names, self.boxes, self.keypoints, self.masks = orig_img, names, boxes, keypoints, masks
        self.obb = obb                   # an oriented-box result: boxes is then None, as upstream
        self.orig_img_device = None      # track_stream(keep_device_frames=True): the frame as a device tensor uint8 [H,W,3] (for Overlay.draw_resident)

    def __len__(self):
        if self.boxes is None:
            return 0 if self.obb is None else len(self.obb)
        return len(self.boxes)


class _HostResults:
    """The pinned host side of F frames' results: counts, detection rows and (n_track_rows > 0) track rows in ONE pinned buffer
    `res` — laid out as csrc ss_pack_results writes one frame: [2, F] counts (detections, tracks; int32 bits), dets [F, R, ld],
    rows [F, n_track_rows, 8] — the prototypes or, from a YOLO(device_masks=True), the mask buffers, with keep_frames a device copy
    of the frames, and the event after which a group handed over on a side stream may be read (`done`).  It lives on the model
    (or in track_stream's ring) and refers to the pipeline, never the other way round: a pipeline that is dropped must be freed
    at once, not by a later garbage collection (which may run inside a graph capture)."""

    def __init__(self, model, pipe, b, F, n_track_rows=0, keep_frames=False):
        self.pipe = pipe
        R, ld = b.dets.shape[1:]
        nd, no = F * R * ld, F * n_track_rows * 8
        self.res = torch.zeros(2 * F + nd + no).pin_memory()
        self.cnt = self.res[:2 * F].view(torch.int32).view(2, F)
        self.dets = self.res[2 * F:2 * F + nd].view(F, R, ld)
        self.rows = self.res[2 * F + nd:].view(F, n_track_rows, 8) if n_track_rows else None
        dmask = pipe.nm and model.device_masks
        self.proto = torch.empty((F,) + tuple(b.proto.shape[1:]), dtype=b.proto.dtype).pin_memory() if pipe.nm and not dmask else None
        self.masks = model._mask_host(pipe, F, R) if dmask else None          # in place of proto
        self.frames = torch.empty((F,) + tuple(b.frames.shape[1:]), dtype=torch.uint8, device=pipe.dev) if keep_frames else None
        self.rbox = torch.zeros(F, n_track_rows, 5).pin_memory() if pipe.ne and n_track_rows else None       # OBB: the track rows' xywh theta
        self.done = torch.cuda.Event()

    def fetch(self, model, b, nv=1, outs=None, nouts=None, packed=False, rbox=None):
        """Enqueue, on the current stream, the hand-over of buffer set b's first nv frames and their track rows outs [nv, 256, 8] /
        counts nouts [nv] (None: detection only).  packed (one frame): counts and rows in one launch (ss_pack_results)."""
        pipe = self.pipe
        if packed:
            pipe.eng.pack_results(b.ndets, b.dets[0], nouts, None if outs is None else outs[0], self.res)
        else:
            if outs is not None:
                self.rows[:nv].copy_(outs, non_blocking=True)
                self.cnt[1, :nv].copy_(nouts, non_blocking=True)
            self.cnt[0, :nv].copy_(b.ndets[:nv], non_blocking=True)
            self.dets[:nv].copy_(b.dets[:nv], non_blocking=True)
        if rbox is not None and outs is not None:
            self.rbox[:nv].copy_(rbox, non_blocking=True)
        if self.masks is not None:
            model._mask_launch(pipe, b.proto[:nv], b.dets[:nv], b.ndets[:nv], self.masks)
        elif self.proto is not None:
            self.proto[:nv].copy_(b.proto[:nv], non_blocking=True)
        if self.frames is not None:
            self.frames[:nv].copy_(b.frames[:nv], non_blocking=True)          # the set's frames, before the set is refilled

    def results(self, model, f, image, track):
        """Frame f as [Results], once the stream (or `done`) is synchronised."""
        n, m = int(self.cnt[0, f]), int(self.cnt[1, f])
        model._warn_if_capped(self.pipe, n, track)
        res = model._results(image, self.pipe, self.dets[f, :n].clone(), self.rows[f, :m].clone() if track else None,
                             None if self.proto is None else self.proto[f].clone(), model._mask_rows(self.masks, f, n),
                             rbox=self.rbox[f, :m].clone() if track and self.rbox is not None else None)
        if self.frames is not None:
            res[0].orig_img_device = self.frames[f]
        return res


class YOLO:
    """`model = YOLO("yolo11n-pose.pt")` (yolo_multi_model.py:17).  `.track(frame)` / `.predict(frame)` replay HIP graphs
    captured once per (frame shape, overrides): the frame goes through a pinned host buffer, every stage runs on the
    device, the results come back through pinned buffers and there is ONE stream synchronisation per call.
    `.track_stream(frames, batch=16)` is the throughput form for sources that can supply frames ahead (files): groups
    of `batch` frames through the two-stream pipeline, same rows.

    Changing `.overrides` (or the frame size) re-captures the graphs and restarts the tracker, as a new
    `model.track(..., persist=False)` would."""

    def __init__(self, weights: str = "yolov8n.pt", seed: int = 0, random_init_ok: bool = False, reid_batch: int = 128,
                 camera_motion: bool = False, reid_weights: Optional[str] = None, reid_fp32: bool = True, half: bool = True,
                 device_masks: bool = False, tracker_type: str = "strongsort", with_reid: bool = False, reid_model: str = "osnet",
                 with_pose: bool = False, gmc_method: str = "ecc", ocsort_use_byte: bool = False, slice_hw=None, slice_overlap=0.2,
                 slice_full: bool = True, slice_merge: str = "nmm", slice_metric: str = "ios", slice_thr: float = 0.5,
                 track_bank: bool = False, hybrid_asso: str = "hmiou", hybrid_use_byte: bool = True):
        """reid_fp32 (default since round 6): ReID crops + OSNet-x0.25 in fp32 on the fp32 kernels — appearance distances within 1e-4 of a CPU fp32
        network, which f16 activations miss by 330x (reid_fp32=False: the f16 throughput mode, ~1.2x the per-frame rate, 1.7x the stream rate).
        half=False: the DETECTOR in fp32 as well (the reference's own precision: it passes no half=, yolo_multi_model.py:41) on the
        fp32 convolution kernels (csrc/ss_ops32.hip k32_conv) — NMS keep lists then equal the CPU fp32 network's; implies reid_fp32.
        device_masks (segmentation models): every call also assembles the kept rows' masks and traces their polygons on the device
        (csrc/ss_mask.hip) and downloads bits and points instead of the prototypes; `Results.masks` then needs no host arithmetic
        beyond unpacking and scale_coords.  Default False: masks are built on the host when first read (assemble_masks / mask_polygon).
        tracker_type: "strongsort" (default: OSNet appearance + NSA Kalman), or the BYTE family on the device (docs/BYTETRACK.md) —
        "bytetrack" (xyah Kalman) / "botsort" (xywh Kalman, no ReID): IoU and scores only, no ReID network or weights;
        track() then runs NMS at conf 0.1 unless track(conf=...) says otherwise (Ultralytics' Model.track), predict() keeps
        overrides['conf'].
        camera_motion: ECC camera-motion warps estimated on the device beside the detector (N4). StrongSORT moves its track
        boxes by them (D-18); "botsort" applies them as BoT-SORT's GMC to every track's Kalman mean and covariance
        (docs/BYTETRACK.md §1b) in track() and track_stream(). "bytetrack" has no GMC: a ValueError.
        gmc_method (camera_motion with "botsort" only, else a ValueError): "ecc" (default, as above) or "sparseOptFlow" — the
        estimator Ultralytics' botsort.yaml names: corners on the half-size grey frame, pyramidal Lucas-Kanade, a RANSAC similarity
        fit, all on the device (docs/BYTETRACK.md §1f); frame sides >= 64.
        with_reid ("botsort" only, else a ValueError): BoT-SORT's ReID branch (docs/BYTETRACK.md §1c) — OSNet-x0.25 features of
        every tracked row (reid_weights, reid_fp32 and half as for StrongSORT) add an appearance term to the IoU association.
        reid_model (with_reid only): "osnet" (default, as above) or "auto" — Ultralytics' `model: auto` (docs/BYTETRACK.md §1d): the
        rows' features are read from the detector's own head inputs, so the detector weights are the only file; no OSNet, no
        crops, no reid_weights (a ValueError), and reid_fp32 does not apply (the features follow `half`).
        with_pose ("botsort" on a pose model only, not with with_reid, else a ValueError): the keypoint term (docs/BYTETRACK.md §1e) —
        the rows' own keypoints add an OKS entry to the IoU association; no second network.
        tracker_type "ocsort": OC-SORT on the device (docs/OCSORT.md) — a 7-state SORT filter with observation-centric re-update,
        momentum and recovery; motion only, so no ReID network or weights, NMS at conf 0.1 in track() as for the BYTE family, and
        camera_motion, with_reid and with_pose are ValueErrors.  ocsort_use_byte ("ocsort" only): its BYTE stage on the rows between
        0.1 and 0.25.
        tracker_type "deep_ocsort": Deep OC-SORT on the device (docs/DEEPOCSORT.md) — OC-SORT without the BYTE stage, with OSNet-x0.25
        features of every tracked row (reid_weights, reid_fp32 and half as for StrongSORT) in an adaptively weighted appearance cost,
        a feature EMA that follows the detection score, and, with camera_motion, the warps (gmc_method "ecc" or "sparseOptFlow")
        applied to filters and observations.  with_reid, with_pose, ocsort_use_byte and reid_model="auto" are ValueErrors.
        tracker_type "hybridsort": Hybrid-SORT on the device (docs/HYBRIDSORT.md) — OC-SORT's machinery with the detection confidence as a
        Kalman state and a cost term, the height-modulated IoU (hybrid_asso "hmiou", or "iou") and the direction term over the four box
        corners; its BYTE stage is on unless hybrid_use_byte=False.  Motion only, as "ocsort": camera_motion, with_reid, with_pose,
        reid_model="auto", ocsort_use_byte and track_bank are ValueErrors.
        slice_hw (sh, sw): sliced inference (SAHI; docs/SLICE.md) — the detector runs on overlapping sh x sw tiles of the frame as one
        batch (slice_overlap: one ratio or (oh, ow); slice_full: the whole frame as one more tile) and the tiles' rows are merged on the
        device (slice_merge "nmm" = GREEDYNMM or "nms", slice_metric "ios" or "iou", slice_thr); predict, track and track_stream then
        see small objects at the tiles' scale.  The detector costs T times as much.  Segmentation models and reid_model="auto" are
        ValueErrors, as are more than 64 tiles; the slice must fit the frame (checked when the first frame arrives).
        track_bank: track() and track_stream() also keep, on the device, one pooled OSNet descriptor per track id (docs/MTMC.md): the
        table `model.track_bank()` returns and `mtmc.link` links across cameras.  It needs a tracker that reads OSNet features
        ("strongsort", "deep_ocsort", or "botsort" with with_reid and reid_model "osnet"); anything else is a ValueError.  Default
        False: nothing changes."""
        self.slice = None
        if slice_hw is not None:
            from .slicing import SliceConfig
            self.slice = SliceConfig(slice_hw, slice_overlap, slice_full, slice_merge, slice_metric, slice_thr)
            if "seg" in os.path.basename(weights):
                raise ValueError("sliced inference cannot run a segmentation model: a row's mask coefficients belong to its tile's prototypes")
            if reid_model == "auto":
                raise ValueError("sliced inference cannot feed reid_model='auto': the detector's anchor indices are per tile")
        hybridsort_config(tracker_type, hybrid_asso, hybrid_use_byte, camera_motion, with_reid, with_pose, ocsort_use_byte)
        deep_ocsort_config(tracker_type, with_reid, with_pose, ocsort_use_byte)               # ValueError on anything else
        ocsort_config(tracker_type, ocsort_use_byte, camera_motion, with_reid, with_pose)      # ValueError on anything else
        byte_config(tracker_type, with_reid, with_pose)
        check_reid_model(reid_model, with_reid, reid_weights)
        self.reid_model = reid_model
        self.tracker_type = tracker_type
        self.with_reid = bool(with_reid)
        self.with_pose = bool(with_pose)
        self._byte = tracker_type != "strongsort"
        from .nets import OBB_DETECTORS
        self._obb = os.path.basename(weights).lower().replace(".pt", "") in OBB_DETECTORS
        if self._obb:                             # docs/OBB.md §5: what is not built for rotated boxes is refused by name
            if tracker_type in ("ocsort", "deep_ocsort", "hybridsort"):
                raise ValueError(f"{weights!r} is an oriented-box model: tracker_type {tracker_type!r} associates on axis-aligned boxes; use "
                                 "'bytetrack' or 'botsort' (ProbIoU of the rotated boxes)")
            for on, what in ((with_reid, "with_reid"), (reid_model == "auto", "reid_model='auto'"), (with_pose, "with_pose"),
                             (camera_motion, "camera_motion"), (slice_hw is not None, "slice_hw"), (device_masks, "device_masks")):
                if on:
                    raise ValueError(f"{weights!r} is an oriented-box model: {what} is not built for rotated boxes (docs/OBB.md §5)")
        if tracker_type == "bytetrack" and camera_motion:
            raise ValueError("camera_motion needs tracker_type 'strongsort' or 'botsort' (ByteTrack has no GMC, G-05)")
        self.gmc_method = check_gmc_method(gmc_method, camera_motion, tracker_type)
        self._conf_track = None                   # BYTE: the NMS threshold of the tracking pipelines (set while track / track_stream build)
        self.weights = weights
        self.reid_weights = reid_weights          # OSNet-x0.25 state_dict; same policy as the detector's (raise unless random init is asked for)
        self.random_init_ok = random_init_ok
        self.arch = os.path.basename(weights).replace(".pt", "")
        self.overrides = {"conf": 0.25, "iou": 0.7, "agnostic_nms": False, "max_det": 300}
        self.seed = seed
        self.reid_batch = reid_batch
        pose = "pose" in self.arch
        if self.with_pose and not pose:
            raise ValueError(f"with_pose needs a pose model (keypoint columns): {weights!r} has none")
        self.names = {0: "person"} if pose else dict(enumerate(DOTA_NAMES if self._obb else COCO_NAMES))
        self._host = {}                 # slot name -> the _HostResults of a per-frame pipeline
        self._pipe = None               # the cached pipelines (each with its .key): track() / predict(),
        self._stream_pipe = None        # track_stream(),
        self._pred_pipe = None          # and the detection-only one for predict() when max_det exceeds the tracker's 128 rows
        self._cap_warned = self._tracker_warned = False           # warnings said once
        # test / bench hooks (synthetic head tensors, no weights exist offline): extra pipeline keywords and a callable
        # fill(buffers, virtual_stream, frame_index) that writes pred_in / anchor_gt / gt_feats before a frame runs
        self._pipe_kw = {"cmc": True} if camera_motion else {}    # N4: ECC camera-motion compensation (off by default)
        if gmc_method != "ecc":
            self._pipe_kw["gmc_method"] = gmc_method
        if reid_fp32 or not half:                                  # OSNet in fp32 (pipeline.FramePipeline reid_half): float distances within 1e-4
            self._pipe_kw["reid_half"] = False
        if not half:
            self._pipe_kw["half"] = False
        if self._byte:
            self._pipe_kw["tracker"] = tracker_type
            if self.with_reid:
                self._pipe_kw["with_reid"] = True
                if reid_model != "osnet":
                    self._pipe_kw["reid_model"] = reid_model
            if self.with_pose:
                self._pipe_kw["with_pose"] = True
            if ocsort_use_byte:
                self._pipe_kw["ocsort_use_byte"] = True
            if tracker_type == "hybridsort":
                if hybrid_asso != "hmiou":
                    self._pipe_kw["hybrid_asso"] = hybrid_asso
                if not hybrid_use_byte:
                    self._pipe_kw["hybrid_use_byte"] = False
        if self.slice is not None:
            self._pipe_kw["slice_cfg"] = self.slice
        self._track_bank, self._bank_pipe = bool(track_bank), None
        if self._track_bank:
            from .mtmc import bank_refusal
            why = bank_refusal(tracker_type, with_reid, reid_model, self._obb)
            if why:
                raise ValueError(f"track_bank=True: {why}")
            self._pipe_kw["track_bank"] = True
        self.device_masks = bool(device_masks)
        self._fill = None
        self._frame_index = 0

    def _dcfg(self):
        o = self.overrides
        conf = o["conf"] if self._conf_track is None else self._conf_track
        return DetectConfig(conf=float(conf), iou=float(o["iou"]), agnostic_nms=bool(o["agnostic_nms"]),
                            max_det=int(o["max_det"]))

    def _state_key(self, shape, device):
        cl = self.overrides.get("classes")
        cl = None if cl is None else tuple(int(c) for c in (cl if isinstance(cl, (list, tuple)) else [cl]))
        return (tuple(shape), int(device or 0), self._dcfg(), cl, None if self.slice is None else self.slice.key())

    def _build(self, cls, shape, device, need_reid=True, **kw):
        from . import nets
        args = dict(reid_batch=self.reid_batch, cfg=StrongSortConfig(), dcfg=self._dcfg(), det_source="detector",
                    feat_source="reid", seed=self.seed)
        args.update(self._pipe_kw)
        args.update(kw)
        pipe = cls(self.arch, 1, shape, device=int(device or 0), **args)
        # the networks' weights, before the first forward (the fused weight-prep caches are built from the loaded tensors).
        # The ReID weights are needed only once the TRACKER consumes OSNet embeddings: model.predict (yolo_multi_model.py:173)
        # works with detector weights alone; the first model.track on such a pipeline rebuilds it with the ReID weights.
        nets.load_weights(pipe.detector, self.weights, f"detector {self.arch}", self.random_init_ok)
        pipe.reid_loaded = pipe.reid is None and pipe.det_rows == 128        # BYTE: nothing to load, the pipeline tracks as built
        if need_reid and pipe.reid is not None and pipe.feat_source == "reid" and pipe.det_rows == 128:
            nets.load_weights(pipe.reid, self.reid_weights, "OSNet-x0.25 ReID", self.random_init_ok)
            pipe.reid_loaded = True
        pipe.eng.nms_set_classes(self.overrides.get("classes"))
        return pipe

    def _cached(self, slot, cls, shape, device, key=(), stale=None, **kw):
        """The pipeline in `slot` (_pipe / _pred_pipe / _stream_pipe) for this frame shape, device and overrides (+ key): the one
        built for them, else the old one closed and a new one built -> (pipeline, whether it is new)."""
        key = self._state_key(shape, device) + key
        pipe = getattr(self, slot)
        if pipe is not None and pipe.key == key and not (stale and stale(pipe)):
            return pipe, False
        if pipe is not None:
            pipe.close()
        pipe = self._build(cls, shape, device, **kw)
        pipe.key = key
        setattr(self, slot, pipe)
        return pipe, True

    # ---- per-frame path -------------------------------------------------------------------------------------
    def _run(self, image, device, track):
        """One frame through a cached FramePipeline: upload, step, results through pinned memory, ONE synchronisation.
        model.predict with max_det > 128 (the reference sets 1000, yolo_multi_model.py:21) has a detection-only pipeline whose NMS
        keeps up to 1024 rows (`_pred_pipe`); the tracking pipeline (128 detections per frame) is not involved.  BYTE models' predict()
        uses it too (its NMS threshold is overrides['conf'], the tracking pipeline's is track's), so that predict calls between track
        calls do not restart the tracker."""
        from .pipeline import FramePipeline
        from .jpeg import EncodedFrame
        if isinstance(image, EncodedFrame):
            raise TypeError("track() / predict() take decoded frames (BGR uint8 arrays): pass EncodedFrames to track_stream(), "
                            "or decode them first with strongsort_yolo_amd.jpeg.decode()")
        if track and self._obb and not self._byte:
            raise ValueError(f"{self.weights!r} is an oriented-box model: tracker_type 'strongsort' associates on axis-aligned boxes; build the "
                             "model with tracker_type 'bytetrack' or 'botsort' (ProbIoU of the rotated boxes)")
        wide = not track and (int(self.overrides["max_det"]) > 128 or self._byte or self._obb)
        slot = "_pred_pipe" if wide else "_pipe"
        if wide:
            pipe, new = self._cached(slot, FramePipeline, image.shape[:2], device, graph="split", detect_only_rows=1024)
        else:
            pipe, new = self._cached(slot, FramePipeline, image.shape[:2], device, graph="split", need_reid=track,
                                     stale=lambda p: track and not p.reid_loaded and p.feat_source == "reid")
        if new:
            # the tracking pipeline: one pinned buffer the device writes the frame's counts, detection rows and track rows into (csrc
            # ss_pack_results), the host reads it after the call's one synchronisation, no copies in between; the wide one: two copies
            self._host[slot] = _HostResults(self, pipe, pipe, 1, 0 if wide else pipe.out.shape[1])
            if not wide:
                self._frame_index = 0
        pipe.eng.upload(pipe.frames[0], image)
        if self._fill is not None:
            self._fill(pipe, 0, self._frame_index)
        pipe.step(track=track)
        if track:
            self._bank_pipe = pipe
        h = self._host[slot]
        h.fetch(self, pipe, 1, pipe.out if track else None, pipe.nout if track else None, packed=not wide,
                rbox=pipe.byte.rbox if track and pipe.ne else None)
        torch.cuda.current_stream(pipe.dev).synchronize()            # the one synchronisation of the call
        pipe.eng.check_errors()
        if not wide:
            self._frame_index += 1
        return h.results(self, 0, image, track)

    def _warn_if_capped(self, pipe, n_kept, track):
        """The tracking pipeline carries at most pipe.max_det (<= 128, <= reid_batch) detections per frame, highest scores first;
        the reference's max_det = 1000 (yolo_multi_model.py:21) applies to its tracker too.  A frame that fills the cap may have
        lost lower-scored detections: say so once (capacity errors elsewhere are loud; this truncation used to be silent)."""
        if track and n_kept >= pipe.max_det and pipe.max_det < int(self.overrides["max_det"]) and not self._cap_warned:
            import warnings
            self._cap_warned = True
            warnings.warn(f"a frame filled the tracker's per-frame limit of {pipe.max_det} detections (overrides['max_det'] = "
                          f"{self.overrides['max_det']}): lower-scored detections beyond it are not tracked "
                          f"(limit = min(max_det, 128, reid_batch = {self.reid_batch}))", RuntimeWarning, stacklevel=4)

    # ---- device masks (device_masks=True) ---------------------------------------------------------------------
    MASK_CAP = 2048            # points per device polygon; a longer one is traced on the host (instance masks on the device)
    MASK_SLOTS = 256           # label planes of the outline kernel's scratch = its workgroups (one per CU)

    def _mask_host(self, pipe, F, R):
        """Pinned host buffers the mask kernels write the kept rows' bits, polygons and lengths into (one frame group), and the
        pipeline's device buffers (packed masks, outline scratch: allocated once per pipeline, MASK_SLOTS label planes)."""
        ih, iw = pipe.geom.out_h, pipe.geom.out_w
        wpr = (iw + 31) // 32
        dev = getattr(pipe, "_mask_dev", None)
        if dev is None or dev["bits"].shape[0] < F or dev["bits"].shape[1] < R:
            dev = pipe._mask_dev = {"bits": torch.empty(F, R, ih, wpr, dtype=torch.int32, device=pipe.dev),
                                    "scratch": torch.empty(self.MASK_SLOTS * ih * iw, dtype=torch.int32, device=pipe.dev)}
        return {"bits": torch.empty(F, R, ih, wpr, dtype=torch.int32).pin_memory(),
                "pts": torch.empty(F, R, self.MASK_CAP, 2, dtype=torch.int32).pin_memory(),
                "npts": torch.empty(F, R, dtype=torch.int32).pin_memory(), "dev": dev, "iw": iw}

    def _mask_launch(self, pipe, proto, dets, ndets, h):
        """Both mask kernels on the current stream for the frames of `dets` [F, R, ld]: packed masks into the pipeline's device
        buffer, then outlines, the outline kernel copying every kept plane into the pinned `h['bits']`."""
        F, R = dets.shape[:2]
        d = h["dev"]
        bits = d["bits"][:F, :R] if d["bits"].shape[:2] != (F, R) else d["bits"]
        pipe.eng.mask_assemble(proto, dets, ndets, pipe.geom_dev[:F], 6 + pipe.nk, bits)
        pipe.eng.mask_outline(bits, ndets, h["iw"], h["pts"][:F], h["npts"][:F], d["scratch"], bits_copy=h["bits"][:F])

    @staticmethod
    def _mask_rows(h, f, n):
        """Frame f's first n device masks from the pinned buffers (after the synchronisation): (bits copy, polygons)."""
        if h is None:
            return None
        npts = h["npts"][f, :n].numpy()
        pts = h["pts"][f].numpy()
        polys = [pts[r, :k].astype(np.float32) if k >= 0 else None for r, k in enumerate(npts.tolist())]
        return h["bits"][f, :n].numpy().copy(), polys

    def _results(self, image, pipe, dets, rows, proto=None, dm=None, rbox=None):
        kpts = masks = None
        if getattr(pipe, "ne", 0):                      # oriented boxes: Results.obb, boxes None as upstream
            if rows is None:
                return [Results(image, self.names, None, obb=OBB.from_rows(dets))]
            sel = rows[:, 7] >= 0
            rows, rbox = rows[sel], rbox[sel]
            return [Results(image, self.names, None, obb=OBB(rbox, rows[:, :4], rows[:, 6], rows[:, 5], rows[:, 4]))]
        if pipe.nk:
            k = dets[:, 6:6 + pipe.nk].reshape(dets.shape[0], pipe.nk // 3, 3).clone()
            k[..., 0] = (k[..., 0] - pipe.pad_x) / pipe.gain
            k[..., 1] = (k[..., 1] - pipe.pad_y) / pipe.gain
            kpts = k
        if pipe.nm and (proto is not None or dm is not None):
            # masks are cut with the DETECTION boxes (as upstream: assembled at predict time, before the tracker replaces the boxes),
            # brought back to the network-input frame: x * gain + pad
            b = dets[:, :4].clone()
            b[:, [0, 2]] = b[:, [0, 2]] * pipe.gain + pipe.pad_x
            b[:, [1, 3]] = b[:, [1, 3]] * pipe.gain + pipe.pad_y
            masks = Masks(proto, dets[:, 6 + pipe.nk:6 + pipe.nk + pipe.nm].clone(), b, (pipe.geom.out_h, pipe.geom.out_w),
                          image.shape, pipe.gain, (pipe.pad_x, pipe.pad_y), _bits=None if dm is None else dm[0],
                          _polys=None if dm is None else dm[1])
        if rows is None:
            return [Results(image, self.names, Boxes(dets[:, :4], dets[:, 4], dets[:, 5]),
                            None if kpts is None else Keypoints(kpts), masks)]
        rows = rows[rows[:, 7] >= 0]                   # ultralytics semantics: results[i] = results[i][det_idx]
        if rows.shape[0] == 0:
            return [Results(image, self.names, Boxes(torch.zeros(0, 4), torch.zeros(0), torch.zeros(0), None))]
        di = rows[:, 7].long()
        return [Results(image, self.names, Boxes(rows[:, :4], rows[:, 6], rows[:, 5], rows[:, 4]),
                        None if kpts is None else Keypoints(kpts[di]), None if masks is None else masks[di])]

    TRACKERS = ("strongsort.yaml", "strongsort", "botsort.yaml", "bytetrack.yaml", "ocsort.yaml", "deep_ocsort.yaml", "hybridsort.yaml")

    def _check_tracker(self, tracker):
        """`tracker=`: the tracker is chosen when the model is built (`tracker_type`), StrongSORT by default (BASELINE north_star).
        The reference passes "botsort.yaml" (yolo_multi_model.py:41) — the Ultralytics tracker configurations are accepted and
        answered by the model's tracker, once with a warning that says so; any other value is an error instead of being ignored."""
        name = os.path.basename(str(tracker))
        if name not in self.TRACKERS:
            raise ValueError(f"tracker={tracker!r}: this library tracks with StrongSORT only (accepted: {', '.join(self.TRACKERS)})")
        if self._byte:
            family = name.split(".")[0]
            if family != self.tracker_type and not self._tracker_warned:
                import warnings
                self._tracker_warned = True
                warnings.warn(f"tracker={tracker!r}: this model was built with tracker_type={self.tracker_type!r}, which rules; "
                              f"its parameters are strongsort_yolo_amd.config.{ {'ocsort': 'OCSortConfig', 'deep_ocsort': 'DeepOCSortConfig', 'hybridsort': 'HybridSortConfig'}.get(self.tracker_type, 'ByteTrackConfig') }",
                              RuntimeWarning, stacklevel=3)
            return
        if not name.startswith("strongsort") and not self._tracker_warned:
            import warnings
            self._tracker_warned = True
            warnings.warn(f"tracker={tracker!r} is an Ultralytics configuration; tracking runs StrongSORT (OSNet-x0.25 appearance + NSA Kalman), "
                          f"its parameters are strongsort_yolo_amd.config.StrongSortConfig", RuntimeWarning, stacklevel=3)

    @torch.no_grad()
    def track(self, image, verbose=False, device=0, persist=True, tracker="strongsort.yaml", **kw) -> List[Results]:
        self._check_tracker(tracker)
        if not persist and self._pipe is not None:
            self._pipe.reset_tracker(-1)
        if self._byte:                            # Ultralytics' Model.track: conf = kwargs.get("conf") or 0.1
            self._conf_track = float(kw.get("conf") or 0.1)
            try:
                return self._run(image, device, True)
            finally:
                self._conf_track = None
        return self._run(image, device, True)

    @torch.no_grad()
    def predict(self, image, verbose=False, device=0, **kw) -> List[Results]:
        return self._run(image, device, False)

    __call__ = predict

    # ---- throughput path ------------------------------------------------------------------------------------
    @torch.no_grad()
    def track_stream(self, frames, batch: int = 16, device=0, keep_device_frames: bool = False, conf: Optional[float] = None,
                     jpeg_entropy: str = "host"):
        """Generator over `frames` (BGR uint8 arrays of one size, or jpeg.EncodedFrames of one size: baseline JPEGs decoded on the
        device, `Results.orig_img` is then the EncodedFrame): yields the same [Results] `track(frame)` would, in
        order, `batch` frames at a time through the overlapped two-stream pipeline (stateless stages of group k+1 run
        while the tracker consumes group k; the tracker reads its galleries once per group).
        keep_device_frames: every Results also carries `orig_img_device`, the frame as a device tensor (a device-to-device copy
        of the group's input buffer taken on the tracker's stream), so that an annotated output needs no second upload
        (`Overlay.draw_resident`); valid until the generator has yielded `ring` more groups.
        conf (BYTE models): the NMS threshold, as track(conf=...) (default 0.1).
        jpeg_entropy (EncodedFrames): "host" (default) decodes the Huffman code on host threads, "device" on the device (docs/JPEG.md §12)."""
        if jpeg_entropy not in ("host", "device"):
            raise ValueError(f"track_stream: jpeg_entropy {jpeg_entropy!r} (\"host\" or \"device\")")
        from .pipeline import OverlappedPipeline
        from .jpeg import EncodedFrame
        it = iter(frames)
        first = next(it, None)
        if first is None:
            return
        encoded = isinstance(first, EncodedFrame)

        def take():
            """the next frame; an encoded stream holds EncodedFrames of the first one's shape only"""
            nxt = next(it, None)
            if encoded and nxt is not None:
                if not isinstance(nxt, EncodedFrame):
                    raise TypeError("track_stream: the first frame is an EncodedFrame, so every frame must be one")
                if nxt.shape != first.shape:
                    raise ValueError(f"track_stream: EncodedFrame of shape {nxt.shape} in a stream of {first.shape}")
            return nxt
        if self._obb and not self._byte:
            raise ValueError(f"{self.weights!r} is an oriented-box model: tracker_type 'strongsort' associates on axis-aligned boxes; build the "
                             "model with tracker_type 'bytetrack' or 'botsort' (ProbIoU of the rotated boxes)")
        self._conf_track = float(conf or 0.1) if self._byte else None
        try:
            pipe, _ = self._cached("_stream_pipe", OverlappedPipeline, first.shape[:2], device, key=(batch,), graph="front", frame_batch=batch,
                                   reid_split=(5 if self.arch == "yolov8n" else 2) if batch > 1 else None, defer_track=batch > 1)     # stage cut: bench.REID_SPLIT's sweep
        finally:
            self._conf_track = None
        self._bank_pipe = pipe
        pipe.on_result = None
        pipe.flush()                                                      # groups an abandoned generator left in flight: tracked, results dropped
        F = batch
        # result slots: groups in flight (<= 3) + margin
        ring = [_HostResults(self, pipe, pipe.bufs[0], F, pipe.outs.shape[2], keep_device_frames) for _ in range(5)]
        pending = []                                                      # (group index, frames of the group)
        state = {"group": 0, "first": {}, "enqueued": -1}                 # first frame index of a group -> group index

        def on_result(frame_idx, f):                                      # runs while a tracker call is being enqueued
            g = state["first"].get(frame_idx - f)
            if g is None:                                                 # a group left over from an abandoned generator
                return
            b, nv = pipe.cur_bufs, pipe.cur_valid                         # the set this tracker call read (the pipeline's own index, not g)
            if f != nv - 1:
                return
            h = ring[g % len(ring)]
            h.fetch(self, b, nv, pipe.outs[:nv, 0], pipe.nouts[:nv, 0], rbox=pipe.rboxs[:nv, 0] if pipe.ne else None)
            h.done.record(torch.cuda.current_stream(pipe.dev))
            state["enqueued"] = g
            del state["first"][frame_idx - f]

        pipe.on_result = on_result

        def finish(g, imgs):
            h = ring[g % len(ring)]
            h.done.synchronize()
            for f, img in enumerate(imgs):
                yield h.results(self, f, img, True)

        try:
            chunk = [first]
            while chunk:
                while len(chunk) < F:
                    nxt = take()
                    if nxt is None:
                        break
                    chunk.append(nxt)
                g = state["group"]
                b = pipe.begin_frame()                                    # waits until this buffer set's last group left the tracker
                with torch.cuda.stream(pipe.s_in):
                    if encoded:                                           # Huffman decoding on host threads, the rest on the device (jpeg.py)
                        pipe.eng.jpeg_decode_batch(b.frames, chunk, pipe.s_in, entropy=jpeg_entropy)
                    else:
                        pipe.eng.upload_batch(b.frames, chunk, pipe.s_in)  # the group's frames: staged by several host threads, one copy
                    if self._fill is not None:
                        for f in range(len(chunk)):
                            self._fill(b, f, self._frame_index + f)
                self._frame_index += len(chunk)
                state["first"][pipe.frames_in] = g                       # submit() numbers the group's frames from here
                pipe.submit(len(chunk))
                pending.append((g, chunk))
                state["group"] = g + 1
                while pending and pending[0][0] <= state["enqueued"] - 1:  # its results are enqueued, and so is a group after it
                    yield from finish(*pending.pop(0))
                nxt = take()
                chunk = [nxt] if nxt is not None else []
            pipe.flush()
            while pending:
                yield from finish(*pending.pop(0))
            pipe.eng.check_errors()
        finally:
            pipe.on_result = None

    def track_bank(self, stream: int = 0):
        """The track bank's table of the pipeline that tracked last (track_bank=True): ids, n, first, last, cls int32 [m] in rising id
        order and desc float32 [m, 512] (docs/MTMC.md).  Synchronous."""
        if not self._track_bank:
            raise RuntimeError("track_bank(): build the model with track_bank=True")
        pipe = self._bank_pipe
        if pipe is None or pipe.bank is None:
            raise RuntimeError("track_bank(): run track() or track_stream() once first (the bank lives in the tracking pipeline)")
        torch.cuda.synchronize(pipe.dev)
        return pipe.bank.table(stream)

    def overlay(self):
        """Annotation overlay bound to this model's device context (drawing of yolo_multi_model.py:58-162 as a kernel)."""
        from .overlay import Overlay
        pipe = self._stream_pipe or self._pipe
        if pipe is None:
            raise RuntimeError("overlay(): run track()/predict()/track_stream() once first (the device context is created there)")
        return Overlay(self.names, pipe.eng)

    def close(self):
        for p in (self._pipe, self._stream_pipe, self._pred_pipe):
            if p is not None:
                p.close()
        self._pipe = self._stream_pipe = self._pred_pipe = self._bank_pipe = None
        self._host = {}
