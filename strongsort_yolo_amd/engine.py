"""Host-side handle on the gfx950 StrongSORT library: one context = S device-resident streams.

torch is used for device memory and streams only; every arithmetic step of the hot path runs in
libstrongsort_hip.so (csrc/).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import sys as _sys
from dataclasses import dataclass

import numpy as np
import torch

from . import lib as _lib
from .config import StrongSortConfig, DetectConfig, ByteTrackConfig, OCSortConfig, DeepOCSortConfig, HybridSortConfig
from .lib import MAX_TRACKS, MAX_DETS, FEAT_DIM, OUT_COLS


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@dataclass
class LetterboxGeom:
    out_h: int
    out_w: int
    new_h: int
    new_w: int
    pad_top: int
    pad_left: int
    gain: float


def letterbox_geometry(h: int, w: int, imgsz: int = 640, stride: int = 32, auto: bool = True) -> LetterboxGeom:
    """Ultralytics LetterBox geometry (host integers; DECISIONS D-14).  Stands behind the
    preprocessing inside model.track / model.predict (yolo_multi_model.py:41, :173)."""
    r = min(imgsz / h, imgsz / w)
    new_w, new_h = int(round(w * r)), int(round(h * r))
    dw, dh = imgsz - new_w, imgsz - new_h
    if auto:
        dw, dh = dw % stride, dh % stride
    dw, dh = dw / 2, dh / 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return LetterboxGeom(new_h + top + bottom, new_w + left + right, new_h, new_w, top, left, r)


def scale_geometry(g: LetterboxGeom, h0: int, w0: int):
    """gain / pad used by scale_boxes to map letterboxed boxes back (Ultralytics scale_boxes)."""
    gain = min(g.out_h / h0, g.out_w / w0)
    pad_x = round((g.out_w - w0 * gain) / 2 - 0.1)
    pad_y = round((g.out_h - h0 * gain) / 2 - 0.1)
    return float(gain), float(pad_x), float(pad_y)


class TrackerEngine:
    def __init__(self, cfg: StrongSortConfig | None = None, n_streams: int = 1, device: int = 0, debug: bool = False):
        if not torch.cuda.is_available():
            raise _lib.SSError(_lib.SS_ERR_HIP, "no HIP device visible: the StrongSORT hot path has no CPU fallback")
        self.cfg = cfg or StrongSortConfig()
        self.S = n_streams
        self.device = torch.device("cuda", device)
        self.L = _lib.load()
        self.ctx = C.c_void_p()
        c = _lib.make_config(self.cfg, n_streams, debug)
        _lib.check(None, self.L.ss_create(C.byref(c), device, C.byref(self.ctx)))
        self.debug_enabled = debug
        self._streams_keep = []                          # handles of create_stream(): destroyed with the context
        self._cmc_keep = self._assoc_ev_keep = None      # set_cmc / set_assoc_event: the library keeps their addresses
        self.use_current_stream()
        dev = self.device
        self.out = torch.zeros(n_streams, MAX_TRACKS, OUT_COLS, dtype=torch.float32, device=dev)
        self.nout = torch.zeros(n_streams, dtype=torch.int32, device=dev)

    def close(self):
        if getattr(self, "ctx", None) and self.ctx.value:
            torch.cuda.synchronize(self.device)          # nothing of ours may still be in flight on any stream
            for h in self._streams_keep:
                self.L.ss_stream_destroy(self.ctx, C.c_void_p(h))
            self._streams_keep = []
            self.L.ss_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:                                             # interpreter teardown: the HIP runtime may already be gone
            if _sys is None or _sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        _lib.check(self.ctx, rc)

    def _st(self, stream=None):
        """`stream` (torch.cuda.Stream), or the current torch stream, as the library takes it."""
        return C.c_void_p((torch.cuda.current_stream(self.device) if stream is None else stream).cuda_stream)

    def use_stream(self, stream=None):
        """The tracker's and the front end's launches go to `stream` (default: the current torch stream) from here on."""
        self._ck(self.L.ss_set_hip_stream(self.ctx, self._st(stream)))

    def use_current_stream(self):
        self.use_stream()

    def reset(self, stream: int = -1):
        self._ck(self.L.ss_reset(self.ctx, stream))

    def set_option(self, name: str, value: int):
        """cos_grid — see include/strongsort_hip.h."""
        self._ck(self.L.ss_set_option(self.ctx, name.encode(), int(value)))

    def check_errors(self):
        self._ck(self.L.ss_check_errors(self.ctx))

    def upload(self, dst: torch.Tensor, src: np.ndarray, stream=None):
        """Host array -> device tensor through the library's write-combined staging ring (asynchronous on `stream`,
        default the current torch stream).  `src` may be reused immediately."""
        src = np.ascontiguousarray(src)
        if src.nbytes != dst.numel() * dst.element_size() or not dst.is_contiguous():
            raise ValueError("upload: size / layout mismatch")
        self._ck(self.L.ss_upload(self.ctx, self._st(stream), _ptr(dst), src.ctypes.data_as(C.c_void_p), src.nbytes))

    def upload_batch(self, dst: torch.Tensor, srcs, stream=None, threads: int = 4):
        """len(srcs) host arrays of one size -> dst[0 .. len(srcs)) (device, contiguous) in ONE asynchronous copy: the arrays are staged
        by `threads` host threads in a write-combined area (a single thread staging 32 frames of 720p costs more than the GPU needs
        for them).  The arrays may be reused immediately."""
        n = len(srcs)
        if n == 0:
            return
        srcs = [np.ascontiguousarray(a) for a in srcs]
        each = srcs[0].nbytes
        if (any(a.nbytes != each or a.shape != srcs[0].shape for a in srcs) or not dst.is_contiguous() or dst[0].numel() * dst.element_size() != each
                or dst.shape[0] < n or tuple(dst.shape[1:]) != tuple(srcs[0].shape)):
            raise ValueError("upload_batch: size / shape / layout mismatch")
        arr = (C.c_void_p * n)(*[a.ctypes.data for a in srcs])
        self._ck(self.L.ss_upload_batch(self.ctx, self._st(stream), _ptr(dst), arr, n, each, int(threads)))

    def jpeg_decode_batch(self, dst: torch.Tensor, frames, stream=None, threads: int = 4, rgb: bool = False, entropy: str = "host"):
        """len(frames) (1 .. 64) jpeg.EncodedFrames of one size -> dst[0 .. len(frames)) (device uint8 [.., H, W, 3], every frame
        contiguous), BGR or RGB: Huffman decoding on `threads` host threads inside the call, then one asynchronous copy of the
        coefficients and two launches (csrc/ss_jpeg.hip).  The frames' bytes may be reused immediately.
        entropy="device": the host only parses the headers and copies the scans; Huffman decoding runs on the device too (docs/JPEG.md
        §12).  Same pixels; a scan that turns out damaged is reported by the next check_errors() or a later decode call."""
        if entropy not in ("host", "device"):
            raise ValueError(f"jpeg_decode_batch: entropy {entropy!r} (\"host\" or \"device\")")
        n = len(frames)
        if n == 0:
            return
        shape = tuple(frames[0].shape)
        if (any(tuple(f.shape) != shape for f in frames) or dst.dtype != torch.uint8 or dst.dim() != 4 or not dst[0].is_contiguous()
                or dst.shape[0] < n or tuple(dst.shape[1:]) != shape or (dst.shape[0] > 1 and dst.stride(0) < dst[0].numel())):
            raise ValueError("jpeg_decode_batch: size / shape / layout mismatch")
        data = (C.c_char_p * n)(*[f.data for f in frames])
        sizes = (C.c_size_t * n)(*[len(f.data) for f in frames])
        stride = dst.stride(0) if dst.shape[0] > 1 else dst[0].numel()
        call = self.L.ss_jpeg_decode_batch_device if entropy == "device" else self.L.ss_jpeg_decode_batch
        self._ck(call(self.ctx, self._st(stream), data, sizes, n, shape[0], shape[1], _ptr(dst), stride, int(bool(rgb)), int(threads)))

    def jpeg_encode_batch(self, src: torch.Tensor, quality: int = 85, subsampling: str = "4:2:0", stream=None, threads: int = 4, rgb: bool = False,
                          entropy: str = "host"):
        """src: device uint8 [n, H, W, 3] (n 1 .. 64, every frame contiguous) or [H, W, 3], BGR (rgb=True: RGB) -> n baseline JPEG
        files as bytes, equal to what Pillow writes at that quality and subsampling ("4:2:0" | "4:2:2" | "4:4:4"): colour
        conversion, downsampling, forward DCT, quantisation and compaction on the device (csrc/ss_jpeg_enc.hip), the sparse
        coefficients back in one copy, Huffman coding on `threads` host threads.  Returns when the files are written.
        entropy="device": Huffman coding and byte stuffing run on the device too (docs/JPEG.md §13); only the scans' own bytes come
        back and the host threads write the headers and copy.  The same files."""
        from .jpeg import SUBSAMPLING
        if entropy not in ("host", "device"):
            raise ValueError(f"jpeg_encode_batch: entropy {entropy!r} (\"host\" or \"device\")")
        if subsampling not in SUBSAMPLING:
            raise ValueError(f"jpeg_encode_batch: subsampling {subsampling!r} (one of {', '.join(SUBSAMPLING)})")
        hs, vs = SUBSAMPLING[subsampling]
        fr = src if src.dim() == 4 else src.unsqueeze(0)
        if (fr.dtype != torch.uint8 or fr.dim() != 4 or fr.shape[3] != 3 or fr.device != self.device or not fr[0].is_contiguous()
                or (fr.shape[0] > 1 and fr.stride(0) < fr[0].numel())):
            raise ValueError("jpeg_encode_batch: a uint8 [n, H, W, 3] tensor on the engine's device, every frame contiguous")
        n, H, W = (int(v) for v in fr.shape[:3])
        bound = int(self.L.ss_jpeg_encode_bound(W, H, hs, vs))
        if bound < 0:
            _lib.check(None, bound)                                       # (a host-only entry point: its message is the library's, not the context's)
        files = np.empty((max(n, 1), bound), np.uint8)                    # (untouched pages cost nothing: a file fills a small part of its bound)
        out = (C.c_void_p * max(n, 1))(*[files[i].ctypes.data for i in range(n)])
        cap = (C.c_size_t * max(n, 1))(*([bound] * n))
        size = (C.c_size_t * max(n, 1))()
        stride = fr.stride(0) if n > 1 else H * W * 3
        call = self.L.ss_jpeg_encode_batch_device if entropy == "device" else self.L.ss_jpeg_encode_batch
        self._ck(call(self.ctx, self._st(stream), _ptr(fr), stride, n, H, W, int(bool(rgb)), int(quality), hs, vs, int(threads), out, cap, size))
        return [files[i, :size[i]].tobytes() for i in range(n)]

    def download(self, dst: np.ndarray, src: torch.Tensor, stream=None):
        """Device tensor -> host array (synchronous)."""
        if dst.nbytes != src.numel() * src.element_size() or not src.is_contiguous() or not dst.flags["C_CONTIGUOUS"]:
            raise ValueError("download: size / layout mismatch")
        self._ck(self.L.ss_download(self.ctx, self._st(stream), dst.ctypes.data_as(C.c_void_p), _ptr(src), dst.nbytes))

    def gsi_smooth(self, offsets, frames, vals, len_scale, alpha: float = 1e-10):
        """GSI's Gaussian-process smoothing of finished tracks (csrc/ss_gsi.hip, docs/GSI.md), host arrays in and out: track t owns
        rows offsets[t] .. offsets[t+1]-1 of frames (int, strictly increasing inside a track) and vals [rows, 4] (x1, y1, w, h);
        len_scale [tracks] is each track's RBF length scale.  -> (out [rows, 4] float64, status [tracks] int32: 0 smoothed, 1 a pivot
        was not positive, 2 longer than ss_gsi_max_len(); the rows of 1 and 2 pass through).  Synchronous, on the engine's stream."""
        offsets = np.ascontiguousarray(offsets, np.int32)
        frames = np.ascontiguousarray(frames, np.int32)
        vals = np.ascontiguousarray(vals, np.float64)
        len_scale = np.ascontiguousarray(len_scale, np.float64)
        nt = len(offsets) - 1
        if offsets.ndim != 1 or nt < 0 or len_scale.shape != (nt,) or frames.ndim != 1 or vals.shape != (len(frames), 4) or (nt >= 0 and len(offsets) and offsets[-1] != len(frames)):
            raise ValueError("gsi_smooth: offsets [tracks + 1], frames [rows], vals [rows, 4], len_scale [tracks] with offsets[-1] == rows")
        out, status = np.empty((max(len(frames), 1), 4), np.float64), np.zeros(max(nt, 1), np.int32)
        pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
        self._ck(self.L.ss_gsi_smooth(self.ctx, nt, offsets.ctypes.data_as(pi), frames.ctypes.data_as(pi), vals.ctypes.data_as(pd),
                                      len_scale.ctypes.data_as(pd), float(alpha), out.ctypes.data_as(pd), status.ctypes.data_as(pi)))
        return out[:len(frames)], status[:nt]

    def aflink_set_weights(self, blob):
        """AFLink's network weights (csrc/ss_aflink.hip, docs/AFLINK.md §3): the float32 blob of aflink.pack, ss_aflink_weight_floats()
        long.  They stay on the device until the next call."""
        blob = np.ascontiguousarray(blob, np.float32)
        if blob.ndim != 1:
            raise ValueError("aflink_set_weights: a flat float32 blob")
        self._ck(self.L.ss_aflink_set_weights(self.ctx, blob.ctypes.data_as(C.POINTER(C.c_float)), len(blob)))

    def aflink_cost(self, offsets, feats, thr_t=(0, 30), thr_s: float = 75.0, want_inputs: bool = False):
        """AFLink's gate, input transform and network, host arrays in and out: tracklet t owns rows offsets[t] .. offsets[t+1]-1 of
        feats [rows, 3] (frame, x1, y1).  -> (pair_i, pair_j int32 [pairs], row-major; cost float64 [pairs]) and, with want_inputs,
        the normalised float32 inputs [pairs, 2, 30, 3].  The library counts the candidates first; the arrays are sized by its
        answer.  Synchronous, on the engine's stream."""
        offsets = np.ascontiguousarray(offsets, np.int32)
        feats = np.ascontiguousarray(feats, np.float64)
        n = len(offsets) - 1
        if offsets.ndim != 1 or n < 0 or feats.ndim != 2 or feats.shape[1] != 3 or (len(offsets) and offsets[-1] != len(feats)) or len(thr_t) != 2:
            raise ValueError("aflink_cost: offsets [tracklets + 1], feats [rows, 3] with offsets[-1] == rows, thr_t (t0, t1)")
        pi, pd, pf, pl = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_longlong)
        head = (self.ctx, n, offsets.ctypes.data_as(pi), feats.ctypes.data_as(pd), int(thr_t[0]), int(thr_t[1]), float(thr_s))
        count = C.c_longlong(0)
        self._ck(self.L.ss_aflink_cost(*head, 0, None, None, None, None, C.byref(count)))
        m = int(count.value)
        pair_i, pair_j, cost = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.float64)
        inputs = np.zeros((m, 2, 30, 3), np.float32) if want_inputs else None
        if m:
            self._ck(self.L.ss_aflink_cost(*head, m, pair_i.ctypes.data_as(pi), pair_j.ctypes.data_as(pi), cost.ctypes.data_as(pd),
                                           inputs.ctypes.data_as(pf) if want_inputs else None, C.byref(count)))
            if int(count.value) != m:
                raise _lib.SSError(_lib.SS_ERR_INVALID, f"aflink_cost: {m} candidates counted, {int(count.value)} written")
        return (pair_i, pair_j, cost, inputs) if want_inputs else (pair_i, pair_j, cost)

    def aflink_match(self, n_tracklets: int, pair_i, pair_j, cost, thr_p: float = 0.05):
        """AFLink's matching of the pairs with cost < thr_p (csrc/ss_aflink.hip: one wave per connected component) -> successor
        [n_tracklets] int32, the tracklet linked behind each or -1.  The costs are the caller's."""
        pair_i, pair_j = np.ascontiguousarray(pair_i, np.int32), np.ascontiguousarray(pair_j, np.int32)
        cost = np.ascontiguousarray(cost, np.float64)
        if pair_i.ndim != 1 or pair_j.shape != pair_i.shape or cost.shape != pair_i.shape:
            raise ValueError("aflink_match: pair_i, pair_j, cost [pairs]")
        succ = np.full(max(int(n_tracklets), 1), -1, np.int32)
        pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
        self._ck(self.L.ss_aflink_match(self.ctx, int(n_tracklets), len(pair_i), pair_i.ctypes.data_as(pi), pair_j.ctypes.data_as(pi),
                                        cost.ctypes.data_as(pd), float(thr_p), succ.ctypes.data_as(pi)))
        return succ[:max(int(n_tracklets), 0)]

    def mot_eval(self, frame_off, gt_off, tr_off, gt_ids, tr_ids, gt_boxes, tr_boxes, n_gt_ids, n_tr_ids, thr: float = 0.5, want_ga: bool = False):
        """HOTA's and CLEAR MOT's matching of ground-truth / tracker pairs (csrc/ss_mot.hip, docs/MOTEVAL.md), host arrays in and out:
        pair p owns frames frame_off[p] .. frame_off[p+1]-1, frame f the rows gt_off[f] .. gt_off[f+1]-1 of gt_ids (dense, per pair) and
        gt_boxes [rows, 4] (x1, y1, x2, y2) and likewise on the tracker side.  -> (hota_match, hota_s, clear_match, clear_s) per
        ground-truth row (a match is the tracker row's index within its frame, -1 none) and, with want_ga, the alignment scores of
        all pairs in one flat array.  Synchronous; one device call for all pairs."""
        n_pairs, k, n_gt_ids, n_tr_ids, ptrs, keep = self._mot_args("mot_eval", frame_off, gt_off, tr_off, gt_ids, tr_ids, gt_boxes, tr_boxes, n_gt_ids, n_tr_ids)
        n = max(k, 1)
        hm, cm, hs, cs = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n), np.zeros(n)
        ga = np.zeros(max(int((n_gt_ids.astype(np.int64) * n_tr_ids).sum()), 1)) if want_ga else None
        pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
        self._ck(self.L.ss_mot_eval(self.ctx, n_pairs, *ptrs, float(thr), hm.ctypes.data_as(pi), hs.ctypes.data_as(pd),
                                    cm.ctypes.data_as(pi), cs.ctypes.data_as(pd), ga.ctypes.data_as(pd) if want_ga else None))
        return (hm[:k], hs[:k], cm[:k], cs[:k]) + ((ga,) if want_ga else ())

    @staticmethod
    def _mot_args(who, frame_off, gt_off, tr_off, gt_ids, tr_ids, gt_boxes, tr_boxes, n_gt_ids, n_tr_ids):
        """The host arrays of mot_eval / mot_identity, checked for shape -> (pairs, ground-truth rows, id counts of both sides, the
        nine pointers in the C order, the arrays behind them)."""
        ai = lambda v: np.ascontiguousarray(v, np.int32).reshape(-1)
        frame_off, gt_off, tr_off, gt_ids, tr_ids, n_gt_ids, n_tr_ids = (ai(v) for v in (frame_off, gt_off, tr_off, gt_ids, tr_ids, n_gt_ids, n_tr_ids))
        gt_boxes, tr_boxes = (np.ascontiguousarray(v, np.float64).reshape(-1, 4) for v in (gt_boxes, tr_boxes))
        n_pairs = len(frame_off) - 1
        if (n_pairs < 1 or len(n_gt_ids) != n_pairs or len(n_tr_ids) != n_pairs or len(gt_off) != len(tr_off) or len(gt_off) != frame_off[-1] + 1
                or gt_off[-1] != len(gt_ids) or tr_off[-1] != len(tr_ids) or len(gt_boxes) != len(gt_ids) or len(tr_boxes) != len(tr_ids)):
            raise ValueError(f"{who}: frame_off [pairs + 1], gt_off / tr_off [frames + 1], ids [rows], boxes [rows, 4], id counts [pairs]")
        k = len(gt_ids)
        if not len(gt_ids):                                               # (a side without rows still passes a pointer)
            gt_ids, gt_boxes = np.zeros(1, np.int32), np.zeros((1, 4))
        if not len(tr_ids):
            tr_ids, tr_boxes = np.zeros(1, np.int32), np.zeros((1, 4))
        keep = (frame_off, gt_off, tr_off, gt_ids, tr_ids, gt_boxes, tr_boxes, n_gt_ids, n_tr_ids)
        pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
        return n_pairs, k, n_gt_ids, n_tr_ids, [v.ctypes.data_as(pd if v.dtype == np.float64 else pi) for v in keep], keep

    def mot_identity(self, frame_off, gt_off, tr_off, gt_ids, tr_ids, gt_boxes, tr_boxes, n_gt_ids, n_tr_ids, thr: float = 0.5, want_pot: bool = False):
        """The identity metrics' device half (csrc/ss_mot.hip, docs/MOTEVAL.md §1 "Identity"), the packing of mot_eval: -> (idtp [pairs]
        int32, the weight of a maximum-weight matching of each pair's ground-truth ids to its tracker ids under the counts pot;
        gt_to_tr [all ground-truth ids] int32, one such matching as dense tracker ids, -1 none) and, with want_pot, the counts of all
        pairs in one flat int32 array, per pair [n_gt_ids, n_tr_ids].  At most ss_mot_max_ids() ids a side of a pair.  Synchronous;
        one device call for all pairs."""
        n_pairs, _, n_gt_ids, n_tr_ids, ptrs, keep = self._mot_args("mot_identity", frame_off, gt_off, tr_off, gt_ids, tr_ids, gt_boxes, tr_boxes, n_gt_ids, n_tr_ids)
        cap = int(self.L.ss_mot_max_ids())                                # (a call over the cap is the library's to refuse: its outputs stay small)
        g, t = np.clip(n_gt_ids, 0, cap).astype(np.int64), np.clip(n_tr_ids, 0, cap).astype(np.int64)
        n_g = int(g.sum())
        idtp, match = np.zeros(n_pairs, np.int32), np.full(max(n_g, 1), -1, np.int32)
        pot = np.zeros(max(int((g * t).sum()), 1), np.int32) if want_pot else None
        pi = C.POINTER(C.c_int)
        self._ck(self.L.ss_mot_identity(self.ctx, n_pairs, *ptrs, float(thr), idtp.ctypes.data_as(pi), match.ctypes.data_as(pi),
                                        pot.ctypes.data_as(pi) if pot is not None else None))
        return (idtp, match[:n_g]) + ((pot,) if want_pot else ())

    def ap_eval(self, similarity, class_cell_off, cell_image, cell_gt_off, cell_det_off, gt_boxes, gt_crowd, det_boxes, det_scores, iou_thrs, rec_thrs,
                areas, max_dets, want_rank: bool = False, want_record: bool = False):
        """COCO's precision and recall arrays of detections against ground truth (csrc/ss_ap.hip, docs/DETEVAL.md), host arrays in and
        out.  similarity 0: boxes [rows, 4] by IoU, 1: [rows, 5] by ProbIoU; the cells come by (class, image) with their row ranges on
        both sides, rows in input order.  -> (precision [T,R,K,A,M], recall [T,K,A,M]), then with want_rank the place of every packed
        detection in its class's order, then with want_record match and ignored [A,T,kept] int32.  Synchronous; one device call."""
        ai = lambda v: np.ascontiguousarray(v, np.int32).reshape(-1)
        ad = lambda v: np.ascontiguousarray(v, np.float64).reshape(-1)
        width = 5 if int(similarity) else 4
        class_cell_off, cell_image, cell_gt_off, cell_det_off, gt_crowd, max_dets = (ai(v) for v in (class_cell_off, cell_image, cell_gt_off, cell_det_off, gt_crowd, max_dets))
        gt_boxes, det_boxes = (np.ascontiguousarray(v, np.float64).reshape(-1, width) for v in (gt_boxes, det_boxes))
        det_scores, iou_thrs, rec_thrs, areas = ad(det_scores), ad(iou_thrs), ad(rec_thrs), ad(areas)
        K, n_cells = len(class_cell_off) - 1, len(cell_image)
        if (K < 1 or len(cell_gt_off) != n_cells + 1 or len(cell_det_off) != n_cells + 1 or len(gt_boxes) != cell_gt_off[-1] or len(gt_crowd) != len(gt_boxes)
                or len(det_boxes) != cell_det_off[-1] or len(det_scores) != len(det_boxes) or len(areas) % 2 or not len(max_dets)):
            raise ValueError("ap_eval: class_cell_off [classes + 1], cell_image [cells], cell offsets [cells + 1], boxes [rows, 4 or 5], crowd flags and "
                             "scores [rows], areas [ranges, 2], max_dets [entries]")
        T, R, A, M, n_det = len(iou_thrs), len(rec_thrs), len(areas) // 2, len(max_dets), len(det_scores)
        kept = int(np.minimum(np.diff(cell_det_off.astype(np.int64)), max(int(max_dets[-1]), 0)).clip(0).sum())
        precision, recall = np.zeros((T, R, K, A, M)), np.zeros((T, K, A, M))
        rank = np.zeros(max(n_det, 1), np.int32) if want_rank else None
        n_rec = A * T * kept if A * T * kept <= 1 << 28 else 0                 # (a call over the cap is the library's to refuse: its outputs stay small)
        match, ignored = (np.full(max(n_rec, 1), -1, np.int32), np.zeros(max(n_rec, 1), np.int32)) if want_record else (None, None)
        if not len(gt_boxes):                                                   # (a side without rows still passes a pointer)
            gt_boxes, gt_crowd = np.zeros((1, width)), np.zeros(1, np.int32)
        if not n_det:
            det_boxes, det_scores = np.zeros((1, width)), np.zeros(1)
        if not n_cells:
            cell_image = np.zeros(1, np.int32)
        pi, pd = C.POINTER(C.c_int), C.POINTER(C.c_double)
        p = lambda v: None if v is None else v.ctypes.data_as(pd if v.dtype == np.float64 else pi)
        self._ck(self.L.ss_ap_eval(self.ctx, int(similarity), K, n_cells, p(class_cell_off), p(cell_image), p(cell_gt_off), p(cell_det_off), p(gt_boxes), p(gt_crowd),
                                   p(det_boxes), p(det_scores), T, p(iou_thrs), R, p(rec_thrs), A, p(areas), M, p(max_dets), p(precision), p(recall),
                                   p(rank), p(match), p(ignored)))
        out = (precision, recall)
        if want_rank:
            out += (rank[:n_det],)
        if want_record:
            out += (match[:n_rec].reshape(A, T, -1), ignored[:n_rec].reshape(A, T, -1))
        return out

    # ---- tracker --------------------------------------------------------------------------------
    # ---- analytics behind the trackers (csrc/ss_zone.hip, docs/ZONES.md); zones.ZoneCounter is the front of these ----
    def zone_create(self, cfg, lines, zones):
        """cfg: lib.ss_zone_config; lines [[ax, ay, bx, by], ...]; zones [[[x, y], ...], ...] in integer pixels.  One state per
        context, shared by its streams; a second call replaces it."""
        ln = np.ascontiguousarray(np.asarray(lines, np.int32).reshape(-1, 4))
        xy = np.ascontiguousarray(np.concatenate([np.asarray(z, np.int32).reshape(-1, 2) for z in zones], 0) if len(zones) else np.zeros((0, 2), np.int32))
        off = np.concatenate([[0], np.cumsum([len(z) for z in zones])]).astype(np.int32)
        pi = C.POINTER(C.c_int)
        self._ck(self.L.ss_zone_create(self.ctx, C.byref(cfg), ln.ctypes.data_as(pi), len(ln), xy.ctypes.data_as(pi), off.ctypes.data_as(pi), len(zones)))

    def zone_destroy(self):
        self._ck(self.L.ss_zone_destroy(self.ctx))

    def zone_reset(self, stream: int = -1):
        self._ck(self.L.ss_zone_reset(self.ctx, int(stream)))

    def zone_update_group(self, n_frames, rows, counts, events=None, inside=None, dwell=None, line_totals=None, occupancy=None, heat_frames=None,
                          heat_max=None):
        """One launch for n_frames (<= 32) frames of every stream: rows [F,S,256,8] f32 and counts [F,S] i32 as a tracker's
        update_group leaves them (device tensors, read in place); every output is a device tensor or None.  Asynchronous."""
        self._ck(self.L.ss_zone_update_group(self.ctx, int(n_frames), _ptr(rows), _ptr(counts), _ptr(events), _ptr(inside), _ptr(dwell), _ptr(line_totals),
                                             _ptr(occupancy), _ptr(heat_frames), _ptr(heat_max)))

    def zone_totals(self, stream: int, n_classes: int) -> dict:
        """Synchronous: the running totals of one stream (the keys of tests/zones_ref.py's totals())."""
        fr, hm = C.c_int(), C.c_int()
        lc, lt = np.zeros((16, 2, n_classes), np.int32), np.zeros((16, 2), np.int32)
        z = {k: np.zeros(16, np.int32) for k in ("entries", "exits", "longest", "peak")}
        ds = np.zeros(16, np.int64)
        pi = C.POINTER(C.c_int)
        self._ck(self.L.ss_zone_get_totals(self.ctx, int(stream), C.byref(fr), lc.ctypes.data_as(pi), lt.ctypes.data_as(pi), z["entries"].ctypes.data_as(pi),
                                           z["exits"].ctypes.data_as(pi), ds.ctypes.data_as(C.POINTER(C.c_longlong)), z["longest"].ctypes.data_as(pi),
                                           z["peak"].ctypes.data_as(pi), C.byref(hm)))
        return dict(z, frames=fr.value, heat_max=hm.value, line_class=lc, line_totals=lt, dwell_sum=ds)

    def zone_heat(self, stream: int = 0) -> np.ndarray:
        """Synchronous: the cumulative heat grid of one stream, int32 [gh, gw]."""
        gh, gw = C.c_int(), C.c_int()
        self._ck(self.L.ss_zone_get_heat(self.ctx, int(stream), None, 0, C.byref(gh), C.byref(gw)))
        g = np.zeros((gh.value, gw.value), np.int32)
        self._ck(self.L.ss_zone_get_heat(self.ctx, int(stream), g.ctypes.data_as(C.POINTER(C.c_int)), g.size, C.byref(gh), C.byref(gw)))
        return g

    def zone_heat_device(self, stream: int = 0):
        """-> (address of the stream's cumulative grid, address of its maximum) on the device."""
        a, b = C.c_void_p(), C.c_void_p()
        self._ck(self.L.ss_zone_heat_device(self.ctx, int(stream), C.byref(a), C.byref(b)))
        return a.value, b.value

    def zone_set_colormap(self, table):
        t = np.ascontiguousarray(table, np.uint8)
        if t.shape != (256, 3):
            raise ValueError("zone_set_colormap: a uint8 [256, 3] BGR table")
        self._ck(self.L.ss_zone_set_colormap(self.ctx, t.ctypes.data_as(C.POINTER(C.c_uint8))))

    def zone_heat_blend(self, frames: torch.Tensor, heat, heat_frame_stride: int, maxes, max_stride: int, alpha: int, stream=None):
        """frames uint8 [B,H,W,3] (or [H,W,3]) on the device, blended in place; heat / maxes: device tensors or addresses."""
        fr = frames if frames.dim() == 4 else frames.unsqueeze(0)
        addr = lambda t: C.c_void_p(t) if isinstance(t, int) else _ptr(t)
        self._ck(self.L.ss_zone_heat_blend(self.ctx, self._st(stream), _ptr(fr), fr.shape[0], fr.stride(0), fr.shape[1], fr.shape[2], fr.stride(1),
                                           addr(heat), int(heat_frame_stride), addr(maxes), int(max_stride), int(alpha)))
        return frames

    # ---- identities across cameras (csrc/ss_mtmc.hip, docs/MTMC.md); mtmc.TrackBank and mtmc.link are the front of these ----
    def bank_create(self, max_ids: int = 4096):
        """One descriptor table per stream of the context for the track ids 1..max_ids (4 KiB an id and stream); a second call
        replaces it."""
        self._ck(self.L.ss_bank_create(self.ctx, int(max_ids)))

    def bank_destroy(self):
        self._ck(self.L.ss_bank_destroy(self.ctx))

    def bank_reset(self, stream: int = -1):
        self._ck(self.L.ss_bank_reset(self.ctx, int(stream)))

    def bank_update_group(self, n_frames, rows, counts, feats):
        """One launch for n_frames (<= 32) frames of every stream: rows [F,S,256,8] f32 and counts [F,S] i32 as a tracker's
        update_group leaves them and feats [F,S,128,512] f32, the raw features that call read (device tensors, read in place).
        Asynchronous on the engine's stream, behind a detached tracker chain."""
        self._ck(self.L.ss_bank_update_group(self.ctx, int(n_frames), _ptr(rows), _ptr(counts), _ptr(feats)))

    def bank_get(self, stream: int = 0) -> dict:
        """Synchronous: the stream's table (the keys of tests/mtmc_ref.py's Bank.table()): ids, n, first, last, cls int32 [m] in
        rising id order and desc float32 [m, 512]."""
        pi = C.POINTER(C.c_int)
        m = C.c_int(0)
        self._ck(self.L.ss_bank_get(self.ctx, int(stream), 0, C.byref(m), None, None, None, None, None, None))
        k = m.value
        t = {name: np.zeros(max(k, 1), np.int32) for name in ("ids", "n", "first", "last", "cls")}
        desc = np.zeros((max(k, 1), FEAT_DIM), np.float32)
        if k:
            self._ck(self.L.ss_bank_get(self.ctx, int(stream), k, C.byref(m), *(t[name].ctypes.data_as(pi) for name in ("ids", "n", "first", "last", "cls")),
                                        desc.ctypes.data_as(C.POINTER(C.c_float))))
            if m.value != k:
                raise _lib.SSError(_lib.SS_ERR_INVALID, f"bank_get: {k} ids counted, {m.value} written")
        return dict({name: v[:k] for name, v in t.items()}, desc=desc[:k])

    def mtmc_link(self, desc, cam, first, last, n, thr: float, min_rows: int = 1, want_dist: bool = False):
        """Distances, constraints and constrained average-linkage clustering of T tracklets (host arrays: desc [T, 512] float32 unit
        rows; cam, first, last, n [T]) -> (global_id int32 [T], merges float64 [m, 3] = (a, b, height)) and, with want_dist, the
        float32 distances [T, T] (i < j; zero elsewhere).  Synchronous, on the engine's stream."""
        desc = np.ascontiguousarray(desc, np.float32)
        cam, first, last, n = (np.ascontiguousarray(v, np.int32).reshape(-1) for v in (cam, first, last, n))
        T = len(cam)
        if desc.shape != (T, FEAT_DIM) or len(first) != T or len(last) != T or len(n) != T:
            raise ValueError(f"mtmc_link: desc [T, {FEAT_DIM}], cam, first, last, n [T]")
        k = max(T, 1)
        gid, merges, nm = np.zeros(k, np.int32), np.zeros((k, 3), np.float64), C.c_int(0)
        dist = np.zeros((min(k, int(self.L.ss_mtmc_max_tracklets())),) * 2, np.float32) if want_dist else None
        pi = C.POINTER(C.c_int)
        self._ck(self.L.ss_mtmc_link(self.ctx, T, desc.ctypes.data_as(C.POINTER(C.c_float)), cam.ctypes.data_as(pi), first.ctypes.data_as(pi),
                                     last.ctypes.data_as(pi), n.ctypes.data_as(pi), float(thr), int(min_rows), gid.ctypes.data_as(pi),
                                     merges.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nm),
                                     dist.ctypes.data_as(C.POINTER(C.c_float)) if want_dist else None))
        out = (gid[:T], merges[:nm.value].copy())
        return out + (dist,) if want_dist else out

    def update_device(self, dets, ndets, feats, img_hw, out=None, nout=None):
        """All streams, one frame; tensors live on the device ([S,128,6] f32, [S] i32, [S,128,512] f32,
        [S,2] i32).  Asynchronous; returns (rows [S,256,8], counts [S]) device tensors (default: self.out, self.nout)."""
        out = self.out if out is None else out
        nout = self.nout if nout is None else nout
        self._ck(self.L.ss_track_update(self.ctx, _ptr(dets), _ptr(ndets), _ptr(feats), _ptr(img_hw), _ptr(out), _ptr(nout)))
        return out, nout

    @property
    def max_group_frames(self) -> int:
        return int(self.L.ss_max_group_frames())

    def update_group(self, n_frames, dets, ndets, feats, img_hw, out, nout):
        """A group of n_frames (<= max_group_frames) consecutive frames of all streams: tensors [F,S,128,6] f32, [F,S] i32,
        [F,S,128,512] f32, [S,2] i32 -> rows out [F,S,256,8], counts nout [F,S] (device tensors, asynchronous).
        Frames are associated in order; the galleries are read once for the whole group."""
        self._ck(self.L.ss_track_update_group(self.ctx, int(n_frames), _ptr(dets), _ptr(ndets), _ptr(feats), _ptr(img_hw),
                                              _ptr(out), _ptr(nout)))
        return out, nout

    def cmc_estimate(self, frames: torch.Tensor, n_frames: int, warps: torch.Tensor = None, stream=None, n_valid: torch.Tensor = None):
        """N4: ECC camera-motion warps of a group: frames uint8 [F*S,H,W,3] ([F][S] order) -> warps float64 [F,S,8]
        (2x3 matrix previous -> current frame, [6] = iterations or -1).  Asynchronous.  n_valid: device int32 [1], the real
        frames of a partial group (the rest of the buffer is stale)."""
        if warps is None:
            warps = torch.zeros(n_frames, self.S, 8, dtype=torch.float64, device=self.device)
        self._ck(self.L.ss_cmc_estimate(self.ctx, self._st(stream), _ptr(frames), int(n_frames), frames.stride(0),
                                        frames.shape[1], frames.shape[2], frames.stride(1), _ptr(n_valid), _ptr(warps)))
        return warps

    def cmc_small(self, frame: int, stream: int = 0) -> np.ndarray:
        """Synchronous: a 0.1x grey image of `stream` as cmc_estimate keeps it (ss_cmc_get_small), uint8 [hs, ws]: frame 0 is the
        remembered predecessor, frame 1..F are the frames of the last call."""
        hs, ws = C.c_int(0), C.c_int(0)
        self._ck(self.L.ss_cmc_get_small(self.ctx, int(frame), int(stream), None, 0, C.byref(hs), C.byref(ws)))
        out = np.zeros((hs.value, ws.value), np.uint8)
        self._ck(self.L.ss_cmc_get_small(self.ctx, int(frame), int(stream), out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size, None, None))
        return out

    def gmc_sparse_estimate(self, frames: torch.Tensor, n_frames: int, warps: torch.Tensor = None, stream=None, n_valid: torch.Tensor = None):
        """Sparse-optical-flow camera-motion warps of a group (docs/BYTETRACK.md §1f): cmc_estimate's arguments and layout;
        [6] = inliers or -1, [7] = tracked corners.  Frame sides >= 64."""
        if warps is None:
            warps = torch.zeros(n_frames, self.S, 8, dtype=torch.float64, device=self.device)
        self._gmc_hw = (int(frames.shape[1]), int(frames.shape[2]))
        self._ck(self.L.ss_gmc_sparse_estimate(self.ctx, self._st(stream), _ptr(frames), int(n_frames), frames.stride(0),
                                               frames.shape[1], frames.shape[2], frames.stride(1), _ptr(n_valid), _ptr(warps)))
        return warps

    def estimate_warps(self, method: str, *args, **kw):
        """cmc_estimate ("ecc") or gmc_sparse_estimate ("sparseOptFlow")."""
        return (self.gmc_sparse_estimate if method == "sparseOptFlow" else self.cmc_estimate)(*args, **kw)

    def gmc_sparse_stages(self, frame: int, stream: int = 0) -> dict:
        """Synchronous: the stages of pair (frame, stream) of the last gmc_sparse_estimate call (ss_gmc_sparse_get): the current
        image's pyramid (4 uint8 arrays), the previous image's corners [n,2] and candidate count, the tracked points [n,2],
        status [n] and inlier mask [n]."""
        g = self._gmc_hw
        sizes = [(g[0] // 2, g[1] // 2)]
        for _ in range(3):
            sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
        lv = [np.zeros(sz, np.uint8) for sz in sizes]
        cxy, pts = np.zeros((1000, 2), np.int32), np.zeros((1000, 2), np.float64)
        st, inl = np.zeros(1000, np.uint8), np.zeros(1000, np.uint8)
        n, nc = C.c_int(0), C.c_int(0)
        u8p, ip, dp = C.POINTER(C.c_uint8), C.POINTER(C.c_int), C.POINTER(C.c_double)
        self._ck(self.L.ss_gmc_sparse_get(self.ctx, int(frame), int(stream), *[a.ctypes.data_as(u8p) for a in lv], cxy.ctypes.data_as(ip),
                                          C.byref(n), C.byref(nc), pts.ctypes.data_as(dp), st.ctypes.data_as(u8p), inl.ctypes.data_as(u8p)))
        k = n.value
        return dict(pyramid=lv, corners=cxy[:k], n_candidates=nc.value, points=pts[:k], status=st[:k], inliers=inl[:k])

    def set_cmc(self, warps):
        """The following tracker calls compensate camera motion with these warps ([F,S,8] float64); None: off."""
        self._cmc_keep = warps
        self._ck(self.L.ss_track_set_cmc(self.ctx, _ptr(warps)))

    def set_assoc_event(self, event):
        """`event` (torch.cuda.Event, recorded at least once, or None) is recorded on the tracker's stream right after the
        association launch of every following update_group call."""
        self._assoc_ev_keep = event
        self._ck(self.L.ss_track_set_assoc_event(self.ctx, C.c_void_p(event.cuda_event if event is not None else 0)))

    def track_join(self, stream):
        """`stream` (torch.cuda.Stream) waits for the detached per-frame chain of the last update_group (option "chain_cus")."""
        self._ck(self.L.ss_track_join(self.ctx, self._st(stream)))

    def create_stream(self, skip_cus: int = 0):
        """A stream whose queue leaves the first `skip_cus` compute units of the CU mask alone (ss_stream_create) as a
        torch.cuda.ExternalStream; the handle lives as long as the engine."""
        h = C.c_void_p()
        self._ck(self.L.ss_stream_create(self.ctx, int(skip_cus), C.byref(h)))
        self._streams_keep.append(h.value)
        return torch.cuda.ExternalStream(h.value, device=self.device)

    def update_host(self, dets: np.ndarray, feats: np.ndarray, img_hw) -> np.ndarray:
        """Single-stream synchronous update with host arrays -> rows [M,8] float32."""
        dets = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 6)
        feats = np.ascontiguousarray(feats, dtype=np.float32).reshape(-1, FEAT_DIM)
        n = dets.shape[0]
        out = np.empty((MAX_TRACKS, OUT_COLS), dtype=np.float32)
        n_out = C.c_int(0)
        f32p = C.POINTER(C.c_float)
        self._ck(self.L.ss_track_update_host(
            self.ctx, 0, dets.ctypes.data_as(f32p), n, feats.ctypes.data_as(f32p), int(img_hw[0]), int(img_hw[1]),
            out.ctypes.data_as(f32p), MAX_TRACKS, C.byref(n_out)))
        return out[: n_out.value].copy()

    # ---- inspection -------------------------------------------------------------------------------
    def tracks(self, stream: int = 0) -> dict:
        T = MAX_TRACKS
        n, nid = C.c_int(), C.c_int()
        ints = {k: np.zeros(T, np.int32) for k in ("track_id", "state", "hits", "age", "tsu", "class_id", "gal_count")}
        conf = np.zeros(T, np.float32)
        mean, cov = np.zeros((T, 8)), np.zeros((T, 8, 8))
        smooth = np.zeros((T, FEAT_DIM), np.float32)
        ip, fp, dp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double)
        self._ck(self.L.ss_get_tracks(
            self.ctx, stream, T, C.byref(n), C.byref(nid), ints["track_id"].ctypes.data_as(ip),
            ints["state"].ctypes.data_as(ip), ints["hits"].ctypes.data_as(ip), ints["age"].ctypes.data_as(ip),
            ints["tsu"].ctypes.data_as(ip), ints["class_id"].ctypes.data_as(ip), conf.ctypes.data_as(fp),
            mean.ctypes.data_as(dp), cov.ctypes.data_as(dp), smooth.ctypes.data_as(fp),
            ints["gal_count"].ctypes.data_as(ip)))
        k = n.value
        d = {key: v[:k].copy() for key, v in ints.items()}
        d.update(conf=conf[:k].copy(), mean=mean[:k].copy(), cov=cov[:k].copy(), smooth=smooth[:k].copy(),
                 next_id=nid.value)
        return d

    def debug(self, stream: int = 0, frame: int = 0) -> dict:
        T, D = MAX_TRACKS, MAX_DETS
        counts = np.zeros(6, np.int32)
        cosd = np.zeros((T, D), np.float32)
        maha, cost_a, cost_b = np.zeros((T, D)), np.zeros((T, D)), np.zeros((T, D))
        gated = np.zeros((T, D), np.uint8)
        lists = np.zeros((4, T), np.int32)
        ip, fp, dp, up = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        self._ck(self.L.ss_get_debug(self.ctx, stream, frame, counts.ctypes.data_as(ip), cosd.ctypes.data_as(fp),
                                     maha.ctypes.data_as(dp), gated.ctypes.data_as(up), cost_a.ctypes.data_as(dp),
                                     cost_b.ctypes.data_as(dp), lists.ctypes.data_as(ip)))
        nC, nCand, nCols, nD, path_a, path_b = (int(v) for v in counts)
        return dict(n_conf=nC, n_cand=nCand, n_cols=nCols, n_dets=nD, path_a=path_a, path_b=path_b, cos=cosd[:nC, :nD], maha=maha[:nC, :nD],
                    gated=gated[:nC, :nD], cost_a=cost_a[:nC, :nD], cost_b=cost_b[:nCand, :nCols],
                    pairs_a=lists[0, :nC], cand=lists[1, :nCand], cols_b=lists[2, :nCols], pairs_b=lists[3, :nCand])

    def gallery(self, stream: int, track_index: int) -> np.ndarray:
        rows = np.zeros((128, FEAT_DIM), np.float32)
        cnt = C.c_int()
        self._ck(self.L.ss_get_gallery(self.ctx, stream, track_index, rows.ctypes.data_as(C.POINTER(C.c_float)), 128, C.byref(cnt)))
        return rows[: cnt.value].copy()

    def assoc_inkernel_timing(self, enable):
        """(mean microseconds, launches) of the association kernel measured by the kernel itself since the last call."""
        us, n = C.c_double(), C.c_int()
        self._ck(self.L.ss_assoc_inkernel_timing(self.ctx, int(enable), C.byref(us), C.byref(n)))
        return us.value, n.value

    def assoc_timeline(self, n_workgroups: int = 512):
        """[n_workgroups, 16] wall-clock stamps (100 MHz) of the last association launch (assoc_inkernel_timing(2))."""
        buf = np.zeros((n_workgroups, 16), np.int64)
        self._ck(self.L.ss_assoc_timeline(self.ctx, buf.ctypes.data_as(C.POINTER(C.c_longlong)), n_workgroups))
        return buf

    def assoc_timing(self, enable: bool):
        ms, n = C.c_float(), C.c_int()
        self._ck(self.L.ss_assoc_timing(self.ctx, int(enable), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def assoc_timing_values(self) -> np.ndarray:
        """Per-launch durations (ms) behind the mean the last assoc_timing() call returned."""
        n = C.c_int()
        self._ck(self.L.ss_assoc_timing_values(self.ctx, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.float32)
        self._ck(self.L.ss_assoc_timing_values(self.ctx, out.ctypes.data_as(C.POINTER(C.c_float)), n.value, C.byref(n)))
        return out[: n.value]

    # ---- stage entry points (device tensors in, device tensors out) ---------------------------------
    def _dev(self, a, dtype):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=self.device).contiguous()

    def feat_normalize(self, raw):
        raw = self._dev(raw, torch.float32)
        out = torch.empty_like(raw)
        self._ck(self.L.ss_feat_normalize(self.ctx, _ptr(raw), raw.shape[0], _ptr(out)))
        return out

    def ema(self, smooth, feat):
        s, f = self._dev(smooth, torch.float32), self._dev(feat, torch.float32)
        out = torch.empty_like(s)
        self._ck(self.L.ss_ema(self.ctx, _ptr(s), _ptr(f), s.shape[0], _ptr(out)))
        return out

    def kf_predict(self, mean, cov):
        m, c = self._dev(mean, torch.float64), self._dev(cov, torch.float64)
        self._ck(self.L.ss_kf_predict(self.ctx, _ptr(m), _ptr(c), m.shape[0]))
        return m, c

    def kf_update(self, mean, cov, z, conf):
        m, c = self._dev(mean, torch.float64), self._dev(cov, torch.float64)
        z, cf = self._dev(z, torch.float64), self._dev(conf, torch.float64)
        self._ck(self.L.ss_kf_update(self.ctx, _ptr(m), _ptr(c), _ptr(z), _ptr(cf), m.shape[0]))
        return m, c

    def kf_project(self, mean, cov, conf=None):
        """a7: (projected mean [n,4], innovation covariance [n,4,4]) of the states, NSA noise for `conf` (None: 0)."""
        m, c = self._dev(mean, torch.float64), self._dev(cov, torch.float64)
        cf = self._dev(conf, torch.float64) if conf is not None else None
        n = m.shape[0]
        z = torch.empty(n, 4, dtype=torch.float64, device=self.device)
        S = torch.empty(n, 4, 4, dtype=torch.float64, device=self.device)
        self._ck(self.L.ss_kf_project(self.ctx, _ptr(m), _ptr(c), _ptr(cf), n, _ptr(z), _ptr(S)))
        return z, S

    def kf_initiate(self, z):
        z = self._dev(z, torch.float64)
        n = z.shape[0]
        m = torch.empty(n, 8, dtype=torch.float64, device=self.device)
        c = torch.empty(n, 8, 8, dtype=torch.float64, device=self.device)
        self._ck(self.L.ss_kf_initiate(self.ctx, _ptr(z), n, _ptr(m), _ptr(c)))
        return m, c

    def gallery_pack(self, gallery):
        g = self._dev(gallery, torch.float32)            # [T,B,512]
        T, B = g.shape[0], g.shape[1]
        frag = torch.zeros(T, 4, 16384, dtype=torch.float32, device=self.device)
        self._ck(self.L.ss_gallery_pack(self.ctx, _ptr(g), T, B, _ptr(frag)))
        return frag

    def assoc_cost(self, gallery_frag, counts, feats, mean, cov, xyah):
        counts = self._dev(counts, torch.int32)
        feats = self._dev(feats, torch.float32)
        mean, cov, xyah = self._dev(mean, torch.float64), self._dev(cov, torch.float64), self._dev(xyah, torch.float64)
        T, D = counts.shape[0], feats.shape[0]
        cost = torch.empty(T, D, dtype=torch.float64, device=self.device)
        cosd = torch.empty(T, D, dtype=torch.float32, device=self.device)
        maha = torch.empty(T, D, dtype=torch.float64, device=self.device)
        gated = torch.empty(T, D, dtype=torch.uint8, device=self.device)
        self._ck(self.L.ss_assoc_cost(self.ctx, _ptr(gallery_frag), _ptr(counts), T, _ptr(feats), D, _ptr(mean),
                                      _ptr(cov), _ptr(xyah), _ptr(cost), _ptr(cosd), _ptr(maha), _ptr(gated)))
        return cost, cosd, maha, gated

    def iou_cost(self, track_tlwh, det_tlwh):
        t, d = self._dev(track_tlwh, torch.float64), self._dev(det_tlwh, torch.float64)
        cost = torch.empty(t.shape[0], d.shape[0], dtype=torch.float64, device=self.device)
        self._ck(self.L.ss_iou_cost(self.ctx, _ptr(t), t.shape[0], _ptr(d), d.shape[0], _ptr(cost)))
        return cost

    def lsap(self, cost):
        c = self._dev(cost, torch.float64)
        nr, nc = c.shape
        r2c = torch.full((max(nr, 1),), -1, dtype=torch.int32, device=self.device)
        self._ck(self.L.ss_lsap(self.ctx, _ptr(c), nr, nc, _ptr(r2c)))
        return r2c[:nr]

    # ---- front end ---------------------------------------------------------------------------------
    def letterbox(self, frame: torch.Tensor, g: LetterboxGeom, half: bool = False, pad_value: int = 114, out=None):
        """frame: uint8 [H,W,3] BGR on the device -> [3,out_h,out_w] float/half."""
        H, W = frame.shape[0], frame.shape[1]
        if out is None:
            out = torch.empty(3, g.out_h, g.out_w, dtype=torch.float16 if half else torch.float32, device=self.device)
        self._ck(self.L.ss_letterbox(self.ctx, _ptr(frame), H, W, frame.stride(0), _ptr(out), int(half), g.out_h,
                                     g.out_w, g.new_h, g.new_w, g.pad_top, g.pad_left, pad_value))
        return out

    def letterbox_batch(self, frames: torch.Tensor, g: LetterboxGeom, half: bool = False, pad_value: int = 114,
                        out=None, channels_last: bool = False):
        """frames: uint8 [B,H,W,3] BGR on the device -> [B,3,out_h,out_w] float/half in one launch;
        channels_last=True writes the NHWC memory format the convolutions read (no permute copy afterwards)."""
        B, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
        if out is None:
            out = torch.empty(B, 3, g.out_h, g.out_w, dtype=torch.float16 if half else torch.float32, device=self.device,
                              memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        flags = (_lib.DST_F16 if half else 0) | (_lib.DST_HWC if channels_last else 0)
        self._ck(self.L.ss_letterbox_batch(self.ctx, _ptr(frames), B, frames.stride(0), H, W, frames.stride(1), _ptr(out),
                                           flags, g.out_h, g.out_w, g.new_h, g.new_w, g.pad_top, g.pad_left, pad_value))
        return out

    def nms_batch(self, pred: torch.Tensor, nc: int, dcfg: DetectConfig, geom: torch.Tensor, n_extra: int = 0,
                  rows=None, keep=None, count=None, max_det: int | None = None):
        """pred: [B,(4+nc+n_extra),N] float32; geom: [B,5] float32 rows (gain, pad_x, pad_y, w0, h0), both on the
        device.  One set of launches for the whole batch."""
        B, N = pred.shape[0], pred.shape[2]
        md = min(dcfg.max_det, 1024) if max_det is None else max_det
        stride = 6 + n_extra
        if rows is None:
            rows = torch.zeros(B, md, stride, dtype=torch.float32, device=self.device)
            keep = torch.zeros(B, md, dtype=torch.int32, device=self.device)
            count = torch.zeros(B, dtype=torch.int32, device=self.device)
        self._ck(self.L.ss_nms_batch(self.ctx, _ptr(pred), B, pred.stride(0), N, nc, n_extra, dcfg.conf, dcfg.iou,
                                     int(dcfg.agnostic_nms), dcfg.max_wh, md, _ptr(geom), _ptr(rows), rows.stride(1),
                                     rows.stride(0), _ptr(keep), keep.stride(0), _ptr(count)))
        return rows, keep, count

    def nms_obb_batch(self, pred: torch.Tensor, nc: int, dcfg: DetectConfig, geom: torch.Tensor, rows=None, keep=None, count=None,
                      max_det: int | None = None):
        """Rotated NMS on ProbIoU (docs/OBB.md).  pred: [B,(4+nc+1),N] float32 (xywh, class scores, theta); geom as nms_batch's.
        rows [B,max_det,11]: the envelope, conf, cls, then cx, cy, w, h, theta in original-image pixels."""
        B, N = pred.shape[0], pred.shape[2]
        md = min(dcfg.max_det, 1024) if max_det is None else max_det
        if rows is None:
            rows = torch.zeros(B, md, 11, dtype=torch.float32, device=self.device)
            keep = torch.zeros(B, md, dtype=torch.int32, device=self.device)
            count = torch.zeros(B, dtype=torch.int32, device=self.device)
        self._ck(self.L.ss_nms_obb_batch(self.ctx, _ptr(pred), B, pred.stride(0), N, nc, dcfg.conf, dcfg.iou, int(dcfg.agnostic_nms), md,
                                         _ptr(geom), _ptr(rows), rows.stride(1), rows.stride(0), _ptr(keep), keep.stride(0), _ptr(count)))
        return rows, keep, count

    def probiou(self, a, b) -> np.ndarray:
        """float32 [n,5] x [m,5] host lists (cx, cy, w, h, theta) -> float64 [n,m], the device function on every pair (synchronous)."""
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 5)
        b = np.ascontiguousarray(b, np.float32).reshape(-1, 5)
        out = np.zeros((a.shape[0], b.shape[0]), np.float64)
        fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
        self._ck(self.L.ss_probiou(self.ctx, a.ctypes.data_as(fp), a.shape[0], b.ctypes.data_as(fp), b.shape[0], out.ctypes.data_as(dp)))
        return out

    def nms_set_classes(self, classes=None):
        """Keep only these class ids in the following NMS calls (None / empty: all) — overrides['classes']."""
        cl = [] if classes is None else ([int(classes)] if np.isscalar(classes) else [int(c) for c in classes])
        arr = (C.c_int * max(len(cl), 1))(*cl)
        self._ck(self.L.ss_nms_set_classes(self.ctx, arr, len(cl)))

    # ---- sliced inference (csrc/ss_slice.hip, docs/SLICE.md); slicing.py makes the table ----
    def slice_config(self, table, frame_hw, canvas_hw, rows_per_tile: int, n_extra: int = 0, n_kpt: int = 0, kpt_geom=(1.0, 0.0, 0.0)):
        """table: int32 [T][8] of slicing.canvas(); one state per context, a second call replaces it.  kpt_geom: (gain, pad_x, pad_y) of
        the whole frame's letterbox, what the merged rows' keypoints are expressed in."""
        t = np.ascontiguousarray(table, np.int32)
        if t.ndim != 2 or t.shape[1] != 8:
            raise ValueError("slice_config: an int32 [T, 8] table")
        self._ck(self.L.ss_slice_config(self.ctx, t.ctypes.data_as(C.POINTER(C.c_int)), t.shape[0], int(frame_hw[0]), int(frame_hw[1]),
                                        int(canvas_hw[0]), int(canvas_hw[1]), int(rows_per_tile), int(n_extra), int(n_kpt),
                                        float(kpt_geom[0]), float(kpt_geom[1]), float(kpt_geom[2])))
        self._slice = (t.shape[0], int(canvas_hw[0]), int(canvas_hw[1]), int(rows_per_tile), int(n_extra))

    def slice_nms_geom(self, batch: int) -> torch.Tensor:
        """float32 [batch * T, 5] on the device: ss_nms_batch's geometry rows of the tiles, image = frame * T + tile."""
        g = torch.zeros(batch * self._slice[0], 5, dtype=torch.float32, device=self.device)
        self._ck(self.L.ss_slice_nms_geom(self.ctx, _ptr(g), int(batch)))
        return g

    def slice_letterbox_batch(self, frames: torch.Tensor, half: bool = False, pad_value: int = 114, out=None, channels_last: bool = False):
        """frames uint8 [B,H,W,3] BGR on the device -> [B*T,3,canvas_h,canvas_w] float/half, every tile of every frame in one launch."""
        T, ch, cw = self._slice[:3]
        B = frames.shape[0]
        if out is None:
            out = torch.empty(B * T, 3, ch, cw, dtype=torch.float16 if half else torch.float32, device=self.device,
                              memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        flags = (_lib.DST_F16 if half else 0) | (_lib.DST_HWC if channels_last else 0)
        self._ck(self.L.ss_slice_letterbox_batch(self.ctx, _ptr(frames), B, frames.stride(0), frames.stride(1), _ptr(out), flags, int(pad_value)))
        return out

    def slice_merge(self, rows: torch.Tensor, counts: torch.Tensor, mode: str = "nmm", metric: str = "ios", thr: float = 0.5,
                    agnostic: bool = False, out_cap: int = 128, out=None, count=None, src=None):
        """rows [B,T,R',6+n_extra] f32 (R' >= rows_per_tile) and counts [B,T] i32 as ss_nms_batch leaves them on B*T images -> (rows
        [B,out_cap,6+n_extra] in frame pixels, counts [B], source indices [B,out_cap] = tile * rows_per_tile + row).  One launch."""
        B, ld = rows.shape[0], 6 + self._slice[4]
        if out is None:
            out = torch.zeros(B, out_cap, ld, dtype=torch.float32, device=self.device)
        if count is None:
            count = torch.zeros(B, dtype=torch.int32, device=self.device)
        if src is None:
            src = torch.zeros(B, out_cap, dtype=torch.int32, device=self.device)
        self._ck(self.L.ss_slice_merge(self.ctx, _ptr(rows), _ptr(counts), B, rows.stride(2), rows.stride(1), rows.stride(0),
                                       ("nms", "nmm").index(mode), ("iou", "ios").index(metric), float(thr), int(bool(agnostic)), int(out_cap),
                                       _ptr(out), out.stride(1), out.stride(0), _ptr(count), _ptr(src), src.stride(0)))
        return out, count, src

    def crop_norm_batch(self, frames: torch.Tensor, dets: torch.Tensor, n: int, counts=None, half: bool = False,
                        out=None, channels_last: bool = False):
        """frames uint8 [B,H,W,3], dets [B,cap,>=4] float32, counts [B] int32 -> crops [B*n,3,256,128]."""
        B, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
        if out is None:
            out = torch.empty(B * n, 3, 256, 128, dtype=torch.float16 if half else torch.float32, device=self.device,
                              memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        flags = (_lib.DST_U8 if out.dtype == torch.uint8 else _lib.DST_F16 if half else 0) | (_lib.DST_HWC if channels_last else 0)
        self._ck(self.L.ss_crop_norm_batch(self.ctx, _ptr(frames), B, frames.stride(0), H, W, frames.stride(1), _ptr(dets),
                                           dets.stride(1), dets.stride(0), n, _ptr(counts), _ptr(out), flags))
        return out

    def crop_norm_packed(self, frames: torch.Tensor, dets: torch.Tensor, n: int, counts: torch.Tensor, offsets: torch.Tensor,
                         out: torch.Tensor, half: bool = True):
        """Packed crops (channels-last `out` [B*n,3,256,128]): offsets int32 [B+1] <- exclusive prefix of min(counts, n); crop d
        of image i at slot offsets[i] + d; offsets[B] = crops in total.  A uint8 `out` receives the rounded bilinear values before
        the normalisation (SS_DST_U8: the fp32 ReID stem applies /255, mean and std itself)."""
        B, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
        flags = ((_lib.DST_U8 if out.dtype == torch.uint8 else _lib.DST_F16 if half else 0)) | _lib.DST_HWC
        self._ck(self.L.ss_crop_norm_packed(self.ctx, _ptr(frames), B, frames.stride(0), H, W, frames.stride(1), _ptr(dets),
                                            dets.stride(1), dets.stride(0), n, _ptr(counts), _ptr(offsets), _ptr(out), flags))
        return out

    def unpack_feats(self, emb: torch.Tensor, offsets: torch.Tensor, counts: torch.Tensor, n: int, feats: torch.Tensor):
        """feats[i, d, :] = emb[offsets[i] + d, :] for d < min(counts[i], n); emb [*, 512] half or float, feats [B, cap, 512] f32."""
        assert emb.is_contiguous() and feats.stride(2) == 1 and feats.stride(1) == 512
        self._ck(self.L.ss_unpack_feats(self.ctx, _ptr(emb), int(emb.dtype == torch.float16), _ptr(offsets), _ptr(counts),
                                        feats.shape[0], n, _ptr(feats), feats.stride(0)))

    def native_feats(self, maps, keep: torch.Tensor, counts: torch.Tensor, out: torch.Tensor, s: int | None = None):
        """docs/BYTETRACK.md §1d (csrc/ss_native.hip k_native_feats): BoT-SORT's `model: auto` raw features of the kept rows from the
        detector's head inputs.  maps: the three levels [B, C_l, H_l, W_l], all f16 or all f32 (any strides; a map whose channel
        stride is not 1 is copied channels-last first); keep [B, >=128] int32 anchor indices, counts [B] int32 -> out [B, 128, 512]
        f32: rows r < count hold the s = min(C_l) group means, then zeros.  Asynchronous on the engine's stream (capturable when
        no copy is needed)."""
        if len(maps) != 3:
            raise ValueError("native_feats: three head inputs (P3, P4, P5)")
        dt = maps[0].dtype
        if dt not in (torch.float16, torch.float32) or any(m.dtype != dt or m.dim() != 4 for m in maps):
            raise ValueError("native_feats: the maps must all be float16 or all float32 [B, C, H, W]")
        B = maps[0].shape[0]
        if any(m.shape[0] != B for m in maps) or keep.dtype != torch.int32 or counts.dtype != torch.int32:
            raise ValueError("native_feats: maps of one batch, int32 keep / counts")
        if out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (B, MAX_DETS, FEAT_DIM):
            raise ValueError(f"native_feats: out must be contiguous float32 [{B}, {MAX_DETS}, {FEAT_DIM}]")
        if keep.dim() != 2 or keep.shape[0] != B or keep.stride(1) != 1 or counts.numel() != B or not counts.is_contiguous():
            raise ValueError("native_feats: keep [B, >=128] with unit column stride, counts [B]")
        maps = [m if m.stride(1) == 1 else m.contiguous(memory_format=torch.channels_last) for m in maps]
        s = min(m.shape[1] for m in maps) if s is None else int(s)
        desc = (_lib.ss_native_map * 3)()
        for d, m in zip(desc, maps):
            d.data, d.img_stride, d.row_stride, d.pix_stride = m.data_ptr(), m.stride(0), m.stride(2), m.stride(3)
            d.channels, d.height, d.width = m.shape[1], m.shape[2], m.shape[3]
        self._ck(self.L.ss_native_feats(self.ctx, B, int(dt == torch.float16), desc, s, _ptr(keep), keep.stride(0), _ptr(counts), _ptr(out)))
        return out

    def pack_results(self, n_dets: torch.Tensor, dets: torch.Tensor, n_out, out, dst: torch.Tensor):
        """One frame's counts, detection rows and track rows into `dst` (float32, device or PINNED host memory) on the engine's stream:
        dst[0:2] = the two counts as int32 bits, then dets rows, then (from 2 + dets.numel()) track rows (csrc ss_pack_results)."""
        assert dets.is_contiguous() and dets.dim() == 2 and dst.dtype == torch.float32 and dst.is_contiguous()
        need = 2 + dets.numel() + (out.numel() if out is not None else 0)
        assert dst.numel() >= need and (dst.is_cuda or dst.is_pinned())
        if out is not None:
            assert out.is_contiguous() and out.dim() == 2
        self._ck(self.L.ss_pack_results(self.ctx, _ptr(n_dets), _ptr(dets), dets.shape[1], dets.shape[0], _ptr(n_out) if out is not None else None,
                                        _ptr(out) if out is not None else None, out.shape[1] if out is not None else 0,
                                        out.shape[0] if out is not None else 0, _ptr(dst)))

    def mask_assemble(self, proto: torch.Tensor, dets: torch.Tensor, counts: torch.Tensor, geom: torch.Tensor, coef_off: int,
                      bits: torch.Tensor, stream=None):
        """Packed instance masks of a frame group (csrc ss_mask.hip k_mask_assemble): proto [F, nm, mh, mw] f16 / f32, dets [F, R, ld]
        float32 (original-pixel boxes, coefficients from column coef_off), counts [F] int32, geom [F, >=3] float32 rows (gain, pad_x,
        pad_y) -> bits uint32-sized [F, R, 4 mh, ceil(4 mw / 32)] (int32 tensor), rows below each frame's count written."""
        F, nm, mh, mw = proto.shape
        assert proto.is_contiguous() and dets.is_contiguous() and bits.is_contiguous() and geom.is_contiguous()
        assert dets.dtype == torch.float32 and geom.dtype == torch.float32 and counts.dtype == torch.int32
        assert proto.dtype in (torch.float16, torch.float32) and dets.shape[0] == F and bits.shape[:2] == dets.shape[:2]
        self._ck(self.L.ss_mask_assemble(self.ctx, self._st(stream), _ptr(proto), int(proto.dtype == torch.float16), proto.stride(0),
                                         nm, mh, mw, _ptr(dets), dets.stride(0), dets.shape[2], coef_off, _ptr(counts), F, dets.shape[1],
                                         _ptr(geom), geom.stride(0) if F > 1 else 0, 4 * mh, 4 * mw, _ptr(bits), bits.stride(0)))

    def mask_outline(self, bits: torch.Tensor, counts: torch.Tensor, iw: int, pts: torch.Tensor, npts: torch.Tensor, scratch: torch.Tensor,
                     bits_copy: torch.Tensor = None, stream=None):
        """The polygon yolo.mask_polygon returns for every kept row of packed masks bits [F, R, ih, ceil(iw/32)] (csrc k_mask_outline):
        pts [F, R, cap, 2] int32, npts [F, R] int32 (-length: longer than cap, no points).  scratch: label planes (4 ih iw bytes
        each, one per workgroup).  bits_copy (device or pinned host, bits' shape): a copy of every processed plane."""
        F, R, ih = bits.shape[:3]
        assert bits.is_contiguous() and pts.is_contiguous() and npts.is_contiguous() and pts.dtype == torch.int32 and npts.dtype == torch.int32
        assert pts.shape[:2] == (F, R) and npts.shape == (F, R) and counts.dtype == torch.int32
        if bits_copy is not None:
            assert bits_copy.is_contiguous() and bits_copy.shape[1:] == bits.shape[1:] and (bits_copy.is_cuda or bits_copy.is_pinned())
        self._ck(self.L.ss_mask_outline(self.ctx, self._st(stream), _ptr(bits), bits.stride(0), _ptr(counts), F, R, ih, iw,
                                        pts.shape[2], _ptr(pts), pts.stride(0), _ptr(npts), npts.stride(0), _ptr(bits_copy),
                                        bits_copy.stride(0) if bits_copy is not None else 0, _ptr(scratch), scratch.numel() * scratch.element_size()))

    def nms(self, pred: torch.Tensor, nc: int, dcfg: DetectConfig, gain: float, pad_x: float, pad_y: float,
            w0: int, h0: int, n_extra: int = 0, rows=None, keep=None, count=None):
        """pred: [(4+nc+n_extra), N] float32 on the device."""
        N = pred.shape[1]
        md = min(dcfg.max_det, 1024)
        stride = 6 + n_extra
        if rows is None:
            rows = torch.zeros(md, stride, dtype=torch.float32, device=self.device)
            keep = torch.zeros(md, dtype=torch.int32, device=self.device)
            count = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._ck(self.L.ss_nms(self.ctx, _ptr(pred), N, nc, n_extra, dcfg.conf, dcfg.iou, int(dcfg.agnostic_nms),
                               dcfg.max_wh, md, gain, pad_x, pad_y, float(w0), float(h0), _ptr(rows), stride,
                               _ptr(keep), _ptr(count)))
        return rows, keep, count

    def crop_norm(self, frame: torch.Tensor, dets: torch.Tensor, n: int, count=None, half: bool = False, out=None):
        H, W = frame.shape[0], frame.shape[1]
        if out is None:
            out = torch.empty(n, 3, 256, 128, dtype=torch.float16 if half else torch.float32, device=self.device)
        self._ck(self.L.ss_crop_norm(self.ctx, _ptr(frame), H, W, frame.stride(0), _ptr(dets), dets.stride(0), n,
                                     _ptr(count), _ptr(out), int(half)))
        return out


class _AttachedTracker:
    """A tracker family attached to the context of a TrackerEngine: what ByteTrackEngine, OCSortEngine and DeepOCSortEngine share.
    `engine`: the TrackerEngine whose context (NMS, streams, error words) the tracker shares; None: a context of its own."""
    # the class's name in its messages; the family's destroy and reset entries; the setting that makes update calls read features
    _name = _destroy = _reset = _feats_need = ""
    _delegated = ("use_stream", "use_current_stream", "check_errors")      # the context's own, under the tracker's name too
    reid = pose = False

    def __init__(self, n_streams: int, device: int, engine):
        self._own = engine is None
        self.base = TrackerEngine(StrongSortConfig(), n_streams, device) if engine is None else engine
        self.S, self.device, self.L = self.base.S, self.base.device, self.base.L
        self.out = torch.zeros(self.S, MAX_TRACKS, OUT_COLS, dtype=torch.float32, device=self.device)
        self.nout = torch.zeros(self.S, dtype=torch.int32, device=self.device)
        for name in self._delegated:
            setattr(self, name, getattr(self.base, name))

    @property
    def ctx(self):
        return self.base.ctx

    @property
    def max_group_frames(self) -> int:
        return self.base.max_group_frames

    def _ck(self, rc):
        _lib.check(self.base.ctx, rc)

    def close(self):
        if self._own:
            self.base.close()
        elif getattr(self.base, "ctx", None) and self.base.ctx.value:
            torch.cuda.synchronize(self.device)
            self._ck(getattr(self.L, self._destroy)(self.base.ctx))

    def reset(self, stream: int = -1):
        """Restart the stream(s) (-1: all): ids from 1, frame count 0, and whatever else the family keeps per stream (BYTE and Deep
        OC-SORT: the tracks' features or poses, and the next estimated frame gets no warp, G-04)."""
        self._ck(getattr(self.L, self._reset)(self.base.ctx, stream))

    def _feats(self, feats, rows):
        if not self.reid:
            return None
        if feats is None:
            raise ValueError(f"{self._name}: {self._feats_need} needs the detections' features [.., 128, 512] f32")
        if feats.dtype != torch.float32 or not feats.is_contiguous() or feats.numel() != rows * MAX_DETS * FEAT_DIM:
            raise ValueError(f"{self._name}: feats must be contiguous float32 [{rows} x {MAX_DETS} x {FEAT_DIM}]")
        return feats

    def update_device(self, dets, ndets, feats=None, img_hw=None, out=None, nout=None):
        """All streams, one frame: dets [S,128,6] f32, ndets [S] i32, feats [S,128,512] f32 (raw, device; read by the trackers that use
        features) -> (rows [S,256,8], counts [S]) device tensors, asynchronous; the engine's own unless out / nout are given.  img_hw is
        accepted for TrackerEngine's call shape and unused."""
        return self.update_group(1, dets, ndets, feats, img_hw, self.out if out is None else out, self.nout if nout is None else nout)


class ByteTrackEngine(_AttachedTracker):
    """The BYTE tracker family (csrc/ss_byte.hip, docs/BYTETRACK.md) on the context of a TrackerEngine: the same
    update_device / update_group / reset / check_errors shape as TrackerEngine; features only with cfg.with_reid (§1c, BoT-SORT's
    ReID branch, switched on at construction), keypoints only with cfg.with_pose (§1e, the OKS term, likewise).  `engine`: share the
    context of an existing TrackerEngine (a pipeline's: its NMS, streams and error words); None: a context of its own."""

    _name, _destroy, _reset, _feats_need = "ByteTrackEngine", "ss_byte_destroy", "ss_byte_reset", "with_reid"
    # the context's own: streams, error words, the warps of a group (N4: frames uint8 [F*S,H,W,3] -> [F,S,8]) and their stages
    _delegated = _AttachedTracker._delegated + ("cmc_estimate", "gmc_sparse_estimate", "estimate_warps", "gmc_sparse_stages", "cmc_small")

    def __init__(self, cfg: ByteTrackConfig | None = None, n_streams: int = 1, device: int = 0, engine: TrackerEngine | None = None,
                 obb: bool = False):
        self.cfg = cfg or ByteTrackConfig()
        if obb and (self.cfg.with_reid or self.cfg.with_pose):
            raise ValueError("ByteTrackEngine: oriented boxes (obb=True) are not combined with with_reid or with_pose (docs/OBB.md §4)")
        super().__init__(n_streams, device, engine)
        c = _lib.make_byte_config(self.cfg)
        self._ck(self.L.ss_byte_create(self.base.ctx, C.byref(c)))
        self.reid = bool(self.cfg.with_reid)
        if self.reid:                               # §1c: BoT-SORT's appearance term (resets the streams)
            self._ck(self.L.ss_byte_set_reid(self.base.ctx, 1, float(self.cfg.proximity_thresh), float(self.cfg.appearance_thresh),
                                             float(self.cfg.feat_alpha)))
        self.pose = bool(self.cfg.with_pose)
        self.K = len(self.cfg.kpt_sigmas)
        if self.pose:                               # §1e: the keypoint term (resets the streams)
            sg = (C.c_double * self.K)(*[float(v) for v in self.cfg.kpt_sigmas])
            self._ck(self.L.ss_byte_set_pose(self.base.ctx, 1, self.K, sg, float(self.cfg.proximity_thresh), float(self.cfg.pose_thresh),
                                             float(self.cfg.kpt_vis_thresh), int(self.cfg.min_common_kpts)))
        self.obb = False
        if obb:                                     # docs/OBB.md §4: association on ProbIoU, 11-column rows (resets the streams)
            self.set_obb(True)
        self._cmc_keep = None

    def set_obb(self, on: bool):
        """docs/OBB.md §4: association on ProbIoU of rotated boxes on or off; every stream restarts.  While on, update_group takes
        ss_nms_obb_batch's 11-column rows and fills `rbox`."""
        self._ck(self.L.ss_byte_set_obb(self.base.ctx, int(bool(on))))
        self.obb = bool(on)
        if self.obb and getattr(self, "rbox", None) is None:
            self.rbox = torch.zeros(self.S, MAX_TRACKS, 5, dtype=torch.float32, device=self.device)

    def angles(self, stream: int = 0) -> np.ndarray:
        """docs/OBB.md §4: the tracks' angles [n] f32 of one stream in tracks()' list order (R-06: the last row's, not filtered)."""
        an = np.zeros(MAX_TRACKS, np.float32)
        self._ck(self.L.ss_byte_get_angles(self.base.ctx, stream, MAX_TRACKS, an.ctypes.data_as(C.POINTER(C.c_float))))
        t = self.tracks(stream)
        return an[:t["n_tracked"] + t["n_lost"]].copy()

    def set_cmc(self, warps):
        """BoT-SORT GMC (docs/BYTETRACK.md §1b): the following update calls move every track by these warps ([F,S,8] float64,
        ss_cmc_estimate's layout, at least as many rows as the calls' frames) after predicting; None: off.  xywh only."""
        self._ck(self.L.ss_byte_set_gmc(self.base.ctx, _ptr(warps)))
        self._cmc_keep = warps

    def _kpts(self, kpts, rows, kpt_col, geom):
        """with_pose: the rows' keypoints as (tensor, row stride, column, geometry) for ss_byte_update_group_kpts.  kpts: float32,
        [rows x 128 x C] with unit column stride — [.., K, 3] triplets (kpt_col 0) or whole NMS rows with the triplets from column
        kpt_col; geom [rows, 5] f32 (ss_nms_batch's rows): the keypoints are network-input pixels, None: original pixels."""
        if kpts is None:
            raise ValueError("ByteTrackEngine: with_pose needs the detections' keypoints [.., 128, K, 3] f32")
        if kpts.dim() >= 3 and kpts.shape[-1] == 3 and kpts.shape[-2] == self.K and kpt_col == 0:
            kpts = kpts.reshape(-1, MAX_DETS, 3 * self.K) if kpts.is_contiguous() else kpts
        C_ = kpts.shape[-1]
        if kpts.dtype != torch.float32 or not kpts.is_contiguous() or kpts.numel() != rows * MAX_DETS * C_ or kpt_col < 0 or C_ < kpt_col + 3 * self.K:
            raise ValueError(f"ByteTrackEngine: kpts must be contiguous float32 [{rows} x {MAX_DETS} x C], C >= kpt_col + {3 * self.K}")
        if geom is not None and (geom.dtype != torch.float32 or not geom.is_contiguous() or geom.numel() != rows * 5):
            raise ValueError(f"ByteTrackEngine: geom must be contiguous float32 [{rows} x 5]")
        return kpts, C_, int(kpt_col), geom

    def update_device(self, dets, ndets, feats=None, img_hw=None, out=None, nout=None, kpts=None, kpt_col=0, geom=None):
        """All streams, one frame: dets [S,128,6] f32, ndets [S] i32, with ReID feats [S,128,512] f32 (raw, device), with the
        keypoint term kpts (see update_group) -> (rows [S,256,8], counts [S]) device tensors, asynchronous.  img_hw is accepted
        for TrackerEngine's call shape and unused (no clipping); feats is unused without ReID."""
        return self.update_group(1, dets, ndets, feats, img_hw, self.out if out is None else out, self.nout if nout is None else nout,
                                 kpts=kpts, kpt_col=kpt_col, geom=geom)

    def update_group(self, n_frames, dets, ndets, feats, img_hw, out, nout, kpts=None, kpt_col=0, geom=None, rbox=None):
        """A group of n_frames (<= 32) frames of all streams in ONE launch: dets [F,S,128,6] f32, ndets [F,S] i32, with ReID
        feats [F,S,128,512] f32 -> rows out [F,S,256,8], counts nout [F,S] (device tensors, asynchronous); frames are
        associated in order.  img_hw unused (TrackerEngine's call shape), feats unused without ReID.  With the keypoint term (§1e):
        kpts [F,S,128,K,3] f32 triplets (x, y, v) in the dets' pixels — or the NMS rows themselves [F*S,128,C] with the triplets
        from column kpt_col in network-input pixels and geom [F*S,5] (the NMS geometry rows) to bring them to the dets' pixels.
        With oriented boxes (set_obb): dets [F,S,128,11] f32 (ss_nms_obb_batch's rows), rows' columns 0..3 the envelope of the track's
        rotated box, and rbox [F,S,256,5] f32 its cx, cy, w, h, theta (None: self.rbox, one frame's)."""
        if self.obb:
            rbox = self.rbox if rbox is None else rbox
            if dets.dtype != torch.float32 or not dets.is_contiguous() or dets.numel() != int(n_frames) * self.S * MAX_DETS * 11:
                raise ValueError(f"ByteTrackEngine: with oriented boxes dets must be contiguous float32 [{int(n_frames) * self.S} x {MAX_DETS} x 11]")
            if rbox.dtype != torch.float32 or not rbox.is_contiguous() or rbox.numel() < int(n_frames) * self.S * MAX_TRACKS * 5:
                raise ValueError(f"ByteTrackEngine: rbox must be contiguous float32 [{int(n_frames) * self.S} x {MAX_TRACKS} x 5]")
            self._ck(self.L.ss_byte_update_group_obb(self.base.ctx, int(n_frames), _ptr(dets), _ptr(ndets), _ptr(out), _ptr(rbox), _ptr(nout)))
        elif self.pose:
            k, stride, col, g = self._kpts(kpts, int(n_frames) * self.S, kpt_col, geom)
            self._ck(self.L.ss_byte_update_group_kpts(self.base.ctx, int(n_frames), _ptr(dets), _ptr(ndets), _ptr(k), stride, col,
                                                      _ptr(g), _ptr(out), _ptr(nout)))
        elif self.reid:
            f = self._feats(feats, int(n_frames) * self.S)
            self._ck(self.L.ss_byte_update_group_feats(self.base.ctx, int(n_frames), _ptr(dets), _ptr(ndets), _ptr(f), _ptr(out), _ptr(nout)))
        else:
            self._ck(self.L.ss_byte_update_group(self.base.ctx, int(n_frames), _ptr(dets), _ptr(ndets), _ptr(out), _ptr(nout)))
        return out, nout

    def features(self, stream: int = 0) -> np.ndarray:
        """§1c: the unit track features [n,512] f32 of one stream in tracks()' list order (ReID only)."""
        if not self.reid:
            raise RuntimeError("ByteTrackEngine.features: with_reid is off")
        sm = np.zeros((MAX_TRACKS, FEAT_DIM), np.float32)
        self._ck(self.L.ss_byte_get_features(self.base.ctx, stream, MAX_TRACKS, sm.ctypes.data_as(C.POINTER(C.c_float))))
        t = self.tracks(stream)
        return sm[:t["n_tracked"] + t["n_lost"]].copy()

    def keypoints(self, stream: int = 0):
        """§1e: the stored poses of one stream in tracks()' list order (with_pose only): (offsets [n,K,2] float64 from the box centre
        in box widths / heights, visibility words [n] uint32, bit k = keypoint k)."""
        if not self.pose:
            raise RuntimeError("ByteTrackEngine.keypoints: with_pose is off")
        off, vis = np.zeros((MAX_TRACKS, self.K, 2)), np.zeros(MAX_TRACKS, np.uint32)
        self._ck(self.L.ss_byte_get_keypoints(self.base.ctx, stream, MAX_TRACKS, off.ctypes.data_as(C.POINTER(C.c_double)),
                                              vis.ctypes.data_as(C.POINTER(C.c_uint32))))
        t = self.tracks(stream)
        n = t["n_tracked"] + t["n_lost"]
        return off[:n].copy(), vis[:n].copy()

    def det_keypoints(self, frame: int = 0, stream: int = 0):
        """§1e (tests): what the last update call's first launch prepared for image (frame, stream): (xy [128,K,2] float32 in
        original pixels, visibility words [128] uint32); rows past the image's count are not written."""
        xy, vis = np.zeros((MAX_DETS, self.K, 2), np.float32), np.zeros(MAX_DETS, np.uint32)
        self._ck(self.L.ss_byte_get_det_keypoints(self.base.ctx, frame, stream, xy.ctypes.data_as(C.POINTER(C.c_float)),
                                                  vis.ctypes.data_as(C.POINTER(C.c_uint32))))
        return xy, vis

    def tracks(self, stream: int = 0) -> dict:
        """The table of one stream in list order (tracked, then lost): track_id, state (1 tracked, 2 lost), activated, mean."""
        T = MAX_TRACKS
        nt, nl, nid, fr = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        ids, st, act = np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T, np.int32)
        mean = np.zeros((T, 8))
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        self._ck(self.L.ss_byte_get_tracks(self.base.ctx, stream, T, C.byref(nt), C.byref(nl), C.byref(nid), C.byref(fr),
                                           ids.ctypes.data_as(ip), st.ctypes.data_as(ip), act.ctypes.data_as(ip), mean.ctypes.data_as(dp)))
        k = nt.value + nl.value
        return dict(track_id=ids[:k].copy(), state=st[:k].copy(), activated=act[:k].copy(), mean=mean[:k].copy(),
                    n_tracked=nt.value, n_lost=nl.value, next_id=nid.value, frame_id=fr.value)


class OCSortEngine(_AttachedTracker):
    """OC-SORT (csrc/ss_ocsort.hip, docs/OCSORT.md) on the context of a TrackerEngine: the same update_device / update_group /
    reset / check_errors shape as ByteTrackEngine, without features, keypoints or warps.  `engine`: share the context of an
    existing TrackerEngine (a pipeline's: its NMS, streams and error words); None: a context of its own."""

    _name, _destroy, _reset = "OCSortEngine", "ss_ocsort_destroy", "ss_ocsort_reset"

    def __init__(self, cfg: OCSortConfig | None = None, n_streams: int = 1, device: int = 0, engine: TrackerEngine | None = None):
        self.cfg = cfg or OCSortConfig()
        super().__init__(n_streams, device, engine)
        c = _lib.make_ocsort_config(self.cfg)
        self._ck(self.L.ss_ocsort_create(self.base.ctx, C.byref(c)))

    def update_group(self, n_frames, dets, ndets, feats, img_hw, out, nout):
        """A group of n_frames (<= 32) frames of all streams in ONE launch: dets [F,S,128,6] f32, ndets [F,S] i32 -> rows out
        [F,S,256,8], counts nout [F,S] (device tensors, asynchronous); frames are associated in order.  feats, img_hw unused."""
        self._ck(self.L.ss_ocsort_update_group(self.base.ctx, int(n_frames), _ptr(dets), _ptr(ndets), _ptr(out), _ptr(nout)))
        return out, nout

    def tracks(self, stream: int = 0) -> dict:
        """The table of one stream in list order (oldest track first): what tests/ocsort_ref.py's tracks() returns."""
        return self._tracks(self.L.ss_ocsort_get_tracks, stream)

    def _tracks(self, get, stream: int) -> dict:
        T = MAX_TRACKS
        nt, nid, fr = C.c_int(), C.c_int(), C.c_int()
        names = ("track_id", "age", "time_since_update", "hits", "hit_streak", "frozen")
        iv = {n: np.zeros(T, np.int32) for n in names}
        x, P, lo, vel = np.zeros((T, 7)), np.zeros((T, 49)), np.zeros((T, 4), np.float32), np.zeros((T, 2))
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        self._ck(get(self.base.ctx, stream, T, C.byref(nt), C.byref(nid), C.byref(fr),
                 *[iv[n].ctypes.data_as(ip) for n in names], x.ctypes.data_as(dp), P.ctypes.data_as(dp),
                                             lo.ctypes.data_as(C.POINTER(C.c_float)), vel.ctypes.data_as(dp)))
        k = nt.value
        return dict({n: iv[n][:k].copy() for n in names}, x=x[:k].copy(), P=P[:k].copy(), last_obs=lo[:k].copy(), velocity=vel[:k].copy(),
                    n_tracks=k, next_id=nid.value, frame_count=fr.value)


class HybridSortEngine(_AttachedTracker):
    """Hybrid-SORT (csrc/ss_hybrid.hip, docs/HYBRIDSORT.md) on the context of a TrackerEngine: OCSortEngine's shape, without
    features, keypoints or warps.  `engine`: share the context of an existing TrackerEngine; None: a context of its own."""

    _name, _destroy, _reset = "HybridSortEngine", "ss_hybridsort_destroy", "ss_hybridsort_reset"

    def __init__(self, cfg: HybridSortConfig | None = None, n_streams: int = 1, device: int = 0, engine: TrackerEngine | None = None):
        self.cfg = cfg or HybridSortConfig()
        super().__init__(n_streams, device, engine)
        c = _lib.make_hybridsort_config(self.cfg)
        self._ck(self.L.ss_hybridsort_create(self.base.ctx, C.byref(c)))

    def update_group(self, n_frames, dets, ndets, feats, img_hw, out, nout):
        """A group of n_frames (<= 32) frames of all streams in ONE launch: dets [F,S,128,6] f32, ndets [F,S] i32 -> rows out
        [F,S,256,8], counts nout [F,S] (device tensors, asynchronous); frames are associated in order.  feats, img_hw unused."""
        self._ck(self.L.ss_hybridsort_update_group(self.base.ctx, int(n_frames), _ptr(dets), _ptr(ndets), _ptr(out), _ptr(nout)))
        return out, nout

    def tracks(self, stream: int = 0) -> dict:
        """The table of one stream in list order (oldest track first): what tests/hybridsort_ref.py's tracks() returns."""
        T = MAX_TRACKS
        nt, nid, fr = C.c_int(), C.c_int(), C.c_int()
        names = ("track_id", "age", "time_since_update", "hits", "hit_streak", "frozen")
        iv = {n: np.zeros(T, np.int32) for n in names}
        x, P, lo, vel = np.zeros((T, 9)), np.zeros((T, 81)), np.zeros((T, 4), np.float32), np.zeros((T, 8))
        conf, prev = np.zeros(T, np.float32), np.zeros(T, np.float32)
        ip, dp, fp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float)
        self._ck(self.L.ss_hybridsort_get_tracks(self.base.ctx, stream, T, C.byref(nt), C.byref(nid), C.byref(fr),
                                                 *[iv[n].ctypes.data_as(ip) for n in names], x.ctypes.data_as(dp), P.ctypes.data_as(dp),
                                                 lo.ctypes.data_as(fp), vel.ctypes.data_as(dp), conf.ctypes.data_as(fp), prev.ctypes.data_as(fp)))
        k = nt.value
        return dict({n: iv[n][:k].copy() for n in names}, x=x[:k].copy(), P=P[:k].copy(), last_obs=lo[:k].copy(), velocity=vel[:k].copy(),
                    conf=conf[:k].copy(), conf_prev=prev[:k].copy(), n_tracks=k, next_id=nid.value, frame_count=fr.value)


class DeepOCSortEngine(OCSortEngine):
    """Deep OC-SORT (csrc/ss_deepoc.hip, docs/DEEPOCSORT.md) on the context of a TrackerEngine: OCSortEngine's shape with the
    detections' raw features (read while cfg.appearance is on) and BoT-SORT's set_cmc.  It stands where the BYTE / OC-SORT engine
    stands.  `engine`: share the context of an existing TrackerEngine; None: a context of its own."""

    _name, _destroy, _reset, _feats_need = "DeepOCSortEngine", "ss_deepoc_destroy", "ss_deepoc_reset", "appearance"
    _delegated = _AttachedTracker._delegated + ("cmc_estimate", "gmc_sparse_estimate", "estimate_warps")

    def __init__(self, cfg: DeepOCSortConfig | None = None, n_streams: int = 1, device: int = 0, engine: TrackerEngine | None = None):
        self.cfg = cfg or DeepOCSortConfig()
        _AttachedTracker.__init__(self, n_streams, device, engine)
        c = _lib.make_deepoc_config(self.cfg)
        self._ck(self.L.ss_deepoc_create(self.base.ctx, C.byref(c)))
        self.reid = bool(self.cfg.appearance)
        self._cmc_keep = None

    def set_cmc(self, warps):
        """Step 1b: the following update calls move every track by these warps ([F,S,8] float64, ss_cmc_estimate's layout, at least
        as many rows as the calls' frames) before predicting; None: off."""
        self._ck(self.L.ss_deepoc_set_gmc(self.base.ctx, _ptr(warps)))
        self._cmc_keep = warps

    def update_group(self, n_frames, dets, ndets, feats, img_hw, out, nout):
        """A group of n_frames (<= 32) frames of all streams in one call: dets [F,S,128,6] f32, ndets [F,S] i32, feats
        [F,S,128,512] f32 -> rows out [F,S,256,8], counts nout [F,S] (device tensors, asynchronous); frames are associated in order."""
        f = self._feats(feats, int(n_frames) * self.S)
        self._ck(self.L.ss_deepoc_update_group(self.base.ctx, int(n_frames), _ptr(dets), _ptr(ndets), _ptr(f), _ptr(out), _ptr(nout)))
        return out, nout

    def tracks(self, stream: int = 0) -> dict:
        """The table of one stream in list order (oldest track first): what tests/deepocsort_ref.py's tracks() returns."""
        return self._tracks(self.L.ss_deepoc_get_tracks, stream)

    def features(self, stream: int = 0) -> np.ndarray:
        """The tracks' unit features [n,512] f32 of one stream in tracks()' list order."""
        em = np.zeros((MAX_TRACKS, FEAT_DIM), np.float32)
        self._ck(self.L.ss_deepoc_get_features(self.base.ctx, stream, MAX_TRACKS, em.ctypes.data_as(C.POINTER(C.c_float))))
        return em[:self.tracks(stream)["n_tracks"]].copy()
