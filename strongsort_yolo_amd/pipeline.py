"""Per-frame tracking pipeline for the S streams owned by one GPU (one process per GPU).

    frame (u8, HBM) -> letterbox [HIP] -> detector [own HIP conv kernels behind nets.py modules] -> NMS [HIP]
      -> ReID crops [HIP] -> OSNet [own HIP kernels] -> StrongSORT update [HIP: k_group_prep / k_assoc / k_frame / k_post / k_newrow]

This is what runs inside `model.track(frame, persist=True)` (/root/reference/yolo_multi_model.py:41).
Everything between the frame and the output rows stays on the device: detection counts, track
counts and assignment results are device-side values, so the whole step is a fixed launch sequence
that is captured once into a HIP graph and replayed per frame (no host round trip, no per-frame
allocation).

Synthetic-workload switches (no weights / no decoder exist offline):
  det_source = "detector"  NMS consumes the detector head output (true end to end)
             = "synthetic" NMS consumes `pred_in` filled by the caller (the detector still runs)
  feat_source = "reid"     the tracker consumes the OSNet embeddings
              = "injected" the tracker consumes `feats_in` filled by the caller (OSNet still runs)
              = "by_anchor" the tracker consumes gt_feats[anchor_gt[keep]]: the feature of the
                            synthetic identity whose anchor survived NMS (OSNet still runs)
  graph = "all"   whole step in one HIP graph;  "front" everything up to the ReID output in the
          graph and the tracker kernels launched eagerly (lets bench.py bracket the association
          kernel with HIP events);  "split" three graphs (detection | ReID | tracker) so that a
          detection-only call replays only the first;  "none" eager.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .config import StrongSortConfig, DetectConfig
from .engine import TrackerEngine, letterbox_geometry, scale_geometry
from .lib import MAX_DETS, MAX_TRACKS, FEAT_DIM
from . import nets


class FramePipeline:
    def __init__(self, detector: str = "yolov8n", n_streams: int = 1, frame_hw=(720, 1280), device: int = 0,
                 half: bool = True, reid_batch: int = 32, cfg: Optional[StrongSortConfig] = None,
                 dcfg: Optional[DetectConfig] = None, det_source: str = "detector", feat_source: str = "reid",
                 graph: str = "all", debug: bool = False, run_nets: bool = True, seed: int = 0, detect_only_rows: int = 0, cmc: bool = False,
                 reid_half: Optional[bool] = None, crops_u8: bool = True, tracker: str = "strongsort", with_reid: bool = False,
                 reid_model: str = "osnet", with_pose: bool = False, gmc_method: str = "ecc", ocsort_use_byte: bool = False, slice_cfg=None,
                 track_bank: bool = False, bank_max_ids: int = 4096, hybrid_asso: str = "hmiou", hybrid_use_byte: bool = True):
        self.cfg, self.dcfg = cfg or StrongSortConfig(), dcfg or DetectConfig()
        self.S, (self.H, self.W) = n_streams, frame_hw
        # tracker = "bytetrack" / "botsort": the BYTE tracker family (csrc/ss_byte.hip) on IoU and scores — no OSNet is built, no
        # crops are cut, the ReID stages drop out of the graphs; the tracker keeps the NMS rows' order (det_idx).
        # with_reid (botsort only): BoT-SORT's ReID branch (docs/BYTETRACK.md §1c) — OSNet, crops and ReID stages stay as for
        # StrongSORT and the BYTE tracker reads the same features.
        # reid_model = "auto" (with_reid only): Ultralytics' `model: auto` (docs/BYTETRACK.md §1d) — no OSNet is built, no crops are
        # cut; one launch after NMS reads the kept rows' features from the detector's own head inputs (a forward pre-hook on
        # detector.detect keeps them until that launch is enqueued)
        # with_pose (botsort only, not with with_reid): the keypoint term (docs/BYTETRACK.md §1e) — the tracker call reads the
        # keypoint columns of the NMS rows in place (b.dets, row stride 6 + nk + nm, column 6) with the NMS geometry; no copy, no stage.
        # gmc_method (cmc only): "ecc" (csrc/ss_cmc.hip) or, for botsort, "sparseOptFlow" (docs/BYTETRACK.md §1f, csrc/ss_gmc.hip):
        # which estimator fills the group's warps; the tracker call reads either the same way.
        # tracker = "ocsort": OC-SORT (csrc/ss_ocsort.hip, docs/OCSORT.md) — motion only: like the BYTE family without ReID it builds no
        # OSNet and cuts no crops, and its engine stands where the BYTE engine stands (self.byte / self.trk: the same stage bodies).
        # tracker = "deep_ocsort": Deep OC-SORT (csrc/ss_deepoc.hip, docs/DEEPOCSORT.md) — OSNet, crops and ReID stages stay as for botsort
        # with with_reid, the warps stage as for botsort; its engine stands where the BYTE engine stands.
        # tracker = "hybridsort": Hybrid-SORT (csrc/ss_hybrid.hip, docs/HYBRIDSORT.md) — motion only, as "ocsort": no OSNet, no crops, its
        # engine stands where the BYTE engine stands; hybrid_asso ("hmiou" / "iou") and hybrid_use_byte are its two switches.
        # slice_cfg (slicing.SliceConfig): sliced inference (csrc/ss_slice.hip, docs/SLICE.md) — the detector sees T tiles of every frame
        # (S * T images: lb, pred_in and the per-tile NMS rows carry that leading dimension), one launch letterboxes them, one launch
        # merges the tiles' rows into b.dets / b.ndets; from there on nothing differs.  None: nothing of it is allocated or launched.
        # track_bank: one pooled appearance descriptor per track id, kept on the device behind every tracker call (csrc/ss_mtmc.hip,
        # docs/MTMC.md): one more launch per call that reads the rows and the features where they are.  Off: nothing is allocated or launched.
        from .config import byte_config, ocsort_config, deep_ocsort_config, hybridsort_config, check_reid_model, check_pose, check_gmc_method
        self.slice = slice_cfg
        self.bank = None
        if track_bank and not detect_only_rows:
            from .mtmc import bank_refusal
            why = bank_refusal(tracker, with_reid, reid_model, detector.lower().replace(".pt", "") in nets.OBB_DETECTORS)
            if why:
                raise ValueError(f"track_bank: {why}")
        # an oriented-box model (docs/OBB.md §5): one angle row behind the class scores, the rotated NMS, 11-column rows (nx = 5), and
        # the BYTE family on ProbIoU; what is not built for rotated boxes is refused by name before anything is allocated
        self.ne = 1 if detector.lower().replace(".pt", "") in nets.OBB_DETECTORS else 0
        if self.ne:
            if tracker in ("ocsort", "deep_ocsort", "hybridsort") or (tracker == "strongsort" and not detect_only_rows):
                raise ValueError(f"'{detector}' is an oriented-box model: tracker '{tracker}' associates on axis-aligned boxes; use 'bytetrack' or "
                                 "'botsort' (ProbIoU of the rotated boxes, docs/OBB.md §4)")
            for on, what in ((with_reid, "with_reid"), (reid_model == "auto", "reid_model='auto'"), (with_pose, "with_pose"),
                             (cmc, "camera_motion"), (slice_cfg is not None, "slice_hw")):
                if on:
                    raise ValueError(f"'{detector}' is an oriented-box model: {what} is not built for rotated boxes (docs/OBB.md §5)")
        if self.slice is not None and reid_model == "auto":
            raise ValueError("sliced inference cannot feed reid_model='auto': the detector's anchor indices are per tile")
        self.hy_cfg = hybridsort_config(tracker, hybrid_asso, hybrid_use_byte, cmc, with_reid, with_pose, ocsort_use_byte)
        self.deep_cfg = deep_ocsort_config(tracker, with_reid, with_pose, ocsort_use_byte)
        self.oc_cfg = ocsort_config(tracker, ocsort_use_byte, cmc, with_reid, with_pose)
        self.byte_cfg = byte_config(tracker, with_reid, with_pose)
        self.gmc_method = check_gmc_method(gmc_method, cmc, tracker)
        self.reid_model = check_reid_model(reid_model, with_reid)
        self.tracker = tracker
        self.native = self.reid_model == "auto" and not detect_only_rows
        self.need_reid = (self.byte_cfg is None and self.oc_cfg is None and self.hy_cfg is None) or (self.byte_cfg is not None and self.byte_cfg.with_reid and self.reid_model == "osnet")
        if self.byte_cfg is not None and cmc and self.byte_cfg.kalman != "xywh":
            raise ValueError("camera-motion compensation needs tracker 'strongsort' or 'botsort' (ByteTrack has no GMC)")
        self.eng = TrackerEngine(self.cfg, n_streams, device, debug=debug)
        # trk: the tracker whose update_device / update_group / set_cmc the pipeline calls (BoT-SORT: GMC on the BYTE state, §1b)
        self.byte, self.trk = None, self.eng
        if self.byte_cfg is not None:
            from .engine import ByteTrackEngine
            self.byte = self.trk = ByteTrackEngine(self.byte_cfg, engine=self.eng, obb=bool(self.ne))
        elif self.oc_cfg is not None:
            from .engine import OCSortEngine
            self.byte = self.trk = OCSortEngine(self.oc_cfg, engine=self.eng)
        elif self.hy_cfg is not None:
            from .engine import HybridSortEngine
            self.byte = self.trk = HybridSortEngine(self.hy_cfg, engine=self.eng)
        elif self.deep_cfg is not None:
            from .engine import DeepOCSortEngine
            self.byte = self.trk = DeepOCSortEngine(self.deep_cfg, engine=self.eng)
        if track_bank and not detect_only_rows:
            from .mtmc import TrackBank
            self.bank = TrackBank(self.eng, bank_max_ids)
        dev = self.dev = self.eng.device
        self.half, self.dtype = half, torch.float16 if half else torch.float32
        # reid_half=False: the ReID crops and OSNet in fp32 on the hand-written fp32 kernels (fused32.py, csrc/ss_ops32.hip:
        # v_mfma_f32_16x16x4_f32) beside a half detector — the accuracy mode: appearance distances then agree with a CPU fp32
        # OSNet to ~1e-5, which f16 activations do not (bench.py reid_f16_vs_f32; north_star's 1e-4 bound on float distances;
        # the reference passes no half=, yolo_multi_model.py:41).  Default: as the detector.
        self.reid_half = half if reid_half is None else bool(reid_half)
        self.reid_dtype = torch.float16 if self.reid_half else torch.float32
        # fp32 ReID: the crops cross HBM as BYTES (the rounded bilinear values; SS_DST_U8) and the fp32 stem applies /255, mean and std while
        # it stages them - the same floats, a quarter of the bytes (crops_u8=False: A/B switch, float crops)
        from . import fused32 as _f32
        self.crops_dtype = torch.uint8 if (not self.reid_half and crops_u8 and run_nets and _f32.ENABLED) else self.reid_dtype
        self.det_source, self.feat_source, self.run_nets = det_source, feat_source, run_nets
        self.RB = reid_batch
        if reid_batch > MAX_DETS:
            raise ValueError("reid_batch <= 128")
        # Only the first reid_batch detections of a frame are cropped and embedded: with OSNet features feeding the
        # tracker, NMS keeps at most that many (highest scores first), so no detection reaches it without a feature.
        self.max_det = min(self.dcfg.max_det, MAX_DETS, reid_batch if (feat_source == "reid" and run_nets and self.need_reid) else MAX_DETS)
        # detect_only_rows > 0: a detection-only pipeline (model.predict, yolo_multi_model.py:173) whose NMS keeps up to
        # that many rows (<= 1024, the reference's max_det is 1000) — it never feeds the tracker (128 detections per frame)
        self.det_rows = MAX_DETS
        if detect_only_rows:
            self.det_rows = min(int(detect_only_rows), 1024)
            self.max_det = min(self.dcfg.max_det, self.det_rows)
        self.geom = letterbox_geometry(self.H, self.W, self.dcfg.imgsz, self.dcfg.stride)
        self.gain, self.pad_x, self.pad_y = scale_geometry(self.geom, self.H, self.W)
        # in_geom: the detector's input.  Sliced: the canvas every tile is letterboxed into; self.geom / gain / pad stay the whole frame's
        # (the merged rows' keypoints are expressed in it, as an unsliced pipeline's are)
        self.in_geom, self.T = self.geom, 1
        if self.slice is not None:
            from . import slicing
            try:
                self.in_geom, self.tile_table = slicing.canvas(self.H, self.W, self.slice, self.dcfg.imgsz, self.dcfg.stride)
            except ValueError:
                self.eng.close()
                raise
            self.T = len(self.tile_table)
            self.tile_rows = slicing.rows_per_tile(self.det_rows, self.T)
        self.detector = self.reid = None
        if run_nets:
            self.detector = nets.build_detector(detector, seed).to(dev, self.dtype).to(memory_format=torch.channels_last)
            if self.need_reid:
                self.reid = nets.build_reid(seed + 1).to(dev, self.reid_dtype).to(memory_format=torch.channels_last)
            self.nc, self.nk = self.detector.nc, self.detector.nk
            self.nm = getattr(self.detector, "nm", 0)           # mask coefficients of a segmentation head (after the keypoints' place)
            if self.native:
                self.detector.detect.register_forward_pre_hook(self._take_head_inputs)
        else:
            self.nc, self.nk, self.nm = 15 if self.ne else 80, 0, 0
        self.nx = 5 if self.ne else self.nk + self.nm           # extra columns NMS carries along with every kept row (OBB: cx, cy, w, h, theta)
        try:
            check_pose(self.byte_cfg, self.nk)
            if self.slice is not None and self.nm:
                raise ValueError("sliced inference cannot run a segmentation model: a row's mask coefficients belong to its tile's prototypes")
        except ValueError:
            self.eng.close()                                    # (the tracker context exists already: do not leak it)
            raise
        g, S = self.in_geom, n_streams
        self.n_anchors = sum((g.out_h // s) * (g.out_w // s) for s in (8, 16, 32))
        # how the stage bodies below differ between this class and OverlappedPipeline, as data: one frame per buffer set,
        # crops at one slot range per stream, net outputs not kept (OverlappedPipeline sets its own after this constructor)
        self.F, self.Sv, self.pack, self.keep_net_outputs = 1, S, False, False
        # N4 (optional): camera-motion warps (gmc_method) estimated beside the detector, applied by the tracker before predicting
        self.cmc = bool(cmc)
        # ---- static buffers (addresses are baked into the graph): ONE set, under the names callers fill and read ----
        b = self.b = _Bufs(self, S, self.det_rows, 1, self.cmc)
        for name in ("frames", "lb", "pred_in", "dets", "dets6", "proto", "keep", "ndets", "crops", "anchor_gt", "gt_feats", "warps"):
            setattr(self, name, getattr(b, name))
        self.feats_in = b.feats_v
        self.geom_dev = torch.tensor([[self.gain, self.pad_x, self.pad_y, float(self.W), float(self.H)]] * S,
                                     dtype=torch.float32, device=dev)      # per-image scale_boxes geometry for ss_nms_batch
        self.img_hw = torch.tensor([[self.H, self.W]] * S, dtype=torch.int32, device=dev)
        if self.slice is not None:
            self.eng.slice_config(self.tile_table, (self.H, self.W), (g.out_h, g.out_w), self.tile_rows, n_extra=self.nx, n_kpt=self.nk // 3,
                                  kpt_geom=(self.gain, self.pad_x, self.pad_y))
            self.tile_geom_dev = self.eng.slice_nms_geom(S)        # per-image geometry of the S * T tile images
        self.out, self.nout = self.eng.out, self.eng.nout
        self._maps = None                   # reid_model "auto": the head inputs of the detector call in flight
        self.graph = None
        self.graph_all = None
        self.graph_mode = graph
        if self.cmc:
            self.eng.estimate_warps(self.gmc_method, self.frames, 1, self.warps)   # sizes the estimator's buffers outside any capture
            self.reset_tracker(-1)
            self.trk.set_cmc(self.warps)

    # ---- stage bodies (b = a buffer set) ---------------------------------------------------------------
    # Every frame-side stage is ONE launch (set) over all virtual streams of the set, written straight in the NHWC layout the
    # convolutions read.  FramePipeline's detect | reid | track stages and OverlappedPipeline's stage lists are compositions of
    # these bodies; where the two classes launch differently, the condition is here (`grouped`, `pack`, `keep_net_outputs`).
    grouped = False                         # OverlappedPipeline: the buffer sets hold frame groups and cross graph boundaries

    def _letterbox(self, b):
        if self.cmc:                                           # the group's F warps, beside the detector (stateless stage)
            self.eng.estimate_warps(self.gmc_method, b.frames, self.F, b.warps, n_valid=b.nvalid)    # a partial group: the last REAL frame becomes "previous"
        if self.run_nets and self.slice is not None:           # every tile of every frame of the set, one launch
            self.eng.slice_letterbox_batch(b.frames, half=self.half, pad_value=self.dcfg.pad_value, out=b.lb, channels_last=True)
        elif self.run_nets:
            self.eng.letterbox_batch(b.frames, self.geom, half=self.half, pad_value=self.dcfg.pad_value, out=b.lb,
                                     channels_last=True)

    @staticmethod
    def _keep(b, name, tensors):
        """Stage outputs that cross a graph boundary live in per-set static buffers."""
        cur = getattr(b, name, None)
        if cur is None:
            cur = [torch.empty_like(t) for t in tensors]
            setattr(b, name, cur)
        for d, t in zip(cur, tensors):
            d.copy_(t)

    def _s_backbone(self, b):
        if self.run_nets:
            self._letterbox(b)
            self._keep(b, "pyr", self.detector.forward_backbone(b.lb))

    def _s_head(self, b):
        self._forward(b, lambda: self.detector.forward_head(*b.pyr))

    def _s_detector(self, b):
        if self.run_nets:
            self._letterbox(b)
            self._forward(b, lambda: self.detector(b.lb))
        elif self.cmc and not self.grouped:                    # FramePipeline estimates the warps without the networks too
            self._letterbox(b)

    def _forward(self, b, head):
        """The detector call that ends in the head, and what follows it: [Sv, 4+nc+nk+nm, A] into the NMS input."""
        with self._decode_into(b.pred_in):
            pred = self._pred(head(), b.proto)
        if self.native:
            # reid_model "auto": the head inputs stay referenced by the buffer set until the NMS body's launch reads them.  No
            # copy across a stage boundary (as b.mid in _reid_a): the maps live in this graph's private pool, keep their addresses
            # over replays, and the NMS stage's graph (captured after this one, for the same buffer set) reads them there.
            b.maps, self._maps = self._maps, None
        if self.keep_net_outputs:
            b.head_out = pred
        if self.det_source == "detector" and pred.data_ptr() != b.pred_in.data_ptr():
            b.pred_in.copy_(pred)

    def _nms(self, b):
        e = self.eng
        if self.slice is not None:
            # the tiles' NMS on S * T images (rows in tile pixels), then the merge: b.dets / b.ndets as an unsliced NMS leaves them,
            # b.keep = the kept rows' source indices (tile * tile_rows + row) where an unsliced pipeline has anchors
            sc = self.slice
            e.nms_batch(b.pred_in, self.nc, self.dcfg, self.tile_geom_dev, n_extra=self.nx, rows=b.tile_dets, keep=b.tile_keep,
                        count=b.tile_ndets, max_det=min(self.max_det, self.tile_rows))
            e.slice_merge(b.tile_dets.view(-1, self.T, self.tile_rows, 6 + self.nx), b.tile_ndets.view(-1, self.T), sc.merge, sc.metric, sc.thr,
                          self.dcfg.agnostic_nms, self.max_det, out=b.dets, count=b.ndets, src=b.keep)
        elif self.ne:                       # rotated NMS on ProbIoU: rows = envelope, conf, cls, cx, cy, w, h, theta
            e.nms_obb_batch(b.pred_in, self.nc, self.dcfg, self.geom_dev, rows=b.dets, keep=b.keep, count=b.ndets, max_det=self.max_det)
        else:
            e.nms_batch(b.pred_in, self.nc, self.dcfg, self.geom_dev, n_extra=self.nx, rows=b.dets, keep=b.keep,
                        count=b.ndets, max_det=self.max_det)
        if self.nx and not self.ne:         # (the OBB tracker call reads the 11-column rows themselves)
            b.dets6.copy_(b.dets[:, :, :6])
        if self.native and self.run_nets and self.feat_source == "reid":
            e.native_feats(b.maps, b.keep, b.ndets, b.feats_v)
        if not self.grouped:
            b.maps = None                   # FramePipeline: detector and NMS are one stage, the maps are let go once the launch is enqueued

    def _crops(self, b):
        if self.run_nets and self.reid is not None:
            if self.pack:        # the group's valid crops contiguous; the ReID kernels skip the rest of the fixed-size batch
                self.eng.crop_norm_packed(b.frames, b.dets6, self.RB, b.ndets, b.crop_off, b.crops, half=self.reid_half)
            else:
                self.eng.crop_norm_batch(b.frames, b.dets6, self.RB, counts=b.ndets, half=self.reid_half, out=b.crops, channels_last=True)

    def _valid(self, b):
        from . import fused, fused32
        if not self.reid_half:                               # fp32 kernels take the count as a launch argument
            return fused32.valid_images(b.crop_off[self.Sv:] if self.pack else None)
        return fused.valid_images(b.crop_off[self.Sv:] if self.pack else None, self.Sv * self.RB)

    def _select(self, b, emb):
        if emb is not None and self.keep_net_outputs:
            b.emb_out = emb
        if emb is not None and self.feat_source == "reid":
            if self.pack:
                self.eng.unpack_feats(emb.contiguous(), b.crop_off, b.ndets, self.RB, b.feats_v)
            else:
                b.feats_v[:, :self.RB].copy_(emb.view(self.Sv, self.RB, FEAT_DIM))
        if self.feat_source == "by_anchor":
            idx = b.anchor_gt.gather(1, b.keep.long().clamp_(0, self.n_anchors - 1))
            torch.gather(b.gt_feats, 1, idx.clamp_(min=0).unsqueeze(-1).expand(-1, -1, FEAT_DIM), out=b.feats_v)

    def _s_reid_select(self, b):
        """Crops, the whole OSNet, feature select."""
        if not (self.grouped or self.need_reid or self.native):
            return                          # FramePipeline without ReID: no stage at all (not even the by_anchor gather)
        self._crops(b)
        emb = None
        if self.run_nets and self.reid is not None:
            with self._valid(b):
                emb = self.reid(b.crops)                        # [Sv*RB, 512]
        self._select(b, emb)

    # ---- one frame for every stream, from the one buffer set --------------------------------------------
    def _detect(self):
        self._s_detector(self.b)
        self._nms(self.b)

    def _take_head_inputs(self, module, args):
        """Forward pre-hook on detector.detect (reid_model "auto"): its input list [P3, P4, P5], as Ultralytics' hook keeps it."""
        self._maps = list(args[0])

    def _decode_into(self, buf):
        """The head's decode launch writes the NMS input in place (fused.decode_into) when the detector feeds the NMS."""
        import contextlib
        from . import fused
        return fused.decode_into(buf) if self.det_source == "detector" else contextlib.nullcontext()

    @staticmethod
    def _pred(out, proto_dst):
        """Detector output -> the row tensor; a segmentation head's prototypes go to their static buffer."""
        if isinstance(out, tuple):
            out, proto = out
            proto_dst.copy_(proto)
        return out

    def _reid(self):
        self._s_reid_select(self.b)

    def _track(self):
        b = self.b
        self.trk.update_device(b.dets if self.ne else b.dets6, b.ndets, b.feats_v, self.img_hw, out=self.out, nout=self.nout,
                               **self._pose_kw(b, 0, self.Sv))
        if self.bank is not None:
            self.bank.update_group_device(self.out, self.nout, b.feats_v, 1)

    def _pose_kw(self, b, v0, v1):
        """with_pose: the NMS rows of virtual streams [v0, v1) as the tracker call's keypoints (their columns from 6, network-input
        pixels, and the images' NMS geometry)."""
        if self.byte is None or not self.byte.pose:
            return {}
        return dict(kpts=b.dets[v0:v1], kpt_col=6, geom=self.geom_dev[v0:v1])

    def reset_tracker(self, stream: int = -1):
        """Restart the tracker of one stream (all: -1), whichever family runs."""
        self.eng.reset(stream)
        if self.byte is not None:
            self.byte.reset(stream)
        if self.bank is not None:
            self.bank.reset(stream)

    def _warm_and_capture(self, warm, captures, tracks: bool = True):
        """Warm `warm` (callables) up on a side stream (MIOpen find, allocator), three eager passes, then capture one HIP graph per
        entry of `captures` (each a list of callables) there.  tracks: the warm-up frames must not count, the tracker is reset
        before the capture and after it (streams start fresh)."""
        st = torch.cuda.Stream(self.dev)
        st.wait_stream(torch.cuda.current_stream(self.dev))
        graphs = []
        with torch.cuda.stream(st):
            self.eng.use_current_stream()
            for _ in range(3):
                for fn in warm:
                    fn()
            st.synchronize()
            if tracks:
                self._restore_tracker()
            for fns in captures:
                gph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gph, stream=st):
                    for fn in fns:
                        fn()
                graphs.append(gph)
        torch.cuda.current_stream(self.dev).wait_stream(st)
        self.eng.use_current_stream()
        if tracks:
            self._restore_tracker()
        return graphs

    @torch.no_grad()
    def step(self, track: bool = True):
        """Run one frame (all streams).  Asynchronous; results in self.out / self.nout (device).
        track=False (graph "none" / "split" only skip the work): detection only — letterbox, detector, NMS."""
        if self.det_rows != MAX_DETS:
            if track:
                raise RuntimeError("a detect_only_rows pipeline cannot track")
            if self.graph_mode != "none":
                if self.graph is None:                       # one graph: letterbox, detector, NMS
                    self.graph, = self._warm_and_capture([self._detect], [[self._detect]], tracks=False)
                self.graph.replay()
                return
        whole = [self._detect, self._reid, self._track]
        if self.graph_mode == "none":
            for fn in (whole if track else whole[:1]):
                fn()
            return
        if self.graph is None:
            if self.graph_mode == "split":
                # three graphs on the same static buffers: detection | ReID | tracker, so a detection-only call
                # (model.predict, yolo_multi_model.py:173) replays just the first
                # ... and the three stages once more as ONE graph for the tracking call (model.track, yolo_multi_model.py:41 / :278: the
                # only call the reference makes per frame): one replay instead of three, no launch boundary between the stages
                stages = whole if self.need_reid else [self._detect, self._track]
                *self.graph, self.graph_all = self._warm_and_capture(whole, [[fn] for fn in stages] + [whole])
            else:
                self.graph, = self._warm_and_capture(whole, [whole if self.graph_mode == "all" else whole[:2]])
        if self.graph_mode == "split":
            (self.graph_all if track else self.graph[0]).replay()
            return
        self.graph.replay()
        if self.graph_mode == "front":
            self._track()

    # the warm-up iterations must not advance the tracker: reset it (callers start streams fresh)
    def _restore_tracker(self):
        torch.cuda.synchronize(self.dev)
        self.reset_tracker(-1)

    # ---- convenience ----------------------------------------------------------------------------------
    def results(self):
        """Synchronise and return per-stream rows (numpy [M,8])."""
        torch.cuda.synchronize(self.dev)
        self.eng.check_errors()
        out, n = self.out.cpu().numpy(), self.nout.cpu().numpy()
        return [out[s, :n[s]].copy() for s in range(self.S)]

    def detections(self):
        torch.cuda.synchronize(self.dev)
        d, n = self.dets.cpu().numpy(), self.ndets.cpu().numpy()
        return [d[s, :n[s]].copy() for s in range(self.S)]

    def close(self):
        torch.cuda.synchronize(self.dev)
        self.graph = None
        self.graph_all = None
        self.eng.close()


class _Bufs:
    """One set of per-frame buffers (static addresses, baked into that set's HIP graphs): S virtual streams, `rows` detection rows
    each, F frames per group; cmc: the group's camera-motion warps.  group: a frame group of OverlappedPipeline, which also
    carries the packed ReID batch's offsets and the count of its real frames."""

    def __init__(self, p: "FramePipeline", S: int, rows: int = MAX_DETS, F: int = 1, cmc: bool = False, group: bool = False):
        dev, g = p.dev, p.in_geom
        ST = S * p.T                        # images the detector sees: sliced, T tiles of every frame (tile-side buffers, leading dimension S * T)
        self.frames = torch.zeros(S, p.H, p.W, 3, dtype=torch.uint8, device=dev)
        self.lb = torch.zeros(ST, 3, g.out_h, g.out_w, dtype=p.dtype, device=dev).contiguous(memory_format=torch.channels_last)
        self.pred_in = torch.zeros(ST, 4 + p.nc + (p.ne or p.nx), p.n_anchors, dtype=torch.float32, device=dev)
        if p.slice is not None:             # the tiles' NMS rows, anchors and counts, which the merge reads
            self.tile_dets = torch.zeros(ST, p.tile_rows, 6 + p.nx, dtype=torch.float32, device=dev)
            self.tile_keep = torch.zeros(ST, p.tile_rows, dtype=torch.int32, device=dev)
            self.tile_ndets = torch.zeros(ST, dtype=torch.int32, device=dev)
        self.dets = torch.zeros(S, rows, 6 + p.nx, dtype=torch.float32, device=dev)
        self.dets6 = self.dets if p.nx == 0 else torch.zeros(S, rows, 6, dtype=torch.float32, device=dev)
        # segmentation: the frame's mask prototypes [nm, out_h/4, out_w/4] stay here until the caller has built its Results
        self.proto = torch.zeros(S, p.nm, g.out_h // 4, g.out_w // 4, dtype=p.dtype, device=dev) if p.nm else None
        self.keep = torch.zeros(S, rows, dtype=torch.int32, device=dev)
        self.ndets = torch.zeros(S, dtype=torch.int32, device=dev)
        self.crops = torch.zeros(S * p.RB if p.need_reid else 0, 3, 256, 128, dtype=p.crops_dtype,
                                 device=dev).contiguous(memory_format=torch.channels_last)
        self.anchor_gt = torch.zeros(S, p.n_anchors, dtype=torch.int64, device=dev)
        self.gt_feats = torch.zeros(S, MAX_DETS, FEAT_DIM, dtype=torch.float32, device=dev)
        self.feats_v = torch.zeros(S, MAX_DETS, FEAT_DIM, dtype=torch.float32, device=dev)    # what the tracker reads (FramePipeline.feats_in)
        self.warps = torch.zeros(F, p.S, 8, dtype=torch.float64, device=dev) if cmc else None
        self.maps = None                    # reid_model "auto": the detector's head inputs, between the head and the NMS body
        self.crop_off = self.nvalid = None
        if group:
            self.crop_off = torch.zeros(S + 1, dtype=torch.int32, device=dev)                 # packed ReID batch: first crop of every image, total
            self.nvalid = torch.full((1,), F, dtype=torch.int32, device=dev)                  # real frames of the group in this set (device side: read by captured kernels)


class OverlappedPipeline(FramePipeline):
    """Software pipeline over the frames of the same streams: stage j of frame k-j runs concurrently with the
    other stages on its own HIP stream,

        stage 0  letterbox -> detector backbone                                frame k
        stage 1  detector neck + head (-> head tensor)                         frame k-1
        stage 2  NMS -> ReID crops -> OSNet (first half)                       frame k-2
        stage 3  OSNet (second half) -> feature select -> StrongSORT update    frame k-3

    (stages 0/1 and 2/3 merge when the network has no split entry points, or with `n_stages=2`).  The
    detector and OSNet are stateless, so only the last stage carries the tracker recurrence, and it sees the
    frames strictly in order.  Results are identical to FramePipeline (same kernels, same order per frame);
    a frame still takes the sum of the stage times to come out, but throughput approaches the longest stage
    because the GPU is otherwise idle between the ~4 us launches of these batch-1 networks.  Every stage of
    every buffer set is one captured HIP graph; buffer sets = stages.  Measured at configs[1] on MI355X: 1 stage
    427, 2 stages 761, 4 stages 659 frames/s (four concurrent launch chains contend in the dispatcher), so the
    default is 2: [letterbox, detector] | [NMS, crops, OSNet, select, tracker]; `reid_split=k` moves the cut to
    after part k of the ReID backbone ([letterbox, detector, NMS, crops, OSNet parts <k] | [rest, tracker]) so
    the two streams carry equal work when frames are batched.
    """

    def __init__(self, *a, n_stages: int = 2, frame_batch: int = 1, reid_split: Optional[int] = None,
                 tracker_stream: bool = False, defer_track: bool = False, keep_net_outputs: bool = False, pack_crops: bool = True,
                 assoc_gate: bool = True, track_priority: bool = False, skip_tracker: bool = False, chain_cus: int = 0, **kw):
        kw = dict(kw)
        kw["graph"] = kw.get("graph", "front")
        if kw["graph"] == "none":
            raise ValueError("OverlappedPipeline needs graph='front' or 'all'")
        super().__init__(*a, **kw)
        # keep_net_outputs: every buffer set keeps a reference to the head tensor and the embeddings its graphs produce
        # (b.head_out / b.emb_out: tensors of the graph's private pool, same address at every replay) even when the synthetic
        # workload does not consume them — bench.py compares them with an eager re-run after the timed region
        self.keep_net_outputs = bool(keep_net_outputs)
        self.skip_tracker = bool(skip_tracker)      # MEASUREMENT ONLY: no tracker calls (rows stay empty) — what the stateless stages alone cost
        # frame batching: F consecutive frames of every stream travel through the stateless stages together as
        # S*F "virtual streams" (index f*S + s); the tracker then consumes them one frame at a time, in order.
        self.F = int(frame_batch)
        if self.F < 1:
            raise ValueError("frame_batch >= 1")
        if self.F > 1:
            self.graph_mode = "front"       # the per-frame tracker calls stay eager (partial last groups)
        self.Sv = self.S * self.F
        # packed ReID batches: the group's valid crops contiguous, the OSNet kernels skip the unused slots of the fixed batch
        # (~28 of 32 slots per frame are used at configs[1]); pack_crops=False: A/B switch
        self.pack = bool(self.run_nets and pack_crops and self.need_reid)
        if self.byte is not None:                # BYTE: no association launch to gate on; without ReID no ReID stage to cut or balance
            assoc_gate = False
            if not self.need_reid:
                reid_split = None
        self.geom_dev = self.geom_dev[:1].repeat(self.Sv, 1).contiguous()
        if self.slice is not None:
            self.tile_geom_dev = self.eng.slice_nms_geom(self.Sv)
        self.outs = torch.zeros(self.F, self.S, MAX_TRACKS, 8, dtype=torch.float32, device=self.dev)
        self.nouts = torch.zeros(self.F, self.S, dtype=torch.int32, device=self.dev)
        self.rboxs = torch.zeros(self.F, self.S, MAX_TRACKS, 5, dtype=torch.float32, device=self.dev) if self.ne else None   # OBB: the rows' cx, cy, w, h, theta
        split_det = self.run_nets and n_stages >= 4 and hasattr(self.detector, "forward_backbone")
        split_reid = self.run_nets and n_stages >= 4 and self.reid is not None and hasattr(self.reid, "forward_a")
        # two stages can also be cut INSIDE the ReID network to balance them: stage 0 = letterbox, detector, NMS,
        # crops and OSNet parts [0, reid_split); stage 1 = the remaining parts, feature select and the tracker
        self.reid_split = None
        if reid_split is not None and n_stages == 2:
            self.reid_split = int(reid_split) if (self.run_nets and hasattr(self.reid, "N_PARTS")) else 0
            if not 0 <= self.reid_split <= getattr(self.reid, "N_PARTS", 0):
                raise ValueError("reid_split out of range")
        # every stage is a list of the stage bodies, run in order on the frame group's buffer set
        if self.reid_split is not None:
            st = [[self._s_detector, self._nms, self._crops, self._reid_a], [self._reid_b]]
        else:
            st = [[self._s_backbone], [self._s_head]] if split_det else [[self._s_detector]]
            st += [[self._nms, self._crops, self._reid_a], [self._reid_b]] if split_reid else [[self._nms, self._s_reid_select]]
        self.stages = st
        self.n = len(st)
        # track_priority=True gives the last stage's stream (the tracker's short dependent launches, the association kernel) high
        # priority.  OFF by default since round 6: with the association launch alone on the chip (assoc_gate) the first two pipelines
        # of a process run the same with and without it (13 700 / 8 900 frames/s, f16 / fp32 ReID), and from the THIRD pipeline a process
        # creates on, the high-priority stream makes things worse — the tracker call takes 0.9-3.1 ms instead of 1.4-1.6 and the step
        # 3.3-3.8 ms instead of 2.3 (f16), 4.4-5.0 instead of 3.6 (fp32): tools/pipeline_reuse.py.  (An application re-creates its
        # pipeline whenever `model.overrides` change; bench.py's side legs did.)
        hi = bool(track_priority)
        # chain_cus = n > 0: the tracker's per-frame chain (one- to 64-workgroup kernels, ~27 us a frame, strictly dependent) is
        # detached onto a library stream that owns n compute units (n / 8 per XCD), every stream of this pipeline is created without
        # them, and the rows are fetched on a results stream that waits for the chain: the chain then runs beside the networks
        # instead of between their kernels in the dispatcher.  (CU-masked streams have no priority: track_priority does not apply.)
        # chain_cus = -1: detached onto a plain high-priority stream, nothing reserved.
        self.chain_cus = int(chain_cus)
        if self.chain_cus and tracker_stream:
            # the tracker-stream branch releases a buffer set on that stream, not behind the detached chain's results stream: the
            # chain could still be reading the set's detections / features when stage 0 refills it
            self.eng.close()                                     # (the tracker context exists already: do not leak it)
            raise ValueError("tracker_stream and chain_cus cannot be combined")
        if self.chain_cus:
            self.eng.set_option("chain_cus", self.chain_cus)
        if self.chain_cus > 0:
            self.streams = [self.eng.create_stream(self.chain_cus) for _ in range(self.n)]
        else:
            self.streams = [torch.cuda.Stream(self.dev, priority=(-1 if (hi and j == self.n - 1) else 0)) for j in range(self.n)]
        self.sR = torch.cuda.Stream(self.dev) if self.chain_cus else None      # result copies / buffer-set release of a detached chain
        self._res_ev = None
        # tracker_stream=True gives the tracker (one-workgroup kernels, ~70 us a frame) a stream of its own next to the
        # last stage of the following group, with one more buffer set so that stage 0 does not wait for it.  Measured
        # at configs[1], same box, frame batch 8: 3110 frames/s with it vs 3280 without — a third concurrent launch
        # chain costs more in the dispatcher than the queue stall it removes (same finding as the 4-stage split) — so
        # it is off by default.
        self.sT = torch.cuda.Stream(self.dev, priority=-1 if hi else 0) if (tracker_stream and self.graph_mode == "front") else None
        # defer_track: the tracker call of group k is enqueued on the last stage's stream AFTER that stream has waited for
        # stage 0 of group k+1 — it then runs beside the START of the other stream's next group (letterbox, the detector's
        # short-lived workgroups) instead of beside whatever that stream happens to be in.  The association kernel needs
        # whole CUs' worth of registers at once; beside the OSNet row-stream kernel (waves that live ~100-200 us and own the
        # register file) its launch took 50-83 us instead of 30.  Results arrive one group later; one more buffer set.
        self.defer = bool(defer_track) and self.sT is None and self.graph_mode == "front"
        self._pending_track = None
        # ... and stage 0 of the next group waits for that call's association launch (not for the per-frame chain after it):
        # for ~40 us the association kernel has the chip to itself (alone: 39.8 us for 32 frames, beside the detector's first
        # layers: 61-65 us)
        self.assoc_ev = None
        if self.defer and assoc_gate:
            self.assoc_ev = torch.cuda.Event()
            self.assoc_ev.record(torch.cuda.current_stream(self.dev))
            self.eng.set_assoc_event(self.assoc_ev)
        self._gate = False
        self.nb = self.n + (1 if (self.sT is not None or self.defer) else 0)              # buffer sets
        self.bufs = [_Bufs(self, self.Sv, MAX_DETS, self.F, self.cmc, group=True) for _ in range(self.nb)]
        self.ev = [[torch.cuda.Event() for _ in range(self.nb)] for _ in range(self.n)]   # ev[stage][set]
        self.ev_graph = [torch.cuda.Event() for _ in range(self.nb)]                      # last stage's graph done (tracker may start)
        self.graphs = [[None] * self.nb for _ in range(self.n)]                           # graphs[stage][set]
        self.sA = self.streams[0]                                  # first stage's stream
        # input stream: the caller fills a buffer set's inputs here (`with torch.cuda.stream(pipe.s_in)`).  Its own stream, so
        # that the copies of group k+1 run as soon as their buffer set is free — beside the networks' kernels of the groups in
        # flight — instead of at the head of stage 0's stream, which is exactly when the deferred tracker call of an older group
        # launches its association kernel (the copies' blit kernels and k_assoc then share the chip: on some boxes / runs the
        # association launch took 86 us instead of 38).  Filling on `sA` stays correct (it is ordered before stage 0).
        self.s_in = self.eng.create_stream(self.chain_cus) if self.chain_cus > 0 else torch.cuda.Stream(self.dev)
        self.ev_in = [torch.cuda.Event() for _ in range(self.nb)]
        self.sB = self.sT if self.sT is not None else self.streams[-1]                    # tracker + result stream
        self.k = 0                          # groups (of frame_batch frames) submitted
        self.stage_done = [0] * self.n      # groups enqueued per stage
        self.valid = [self.F] * self.nb     # real frames in the group occupying each buffer set
        self.base = [0] * self.nb           # frame index of the first frame of that group
        self.frames_in = 0
        self._captured = False

    grouped = True

    # ---- the ReID network cut in two (b = the frame group's buffer set) ----------------------------------
    def _reid_a(self, b):
        """OSNet up to the cut: the network's own (four stages, reid_split None) or before part reid_split."""
        if self.reid_split is None:
            with self._valid(b):
                st = self.reid.forward_a(b.crops)                # a tensor or a tuple of tensors (nets.OSNet._block_part)
            b.mid_tuple = isinstance(st, tuple)
            self._keep(b, "mid", list(st) if b.mid_tuple else [st])
        elif self.run_nets and self.reid_split > 0:
            # no copy across the stage boundary: the tensor lives in this graph's private pool, keeps its address over
            # replays, and the next stage's graph (captured after this one, for the same buffer set) reads it there
            with self._valid(b):
                b.mid = [self.reid.forward_a(b.crops, self.reid_split)]

    def _reid_b(self, b):
        """The rest of OSNet, feature select."""
        emb = None
        if self.reid_split is None:
            with self._valid(b):
                emb = self.reid.forward_b(tuple(b.mid) if b.mid_tuple else b.mid[0])
        elif self.run_nets:
            with self._valid(b):
                emb = self.reid.forward_b(b.mid[0] if self.reid_split > 0 else b.crops, self.reid_split)
        self._select(b, emb)

    def _track_b(self, b: _Bufs, n_valid: int = None, group: int = None):
        """Tracker update of the group's frames in ONE call: the library associates them strictly in order (frame f =
        virtual streams f*S..) and reads the galleries once for all of them; `group` = index of the group's first
        frame (None while warming up / capturing: no callbacks)."""
        e = self.trk
        nv = self.F if n_valid is None else n_valid
        G, S = self.eng.max_group_frames, self.S             # frames per library call (SS_FMAX)
        if self.sR is not None and self._res_ev is not None:
            torch.cuda.current_stream(self.dev).wait_event(self._res_ev)     # the previous group's rows have left self.outs
        for f0 in range(0, nv if not self.skip_tracker else 0, G):
            n, v0, v1 = min(G, nv - f0), f0 * S, min(nv, f0 + G) * S
            if self.cmc:
                e.set_cmc(b.warps[f0:f0 + n])
            if self.ne:
                e.update_group(n, b.dets[v0:v1], b.ndets[v0:v1], None, self.img_hw, self.outs[f0:f0 + n], self.nouts[f0:f0 + n],
                               rbox=self.rboxs[f0:f0 + n])
                continue
            e.update_group(n, b.dets6[v0:v1], b.ndets[v0:v1], b.feats_v[v0:v1], self.img_hw, self.outs[f0:f0 + n], self.nouts[f0:f0 + n],
                           **self._pose_kw(b, v0, v1))
            if self.bank is not None:                           # the same slices, behind the rows (the library joins a detached chain first)
                self.bank.update_group_device(self.outs[f0:f0 + n], self.nouts[f0:f0 + n], b.feats_v[v0:v1], n)
        if self.sR is not None:                                 # detached chain: the rows exist once the chain's stream is done
            self.eng.track_join(self.sR)
            if self.bank is not None:                           # the set is released on sR: not before the bank has read its features
                self.sR.wait_stream(torch.cuda.current_stream(self.dev))
        if group is not None and self.on_result is not None:
            self.cur_bufs, self.cur_valid = b, nv               # the buffer set / real-frame count the callbacks below refer to
            with torch.cuda.stream(self.sR if self.sR is not None else torch.cuda.current_stream(self.dev)):
                for f in range(nv):
                    self.on_result(group + f, f)       # e.g. enqueue the D2H copy of self.outs[f] on this stream

    @torch.no_grad()
    def _capture(self):
        cur = torch.cuda.current_stream(self.dev)
        for st in self.streams:
            st.wait_stream(cur)
        last = self.n - 1
        for i, b in enumerate(self.bufs):                       # eager warm-up in stage order (MIOpen find, allocator)
            for j, bodies in enumerate(self.stages):
                with torch.cuda.stream(self.streams[j]):
                    self.eng.use_stream(self.streams[j])
                    for _ in range(2):
                        for fn in bodies:
                            fn(b)
                        if j == last:
                            self._track_b(b)
                self.streams[j].synchronize()
        for i, b in enumerate(self.bufs):
            for j, bodies in enumerate(self.stages):
                with torch.cuda.stream(self.streams[j]):
                    self.eng.use_stream(self.streams[j])
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=self.streams[j]):
                        for fn in bodies:
                            fn(b)
                        if j == last and self.graph_mode == "all":
                            self._track_b(b)
                    self.graphs[j][i] = g
        torch.cuda.synchronize(self.dev)
        self.eng.use_stream(self.sB)                                 # the tracker lives on the last stage's stream
        self.reset_tracker(-1)
        self._captured = True

    # ---- driver API --------------------------------------------------------------------------------------
    on_result = None
    cur_bufs, cur_valid = None, 0

    def begin_frame(self) -> _Bufs:
        """Buffer set for the next frame.  Fill its inputs inside `with torch.cuda.stream(pipe.sA):`."""
        if not self._captured:
            self._capture()
        i = self.k % self.nb
        self.sA.wait_event(self.ev[self.n - 1][i])               # the group that used this set has left the tracker
        self.s_in.wait_event(self.ev[self.n - 1][i])
        return self.bufs[i]

    @torch.no_grad()
    def _run_stage(self, j: int, frame_idx: int):
        i = frame_idx % self.nb
        st = self.streams[j]
        with torch.cuda.stream(st):
            if j > 0:
                st.wait_event(self.ev[j - 1][i])
            if j == self.n - 1 and self.defer:
                self._flush_track(st)                            # the previous group's tracker call, now that stage 0 moved on
            self._mark(f"stage{j}_start", frame_idx, st)
            self.graphs[j][i].replay()
            self._mark(f"stage{j}_end", frame_idx, st)
            if j == self.n - 1 and self.defer:
                self._pending_track = i
            elif j == self.n - 1 and self.sT is not None:        # tracker of this group on its own stream
                self.ev_graph[i].record(st)
                with torch.cuda.stream(self.sT):
                    self.sT.wait_event(self.ev_graph[i])
                    self._track_b(self.bufs[i], self.valid[i], self.base[i])
                    self.ev[j][i].record(self.sT)
            else:
                if j == self.n - 1:
                    if self.graph_mode == "front":
                        self._track_b(self.bufs[i], self.valid[i], self.base[i])
                    elif self.on_result is not None:
                        self.on_result(self.base[i], 0)          # graph == "all" implies frame_batch == 1
                    self._mark_tracked(i, st)
                else:
                    self.ev[j][i].record(st)
        self.stage_done[j] = frame_idx + 1

    def _mark_tracked(self, i, st):
        """Buffer set i has left the tracker (its rows are fetched): on the results stream when the chain is detached."""
        ev = self.ev[self.n - 1][i]
        ev.record(self.sR if self.sR is not None else st)
        self._res_ev = ev

    trace = None                                                 # a list: (name, group, timing event) of every stage / tracker boundary (tools/overlap_timeline.py)

    def _mark(self, name, k, st):
        if self.trace is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(st)
            self.trace.append((name, k, ev))

    def _flush_track(self, st):
        i = self._pending_track
        if i is not None:
            self._pending_track = None
            self._mark("track_start", self.base[i], st)
            self._track_b(self.bufs[i], self.valid[i], self.base[i])
            self._mark("track_end", self.base[i], st)
            self._mark_tracked(i, st)
            self._gate = self.assoc_ev is not None

    def submit(self, n_valid: int = None):
        """Stage 0 of the group of frames just filled (n_valid <= frame_batch of them are real), and stage j of
        group k-j for every j that has one."""
        k = self.k
        nv = self.F if n_valid is None else int(n_valid)
        self.valid[k % self.nb] = nv
        self.base[k % self.nb] = self.frames_in                 # index of the group's first frame (partial groups allowed)
        self.frames_in += nv
        self.ev_in[k % self.nb].record(self.s_in)               # inputs filled on the input stream: stage 0 waits for them
        self.sA.wait_event(self.ev_in[k % self.nb])
        if self.cmc:
            with torch.cuda.stream(self.sA):
                self.bufs[k % self.nb].nvalid.fill_(nv)
        for j in (range(self.n - 1, -1, -1) if self.defer else range(self.n)):     # deferred: the tracker call is enqueued first
            f = k - j
            if f >= 0 and self.stage_done[j] == f:
                if j == 0 and self._gate:
                    self.sA.wait_event(self.assoc_ev)           # the association launch just enqueued on the other stream
                    self._gate = False
                self._run_stage(j, f)
        self.k += 1

    def flush(self):
        """Push every submitted frame through the remaining stages (results are then enqueued on stream sB)."""
        for j in range(1, self.n):
            while self.stage_done[j] < self.stage_done[j - 1]:
                self._run_stage(j, self.stage_done[j])
        if self.defer and self._pending_track is not None:
            with torch.cuda.stream(self.streams[self.n - 1]):
                self._flush_track(self.streams[self.n - 1])

    def step(self, track: bool = True):
        raise RuntimeError("use begin_frame()/submit()/flush() on an OverlappedPipeline")

    def close(self):
        torch.cuda.synchronize(self.dev)
        self.graphs = None                               # captured graphs reference the context's buffers: drop them first
        super().close()
