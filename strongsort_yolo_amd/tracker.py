"""StrongSORT.update(dets, frame) — the tracker seam BASELINE.json's north_star names.

Stands behind the tracker callback inside `model.track(...)` (/root/reference/yolo_multi_model.py:41):
detections of one frame in, rows of confirmed tracks out.  All arithmetic runs in
libstrongsort_hip.so (crop-extract, feature normalise, Kalman, cost matrix, LSAP, bookkeeping) and in
the PyTorch-ROCm OSNet; there is no CPU fallback.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import nets
from .config import StrongSortConfig, ByteTrackConfig, OCSortConfig, DeepOCSortConfig, HybridSortConfig, check_reid_model, check_gmc_method
from .engine import TrackerEngine, ByteTrackEngine, OCSortEngine, DeepOCSortEngine, HybridSortEngine
from .lib import MAX_DETS, FEAT_DIM


class StrongSORT:
    """One video stream.  `update(dets, frame)`:
         dets  [N,6] float  x1,y1,x2,y2,conf,cls in frame pixels (numpy or torch)
         frame uint8 [H,W,3] BGR (numpy, or a torch tensor already on the device)
       returns float32 [M,8]: x1,y1,x2,y2,track_id,class_id,conf,det_idx for every confirmed track seen
       within the last frame (det_idx = row of `dets` matched this frame, -1 while coasting)."""

    def __init__(self, model_weights: Optional[str] = None, device: int = 0, fp16: bool = True,
                 max_dist: float = 0.2, max_iou_distance: float = 0.7, max_age: int = 30, n_init: int = 3,
                 nn_budget: int = 100, mc_lambda: float = 0.995, ema_alpha: float = 0.9, reid_seed: int = 1,
                 random_init_ok: bool = False):
        self.cfg = StrongSortConfig(max_dist=max_dist, max_iou_distance=max_iou_distance, max_age=max_age,
                                    n_init=n_init, nn_budget=nn_budget, mc_lambda=mc_lambda, ema_alpha=ema_alpha)
        self.eng = TrackerEngine(self.cfg, 1, device)
        self.dev = self.eng.device
        self.dtype = torch.float16 if fp16 else torch.float32
        self.reid = nets.build_reid(reid_seed)
        nets.load_weights(self.reid, model_weights, "OSNet-x0.25 ReID", random_init_ok)
        self.reid = self.reid.to(self.dev, self.dtype).to(memory_format=torch.channels_last)
        self._dets = torch.zeros(1, MAX_DETS, 6, dtype=torch.float32, device=self.dev)
        self._feats = torch.zeros(1, MAX_DETS, FEAT_DIM, dtype=torch.float32, device=self.dev)
        self._n = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._hw = torch.zeros(1, 2, dtype=torch.int32, device=self.dev)

    @torch.no_grad()
    def update(self, dets, frame, features=None) -> np.ndarray:
        self.eng.use_current_stream()                    # launch on the caller's current torch stream
        dets = torch.as_tensor(dets, dtype=torch.float32).reshape(-1, 6)
        n = dets.shape[0]
        if n > MAX_DETS:
            raise ValueError(f"at most {MAX_DETS} detections per frame (got {n})")
        frame_t = frame if isinstance(frame, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frame))
        frame_t = frame_t.to(self.dev, non_blocking=True)
        H, W = int(frame_t.shape[0]), int(frame_t.shape[1])
        self._dets[0, :n].copy_(dets, non_blocking=True)
        self._n.fill_(n)
        self._hw.copy_(torch.tensor([[H, W]], dtype=torch.int32))
        if features is not None:
            self._feats[0, :n].copy_(torch.as_tensor(features, dtype=torch.float32).reshape(n, FEAT_DIM))
        elif n:
            crops = self.eng.crop_norm(frame_t, self._dets[0], n, half=self.dtype == torch.float16)
            self._feats[0, :n].copy_(self.reid(crops.contiguous(memory_format=torch.channels_last)))
        out, nout = self.eng.update_device(self._dets, self._n, self._feats, self._hw)
        torch.cuda.synchronize(self.dev)
        self.eng.check_errors()
        return out[0, : int(nout[0])].cpu().numpy()

    def reset(self):
        self.eng.reset(-1)

    def close(self):
        self.eng.close()


class BYTETracker:
    """The BYTE tracker family for one video stream (docs/BYTETRACK.md): `update(dets)` needs no ReID weights.
         dets  [N,6] float  x1,y1,x2,y2,conf,cls in frame pixels (numpy or torch), N <= 128
         frame uint8 [H,W,3] BGR (numpy, or a torch tensor on the device): only with camera_motion=True
       returns float32 [M,8]: x1,y1,x2,y2,track_id,class_id,conf,det_idx for every activated tracked track (det_idx = row of
       `dets` matched this frame, always >= 0).  cfg.kalman = "xyah": ByteTrack; "xywh": BoT-SORT without ReID.
       camera_motion=True (xywh only): BoT-SORT's GMC (§1b) with the ECC warp between the previous frame and this one,
       estimated on the device; `update(dets, frame)` then needs the frame.  gmc_method="sparseOptFlow": the sparse-optical-flow
       estimator (§1f, Ultralytics' botsort.yaml default) instead of ECC; frame sides >= 64.
       cfg.with_reid=True (xywh only): BoT-SORT's ReID branch (§1c).  `update(dets, frame, features)` takes the rows' raw
       features [N,k] (k <= 512, zero-padded to 512: the §1d features of a `model: auto` detector have k = min(C_l)), or cuts
       the crops from `frame` and runs OSNet-x0.25 (reid_weights, loaded as StrongSORT loads them; fp16 selects half
       activations) when `features` is None.  reid_model="auto" (§1d): no OSNet is built; update needs `features`.
       cfg.with_pose=True (xywh only, not with with_reid): the keypoint term (§1e).  `update(dets, keypoints=...)` takes the rows'
       keypoints [N,K,3] (x, y, visibility) in the same frame pixels as `dets`.
       obb=True (docs/OBB.md §4; not with camera_motion, with_reid or with_pose): oriented boxes, associated on ProbIoU.  `update(dets)`
       takes [N,7+] rows cx, cy, w, h, theta, conf, cls (taken as they are: not regularised) and returns float32 [M,13]: the eight
       columns above with the rotated box's axis-aligned envelope in front, then the track's cx, cy, w, h, theta."""

    def __init__(self, cfg: Optional[ByteTrackConfig] = None, device: int = 0, camera_motion: bool = False,
                 reid_weights: Optional[str] = None, fp16: bool = False, random_init_ok: bool = False, reid_seed: int = 1,
                 reid_model: str = "osnet", gmc_method: str = "ecc", obb: bool = False):
        self.cfg = cfg or ByteTrackConfig()
        self.obb = bool(obb)
        if self.obb and (camera_motion or self.cfg.with_reid or self.cfg.with_pose):
            raise ValueError("obb=True: oriented boxes are not combined with camera_motion, with_reid or with_pose (docs/OBB.md §4)")
        self.reid_model = check_reid_model(reid_model, self.cfg.with_reid, reid_weights)
        self.gmc_method = check_gmc_method(gmc_method, camera_motion, "botsort" if self.cfg.kalman == "xywh" else "bytetrack")
        if camera_motion and self.cfg.kalman != "xywh":
            raise ValueError("camera_motion needs the xywh (BoT-SORT) filter: ByteTrack has no GMC")
        self.eng = ByteTrackEngine(self.cfg, 1, device, obb=self.obb)
        self.dev = self.eng.device
        self.camera_motion = bool(camera_motion)
        self._dets11 = torch.zeros(1, MAX_DETS, 11, dtype=torch.float32, device=self.dev) if self.obb else None
        self.reid = None
        if self.cfg.with_reid:
            self.dtype = torch.float16 if fp16 else torch.float32
            self._feats = torch.zeros(1, MAX_DETS, FEAT_DIM, dtype=torch.float32, device=self.dev)
        if self.cfg.with_reid and self.reid_model == "osnet":
            self.reid = nets.build_reid(reid_seed)           # the same loading policy as StrongSORT's (raise unless random init is asked for)
            nets.load_weights(self.reid, reid_weights, "OSNet-x0.25 ReID", random_init_ok)
            self.reid = self.reid.to(self.dev, self.dtype).to(memory_format=torch.channels_last)
        self._dets = torch.zeros(1, MAX_DETS, 6, dtype=torch.float32, device=self.dev)
        self._n = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._kpts = torch.zeros(1, MAX_DETS, len(self.cfg.kpt_sigmas), 3, dtype=torch.float32, device=self.dev) if self.cfg.with_pose else None
        self._warps = torch.zeros(1, 1, 8, dtype=torch.float64, device=self.dev) if self.camera_motion else None

    @torch.no_grad()
    def update(self, dets, frame=None, features=None, keypoints=None) -> np.ndarray:
        self.eng.use_current_stream()
        if self.obb:
            return self._update_obb(dets)
        dets = torch.as_tensor(dets, dtype=torch.float32).reshape(-1, 6)
        n = dets.shape[0]
        if n > self.cfg.max_dets:
            raise ValueError(f"at most {self.cfg.max_dets} detections per frame (got {n})")
        frame_t = None
        if frame is not None and (self.camera_motion or (self.cfg.with_reid and features is None)):
            frame_t = frame if isinstance(frame, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frame))
            frame_t = frame_t.to(self.dev, non_blocking=True).contiguous()
        if self.camera_motion:
            if frame_t is None:
                raise ValueError("camera_motion=True: update(dets, frame) needs the BGR frame")
            self.eng.estimate_warps(self.gmc_method, frame_t[None], 1, self._warps)
            self.eng.set_cmc(self._warps)
        self._dets[0, :n].copy_(dets, non_blocking=True)
        self._n.fill_(n)
        feats = None
        if self.cfg.with_reid:
            feats = self._feats
            if features is not None:
                ft = torch.as_tensor(features, dtype=torch.float32)
                ft = ft.reshape(n, -1) if n else ft.reshape(0, ft.shape[-1] if ft.dim() else 0)
                k = ft.shape[1]
                if k > FEAT_DIM:
                    raise ValueError(f"features [N,k]: k <= {FEAT_DIM} (got {k})")
                self._feats[0, :n, :k].copy_(ft)
                self._feats[0, :n, k:].zero_()                          # §1d: a shorter vector is zero-padded to 512
            elif self.reid is None:
                raise ValueError("reid_model='auto': update(dets, frame, features) needs the rows' features [N,k]")
            elif frame_t is None:
                raise ValueError("with_reid: update(dets, frame) needs the BGR frame or features [N,512]")
            elif n:
                crops = self.eng.base.crop_norm(frame_t, self._dets[0], n, half=self.dtype == torch.float16)
                self._feats[0, :n].copy_(self.reid(crops.contiguous(memory_format=torch.channels_last)))
        elif features is not None:
            raise ValueError("features given, but cfg.with_reid is off")
        if self.cfg.with_pose:
            if keypoints is None:
                raise ValueError("with_pose: update(dets, keypoints=...) needs the rows' keypoints [N,K,3]")
            kp = torch.as_tensor(keypoints, dtype=torch.float32).reshape(-1, self._kpts.shape[2], 3)
            if kp.shape[0] != n:
                raise ValueError(f"keypoints [N,K,3]: one row per detection ({n}), got {kp.shape[0]}")
            self._kpts[0, :n].copy_(kp)
        elif keypoints is not None:
            raise ValueError("keypoints given, but cfg.with_pose is off")
        out, nout = self.eng.update_device(self._dets, self._n, feats, kpts=self._kpts)
        torch.cuda.synchronize(self.dev)
        self.eng.check_errors()
        return out[0, : int(nout[0])].cpu().numpy()

    def _update_obb(self, dets) -> np.ndarray:
        dets = torch.as_tensor(dets, dtype=torch.float32)
        dets = dets.reshape(-1, dets.shape[-1] if dets.dim() > 1 else 7)
        n = dets.shape[0]
        if dets.shape[1] < 7:
            raise ValueError("obb=True: dets [N,7+] = cx, cy, w, h, theta, conf, cls")
        if n > self.cfg.max_dets:
            raise ValueError(f"at most {self.cfg.max_dets} detections per frame (got {n})")
        rows = torch.zeros(n, 11, dtype=torch.float32)               # the tracker call reads conf, cls and the rotated box, not the envelope
        rows[:, 4:6], rows[:, 6:11] = dets[:, 5:7], dets[:, :5]
        self._dets11[0, :n].copy_(rows, non_blocking=True)
        self._n.fill_(n)
        out, nout = self.eng.update_device(self._dets11, self._n)
        torch.cuda.synchronize(self.dev)
        self.eng.check_errors()
        m = int(nout[0])
        return torch.cat([out[0, :m], self.eng.rbox[0, :m]], 1).cpu().numpy()

    def reset(self):
        self.eng.reset(-1)

    def close(self):
        self.eng.close()


class OCSORTTracker:
    """OC-SORT for one video stream (docs/OCSORT.md): `update(dets)` needs no weights and no frame.
         dets  [N,6] float  x1,y1,x2,y2,conf,cls in frame pixels (numpy or torch), N <= cfg.max_dets
       returns float32 [M,8]: x1,y1,x2,y2,track_id,class_id,conf,det_idx for every track matched this frame with
       hit_streak >= min_hits (or within the first min_hits frames), newest track first; the box is the matched row's
       (det_idx = its row in `dets`, always >= 0)."""

    def __init__(self, cfg: Optional[OCSortConfig] = None, device: int = 0):
        self.cfg = cfg or OCSortConfig()
        self.eng = OCSortEngine(self.cfg, 1, device)
        self.dev = self.eng.device
        self._dets = torch.zeros(1, MAX_DETS, 6, dtype=torch.float32, device=self.dev)
        self._n = torch.zeros(1, dtype=torch.int32, device=self.dev)

    @torch.no_grad()
    def update(self, dets, frame=None) -> np.ndarray:
        self.eng.use_current_stream()
        dets = torch.as_tensor(dets, dtype=torch.float32).reshape(-1, 6)
        n = dets.shape[0]
        if n > self.cfg.max_dets:
            raise ValueError(f"at most {self.cfg.max_dets} detections per frame (got {n})")
        self._dets[0, :n].copy_(dets, non_blocking=True)
        self._n.fill_(n)
        out, nout = self.eng.update_device(self._dets, self._n)
        torch.cuda.synchronize(self.dev)
        self.eng.check_errors()
        return out[0, : int(nout[0])].cpu().numpy()

    def reset(self):
        self.eng.reset(-1)

    def close(self):
        self.eng.close()


class HybridSORTTracker(OCSORTTracker):
    """Hybrid-SORT for one video stream (docs/HYBRIDSORT.md): `update(dets)` as OCSORTTracker.update, no weights and no frame."""

    def __init__(self, cfg: Optional[HybridSortConfig] = None, device: int = 0):
        self.cfg = cfg or HybridSortConfig()
        self.eng = HybridSortEngine(self.cfg, 1, device)
        self.dev = self.eng.device
        self._dets = torch.zeros(1, MAX_DETS, 6, dtype=torch.float32, device=self.dev)
        self._n = torch.zeros(1, dtype=torch.int32, device=self.dev)


class DeepOCSORTTracker:
    """Deep OC-SORT for one video stream (docs/DEEPOCSORT.md), shaped like ByteTracker with with_reid.
         dets     [N,6] float  x1,y1,x2,y2,conf,cls in frame pixels (numpy or torch), N <= cfg.max_dets
         frame    uint8 [H,W,3] BGR (numpy, or a torch tensor on the device): with camera_motion=True, and for the crops when
                  `features` is None
         features [N,k] raw features of the rows (k <= 512, zero-padded); None: the crops go through OSNet-x0.25 (reid_weights,
                  loaded as StrongSORT loads them; fp16 selects half activations)
       returns float32 [M,8] as OCSORTTracker.update.  camera_motion=True: step 1b with the warp between the previous frame and this
       one, estimated on the device (gmc_method "ecc" or "sparseOptFlow").  cfg.appearance=False: no network, no features."""

    def __init__(self, cfg: Optional[DeepOCSortConfig] = None, device: int = 0, camera_motion: bool = False,
                 reid_weights: Optional[str] = None, fp16: bool = False, random_init_ok: bool = False, gmc_method: str = "ecc",
                 reid_seed: int = 1):
        self.cfg = cfg or DeepOCSortConfig()
        self.gmc_method = check_gmc_method(gmc_method, camera_motion, "deep_ocsort")
        self.reid = None
        if self.cfg.appearance and (reid_weights or random_init_ok):
            self.reid = nets.build_reid(reid_seed)
            nets.load_weights(self.reid, reid_weights, "OSNet-x0.25 ReID", random_init_ok)
        self.eng = DeepOCSortEngine(self.cfg, 1, device)
        self.dev = self.eng.device
        self.camera_motion = bool(camera_motion)
        self.dtype = torch.float16 if fp16 else torch.float32
        if self.reid is not None:
            self.reid = self.reid.to(self.dev, self.dtype).to(memory_format=torch.channels_last)
        self._feats = torch.zeros(1, MAX_DETS, FEAT_DIM, dtype=torch.float32, device=self.dev) if self.cfg.appearance else None
        self._dets = torch.zeros(1, MAX_DETS, 6, dtype=torch.float32, device=self.dev)
        self._n = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._warps = torch.zeros(1, 1, 8, dtype=torch.float64, device=self.dev) if self.camera_motion else None

    @torch.no_grad()
    def update(self, dets, frame=None, features=None) -> np.ndarray:
        self.eng.use_current_stream()
        dets = torch.as_tensor(dets, dtype=torch.float32).reshape(-1, 6)
        n = dets.shape[0]
        if n > self.cfg.max_dets:
            raise ValueError(f"at most {self.cfg.max_dets} detections per frame (got {n})")
        frame_t = None
        if frame is not None and (self.camera_motion or (self.cfg.appearance and features is None)):
            frame_t = frame if isinstance(frame, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frame))
            frame_t = frame_t.to(self.dev, non_blocking=True).contiguous()
        if self.camera_motion:
            if frame_t is None:
                raise ValueError("camera_motion=True: update(dets, frame) needs the BGR frame")
            self.eng.estimate_warps(self.gmc_method, frame_t[None], 1, self._warps)
            self.eng.set_cmc(self._warps)
        self._dets[0, :n].copy_(dets, non_blocking=True)
        self._n.fill_(n)
        if not self.cfg.appearance:
            if features is not None:
                raise ValueError("features given, but cfg.appearance is off")
        elif features is not None:
            ft = torch.as_tensor(features, dtype=torch.float32)
            ft = ft.reshape(n, -1) if n else ft.reshape(0, ft.shape[-1] if ft.dim() else 0)
            k = ft.shape[1]
            if k > FEAT_DIM:
                raise ValueError(f"features [N,k]: k <= {FEAT_DIM} (got {k})")
            self._feats[0, :n, :k].copy_(ft)
            self._feats[0, :n, k:].zero_()
        elif self.reid is None:
            raise ValueError("no ReID network was loaded (reid_weights): update(dets, frame, features) needs the rows' features [N,k]")
        elif frame_t is None:
            raise ValueError("appearance: update(dets, frame) needs the BGR frame or features [N,512]")
        elif n:
            crops = self.eng.base.crop_norm(frame_t, self._dets[0], n, half=self.dtype == torch.float16)
            self._feats[0, :n].copy_(self.reid(crops.contiguous(memory_format=torch.channels_last)))
        out, nout = self.eng.update_device(self._dets, self._n, self._feats)
        torch.cuda.synchronize(self.dev)
        self.eng.check_errors()
        return out[0, : int(nout[0])].cpu().numpy()

    def reset(self):
        self.eng.reset(-1)

    def close(self):
        self.eng.close()
