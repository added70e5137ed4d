"""Frozen constants of the StrongSORT hot path (shared by the product and, by value, the oracle).

Every number here is a *decision* recorded in oracle/DECISIONS.md: the reference snapshot pins only
conf/iou/agnostic_nms/max_det (/root/reference/yolo_multi_model.py:18-21); everything else follows
BASELINE.json's north_star + SURVEY.md Appendix A.1 (upstream recall, unverified).
"""
from __future__ import annotations

from dataclasses import dataclass, asdict

# Layout constants compiled into the HIP library (csrc/ss_common.h mirrors these).
FEAT_DIM = 512          # OSNet embedding width (F = 512)
SEG_LEN = 64            # dot-product segment length: 8 segments of 64, each an fmaf chain
ROW_TILE = 32           # gallery rows / detection columns per MFMA 32x32 tile
CROP_H, CROP_W = 256, 128

TENTATIVE, CONFIRMED, DELETED = 1, 2, 3


@dataclass(frozen=True)
class StrongSortConfig:
    # association
    max_dist: float = 0.2            # cosine matching threshold (appearance stage)
    max_iou_distance: float = 0.7    # IoU-stage threshold on 1-IoU
    max_age: int = 30
    n_init: int = 3
    nn_budget: int = 100             # gallery rows kept per track
    mc_lambda: float = 0.995         # appearance/motion blend
    ema_alpha: float = 0.9
    gating_threshold: float = 9.4877  # chi2inv95[4]
    gated_cost: float = 1e5           # INFTY_COST
    # Kalman (DeepSORT xyah, h-scaled)
    std_weight_position: float = 1.0 / 20
    std_weight_velocity: float = 1.0 / 160
    # capacities of the device-resident track table (per stream)
    max_tracks: int = 256
    max_dets: int = 128

    def as_dict(self):
        return asdict(self)


@dataclass(frozen=True)
class DetectConfig:
    """The four overrides the reference pins (yolo_multi_model.py:18-21) + letterbox geometry."""
    conf: float = 0.3
    iou: float = 0.4
    agnostic_nms: bool = False
    max_det: int = 1000
    imgsz: int = 640
    stride: int = 32
    pad_value: int = 114
    max_wh: float = 7680.0            # per-class box offset (non-agnostic NMS)
    max_nms: int = 8192               # candidate cap after the confidence filter (LDS sort capacity)


COCO_KPT_SIGMAS = (.026, .025, .025, .035, .035, .079, .079, .072, .072, .062, .062, .107, .107, .087, .087, .089, .089)


@dataclass(frozen=True)
class ByteTrackConfig:
    """The BYTE tracker family (docs/BYTETRACK.md, decisions B-01..): Ultralytics' bytetrack.yaml / botsort.yaml defaults
    (recalled from Ultralytics 8.3.x).  kalman = "xyah" (ByteTrack) or "xywh" (BoT-SORT).  with_reid (xywh only): BoT-SORT's
    appearance term (§1c, decisions R-01..) with proximity_thresh on 1 - IoU, appearance_thresh on the halved cosine
    distance and the feature EMA weight feat_alpha.  with_pose (xywh only, not with with_reid): this project's keypoint term (§1e,
    decisions K-01..) — an OKS entry beside the fused IoU for the pairs within proximity_thresh, kept when (1 - OKS) / 2 <= pose_thresh;
    a keypoint counts when its visibility >= kpt_vis_thresh (float32), a pair when at least min_common_kpts count on both sides."""
    track_high_thresh: float = 0.25
    track_low_thresh: float = 0.1
    new_track_thresh: float = 0.25
    track_buffer: int = 30
    match_thresh: float = 0.8
    fuse_score: bool = True
    frame_rate: int = 30
    kalman: str = "xyah"
    std_weight_position: float = 1.0 / 20
    std_weight_velocity: float = 1.0 / 160
    # capacities of the device-resident track table (per stream: tracked + lost + unconfirmed) and of a frame
    max_tracks: int = 256
    max_dets: int = 128
    # BoT-SORT's ReID branch (§1c); appearance_thresh: older botsort.yaml files have 0.25, later 8.3.x ones 0.8 (R-03)
    with_reid: bool = False
    proximity_thresh: float = 0.5
    appearance_thresh: float = 0.25
    feat_alpha: float = 0.9
    # the keypoint (OKS) term (§1e); kpt_sigmas: the COCO-17 per-keypoint constants
    with_pose: bool = False
    pose_thresh: float = 0.25
    kpt_vis_thresh: float = 0.5
    min_common_kpts: int = 3
    kpt_sigmas: tuple = COCO_KPT_SIGMAS

    def __post_init__(self):
        if self.kalman not in ("xyah", "xywh"):
            raise ValueError(f"ByteTrackConfig.kalman: 'xyah' or 'xywh', not {self.kalman!r}")
        if self.with_reid and self.kalman != "xywh":
            raise ValueError("ByteTrackConfig.with_reid needs kalman='xywh' (BoT-SORT): ByteTrack has no ReID")
        if self.with_pose and self.kalman != "xywh":
            raise ValueError("ByteTrackConfig.with_pose needs kalman='xywh' (BoT-SORT): ByteTrack has no keypoint term")
        if self.with_pose and self.with_reid:
            raise ValueError("ByteTrackConfig: with_pose and with_reid cannot be combined")
        if self.with_pose and not 1 <= len(self.kpt_sigmas) <= 32:
            raise ValueError("ByteTrackConfig.kpt_sigmas: 1..32 keypoints")
        if not (0 < self.max_tracks <= 256 and 0 < self.max_dets <= 128):
            raise ValueError("ByteTrackConfig: max_tracks <= 256 and max_dets <= 128 (the device table's capacity)")

    @property
    def max_time_lost(self) -> int:
        return int(self.frame_rate / 30.0 * self.track_buffer)

    def as_dict(self):
        return asdict(self)


@dataclass(frozen=True)
class OCSortConfig:
    """OC-SORT (docs/OCSORT.md, decisions O-01..): the motion-only tracker with observation-centric re-update, momentum
    (inertia, delta_t) and recovery; use_byte adds the second association on the rows between low_thresh and det_thresh.
    det_thresh is ByteTrackConfig.track_high_thresh, so the three IoU trackers see the same high rows at default settings (O-01)."""
    det_thresh: float = 0.25
    low_thresh: float = 0.1
    max_age: int = 30
    min_hits: int = 3
    iou_threshold: float = 0.3
    delta_t: int = 3
    inertia: float = 0.2
    use_byte: bool = False
    # capacities of the device-resident track table (per stream) and of a frame
    max_tracks: int = 256
    max_dets: int = 128

    def __post_init__(self):
        if not 1 <= self.delta_t <= 8:
            raise ValueError(f"OCSortConfig.delta_t: 1..8, not {self.delta_t}")
        if self.max_age < 1 or self.min_hits < 0:
            raise ValueError("OCSortConfig: max_age >= 1 and min_hits >= 0")
        if not 0.0 < self.iou_threshold <= 1.0:
            raise ValueError(f"OCSortConfig.iou_threshold: in (0, 1], not {self.iou_threshold}")
        if not self.inertia >= 0.0:
            raise ValueError(f"OCSortConfig.inertia: >= 0, not {self.inertia}")
        if not self.low_thresh <= self.det_thresh:
            raise ValueError("OCSortConfig: low_thresh <= det_thresh")
        if not (0 < self.max_tracks <= 256 and 0 < self.max_dets <= 128):
            raise ValueError("OCSortConfig: max_tracks <= 256 and max_dets <= 128 (the device table's capacity)")

    def as_dict(self):
        return asdict(self)


@dataclass(frozen=True)
class DeepOCSortConfig:
    """Deep OC-SORT (docs/DEEPOCSORT.md, decisions DO-01..): OC-SORT without the BYTE stage, plus camera-motion compensation of
    filter and observations, a feature EMA whose weight follows the detection score (dynamic_appearance, alpha_fixed_emb) and an
    appearance cost weighted by how clearly a row or track prefers one partner (adaptive_weighting, w_association_emb, aw_param)."""
    det_thresh: float = 0.25
    max_age: int = 30
    min_hits: int = 3
    iou_threshold: float = 0.3
    delta_t: int = 3
    inertia: float = 0.2
    w_association_emb: float = 0.75
    alpha_fixed_emb: float = 0.95
    aw_param: float = 0.5
    appearance: bool = True
    dynamic_appearance: bool = True
    adaptive_weighting: bool = True
    # capacities of the device-resident track table (per stream) and of a frame
    max_tracks: int = 256
    max_dets: int = 128

    def __post_init__(self):
        if not 1 <= self.delta_t <= 8:
            raise ValueError(f"DeepOCSortConfig.delta_t: 1..8, not {self.delta_t}")
        if self.max_age < 1 or self.min_hits < 0:
            raise ValueError("DeepOCSortConfig: max_age >= 1 and min_hits >= 0")
        if not 0.0 < self.iou_threshold <= 1.0:
            raise ValueError(f"DeepOCSortConfig.iou_threshold: in (0, 1], not {self.iou_threshold}")
        if not self.inertia >= 0.0:
            raise ValueError(f"DeepOCSortConfig.inertia: >= 0, not {self.inertia}")
        if not self.det_thresh < 1.0:
            raise ValueError(f"DeepOCSortConfig.det_thresh: < 1 (the trust of a score divides by 1 - det_thresh), not {self.det_thresh}")
        if not self.w_association_emb >= 0.0:
            raise ValueError(f"DeepOCSortConfig.w_association_emb: >= 0, not {self.w_association_emb}")
        if not 0.0 <= self.alpha_fixed_emb <= 1.0:
            raise ValueError(f"DeepOCSortConfig.alpha_fixed_emb: in [0, 1], not {self.alpha_fixed_emb}")
        if not 0.0 <= self.aw_param < 1.0:
            raise ValueError(f"DeepOCSortConfig.aw_param: in [0, 1), not {self.aw_param}")
        if not (0 < self.max_tracks <= 256 and 0 < self.max_dets <= 128):
            raise ValueError("DeepOCSortConfig: max_tracks <= 256 and max_dets <= 128 (the device table's capacity)")

    def as_dict(self):
        return asdict(self)


@dataclass(frozen=True)
class HybridSortConfig:
    """Hybrid-SORT (docs/HYBRIDSORT.md, decisions H-01..): OC-SORT's machinery with three weak cues — the detection confidence as
    a Kalman state and a cost term (tcm_first_weight, tcm_byte_weight; 0 switches the cue off), the height-modulated IoU
    (asso "hmiou", or plain "iou"), and the direction-consistency term over the four box corners and delta_t time offsets
    (inertia is the weight of each corner's term)."""
    det_thresh: float = 0.25
    low_thresh: float = 0.1
    max_age: int = 30
    min_hits: int = 3
    iou_threshold: float = 0.3
    delta_t: int = 3
    inertia: float = 0.05
    use_byte: bool = True
    asso: str = "hmiou"
    tcm_first_weight: float = 1.0
    tcm_byte_weight: float = 1.0
    # capacities of the device-resident track table (per stream) and of a frame
    max_tracks: int = 256
    max_dets: int = 128

    ASSO = ("hmiou", "iou")

    def __post_init__(self):
        if not 1 <= self.delta_t <= 8:
            raise ValueError(f"HybridSortConfig.delta_t: 1..8, not {self.delta_t}")
        if self.max_age < 1 or self.min_hits < 0:
            raise ValueError("HybridSortConfig: max_age >= 1 and min_hits >= 0")
        if not 0.0 < self.iou_threshold <= 1.0:
            raise ValueError(f"HybridSortConfig.iou_threshold: in (0, 1], not {self.iou_threshold}")
        if not self.inertia >= 0.0:
            raise ValueError(f"HybridSortConfig.inertia: >= 0, not {self.inertia}")
        if not self.low_thresh <= self.det_thresh:
            raise ValueError("HybridSortConfig: low_thresh <= det_thresh")
        if self.asso not in self.ASSO:
            raise ValueError(f"HybridSortConfig.asso: one of {self.ASSO}, not {self.asso!r}")
        if not (self.tcm_first_weight >= 0.0 and self.tcm_byte_weight >= 0.0):
            raise ValueError("HybridSortConfig: tcm_first_weight >= 0 and tcm_byte_weight >= 0")
        if not (0 < self.max_tracks <= 256 and 0 < self.max_dets <= 128):
            raise ValueError("HybridSortConfig: max_tracks <= 256 and max_dets <= 128 (the device table's capacity)")

    def as_dict(self):
        return asdict(self)


# tracker_type of YOLO / FramePipeline / the CLI -> the BYTE configuration it runs (None: StrongSORT, the OC-SORT family)
TRACKER_TYPES = ("strongsort", "bytetrack", "botsort", "ocsort", "deep_ocsort", "hybridsort")


def hybridsort_config(tracker_type: str, asso: str = "hmiou", use_byte: bool = True, camera_motion: bool = False, with_reid: bool = False,
                      with_pose: bool = False, ocsort_use_byte: bool = False):
    """tracker_type -> the Hybrid-SORT configuration it runs (None: another tracker).  Hybrid-SORT is motion only: BoT-SORT's
    options are refused by name, and its BYTE stage has a switch of its own (use_byte), not OC-SORT's."""
    if tracker_type not in TRACKER_TYPES:
        raise ValueError(f"tracker_type must be one of {TRACKER_TYPES}, not {tracker_type!r}")
    if tracker_type != "hybridsort":
        if asso != "hmiou" or not use_byte:
            raise ValueError(f"hybrid_asso and hybrid_use_byte are Hybrid-SORT's: tracker_type 'hybridsort', not {tracker_type!r}")
        return None
    for name, on in (("camera_motion", camera_motion), ("with_reid", with_reid), ("with_pose", with_pose)):
        if on:
            raise ValueError(f"{name} is not available with tracker_type 'hybridsort' (Hybrid-SORT is motion only, docs/HYBRIDSORT.md)")
    if ocsort_use_byte:
        raise ValueError("ocsort_use_byte is OC-SORT's BYTE stage: Hybrid-SORT's is hybrid_use_byte, on by default (docs/HYBRIDSORT.md)")
    return HybridSortConfig(asso=asso, use_byte=bool(use_byte))


def deep_ocsort_config(tracker_type: str, with_reid: bool = False, with_pose: bool = False, ocsort_use_byte: bool = False):
    """tracker_type -> the Deep OC-SORT configuration it runs (None: another tracker).  Its appearance branch is its own: BoT-SORT's
    options and OC-SORT's BYTE stage are refused by name.  camera_motion is accepted (docs/DEEPOCSORT.md step 1b)."""
    if tracker_type not in TRACKER_TYPES:
        raise ValueError(f"tracker_type must be one of {TRACKER_TYPES}, not {tracker_type!r}")
    if tracker_type != "deep_ocsort":
        return None
    for name, on in (("with_reid", with_reid), ("with_pose", with_pose)):
        if on:
            raise ValueError(f"{name} is BoT-SORT's: it is not available with tracker_type 'deep_ocsort' (its appearance is always on, docs/DEEPOCSORT.md)")
    if ocsort_use_byte:
        raise ValueError("ocsort_use_byte is OC-SORT's BYTE stage: Deep OC-SORT has none (docs/DEEPOCSORT.md)")
    return DeepOCSortConfig()


def ocsort_config(tracker_type: str, use_byte: bool = False, camera_motion: bool = False, with_reid: bool = False, with_pose: bool = False):
    """tracker_type -> the OC-SORT configuration it runs (None: another tracker).  OC-SORT is motion only: the BoT-SORT options
    are refused by name."""
    if tracker_type not in TRACKER_TYPES:
        raise ValueError(f"tracker_type must be one of {TRACKER_TYPES}, not {tracker_type!r}")
    if tracker_type != "ocsort":
        if use_byte:
            raise ValueError(f"use_byte is OC-SORT's BYTE stage: tracker_type 'ocsort', not {tracker_type!r}")
        return None
    for name, on in (("camera_motion", camera_motion), ("with_reid", with_reid), ("with_pose", with_pose)):
        if on:
            raise ValueError(f"{name} is not available with tracker_type 'ocsort' (OC-SORT is motion only, docs/OCSORT.md)")
    return OCSortConfig(use_byte=bool(use_byte))


def byte_config(tracker_type: str, with_reid: bool = False, with_pose: bool = False):
    if tracker_type not in TRACKER_TYPES:
        raise ValueError(f"tracker_type must be one of {TRACKER_TYPES}, not {tracker_type!r}")
    if tracker_type == "ocsort":
        if with_reid or with_pose:
            raise ValueError(f"{'with_reid' if with_reid else 'with_pose'} is not available with tracker_type 'ocsort' (OC-SORT is motion only)")
        return None
    if with_reid and tracker_type != "botsort":
        raise ValueError(f"with_reid is BoT-SORT's ReID branch: tracker_type 'botsort', not {tracker_type!r}")
    if with_pose and tracker_type != "botsort":
        raise ValueError(f"with_pose is BoT-SORT's keypoint term: tracker_type 'botsort', not {tracker_type!r}")
    if tracker_type in ("strongsort", "deep_ocsort", "hybridsort"):
        return None
    return ByteTrackConfig(kalman="xywh" if tracker_type == "botsort" else "xyah", with_reid=bool(with_reid), with_pose=bool(with_pose))


def check_pose(cfg, nk: int):
    """with_pose against the detector's keypoint columns nk (3 per keypoint): a pose head whose keypoint count has sigmas."""
    if cfg is None or not cfg.with_pose:
        return
    if nk == 0:
        raise ValueError("with_pose needs a pose detector (this one has no keypoint columns)")
    if nk // 3 != len(cfg.kpt_sigmas):
        raise ValueError(f"with_pose: the detector has {nk // 3} keypoints, kpt_sigmas {len(cfg.kpt_sigmas)}")


# BoT-SORT's ReID model (docs/BYTETRACK.md §1d): "osnet" — OSNet-x0.25 on the detections' crops (§1c, the default); "auto" —
# Ultralytics' `model: auto`, the detections' features read from the detector's own head inputs (no second network or weights file)
REID_MODELS = ("osnet", "auto")


def check_reid_model(reid_model: str, with_reid: bool, reid_weights=None) -> str:
    if reid_model not in REID_MODELS:
        raise ValueError(f"reid_model must be one of {REID_MODELS}, not {reid_model!r}")
    if reid_model == "auto" and not with_reid:
        raise ValueError("reid_model='auto' is a model for BoT-SORT's ReID branch: it needs with_reid=True (tracker_type 'botsort')")
    if reid_model == "auto" and reid_weights:
        raise ValueError("reid_model='auto' reads the detector's own features: reid_weights (OSNet) does not apply")
    return reid_model


# BoT-SORT's camera-motion estimator: "ecc" — the 0.1x euclidean ECC of csrc/ss_cmc.hip (G-01, the default: what camera_motion=True
# has always meant); "sparseOptFlow" — Ultralytics' botsort.yaml default, restated in docs/BYTETRACK.md §1f (csrc/ss_gmc.hip)
GMC_METHODS = ("ecc", "sparseOptFlow")


def check_gmc_method(gmc_method: str, camera_motion: bool, tracker_type: str) -> str:
    if gmc_method not in GMC_METHODS:
        raise ValueError(f"gmc_method must be one of {GMC_METHODS}, not {gmc_method!r}")
    if gmc_method == "sparseOptFlow" and not camera_motion:
        raise ValueError("gmc_method='sparseOptFlow' is a camera-motion estimator: it needs camera_motion=True")
    if gmc_method == "sparseOptFlow" and tracker_type not in ("botsort", "deep_ocsort"):
        raise ValueError(f"gmc_method='sparseOptFlow' is BoT-SORT's GMC: tracker_type 'botsort', not {tracker_type!r} "
                         "(StrongSORT's compensation is ECC, ByteTrack has none, G-05)")
    return gmc_method
