"""ctypes binding of libstrongsort_hip.so (include/strongsort_hip.h).

The product path has no CPU fallback: if the HIP library is missing or a call fails, this module
raises.  Device memory is managed with torch tensors; their data_ptr() values cross the C ABI as
plain pointers.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

from . import cheader

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("SS_LIB_PATH") or os.path.join(_HERE, "libstrongsort_hip.so")     # SS_LIB_PATH: a differently built library (kernel experiments)
CSRC = os.path.join(_HERE, "csrc")

_H = cheader.parse(os.path.join(_HERE, "..", "include", "strongsort_hip.h"))      # the one place a signature, struct or constant is written
SS_OK, SS_ERR_INVALID, SS_ERR_CAPACITY, SS_ERR_HIP, SS_ERR_INFEASIBLE = (
    _H.defines[n] for n in ("SS_OK", "SS_ERR_INVALID", "SS_ERR_CAPACITY", "SS_ERR_HIP", "SS_ERR_INFEASIBLE"))
MAX_TRACKS, MAX_DETS, FEAT_DIM, OUT_COLS, DST_F16, DST_HWC, DST_U8 = (
    _H.defines["SS_" + n] for n in ("MAX_TRACKS", "MAX_DETS", "FEAT_DIM", "OUT_COLS", "DST_F16", "DST_HWC", "DST_U8"))
EXPORTS = list(_H.functions)
ss_config, ss_byte_config, ss_ocsort_config, ss_deepoc_config, ss_hybridsort_config, ss_conv_desc, ss_native_map, ss_zone_config = (
    _H.structs[n] for n in ("ss_config", "ss_byte_config", "ss_ocsort_config", "ss_deepoc_config", "ss_hybridsort_config", "ss_conv_desc",
                            "ss_native_map", "ss_zone_config"))


class SSError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"strongsort_hip error {code}: {msg}")
        self.code = code


def build(force: bool = False) -> str:
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(_HERE, "..", "include", "strongsort_hip.h"))
    stale = (not os.path.exists(SO_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(SO_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j4"] + (["-B"] if force else []))
    return SO_PATH


_lib = None


def load():
    """Load the library; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own HIP runtime: it must be the first one mapped into the process, or the
    # library would bind the system libamdhip64 and see no device.
    import torch  # noqa: F401
    if not os.path.exists(SO_PATH):
        raise SSError(SS_ERR_INVALID, f"{SO_PATH} not built — run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(SO_PATH)
    for name, (restype, argtypes) in _H.functions.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(ctx, rc):
    if rc != SS_OK:
        msg = load().ss_last_error(ctx)
        raise SSError(rc, msg.decode() if msg else "?")


def make_config(cfg, n_streams=1, debug=False) -> ss_config:
    return ss_config(cfg.max_dist, cfg.max_iou_distance, cfg.mc_lambda, cfg.gating_threshold, cfg.gated_cost,
                     cfg.std_weight_position, cfg.std_weight_velocity, cfg.ema_alpha, cfg.max_age, cfg.n_init,
                     cfg.nn_budget, n_streams, int(debug))


def make_byte_config(cfg) -> ss_byte_config:
    return ss_byte_config(cfg.track_high_thresh, cfg.track_low_thresh, cfg.new_track_thresh, cfg.match_thresh,
                          cfg.std_weight_position, cfg.std_weight_velocity, cfg.track_buffer, cfg.frame_rate, int(cfg.fuse_score),
                          int(cfg.kalman == "xywh"), cfg.max_tracks, cfg.max_dets)


def make_ocsort_config(cfg) -> ss_ocsort_config:
    return ss_ocsort_config(cfg.det_thresh, cfg.low_thresh, cfg.iou_threshold, cfg.inertia, cfg.max_age, cfg.min_hits, cfg.delta_t,
                            int(cfg.use_byte), cfg.max_tracks, cfg.max_dets)


def make_hybridsort_config(cfg) -> ss_hybridsort_config:
    return ss_hybridsort_config(cfg.det_thresh, cfg.low_thresh, cfg.iou_threshold, cfg.inertia, cfg.tcm_first_weight, cfg.tcm_byte_weight,
                                cfg.max_age, cfg.min_hits, cfg.delta_t, int(cfg.use_byte), int(cfg.asso == "hmiou"), cfg.max_tracks, cfg.max_dets)


def make_deepoc_config(cfg) -> ss_deepoc_config:
    return ss_deepoc_config(cfg.det_thresh, cfg.iou_threshold, cfg.inertia, cfg.w_association_emb, cfg.alpha_fixed_emb, cfg.aw_param,
                            cfg.max_age, cfg.min_hits, cfg.delta_t, int(cfg.appearance), int(cfg.dynamic_appearance),
                            int(cfg.adaptive_weighting), cfg.max_tracks, cfg.max_dets)
