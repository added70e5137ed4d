"""The tracker families' entries and their two host helpers without a device.

The BYTE, OC-SORT and Deep OC-SORT entries look at their arguments before they look for a context (the zone / bank convention,
tests/test_zones_cpu.py), so every argument fault is reported on a machine without a GPU.  csrc/ss_host.h's offset plan of a
carve-out and its list-order gather are plain host code: tests/tracker_state_host_main.cpp runs them against a double loop and the
stated layout, built with the host compiler and -fsanitize=address,undefined as a program of its own.
"""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from strongsort_yolo_amd import lib
from strongsort_yolo_amd.config import ByteTrackConfig, DeepOCSortConfig, OCSortConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
BYTE_RANGE = "1 <= max_tracks <= 256, 1 <= max_dets <= 128, frame_rate >= 1, kalman_xywh 0 / 1"
OC_RANGE = "1 <= max_tracks <= 256, 1 <= max_dets <= 128, 1 <= delta_t <= 8, max_age >= 1"
FAMILIES = {
    "byte": (lambda: lib.make_byte_config(ByteTrackConfig()), BYTE_RANGE,
             dict(max_tracks=(0, 257), max_dets=(0, 129), kalman_xywh=(2,), frame_rate=(0,))),
    "ocsort": (lambda: lib.make_ocsort_config(OCSortConfig()), OC_RANGE + ", min_hits >= 0, 0 < iou_threshold <= 1, inertia >= 0, low_thresh",
               dict(max_tracks=(0, 257), max_dets=(0, 129), delta_t=(0, 9), iou_threshold=(0.0, 1.5), use_byte=(2,))),
    "deepoc": (lambda: lib.make_deepoc_config(DeepOCSortConfig()), OC_RANGE + ", min_hits >= 0, 0 < iou_threshold <= 1, inertia >= 0, det_thresh",
               dict(max_tracks=(0, 257), max_dets=(0, 129), delta_t=(0, 9), iou_threshold=(0.0, 1.5), alpha_fixed_emb=(1.5,), aw_param=(1.0,))),
}


def _last(L):
    return L.ss_last_error(None).decode()


@pytest.mark.parametrize("family", list(FAMILIES))
def test_create_checks_the_config_before_the_context(family):
    L = lib.load()
    make, words, bad = FAMILIES[family]
    create = getattr(L, f"ss_{family}_create")
    assert create(None, C.byref(make())) == lib.SS_ERR_INVALID                    # a good config: only the context is missing
    assert "null context" in _last(L) or "null argument" in _last(L)
    assert create(None, None) == lib.SS_ERR_INVALID and "null argument" in _last(L)
    for field, values in bad.items():
        for v in values:
            cfg = make()
            setattr(cfg, field, v)
            assert create(None, C.byref(cfg)) == lib.SS_ERR_INVALID, (field, v)
            msg = _last(L)
            assert msg.startswith(f"ss_{family}_create: ") and words in msg and "null" not in msg, (field, v, msg)


def _update_calls(L):
    """(name, call(n_frames, missing)) of every update entry with a NULL context: `missing` names the pointer argument left NULL"""
    f, i = (C.c_float * 4)(), (C.c_int * 4)()
    fp, ip = C.cast(f, C.POINTER(C.c_float)), C.cast(i, C.POINTER(C.c_int))

    def args(names, missing):
        return [None if n == missing or n in ("feats", "geom") else (ip if n in ("ndets", "nout") else fp) for n in names]

    plain = ("dets", "ndets", "out", "nout")
    yield "ss_byte_update_group", plain, lambda n, m: L.ss_byte_update_group(None, n, *args(plain, m))
    yield "ss_ocsort_update_group", plain, lambda n, m: L.ss_ocsort_update_group(None, n, *args(plain, m))
    feats = ("dets", "ndets", "feats", "out", "nout")
    yield "ss_byte_update_group_feats", plain, lambda n, m: L.ss_byte_update_group_feats(None, n, *args(feats, m))
    yield "ss_deepoc_update_group", plain, lambda n, m: L.ss_deepoc_update_group(None, n, *args(feats, m))
    obb = ("dets", "ndets", "out", "rbox", "nout")
    yield "ss_byte_update_group_obb", obb, lambda n, m: L.ss_byte_update_group_obb(None, n, *args(obb, m))
    need = ("dets", "ndets", "kpts", "out", "nout")

    def kpts(n, m):
        a = args(need, m)
        return L.ss_byte_update_group_kpts(None, n, a[0], a[1], a[2], 51, 0, None, a[3], a[4])
    yield "ss_byte_update_group_kpts", need, kpts


def test_update_entries_check_their_arguments_before_the_context():
    L = lib.load()
    for name, pointers, call in _update_calls(L):
        for n in (0, 33):
            assert call(n, None) == lib.SS_ERR_INVALID and _last(L) == f"{name}: 1 <= n_frames <= SS_FMAX", (name, n, _last(L))
        for missing in pointers:
            assert call(4, missing) == lib.SS_ERR_INVALID and _last(L) == f"{name}: null argument", (name, missing, _last(L))
        assert call(4, None) == lib.SS_ERR_INVALID and "null context" in _last(L), (name, _last(L))      # sound arguments


def test_every_other_entry_refuses_a_null_context():
    L = lib.load()
    n = [None] * 16
    for fam in ("byte", "ocsort", "deepoc"):
        assert getattr(L, f"ss_{fam}_reset")(None, 0) == lib.SS_ERR_INVALID
        assert getattr(L, f"ss_{fam}_reset")(None, -1) == lib.SS_ERR_INVALID
        assert getattr(L, f"ss_{fam}_destroy")(None) == lib.SS_ERR_INVALID and "null context" in _last(L)
    assert L.ss_byte_get_tracks(None, 0, 256, *n[:8]) == lib.SS_ERR_INVALID and "ss_byte_get_tracks" in _last(L)
    assert L.ss_ocsort_get_tracks(None, 0, 256, *n[:13]) == lib.SS_ERR_INVALID and "ss_ocsort_get_tracks" in _last(L)
    assert L.ss_deepoc_get_tracks(None, 0, 256, *n[:13]) == lib.SS_ERR_INVALID and "ss_deepoc_get_tracks" in _last(L)
    f = C.cast((C.c_float * 4)(), C.POINTER(C.c_float))
    u = C.cast((C.c_uint32 * 4)(), C.POINTER(C.c_uint32))
    assert L.ss_byte_get_features(None, 0, 256, f) == lib.SS_ERR_INVALID
    assert L.ss_deepoc_get_features(None, 0, 256, f) == lib.SS_ERR_INVALID
    assert L.ss_byte_get_angles(None, 0, 256, f) == lib.SS_ERR_INVALID
    assert L.ss_byte_get_keypoints(None, 0, 256, None, u) == lib.SS_ERR_INVALID
    assert L.ss_byte_get_det_keypoints(None, 0, 0, f, u) == lib.SS_ERR_INVALID
    assert L.ss_byte_set_reid(None, 1, 0.5, 0.25, 0.9) == lib.SS_ERR_INVALID and "no BYTE state (ss_byte_create)" in _last(L)
    assert L.ss_byte_set_pose(None, 0, 0, None, 0.5, 0.25, 0.5, 3) == lib.SS_ERR_INVALID
    assert L.ss_byte_set_obb(None, 1) == lib.SS_ERR_INVALID and L.ss_byte_set_gmc(None, None) == lib.SS_ERR_INVALID
    assert L.ss_deepoc_set_gmc(None, None) == lib.SS_ERR_INVALID and "no Deep OC-SORT state (ss_deepoc_create)" in _last(L)


def test_host_helpers_under_the_sanitizers(tmp_path):
    """The offset plan and the gather of csrc/ss_host.h in a program of their own (it prints what it checked and exits 0)."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "clang++"
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))               # the HIP headers are next to the compiler the library is built with
    rocm = os.environ.get("ROCM_PATH") or (os.path.dirname(os.path.dirname(os.path.realpath(hipcc))) if hipcc else "/opt/rocm")
    exe = str(tmp_path / "tracker_state_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"), os.path.join(_HERE, "tracker_state_host_main.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plans 5" in out.stdout and "gathers 48" in out.stdout, out.stdout
