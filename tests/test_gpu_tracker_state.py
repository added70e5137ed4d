"""The states of the three tracker families on the MI355X (BYTE with its modes, OC-SORT, Deep OC-SORT): what owning their device
memory must keep true.  A state made again on a live context, a reset of one stream beside another, another keypoint count on a live
BYTE state, read-backs into arrays that are too small, and the mode exclusions.  Two streams, 8 frames of at most 8 rows; the scenes
are the existing generators', and every comparison is byte for byte against another run of the device (the references are the other
suites' business)."""
import ctypes as C

import numpy as np
import pytest
import torch

from strongsort_yolo_amd import lib
from strongsort_yolo_amd.config import ByteTrackConfig, DeepOCSortConfig, OCSortConfig
from tests import obb_ref
from tests.deepocsort_scenes import deep_stream
from tests.test_botsort_pose_cpu import pose_stream
from tests.test_bytetrack_cpu import byte_stream

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
S, F, ROWS = 2, 8, 8
SIGMAS = ByteTrackConfig().kpt_sigmas
BOT = dict(kalman="xywh")


def _scene(seed):
    """per stream a dict of lists over the frames: dets [n,6], feats [n,512], kpts [n,17,3] (n <= 8), and 11-column oriented rows"""
    out = []
    for s in range(S):
        frames, feats, _ = deep_stream(seed + s, F, n_ids=5, camera=False)
        byte = byte_stream(seed + s, F, n_ids=5)
        pose = pose_stream(seed + s, F, n_ids=5)
        out.append(dict(dets=[d[:ROWS] for d in frames], feats=[f[:ROWS] for f in feats], byte=[d[:ROWS] for d in byte],
                        pdets=[d[:ROWS] for d, _ in pose], kpts=[k[:ROWS] for _, k in pose], obb=[d[:ROWS] for d in obb_ref.rotating_scene(seed + s, F)]))
    return out


SCENE = _scene(40)


def _engines():
    from strongsort_yolo_amd.engine import ByteTrackEngine, DeepOCSortEngine, OCSortEngine
    return dict(
        byte=(lambda base=None, **kw: ByteTrackEngine(ByteTrackConfig(**kw), S, 0, engine=base), "byte", dict(track_buffer=3, max_tracks=64), "no BYTE state"),
        byte_reid=(lambda base=None, **kw: ByteTrackEngine(ByteTrackConfig(with_reid=True, **BOT, **kw), S, 0, engine=base), "dets", {}, "no BYTE state"),
        ocsort=(lambda base=None, **kw: OCSortEngine(OCSortConfig(**kw), S, 0, engine=base), "dets", dict(max_age=2, max_tracks=64), "no OC-SORT state"),
        deepoc=(lambda base=None, **kw: DeepOCSortEngine(DeepOCSortConfig(**kw), S, 0, engine=base), "dets", dict(max_age=2, max_tracks=64), "no Deep OC-SORT state"))


def _run(eng, f0, f1, dets="dets", group=4, k=None, scene=SCENE):
    """frames f0 .. f1 - 1 of both streams through update_group calls of `group` frames -> per stream a list of row arrays.  k: the
    keypoints per row of a BYTE engine with the keypoint term (the scene's first k of 17)"""
    cols = 11 if dets == "obb" else 6
    rows = [[] for _ in range(S)]
    out, nout = torch.zeros(group, S, 256, 8, device=DEV), torch.zeros(group, S, dtype=torch.int32, device=DEV)
    for g0 in range(f0, f1, group):
        n = min(group, f1 - g0)
        hd, hn, hf = np.zeros((n, S, 128, cols), np.float32), np.zeros((n, S), np.int32), np.zeros((n, S, 128, 512), np.float32)
        hk = np.zeros((n, S, 128, k or 1, 3), np.float32)
        for f in range(n):
            for s in range(S):
                d = scene[s][dets][g0 + f]
                hd[f, s, :len(d)], hn[f, s] = d, len(d)
                if dets == "dets":
                    hf[f, s, :len(d)] = scene[s]["feats"][g0 + f]
                if k:
                    hk[f, s, :len(d)] = scene[s]["kpts"][g0 + f][:, :k]
        kw = dict(kpts=torch.from_numpy(hk).to(DEV)) if k else {}
        if dets == "obb":
            kw = dict(rbox=torch.zeros(n, S, 256, 5, device=DEV))
        eng.update_group(n, torch.from_numpy(hd).to(DEV), torch.from_numpy(hn).to(DEV), torch.from_numpy(hf).to(DEV), None, out[:n], nout[:n], **kw)
        eng.check_errors()
        ho, hno = out[:n].cpu().numpy(), nout[:n].cpu().numpy()
        for f in range(n):
            for s in range(S):
                rows[s].append(ho[f, s, :hno[f, s]].tobytes())
    return rows


def _snap(eng, s):
    """everything the engine reads back of one stream, arrays as bytes"""
    t = dict(eng.tracks(s))
    if eng.reid:
        t["features"] = eng.features(s)
    if eng.pose:
        t["offsets"], t["visible"] = eng.keypoints(s)
    return {k: (v.shape, v.tobytes()) if isinstance(v, np.ndarray) else v for k, v in t.items()}


def _n_tracks(t):
    return t["n_tracks"] if "n_tracks" in t else t["n_tracked"] + t["n_lost"]


@pytest.mark.parametrize("family", ["byte", "ocsort", "deepoc"])
def test_a_state_made_again_on_a_live_context_starts_from_nothing(family):
    from strongsort_yolo_amd.engine import TrackerEngine
    make, dets, other, no_state = _engines()[family]
    base = TrackerEngine(n_streams=S)
    first = make(base)
    rows = _run(first, 0, F, dets)
    snaps = [_snap(first, s) for s in range(S)]
    assert all(_n_tracks(t) >= 2 for t in snaps)
    _run(make(base, **other), 0, F, dets)                           # another table size and another age limit in the first one's place
    again = make(base)
    assert _run(again, 0, F, dets) == rows
    assert [_snap(again, s) for s in range(S)] == snaps
    again.close()                                                   # a shared context: the state goes, the context stays
    base.check_errors()
    with pytest.raises(lib.SSError, match=no_state) as ei:
        _run(again, 0, 1, dets)
    assert ei.value.code == lib.SS_ERR_INVALID
    base.close()


@pytest.mark.parametrize("family", ["byte", "byte_reid", "ocsort", "deepoc"])
def test_reset_of_one_stream_leaves_the_other_alone(family):
    make, dets, _, _ = _engines()[family]
    eng = make()
    head = _run(eng, 0, 4, dets)
    kept = _snap(eng, 0)
    eng.reset(1)
    assert _snap(eng, 0) == kept                                    # (with ReID the features are part of it)
    t = eng.tracks(1)
    assert _n_tracks(t) == 0 and t["next_id"] == 1 and t.get("frame_id", t.get("frame_count")) == 0
    tail = _run(eng, 4, F, dets)
    whole, rest = make(), make()
    assert head[0] + tail[0] == _run(whole, 0, F, dets)[0] and _snap(eng, 0) == _snap(whole, 0)
    assert tail[1] == _run(rest, 4, F, dets)[1] and _snap(eng, 1) == _snap(rest, 1)
    for e in (eng, whole, rest):
        e.close()


def _pose(k):
    from strongsort_yolo_amd.engine import ByteTrackEngine
    return ByteTrackEngine(ByteTrackConfig(with_pose=True, kpt_sigmas=SIGMAS[:k], **BOT), S, 0)


def test_another_keypoint_count_on_a_live_state():
    fresh = {}
    for k in (5, 17):
        e = _pose(k)
        fresh[k] = (_run(e, 0, F, "pdets", k=k), [_snap(e, s) for s in range(S)])
        e.close()
    assert fresh[5] != fresh[17]
    eng = _pose(17)
    _run(eng, 0, 3, "pdets", k=17)
    side = torch.cuda.Stream(DEV)                                   # a non-blocking stream: nothing orders it with the null stream
    with torch.cuda.stream(side):
        eng.use_current_stream()
        for k in (5, 17, 5):                                        # smaller tables in the same memory, larger ones again, smaller again
            sg = (C.c_double * k)(*SIGMAS[:k])
            eng._ck(eng.L.ss_byte_set_pose(eng.ctx, 1, k, sg, eng.cfg.proximity_thresh, eng.cfg.pose_thresh, eng.cfg.kpt_vis_thresh, eng.cfg.min_common_kpts))
            eng.K = k
            assert (_run(eng, 0, F, "pdets", k=k), [_snap(eng, s) for s in range(S)]) == fresh[k], k
    eng.close()


def _sentinel(shape, dtype):
    """an array whose every byte is 0x5A"""
    return np.frombuffer(b"\x5a" * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype).reshape(shape).copy()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _capacity(call, n, arrays):
    """call(cap, arrays) with cap = n - 1 refuses and leaves the sentinel-filled arrays alone; with cap = n it fills n rows of each"""
    before = [a.tobytes() for a in arrays]
    assert call(n - 1) == lib.SS_ERR_CAPACITY
    assert [a.tobytes() for a in arrays] == before
    assert call(n) == lib.SS_OK
    for a, b in zip(arrays, before):
        assert a[:n].tobytes() != b[:a[:n].nbytes] and a[n:].tobytes() == b[a[:n].nbytes:]


def _cast(name):
    """the entry with untyped pointer arguments (the arrays of this test go in as void pointers)"""
    fn = getattr(C.CDLL(lib.SO_PATH), name)
    fn.restype, fn.argtypes = C.c_int, None
    return fn


@pytest.mark.parametrize("family", ["byte_reid", "byte_pose", "byte_obb", "ocsort", "deepoc"])
def test_read_backs_into_arrays_that_are_too_small(family):
    from strongsort_yolo_amd.engine import ByteTrackEngine
    T = 256
    if family == "byte_pose":
        eng, dets, k = _pose(17), "pdets", 17
    elif family == "byte_obb":
        eng, dets, k = ByteTrackEngine(ByteTrackConfig(), S, 0, obb=True), "obb", None
    else:
        eng, dets, k = _engines()[family][0](), "dets", None
    _run(eng, 0, F, dets, k=k)
    t = eng.tracks(0)
    n = _n_tracks(t)
    assert n >= 2
    ctx, counts = eng.ctx, [C.c_int(-7) for _ in range(4)]
    refs = [C.byref(c) for c in counts]
    if family.startswith("byte"):
        arrays = [_sentinel(T, np.int32) for _ in range(3)] + [_sentinel((T, 8), np.float64)]
        get = _cast("ss_byte_get_tracks")
        _capacity(lambda cap: get(ctx, 0, cap, *refs, *[_p(a) for a in arrays]), n, arrays)
        assert [c.value for c in counts] == [t["n_tracked"], t["n_lost"], t["next_id"], t["frame_id"]]
        for c in counts:
            c.value = -7
        assert get(ctx, 0, n - 1, *refs, *[_p(a) for a in arrays]) == lib.SS_ERR_CAPACITY              # the counts all the same
        assert [c.value for c in counts] == [t["n_tracked"], t["n_lost"], t["next_id"], t["frame_id"]]
        more = dict(byte_reid=("ss_byte_get_features", [_sentinel((T, 512), np.float32)]),
                    byte_pose=("ss_byte_get_keypoints", [_sentinel((T, 17, 2), np.float64), _sentinel(T, np.uint32)]),
                    byte_obb=("ss_byte_get_angles", [_sentinel(T, np.float32)]))[family]
    else:
        arrays = [_sentinel(T, np.int32) for _ in range(6)] + [_sentinel((T, 7), np.float64), _sentinel((T, 49), np.float64),
                                                               _sentinel((T, 4), np.float32), _sentinel((T, 2), np.float64)]
        get = _cast(f"ss_{family}_get_tracks")
        _capacity(lambda cap: get(ctx, 0, cap, *refs[:3], *[_p(a) for a in arrays]), n, arrays)
        for c in counts:
            c.value = -7
        assert get(ctx, 0, n - 1, *refs[:3], *[_p(a) for a in arrays]) == lib.SS_ERR_CAPACITY
        assert [c.value for c in counts[:3]] == [t["n_tracks"], t["next_id"], t["frame_count"]]
        more = ("ss_deepoc_get_features", [_sentinel((T, 512), np.float32)]) if family == "deepoc" else None
    if more:
        fn = _cast(more[0])
        _capacity(lambda cap: fn(ctx, 0, cap, *[_p(a) for a in more[1]]), n, more[1])
        assert fn(ctx, 0, n - 1, *[_p(a) for a in more[1]]) == lib.SS_ERR_CAPACITY
    assert eng.L.ss_last_error(ctx).decode().endswith("cap too small")
    eng.close()


def test_mode_exclusions_by_name():
    """the pairings tests/test_gpu_botsort_pose.py and tests/test_gpu_obb.py do not already refuse, each with its message"""
    from strongsort_yolo_amd.engine import ByteTrackEngine, _ptr
    L = lib.load()
    d6, d11, n1 = torch.zeros(1, S, 128, 6, device=DEV), torch.zeros(1, S, 128, 11, device=DEV), torch.zeros(1, S, dtype=torch.int32, device=DEV)
    o8, o5, ft = torch.zeros(1, S, 256, 8, device=DEV), torch.zeros(1, S, 256, 5, device=DEV), torch.zeros(1, S, 128, 512, device=DEV)
    kp = torch.zeros(1, S, 128, 17, 3, device=DEV)
    sg = (C.c_double * 17)(*SIGMAS)

    def refused(eng, rc, words):
        assert rc == lib.SS_ERR_INVALID and words in L.ss_last_error(eng.ctx).decode(), L.ss_last_error(eng.ctx).decode()

    def updates(eng):
        return dict(plain=lambda: L.ss_byte_update_group(eng.ctx, 1, _ptr(d6), _ptr(n1), _ptr(o8), _ptr(n1)),
                    feats=lambda: L.ss_byte_update_group_feats(eng.ctx, 1, _ptr(d6), _ptr(n1), _ptr(ft), _ptr(o8), _ptr(n1)),
                    kpts=lambda: L.ss_byte_update_group_kpts(eng.ctx, 1, _ptr(d6), _ptr(n1), _ptr(kp), 51, 0, None, _ptr(o8), _ptr(n1)),
                    obb=lambda: L.ss_byte_update_group_obb(eng.ctx, 1, _ptr(d11), _ptr(n1), _ptr(o8), _ptr(o5), _ptr(n1)))

    x = ByteTrackEngine(ByteTrackConfig(kalman="xyah"), S, 0)                          # ByteTrack: no ReID, no keypoint term, no GMC
    refused(x, L.ss_byte_set_reid(x.ctx, 1, 0.5, 0.25, 0.9), "ss_byte_set_reid: ReID needs the xywh (BoT-SORT) state")
    refused(x, L.ss_byte_set_pose(x.ctx, 1, 17, sg, 0.5, 0.25, 0.5, 3), "ss_byte_set_pose: the keypoint term needs the xywh (BoT-SORT) state")
    refused(x, L.ss_byte_set_gmc(x.ctx, _ptr(torch.zeros(1, S, 8, dtype=torch.float64, device=DEV))), "ss_byte_set_gmc: GMC needs the xywh (BoT-SORT) state")
    u = updates(x)
    refused(x, u["kpts"](), "ss_byte_update_group_kpts: the keypoint term is off (ss_byte_set_pose)")
    refused(x, u["obb"](), "ss_byte_update_group_obb: oriented boxes are off (ss_byte_set_obb)")
    assert u["plain"]() == lib.SS_OK and u["feats"]() == lib.SS_OK                     # features are not read without ReID
    x.set_obb(True)                                                                     # oriented boxes on: neither ReID nor the keypoint term
    refused(x, u["feats"](), "ss_byte_update_group_feats: oriented boxes are on, the 11-column rows go through ss_byte_update_group_obb")
    x.close()
    o = ByteTrackEngine(ByteTrackConfig(**BOT), S, 0, obb=True)
    refused(o, L.ss_byte_set_reid(o.ctx, 1, 0.5, 0.25, 0.9), "ss_byte_set_reid: oriented boxes are on (ss_byte_set_obb): the two are not combined")
    refused(o, L.ss_byte_set_pose(o.ctx, 1, 17, sg, 0.5, 0.25, 0.5, 3), "ss_byte_set_pose: oriented boxes are on (ss_byte_set_obb): the two are not combined")
    assert updates(o)["obb"]() == lib.SS_OK
    o.close()
    r = ByteTrackEngine(ByteTrackConfig(with_reid=True, **BOT), S, 0)                   # ReID on
    u = updates(r)
    refused(r, u["plain"](), "ss_byte_update_group: ReID is on, the features go through ss_byte_update_group_feats")
    refused(r, L.ss_byte_update_group_feats(r.ctx, 1, _ptr(d6), _ptr(n1), None, _ptr(o8), _ptr(n1)), "ss_byte_update_group_feats: ReID is on and d_feats is NULL")
    refused(r, u["kpts"](), "the keypoint term is off")
    refused(r, u["obb"](), "oriented boxes are off")
    refused(r, L.ss_byte_set_obb(r.ctx, 1), "ss_byte_set_obb: ReID, the keypoint term or GMC is on")
    assert u["feats"]() == lib.SS_OK
    r.check_errors()
    r.close()
