// ss_ocsort.hip — the OC-SORT tracker on the device (docs/OCSORT.md): S independent streams, a GROUP of F <= SS_FMAX frames per call.
//
//   k_ocsort_group  one workgroup (256 threads) per stream walks the group's frames in order inside the launch: score split,
//                   predict of every track (7-state SORT filter), the first association (IoU + the momentum term; upstream's
//                   shortcut when every row and track has at most one partner, else the one-wave LSAP), the optional BYTE stage
//                   on the low-score rows, the recovery stage (OCR) against the tracks' last observations, the Kalman updates
//                   with the observation-centric re-update (ORU) of a track re-found after a gap, births, the list rebuild and
//                   the output rows.  One launch per call, no host round trip: capturable.
//
// The frame procedure and its step bodies are ss_ocsort_body.h's, shared with Deep OC-SORT (csrc/ss_deepoc.hip); this kernel is the
// instantiation without the appearance and camera-motion steps.
#include "ss_ocsort_body.h"

__global__ __launch_bounds__(256) void k_ocsort_group(SSOcDev o, int F, const float* __restrict__ dets, const int* __restrict__ ndets,
                                                      float* __restrict__ out, int* __restrict__ nout)
{
    __shared__ OcLds m;
    oc_group<false>(o, nullptr, nullptr, F, dets, ndets, out, nout, m);
}

void ss_launch_ocsort_group(const SSOcDev& o, int F, const float* dets, const int* ndets, float* out, int* nout, hipStream_t st)
{
    hipLaunchKernelGGL(k_ocsort_group, dim3(o.S), dim3(256), 0, st, o, F, dets, ndets, out, nout);
}

// ---- host side: the state of a context.  What works on an SSOcDev (ss_oc_*) serves Deep OC-SORT's state as well. --------------------
struct SSOc {
    SSOcDev dev;
    SsBuf<SS_DEVICE> buf;               // every table of dev
};

void ss_ocsort_free(SSOc* o) { delete o; }
const SSOcDev& ss_ocsort_dev(const SSOc* o) { return o->dev; }

// the error words [S] of a tracker family, for ss_check_errors: SS_OK, or the code of the first stream that has one
int ss_tracker_pending_impl(const int* d_err, int S, hipStream_t st, const char* family, std::string& err)
{
    std::vector<int> e(S);
    SS_HIPCHK("ss_check_errors: ", hipMemcpyAsync(e.data(), d_err, e.size() * 4, hipMemcpyDeviceToHost, st));
    SS_HIPCHK("ss_check_errors: ", hipStreamSynchronize(st));
    for (size_t s = 0; s < e.size(); ++s)
        if (e[s]) { err = std::string(family) + ": device error flag on stream " + std::to_string(s); return e[s]; }
    return SS_OK;
}

int ss_ocsort_pending_impl(SSOc* o, hipStream_t st, std::string& err) { return o ? ss_tracker_pending_impl(o->dev.err, o->dev.S, st, "OC-SORT tracker", err) : (int)SS_OK; }

// the tables of an OC-SORT state (o.S set) out of buf, zeroed
int ss_oc_carve_impl(SSOcDev& o, SsBuf<SS_DEVICE>& buf, hipStream_t st, const char* who, std::string& err)
{
    const size_t S = o.S, T = SS_MAXT;
    SsCarve c;
    c.add(&o.frame, S); c.add(&o.next_id, S); c.add(&o.err, S); c.add(&o.n_trk, S);
    c.add(&o.trk, S * T);
    c.add(&o.tid, S * T); c.add(&o.age, S * T); c.add(&o.tsu, S * T); c.add(&o.hits, S * T); c.add(&o.streak, S * T); c.add(&o.hasobs, S * T);
    c.add(&o.obsd, S * T); c.add(&o.frozen, S * T); c.add(&o.det, S * T);
    c.add(&o.score, S * T); c.add(&o.cls, S * T); c.add(&o.lobs, S * T * 4);
    c.add(&o.ring, S * T * SS_OC_MAXDT * 4); c.add(&o.rage, S * T * SS_OC_MAXDT); c.add(&o.vel, S * T * 2);
    c.add(&o.x, S * T * 7); c.add(&o.P, S * T * 49); c.add(&o.xf, S * T * 7); c.add(&o.Pf, S * T * 49); c.add(&o.spill, S * T * SS_MAXD);
    SS_HIPCHK(who, c.carve(buf, st));
    return SS_OK;
}

// the streams' lists, counters and error words restart; synchronises
int ss_oc_reset_impl(const SSOcDev& o, hipStream_t st, int stream, const char* who, std::string& err)
{
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? o.S : stream + 1;
    const std::vector<int> ones(o.S, 1);
    SS_HIPCHK(who, hipMemsetAsync(o.frame + s0, 0, (s1 - s0) * 4, st));
    SS_HIPCHK(who, hipMemsetAsync(o.err + s0, 0, (s1 - s0) * 4, st));
    SS_HIPCHK(who, hipMemsetAsync(o.n_trk + s0, 0, (s1 - s0) * 4, st));
    SS_HIPCHK(who, hipMemcpyAsync(o.next_id + s0, ones.data(), (s1 - s0) * 4, hipMemcpyHostToDevice, st));
    SS_HIPCHK(who, hipStreamSynchronize(st));
    return SS_OK;
}

// Synchronous: the table of one stream in list order.  slots (may be NULL): the list's slots, for a caller that gathers more.
int ss_oc_get_tracks_impl(const SSOcDev& o, hipStream_t st, const char* entry, int s, int cap, int* n_tracks, int* next_id, int* frame_count,
                          int* track_id, int* age, int* time_since_update, int* hits, int* hit_streak, int* frozen, double* x, double* P,
                          float* last_obs, double* velocity, std::vector<int>* slots, std::string& err)
{
    const std::string who = std::string(entry) + ": ";
    SS_HIPCHK(who, hipStreamSynchronize(st));
    int nt = 0, nid = 0, fr = 0;
    SS_HIPCHK(who, hipMemcpy(&nt, o.n_trk + s, 4, hipMemcpyDeviceToHost));
    SS_HIPCHK(who, hipMemcpy(&nid, o.next_id + s, 4, hipMemcpyDeviceToHost));
    SS_HIPCHK(who, hipMemcpy(&fr, o.frame + s, 4, hipMemcpyDeviceToHost));
    if (n_tracks) *n_tracks = nt;                                    // the counts also when cap is too small: the caller sizes by them
    if (next_id) *next_id = nid;
    if (frame_count) *frame_count = fr;
    if (nt < 0 || nt > SS_MAXT) { err = who + "corrupt list"; return SS_ERR_CAPACITY; }
    if (nt > cap) { err = who + "cap too small"; return SS_ERR_CAPACITY; }
    const size_t T = SS_MAXT, sb = (size_t)s * T;
    std::vector<int> trk(T), has(nt);
    SS_HIPCHK(who, hipMemcpy(trk.data(), o.trk + sb, T * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < nt; ++i)
        if (trk[i] < 0 || trk[i] >= SS_MAXT) { err = who + "corrupt list"; return SS_ERR_CAPACITY; }
    const int* const isrc[6] = {o.tid, o.age, o.tsu, o.hits, o.streak, o.frozen};
    int* const idst[6] = {track_id, age, time_since_update, hits, hit_streak, frozen};
    for (int k = 0; k < 6; ++k) SS_HIPCHK(who, ss_gather_device(trk.data(), nt, isrc[k] + sb, T, 1, idst[k]));
    SS_HIPCHK(who, ss_gather_device(trk.data(), nt, o.x + sb * 7, T, 7, x));
    SS_HIPCHK(who, ss_gather_device(trk.data(), nt, o.P + sb * 49, T, 49, P));
    SS_HIPCHK(who, ss_gather_device(trk.data(), nt, o.vel + sb * 2, T, 2, velocity));
    SS_HIPCHK(who, ss_gather_device(trk.data(), nt, o.lobs + sb * 4, T, 4, last_obs));
    if (last_obs) SS_HIPCHK(who, ss_gather_device(trk.data(), nt, o.hasobs + sb, T, 1, has.data()));
    for (int i = 0; last_obs && i < nt; ++i)                         // a track without an observation: -1
        if (!has[i]) for (int k = 0; k < 4; ++k) last_obs[i * 4 + k] = -1.0f;
    if (slots) slots->assign(trk.begin(), trk.begin() + nt);
    return SS_OK;
}

int ss_ocsort_create_check_impl(const ss_ocsort_config* cfg, std::string& err)
{
    if (!cfg) { err = "ss_ocsort_create: null argument"; return SS_ERR_INVALID; }
    if (cfg->max_tracks < 1 || cfg->max_tracks > SS_MAXT || cfg->max_dets < 1 || cfg->max_dets > SS_MAXD || cfg->delta_t < 1 ||
        cfg->delta_t > SS_OC_MAXDT || cfg->max_age < 1 || cfg->min_hits < 0 || !(cfg->iou_threshold > 0.0 && cfg->iou_threshold <= 1.0) ||
        !(cfg->inertia >= 0.0) || !(cfg->low_thresh <= cfg->det_thresh) || (cfg->use_byte != 0 && cfg->use_byte != 1)) {
        err = "ss_ocsort_create: 1 <= max_tracks <= 256, 1 <= max_dets <= 128, 1 <= delta_t <= 8, max_age >= 1, "
              "min_hits >= 0, 0 < iou_threshold <= 1, inertia >= 0, low_thresh <= det_thresh, use_byte 0 / 1";
        return SS_ERR_INVALID;
    }
    return SS_OK;
}

// the caller has drained the stream and freed the state this one replaces: a failure leaves none attached
int ss_ocsort_create_impl(SSOc** po, hipStream_t st, int S, const ss_ocsort_config* cfg, std::string& err)
{
    std::unique_ptr<SSOc> O(new SSOc());
    SSOcDev& o = O->dev;
    memset(&o, 0, sizeof o);
    o.S = S;
    o.max_age = cfg->max_age; o.min_hits = cfg->min_hits; o.delta_t = cfg->delta_t; o.use_byte = cfg->use_byte;
    o.max_tracks = cfg->max_tracks; o.max_dets = cfg->max_dets;
    o.det_thresh = (float)cfg->det_thresh; o.low_thresh = (float)cfg->low_thresh;
    o.iou_thr = cfg->iou_threshold; o.inertia = cfg->inertia;
    if (const int rc = ss_oc_carve_impl(o, O->buf, st, "ss_ocsort_create: ", err)) return rc;
    if (const int rc = ss_oc_reset_impl(o, st, -1, "ss_ocsort_create: ", err)) return rc;
    *po = O.release();
    return SS_OK;
}
