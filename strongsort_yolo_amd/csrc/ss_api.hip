// ss_api.hip — C ABI (include/strongsort_hip.h) over the gfx950 kernels.  No torch types, no
// exceptions across the boundary; the context owns all device-resident tracker state.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "ss_common.h"
#include "ss_host.h"
#include "ss_launch.h"

static std::string g_last_error;

struct ss_ctx {
    ss_config cfg;
    SSParams prm;
    SSDev dev;
    int device;
    hipStream_t stream;
    std::vector<void*> allocs;
    std::string err;
    // staging for the host convenience path
    float *d_dets, *d_feats, *d_out;
    int *d_ndets, *d_imghw, *d_nout;
    // KAT scratch
    float *kat_featfrag, *kat_partmin;
    double* kat_lsap_t;
    int* kat_err;
    void* nms_ws;               // nms_units workspace units (grown on demand outside graph capture)
    size_t nms_ws_bytes;
    int nms_units;
    unsigned long long cls_mask[2];   // classes the NMS keeps (ss_nms_set_classes); all ones = every class
    // host -> device upload staging (ss_upload): write-combined pinned buffers, used round robin
    struct Stage { SsBuf<SS_PINNED_WC> buf; SsEvent ev; bool busy = false; int acquire(ss_ctx* c, size_t bytes); } stage[4];
    int stage_next = 0;
    Stage bstage[2];            // ss_upload_batch: a whole frame group per staging area
    int bstage_next = 0;
    uint8_t* font;              // [95][5] overlay font (ss_overlay_set_font)
    // N4 camera-motion compensation
    uint8_t* cmc_small;         // [FMAX+1][S][cmc_stride] down-scaled grey frames (index 0 = last frame of the previous group)
    size_t cmc_stride;          // bytes per small image (multiple of 16), 0 until the first ss_cmc_estimate
    int cmc_hw[2];              // frame size the buffer was made for
    int cmc_frames;             // n_frames of the last ss_cmc_estimate (what ss_cmc_get_small may read)
    int* cmc_prev_valid;        // [S]
    const double* cmc_warps;    // what ss_track_set_cmc installed
    SSGmcDev gmc;               // sparse-optical-flow estimator (ss_gmc.hip); gmc.h == 0 until the first ss_gmc_sparse_estimate
    hipEvent_t assoc_event;     // what ss_track_set_assoc_event installed (recorded after every association launch)
    SsBuf<SS_PINNED> back;      // device -> host staging (ss_download)
    int cos_grid;               // persistent workgroups of the association kernel
    int comp_rows;              // ragged last tiles with at most this many rows travel as 4-row groups of composite tiles (0: never)
    int assoc_stage;            // staging of the association kernel's detection operand (SSDev.assoc_stage)
    int xcd_map;                // SSDev.xcd_map
    int inkernel;               // in-kernel timing of the association kernel: 0 off, 1 duration, 2 + timeline
    // association-kernel timing
    bool timing;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    size_t ev_used;
    std::vector<float> ev_ms;   // the durations behind the last ss_assoc_timing mean
    // the per-frame chain of a group (3 F - 1 launches) as captured HIP graphs, one per distinct kernel-argument set
    struct Chain { std::vector<char> key; hipGraph_t graph; hipGraphExec_t exec; unsigned long long used; hipStream_t last_st; };   // last_st: the stream of its last replay
    std::vector<Chain> chains;
    hipStream_t cap_stream;     // capture-only stream (nothing ever executes on it)
    int track_graph;            // option "track_graph": 1 (default) replay the chain as a graph for groups of >= 2 frames, 0 plain launches
    unsigned long long chain_clock;
    std::vector<unsigned long long> chain_seen;   // hashes of argument sets launched plainly once
    // option "chain_cus": the per-frame chain runs on a stream of its own that owns the first `chain_cus` compute units of the
    // CU mask (see ss_stream_create) instead of on the caller's stream
    int chain_cus;
    hipStream_t chain_stream;
    hipEvent_t ev_head, ev_chain;
    bool chain_pending;
    SSByte* byte = nullptr;     // the BYTE tracker family (ss_byte_create), NULL until attached
    SSOc* oc = nullptr;         // the OC-SORT tracker (ss_ocsort_create), NULL until attached
    SSDeepOc* deepoc = nullptr; // the Deep OC-SORT tracker (ss_deepoc_create), NULL until attached
    SSHybrid* hybrid = nullptr; // the Hybrid-SORT tracker (ss_hybridsort_create), NULL until attached
    SSJpeg* jpeg = nullptr;     // ss_jpeg_decode_batch's staging areas and planes, made by its first call
    SSJpegEnc* jpeg_enc = nullptr;   // ss_jpeg_encode_batch's buffers, made by its first call
    SSGsi* gsi = nullptr;       // ss_gsi_smooth's staging and scratch slots, made by its first call
    SSMot* mot = nullptr;       // ss_mot_eval's and ss_mot_identity's staging, scratch and second stream, made by its first call
    SSAp* ap = nullptr;         // ss_ap_eval's staging and scratch, made by its first call
    SSAflink* aflink = nullptr; // ss_aflink_*'s weights, staging and activation scratch, made by its first call
    SSZone* zone = nullptr;     // the analytics stage (ss_zone_create), NULL until attached
    SSBank* bank = nullptr;     // the track bank (ss_bank_create), NULL until attached
    SSMtmc* mtmc = nullptr;     // ss_mtmc_link's scratch, made by its first call
    SSSlice* slice = nullptr;   // sliced inference (ss_slice_config): tile table, NMS geometry, merge workspace; NULL until configured
};

static int fail(ss_ctx* c, int code, const std::string& msg)
{
    g_last_error = msg;
    if (c) c->err = msg;
    return code;
}

#define HIPCHK(c, x)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess)                                                               \
            return fail(c, SS_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));     \
    } while (0)

template <typename T>
static int dalloc(ss_ctx* c, T** p, size_t n, bool zero = true)
{
    void* q = nullptr;
    HIPCHK(c, hipMalloc(&q, n * sizeof(T)));
    if (zero) HIPCHK(c, hipMemsetAsync(q, 0, n * sizeof(T), c->stream));
    c->allocs.push_back(q);
    *p = (T*)q;
    return SS_OK;
}

// CU masks: bit i of the mask = compute unit i / n_xcd of XCD i % n_xcd (the driver deals the bits of a queue's mask out to the
// XCDs in turn), so the first 8 k bits are k compute units of every XCD.
static int cu_mask_stream(ss_ctx* c, int first, int count, hipStream_t* out)
{
    hipDeviceProp_t prop;
    HIPCHK(c, hipGetDeviceProperties(&prop, c ? c->device : 0));
    const int total = prop.multiProcessorCount;
    if (first < 0 || count < 1 || first + count > total) return fail(c, SS_ERR_INVALID, "CU mask: range outside the device's compute units");
    std::vector<uint32_t> mask((total + 31) / 32, 0u);
    for (int i = first; i < first + count; ++i) mask[i >> 5] |= 1u << (i & 31);
    HIPCHK(c, hipExtStreamCreateWithCUMask(out, (uint32_t)mask.size(), mask.data()));
    return SS_OK;
}

// a later launch on `s` sees what the detached chain wrote (no-op when nothing is detached)
static int chain_join(ss_ctx* c, hipStream_t s)
{
    if (c->chain_pending) HIPCHK(c, hipStreamWaitEvent(s, c->ev_chain, 0));
    return SS_OK;
}

extern "C" const char* ss_last_error(const ss_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

extern "C" int ss_create(const ss_config* cfg, int device, ss_ctx** out)
{
    if (!cfg || !out) return fail(nullptr, SS_ERR_INVALID, "ss_create: null argument");
    if (cfg->n_streams < 1 || cfg->nn_budget < 1 || cfg->nn_budget > SS_NRT * SS_TILE)
        return fail(nullptr, SS_ERR_INVALID, "ss_create: n_streams >= 1 and 1 <= nn_budget <= 128 required");
    ss_ctx* c = new ss_ctx();
    c->cfg = *cfg;
    c->device = device;
    c->stream = nullptr;
    c->timing = false;
    c->ev_used = 0;
    c->cos_grid = 512;           // persistent workgroups of the association kernel: two per CU
    c->comp_rows = 12;
    c->assoc_stage = 5;          // LDS-DMA in four pieces, first piece + first gallery piece only before the first barrier (r04: 37.8 -> 36.4 us per 1 x 32-frame launch)
    c->xcd_map = 0;
    c->cap_stream = nullptr; c->track_graph = 1; c->chain_clock = 0;
    c->chain_cus = 0; c->chain_stream = nullptr; c->ev_head = c->ev_chain = nullptr; c->chain_pending = false;
    c->inkernel = 0;
    c->cls_mask[0] = c->cls_mask[1] = ~0ull;
    memset(&c->gmc, 0, sizeof c->gmc);
    c->cmc_small = nullptr; c->cmc_stride = 0; c->cmc_hw[0] = c->cmc_hw[1] = 0; c->cmc_frames = 0; c->cmc_warps = nullptr; c->assoc_event = nullptr;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { int r = fail(nullptr, SS_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e)); delete c; return r; }
    SSParams& p = c->prm;
    p.max_dist = cfg->max_dist; p.max_iou_distance = cfg->max_iou_distance; p.mc_lambda = cfg->mc_lambda;
    p.gating_threshold = cfg->gating_threshold; p.gated_cost = cfg->gated_cost;
    p.wp = cfg->std_weight_position; p.wv = cfg->std_weight_velocity;
    p.ema_alpha = (float)cfg->ema_alpha; p.ema_one_minus_alpha = (float)(1.0 - cfg->ema_alpha);
    p.max_age = cfg->max_age; p.n_init = cfg->n_init; p.nn_budget = cfg->nn_budget; p.debug = cfg->debug;
    const size_t S = cfg->n_streams, T = SS_MAXT, D = SS_MAXD;
    SSDev& d = c->dev;
    memset(&d, 0, sizeof d);
    d.S = (int)S;
    d.budget = cfg->nn_budget;
    d.cap_cost = SS_COST_CAP; d.cap_t = SS_MAXT; d.cap_d = SS_MAXD;
    d.chain_merge = 1;
    d.pred_ahead = 1;
    d.assoc_pack = 1;
    int rc = SS_OK;
#define A(field, n) if (rc == SS_OK) rc = dalloc(c, &d.field, (n))
    A(n_tracks, S); A(next_id, S); A(frame, S); A(err, S); A(order, S * T);
    A(slot_used, S * T); A(track_id, S * T); A(state, S * T); A(hits, S * T); A(age, S * T); A(tsu, S * T);
    A(class_id, S * T); A(det_idx, S * T); A(gal_count, S * T); A(gal_head, S * T); A(conf, S * T);
    A(mean, S * T * 8); A(cov, S * T * 64); A(mean_p, S * T * 8); A(cov_p, S * T * 64); A(smooth, S * T * 2 * SS_F); A(smooth_sel, S * T);
    A(gallery, S * T * SS_NRT * SS_TILE_FLOATS);
    const size_t FM = SS_FMAX;
    A(feat_unit, FM * S * D * SS_F); A(feat_frag, FM * S * SS_NCT * SS_TILE_FLOATS);
    A(feat_pack, S * SS_NCTP * SS_TILE_FLOATS); A(colmap, S * (FM * D + 64));
    A(tlwh, FM * S * D * 4); A(xyah, FM * S * D * 4);
    A(M, S * T * FM * D); A(pl, S * SS_PLMAX); A(n_pl, S); A(pf, S * (FM + 1));
    d.items_cap = (int)(S * 4096);        // records per XCD list (<= F * max(cos_grid / (S F), pairs * ceil(tiles / SS_RECT)) per stream, spread over 8 lists)
    A(items, 8 * (size_t)d.items_cap * SS_RECI4); A(n_items, 8);
    A(post, S * T); A(n_post, S); A(rowlist, S * T); A(n_rows, S); A(cost_spill, S * T * D); A(frame_scratch, S * (T * 18 + D * 8)); A(tstamp, 4); A(timeline, 4096 * 16);
    if (cfg->debug) {
        A(dbg_cos, FM * S * T * D); A(dbg_maha, FM * S * T * D); A(dbg_cost_a, FM * S * T * D); A(dbg_cost_b, FM * S * T * D);
        A(dbg_gated, FM * S * T * D); A(dbg_lists, FM * S * 4 * T); A(dbg_counts, FM * S * 8);
    }
#undef A
    if (rc == SS_OK) rc = dalloc(c, &c->d_dets, S * D * 6);
    if (rc == SS_OK) rc = dalloc(c, &c->d_feats, S * D * SS_F);
    if (rc == SS_OK) rc = dalloc(c, &c->d_out, S * T * 8);
    if (rc == SS_OK) rc = dalloc(c, &c->d_ndets, S);
    if (rc == SS_OK) rc = dalloc(c, &c->d_imghw, S * 2);
    if (rc == SS_OK) rc = dalloc(c, &c->d_nout, S);
    if (rc == SS_OK) rc = dalloc(c, &c->kat_featfrag, (size_t)SS_NCT * SS_TILE_FLOATS);
    if (rc == SS_OK) rc = dalloc(c, &c->kat_partmin, T * SS_NRT * D);
    if (rc == SS_OK) rc = dalloc(c, &c->kat_lsap_t, (size_t)256 * 256);
    if (rc == SS_OK) rc = dalloc(c, &c->kat_err, 4);
    if (rc == SS_OK) rc = dalloc(c, &c->font, 95 * 5);
    if (rc == SS_OK) rc = dalloc(c, &c->cmc_prev_valid, S);
    if (rc == SS_OK) rc = dalloc(c, &c->gmc.prev_valid, S);
    if (rc == SS_OK) rc = dalloc(c, &c->gmc.last, 1);
    c->nms_ws_bytes = ss_nms_workspace_bytes();
    c->nms_units = 1;
    if (rc == SS_OK) { char* w; rc = dalloc(c, &w, c->nms_ws_bytes); c->nms_ws = w; }
    if (rc == SS_OK) { ss_step_kernel_attr(); if (ss_front_init() != 0) rc = fail(c, SS_ERR_HIP, "kernel attribute setup failed"); }
    if (rc == SS_OK) { hipError_t e2 = hipStreamSynchronize(c->stream); if (e2 != hipSuccess) rc = fail(c, SS_ERR_HIP, hipGetErrorString(e2)); }
    if (rc != SS_OK) { std::string m = c->err; ss_destroy(c); g_last_error = m; return rc; }
    // next_id starts at 1
    std::vector<int> ones(S, 1);
    hipError_t e3 = hipMemcpy(d.next_id, ones.data(), S * sizeof(int), hipMemcpyHostToDevice);
    if (e3 != hipSuccess) { int r = fail(nullptr, SS_ERR_HIP, std::string("ss_create: ") + hipGetErrorString(e3)); ss_destroy(c); return r; }
    *out = c;
    return SS_OK;
}

extern "C" void ss_destroy(ss_ctx* c)
{
    if (!c) return;
    // teardown: nothing useful can be done with an error here
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (auto& e : c->ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (auto& g : c->chains) { (void)hipGraphExecDestroy(g.exec); (void)hipGraphDestroy(g.graph); }
    if (c->cap_stream) (void)hipStreamDestroy(c->cap_stream);
    if (c->chain_stream) { (void)hipStreamSynchronize(c->chain_stream); (void)hipStreamDestroy(c->chain_stream); }
    if (c->ev_head) (void)hipEventDestroy(c->ev_head);
    if (c->ev_chain) (void)hipEventDestroy(c->ev_chain);
    for (void* p : c->allocs) (void)hipFree(p);
    ss_byte_free(c->byte);
    ss_ocsort_free(c->oc);
    ss_deepoc_free(c->deepoc);
    ss_hybrid_free(c->hybrid);
    ss_jpeg_free(c->jpeg);
    ss_jpeg_enc_free(c->jpeg_enc);
    ss_gsi_free(c->gsi);
    ss_mot_free(c->mot);
    ss_ap_free(c->ap);
    ss_aflink_free(c->aflink);
    ss_zone_free(c->zone);
    ss_bank_free(c->bank);
    ss_mtmc_free(c->mtmc);
    ss_slice_free(c->slice);
    delete c;                   // (the staging areas of ss_upload, ss_upload_batch and ss_download go with it)
}

extern "C" int ss_set_hip_stream(ss_ctx* c, void* s)
{
    if (!c) return SS_ERR_INVALID;
    c->stream = (hipStream_t)s;
    return SS_OK;
}

// What an upload does before it fills a staging area: the area's previous upload has left it, it holds `bytes`, its event exists
int ss_ctx::Stage::acquire(ss_ctx* c, size_t bytes)
{
    if (busy) { HIPCHK(c, hipEventSynchronize(ev)); busy = false; }
    HIPCHK(c, buf.reserve(bytes, SS_EXACT));
    HIPCHK(c, ev.ensure());
    return SS_OK;
}

// Frame upload: the caller's pageable buffer -> write-combined pinned staging (streaming CPU stores, no cache snooping
// on the DMA read) -> device, asynchronous on `hip_stream`.  Measured on the MI355X box for a 1280x720x3 frame: a
// cacheable pinned buffer costs 3.6 ms to fill + 2.8 ms to DMA right after the CPU wrote it; pageable hipMemcpy 1.7 ms.
extern "C" int ss_upload(ss_ctx* c, void* hip_stream, void* d_dst, const void* h_src, size_t bytes)
{
    if (!c || !d_dst || !h_src) return fail(c, SS_ERR_INVALID, "ss_upload: null argument");
    if (bytes == 0) return SS_OK;
    ss_ctx::Stage& st = c->stage[c->stage_next];
    c->stage_next = (c->stage_next + 1) & 3;
    if (int rc = st.acquire(c, bytes)) return rc;
    memcpy(st.buf.as(), h_src, bytes);
    HIPCHK(c, hipMemcpyAsync(d_dst, st.buf.as(), bytes, hipMemcpyHostToDevice, (hipStream_t)hip_stream));
    HIPCHK(c, hipEventRecord(st.ev, (hipStream_t)hip_stream));
    st.busy = true;
    return SS_OK;
}

// A group of frames at once: the n host buffers (bytes_each each) are copied into ONE write-combined staging area by `threads`
// host threads (a single thread fills write-combined memory at ~30 GB/s: 0.09 ms per 720p frame, 2.9 ms for a group of 32 — more
// than the GPU needs for the group), then leave in one asynchronous copy to d_dst (the frames contiguous there).  Two staging
// areas alternate; h_srcs may be reused on return.
extern "C" int ss_upload_batch(ss_ctx* c, void* hip_stream, void* d_dst, const void* const* h_srcs, int n, size_t bytes_each, int threads)
{
    if (!c || !d_dst || !h_srcs || n < 0 || threads < 1) return fail(c, SS_ERR_INVALID, "ss_upload_batch: bad argument");
    if (n == 0 || bytes_each == 0) return SS_OK;
    for (int i = 0; i < n; ++i) if (!h_srcs[i]) return fail(c, SS_ERR_INVALID, "ss_upload_batch: null frame");
    ss_ctx::Stage& st = c->bstage[c->bstage_next];                  // (the area is taken for good only when the copy has been enqueued)
    const size_t bytes = (size_t)n * bytes_each;
    if (int rc = st.acquire(c, bytes)) return rc;
    // small groups are not worth the threads' start + join (tens of microseconds); nothing the standard library throws
    // (std::system_error when no thread can be started, bad_alloc) may cross the C boundary: run_threads sees to that
    int T = threads < n ? threads : n;
    if (bytes < (size_t)4 << 20) T = 1;
    char* base = st.buf.as();
    auto work = [=](int t, int nt) { for (int i = t; i < n; i += nt) memcpy(base + (size_t)i * bytes_each, h_srcs[i], bytes_each); };
    if (!run_threads(T, work)) return fail(c, SS_ERR_INVALID, "ss_upload_batch: host staging failed");
    HIPCHK(c, hipMemcpyAsync(d_dst, base, bytes, hipMemcpyHostToDevice, (hipStream_t)hip_stream));
    HIPCHK(c, hipEventRecord(st.ev, (hipStream_t)hip_stream));
    st.busy = true;
    c->bstage_next ^= 1;
    return SS_OK;
}

// ---- N3 frame source: baseline JPEG (ss_jpeg.hip) ----------------------------------------------------------
extern "C" int ss_jpeg_probe(const unsigned char* data, size_t size, int* width, int* height, int* components, int* h_samp, int* v_samp)
{
    if (!data || !size || !width || !height || !components || !h_samp || !v_samp) return fail(nullptr, SS_ERR_INVALID, "ss_jpeg_probe: null argument");
    std::string err;
    const int rc = ss_jpeg_probe_impl(data, size, width, height, components, h_samp, v_samp, err);
    return rc == SS_OK ? rc : fail(nullptr, rc, "ss_jpeg_probe: " + err);
}

extern "C" int ss_jpeg_coefficients(const unsigned char* data, size_t size, short* coef, size_t coef_cap, unsigned short* quant)
{
    if (!data || !size || !coef || !quant) return fail(nullptr, SS_ERR_INVALID, "ss_jpeg_coefficients: null argument");
    std::string err;
    const int rc = ss_jpeg_coefficients_impl(data, size, coef, coef_cap, quant, err);
    return rc == SS_OK ? rc : fail(nullptr, rc, "ss_jpeg_coefficients: " + err);
}

// ss_jpeg_decode_batch and ss_jpeg_decode_batch_device: one set of checks, the messages under the caller's name
static int jpeg_decode_checks(ss_ctx* c, const std::string& who, const unsigned char* const* data, const size_t* sizes, int n, int height, int width,
                              const void* d_out, long long out_frame_stride, int rgb, int threads)
{
    if (!c || !data || !sizes || !d_out) return fail(c, SS_ERR_INVALID, who + ": null argument");
    if (n < 1 || n > 64 || threads < 1 || threads > 16 || height < 1 || height > 8192 || width < 1 || width > 8192 || (rgb != 0 && rgb != 1) ||
        out_frame_stride < (long long)height * width * 3)
        return fail(c, SS_ERR_INVALID, who + ": 1 <= n <= 64, 1 <= threads <= 16, sides 1 .. 8192, rgb 0 / 1, out_frame_stride >= height * width * 3");
    for (int i = 0; i < n; ++i) if (!data[i] || !sizes[i]) return fail(c, SS_ERR_INVALID, who + ": image " + std::to_string(i) + ": no data");
    return SS_OK;
}

extern "C" int ss_jpeg_decode_batch(ss_ctx* c, void* hip_stream, const unsigned char* const* data, const size_t* sizes, int n, int height,
                                    int width, void* d_out, long long out_frame_stride, int rgb, int threads)
{
    if (const int bad = jpeg_decode_checks(c, "ss_jpeg_decode_batch", data, sizes, n, height, width, d_out, out_frame_stride, rgb, threads)) return bad;
    std::string err;
    const int rc = ss_jpeg_decode_impl(&c->jpeg, (hipStream_t)hip_stream, data, sizes, n, height, width, d_out, out_frame_stride, rgb, threads, err);
    return rc == SS_OK ? rc : fail(c, rc, err);
}

// The entropy stage on the device (docs/JPEG.md section 12): ss_jpeg_decode_batch's arguments and checks
extern "C" int ss_jpeg_decode_batch_device(ss_ctx* c, void* hip_stream, const unsigned char* const* data, const size_t* sizes, int n, int height,
                                           int width, void* d_out, long long out_frame_stride, int rgb, int threads)
{
    if (const int bad = jpeg_decode_checks(c, "ss_jpeg_decode_batch_device", data, sizes, n, height, width, d_out, out_frame_stride, rgb, threads)) return bad;
    std::string err;
    const int rc = ss_jpeg_decode_device_impl(&c->jpeg, (hipStream_t)hip_stream, data, sizes, n, height, width, d_out, out_frame_stride, rgb, threads, nullptr, 0, err);
    return rc == SS_OK ? rc : fail(c, rc, err);
}

extern "C" int ss_jpeg_scan_segments(const unsigned char* data, size_t size, unsigned char* bytes, size_t bytes_cap, size_t* bytes_used, unsigned int* segments,
                                     size_t seg_cap, int* n_segments, unsigned int* header)
{
    if (!data || !size || !bytes_used || !n_segments || (bytes && !segments)) return fail(nullptr, SS_ERR_INVALID, "ss_jpeg_scan_segments: null argument");
    std::string err;
    const int rc = ss_jpeg_scan_segments_impl(data, size, bytes, bytes_cap, bytes_used, segments, seg_cap, n_segments, header, err);
    return rc == SS_OK ? rc : fail(nullptr, rc, "ss_jpeg_scan_segments: " + err);
}

extern "C" int ss_jpeg_device_coefficients(ss_ctx* c, const unsigned char* data, size_t size, short* coef, size_t coef_cap)
{
    if (!c || !data || !size || !coef) return fail(c, SS_ERR_INVALID, "ss_jpeg_device_coefficients: null argument");
    std::string err;
    const int rc = ss_jpeg_decode_device_impl(&c->jpeg, c->stream, &data, &size, 1, 0, 0, nullptr, 0, 0, 1, coef, coef_cap, err);
    return rc == SS_OK ? rc : fail(c, rc, err);
}

extern "C" int ss_jpeg_device_rounds(ss_ctx* c, int* rounds, int cap)
{
    if (!c || (!rounds && cap > 0) || cap < 0) return fail(c, SS_ERR_INVALID, "ss_jpeg_device_rounds: bad argument");
    return ss_jpeg_device_rounds_impl(c->jpeg, rounds, cap);
}

// ---- N3 frame sink: baseline JPEG (ss_jpeg_enc.hip) --------------------------------------------------------
static const char* jpeg_enc_shape_error(int width, int height, int quality, int h_samp, int v_samp)
{
    if (width < 1 || width > 8192 || height < 1 || height > 8192) return "sides must be 1 .. 8192";
    if (quality < 1 || quality > 100) return "quality must be 1 .. 100";
    if (!((h_samp == 2 && v_samp == 2) || (h_samp == 2 && v_samp == 1) || (h_samp == 1 && v_samp == 1))) return "luma sampling must be 2x2, 2x1 or 1x1";
    return nullptr;
}

extern "C" long long ss_jpeg_encode_bound(int width, int height, int h_samp, int v_samp)
{
    if (const char* why = jpeg_enc_shape_error(width, height, 50, h_samp, v_samp)) return fail(nullptr, SS_ERR_INVALID, std::string("ss_jpeg_encode_bound: ") + why);
    return (long long)ss_jpeg_encode_bound_impl(width, height, h_samp, v_samp);
}

extern "C" int ss_jpeg_entropy_encode(const short* coef, int quality, int width, int height, int h_samp, int v_samp, unsigned char* out, size_t out_cap,
                                      size_t* out_size)
{
    if (!coef || !out || !out_size) return fail(nullptr, SS_ERR_INVALID, "ss_jpeg_entropy_encode: null argument");
    if (const char* why = jpeg_enc_shape_error(width, height, quality, h_samp, v_samp)) return fail(nullptr, SS_ERR_INVALID, std::string("ss_jpeg_entropy_encode: ") + why);
    const size_t bound = ss_jpeg_encode_bound_impl(width, height, h_samp, v_samp);
    if (out_cap < bound) return fail(nullptr, SS_ERR_INVALID, "ss_jpeg_entropy_encode: out_cap " + std::to_string(out_cap) + " is below the bound " + std::to_string(bound));
    std::string err;
    const int rc = ss_jpeg_entropy_encode_impl(coef, quality, width, height, h_samp, v_samp, out, out_size, err);
    return rc == SS_OK ? rc : fail(nullptr, rc, "ss_jpeg_entropy_encode: " + err);
}

// ss_jpeg_encode_batch and ss_jpeg_encode_batch_device: one set of checks, the messages under the caller's name
static int jpeg_encode_checks(ss_ctx* c, const std::string& who, const void* d_in, long long in_frame_stride, int n, int height, int width, int rgb, int quality,
                              int h_samp, int v_samp, int threads, unsigned char* const* out, const size_t* out_cap, size_t* out_size)
{
    if (!c || !d_in || !out || !out_cap || !out_size) return fail(c, SS_ERR_INVALID, who + ": null argument");
    if (n < 1 || n > 64) return fail(c, SS_ERR_INVALID, who + ": 1 <= n <= 64");
    if (threads < 1 || threads > 16) return fail(c, SS_ERR_INVALID, who + ": 1 <= threads <= 16");
    if (rgb != 0 && rgb != 1) return fail(c, SS_ERR_INVALID, who + ": rgb 0 / 1");
    if (const char* why = jpeg_enc_shape_error(width, height, quality, h_samp, v_samp)) return fail(c, SS_ERR_INVALID, who + ": " + why);
    if (n > 1 && in_frame_stride < (long long)height * width * 3) return fail(c, SS_ERR_INVALID, who + ": in_frame_stride >= height * width * 3");
    const size_t bound = ss_jpeg_encode_bound_impl(width, height, h_samp, v_samp);
    for (int i = 0; i < n; ++i) {
        if (!out[i]) return fail(c, SS_ERR_INVALID, who + ": image " + std::to_string(i) + ": null buffer");
        if (out_cap[i] < bound)
            return fail(c, SS_ERR_INVALID, who + ": image " + std::to_string(i) + ": out_cap " + std::to_string(out_cap[i]) + " is below the bound " + std::to_string(bound));
    }
    return SS_OK;
}

extern "C" int ss_jpeg_encode_batch(ss_ctx* c, void* hip_stream, const void* d_in, long long in_frame_stride, int n, int height, int width, int rgb,
                                    int quality, int h_samp, int v_samp, int threads, unsigned char* const* out, const size_t* out_cap, size_t* out_size)
{
    if (const int bad = jpeg_encode_checks(c, "ss_jpeg_encode_batch", d_in, in_frame_stride, n, height, width, rgb, quality, h_samp, v_samp, threads, out, out_cap, out_size))
        return bad;
    std::string err;
    const int rc = ss_jpeg_encode_impl(&c->jpeg_enc, (hipStream_t)hip_stream, d_in, in_frame_stride, n, height, width, rgb, quality, h_samp, v_samp, threads, out,
                                       out_size, err);
    return rc == SS_OK ? rc : fail(c, rc, err);
}

// The same call with the entropy stage on the device (docs/JPEG.md section 13): same arguments, same checks, same files
extern "C" int ss_jpeg_encode_batch_device(ss_ctx* c, void* hip_stream, const void* d_in, long long in_frame_stride, int n, int height, int width, int rgb,
                                           int quality, int h_samp, int v_samp, int threads, unsigned char* const* out, const size_t* out_cap, size_t* out_size)
{
    if (const int bad = jpeg_encode_checks(c, "ss_jpeg_encode_batch_device", d_in, in_frame_stride, n, height, width, rgb, quality, h_samp, v_samp, threads, out, out_cap,
                                           out_size))
        return bad;
    std::string err;
    const int rc = ss_jpeg_encode_device_impl(&c->jpeg_enc, (hipStream_t)hip_stream, d_in, in_frame_stride, n, height, width, rgb, quality, h_samp, v_samp, threads, out,
                                              out_size, err);
    return rc == SS_OK ? rc : fail(c, rc, err);
}

// The device entropy stage alone on one image's coefficients, for tests: ss_jpeg_entropy_encode's arguments and checks
extern "C" int ss_jpeg_entropy_encode_device(ss_ctx* c, const short* coef, int quality, int width, int height, int h_samp, int v_samp, unsigned char* out,
                                             size_t out_cap, size_t* out_size)
{
    if (!c || !coef || !out || !out_size) return fail(c, SS_ERR_INVALID, "ss_jpeg_entropy_encode_device: null argument");
    if (const char* why = jpeg_enc_shape_error(width, height, quality, h_samp, v_samp)) return fail(c, SS_ERR_INVALID, std::string("ss_jpeg_entropy_encode_device: ") + why);
    const size_t bound = ss_jpeg_encode_bound_impl(width, height, h_samp, v_samp);
    if (out_cap < bound)
        return fail(c, SS_ERR_INVALID, "ss_jpeg_entropy_encode_device: out_cap " + std::to_string(out_cap) + " is below the bound " + std::to_string(bound));
    std::string err;
    const int rc = ss_jpeg_entropy_encode_device_impl(&c->jpeg_enc, c->stream, coef, quality, width, height, h_samp, v_samp, out, out_size, err);
    return rc == SS_OK ? rc : fail(c, rc, err);
}

// ---- the post-run entries: GSI, HOTA / CLEAR MOT, identity metrics, AFLink ------------------------------------------------
// check(err) looks at the arguments first and needs no context; work(err) runs when it found nothing.  Both build vectors and strings
// sized by the caller's input and `work` makes the stage's state on first use: nothing they throw may cross the C boundary.
template <class Check, class Work>
static int post_run(ss_ctx* c, const char* entry, Check check, Work work)
{
    try {
        std::string err;
        int rc = check(err);
        if (rc != SS_OK) return fail(c, rc, err);
        rc = work(err);
        return rc == SS_OK ? rc : fail(c, rc, err);
    } catch (...) {
        return fail(c, SS_ERR_INVALID, std::string(entry) + ": out of memory");
    }
}

// The checks an entry of an attached stage (the zones, the bank, a tracker family) makes after its own arguments: a context, the
// stage's state (have_state), a stream of it.  what: the state and the entry that makes it, said after "no ".  one_wording (the
// trackers' reset and get entries): a missing context and a bad stream read "no <what>" as well.
static int stage_state(ss_ctx* c, const char* entry, bool have_state, const char* what, int stream, bool need_stream, std::string& err,
                       bool one_wording = false)
{
    const std::string who = std::string(entry) + ": ";
    const bool bad_stream = c && (stream >= c->dev.S || (need_stream && stream < 0));
    if (one_wording ? (!have_state || bad_stream) : (c && !have_state)) { err = who + "no " + what; return SS_ERR_INVALID; }
    if (!c) { err = who + "null context"; return SS_ERR_INVALID; }
    if (bad_stream) { err = who + "stream " + std::to_string(stream) + " out of range"; return SS_ERR_INVALID; }
    return SS_OK;
}

// A create entry of an attached stage: check(err) on its arguments; then a context with nothing of the state the call replaces still
// in flight, that state freed (a failure leaves none attached), and make(err)
template <class State, class Check, class Make>
static int create_run(ss_ctx* c, const char* entry, State* ss_ctx::*state, void (*release)(State*), Check check, Make make)
{
    return post_run(c, entry, check, [&](std::string& err) {
        if (!c) { err = std::string(entry) + ": null context"; return (int)SS_ERR_INVALID; }
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { err = std::string(entry) + ": " + hipGetErrorString(e); return (int)SS_ERR_HIP; }
        release(c->*state);
        c->*state = nullptr;
        return make(err);
    });
}

// What a destroy entry of an attached stage does: the stream drains, the state goes
template <class State>
static int stage_destroy(ss_ctx* c, const char* entry, State* ss_ctx::*state, void (*release)(State*))
{
    if (!c) return fail(nullptr, SS_ERR_INVALID, std::string(entry) + ": null context");
    if (!(c->*state)) return SS_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    release(c->*state);
    c->*state = nullptr;
    return SS_OK;
}

// ---- GSI post-processing (ss_gsi.hip, docs/GSI.md) ------------------------------------------------------------
extern "C" int ss_gsi_max_len(void) { return ss_gsi_max_len_impl(); }

extern "C" int ss_gsi_smooth(ss_ctx* c, int n_tracks, const int* offsets, const int* frames, const double* vals, const double* len_scale, double alpha,
                             double* out, int* status)
{
    // (tracks over the cap and empty tracks are settled on the host: a call that holds nothing else needs no context)
    return post_run(c, "ss_gsi_smooth",
        [&](std::string& err) { return ss_gsi_check_impl(n_tracks, offsets, frames, vals, len_scale, alpha, out, status, err); },
        [&](std::string& err) { return ss_gsi_smooth_impl(c ? &c->gsi : nullptr, c ? c->stream : nullptr, n_tracks, offsets, frames, vals, len_scale, alpha, out,
                                                          status, err); });
}

// ---- HOTA and CLEAR MOT against ground truth (ss_mot.hip, docs/MOTEVAL.md) --------------------------------------------------
extern "C" int ss_mot_max_boxes(void) { return ss_mot_max_boxes_impl(); }

extern "C" int ss_mot_eval(ss_ctx* c, int n_pairs, const int* frame_off, const int* gt_off, const int* tr_off, const int* gt_ids, const int* tr_ids,
                           const double* gt_boxes, const double* tr_boxes, const int* n_gt_ids, const int* n_tr_ids, double thr,
                           int* hota_match, double* hota_s, int* clear_match, double* clear_s, double* ga)
{
    return post_run(c, "ss_mot_eval",
        [&](std::string& err) { return ss_mot_check_impl(n_pairs, frame_off, gt_off, tr_off, gt_ids, tr_ids, gt_boxes, tr_boxes, n_gt_ids, n_tr_ids, thr,
                                                         hota_match, hota_s, clear_match, clear_s, err); },
        [&](std::string& err) { return ss_mot_eval_impl(c ? &c->mot : nullptr, c ? c->stream : nullptr, n_pairs, frame_off, gt_off, tr_off, gt_ids, tr_ids, gt_boxes,
                                                        tr_boxes, n_gt_ids, n_tr_ids, thr, hota_match, hota_s, clear_match, clear_s, ga, err); });
}

// ---- the identity metrics IDF1, IDP, IDR (ss_mot.hip, docs/MOTEVAL.md) ----------------------------------------------------------
extern "C" int ss_mot_max_ids(void) { return ss_mot_max_ids_impl(); }

extern "C" int ss_mot_identity(ss_ctx* c, int n_pairs, const int* frame_off, const int* gt_off, const int* tr_off, const int* gt_ids, const int* tr_ids,
                               const double* gt_boxes, const double* tr_boxes, const int* n_gt_ids, const int* n_tr_ids, double thr,
                               int* idtp, int* gt_to_tr, int* pot)
{
    return post_run(c, "ss_mot_identity",
        [&](std::string& err) { return ss_mot_identity_check_impl(n_pairs, frame_off, gt_off, tr_off, gt_ids, tr_ids, gt_boxes, tr_boxes, n_gt_ids, n_tr_ids, thr,
                                                                  idtp, gt_to_tr, err); },
        [&](std::string& err) { return ss_mot_identity_impl(c ? &c->mot : nullptr, c ? c->stream : nullptr, n_pairs, frame_off, gt_off, tr_off, gt_ids, tr_ids, gt_boxes,
                                                            tr_boxes, n_gt_ids, n_tr_ids, thr, idtp, gt_to_tr, pot, err); });
}

// ---- AFLink tracklet linking (ss_aflink.hip, docs/AFLINK.md) ---------------------------------------------------------------------
extern "C" long long ss_aflink_weight_floats(void) { return ss_aflink_weight_floats_impl(); }
extern "C" int ss_aflink_max_component(void) { return ss_aflink_max_component_impl(); }

extern "C" int ss_aflink_set_weights(ss_ctx* c, const float* blob, long long n)
{
    return post_run(c, "ss_aflink_set_weights",
        [&](std::string& err) { return ss_aflink_set_weights_check_impl(blob, n, err); },
        [&](std::string& err) { return ss_aflink_set_weights_impl(c ? &c->aflink : nullptr, c ? c->stream : nullptr, blob, err); });
}

// ---- COCO AP and AR of detections against ground truth (ss_ap.hip, docs/DETEVAL.md) ----------------------------------------------
extern "C" int ss_ap_max_gts(void) { return ss_ap_max_gts_impl(); }
extern "C" int ss_ap_max_cell_dets(void) { return ss_ap_max_cell_dets_impl(); }
extern "C" int ss_ap_max_keep(void) { return ss_ap_max_keep_impl(); }
extern "C" int ss_ap_max_dets(void) { return ss_ap_max_dets_impl(); }

extern "C" int ss_ap_eval(ss_ctx* c, int similarity, int n_classes, int n_cells, const int* class_cell_off, const int* cell_image, const int* cell_gt_off,
                          const int* cell_det_off, const double* gt_boxes, const int* gt_crowd, const double* det_boxes, const double* det_scores,
                          int n_thrs, const double* iou_thrs, int n_recs, const double* rec_thrs, int n_areas, const double* areas, int n_max_dets,
                          const int* max_dets, double* precision, double* recall, int* det_rank, int* rec_match, int* rec_ignored)
{
    return post_run(c, "ss_ap_eval",
        [&](std::string& err) { return ss_ap_check_impl(similarity, n_classes, n_cells, class_cell_off, cell_image, cell_gt_off, cell_det_off, gt_boxes, gt_crowd,
                                                        det_boxes, det_scores, n_thrs, iou_thrs, n_recs, rec_thrs, n_areas, areas, n_max_dets, max_dets, precision,
                                                        recall, det_rank, rec_match, rec_ignored, err); },
        [&](std::string& err) { return ss_ap_eval_impl(c ? &c->ap : nullptr, c ? c->stream : nullptr, similarity, n_classes, n_cells, class_cell_off, cell_gt_off,
                                                       cell_det_off, gt_boxes, gt_crowd, det_boxes, det_scores, n_thrs, iou_thrs, n_recs, rec_thrs, n_areas, areas,
                                                       n_max_dets, max_dets, precision, recall, det_rank, rec_match, rec_ignored, err); });
}

extern "C" int ss_aflink_cost(ss_ctx* c, int n_tracklets, const int* offsets, const double* feats, int thr_t0, int thr_t1, double thr_s, long long cap,
                              int* pair_i, int* pair_j, double* cost, float* inputs, long long* n_pairs)
{
    return post_run(c, "ss_aflink_cost",
        [&](std::string& err) { return ss_aflink_cost_check_impl(n_tracklets, offsets, feats, thr_t0, thr_t1, thr_s, cap, pair_i, pair_j, cost, n_pairs, err); },
        [&](std::string& err) { return ss_aflink_cost_impl(c ? &c->aflink : nullptr, c ? c->stream : nullptr, n_tracklets, offsets, feats, thr_t0, thr_t1, thr_s, cap,
                                                           pair_i, pair_j, cost, inputs, n_pairs, err); });
}

extern "C" int ss_aflink_match(ss_ctx* c, int n_tracklets, long long n_pairs, const int* pair_i, const int* pair_j, const double* cost, double thr_p,
                               int* successor)
{
    // (a call without a surviving pair is settled on the host and needs no context)
    return post_run(c, "ss_aflink_match",
        [&](std::string& err) { return ss_aflink_match_check_impl(n_tracklets, n_pairs, pair_i, pair_j, cost, thr_p, successor, err); },
        [&](std::string& err) { return ss_aflink_match_impl(c ? &c->aflink : nullptr, c ? c->stream : nullptr, n_tracklets, n_pairs, pair_i, pair_j, cost, thr_p,
                                                            successor, err); });
}

// Device -> host through a pinned staging buffer; synchronous (returns when h_dst holds the bytes).
extern "C" int ss_download(ss_ctx* c, void* hip_stream, void* h_dst, const void* d_src, size_t bytes)
{
    if (!c || !h_dst || !d_src) return fail(c, SS_ERR_INVALID, "ss_download: null argument");
    if (bytes == 0) return SS_OK;
    HIPCHK(c, c->back.reserve(bytes, SS_EXACT));
    HIPCHK(c, hipMemcpyAsync(c->back.as(), d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
    HIPCHK(c, hipStreamSynchronize((hipStream_t)hip_stream));
    memcpy(h_dst, c->back.as(), bytes);
    return SS_OK;
}

// ---- N4 camera-motion compensation ------------------------------------------------------------------------
extern "C" int ss_cmc_estimate(ss_ctx* c, void* hip_stream, const uint8_t* d_frames, int n_frames, long long frame_stride, int h,
                               int w, int row_stride, const int* d_n_valid, double* d_warps)
{
    if (!c || !d_frames || !d_warps || n_frames < 1 || n_frames > SS_FMAX || h < 20 || w < 20 || row_stride < 3 * w)
        return fail(c, SS_ERR_INVALID, "ss_cmc_estimate: bad argument");
    const int hs = (int)(h * 0.1), ws = (int)(w * 0.1);
    const size_t stride = ((size_t)hs * ws + 15) / 16 * 16;
    if (c->cmc_hw[0] != h || c->cmc_hw[1] != w) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hip_stream) HIPCHK(c, hipStreamIsCapturing((hipStream_t)hip_stream, &cs));
        if (cs != hipStreamCaptureStatusNone)
            return fail(c, SS_ERR_INVALID, "ss_cmc_estimate: first call for a frame size must not be inside a graph capture");
        uint8_t* buf = nullptr;
        int rc = dalloc(c, &buf, (size_t)(SS_FMAX + 1) * c->dev.S * stride);
        if (rc) return rc;
        c->cmc_small = buf; c->cmc_stride = stride; c->cmc_hw[0] = h; c->cmc_hw[1] = w;
        HIPCHK(c, hipMemsetAsync(c->cmc_prev_valid, 0, (size_t)c->dev.S * 4, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    ss_launch_cmc(d_frames, n_frames * c->dev.S, frame_stride, h, w, row_stride, c->cmc_small, (long long)c->cmc_stride, c->dev.S,
                  n_frames, hs, ws, 100, 1e-5, c->cmc_prev_valid, d_n_valid, d_warps, (hipStream_t)hip_stream);
    HIPCHK(c, hipGetLastError());
    c->cmc_frames = n_frames;
    return SS_OK;
}

extern "C" int ss_cmc_get_small(ss_ctx* c, int frame, int stream, uint8_t* out, int cap, int* hs, int* ws)
{
    if (!c || !c->cmc_stride || frame < 0 || frame > c->cmc_frames || stream < 0 || stream >= c->dev.S)
        return fail(c, SS_ERR_INVALID, "ss_cmc_get_small: no estimate yet, or frame / stream out of range");
    const int h = (int)(c->cmc_hw[0] * 0.1), w = (int)(c->cmc_hw[1] * 0.1);
    if (hs) *hs = h;
    if (ws) *ws = w;
    if (!out) return SS_OK;                                            // a size query
    if (cap < h * w) return fail(c, SS_ERR_INVALID, "ss_cmc_get_small: cap below hs * ws");
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(out, c->cmc_small + ((size_t)frame * c->dev.S + stream) * c->cmc_stride, (size_t)h * w, hipMemcpyDeviceToHost));
    return SS_OK;
}

extern "C" int ss_track_set_cmc(ss_ctx* c, const double* d_warps)
{
    if (!c) return SS_ERR_INVALID;
    c->cmc_warps = d_warps;
    return SS_OK;
}

// ---- sparse-optical-flow camera motion (ss_gmc.hip, docs/BYTETRACK.md §1f) -----------------------------------------------------
// Arguments are checked before the context: a bad call returns SS_ERR_INVALID without touching the device, context or not.
extern "C" int ss_gmc_sparse_estimate(ss_ctx* c, void* hip_stream, const uint8_t* d_frames, int n_frames, long long frame_stride, int h,
                                      int w, int row_stride, const int* d_n_valid, double* d_warps)
{
    const char* bad = nullptr;
    if (!d_frames || !d_warps) bad = "null pointer";
    else if (n_frames < 1 || n_frames > SS_FMAX) bad = "n_frames outside 1..32";
    else if (h < SS_GMC_MIN_SIDE || w < SS_GMC_MIN_SIDE || h > 16384 || w > 16384) bad = "frame sides outside 64..16384 (level 3 of the half image must be at least 4 x 4)";
    else if (row_stride < 3 * w) bad = "row_stride below 3 * w";
    if (bad) return fail(c, SS_ERR_INVALID, std::string("ss_gmc_sparse_estimate: ") + bad);
    if (!c) return fail(c, SS_ERR_INVALID, "ss_gmc_sparse_estimate: null context");
    SSGmcDev& g = c->gmc;
    if (g.h != h || g.w != w) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hip_stream) HIPCHK(c, hipStreamIsCapturing((hipStream_t)hip_stream, &cs));
        if (cs != hipStreamCaptureStatusNone)
            return fail(c, SS_ERR_INVALID, "ss_gmc_sparse_estimate: first call for a frame size must not be inside a graph capture");
        const size_t S = c->dev.S, FM = SS_FMAX;
        g.S = (int)S;
        long long off = 0;
        for (int L = 0; L < SS_GMC_LEVELS; ++L) {
            g.lw[L] = L ? (g.lw[L - 1] + 1) / 2 : w / 2;
            g.lh[L] = L ? (g.lh[L - 1] + 1) / 2 : h / 2;
            g.loff[L] = off;
            off += (long long)g.lw[L] * g.lh[L];
        }
        g.pyr_stride = (off + 15) / 16 * 16;
        const size_t npix = (size_t)g.lw[0] * g.lh[0];
        int rc = dalloc(c, &g.pyr, (FM + 1) * S * (size_t)g.pyr_stride);
        if (rc == SS_OK) rc = dalloc(c, &g.eig, FM * S * npix);
        if (rc == SS_OK) rc = dalloc(c, &g.cand, FM * S * npix);
        if (rc == SS_OK) rc = dalloc(c, &g.emax, FM * S);
        if (rc == SS_OK) rc = dalloc(c, &g.corners, (FM + 1) * S * SS_GMC_MAXC);
        if (rc == SS_OK) rc = dalloc(c, &g.ncorner, (FM + 1) * S);
        if (rc == SS_OK) rc = dalloc(c, &g.ncand, (FM + 1) * S);
        if (rc == SS_OK) rc = dalloc(c, &g.pts, FM * S * SS_GMC_MAXC * 2);
        if (rc == SS_OK) rc = dalloc(c, &g.status, FM * S * SS_GMC_MAXC);
        if (rc == SS_OK) rc = dalloc(c, &g.inlier, FM * S * SS_GMC_MAXC);
        if (rc) { g.h = g.w = 0; return rc; }
        g.h = h; g.w = w;
        HIPCHK(c, hipMemsetAsync(g.prev_valid, 0, S * 4, c->stream));
        HIPCHK(c, hipMemsetAsync(g.last, 0, 4, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    ss_launch_gmc_sparse(g, d_frames, n_frames, frame_stride, row_stride, d_n_valid, d_warps, (hipStream_t)hip_stream);
    HIPCHK(c, hipGetLastError());
    return SS_OK;
}

extern "C" int ss_gmc_sparse_get(ss_ctx* c, int frame, int stream, uint8_t* half, uint8_t* level1, uint8_t* level2, uint8_t* level3,
                                 int* corners_xy, int* n_corners, int* n_candidates, double* points, uint8_t* status, uint8_t* inliers)
{
    if (!c || !c->gmc.h || frame < 0 || frame >= SS_FMAX || stream < 0 || stream >= c->dev.S)
        return fail(c, SS_ERR_INVALID, "ss_gmc_sparse_get: no estimate yet, or frame / stream out of range");
    const SSGmcDev& g = c->gmc;
    HIPCHK(c, hipDeviceSynchronize());
    const size_t prev = (size_t)frame * g.S + stream, cur = prev + g.S;
    uint8_t* lv[SS_GMC_LEVELS] = { half, level1, level2, level3 };
    for (int L = 0; L < SS_GMC_LEVELS; ++L)
        if (lv[L]) HIPCHK(c, hipMemcpy(lv[L], g.pyr + cur * g.pyr_stride + g.loff[L], (size_t)g.lw[L] * g.lh[L], hipMemcpyDeviceToHost));
    int n = 0;
    HIPCHK(c, hipMemcpy(&n, g.ncorner + prev, 4, hipMemcpyDeviceToHost));
    if (n_corners) *n_corners = n;
    if (n_candidates) HIPCHK(c, hipMemcpy(n_candidates, g.ncand + prev, 4, hipMemcpyDeviceToHost));
    if (corners_xy) {
        std::vector<int> idx(SS_GMC_MAXC);
        HIPCHK(c, hipMemcpy(idx.data(), g.corners + prev * SS_GMC_MAXC, SS_GMC_MAXC * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) { corners_xy[2 * i] = idx[i] % g.lw[0]; corners_xy[2 * i + 1] = idx[i] / g.lw[0]; }
    }
    if (points) HIPCHK(c, hipMemcpy(points, g.pts + prev * SS_GMC_MAXC * 2, SS_GMC_MAXC * 16, hipMemcpyDeviceToHost));
    if (status) HIPCHK(c, hipMemcpy(status, g.status + prev * SS_GMC_MAXC, SS_GMC_MAXC, hipMemcpyDeviceToHost));
    if (inliers) HIPCHK(c, hipMemcpy(inliers, g.inlier + prev * SS_GMC_MAXC, SS_GMC_MAXC, hipMemcpyDeviceToHost));
    return SS_OK;
}

// ---- N2 overlay -----------------------------------------------------------------------------------------
extern "C" int ss_overlay_set_font(ss_ctx* c, const uint8_t* h_font_95x5)
{
    if (!c || !h_font_95x5) return fail(c, SS_ERR_INVALID, "ss_overlay_set_font: null argument");
    HIPCHK(c, hipMemcpy(c->font, h_font_95x5, 95 * 5, hipMemcpyHostToDevice));
    return SS_OK;
}

extern "C" int ss_overlay(ss_ctx* c, void* hip_stream, uint8_t* d_frames, int batch, long long frame_batch_stride, int h, int w,
                          int row_stride, const int* d_prims, const int* d_prim_off, const uint8_t* d_chars)
{
    if (!c || !d_frames || !d_prims || !d_prim_off || !d_chars || batch < 0 || batch > 65535 || row_stride < 3 * w)
        return fail(c, SS_ERR_INVALID, "ss_overlay: bad argument");
    ss_launch_overlay(d_frames, batch, frame_batch_stride, h, w, row_stride, d_prims, d_prim_off, d_chars, c->font, (hipStream_t)hip_stream);
    HIPCHK(c, hipGetLastError());
    return SS_OK;
}

// ---- instance masks of a segmentation head (ss_mask.hip) -------------------------------------------------------------------
// Every argument is checked before the context: a bad call returns SS_ERR_INVALID without touching the device, context or not.
extern "C" int ss_mask_assemble(ss_ctx* c, void* hip_stream, const void* d_proto, int proto_f16, long long proto_frame_stride, int nm, int mh,
                                int mw, const float* d_dets, long long dets_frame_stride, int det_ld, int coef_off, const int* d_counts,
                                int n_frames, int max_rows, const float* d_geom, long long geom_frame_stride, int ih, int iw, uint32_t* d_bits,
                                long long bits_frame_stride)
{
    const char* bad = nullptr;
    const long long wpr = (iw + 31) / 32;
    if (!d_proto || !d_dets || !d_counts || !d_geom || !d_bits) bad = "null pointer";
    else if (nm < 1 || nm > 64) bad = "nm outside 1..64";
    else if (mh < 1 || mw < 1 || mw > 256 || ih != 4 * mh || iw != 4 * mw) bad = "input size must be 4 x the prototype size, prototype width <= 256";
    else if (n_frames < 1 || n_frames > 65535 || max_rows < 1 || max_rows > 65535) bad = "n_frames / max_rows outside 1..65535";
    else if (coef_off < 4 || det_ld < coef_off + nm) bad = "coefficient columns outside the detection row";
    else if (n_frames > 1 && (proto_frame_stride < (long long)nm * mh * mw || dets_frame_stride < (long long)max_rows * det_ld ||
                              geom_frame_stride < 0 || bits_frame_stride < (long long)max_rows * ih * wpr))
        bad = "frame strides overlap";
    if (bad) return fail(c, SS_ERR_INVALID, std::string("ss_mask_assemble: ") + bad);
    if (!c) return fail(c, SS_ERR_INVALID, "ss_mask_assemble: null context");
    ss_launch_mask_assemble(d_proto, proto_f16, proto_frame_stride, nm, mh, mw, d_dets, dets_frame_stride, det_ld, coef_off, d_counts, n_frames,
                            max_rows, d_geom, geom_frame_stride, ih, iw, d_bits, bits_frame_stride, (hipStream_t)hip_stream);
    HIPCHK(c, hipGetLastError());
    return SS_OK;
}

extern "C" int ss_mask_outline(ss_ctx* c, void* hip_stream, const uint32_t* d_bits, long long bits_frame_stride, const int* d_counts, int n_frames,
                               int max_rows, int ih, int iw, int cap, int* d_pts, long long pts_frame_stride, int* d_npts, long long npts_frame_stride,
                               uint32_t* d_bits_copy, long long copy_frame_stride, void* d_scratch, long long scratch_bytes)
{
    const char* bad = nullptr;
    const long long wpr = (iw + 31) / 32, plane = (long long)ih * iw * 4;
    if (!d_bits || !d_counts || !d_pts || !d_npts || !d_scratch) bad = "null pointer";
    else if (ih < 1 || iw < 1 || ih * wpr > ss_mask_max_words()) bad = "mask larger than the kernel's LDS plane";
    else if (n_frames < 1 || n_frames > 65535 || max_rows < 1 || max_rows > 65535) bad = "n_frames / max_rows outside 1..65535";
    else if (cap < 1 || cap > (1 << 20)) bad = "cap outside 1..2^20";
    else if (scratch_bytes < plane) bad = "scratch smaller than one label plane (4 * ih * iw bytes)";
    else if (n_frames > 1 && (bits_frame_stride < (long long)max_rows * ih * wpr || pts_frame_stride < (long long)max_rows * cap * 2 ||
                              npts_frame_stride < max_rows || (d_bits_copy && copy_frame_stride < (long long)max_rows * ih * wpr)))
        bad = "frame strides overlap";
    if (bad) return fail(c, SS_ERR_INVALID, std::string("ss_mask_outline: ") + bad);
    if (!c) return fail(c, SS_ERR_INVALID, "ss_mask_outline: null context");
    const long long slots = scratch_bytes / plane;
    ss_launch_mask_outline(d_bits, bits_frame_stride, d_counts, n_frames, max_rows, ih, iw, cap, d_pts, pts_frame_stride, d_npts,
                           npts_frame_stride, d_bits_copy, copy_frame_stride, (int*)d_scratch, (int)(slots < 1024 ? slots : 1024),
                           (hipStream_t)hip_stream);
    HIPCHK(c, hipGetLastError());
    return SS_OK;
}

extern "C" int ss_synchronize(ss_ctx* c)
{
    if (!c) return SS_ERR_INVALID;
    if (int rcj = chain_join(c, c->stream)) return rcj;               // a detached chain wrote what this call reads
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SS_OK;
}

extern "C" int ss_reset(ss_ctx* c, int stream)
{
    if (!c || stream >= c->dev.S) return fail(c, SS_ERR_INVALID, "ss_reset: bad stream");
    if (int rcj = chain_join(c, c->stream)) return rcj;               // a detached chain wrote what this call reads
    SSDev& d = c->dev;
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? d.S : stream + 1;
    const size_t T = SS_MAXT;
    for (int s = s0; s < s1; ++s) {
        int one = 1;
        HIPCHK(c, hipMemsetAsync(d.n_tracks + s, 0, 4, c->stream));
        HIPCHK(c, hipMemsetAsync(d.frame + s, 0, 4, c->stream));
        HIPCHK(c, hipMemsetAsync(d.err + s, 0, 4, c->stream));
        HIPCHK(c, hipMemsetAsync(d.slot_used + s * T, 0, T * 4, c->stream));
        HIPCHK(c, hipMemsetAsync(d.gal_count + s * T, 0, T * 4, c->stream));
        HIPCHK(c, hipMemsetAsync(d.gal_head + s * T, 0, T * 4, c->stream));
        HIPCHK(c, hipMemcpyAsync(d.next_id + s, &one, 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    HIPCHK(c, hipMemsetAsync(d.n_items, 0, 32, c->stream));
    for (int s = s0; s < s1; ++s) HIPCHK(c, hipMemsetAsync(c->cmc_prev_valid + s, 0, 4, c->stream));
    HIPCHK(c, hipMemsetAsync(c->gmc.prev_valid + s0, 0, (size_t)(s1 - s0) * 4, c->stream));
    if (stream < 0)
        for (int u = 0; u < c->nms_units; ++u) HIPCHK(c, hipMemsetAsync(ss_nms_error_flag(c->nms_ws, u), 0, 4, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SS_OK;
}

// ---- tracker -----------------------------------------------------------------------------------
extern "C" int ss_track_update_group(ss_ctx* c, int n_frames, const float* d_dets, const int* d_ndets, const float* d_feats,
                                     const int* d_img_hw, float* d_out, int* d_nout)
{
    if (!c || !d_dets || !d_ndets || !d_feats || !d_img_hw || !d_out || !d_nout)
        return fail(c, SS_ERR_INVALID, "ss_track_update_group: null argument");
    if (n_frames < 1 || n_frames > SS_FMAX) return fail(c, SS_ERR_INVALID, "ss_track_update_group: 1 <= n_frames <= SS_FMAX");
    // a gallery ring position must be overwritten at most once per group (k_assoc's per-frame row mask, k_newrow)
    if (n_frames > c->cfg.nn_budget) return fail(c, SS_ERR_INVALID, "ss_track_update_group: n_frames <= nn_budget required");
    SSDev dev;
    memcpy(&dev, &c->dev, sizeof dev);                          // byte copy: the padding stays zero (the chain graphs are keyed by the struct's bytes)
    dev.F = n_frames;
    dev.dets = d_dets; dev.n_dets = d_ndets; dev.feats_raw = d_feats; dev.img_hw = (int*)d_img_hw;
    dev.out_rows = d_out; dev.n_out = d_nout;
    // Every launch dimension is fixed by (streams, n_frames): track and detection counts are device-side values read
    // from the work lists, so nothing here needs a host round trip and the sequence can be captured into a HIP graph.
    dev.cos_grid = c->cos_grid; dev.comp_rows = c->comp_rows; dev.assoc_stage = c->assoc_stage; dev.xcd_map = c->xcd_map;
    dev.ts_enable = c->inkernel;
    dev.cmc = c->cmc_warps;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (c->timing) {
        if (c->ev_used == c->ev.size()) {
            hipEvent_t a, b;
            HIPCHK(c, hipEventCreate(&a)); HIPCHK(c, hipEventCreate(&b));
            c->ev.emplace_back(a, b);
        }
        e0 = c->ev[c->ev_used].first; e1 = c->ev[c->ev_used].second; ++c->ev_used;
    }
    if (int rc = chain_join(c, c->stream)) return rc;          // the previous group's detached chain wrote the track tables this call reads
    ss_launch_group_head(dev, c->prm, c->stream, e0, e1, c->assoc_event);
    HIPCHK(c, hipGetLastError());
    // The chain: k_frame / k_post / k_newrow per frame, strictly dependent.  For a group of several frames that is up to 95
    // launches (~3.5 us of host time each); replayed as one graph it costs one hipGraphLaunch.  The kernels' arguments are
    // values (SSDev, SSParams, f): a graph is valid for exactly one (frames, caller buffers, options) combination, which is
    // what the key compares.  Not inside somebody else's stream capture (torch capturing the frame-at-a-time pipeline).
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (c->stream) HIPCHK(c, hipStreamIsCapturing(c->stream, &cs));
    // Detached chain (option "chain_cus"): the chain's one- to 64-workgroup kernels go to a stream whose queue owns a few compute
    // units, ordered after the association launch by an event; the caller's stream goes on with its next launches (the networks
    // of the following group) and ss_track_join makes whoever consumes the rows wait for the chain.
    hipStream_t chain_st = c->stream;
    struct Done { ss_ctx* c; hipStream_t st; bool on; ~Done() { if (on && hipEventRecord(c->ev_chain, st) == hipSuccess) c->chain_pending = true; } };
    const bool detach = c->chain_stream && cs == hipStreamCaptureStatusNone;
    if (detach) {
        HIPCHK(c, hipEventRecord(c->ev_head, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->chain_stream, c->ev_head, 0));
        chain_st = c->chain_stream;
    }
    Done done{ c, chain_st, detach };                          // recorded after whichever form of the chain is enqueued below
    if (!c->track_graph || n_frames < 2 || cs != hipStreamCaptureStatusNone) {
        ss_launch_group_chain(dev, c->prm, chain_st);
        HIPCHK(c, hipGetLastError());
        return SS_OK;
    }
    std::vector<char> key(sizeof(SSDev) + sizeof(SSParams));
    memcpy(key.data(), &dev, sizeof(SSDev));
    memcpy(key.data() + sizeof(SSDev), &c->prm, sizeof(SSParams));
    ss_ctx::Chain* hit = nullptr;
    for (auto& g : c->chains) if (g.key == key) { hit = &g; break; }
    if (!hit) {
        // a combination is captured the SECOND time it is seen: a caller that walks through fresh buffers (every call another
        // slice of a long array) would otherwise pay a capture + instantiation per call and never replay anything
        unsigned long long h = 1469598103934665603ull;
        for (char ch : key) h = (h ^ (unsigned char)ch) * 1099511628211ull;
        bool seen = false;
        for (unsigned long long v : c->chain_seen) seen = seen || v == h;
        if (!seen) {
            if (c->chain_seen.size() >= 64) c->chain_seen.erase(c->chain_seen.begin());
            c->chain_seen.push_back(h);
            ss_launch_group_chain(dev, c->prm, chain_st);
            HIPCHK(c, hipGetLastError());
            return SS_OK;
        }
        // From here on the group's head (k_group_prep + k_assoc) is enqueued: whatever fails below, the chain still goes out (as
        // plain launches) before the error is reported — a group is never left half-applied.
        auto plain_then = [&](hipError_t e) -> int {
            (void)hipGetLastError();
            ss_launch_group_chain(dev, c->prm, chain_st);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, e);
            return SS_OK;
        };
        if (!c->cap_stream) { const hipError_t e = hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking); if (e != hipSuccess) { c->cap_stream = nullptr; return plain_then(e); } }
        if (c->chains.size() >= 16) {                            // least recently used entry goes
            size_t lru = 0;
            for (size_t i = 1; i < c->chains.size(); ++i) if (c->chains[i].used < c->chains[lru].used) lru = i;
            // its last replay may still be running (16 other launches is no guarantee on a detached, slow chain), and on ANOTHER stream
            // than today's if chain_cus / ss_set_hip_stream changed in between: the stream it was last launched on is drained before
            // the executable graph goes
            const hipError_t e = hipStreamSynchronize(c->chains[lru].last_st);
            if (e != hipSuccess) return plain_then(e);
            (void)hipGraphExecDestroy(c->chains[lru].exec); (void)hipGraphDestroy(c->chains[lru].graph);
            c->chains.erase(c->chains.begin() + lru);
        }
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        // A failed capture / instantiation must not leave the group half-applied (its head, k_group_prep + k_assoc, is already
        // enqueued): the chain then goes out as plain launches, the captured graph (if any) is released.
        hipError_t be = hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeThreadLocal), le = hipSuccess, ee = hipSuccess, ie = hipSuccess;
        if (be == hipSuccess) {
            ss_launch_group_chain(dev, c->prm, c->cap_stream);
            le = hipGetLastError();
            ee = hipStreamEndCapture(c->cap_stream, &graph);
            if (le == hipSuccess && ee == hipSuccess && graph) ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        }
        if (be != hipSuccess || le != hipSuccess || ee != hipSuccess || !graph || ie != hipSuccess || !exec) {
            if (graph) (void)hipGraphDestroy(graph);
            (void)hipGetLastError();
            ss_launch_group_chain(dev, c->prm, chain_st);
            HIPCHK(c, hipGetLastError());
            return SS_OK;
        }
        c->chains.push_back({ key, graph, exec, 0, chain_st });
        hit = &c->chains.back();
    }
    hit->used = ++c->chain_clock;
    hit->last_st = chain_st;
    if (hipGraphLaunch(hit->exec, chain_st) != hipSuccess) {     // (the replay did not start: the same kernels as plain launches)
        (void)hipGetLastError();
        ss_launch_group_chain(dev, c->prm, chain_st);
        HIPCHK(c, hipGetLastError());
    }
    return SS_OK;
}

extern "C" int ss_track_join(ss_ctx* c, void* hip_stream)
{
    if (!c) return SS_ERR_INVALID;
    return chain_join(c, (hipStream_t)hip_stream);
}

extern "C" int ss_stream_create(ss_ctx* c, int skip_cus, void** out)
{
    if (!c || !out || skip_cus < 0) return fail(c, SS_ERR_INVALID, "ss_stream_create: bad argument");
    hipDeviceProp_t prop;
    HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
    hipStream_t st = nullptr;
    if (skip_cus == 0) HIPCHK(c, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    else if (int rc = cu_mask_stream(c, skip_cus, prop.multiProcessorCount - skip_cus, &st)) return rc;
    *out = (void*)st;
    return SS_OK;
}

extern "C" int ss_stream_destroy(ss_ctx* c, void* hip_stream)
{
    if (!c || !hip_stream) return SS_ERR_INVALID;
    HIPCHK(c, hipStreamDestroy((hipStream_t)hip_stream));
    return SS_OK;
}

extern "C" int ss_max_group_frames(void) { return SS_FMAX; }

extern "C" int ss_track_set_assoc_event(ss_ctx* c, void* hip_event)
{
    if (!c) return SS_ERR_INVALID;
    c->assoc_event = (hipEvent_t)hip_event;
    return SS_OK;
}

extern "C" int ss_track_update(ss_ctx* c, const float* d_dets, const int* d_ndets, const float* d_feats,
                               const int* d_img_hw, float* d_out, int* d_nout)
{
    return ss_track_update_group(c, 1, d_dets, d_ndets, d_feats, d_img_hw, d_out, d_nout);
}

extern "C" int ss_track_update_host(ss_ctx* c, int stream, const float* h_dets, int n, const float* h_feats,
                                    int img_h, int img_w, float* h_out, int cap_rows, int* n_out)
{
    if (!c || stream < 0 || stream >= c->dev.S || n < 0 || !n_out) return fail(c, SS_ERR_INVALID, "ss_track_update_host: bad argument");
    if (n > SS_MAXD) return fail(c, SS_ERR_CAPACITY, "ss_track_update_host: more than SS_MAX_DETS detections");
    const int S = c->dev.S;
    // other streams see 0 detections this call only if they are not driven: to keep streams
    // independent the host path requires a single-stream context.
    if (S != 1) return fail(c, SS_ERR_INVALID, "ss_track_update_host: context must hold exactly one stream");
    int hw[2] = { img_h, img_w };
    if (n) {
        HIPCHK(c, hipMemcpyAsync(c->d_dets, h_dets, (size_t)n * 6 * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_feats, h_feats, (size_t)n * SS_F * 4, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(c->d_ndets, &n, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_imghw, hw, 8, hipMemcpyHostToDevice, c->stream));
    int rc = ss_track_update(c, c->d_dets, c->d_ndets, c->d_feats, c->d_imghw, c->d_out, c->d_nout);
    if (rc) return rc;
    if (int rcj = chain_join(c, c->stream)) return rcj;
    int cnt[2] = { 0, 0 }, err = 0;
    HIPCHK(c, hipMemcpyAsync(&cnt[0], c->d_nout, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&err, c->dev.err, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (err) return fail(c, err, err == SS_ERR_CAPACITY ? "tracker capacity exceeded on device" : "assignment infeasible on device");
    *n_out = cnt[0];
    if (cnt[0] > cap_rows) return fail(c, SS_ERR_CAPACITY, "ss_track_update_host: output buffer too small");
    if (cnt[0]) HIPCHK(c, hipMemcpy(h_out, c->d_out, (size_t)cnt[0] * 8 * 4, hipMemcpyDeviceToHost));
    return SS_OK;
}

extern "C" int ss_set_option(ss_ctx* c, const char* name, int value)
{
    if (!c || !name) return fail(c, SS_ERR_INVALID, "ss_set_option: null argument");
    const std::string n(name);
    if (n == "cos_grid") { if (value < 8 || value > 4096 || value % 8) return fail(c, SS_ERR_INVALID, "cos_grid: a multiple of 8 in 8..4096"); c->cos_grid = value; }
    else if (n == "nms_fused") ss_nms_fused = value != 0;       // process-wide: one workgroup per image after the filter (1, default) or sort / mask / scan launches
    else if (n == "assoc_comp_rows") { if (value < 0 || value > 12) return fail(c, SS_ERR_INVALID, "assoc_comp_rows: 0..12"); c->comp_rows = value; }
    else if (n == "assoc_stage") { if (value != 0 && value != 1 && value != 2 && value != 4 && value != 5) return fail(c, SS_ERR_INVALID, "assoc_stage: 0, 1, 2, 4 or 5"); c->assoc_stage = value; }
    else if (n == "assoc_pack") c->dev.assoc_pack = value != 0;         // association on detection columns packed across the group's frames (default) / per-frame pairs
    else if (n == "pred_ahead") c->dev.pred_ahead = value != 0;         // k_frame takes the predicted state post_track left (default) / predicts itself
    else if (n == "chain_merge") c->dev.chain_merge = value != 0;       // k_post + k_newrow of a frame as one launch (default) / two launches
    else if (n == "frame_caps") {
        // value = tracks and detections k_frame keeps in LDS (cost entries = value^2): 0 restores the maxima (256 tracks, 128 detections, 12288 entries)
        // (112 is the largest square that fits: 128 x 128 cost entries + the per-track areas would be 173 KB of LDS, past the CU's 160)
        if (value != 0 && (value < 16 || value > 112 || value % 16)) return fail(c, SS_ERR_INVALID, "frame_caps: 0 or a multiple of 16 in 16..112");
        c->dev.cap_t = value ? value : SS_MAXT; c->dev.cap_d = value ? value : SS_MAXD;
        c->dev.cap_cost = value ? (value * value < SS_COST_CAP ? value * value : SS_COST_CAP) : SS_COST_CAP;
    }
    else if (n == "chain_cus") {
        if (value < -1 || value > 128 || (value > 0 && value % 8)) return fail(c, SS_ERR_INVALID, "chain_cus: 0 (off), -1 (detached, no reservation) or a multiple of 8 up to 128");
        if (c->chain_stream) { HIPCHK(c, hipStreamSynchronize(c->chain_stream)); HIPCHK(c, hipStreamDestroy(c->chain_stream)); c->chain_stream = nullptr; }
        c->chain_pending = false;
        if (value) {
            if (value < 0) {                                     // detached onto a plain high-priority stream: every compute unit, no reservation
                int lo = 0, hi = 0;
                HIPCHK(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
                HIPCHK(c, hipStreamCreateWithPriority(&c->chain_stream, hipStreamNonBlocking, hi));
            } else if (int rc = cu_mask_stream(c, 0, value, &c->chain_stream)) return rc;
            if (!c->ev_head) { HIPCHK(c, hipEventCreateWithFlags(&c->ev_head, hipEventDisableTiming)); HIPCHK(c, hipEventCreateWithFlags(&c->ev_chain, hipEventDisableTiming)); }
        }
        c->chain_cus = value;
    }
    else if (n == "track_graph") { if (value != 0 && value != 1) return fail(c, SS_ERR_INVALID, "track_graph: 0 or 1"); c->track_graph = value; }
    else if (n == "assoc_xcd_map") { if (value != 0 && value != 1) return fail(c, SS_ERR_INVALID, "assoc_xcd_map: 0 or 1"); c->xcd_map = value; }
    else return fail(c, SS_ERR_INVALID, "ss_set_option: unknown option '" + n + "'");
    return SS_OK;
}

extern "C" int ss_check_errors(ss_ctx* c)
{
    if (!c) return SS_ERR_INVALID;
    if (int rcj = chain_join(c, c->stream)) return rcj;               // a detached chain wrote what this call reads
    std::vector<int> e(c->dev.S);
    HIPCHK(c, hipMemcpyAsync(e.data(), c->dev.err, e.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t s = 0; s < e.size(); ++s)
        if (e[s]) return fail(c, e[s], "device error flag on stream " + std::to_string(s));
    std::string err;                                         // the attached stages' flags, each SS_OK without its state:
    int rc = ss_byte_pending_impl(c->byte, c->stream, err);                     // the tracker families' (capacity, infeasible)
    if (rc == SS_OK) rc = ss_ocsort_pending_impl(c->oc, c->stream, err);
    if (rc == SS_OK) rc = ss_deepoc_pending_impl(c->deepoc, c->stream, err);
    if (rc == SS_OK) rc = ss_hybrid_pending_impl(c->hybrid, c->stream, err);
    if (rc == SS_OK) rc = ss_zone_pending_impl(c->zone, c->stream, err);        // more live tracks than the analytics table holds
    if (rc == SS_OK) rc = ss_bank_pending_impl(c->bank, c->stream, err);        // an id above the track bank's max_ids
    if (rc == SS_OK) rc = ss_jpeg_pending_impl(c->jpeg, err);                   // images a device-entropy JPEG call refused (docs/JPEG.md section 12)
    if (rc != SS_OK) return fail(c, rc, err);
    for (int u = 0; u < c->nms_units; ++u) {                 // NMS candidate overflow (flag stays set until ss_reset)
        int f = 0;
        HIPCHK(c, hipMemcpy(&f, ss_nms_error_flag(c->nms_ws, u), 4, hipMemcpyDeviceToHost));
        if (f) return fail(c, f, "ss_nms: more than 8192 candidates above conf_thres (image " + std::to_string(u) + " of the batch)");
    }
    return SS_OK;
}

// ---- stage entry points ---------------------------------------------------------------------------
extern "C" int ss_feat_normalize(ss_ctx* c, const float* raw, int n, float* unit)
{ if (!c) return SS_ERR_INVALID; ss_launch_normalize(raw, n, unit, c->stream); HIPCHK(c, hipGetLastError()); return SS_OK; }

extern "C" int ss_ema(ss_ctx* c, const float* s, const float* f, int n, float* o)
{ if (!c) return SS_ERR_INVALID; ss_launch_ema(s, f, n, c->prm.ema_alpha, c->prm.ema_one_minus_alpha, o, c->stream); HIPCHK(c, hipGetLastError()); return SS_OK; }

extern "C" int ss_kf_predict(ss_ctx* c, double* mean, double* cov, int n)
{ if (!c) return SS_ERR_INVALID; ss_launch_kf(0, mean, cov, nullptr, nullptr, n, c->prm.wp, c->prm.wv, c->stream); HIPCHK(c, hipGetLastError()); return SS_OK; }

extern "C" int ss_kf_update(ss_ctx* c, double* mean, double* cov, const double* z, const double* conf, int n)
{ if (!c) return SS_ERR_INVALID; ss_launch_kf(1, mean, cov, z, conf, n, c->prm.wp, c->prm.wv, c->stream); HIPCHK(c, hipGetLastError()); return SS_OK; }

extern "C" int ss_kf_project(ss_ctx* c, const double* mean, const double* cov, const double* conf, int n, double* zmean, double* S)
{
    if (!c || !mean || !cov || !zmean || !S || n < 0) return fail(c, SS_ERR_INVALID, "ss_kf_project: bad argument");
    ss_launch_project(mean, cov, conf, n, c->prm.wp, zmean, S, c->stream); HIPCHK(c, hipGetLastError()); return SS_OK;
}

extern "C" int ss_kf_initiate(ss_ctx* c, const double* z, int n, double* mean, double* cov)
{ if (!c) return SS_ERR_INVALID; ss_launch_kf(2, mean, cov, z, nullptr, n, c->prm.wp, c->prm.wv, c->stream); HIPCHK(c, hipGetLastError()); return SS_OK; }

extern "C" int ss_gallery_pack(ss_ctx* c, const float* nat, int T, int B, float* frag)
{
    if (!c || B > SS_NRT * SS_TILE) return fail(c, SS_ERR_INVALID, "ss_gallery_pack: B > 128");
    ss_launch_pack(nat, T, B, frag, c->stream); HIPCHK(c, hipGetLastError()); return SS_OK;
}

extern "C" int ss_assoc_cost(ss_ctx* c, const float* gal, const int* counts, int T, const float* feats, int D,
                             const double* mean, const double* cov, const double* xyah, double* cost,
                             float* cosd, double* maha, uint8_t* gated)
{
    if (!c) return SS_ERR_INVALID;
    if (T > SS_MAXT || D > SS_MAXD) return fail(c, SS_ERR_CAPACITY, "ss_assoc_cost: T <= 256, D <= 128");
    ss_launch_assoc(gal, counts, T, feats, D, mean, cov, xyah, c->prm, c->kat_featfrag, c->kat_partmin,
                    cost, cosd, maha, gated, c->stream);
    HIPCHK(c, hipGetLastError());
    return SS_OK;
}

extern "C" int ss_iou_cost(ss_ctx* c, const double* t, int T, const double* d, int D, double* cost)
{ if (!c) return SS_ERR_INVALID; ss_launch_iou(t, T, d, D, c->prm.max_iou_distance, cost, c->stream); HIPCHK(c, hipGetLastError()); return SS_OK; }

extern "C" int ss_lsap(ss_ctx* c, const double* cost, int nr, int nc, int* r2c)
{
    if (!c) return SS_ERR_INVALID;
    if (nr > 256 || nc > 256) return fail(c, SS_ERR_CAPACITY, "ss_lsap: at most 256 x 256");
    if (nr == 0) return SS_OK;
    HIPCHK(c, hipMemsetAsync(c->kat_err, 0, 4, c->stream));
    ss_launch_lsap(cost, nr, nc, r2c, c->kat_lsap_t, c->kat_err, c->stream);
    HIPCHK(c, hipGetLastError());
    int e = 0;
    HIPCHK(c, hipMemcpyAsync(&e, c->kat_err, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (e) return fail(c, e, "ss_lsap: infeasible cost matrix");
    return SS_OK;
}

// ---- front end ----------------------------------------------------------------------------------------
extern "C" int ss_letterbox_batch(ss_ctx* c, const uint8_t* src, int batch, long long src_batch_stride, int h, int w,
                                  int stride, void* dst, int dst_flags, int out_h, int out_w, int new_h, int new_w,
                                  int pad_top, int pad_left, int pad_value)
{
    if (!c || !src || !dst || new_h < 1 || new_w < 1 || batch < 0 || batch > 65535 || out_h > 65535)
        return fail(c, SS_ERR_INVALID, "ss_letterbox: bad argument");
    ss_launch_letterbox(src, batch, src_batch_stride, h, w, stride, dst, dst_flags, out_h, out_w, new_h, new_w, pad_top,
                        pad_left, pad_value, c->stream);
    HIPCHK(c, hipGetLastError());
    return SS_OK;
}

extern "C" int ss_letterbox(ss_ctx* c, const uint8_t* src, int h, int w, int stride, void* dst, int dst_flags,
                            int out_h, int out_w, int new_h, int new_w, int pad_top, int pad_left, int pad_value)
{
    return ss_letterbox_batch(c, src, 1, 0, h, w, stride, dst, dst_flags, out_h, out_w, new_h, new_w, pad_top, pad_left,
                              pad_value);
}

// workspace for `batch` images; growing it allocates, which a stream capture does not allow
static int nms_reserve(ss_ctx* c, int batch)
{
    if (batch <= c->nms_units) return SS_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (c->stream) HIPCHK(c, hipStreamIsCapturing(c->stream, &cs));
    if (cs != hipStreamCaptureStatusNone)
        return fail(c, SS_ERR_INVALID, "ss_nms_batch: first call with this batch size must not be inside a graph capture");
    char* w = nullptr;
    int rc = dalloc(c, &w, c->nms_ws_bytes * (size_t)batch);
    if (rc) return rc;
    c->nms_ws = w;               // the smaller workspace stays owned by the context until ss_destroy
    c->nms_units = batch;
    return SS_OK;
}

extern "C" int ss_nms_batch(ss_ctx* c, const float* pred, int batch, long long pred_batch_stride, int n_anchors, int nc,
                            int n_extra, float conf_thres, float iou_thres, int agnostic, float max_wh, int max_det,
                            const float* d_geom, float* rows, int row_stride, long long rows_batch_stride, int* keep,
                            long long keep_batch_stride, int* count)
{
    if (!c || !pred || !d_geom || !rows || !keep || !count || row_stride < 6 + n_extra || batch < 0 || batch > 65535)
        return fail(c, SS_ERR_INVALID, "ss_nms_batch: bad argument");
    int rc = nms_reserve(c, batch);
    if (rc) return rc;
    rc = ss_launch_nms(pred, batch, pred_batch_stride, n_anchors, nc, n_extra, conf_thres, iou_thres, agnostic, max_wh,
                       max_det, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, d_geom, rows, row_stride, rows_batch_stride, keep,
                       keep_batch_stride, count, c->nms_ws, c->nms_ws_bytes * (size_t)c->nms_units, c->cls_mask[0], c->cls_mask[1],
                       c->stream);
    if (rc) return fail(c, rc, "ss_nms_batch: anchors exceed the workspace (n_anchors <= 32768)");
    HIPCHK(c, hipGetLastError());
    return SS_OK;
}

extern "C" int ss_nms_obb_batch(ss_ctx* c, const float* pred, int batch, long long pred_batch_stride, int n_anchors, int nc,
                                float conf_thres, float iou_thres, int agnostic, int max_det, const float* d_geom, float* rows,
                                int row_stride, long long rows_batch_stride, int* keep, long long keep_batch_stride, int* count)
{
    if (!c || !pred || !d_geom || !rows || !keep || !count || row_stride < 11 || batch < 0 || batch > 65535 || nc < 1 || n_anchors < 0)
        return fail(c, SS_ERR_INVALID, "ss_nms_obb_batch: bad argument");
    int rc = nms_reserve(c, batch);
    if (rc) return rc;
    rc = ss_launch_nms_obb(pred, batch, pred_batch_stride, n_anchors, nc, conf_thres, iou_thres, agnostic, max_det, d_geom, rows, row_stride,
                           rows_batch_stride, keep, keep_batch_stride, count, c->nms_ws, c->nms_ws_bytes * (size_t)c->nms_units,
                           c->cls_mask[0], c->cls_mask[1], c->stream);
    if (rc) return fail(c, rc, "ss_nms_obb_batch: anchors exceed the workspace (n_anchors <= 32768)");
    HIPCHK(c, hipGetLastError());
    return SS_OK;
}

// synchronous known-answer entry: host lists in, the device function on every pair, host matrix out
extern "C" int ss_probiou(ss_ctx* c, const float* h_a, int n, const float* h_b, int m, double* h_out)
{
    if (!c || n < 0 || m < 0 || n > 4096 || m > 4096 || ((n > 0 && !h_a) || (m > 0 && !h_b) || (n > 0 && m > 0 && !h_out)))
        return fail(c, SS_ERR_INVALID, "ss_probiou: null argument or a list outside 0..4096");
    if (n == 0 || m == 0) return SS_OK;
    SsBuf<SS_DEVICE> da, db, dout;
    HIPCHK(c, da.reserve((size_t)n * 5 * sizeof(float), SS_EXACT));
    HIPCHK(c, db.reserve((size_t)m * 5 * sizeof(float), SS_EXACT));
    HIPCHK(c, dout.reserve((size_t)n * m * sizeof(double), SS_EXACT));
    HIPCHK(c, hipMemcpyAsync(da.as(), h_a, (size_t)n * 5 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(db.as(), h_b, (size_t)m * 5 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    ss_launch_probiou(da.as<float>(), n, db.as<float>(), m, dout.as<double>(), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_out, dout.as(), (size_t)n * m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SS_OK;
}

extern "C" int ss_nms_set_classes(ss_ctx* c, const int* classes, int n)
{
    if (!c || n < 0 || (n > 0 && !classes)) return fail(c, SS_ERR_INVALID, "ss_nms_set_classes: bad argument");
    if (n == 0) { c->cls_mask[0] = c->cls_mask[1] = ~0ull; return SS_OK; }
    unsigned long long m[2] = { 0, 0 };
    for (int i = 0; i < n; ++i) {
        if (classes[i] < 0 || classes[i] >= 128) return fail(c, SS_ERR_INVALID, "ss_nms_set_classes: class ids 0..127");
        m[classes[i] >> 6] |= 1ull << (classes[i] & 63);
    }
    c->cls_mask[0] = m[0]; c->cls_mask[1] = m[1];
    return SS_OK;
}

extern "C" int ss_nms(ss_ctx* c, const float* pred, int n_anchors, int nc, int n_extra, float conf_thres,
                      float iou_thres, int agnostic, float max_wh, int max_det, float gain, float pad_x,
                      float pad_y, float w0, float h0, float* rows, int row_stride, int* keep, int* count)
{
    if (!c || !pred || !rows || !keep || !count || row_stride < 6 + n_extra)
        return fail(c, SS_ERR_INVALID, "ss_nms: bad argument");
    int rc = ss_launch_nms(pred, 1, 0, n_anchors, nc, n_extra, conf_thres, iou_thres, agnostic, max_wh, max_det, gain,
                           pad_x, pad_y, w0, h0, nullptr, rows, row_stride, 0, keep, 0, count, c->nms_ws,
                           c->nms_ws_bytes * (size_t)c->nms_units, c->cls_mask[0], c->cls_mask[1], c->stream);
    if (rc) return fail(c, rc, "ss_nms: anchors exceed the workspace (n_anchors <= 32768)");
    HIPCHK(c, hipGetLastError());
    return SS_OK;
}

extern "C" int ss_crop_norm_batch(ss_ctx* c, const uint8_t* frames, int batch, long long frame_batch_stride, int h,
                                  int w, int stride, const float* dets, int det_stride, long long dets_batch_stride,
                                  int n, const int* d_counts, void* out, int out_flags)
{
    if (!c || !frames || !dets || !out || batch < 0 || n < 0 || (long long)batch * n > 65535)
        return fail(c, SS_ERR_INVALID, "ss_crop_norm: bad argument (batch * n <= 65535)");
    if ((out_flags & 4) && !(out_flags & 2)) return fail(c, SS_ERR_INVALID, "ss_crop_norm: SS_DST_U8 needs SS_DST_HWC");
    ss_launch_crop(frames, batch, frame_batch_stride, h, w, stride, dets, det_stride, dets_batch_stride, n, d_counts, out,
                   out_flags, c->stream, nullptr);
    HIPCHK(c, hipGetLastError());
    return SS_OK;
}

// Packed form: d_off[batch + 1] <- exclusive prefix of min(count, n) (d_off[batch] = crops in total), crop d of image i is
// written at slot d_off[i] + d.  The network behind it then computes *(d_off + batch) crops (ss_op_set_valid_images) and
// ss_unpack_feats puts the embeddings back at [image][d].
extern "C" int ss_crop_norm_packed(ss_ctx* c, const uint8_t* frames, int batch, long long frame_batch_stride, int h, int w,
                                   int stride, const float* dets, int det_stride, long long dets_batch_stride, int n,
                                   const int* d_counts, int* d_off, void* out, int out_flags)
{
    if (!c || !frames || !dets || !out || !d_counts || !d_off || batch < 1 || n < 1 || (long long)batch * n > 65535 || !(out_flags & 2))
        return fail(c, SS_ERR_INVALID, "ss_crop_norm_packed: bad argument (channels-last output, batch * n <= 65535)");
    ss_launch_crop_offsets(d_counts, batch, n, d_off, c->stream);
    ss_launch_crop(frames, batch, frame_batch_stride, h, w, stride, dets, det_stride, dets_batch_stride, n, d_counts, out,
                   out_flags, c->stream, d_off);
    HIPCHK(c, hipGetLastError());
    return SS_OK;
}

extern "C" int ss_unpack_feats(ss_ctx* c, const void* d_emb, int emb_half, const int* d_off, const int* d_counts, int batch, int n,
                               float* d_feats, long long feats_image_stride)
{
    if (!c || !d_emb || !d_off || !d_counts || !d_feats || batch < 1 || n < 1 || n > 65535 || batch > 65535)
        return fail(c, SS_ERR_INVALID, "ss_unpack_feats: bad argument");
    ss_launch_unpack_feats(d_emb, emb_half, d_off, d_counts, batch, n, d_feats, feats_image_stride, c->stream);
    HIPCHK(c, hipGetLastError());
    return SS_OK;
}

extern "C" int ss_pack_results(ss_ctx* c, const int* d_n_dets, const float* d_dets, int det_ld, int det_cap, const int* d_n_out,
                               const float* d_out, int out_ld, int out_cap, float* d_dst)
{
    if (!c || !d_n_dets || !d_dets || !d_dst || det_ld < 1 || det_cap < 1 || ((d_n_out || d_out) && (!d_n_out || !d_out || out_ld < 1 || out_cap < 1)))
        return fail(c, SS_ERR_INVALID, "ss_pack_results: bad argument");
    ss_launch_pack_results(d_n_dets, d_dets, det_ld, det_cap, d_n_out, d_out, out_ld, out_cap, d_dst, c->stream);
    HIPCHK(c, hipGetLastError());
    return SS_OK;
}

extern "C" int ss_crop_norm(ss_ctx* c, const uint8_t* frame, int h, int w, int stride, const float* dets,
                            int det_stride, int n, const int* d_count, void* out, int out_flags)
{
    return ss_crop_norm_batch(c, frame, 1, 0, h, w, stride, dets, det_stride, 0, n, d_count, out, out_flags);
}

// §1d: BoT-SORT's `model: auto` features of the kept rows from the detector's head inputs (ss_native.hip k_native_feats).  Every
// argument is checked before the device is touched; one launch on the context's stream (capturable).
extern "C" int ss_native_feats(ss_ctx* c, int n_img, int half, const ss_native_map* maps, int s, const int* d_keep, long long keep_stride,
                               const int* d_counts, float* d_out)
{
    if (!c || !maps || !d_keep || !d_counts || !d_out) return fail(c, SS_ERR_INVALID, "ss_native_feats: null argument");
    if (n_img < 1 || n_img > 65535 || (half != 0 && half != 1) || s < 1 || s > SS_F || keep_stride < SS_MAXD)
        return fail(c, SS_ERR_INVALID, "ss_native_feats: 1 <= n_img <= 65535, half 0 / 1, 1 <= s <= 512, keep_stride >= 128");
    const void* p[3];
    long long is[3], rs[3], ps[3];
    int ch[3], h[3], w[3];
    long long anchors = 0;
    const size_t esz = half ? 2 : 4;
    for (int l = 0; l < 3; ++l) {
        const ss_native_map& m = maps[l];
        p[l] = m.data; is[l] = m.img_stride; rs[l] = m.row_stride; ps[l] = m.pix_stride;
        ch[l] = m.channels; h[l] = m.height; w[l] = m.width;
        if (!m.data || ((uintptr_t)m.data % esz) != 0) return fail(c, SS_ERR_INVALID, "ss_native_feats: a map is NULL or misaligned");
        if (m.channels < s || m.channels % s != 0) return fail(c, SS_ERR_INVALID, "ss_native_feats: every level's channels must be a multiple of s");
        if (m.height < 1 || m.width < 1 || m.pix_stride < m.channels || m.row_stride < (long long)m.width * m.pix_stride
            || (n_img > 1 && m.img_stride < (long long)m.height * m.row_stride))
            return fail(c, SS_ERR_INVALID, "ss_native_feats: bad map shape or strides (channel stride 1, maps must not overlap)");
        anchors += (long long)m.height * m.width;
    }
    if (anchors > 0x7fffffffLL) return fail(c, SS_ERR_INVALID, "ss_native_feats: too many anchors");
    ss_launch_native_feats(n_img, half, p, is, rs, ps, ch, h, w, s, d_keep, keep_stride, d_counts, d_out, c->stream);
    HIPCHK(c, hipGetLastError());
    return SS_OK;
}

// ---- inspection ----------------------------------------------------------------------------------------
extern "C" int ss_get_tracks(ss_ctx* c, int s, int cap, int* n_tracks, int* next_id, int* track_id, int* state,
                             int* hits, int* age, int* tsu, int* class_id, float* conf, double* mean,
                             double* cov, float* smooth, int* gal_count)
{
    if (!c || s < 0 || s >= c->dev.S) return fail(c, SS_ERR_INVALID, "ss_get_tracks: bad stream");
    if (int rcj = chain_join(c, c->stream)) return rcj;               // a detached chain wrote what this call reads
    HIPCHK(c, hipStreamSynchronize(c->stream));
    SSDev& d = c->dev;
    int nt = 0, nid = 0;
    HIPCHK(c, hipMemcpy(&nt, d.n_tracks + s, 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&nid, d.next_id + s, 4, hipMemcpyDeviceToHost));
    if (n_tracks) *n_tracks = nt;
    if (next_id) *next_id = nid;
    if (nt > cap) return fail(c, SS_ERR_CAPACITY, "ss_get_tracks: cap too small");
    const size_t T = SS_MAXT, sb = (size_t)s * T;
    std::vector<int> order(T);
    HIPCHK(c, hipMemcpy(order.data(), d.order + sb, T * 4, hipMemcpyDeviceToHost));
    auto column = [&](const auto* src, auto* dst) { return ss_gather_device(order.data(), nt, src + sb, T, 1, dst) != hipSuccess; };
    if (column(d.track_id, track_id) || column(d.state, state) || column(d.hits, hits) || column(d.age, age) || column(d.tsu, tsu) ||
        column(d.class_id, class_id) || column(d.gal_count, gal_count) || column(d.conf, conf))
        return fail(c, SS_ERR_HIP, "ss_get_tracks: copy failed");
    for (int i = 0; i < nt; ++i) {
        const size_t g = sb + order[i];
        if (mean) HIPCHK(c, hipMemcpy(mean + (size_t)i * 8, d.mean + g * 8, 64, hipMemcpyDeviceToHost));
        if (cov) HIPCHK(c, hipMemcpy(cov + (size_t)i * 64, d.cov + g * 64, 512, hipMemcpyDeviceToHost));
        if (smooth) {
            int sel = 0;
            HIPCHK(c, hipMemcpy(&sel, d.smooth_sel + g, 4, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(smooth + (size_t)i * SS_F, d.smooth + (g * 2 + (sel & 1)) * SS_F, SS_F * 4, hipMemcpyDeviceToHost));
        }
    }
    return SS_OK;
}

extern "C" int ss_get_debug(ss_ctx* c, int s, int frame, int* counts, float* cosd, double* maha, uint8_t* gated,
                            double* cost_a, double* cost_b, int* lists)
{
    if (!c || s < 0 || s >= c->dev.S || frame < 0 || frame >= SS_FMAX) return fail(c, SS_ERR_INVALID, "ss_get_debug: bad stream / frame");
    if (int rcj = chain_join(c, c->stream)) return rcj;               // a detached chain wrote what this call reads
    if (!c->cfg.debug) return fail(c, SS_ERR_INVALID, "ss_get_debug: context created without debug");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    SSDev& d = c->dev;
    const size_t fs = (size_t)frame * d.S + s;                     // [F][S] layout of the group
    const size_t n = (size_t)SS_MAXT * SS_MAXD, o = fs * n;
    if (counts) HIPCHK(c, hipMemcpy(counts, d.dbg_counts + fs * 8, 24, hipMemcpyDeviceToHost));
    if (cosd) HIPCHK(c, hipMemcpy(cosd, d.dbg_cos + o, n * 4, hipMemcpyDeviceToHost));
    if (maha) HIPCHK(c, hipMemcpy(maha, d.dbg_maha + o, n * 8, hipMemcpyDeviceToHost));
    if (gated) HIPCHK(c, hipMemcpy(gated, d.dbg_gated + o, n, hipMemcpyDeviceToHost));
    if (cost_a) HIPCHK(c, hipMemcpy(cost_a, d.dbg_cost_a + o, n * 8, hipMemcpyDeviceToHost));
    if (cost_b) HIPCHK(c, hipMemcpy(cost_b, d.dbg_cost_b + o, n * 8, hipMemcpyDeviceToHost));
    if (lists) HIPCHK(c, hipMemcpy(lists, d.dbg_lists + fs * 4 * SS_MAXT, 4 * SS_MAXT * 4, hipMemcpyDeviceToHost));
    return SS_OK;
}

extern "C" int ss_get_gallery(ss_ctx* c, int s, int track_index, float* rows, int cap_rows, int* count)
{
    if (!c || s < 0 || s >= c->dev.S || track_index < 0 || track_index >= SS_MAXT) return fail(c, SS_ERR_INVALID, "ss_get_gallery: bad argument");
    if (int rcj = chain_join(c, c->stream)) return rcj;               // a detached chain wrote what this call reads
    HIPCHK(c, hipStreamSynchronize(c->stream));
    SSDev& d = c->dev;
    int slot = 0, cnt = 0;
    HIPCHK(c, hipMemcpy(&slot, d.order + (size_t)s * SS_MAXT + track_index, 4, hipMemcpyDeviceToHost));
    const size_t g = (size_t)s * SS_MAXT + slot;
    HIPCHK(c, hipMemcpy(&cnt, d.gal_count + g, 4, hipMemcpyDeviceToHost));
    if (count) *count = cnt;
    if (!rows) return SS_OK;
    if (cnt > cap_rows) return fail(c, SS_ERR_CAPACITY, "ss_get_gallery: cap too small");
    std::vector<float> frag((size_t)SS_NRT * SS_TILE_FLOATS);
    HIPCHK(c, hipMemcpy(frag.data(), d.gallery + g * SS_NRT * SS_TILE_FLOATS, frag.size() * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < cnt; ++b)
        for (int k = 0; k < SS_F; ++k)
            rows[(size_t)b * SS_F + k] = frag[(size_t)(b / SS_TILE) * SS_TILE_FLOATS + ss_frag_index(b % SS_TILE, k)];
    return SS_OK;
}

extern "C" int ss_assoc_inkernel_timing(ss_ctx* c, int enable, double* mean_us, int* launches)
{
    if (!c) return SS_ERR_INVALID;
    if (int rcj = chain_join(c, c->stream)) return rcj;               // a detached chain wrote what this call reads
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsigned long long t[4] = { 0, 0, 0, 0 };
    HIPCHK(c, hipMemcpy(t, c->dev.tstamp, sizeof t, hipMemcpyDeviceToHost));
    if (c->inkernel && t[1] > t[0] && t[0] != ~0ull) { t[2] += t[1] - t[0]; t[3] += 1; }      // the last launch is not folded yet
    if (mean_us) *mean_us = t[3] ? (double)t[2] / (double)t[3] / 100.0 : 0.0;                   // 100 MHz ticks
    if (launches) *launches = (int)t[3];
    const unsigned long long arm[4] = { ~0ull, 0, 0, 0 };
    HIPCHK(c, hipMemcpy(c->dev.tstamp, arm, sizeof arm, hipMemcpyHostToDevice));
    c->inkernel = enable < 0 ? 0 : enable > 2 ? 2 : enable;
    return SS_OK;
}

extern "C" int ss_assoc_timeline(ss_ctx* c, long long* out, int n_workgroups)
{
    if (!c || !out || n_workgroups < 1 || n_workgroups > 4096) return SS_ERR_INVALID;
    if (int rcj = chain_join(c, c->stream)) return rcj;               // a detached chain wrote what this call reads
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->dev.timeline, (size_t)n_workgroups * 16 * 8, hipMemcpyDeviceToHost));
    return SS_OK;
}

// ---- sliced inference: tiled letterbox, cross-tile merge (ss_slice.hip, docs/SLICE.md) -----------------------------------------
extern "C" int ss_slice_max_tiles(void) { return ss_slice_max_tiles_impl(); }
extern "C" int ss_slice_max_candidates(void) { return ss_slice_max_candidates_impl(); }

extern "C" int ss_slice_config(ss_ctx* c, const int* h_tiles, int n_tiles, int frame_h, int frame_w, int canvas_h, int canvas_w, int rows_per_tile,
                               int n_extra, int n_kpt, float kpt_gain, float kpt_pad_x, float kpt_pad_y)
{
    return post_run(c, "ss_slice_config",
        [&](std::string& err) {
            return ss_slice_config_check_impl(h_tiles, n_tiles, frame_h, frame_w, canvas_h, canvas_w, rows_per_tile, n_extra, n_kpt, kpt_gain, kpt_pad_x,
                                              kpt_pad_y, err);
        },
        [&](std::string& err) {
            if (!c) { err = "ss_slice_config: null context"; return (int)SS_ERR_INVALID; }
            hipError_t e = hipStreamSynchronize(c->stream);          // nothing of a state this call replaces may still be in flight
            if (e != hipSuccess) { err = std::string("ss_slice_config: ") + hipGetErrorString(e); return (int)SS_ERR_HIP; }
            return ss_slice_config_impl(&c->slice, h_tiles, n_tiles, frame_h, frame_w, canvas_h, canvas_w, rows_per_tile, n_extra, n_kpt, kpt_gain,
                                        kpt_pad_x, kpt_pad_y, err);
        });
}

extern "C" int ss_slice_nms_geom(ss_ctx* c, float* d_geom, int batch)
{
    return post_run(c, "ss_slice_nms_geom",
        [&](std::string& err) {
            if (!d_geom || batch < 1 || batch > 65535) { err = "ss_slice_nms_geom: null output or batch outside 1..65535"; return (int)SS_ERR_INVALID; }
            return stage_state(c, "ss_slice_nms_geom", c && c->slice, "slice state (ss_slice_config)", -1, false, err);
        },
        [&](std::string& err) { return ss_slice_nms_geom_impl(c->slice, d_geom, batch, err); });
}

extern "C" int ss_slice_letterbox_batch(ss_ctx* c, const uint8_t* d_src, int batch, long long src_batch_stride, int row_stride, void* d_dst, int dst_flags,
                                        int pad_value)
{
    return post_run(c, "ss_slice_letterbox_batch",
        [&](std::string& err) {
            if (int rc = ss_slice_letterbox_check_impl(d_src, batch, src_batch_stride, row_stride, d_dst, dst_flags, pad_value, err)) return rc;
            return stage_state(c, "ss_slice_letterbox_batch", c && c->slice, "slice state (ss_slice_config)", -1, false, err);
        },
        [&](std::string& err) { return ss_slice_letterbox_impl(c->slice, c->stream, d_src, batch, src_batch_stride, row_stride, d_dst, dst_flags, pad_value, err); });
}

extern "C" int ss_slice_merge(ss_ctx* c, const float* d_rows, const int* d_counts, int batch, int row_stride, long long tile_stride, long long frame_stride,
                              int mode, int metric, float thr, int agnostic, int out_cap, float* d_out, int out_row_stride, long long out_frame_stride,
                              int* d_out_count, int* d_out_src, long long src_frame_stride)
{
    return post_run(c, "ss_slice_merge",
        [&](std::string& err) {
            if (int rc = ss_slice_merge_check_impl(d_rows, d_counts, batch, row_stride, tile_stride, frame_stride, mode, metric, thr, agnostic, out_cap, d_out,
                                                   out_row_stride, out_frame_stride, d_out_count, d_out_src, src_frame_stride, err))
                return rc;
            return stage_state(c, "ss_slice_merge", c && c->slice, "slice state (ss_slice_config)", -1, false, err);
        },
        [&](std::string& err) {
            return ss_slice_merge_impl(c->slice, c->stream, d_rows, d_counts, batch, row_stride, tile_stride, frame_stride, mode, metric, thr, agnostic,
                                       out_cap, d_out, out_row_stride, out_frame_stride, d_out_count, d_out_src, src_frame_stride, err);
        });
}

extern "C" int ss_assoc_timing(ss_ctx* c, int enable, float* mean_ms, int* launches)
{
    if (!c) return SS_ERR_INVALID;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double tot = 0;
    c->ev_ms.clear();
    for (size_t i = 0; i < c->ev_used; ++i) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[i].first, c->ev[i].second));
        tot += ms;
        c->ev_ms.push_back(ms);
    }
    if (mean_ms) *mean_ms = c->ev_used ? (float)(tot / c->ev_used) : 0.f;
    if (launches) *launches = (int)c->ev_used;
    c->ev_used = 0;
    c->timing = enable != 0;
    return SS_OK;
}

extern "C" int ss_assoc_timing_values(ss_ctx* c, float* out_ms, int cap, int* n)
{
    if (!c || !n || cap < 0 || (cap > 0 && !out_ms)) return SS_ERR_INVALID;
    *n = (int)c->ev_ms.size();
    for (int i = 0; i < cap && i < *n; ++i) out_ms[i] = c->ev_ms[i];
    return SS_OK;
}

// ---- identities across cameras: the track bank and the linking (ss_mtmc.hip, docs/MTMC.md) ----------------------------------------
extern "C" int ss_bank_max_ids(void) { return ss_bank_max_ids_impl(); }
extern "C" int ss_mtmc_max_tracklets(void) { return ss_mtmc_max_tracklets_impl(); }

extern "C" int ss_bank_create(ss_ctx* c, int max_ids)
{
    return create_run(c, "ss_bank_create", &ss_ctx::bank, ss_bank_free,
        [&](std::string& err) {
            if (max_ids < 1 || max_ids > ss_bank_max_ids_impl()) { err = "ss_bank_create: max_ids " + std::to_string(max_ids) + " outside 1.." + std::to_string(ss_bank_max_ids_impl()); return (int)SS_ERR_INVALID; }
            return (int)SS_OK;
        },
        [&](std::string& err) { return ss_bank_create_impl(&c->bank, c->stream, c->dev.S, max_ids, err); });
}

extern "C" int ss_bank_destroy(ss_ctx* c) { return stage_destroy(c, "ss_bank_destroy", &ss_ctx::bank, ss_bank_free); }

extern "C" int ss_bank_reset(ss_ctx* c, int stream)
{
    return post_run(c, "ss_bank_reset",
        [&](std::string& err) { return stage_state(c, "ss_bank_reset", c && c->bank, "bank (ss_bank_create)", stream, false, err); },
        [&](std::string& err) { return ss_bank_reset_impl(c->bank, c->stream, stream, err); });
}

extern "C" int ss_bank_update_group(ss_ctx* c, int n_frames, const float* d_rows, const int* d_nrows, const float* d_feats)
{
    return post_run(c, "ss_bank_update_group",
        [&](std::string& err) {
            if (int rc = ss_bank_update_check_impl(n_frames, d_rows, d_nrows, d_feats, err)) return rc;
            return stage_state(c, "ss_bank_update_group", c && c->bank, "bank (ss_bank_create)", -1, false, err);
        },
        [&](std::string& err) {
            if (int rc = chain_join(c, c->stream)) { err = c->err; return rc; }     // the rows of a detached tracker chain exist first
            return ss_bank_update_impl(c->bank, c->stream, n_frames, d_rows, d_nrows, d_feats, err);
        });
}

extern "C" int ss_bank_get(ss_ctx* c, int stream, int cap, int* n, int* ids, int* counts, int* first, int* last, int* cls, float* desc)
{
    return post_run(c, "ss_bank_get",
        [&](std::string& err) {
            if (!n || cap < 0 || (cap > 0 && (!ids || !counts || !first || !last || !cls || !desc))) { err = "ss_bank_get: null argument or negative cap"; return (int)SS_ERR_INVALID; }
            return stage_state(c, "ss_bank_get", c && c->bank, "bank (ss_bank_create)", stream, true, err);
        },
        [&](std::string& err) { return ss_bank_get_impl(c->bank, c->stream, stream, cap, n, ids, counts, first, last, cls, desc, err); });
}

extern "C" int ss_mtmc_link(ss_ctx* c, int T, const float* desc, const int* cam, const int* first, const int* last, const int* n, double thr, int min_rows,
                            int* global_id, double* merges, int* n_merges, float* dist_out)
{
    return post_run(c, "ss_mtmc_link",
        [&](std::string& err) { return ss_mtmc_link_check_impl(T, desc, cam, first, last, n, thr, min_rows, global_id, merges, n_merges, err); },
        [&](std::string& err) { return ss_mtmc_link_impl(c ? &c->mtmc : nullptr, c ? c->stream : nullptr, T, desc, cam, first, last, n, thr, min_rows, global_id,
                                                         merges, n_merges, dist_out, err); });
}

// ---- analytics behind the trackers: lines, zones, dwell, heat (ss_zone.hip, docs/ZONES.md) -----------------------------------
extern "C" int ss_zone_max_lines(void) { return ss_zone_max_lines_impl(); }
extern "C" int ss_zone_max_zones(void) { return ss_zone_max_zones_impl(); }
extern "C" int ss_zone_max_vertices(void) { return ss_zone_max_vertices_impl(); }
extern "C" int ss_zone_max_live(void) { return ss_zone_max_live_impl(); }

extern "C" int ss_zone_create(ss_ctx* c, const ss_zone_config* cfg, const int* lines, int n_lines, const int* poly_xy, const int* poly_off, int n_zones)
{
    return create_run(c, "ss_zone_create", &ss_ctx::zone, ss_zone_free,
        [&](std::string& err) { return ss_zone_create_check_impl(cfg, lines, n_lines, poly_xy, poly_off, n_zones, err); },
        [&](std::string& err) { return ss_zone_create_impl(&c->zone, c->stream, c->dev.S, cfg, lines, n_lines, poly_xy, poly_off, n_zones, err); });
}

extern "C" int ss_zone_destroy(ss_ctx* c) { return stage_destroy(c, "ss_zone_destroy", &ss_ctx::zone, ss_zone_free); }

extern "C" int ss_zone_reset(ss_ctx* c, int stream)
{
    return post_run(c, "ss_zone_reset",
        [&](std::string& err) { return stage_state(c, "ss_zone_reset", c && c->zone, "zone state (ss_zone_create)", stream, false, err); },
        [&](std::string& err) { return ss_zone_reset_impl(c->zone, c->stream, stream, err); });
}

extern "C" int ss_zone_update_group(ss_ctx* c, int n_frames, const float* d_rows, const int* d_nrows, uint32_t* d_events, uint32_t* d_inside,
                                    int* d_dwell, int* d_line_totals, int* d_occupancy, int* d_heat_frames, int* d_heat_max)
{
    return post_run(c, "ss_zone_update_group",
        [&](std::string& err) {
            if (int rc = ss_zone_update_check_impl(n_frames, d_rows, d_nrows, err)) return rc;
            return stage_state(c, "ss_zone_update_group", c && c->zone, "zone state (ss_zone_create)", -1, false, err);
        },
        [&](std::string& err) {
            return ss_zone_update_impl(c->zone, c->stream, n_frames, d_rows, d_nrows, d_events, d_inside, d_dwell, d_line_totals, d_occupancy,
                                       d_heat_frames, d_heat_max, err);
        });
}

extern "C" int ss_zone_get_totals(ss_ctx* c, int stream, int* frames, int* line_class, int* line_totals, int* zone_entries, int* zone_exits,
                                  long long* zone_dwell_sum, int* zone_longest, int* zone_peak, int* heat_max)
{
    return post_run(c, "ss_zone_get_totals",
        [&](std::string& err) { return stage_state(c, "ss_zone_get_totals", c && c->zone, "zone state (ss_zone_create)", stream, true, err); },
        [&](std::string& err) {
            return ss_zone_get_totals_impl(c->zone, c->stream, stream, frames, line_class, line_totals, zone_entries, zone_exits, zone_dwell_sum,
                                           zone_longest, zone_peak, heat_max, err);
        });
}

extern "C" int ss_zone_get_heat(ss_ctx* c, int stream, int* grid, int cap, int* gh, int* gw)
{
    return post_run(c, "ss_zone_get_heat",
        [&](std::string& err) {
            if (!gh || !gw || cap < 0 || (cap > 0 && !grid)) { err = "ss_zone_get_heat: null argument or negative cap"; return (int)SS_ERR_INVALID; }
            return stage_state(c, "ss_zone_get_heat", c && c->zone, "zone state (ss_zone_create)", stream, true, err);
        },
        [&](std::string& err) {
            int S, heat, h, w;
            ss_zone_shape_impl(c->zone, &S, &heat, gh, gw, &h, &w);
            if (!heat) { err = "ss_zone_get_heat: the zone state was made without a heat map"; return (int)SS_ERR_INVALID; }
            if (cap == 0) return (int)SS_OK;
            if (cap < *gh * *gw) { err = "ss_zone_get_heat: cap " + std::to_string(cap) + " is below the grid's " + std::to_string(*gh * *gw) + " cells"; return (int)SS_ERR_INVALID; }
            return ss_zone_get_heat_impl(c->zone, c->stream, stream, grid, err);
        });
}

extern "C" int ss_zone_heat_device(ss_ctx* c, int stream, void** d_heat, void** d_max)
{
    return post_run(c, "ss_zone_heat_device",
        [&](std::string& err) {
            if (!d_heat || !d_max) { err = "ss_zone_heat_device: null argument"; return (int)SS_ERR_INVALID; }
            return stage_state(c, "ss_zone_heat_device", c && c->zone, "zone state (ss_zone_create)", stream, true, err);
        },
        [&](std::string&) { ss_zone_heat_device_impl(c->zone, stream, d_heat, d_max); return (int)SS_OK; });
}

extern "C" int ss_zone_set_colormap(ss_ctx* c, const uint8_t* bgr_256x3)
{
    return post_run(c, "ss_zone_set_colormap",
        [&](std::string& err) {
            if (!bgr_256x3) { err = "ss_zone_set_colormap: null table"; return (int)SS_ERR_INVALID; }
            return stage_state(c, "ss_zone_set_colormap", c && c->zone, "zone state (ss_zone_create)", -1, false, err);
        },
        [&](std::string& err) { return ss_zone_set_colormap_impl(c->zone, bgr_256x3, err); });
}

extern "C" int ss_zone_heat_blend(ss_ctx* c, void* hip_stream, uint8_t* d_frames, int batch, long long frame_batch_stride, int h, int w, int row_stride,
                                  const int* d_heat, long long heat_frame_stride, const int* d_max, int max_stride, int alpha)
{
    return post_run(c, "ss_zone_heat_blend",
        [&](std::string& err) {
            if (int rc = ss_zone_blend_check_impl(d_frames, batch, frame_batch_stride, h, w, row_stride, d_heat, heat_frame_stride, d_max, max_stride, alpha, err))
                return rc;
            return stage_state(c, "ss_zone_heat_blend", c && c->zone, "zone state (ss_zone_create)", -1, false, err);
        },
        [&](std::string& err) {
            return ss_zone_blend_impl(c->zone, (hipStream_t)hip_stream, d_frames, batch, frame_batch_stride, h, w, row_stride, d_heat, heat_frame_stride,
                                      d_max, max_stride, alpha, err);
        });
}

// ---- redaction of regions of resident frames: blur, pixelate, fill (ss_redact.hip, docs/REDACT.md) ---------------------------------
extern "C" int ss_redact_max_regions(void) { return ss_redact_max_regions_impl(); }
extern "C" int ss_redact_max_vertices(void) { return ss_redact_max_vertices_impl(); }
extern "C" int ss_redact_max_radius(void) { return ss_redact_max_radius_impl(); }
extern "C" long long ss_redact_scratch_bytes(int batch, int h, int w) { return ss_redact_scratch_bytes_impl(batch, h, w); }

extern "C" int ss_redact(ss_ctx* c, void* hip_stream, uint8_t* d_frames, int batch, long long frame_batch_stride, int h, int w, int row_stride,
                         const int* d_regions, const int* d_region_off, const int* d_verts, int effect, int strength, int fill_bgr, void* d_scratch,
                         long long scratch_bytes)
{
    return post_run(c, "ss_redact",
        [&](std::string& err) {
            if (int rc = ss_redact_check_impl(d_frames, batch, frame_batch_stride, h, w, row_stride, d_regions, d_region_off, d_verts, effect, strength,
                                              fill_bgr, d_scratch, scratch_bytes, err))
                return rc;
            if (!c) { err = "ss_redact: null context"; return (int)SS_ERR_INVALID; }
            return (int)SS_OK;
        },
        [&](std::string& err) {
            return ss_redact_impl((hipStream_t)hip_stream, d_frames, batch, frame_batch_stride, h, w, row_stride, d_regions, d_region_off, d_verts, effect,
                                  strength, fill_bgr, d_scratch, err);
        });
}

// ---- the tracker families: BYTE (ss_byte.hip), OC-SORT (ss_ocsort.hip), Deep OC-SORT (ss_deepoc.hip), Hybrid-SORT (ss_hybrid.hip) --------------------------------
// Each family's state, tables, reset and read-back live beside its kernels; include/strongsort_hip.h says what each entry does.
// An entry that needs the state: ok (it is there and the entry's own arguments are sound) and the stream, all worded "no <what>".
template <class Work>
static int tracker_run(ss_ctx* c, const char* entry, bool ok, const char* what, int stream, bool need_stream, Work work)
{
    return post_run(c, entry, [&](std::string& err) { return stage_state(c, entry, ok, what, stream, need_stream, err, true); }, work);
}

static int invalid(std::string& err, const char* entry, const char* why) { err = std::string(entry) + ": " + why; return SS_ERR_INVALID; }

// An update entry: its arguments, a context that has the family's state, then launch(err): the mode's own checks and its launches on
// the context's stream.  Nothing else touches the device: capturable.
template <class Launch>
static int update_run(ss_ctx* c, const char* entry, bool pointers, int n_frames, bool have_state, const char* what, Launch launch)
{
    return post_run(c, entry,
        [&](std::string& err) {
            if (!pointers) return invalid(err, entry, "null argument");
            if (n_frames < 1 || n_frames > SS_FMAX) return invalid(err, entry, "1 <= n_frames <= SS_FMAX");
            return stage_state(c, entry, have_state, what, -1, false, err);
        },
        [&](std::string& err) {
            if (int rc = launch(err)) return rc;
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) { err = std::string(entry) + ": " + hipGetErrorString(e); return (int)SS_ERR_HIP; }
            return (int)SS_OK;
        });
}

static SsWarpFlags warp_flags(ss_ctx* c) { return {c->cmc_prev_valid, c->gmc.prev_valid}; }      // what a BYTE or Deep OC-SORT restart clears

// ---- OC-SORT (docs/OCSORT.md)
static const char *const OC_STATE = "OC-SORT state (ss_ocsort_create)", *const OC_OR_STREAM = "OC-SORT state or bad stream";

extern "C" int ss_ocsort_destroy(ss_ctx* c) { return stage_destroy(c, "ss_ocsort_destroy", &ss_ctx::oc, ss_ocsort_free); }

extern "C" int ss_ocsort_create(ss_ctx* c, const ss_ocsort_config* cfg)
{
    return create_run(c, "ss_ocsort_create", &ss_ctx::oc, ss_ocsort_free, [&](std::string& err) { return ss_ocsort_create_check_impl(cfg, err); },
                      [&](std::string& err) { return ss_ocsort_create_impl(&c->oc, c->stream, c->dev.S, cfg, err); });
}

extern "C" int ss_ocsort_reset(ss_ctx* c, int stream)
{
    return tracker_run(c, "ss_ocsort_reset", c && c->oc, OC_OR_STREAM, stream, false,
                       [&](std::string& err) { return ss_oc_reset_impl(ss_ocsort_dev(c->oc), c->stream, stream, "ss_ocsort_reset: ", err); });
}

extern "C" int ss_ocsort_update_group(ss_ctx* c, int n_frames, const float* d_dets, const int* d_ndets, float* d_out, int* d_nout)
{
    return update_run(c, "ss_ocsort_update_group", d_dets && d_ndets && d_out && d_nout, n_frames, c && c->oc, OC_STATE,
                      [&](std::string&) { ss_launch_ocsort_group(ss_ocsort_dev(c->oc), n_frames, d_dets, d_ndets, d_out, d_nout, c->stream); return (int)SS_OK; });
}

extern "C" int ss_ocsort_update(ss_ctx* c, const float* d_dets, const int* d_ndets, float* d_out, int* d_nout) { return ss_ocsort_update_group(c, 1, d_dets, d_ndets, d_out, d_nout); }

extern "C" int ss_ocsort_get_tracks(ss_ctx* c, int s, int cap, int* n_tracks, int* next_id, int* frame_count, int* track_id, int* age,
                                    int* time_since_update, int* hits, int* hit_streak, int* frozen, double* x, double* P, float* last_obs,
                                    double* velocity)
{
    return tracker_run(c, "ss_ocsort_get_tracks", c && c->oc && cap >= 0, OC_OR_STREAM, s, true, [&](std::string& err) {
        return ss_oc_get_tracks_impl(ss_ocsort_dev(c->oc), c->stream, "ss_ocsort_get_tracks", s, cap, n_tracks, next_id, frame_count, track_id, age,
                                     time_since_update, hits, hit_streak, frozen, x, P, last_obs, velocity, nullptr, err);
    });
}

// ---- Deep OC-SORT (docs/DEEPOCSORT.md)
static const char *const DEEPOC_STATE = "Deep OC-SORT state (ss_deepoc_create)", *const DEEPOC_OR_STREAM = "Deep OC-SORT state or bad stream";

extern "C" int ss_deepoc_destroy(ss_ctx* c) { return stage_destroy(c, "ss_deepoc_destroy", &ss_ctx::deepoc, ss_deepoc_free); }

extern "C" int ss_deepoc_create(ss_ctx* c, const ss_deepoc_config* cfg)
{
    return create_run(c, "ss_deepoc_create", &ss_ctx::deepoc, ss_deepoc_free, [&](std::string& err) { return ss_deepoc_create_check_impl(cfg, err); },
                      [&](std::string& err) { return ss_deepoc_create_impl(&c->deepoc, c->stream, warp_flags(c), c->dev.S, cfg, err); });
}

extern "C" int ss_deepoc_reset(ss_ctx* c, int stream)
{
    return tracker_run(c, "ss_deepoc_reset", c && c->deepoc, DEEPOC_OR_STREAM, stream, false,
                       [&](std::string& err) { return ss_deepoc_reset_impl(c->deepoc, c->stream, warp_flags(c), stream, err); });
}

extern "C" int ss_deepoc_set_gmc(ss_ctx* c, const double* d_warps)
{
    return tracker_run(c, "ss_deepoc_set_gmc", c && c->deepoc, DEEPOC_STATE, -1, false,
                       [&](std::string&) { ss_deepoc_set_gmc_impl(c->deepoc, d_warps); return (int)SS_OK; });
}

extern "C" int ss_deepoc_update_group(ss_ctx* c, int n_frames, const float* d_dets, const int* d_ndets, const float* d_feats, float* d_out,
                                      int* d_nout)
{
    const char* fn = "ss_deepoc_update_group";
    return update_run(c, fn, d_dets && d_ndets && d_out && d_nout, n_frames, c && c->deepoc, DEEPOC_STATE, [&](std::string& err) {
        const SSDeepOcDev& d = ss_deepoc_dev(c->deepoc);
        if (d.appearance && !d_feats) return invalid(err, fn, "appearance is on and d_feats is NULL");
        ss_launch_deepoc_group(d, n_frames, d_dets, d_ndets, d_feats, d_out, d_nout, c->stream);
        return (int)SS_OK;
    });
}

extern "C" int ss_deepoc_update(ss_ctx* c, const float* d_dets, const int* d_ndets, const float* d_feats, float* d_out, int* d_nout) { return ss_deepoc_update_group(c, 1, d_dets, d_ndets, d_feats, d_out, d_nout); }

extern "C" int ss_deepoc_get_tracks(ss_ctx* c, int s, int cap, int* n_tracks, int* next_id, int* frame_count, int* track_id, int* age,
                                    int* time_since_update, int* hits, int* hit_streak, int* frozen, double* x, double* P, float* last_obs,
                                    double* velocity)
{
    return tracker_run(c, "ss_deepoc_get_tracks", c && c->deepoc && cap >= 0, DEEPOC_OR_STREAM, s, true, [&](std::string& err) {
        return ss_oc_get_tracks_impl(ss_deepoc_dev(c->deepoc).oc, c->stream, "ss_deepoc_get_tracks", s, cap, n_tracks, next_id, frame_count, track_id,
                                     age, time_since_update, hits, hit_streak, frozen, x, P, last_obs, velocity, nullptr, err);
    });
}

extern "C" int ss_deepoc_get_features(ss_ctx* c, int s, int cap, float* emb)
{
    return tracker_run(c, "ss_deepoc_get_features", c && c->deepoc && cap >= 0 && emb, "Deep OC-SORT state, bad stream or NULL", s, true,
                       [&](std::string& err) { return ss_deepoc_get_features_impl(c->deepoc, c->stream, s, cap, emb, err); });
}

// ---- Hybrid-SORT (docs/HYBRIDSORT.md)
static const char *const HY_STATE = "Hybrid-SORT state (ss_hybridsort_create)", *const HY_OR_STREAM = "Hybrid-SORT state or bad stream";

extern "C" int ss_hybridsort_destroy(ss_ctx* c) { return stage_destroy(c, "ss_hybridsort_destroy", &ss_ctx::hybrid, ss_hybrid_free); }

extern "C" int ss_hybridsort_create(ss_ctx* c, const ss_hybridsort_config* cfg)
{
    return create_run(c, "ss_hybridsort_create", &ss_ctx::hybrid, ss_hybrid_free, [&](std::string& err) { return ss_hybrid_create_check_impl(cfg, err); },
                      [&](std::string& err) { return ss_hybrid_create_impl(&c->hybrid, c->stream, c->dev.S, cfg, err); });
}

extern "C" int ss_hybridsort_reset(ss_ctx* c, int stream)
{
    return tracker_run(c, "ss_hybridsort_reset", c && c->hybrid, HY_OR_STREAM, stream, false,
                       [&](std::string& err) { return ss_hybrid_reset_impl(c->hybrid, c->stream, stream, err); });
}

extern "C" int ss_hybridsort_update_group(ss_ctx* c, int n_frames, const float* d_dets, const int* d_ndets, float* d_out, int* d_nout)
{
    return update_run(c, "ss_hybridsort_update_group", d_dets && d_ndets && d_out && d_nout, n_frames, c && c->hybrid, HY_STATE,
                      [&](std::string&) { ss_launch_hybrid_group(ss_hybrid_dev(c->hybrid), n_frames, d_dets, d_ndets, d_out, d_nout, c->stream); return (int)SS_OK; });
}

extern "C" int ss_hybridsort_update(ss_ctx* c, const float* d_dets, const int* d_ndets, float* d_out, int* d_nout) { return ss_hybridsort_update_group(c, 1, d_dets, d_ndets, d_out, d_nout); }

extern "C" int ss_hybridsort_get_tracks(ss_ctx* c, int s, int cap, int* n_tracks, int* next_id, int* frame_count, int* track_id, int* age,
                                        int* time_since_update, int* hits, int* hit_streak, int* frozen, double* x, double* P, float* last_obs,
                                        double* velocity, float* conf, float* conf_prev)
{
    return tracker_run(c, "ss_hybridsort_get_tracks", c && c->hybrid && cap >= 0, HY_OR_STREAM, s, true, [&](std::string& err) {
        return ss_hybrid_get_tracks_impl(c->hybrid, c->stream, s, cap, n_tracks, next_id, frame_count, track_id, age, time_since_update, hits,
                                         hit_streak, frozen, x, P, last_obs, velocity, conf, conf_prev, err);
    });
}

// ---- BYTE tracker family (docs/BYTETRACK.md; oriented boxes: docs/OBB.md §4)
static const char *const BYTE_STATE = "BYTE state (ss_byte_create)", *const BYTE_OR_STREAM = "BYTE state or bad stream",
                  *const BYTE_OR_STREAM_NULL = "BYTE state, bad stream or NULL";

extern "C" int ss_byte_destroy(ss_ctx* c) { return stage_destroy(c, "ss_byte_destroy", &ss_ctx::byte, ss_byte_free); }

extern "C" int ss_byte_create(ss_ctx* c, const ss_byte_config* cfg)
{
    return create_run(c, "ss_byte_create", &ss_ctx::byte, ss_byte_free, [&](std::string& err) { return ss_byte_create_check_impl(cfg, err); },
                      [&](std::string& err) { return ss_byte_create_impl(&c->byte, c->stream, warp_flags(c), c->dev.S, cfg, err); });
}

extern "C" int ss_byte_reset(ss_ctx* c, int stream)
{
    return tracker_run(c, "ss_byte_reset", c && c->byte, BYTE_OR_STREAM, stream, false,
                       [&](std::string& err) { return ss_byte_reset_impl(c->byte, c->stream, warp_flags(c), stream, err); });
}

// ss_byte_update_group (d_feats NULL, feats_entry 0) and ss_byte_update_group_feats: up to two launches (unit features, then the group)
static int byte_update(ss_ctx* c, const char* fn, int feats_entry, int n_frames, const float* d_dets, const int* d_ndets, const float* d_feats,
                       float* d_out, int* d_nout)
{
    return update_run(c, fn, d_dets && d_ndets && d_out && d_nout, n_frames, c && c->byte, BYTE_STATE, [&](std::string& err) {
        const SSByteDev& b = ss_byte_dev(c->byte);
        if (!feats_entry && b.reid) return invalid(err, fn, "ReID is on, the features go through ss_byte_update_group_feats");
        if (b.reid && !d_feats) return invalid(err, fn, "ReID is on and d_feats is NULL");
        if (b.pose) return invalid(err, fn, "the keypoint term is on, the keypoints go through ss_byte_update_group_kpts");
        if (b.obb) return invalid(err, fn, "oriented boxes are on, the 11-column rows go through ss_byte_update_group_obb");
        ss_launch_byte_group(b, n_frames, d_dets, d_ndets, d_feats, d_out, d_nout, c->stream);
        return (int)SS_OK;
    });
}

extern "C" int ss_byte_update_group(ss_ctx* c, int n_frames, const float* d_dets, const int* d_ndets, float* d_out, int* d_nout)
{ return byte_update(c, "ss_byte_update_group", 0, n_frames, d_dets, d_ndets, nullptr, d_out, d_nout); }

extern "C" int ss_byte_update(ss_ctx* c, const float* d_dets, const int* d_ndets, float* d_out, int* d_nout) { return ss_byte_update_group(c, 1, d_dets, d_ndets, d_out, d_nout); }

extern "C" int ss_byte_update_group_feats(ss_ctx* c, int n_frames, const float* d_dets, const int* d_ndets, const float* d_feats,
                                          float* d_out, int* d_nout)
{ return byte_update(c, "ss_byte_update_group_feats", 1, n_frames, d_dets, d_ndets, d_feats, d_out, d_nout); }

extern "C" int ss_byte_update_group_kpts(ss_ctx* c, int n_frames, const float* d_dets, const int* d_ndets, const float* d_kpts,
                                         long long kpt_row_stride, int kpt_col_offset, const float* d_geom, float* d_out, int* d_nout)
{
    const char* fn = "ss_byte_update_group_kpts";
    return update_run(c, fn, d_dets && d_ndets && d_kpts && d_out && d_nout, n_frames, c && c->byte, BYTE_STATE, [&](std::string& err) {
        const SSByteDev& b = ss_byte_dev(c->byte);
        if (!b.pose) return invalid(err, fn, "the keypoint term is off (ss_byte_set_pose)");
        if (kpt_col_offset < 0 || kpt_row_stride < (long long)kpt_col_offset + 3 * b.nk)
            return invalid(err, fn, "kpt_col_offset >= 0, kpt_row_stride >= kpt_col_offset + 3 n_kpt");
        ss_launch_byte_group_kpts(b, n_frames, d_dets, d_ndets, d_kpts, kpt_row_stride, kpt_col_offset, d_geom, d_out, d_nout, c->stream);
        return (int)SS_OK;
    });
}

extern "C" int ss_byte_update_group_obb(ss_ctx* c, int n_frames, const float* d_dets, const int* d_ndets, float* d_out, float* d_out_rbox,
                                        int* d_nout)
{
    const char* fn = "ss_byte_update_group_obb";
    return update_run(c, fn, d_dets && d_ndets && d_out && d_out_rbox && d_nout, n_frames, c && c->byte, BYTE_STATE, [&](std::string& err) {
        if (!ss_byte_dev(c->byte).obb) return invalid(err, fn, "oriented boxes are off (ss_byte_set_obb)");
        ss_launch_byte_group_obb(ss_byte_dev(c->byte), n_frames, d_dets, d_ndets, d_out, d_out_rbox, d_nout, c->stream);
        return (int)SS_OK;
    });
}

extern "C" int ss_byte_set_reid(ss_ctx* c, int on, double proximity_thresh, double appearance_thresh, double alpha)
{
    return tracker_run(c, "ss_byte_set_reid", c && c->byte, BYTE_STATE, -1, false, [&](std::string& err) {
        return ss_byte_set_reid_impl(c->byte, c->stream, warp_flags(c), on, proximity_thresh, appearance_thresh, alpha, err);
    });
}

extern "C" int ss_byte_set_pose(ss_ctx* c, int on, int n_kpt, const double* sigmas, double proximity_thresh, double pose_thresh,
                                double vis_thresh, int min_common)
{
    return tracker_run(c, "ss_byte_set_pose", c && c->byte, BYTE_STATE, -1, false, [&](std::string& err) {
        return ss_byte_set_pose_impl(c->byte, c->stream, warp_flags(c), on, n_kpt, sigmas, proximity_thresh, pose_thresh, vis_thresh, min_common, err);
    });
}

extern "C" int ss_byte_set_obb(ss_ctx* c, int on)
{
    return tracker_run(c, "ss_byte_set_obb", c && c->byte, BYTE_STATE, -1, false,
                       [&](std::string& err) { return ss_byte_set_obb_impl(c->byte, c->stream, warp_flags(c), on, err); });
}

extern "C" int ss_byte_set_gmc(ss_ctx* c, const double* d_warps)
{
    return tracker_run(c, "ss_byte_set_gmc", c && c->byte, BYTE_STATE, -1, false,
                       [&](std::string& err) { return ss_byte_set_gmc_impl(c->byte, d_warps, err); });
}

// the read-backs of one stream, each in list order (tracked, then lost): ss_byte_get_impl fills the tables r names
static int byte_get(ss_ctx* c, const char* fn, bool ok, const char* what, int s, int cap, const SsByteRows& r)
{
    return tracker_run(c, fn, c && c->byte && cap >= 0 && ok, what, s, true,
                       [&](std::string& err) { return ss_byte_get_impl(c->byte, c->stream, fn, s, cap, r, err); });
}

extern "C" int ss_byte_get_tracks(ss_ctx* c, int s, int cap, int* n_tracked, int* n_lost, int* next_id, int* frame_id,
                                  int* track_id, int* state, int* activated, double* mean)
{
    SsByteRows r;
    r.n_tracked = n_tracked; r.n_lost = n_lost; r.next_id = next_id; r.frame_id = frame_id; r.track_id = track_id; r.state = state; r.activated = activated; r.mean = mean;
    return byte_get(c, "ss_byte_get_tracks", true, BYTE_OR_STREAM, s, cap, r);
}

extern "C" int ss_byte_get_features(ss_ctx* c, int s, int cap, float* smooth)
{ SsByteRows r; r.smooth = smooth; return byte_get(c, "ss_byte_get_features", smooth, BYTE_OR_STREAM_NULL, s, cap, r); }

extern "C" int ss_byte_get_keypoints(ss_ctx* c, int s, int cap, double* offsets, unsigned* visible)
{ SsByteRows r; r.offsets = offsets; r.visible = visible; r.pose = true; return byte_get(c, "ss_byte_get_keypoints", true, BYTE_OR_STREAM, s, cap, r); }

extern "C" int ss_byte_get_angles(ss_ctx* c, int s, int cap, float* angles)
{ SsByteRows r; r.angles = angles; return byte_get(c, "ss_byte_get_angles", angles, BYTE_OR_STREAM_NULL, s, cap, r); }

extern "C" int ss_byte_get_det_keypoints(ss_ctx* c, int frame, int s, float* xy, unsigned* visible)
{
    return tracker_run(c, "ss_byte_get_det_keypoints", c && c->byte && frame >= 0 && frame < SS_FMAX && xy && visible, "BYTE state, bad frame / stream or NULL", s, true,
                       [&](std::string& err) { return ss_byte_get_det_keypoints_impl(c->byte, c->stream, frame, s, xy, visible, err); });
}
