// ss_deepoc.hip — the Deep OC-SORT tracker on the device (docs/DEEPOCSORT.md): S independent streams, a GROUP of F <= SS_FMAX frames
// per call.
//
//   k_deepoc_feats  (appearance only, before k_deepoc_group in the same call) one wave per high-score detection row of the group:
//                   so_normalize of the raw 512-float feature into ufeat.
//   k_deepoc_group  ss_ocsort_body.h's frame procedure (OC-SORT without the BYTE stage) with the three additions defined here:
//                   deepoc_cmc         step 1b: the warp of ss_cmc_estimate / ss_gmc_sparse_estimate applied to every track's filter,
//                                      frozen filter, last observation and ring of observations, before the predict;
//                   deepoc_appearance  the similarities E of the high rows and the tracks' features (all four waves, eight lanes per
//                                      pair), the adaptive weights, and the appearance cost added to the matrix the LSAP solves;
//                   deepoc_features    the births' features and the matched tracks' EMA, its weight following the detection score.
//                   One launch per call, no host round trip: capturable.
//
// tests/deepocsort_ref.py restates every step in the same order (rows, tables and features are compared bit for bit).
#include "ss_ocsort_body.h"

// step 1b on one filter in global memory: x[0:2] = R x[0:2] + t, x[4:6] = R x[4:6], and the diagonal 2x2 blocks of P at 0 and 4
// become R B R^T (X = R B, then X R^T).  Every entry is two products and one add (-ffp-contract=off).  Nothing else moves (DO-03).
__device__ inline void deepoc_warp_filter(double* x, double* P, const double* w)
{
    const double r00 = w[0], r01 = w[1], r10 = w[3], r11 = w[4];
    const double u = x[0], v = x[1], a = x[4], b = x[5];
    x[0] = (r00 * u + r01 * v) + w[2];
    x[1] = (r10 * u + r11 * v) + w[5];
    x[4] = r00 * a + r01 * b;
    x[5] = r10 * a + r11 * b;
#pragma unroll
    for (int o = 0; o < 8; o += 4) {
        double* q = P + o * 7 + o;
        const double b00 = q[0], b01 = q[1], b10 = q[7], b11 = q[8];
        const double x00 = r00 * b00 + r01 * b10, x01 = r00 * b01 + r01 * b11;
        const double x10 = r10 * b00 + r11 * b10, x11 = r10 * b01 + r11 * b11;
        q[0] = x00 * r00 + x01 * r01; q[1] = x00 * r10 + x01 * r11;
        q[7] = x10 * r00 + x11 * r01; q[8] = x10 * r10 + x11 * r11;
    }
}

// both corners of a float32 xyxy box moved as points, p' = R p + t in f64, rounded to float32 once
__device__ inline void deepoc_warp_box(float* b, const double* w)
{
    const double x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
    b[0] = (float)((w[0] * x1 + w[1] * y1) + w[2]);
    b[1] = (float)((w[3] * x1 + w[4] * y1) + w[5]);
    b[2] = (float)((w[0] * x2 + w[1] * y2) + w[2]);
    b[3] = (float)((w[3] * x2 + w[4] * y2) + w[5]);
}

// step 1b (thread = list position), before the predict: the ages are those before this frame's increment
__device__ inline void deepoc_cmc(const SSOcDev& o, const double* w, size_t sb, int nT, OcLds& m)
{
    const int tid = threadIdx.x, D = o.delta_t;
    if (tid < nT) {
        const int slot = m.trk[tid];
        const size_t g = sb + slot;
        deepoc_warp_filter(o.x + g * 7, o.P + g * 49, w);
        if (o.frozen[g]) deepoc_warp_filter(o.xf + g * 7, o.Pf + g * 49, w);
        if (m.hasobs[slot]) deepoc_warp_box(m.lobs[slot], w);
        const int age = m.age[slot];
        for (int e = 0; e < D; ++e) {
            const int a = o.rage[g * SS_OC_MAXDT + e];
            if (a >= 0 && a >= age - D && a <= age) deepoc_warp_box(o.ring + (g * SS_OC_MAXDT + e) * 4, w);
        }
    }
    __syncthreads();
}

// the factor of a row or column from its largest and second largest similarity (values: a tie gives m2 == m1):
// 0 if m1 == 0, else 1 - max(m2 / m1 - aw, 0) / (1 - aw) (docs/DEEPOCSORT.md DO-07)
__device__ inline double deepoc_factor(double m1, double m2, double aw)
{
    if (m1 == 0.0) return 0.0;
    double d = m2 / m1 - aw;
    d = d > 0.0 ? d : 0.0;
    return 1.0 - d / (1.0 - aw);
}

// one more value into a running (largest, second largest)
__device__ inline void deepoc_top2(double a, double& m1, double& m2)
{
    if (a > m1) { m2 = m1; m1 = a; }
    else if (a > m2) m2 = a;
}

// The appearance cost of the first association, nHi high rows x nT tracks, when the LSAP runs.  `cost` holds -(iou + term) by
// lsap_cidx (each entry written by the thread that revisits it here).
//   E[r][k] = (double) so_dot(curr_r, emb_k) where iou > 0, else 0 (a dead track's IoU is 0).  The entries go by chunks of 256, one
//             thread each for the IoU test; the overlapping pairs are compacted (m.freel, free until the births) and eight lanes per
//             pair run so_dot's eight 64-long fmaf chains (lane = segment), lane 0 of the eight adding them in segment order.
//   rf / cf   the adaptive factors (1 where there is one column / row, or without adaptive weighting): a wave per row, its lanes
//             striding the row and merging their (largest, second largest) pairs by a butterfly; a thread per column (its loads
//             are coalesced across the wave).  The two largest are values, so no order of the comparisons matters.
//   cost      -((iou + term) + ((w * rf[r]) * cf[k]) * E[r][k]).
__device__ inline void deepoc_appearance(const SSDeepOcDev& x, int nHi, int nT, double* cost, size_t s, size_t fs, OcLds& m, DeepLds& dl)
{
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, seg = tid & 7, base = l & ~7, n = nHi * nT;
    const size_t sb = s * SS_MAXT;
    double* E = x.E + s * SS_MAXT * SS_MAXD;
    for (int e0 = 0; e0 < n; e0 += 256) {
        const int e = e0 + tid;
        int need = 0;
        if (e < n) {
            const int r = e / nT, k = e - r * nT;
            need = m.mdet[k] != SS_OC_DEAD && oc_iou(m.dbox[m.hi[r]], m.pbox[k]) > 0.0;
            if (!need) E[e] = 0.0;
        }
        int pos, nA;
        block_scan256(need, m.wtot, pos, nA);
        if (need) m.freel[pos] = e;
        __syncthreads();
        for (int j0 = 0; j0 < nA; j0 += 32) {
            const int j = j0 + (tid >> 3);
            int ee = 0;
            float p = 0.0f;
            if (j < nA) {
                ee = m.freel[j];
                const int r = ee / nT, k = ee - r * nT;
                const float4* g = reinterpret_cast<const float4*>(x.emb + (sb + m.trk[k]) * SS_F + SS_SEG * seg);
                const float4* q = reinterpret_cast<const float4*>(x.ufeat + (fs * SS_MAXD + m.hi[r]) * SS_F + SS_SEG * seg);
#pragma unroll 8
                for (int i = 0; i < SS_SEG / 4; ++i) {
                    const float4 a = q[i], b = g[i];
                    p = fmaf(a.x, b.x, p); p = fmaf(a.y, b.y, p); p = fmaf(a.z, b.z, p); p = fmaf(a.w, b.w, p);
                }
            }
            float tot = __shfl(p, base);
#pragma unroll
            for (int i = 1; i < SS_NSEG; ++i) tot = tot + __shfl(p, base + i);
            if (j < nA && seg == 0) E[ee] = (double)tot;
        }
        __syncthreads();                                           // m.freel: the next chunk's
    }
    __threadfence();                                               // E is read back by other threads
    __syncthreads();
    if (x.adaptive && nT >= 2) {
        for (int r = w; r < nHi; r += 4) {                         // the same rows for the whole wave
            double m1 = -INFINITY, m2 = -INFINITY;
            for (int k = l; k < nT; k += 64) deepoc_top2(E[(size_t)r * nT + k], m1, m2);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {              // top 2 of the union of two (largest, second largest) pairs
                const double b1 = __shfl_xor(m1, off), b2 = __shfl_xor(m2, off);
                const double lo = m1 > b1 ? b1 : m1, s2 = m2 > b2 ? m2 : b2;
                m1 = m1 > b1 ? m1 : b1;
                m2 = lo > s2 ? lo : s2;
            }
            if (l == 0) dl.rf[r] = deepoc_factor(m1, m2, x.aw);
        }
    } else if (tid < nHi) dl.rf[tid] = 1.0;
    if (tid < nT) {
        double f = 1.0;
        if (x.adaptive && nHi >= 2) {
            double m1 = -INFINITY, m2 = -INFINITY;
            for (int r = 0; r < nHi; ++r) deepoc_top2(E[(size_t)r * nT + tid], m1, m2);
            f = deepoc_factor(m1, m2, x.aw);
        }
        dl.cf[tid] = f;
    }
    __syncthreads();
    for (int e = tid; e < n; e += 256) {
        const int r = e / nT, k = e - r * nT;
        const double W = (x.w_emb * dl.rf[r]) * dl.cf[k];
        const double A = W * E[e];
        const int i = lsap_cidx(r, k, nHi, nT);
        cost[i] = -(-cost[i] + A);
    }
}

// The features after the frame's updates: a birth copies its row's unit feature; a matched track (first association or OCR) takes
// so_ema(emb, curr, (float)alpha, (float)(1.0 - alpha)) with alpha = af + (1 - af) (1 - trust), trust = (score - det_thresh) /
// (1 - det_thresh) in f64 (alpha = af without dynamic appearance).  One wave per track, in place.
__device__ inline void deepoc_features(const SSDeepOcDev& x, size_t sb, size_t fs, int nT, int nB, OcLds& m)
{
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    for (int i = w; i < nB; i += 4) {
        const int slot = m.born[i];
        const float* cu = x.ufeat + (fs * SS_MAXD + m.det[slot]) * SS_F;
        float* em = x.emb + (sb + slot) * SS_F;
#pragma unroll
        for (int j = 0; j < 8; ++j) em[l + 64 * j] = cu[l + 64 * j];
    }
    for (int p = w; p < nT; p += 4) {
        const int d = m.mdet[p];
        if (d < 0) continue;                                       // the same for the whole wave
        double al = x.alpha_fixed;
        if (x.dynamic) {
            const double trust = ((double)m.dsc[d] - x.det_thresh) / (1.0 - x.det_thresh);
            al = x.alpha_fixed + (1.0 - x.alpha_fixed) * (1.0 - trust);
        }
        float* em = x.emb + (sb + m.trk[p]) * SS_F;
        const float* cu = x.ufeat + (fs * SS_MAXD + d) * SS_F;
        float sv[8], cv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { sv[j] = em[l + 64 * j]; cv[j] = cu[l + 64 * j]; }
        ss_ema_regs(sv, cv, (float)al, (float)(1.0 - al), em);
    }
}

// the unit feature of every high-score row of the group (ss_unit8: so_normalize order; only these rows' features are read, DO-05).
// Block = 4 rows (one wave each) of one (frame, stream).
__global__ __launch_bounds__(256) void k_deepoc_feats(SSDeepOcDev x, const float* __restrict__ dets, const float* __restrict__ feats,
                                                      const int* __restrict__ ndets)
{
    const int s = blockIdx.y, f = blockIdx.z, r = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    const size_t fs = (size_t)f * x.oc.S + s;
    const int N = min(max(ndets[fs], 0), x.oc.max_dets);
    if (r >= N) return;                                           // whole waves
    if (!(dets[(fs * SS_MAXD + r) * 6 + 4] > x.oc.det_thresh)) return;
    const float* in = feats + (fs * SS_MAXD + r) * SS_F;
    float* out = x.ufeat + (fs * SS_MAXD + r) * SS_F;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = in[l + 64 * j];
    ss_unit8(v, out);
}

__global__ __launch_bounds__(256) void k_deepoc_group(SSDeepOcDev x, int F, const float* __restrict__ dets, const int* __restrict__ ndets,
                                                      float* __restrict__ out, int* __restrict__ nout)
{
    __shared__ OcLds m;
    __shared__ DeepLds dl;
    oc_group<true>(x.oc, &x, &dl, F, dets, ndets, out, nout, m);
}

void ss_launch_deepoc_group(const SSDeepOcDev& x, int F, const float* dets, const int* ndets, const float* feats, float* out, int* nout,
                            hipStream_t st)
{
    if (x.appearance) hipLaunchKernelGGL(k_deepoc_feats, dim3(SS_MAXD / 4, x.oc.S, F), dim3(256), 0, st, x, dets, feats, ndets);
    hipLaunchKernelGGL(k_deepoc_group, dim3(x.oc.S), dim3(256), 0, st, x, F, dets, ndets, out, nout);
}

// ---- host side: the state of a context; dev.oc's tables, reset and read-back are ss_ocsort.hip's (ss_oc_*) ---------------------------
struct SSDeepOc {
    SSDeepOcDev dev;
    SsBuf<SS_DEVICE> base, feat;        // dev.oc's tables; emb, ufeat and E
};

void ss_deepoc_free(SSDeepOc* d) { delete d; }
const SSDeepOcDev& ss_deepoc_dev(const SSDeepOc* d) { return d->dev; }
void ss_deepoc_set_gmc_impl(SSDeepOc* d, const double* d_warps) { d->dev.gmc = d_warps; }
int ss_deepoc_pending_impl(SSDeepOc* d, hipStream_t st, std::string& err) { return d ? ss_tracker_pending_impl(d->dev.oc.err, d->dev.oc.S, st, "Deep OC-SORT tracker", err) : (int)SS_OK; }

int ss_deepoc_create_check_impl(const ss_deepoc_config* cfg, std::string& err)
{
    if (!cfg) { err = "ss_deepoc_create: null argument"; return SS_ERR_INVALID; }
    auto flag = [](int v) { return v == 0 || v == 1; };
    if (cfg->max_tracks < 1 || cfg->max_tracks > SS_MAXT || cfg->max_dets < 1 || cfg->max_dets > SS_MAXD || cfg->delta_t < 1 ||
        cfg->delta_t > SS_OC_MAXDT || cfg->max_age < 1 || cfg->min_hits < 0 || !(cfg->iou_threshold > 0.0 && cfg->iou_threshold <= 1.0) ||
        !(cfg->inertia >= 0.0) || !(cfg->det_thresh < 1.0) || !(cfg->w_association_emb >= 0.0) ||
        !(cfg->alpha_fixed_emb >= 0.0 && cfg->alpha_fixed_emb <= 1.0) || !(cfg->aw_param >= 0.0 && cfg->aw_param < 1.0) ||
        !flag(cfg->appearance) || !flag(cfg->dynamic_appearance) || !flag(cfg->adaptive_weighting)) {
        err = "ss_deepoc_create: 1 <= max_tracks <= 256, 1 <= max_dets <= 128, 1 <= delta_t <= 8, max_age >= 1, "
              "min_hits >= 0, 0 < iou_threshold <= 1, inertia >= 0, det_thresh < 1, w_association_emb >= 0, "
              "0 <= alpha_fixed_emb <= 1, 0 <= aw_param < 1, flags 0 / 1";
        return SS_ERR_INVALID;
    }
    return SS_OK;
}

// the streams restart: their warp flags and track features, then what an OC-SORT state resets; synchronises
static int deepoc_reset(const SSDeepOcDev& d, hipStream_t st, SsWarpFlags wf, int stream, const char* who, std::string& err)
{
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? d.oc.S : stream + 1;
    SS_HIPCHK(who, hipMemsetAsync(wf.cmc + s0, 0, (s1 - s0) * 4, st));
    SS_HIPCHK(who, hipMemsetAsync(wf.gmc + s0, 0, (s1 - s0) * 4, st));
    SS_HIPCHK(who, hipMemsetAsync(d.emb + (size_t)s0 * SS_MAXT * SS_F, 0, (size_t)(s1 - s0) * SS_MAXT * SS_F * 4, st));
    return ss_oc_reset_impl(d.oc, st, stream, who, err);
}

int ss_deepoc_reset_impl(SSDeepOc* d, hipStream_t st, SsWarpFlags wf, int stream, std::string& err) { return deepoc_reset(d->dev, st, wf, stream, "ss_deepoc_reset: ", err); }

// the caller has drained the stream and freed the state this one replaces: a failure leaves none attached
int ss_deepoc_create_impl(SSDeepOc** pd, hipStream_t st, SsWarpFlags wf, int S, const ss_deepoc_config* cfg, std::string& err)
{
    const char* who = "ss_deepoc_create: ";
    std::unique_ptr<SSDeepOc> D(new SSDeepOc());
    SSDeepOcDev& d = D->dev;
    memset(&d, 0, sizeof d);
    SSOcDev& o = d.oc;
    o.S = S;
    o.max_age = cfg->max_age; o.min_hits = cfg->min_hits; o.delta_t = cfg->delta_t; o.use_byte = 0;
    o.max_tracks = cfg->max_tracks; o.max_dets = cfg->max_dets;
    o.det_thresh = (float)cfg->det_thresh; o.low_thresh = (float)cfg->det_thresh;
    o.iou_thr = cfg->iou_threshold; o.inertia = cfg->inertia;
    d.appearance = cfg->appearance; d.dynamic = cfg->dynamic_appearance; d.adaptive = cfg->adaptive_weighting;
    d.det_thresh = cfg->det_thresh; d.w_emb = cfg->w_association_emb; d.alpha_fixed = cfg->alpha_fixed_emb; d.aw = cfg->aw_param;
    SsCarve c;
    c.add(&d.emb, (size_t)S * SS_MAXT * SS_F); c.add(&d.ufeat, (size_t)SS_FMAX * S * SS_MAXD * SS_F); c.add(&d.E, (size_t)S * SS_MAXT * SS_MAXD);
    if (const int rc = ss_oc_carve_impl(o, D->base, st, who, err)) return rc;
    SS_HIPCHK(who, c.carve(D->feat, st));
    if (const int rc = deepoc_reset(d, st, wf, -1, who, err)) return rc;
    *pd = D.release();
    return SS_OK;
}

// Synchronous: the tracks' unit features [n][512] of one stream in ss_deepoc_get_tracks' list order
int ss_deepoc_get_features_impl(SSDeepOc* d, hipStream_t st, int s, int cap, float* emb, std::string& err)
{
    const auto none = nullptr;
    std::vector<int> slots;
    if (const int rc = ss_oc_get_tracks_impl(d->dev.oc, st, "ss_deepoc_get_features", s, cap, none, none, none, none, none, none, none, none, none, none,
                                             none, none, none, &slots, err)) return rc;
    SS_HIPCHK("ss_deepoc_get_features: ", ss_gather_device(slots.data(), (int)slots.size(), d->dev.emb + (size_t)s * SS_MAXT * SS_F, SS_MAXT, SS_F, emb));
    return SS_OK;
}
