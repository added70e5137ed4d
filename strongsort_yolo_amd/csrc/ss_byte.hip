// ss_byte.hip — the BYTE tracker family on the device (docs/BYTETRACK.md): ByteTrack (xyah Kalman) and BoT-SORT (xywh Kalman,
// optional GMC, optional ReID), S independent streams, a GROUP of F <= SS_FMAX frames per call.
//
//   k_byte_feats  (ReID only, before k_byte_group in the same call) one wave per detection row of the group: so_normalize of
//                 the raw 512-float feature into b.ufeat.
//   k_byte_kpts   (pose only, before k_byte_group in the same call) one half wave per detection row of the group: the row's
//                 keypoints in original pixels and their visibility word into b.kp / b.kvis.
//   k_byte_group  one workgroup (256 threads) per stream walks the group's frames in order inside the launch: score split,
//                 Kalman predict of the pool, BoT-SORT's GMC (§1b, the GMC variant only: the warps of ss_cmc_estimate
//                 applied to the predicted pool and the unconfirmed tracks), three IoU associations (fused high / plain low / unconfirmed) each solved by
//                 the one-wave LSAP (SciPy's optimum of the raw matrix, then the threshold), births, lost-track expiry, the
//                 list rebuild with duplicate removal, output rows.  One launch per call, no host round trip: capturable.
//                 The REID variant (§1c) adds the appearance entries of stages 4 and 6 and the tracks' smoothed features.
//                 The POSE variant (§1e) adds the OKS entries of stages 4 and 6 and the tracks' stored poses.
//
// The list logic lives in LDS (slot fields, list orders); means / covariances stay in global memory, one thread per track
// for the f64 Kalman work.  tests/bytetrack_ref.py restates every step in the same order (rows are compared bit for bit).
#include "ss_common.h"
#include "ss_launch.h"
#include "ss_lsap.h"
#include "ss_expneg.h"
#include "ss_probiou.h"

#define SS_BYTE_COST_CAP 2048          // LDS-resident cost entries (f64); a larger matrix lives in the stream's global spill area

struct ByteLds {
    // slot fields (copies of the global table for the duration of the launch)
    int state[SS_MAXT], act[SS_MAXT], id[SS_MAXT], start[SS_MAXT], end[SS_MAXT], len[SS_MAXT], det[SS_MAXT];
    float score[SS_MAXT], cls[SS_MAXT];
    int trk[SS_MAXT], lost[SS_MAXT];   // the lists, in order
    int upd[SS_MAXT];                  // per slot: detection to apply this frame (Kalman update) or -1
    double tl[SS_MAXT][4];             // per slot: tlwh of the current mean (predicted / updated / initiated this frame); OBB: cx, cy, w, h
    // the frame's detections
    double dtl[SS_MAXD][4], dz[SS_MAXD][4];
    float dsc[SS_MAXD], dcls[SS_MAXD];
    int hi[SS_MAXD], lo[SS_MAXD], left[SS_MAXD], hused[SS_MAXD], lused[SS_MAXD];
    // work lists (pool / unconfirmed / second-stage rows by index)
    int pool[SS_MAXT], unc[SS_MAXT], r2[SS_MAXT], asg[SS_MAXT], col4row[SS_MAXT], freel[SS_MAXT], born[SS_MAXT], flag[SS_MAXT];
    int dupa[SS_MAXT], dupb[SS_MAXT];
    double cost[SS_BYTE_COST_CAP];
    int wtot[4];
    int n_trk, n_lost, frame, next_id;
};

// the current mean's box as tlwh (ss_track's track box for xyah; centre / size for xywh)
__device__ inline void byte_tlwh(const double* m, bool xywh, double* t)
{
    if (xywh) { t[0] = m[0] - m[2] / 2; t[1] = m[1] - m[3] / 2; t[2] = m[2]; t[3] = m[3]; }
    else { const double w = m[2] * m[3]; t[0] = m[0] - w / 2; t[1] = m[1] - m[3] / 2; t[2] = w; t[3] = m[3]; }
}

// The slot's box from its current mean.  OBB (docs/OBB.md §4): centre and size, the rotated box's own frame, and the ProbIoU terms of
// the box rounded to float32 (the floats d_out_rbox shows) with the slot's angle th into b.tbox[g]; the terms live in global memory,
// so the plain variants' LDS is what it was.
template <bool XYWH, bool OBB>
__device__ inline void byte_box(const SSByteDev& b, size_t g, const double* m, float th, double* t)
{
    if constexpr (OBB) {
        t[0] = m[0]; t[1] = m[1]; t[2] = XYWH ? m[2] : m[2] * m[3]; t[3] = m[3];
        *reinterpret_cast<ss_pbox*>(b.tbox + g * 6) = ss_probiou_box((float)t[0], (float)t[1], (float)t[2], (float)t[3], th);
    }
    else byte_tlwh(m, XYWH, t);
}

// step 3b (docs/BYTETRACK.md §1b, G-02): Ultralytics' STrack.multi_gmc with warp w (R = [[w0, w1], [w3, w4]], t = (w2, w5)):
// mean <- R8 mean + (t, 0, ...), cov <- R8 cov R8^T, R8 = kron(I4, R) as 2x2 blocks.  Every entry is two products and one add
// (the library is built with -ffp-contract=off); tests/botsort_gmc_ref.py restates this order.
__device__ inline void byte_gmc(double* mean, double* cov, const double* w)
{
    const double r00 = w[0], r01 = w[1], r10 = w[3], r11 = w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double u = mean[2 * k], v = mean[2 * k + 1];
        mean[2 * k] = r00 * u + r01 * v;
        mean[2 * k + 1] = r10 * u + r11 * v;
    }
    mean[0] += w[2];
    mean[1] += w[5];
#pragma unroll
    for (int i = 0; i < 4; ++i)                  // X = R8 P: block rows
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const double a = cov[(2 * i) * 8 + c], e = cov[(2 * i + 1) * 8 + c];
            cov[(2 * i) * 8 + c] = r00 * a + r01 * e;
            cov[(2 * i + 1) * 8 + c] = r10 * a + r11 * e;
        }
#pragma unroll
    for (int r = 0; r < 8; ++r)                  // P' = X R8^T: block columns
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double a = cov[r * 8 + 2 * j], e = cov[r * 8 + 2 * j + 1];
            cov[r * 8 + 2 * j] = a * r00 + e * r01;
            cov[r * 8 + 2 * j + 1] = a * r10 + e * r11;
        }
}

// LSAP of an n_rows x n_cols matrix already stored by lsap_cidx -> m.asg[row] = column or -1 (all threads call it).
__device__ inline void byte_assign(int n_rows, int n_cols, const double* cost, bool glb, ByteLds& m, int* err)
{
    const int tid = threadIdx.x;
    m.asg[tid] = -1;
    if (glb) __threadfence();                     // the spilled matrix is read back by wave 0
    __syncthreads();
    if (n_rows > 0 && n_cols > 0 && (tid >> 6) == 0) {
        LsapLds L;
        L.col4row = m.col4row;
        if (lsap_wave_assign(n_rows, n_cols, cost, L, m.asg) && tid == 0) *err = SS_ERR_INFEASIBLE;
    }
    __syncthreads();
}

// §1c: the unit feature of every detection row of the group (ss_unit8: so_normalize order).  Block = 4 rows (one wave each) of one
// (frame, stream).
__global__ __launch_bounds__(256) void k_byte_feats(SSByteDev b, const float* __restrict__ feats, const int* __restrict__ ndets)
{
    const int s = blockIdx.y, f = blockIdx.z, r = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    const size_t fs = (size_t)f * b.S + s;
    const int N = min(max(ndets[fs], 0), b.max_dets);
    if (r >= N) return;                                           // whole waves
    const float* in = feats + (fs * SS_MAXD + r) * SS_F;
    float* out = b.ufeat + (fs * SS_MAXD + r) * SS_F;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = in[l + 64 * j];
    ss_unit8(v, out);
}

// First half of a 256-entry chunk of BoT-SORT's get_dists with a second term (§1c ReID, §1e keypoints), each thread one entry e0 + tid
// of rows (track slots rs[r]) x columns (detections cd[k]), stored by lsap_cidx:  iou = 1 - IoU;  c = fused(iou) if fuse.  An entry
// with iou > prox is masked: its second term is 1, so it stores min(c, 1) — c itself for ReID (pose = false: c <= 1, or NaN, which
// np.minimum keeps), the clamped value for the keypoint term.  The others — overlapping boxes, about one per track — are compacted
// into ae / ac (entry, c; one pair of LDS arrays for both terms: they are never instantiated together) for the caller's second
// half.  Returns their number.
__device__ inline int byte_cost_chunk(int e0, int nR, int nC, const int* rs, const int* cd, double* cost, const SSByteDev& b, bool pose,
                                      ByteLds& m, int*& ae, double*& ac)
{
    __shared__ int s_ae[256];
    __shared__ double s_ac[256];
    ae = s_ae; ac = s_ac;
    const int e = e0 + threadIdx.x;
    int need = 0;
    double c = 0.0;
    if (e < nR * nC) {
        const int r = e / nC, k = e - r * nC, d = cd[k];
        const double iou = ss_iou_cost(m.tl[rs[r]], m.dtl[d], 2.0);
        c = b.fuse ? 1.0 - (1.0 - iou) * (double)m.dsc[d] : iou;
        need = !(iou > b.prox);
        if (!need) cost[lsap_cidx(r, k, nR, nC)] = pose && 1.0 < c ? 1.0 : c;
    }
    int pos, nA;
    block_scan256(need, m.wtot, pos, nA);
    if (need) { s_ae[pos] = e; s_ac[pos] = c; }
    __syncthreads();
    return nA;
}

// §1c get_dists with ReID on rows (track slots rs[r]) x columns (detections cd[k]) of frame fs, stored by lsap_cidx:
//   iou = 1 - IoU;  c = fused(iou) if fuse;  e = 1 if iou > prox, else max(0, 1 - so_dot(smooth, curr)) / 2 -> 1 if > appear;
//   cost = min(c, e).
// Only the unmasked pairs get a dot product.  The entries go by chunks of 256 (byte_cost_chunk), then eight lanes per pair run
// so_dot's eight 64-long fmaf chains (lane = segment) and lane 0 of the eight adds
// them in segment order.  A dense MFMA matrix (k_cosine_kat's form) would compute the whole rows x columns product for the
// few unmasked pairs (docs/BYTETRACK.md §3).
__device__ inline void byte_reid_cost(int nR, int nC, const int* rs, const int* cd, double* cost, const SSByteDev& b,
                                            size_t sb, size_t fs, ByteLds& m)
{
    const int tid = threadIdx.x, seg = tid & 7, base = (tid & 63) & ~7, n = nR * nC;
    int* ae;
    double* ac;
    for (int e0 = 0; e0 < n; e0 += 256) {
        const int nA = byte_cost_chunk(e0, nR, nC, rs, cd, cost, b, false, m, ae, ac);
        for (int j0 = 0; j0 < nA; j0 += 32) {
            const int j = j0 + (tid >> 3);
            int r = 0, k = 0;
            float p = 0.0f;
            if (j < nA) {
                r = ae[j] / nC; k = ae[j] - r * nC;
                const float4* g = reinterpret_cast<const float4*>(b.smooth + (sb + rs[r]) * SS_F + SS_SEG * seg);
                const float4* q = reinterpret_cast<const float4*>(b.ufeat + (fs * SS_MAXD + cd[k]) * SS_F + SS_SEG * seg);
#pragma unroll 8
                for (int i = 0; i < SS_SEG / 4; ++i) {
                    const float4 x = g[i], y = q[i];
                    p = fmaf(x.x, y.x, p); p = fmaf(x.y, y.y, p); p = fmaf(x.z, y.z, p); p = fmaf(x.w, y.w, p);
                }
            }
            float tot = __shfl(p, base);
#pragma unroll
            for (int i = 1; i < SS_NSEG; ++i) tot = tot + __shfl(p, base + i);
            if (j < nA && seg == 0) {
                double a = (double)fmaxf(0.0f, 1.0f - tot) / 2.0;
                if (a > b.appear) a = 1.0;
                const double cf = ac[j];
                cost[lsap_cidx(r, k, nR, nC)] = a < cf ? a : cf;
            }
        }
        __syncthreads();                                           // ae / ac: the next chunk's
    }
}

// the smoothed features after the frame's Kalman updates (§1c): a birth copies its unit feature; a match of stages 4-6 takes
// so_ema(smooth, curr, alpha, 1 - alpha) — the EMA, then so_normalize's order.  One wave per slot, in place (a lane reads and
// writes the same elements); the updated slots are compacted into m.freel (free after the births) and every wave takes two
// at a time, so that both slots' loads are in flight together.
__device__ inline void byte_reid_smooth(const SSByteDev& b, size_t sb, size_t fs, int nB, ByteLds& m)
{
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    for (int i = w; i < nB; i += 4) {
        const int slot = m.born[i];
        const float* cu = b.ufeat + (fs * SS_MAXD + m.det[slot]) * SS_F;
        float* sm = b.smooth + (sb + slot) * SS_F;
#pragma unroll
        for (int j = 0; j < 8; ++j) sm[l + 64 * j] = cu[l + 64 * j];
    }
    int pos, nU;
    block_scan256(m.upd[tid] >= 0, m.wtot, pos, nU);
    if (m.upd[tid] >= 0) m.freel[pos] = tid;
    __syncthreads();
    for (int i = 2 * w; i < nU; i += 8) {
        const int two = i + 1 < nU;
        float* sm[2];
        float sv[2][8], cv[2][8];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int slot = m.freel[two ? i + u : i];
            sm[u] = b.smooth + (sb + slot) * SS_F;
            const float* cu = b.ufeat + (fs * SS_MAXD + m.upd[slot]) * SS_F;
#pragma unroll
            for (int j = 0; j < 8; ++j) { sv[u][j] = sm[u][l + 64 * j]; cv[u][j] = cu[l + 64 * j]; }
        }
        ss_ema_regs(sv[0], cv[0], b.alpha, b.one_minus_alpha, sm[0]);
        if (two) ss_ema_regs(sv[1], cv[1], b.alpha, b.one_minus_alpha, sm[1]);
    }
}

// §1e: the keypoints of every detection row of the group.  kpts: row (fs, r) at kpts + (fs * MAXD + r) * stride + off, nk triplets
// (x, y, v); geom [F * S][5] = {gain, pad_x, pad_y, ..} (ss_nms_batch's rows): x, y are network-input pixels and become
// (x - pad) / gain in float32, the floats Results.keypoints shows; NULL: they are original pixels already.  Half a wave per
// row, lane = keypoint; the visibility word is the half's ballot.  Block = 8 rows of one (frame, stream).
__global__ __launch_bounds__(256) void k_byte_kpts(SSByteDev b, const float* __restrict__ kpts, long long stride, int off,
                                                   const float* __restrict__ geom, const int* __restrict__ ndets)
{
    const int s = blockIdx.y, f = blockIdx.z, r = blockIdx.x * 8 + (threadIdx.x >> 5), k = threadIdx.x & 31;
    const size_t fs = (size_t)f * b.S + s;
    const int N = min(max(ndets[fs], 0), b.max_dets);
    const bool on = r < N && k < b.nk;
    int v = 0;
    if (on) {
        const float* in = kpts + (fs * SS_MAXD + r) * stride + off + 3 * k;
        float x = in[0], y = in[1];
        if (geom) { const float* g = geom + fs * 5; x = (x - g[1]) / g[0]; y = (y - g[2]) / g[0]; }
        v = in[2] >= b.vis;
        float* o = b.kp + ((fs * SS_MAXD + r) * b.nk + k) * 2;
        o[0] = x; o[1] = y;
    }
    const unsigned long long w = __ballot(v);
    if (on && k == 0) b.kvis[fs * SS_MAXD + r] = (unsigned)(w >> (threadIdx.x & 32));
}

// §1e get_dists with the keypoint term on rows (track slots rs[r]) x columns (detections cd[k]) of frame fs, stored by lsap_cidx:
//   iou = 1 - IoU;  c = fused(iou) if fuse;  e = 1 if iou > prox, else the pair's OKS entry;  cost = min(c, e).
// byte_reid_cost's chunked shape (byte_cost_chunk); then half a wave per surviving pair, lane = keypoint: the track's stored offset
// on its predicted mean (b.mean, moved
// by GMC already) against the row's keypoint, t_k = ss_expneg(d2 / (2 area (2 sigma_k)^2)).  Every lane of the half then adds
// the common keypoints' terms in keypoint order (shuffles within the half) and lane 0 stores.
__device__ inline void byte_pose_cost(int nR, int nC, const int* rs, const int* cd, double* cost, const SSByteDev& b,
                                      size_t sb, size_t fs, ByteLds& m)
{
    const int tid = threadIdx.x, kk = tid & 31, base = tid & 32, n = nR * nC, K = b.nk;
    int* pe;
    double* pc;
    for (int e0 = 0; e0 < n; e0 += 256) {
        const int nA = byte_cost_chunk(e0, nR, nC, rs, cd, cost, b, true, m, pe, pc);
        for (int j0 = 0; j0 < nA; j0 += 8) {
            const int j = j0 + (tid >> 5);
            const bool act = j < nA;
            int r = 0, k = 0;
            unsigned common = 0;
            double t = 0.0, area = 0.0;
            if (act) {
                r = pe[j] / nC; k = pe[j] - r * nC;
                const int slot = rs[r], d = cd[k];
                common = b.tvis[sb + slot] & b.kvis[fs * SS_MAXD + d];
                area = m.dtl[d][2] * m.dtl[d][3];
                if (kk < K && ((common >> kk) & 1u)) {
                    const double* mn = b.mean + (sb + slot) * 8;
                    const double* po = b.tpose + ((sb + slot) * K + kk) * 2;
                    const float* kp = b.kp + ((fs * SS_MAXD + d) * K + kk) * 2;
                    const double px = mn[0] + po[0] * mn[2], py = mn[1] + po[1] * mn[3];
                    const double dx = px - (double)kp[0], dy = py - (double)kp[1];
                    const double d2 = dx * dx + dy * dy, s2 = b.ks2[kk];
                    t = ss_expneg(d2 / (2.0 * area * s2 * s2));
                }
            }
            double acc = 0.0;
            for (int i = 0; i < K; ++i) {                              // every lane of the wave takes part in the shuffles
                const double ti = __shfl(t, base + i);
                if ((common >> i) & 1u) acc = acc + ti;
            }
            if (act && kk == 0) {
                const int nc = __popc(common);
                double a = 1.0;
                if (nc >= b.min_common && area > 0.0) {
                    a = (1.0 - acc / (double)nc) / 2.0;
                    if (a > b.pose_thresh) a = 1.0;
                }
                const double cf = pc[j];
                cost[lsap_cidx(r, k, nR, nC)] = a < cf ? a : cf;
            }
        }
        __syncthreads();                                           // pe / pc: the next chunk's
    }
}

// the stored poses after the frame's Kalman updates (§1e, K-03: the last observation, no smoothing): the slots updated in stages
// 4-6 compacted into m.freel (free after the births), the births behind them; m.det[slot] is the row either way.  Half a wave
// per slot, lane = keypoint: offsets from the row's box centre in widths / heights (m.dz, the measurement), all invisible when
// the box has no extent.
__device__ inline void byte_pose_store(const SSByteDev& b, size_t sb, size_t fs, int nB, ByteLds& m)
{
    const int tid = threadIdx.x, kk = tid & 31, K = b.nk;
    int pos, nU;
    block_scan256(m.upd[tid] >= 0, m.wtot, pos, nU);
    if (m.upd[tid] >= 0) m.freel[pos] = tid;
    if (tid < nB) m.freel[nU + tid] = m.born[tid];
    __syncthreads();
    for (int i0 = 0; i0 < nU + nB; i0 += 8) {
        const int i = i0 + (tid >> 5);
        if (i >= nU + nB) continue;
        const int slot = m.freel[i], d = m.det[slot];
        const double* z = m.dz[d];
        const bool box = z[2] > 0.0 && z[3] > 0.0;
        if (kk < K) {
            const float* kp = b.kp + ((fs * SS_MAXD + d) * K + kk) * 2;
            double* po = b.tpose + ((sb + slot) * K + kk) * 2;
            po[0] = box ? ((double)kp[0] - z[0]) / z[2] : 0.0;
            po[1] = box ? ((double)kp[1] - z[1]) / z[3] : 0.0;
        }
        if (kk == 0) b.tvis[sb + slot] = box ? b.kvis[fs * SS_MAXD + d] : 0u;
    }
    __syncthreads();
}

// GMC: BoT-SORT's camera-motion step 3b from b.gmc; REID: §1c's appearance term and smoothed features from b.smooth / b.ufeat
// POSE: §1e's keypoint term and stored poses from b.tpose / b.kp (all three only instantiated with XYWH, REID and POSE never
// together; without them the code is the plain tracker's).  OBB (docs/OBB.md §4, never with the other three): 11-column rows, the
// cost of every association and of the duplicate test is 1 - ProbIoU of the rotated boxes, the slot carries its last row's angle
// (R-06), rows carry the rotated box's envelope and b.rbox its xywh theta.
template <bool XYWH, bool GMC, bool REID, bool POSE, bool OBB = false>
__global__ __launch_bounds__(256) void k_byte_group(SSByteDev b, int F, const float* __restrict__ dets, const int* __restrict__ ndets,
                                                    float* __restrict__ out, int* __restrict__ nout)
{
    __shared__ ByteLds m;
    const int s = blockIdx.x, tid = threadIdx.x, S = b.S;
    const size_t sb = (size_t)s * SS_MAXT;
    double* spill = b.spill + (size_t)s * SS_MAXT * SS_MAXD;
    int* err = b.err + s;
    [[maybe_unused]] const size_t db = (size_t)s * SS_MAXD;
    // 1 - IoU of a slot's box and a row's (OBB: 1 - ProbIoU from the two boxes' terms), and of two slots' boxes
    auto cost_td = [&](int slot, int d) -> double {
        if constexpr (OBB) return 1.0 - ss_probiou_pair(*reinterpret_cast<const ss_pbox*>(b.tbox + (sb + slot) * 6),
                                                        *reinterpret_cast<const ss_pbox*>(b.dbox + (db + d) * 6));
        else return ss_iou_cost(m.tl[slot], m.dtl[d], 2.0);
    };
    auto cost_tt = [&](int a, int c) -> double {
        if constexpr (OBB) return 1.0 - ss_probiou_pair(*reinterpret_cast<const ss_pbox*>(b.tbox + (sb + a) * 6),
                                                        *reinterpret_cast<const ss_pbox*>(b.tbox + (sb + c) * 6));
        else return ss_iou_cost(m.tl[a], m.tl[c], 2.0);
    };
    // ---- the stream's table into LDS ----
    m.state[tid] = b.state[sb + tid]; m.act[tid] = b.act[sb + tid]; m.id[tid] = b.tid[sb + tid]; m.start[tid] = b.start[sb + tid];
    m.end[tid] = b.end[sb + tid]; m.len[tid] = b.len[sb + tid]; m.det[tid] = b.det[sb + tid]; m.score[tid] = b.score[sb + tid];
    m.cls[tid] = b.cls[sb + tid]; m.trk[tid] = b.trk[sb + tid]; m.lost[tid] = b.lost[sb + tid];
    if (tid == 0) { m.n_trk = b.n_trk[s]; m.n_lost = b.n_lost[s]; m.frame = b.frame[s]; m.next_id = b.next_id[s]; }
    __syncthreads();

    for (int f = 0; f < F; ++f) {
        const size_t fs = (size_t)f * S + s;
        const int nraw = ndets[fs];
        const int N = min(max(nraw, 0), b.max_dets);
        const int nT = m.n_trk, nL = m.n_lost, n_live = nT + nL;
        const int fid = m.frame + 1;
        if (tid == 0 && (nraw < 0 || nraw > b.max_dets)) *err = SS_ERR_CAPACITY;
        // ---- 1. detections and the score split ----
        int isHi = 0, isLo = 0;
        if (tid < N) {
            const float* d = dets + (fs * SS_MAXD + tid) * (OBB ? 11 : 6);
            const float sc = d[4];
            double* t = m.dtl[tid];
            double* z = m.dz[tid];
            if constexpr (OBB) {                                   // the rotated box's own centre and size; the envelope is not read
                t[0] = d[6]; t[1] = d[7]; t[2] = d[8]; t[3] = d[9];
                z[0] = t[0]; z[1] = t[1];
                *reinterpret_cast<ss_pbox*>(b.dbox + (db + tid) * 6) = ss_probiou_box(d[6], d[7], d[8], d[9], d[10]);
            }
            else {
                const double x1 = d[0], y1 = d[1], x2 = d[2], y2 = d[3];
                t[0] = x1; t[1] = y1; t[2] = x2 - x1; t[3] = y2 - y1;
                z[0] = t[0] + t[2] / 2; z[1] = t[1] + t[3] / 2;
            }
            if (XYWH) { z[2] = t[2]; z[3] = t[3]; } else { z[2] = t[2] / t[3]; z[3] = t[3]; }
            m.dsc[tid] = sc; m.dcls[tid] = d[5];
            isHi = sc >= b.high;
            isLo = sc > b.low && sc < b.high;
        }
        if (tid < SS_MAXD) { m.hused[tid] = 0; m.lused[tid] = 0; }
        m.upd[tid] = -1; m.flag[tid] = 0; m.dupa[tid] = 0; m.dupb[tid] = 0;
        int pos, nHi, nLo;
        block_scan256(isHi, m.wtot, pos, nHi);
        if (isHi) m.hi[pos] = tid;
        block_scan256(isLo, m.wtot, pos, nLo);
        if (isLo) m.lo[pos] = tid;
        // ---- 2. unconfirmed tracks and the pool (activated tracked, then lost) ----
        const int tslot = tid < nT ? m.trk[tid] : -1;
        const int isU = tid < nT && !m.act[tslot], isP = tid < nT && m.act[tslot];
        int nU, nPT;
        block_scan256(isU, m.wtot, pos, nU);
        if (isU) m.unc[pos] = tslot;
        block_scan256(isP, m.wtot, pos, nPT);
        if (isP) m.pool[pos] = tslot;
        if (tid < nL) m.pool[nPT + tid] = m.lost[tid];
        const int nP = nPT + nL;
        __syncthreads();
        // ---- 3. predict the pool (thread = pool index); the unconfirmed tracks keep their mean ----
        // ---- 3b. GMC (w6 >= 0: a warp, G-03): the predicted pool in registers, then the unconfirmed tracks ----
        const double* gw = GMC ? b.gmc + fs * 8 : nullptr;
        const bool warp = GMC && gw[6] >= 0.0;
        if (tid < nP) {
            const int slot = m.pool[tid];
            double mean[8], cov[64];
            const size_t g = sb + slot;
#pragma unroll
            for (int i = 0; i < 8; ++i) mean[i] = b.mean[g * 8 + i];
#pragma unroll
            for (int i = 0; i < 64; ++i) cov[i] = b.cov[g * 64 + i];
            if (m.state[slot] != SS_BYTE_TRACKED) { mean[7] = 0.0; if (XYWH) mean[6] = 0.0; }
            ss_kf_predict<XYWH>(mean, cov, b.wp, b.wv);
            if (warp) byte_gmc(mean, cov, gw);
#pragma unroll
            for (int i = 0; i < 8; ++i) b.mean[g * 8 + i] = mean[i];
#pragma unroll
            for (int i = 0; i < 64; ++i) b.cov[g * 64 + i] = cov[i];
            byte_box<XYWH, OBB>(b, g, mean, OBB ? b.angle[g] : 0.0f, m.tl[slot]);
        }
        if (tid < nU) {
            const int slot = m.unc[tid];
            const size_t g = sb + slot;
            double mean[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) mean[i] = b.mean[g * 8 + i];
            if (warp) {
                double cov[64];
#pragma unroll
                for (int i = 0; i < 64; ++i) cov[i] = b.cov[g * 64 + i];
                byte_gmc(mean, cov, gw);
#pragma unroll
                for (int i = 0; i < 8; ++i) b.mean[g * 8 + i] = mean[i];
#pragma unroll
                for (int i = 0; i < 64; ++i) b.cov[g * 64 + i] = cov[i];
            }
            byte_box<XYWH, OBB>(b, g, mean, OBB ? b.angle[g] : 0.0f, m.tl[slot]);
        }
        __syncthreads();
        // ---- 4. first association: pool x high rows, fused 1 - IoU, match_thresh ----
        {
            const bool glb = nP * nHi > SS_BYTE_COST_CAP;
            double* cost = glb ? spill : m.cost;
            if constexpr (REID) byte_reid_cost(nP, nHi, m.pool, m.hi, cost, b, sb, fs, m);
            else if constexpr (POSE) byte_pose_cost(nP, nHi, m.pool, m.hi, cost, b, sb, fs, m);
            else
            for (int e = tid; e < nP * nHi; e += 256) {
                const int r = e / nHi, k = e - r * nHi, d = m.hi[k];
                double c = cost_td(m.pool[r], d);
                if (b.fuse) c = 1.0 - (1.0 - c) * (double)m.dsc[d];
                cost[lsap_cidx(r, k, nP, nHi)] = c;
            }
            byte_assign(nP, nHi, cost, glb, m, err);
            if (tid < nP) {
                const int k = m.asg[tid];
                if (k >= 0 && cost[lsap_cidx(tid, k, nP, nHi)] <= b.match) {
                    const int slot = m.pool[tid], d = m.hi[k];
                    m.hused[k] = 1;
                    m.upd[slot] = d;
                    if (m.state[slot] == SS_BYTE_TRACKED) m.len[slot] += 1;
                    else { m.len[slot] = 0; m.flag[tid] = 1; }            // re-found (pool index tid)
                }
            }
        }
        __syncthreads();
        // ---- 5. second association: unmatched Tracked pool tracks x low rows, plain 1 - IoU, 0.5 ----
        int nR2;
        {
            const int isR = tid < nP && m.upd[m.pool[tid]] < 0 && m.state[m.pool[tid]] == SS_BYTE_TRACKED;
            block_scan256(isR, m.wtot, pos, nR2);
            if (isR) m.r2[pos] = m.pool[tid];
            __syncthreads();
            const bool glb = nR2 * nLo > SS_BYTE_COST_CAP;
            double* cost = glb ? spill : m.cost;
            for (int e = tid; e < nR2 * nLo; e += 256) {
                const int r = e / nLo, k = e - r * nLo;
                cost[lsap_cidx(r, k, nR2, nLo)] = cost_td(m.r2[r], m.lo[k]);
            }
            byte_assign(nR2, nLo, cost, glb, m, err);
            if (tid < nR2) {
                const int k = m.asg[tid], slot = m.r2[tid];
                if (k >= 0 && cost[lsap_cidx(tid, k, nR2, nLo)] <= 0.5) { m.upd[slot] = m.lo[k]; m.len[slot] += 1; }
                else m.state[slot] = SS_BYTE_LOST;                       // new lost (r2 index tid)
            }
        }
        __syncthreads();
        // ---- 6. unconfirmed x the high rows left over, fused, 0.7 ----
        int nLeft;
        {
            const int isL = tid < nHi && !m.hused[tid];
            block_scan256(isL, m.wtot, pos, nLeft);
            if (isL) m.left[pos] = m.hi[tid];
            __syncthreads();
            const bool glb = nU * nLeft > SS_BYTE_COST_CAP;
            double* cost = glb ? spill : m.cost;
            if constexpr (REID) byte_reid_cost(nU, nLeft, m.unc, m.left, cost, b, sb, fs, m);
            else if constexpr (POSE) byte_pose_cost(nU, nLeft, m.unc, m.left, cost, b, sb, fs, m);
            else
            for (int e = tid; e < nU * nLeft; e += 256) {
                const int r = e / nLeft, k = e - r * nLeft, d = m.left[k];
                double c = cost_td(m.unc[r], d);
                if (b.fuse) c = 1.0 - (1.0 - c) * (double)m.dsc[d];
                cost[lsap_cidx(r, k, nU, nLeft)] = c;
            }
            byte_assign(nU, nLeft, cost, glb, m, err);
            if (tid < nU) {
                const int k = m.asg[tid], slot = m.unc[tid];
                if (k >= 0 && cost[lsap_cidx(tid, k, nU, nLeft)] <= 0.7) { m.upd[slot] = m.left[k]; m.len[slot] += 1; m.lused[k] = 1; }
                else m.state[slot] = SS_BYTE_REMOVED;
            }
        }
        __syncthreads();
        // ---- 7. births: high rows still unmatched, ascending, score >= new_track_thresh, into the free slots ascending ----
        int nB;
        {
            const int isB = tid < nLeft && !m.lused[tid] && m.dsc[m.left[tid]] >= b.new_thresh;
            int rank, nCand, fpos, nFree;
            // a slot is free when no list holds it (the lists at the frame's start)
            m.asg[tid] = 0;
            __syncthreads();
            if (tid < nT) m.asg[m.trk[tid]] = 1;
            if (tid < nL) m.asg[m.lost[tid]] = 1;
            __syncthreads();
            const int isF = !m.asg[tid];
            block_scan256(isF, m.wtot, fpos, nFree);
            if (isF) m.freel[fpos] = tid;
            block_scan256(isB, m.wtot, rank, nCand);
            const int allowed = max(0, b.max_tracks - n_live);
            nB = min(nCand, allowed);
            if (tid == 0 && nCand > allowed) *err = SS_ERR_CAPACITY;
            __syncthreads();
            if (isB && rank < nB) {
                const int slot = m.freel[rank], d = m.left[tid];
                double mean[8], cov[64];
                ss_kf_initiate<XYWH>(m.dz[d], b.wp, b.wv, mean, cov);
                const size_t g = sb + slot;
#pragma unroll
                for (int i = 0; i < 8; ++i) b.mean[g * 8 + i] = mean[i];
                for (int i = 0; i < 64; ++i) b.cov[g * 64 + i] = cov[i];
                float th = 0.0f;
                if constexpr (OBB) { th = dets[(fs * SS_MAXD + d) * 11 + 10]; b.angle[g] = th; }       // R-06
                byte_box<XYWH, OBB>(b, g, mean, th, m.tl[slot]);
                m.id[slot] = m.next_id + rank;
                m.len[slot] = 0; m.state[slot] = SS_BYTE_TRACKED; m.act[slot] = fid == 1;
                m.start[slot] = fid; m.end[slot] = fid;
                m.score[slot] = m.dsc[d]; m.cls[slot] = m.dcls[d]; m.det[slot] = d;
                m.born[rank] = slot;
            }
        }
        // ---- Kalman updates of this frame's matches (thread = slot): stages 4-6 ----
        {
            const int d = m.upd[tid];
            if (d >= 0) {
                const size_t g = sb + tid;
                double mean[8], cov[64];
#pragma unroll
                for (int i = 0; i < 8; ++i) mean[i] = b.mean[g * 8 + i];
#pragma unroll
                for (int i = 0; i < 64; ++i) cov[i] = b.cov[g * 64 + i];
                ss_kf_update<XYWH>(mean, cov, m.dz[d], 0.0, b.wp);
#pragma unroll
                for (int i = 0; i < 8; ++i) b.mean[g * 8 + i] = mean[i];
#pragma unroll
                for (int i = 0; i < 64; ++i) b.cov[g * 64 + i] = cov[i];
                float th = 0.0f;
                if constexpr (OBB) { th = dets[(fs * SS_MAXD + d) * 11 + 10]; b.angle[g] = th; }       // R-06
                byte_box<XYWH, OBB>(b, g, mean, th, m.tl[tid]);
                m.state[tid] = SS_BYTE_TRACKED; m.act[tid] = 1; m.end[tid] = fid;
                m.score[tid] = m.dsc[d]; m.cls[tid] = m.dcls[d]; m.det[tid] = d;
            }
        }
        __syncthreads();
        if constexpr (REID) byte_reid_smooth(b, sb, fs, nB, m);
        if constexpr (POSE) byte_pose_store(b, sb, fs, nB, m);
        // ---- 8. lost tracks past max_time_lost ----
        if (tid < nL) {
            const int slot = m.lost[tid];
            if (m.state[slot] == SS_BYTE_LOST && fid - m.end[slot] > b.max_time_lost) m.state[slot] = SS_BYTE_REMOVED;
        }
        __syncthreads();
        // ---- 9. the lists: tracked = old tracked still Tracked + births + re-found; lost = old lost still Lost + new lost ----
        int nT2, nL2;
        {
            const int keepT = tid < nT && m.state[m.trk[tid]] == SS_BYTE_TRACKED;
            const int refd = tid < nP && m.flag[tid];
            const int keepL = tid < nL && m.state[m.lost[tid]] == SS_BYTE_LOST;
            const int isNL = tid < nR2 && m.upd[m.r2[tid]] < 0;                // the second stage's unmatched rows (now Lost)
            int p0, p1, p2, t0, t1, t2, p3, t3;
            block_scan256(keepT, m.wtot, p0, t0);
            block_scan256(refd, m.wtot, p1, t1);
            block_scan256(keepL, m.wtot, p2, t2);
            block_scan256(isNL, m.wtot, p3, t3);
            const int vT = keepT ? m.trk[tid] : -1, vR = refd ? m.pool[tid] : -1, vL = keepL ? m.lost[tid] : -1, vN = isNL ? m.r2[tid] : -1;
            __syncthreads();
            if (keepT) m.trk[p0] = vT;
            if (tid < nB) m.trk[t0 + tid] = m.born[tid];
            if (refd) m.trk[t0 + nB + p1] = vR;
            if (keepL) m.lost[p2] = vL;
            if (isNL) m.lost[t2 + p3] = vN;
            nT2 = t0 + nB + t1;
            nL2 = t2 + t3;
        }
        __syncthreads();
        // ---- duplicates between the lists: 1 - IoU < 0.15, the shorter-lived track goes (the tracked one on a tie) ----
        for (int e = tid; e < nT2 * nL2; e += 256) {
            const int p = e / nL2, q = e - p * nL2, a = m.trk[p], c = m.lost[q];
            if (cost_tt(a, c) < 0.15) {
                if (m.end[a] - m.start[a] > m.end[c] - m.start[c]) m.dupb[q] = 1;
                else m.dupa[p] = 1;
            }
        }
        __syncthreads();
        {
            const int kA = tid < nT2 && !m.dupa[tid], kB = tid < nL2 && !m.dupb[tid];
            int pA, pB, tA, tB;
            block_scan256(kA, m.wtot, pA, tA);
            block_scan256(kB, m.wtot, pB, tB);
            const int vA = tid < nT2 ? m.trk[tid] : -1, vB = tid < nL2 ? m.lost[tid] : -1;
            __syncthreads();
            if (tid < nT2 && !kA) m.state[vA] = SS_BYTE_REMOVED;
            if (tid < nL2 && !kB) m.state[vB] = SS_BYTE_REMOVED;
            if (kA) m.trk[pA] = vA;
            if (kB) m.lost[pB] = vB;
            nT2 = tA; nL2 = tB;
        }
        __syncthreads();
        // ---- 10. one row per activated tracked track, in list order ----
        {
            const int slot = tid < nT2 ? m.trk[tid] : 0;
            const int emit = tid < nT2 && m.act[slot];
            int row, nRow;
            block_scan256(emit, m.wtot, row, nRow);
            if (emit) {
                const double* t = m.tl[slot];
                float* o = out + (fs * SS_MAXT + row) * 8;
                if constexpr (OBB) {
                    float* q = b.rbox + (fs * SS_MAXT + row) * 5;
                    const float cx = (float)t[0], cy = (float)t[1], bw = (float)t[2], bh = (float)t[3], th = b.angle[sb + slot];
                    double e[4];
                    ss_rbox_envelope(cx, cy, bw, bh, th, e);
                    o[0] = (float)e[0]; o[1] = (float)e[1]; o[2] = (float)e[2]; o[3] = (float)e[3];
                    q[0] = cx; q[1] = cy; q[2] = bw; q[3] = bh; q[4] = th;
                }
                else { o[0] = (float)t[0]; o[1] = (float)t[1]; o[2] = (float)(t[0] + t[2]); o[3] = (float)(t[1] + t[3]); }
                o[4] = (float)m.id[slot]; o[5] = m.cls[slot]; o[6] = m.score[slot]; o[7] = (float)m.det[slot];
            }
            if (tid == 0) {
                nout[fs] = nRow;
                m.n_trk = nT2; m.n_lost = nL2; m.frame = fid; m.next_id += nB;
            }
        }
        __syncthreads();
    }
    // ---- the table back to global memory ----
    b.state[sb + tid] = m.state[tid]; b.act[sb + tid] = m.act[tid]; b.tid[sb + tid] = m.id[tid]; b.start[sb + tid] = m.start[tid];
    b.end[sb + tid] = m.end[tid]; b.len[sb + tid] = m.len[tid]; b.det[sb + tid] = m.det[tid]; b.score[sb + tid] = m.score[tid];
    b.cls[sb + tid] = m.cls[tid]; b.trk[sb + tid] = m.trk[tid]; b.lost[sb + tid] = m.lost[tid];
    if (tid == 0) { b.n_trk[s] = m.n_trk; b.n_lost[s] = m.n_lost; b.frame[s] = m.frame; b.next_id[s] = m.next_id; }
}

size_t ss_byte_lds_bytes() { return sizeof(ByteLds); }

// feats [F][S][MAXD][F] raw detection features, read when ReID is on (b.reid: xywh only, ss_byte_set_reid)
void ss_launch_byte_group(const SSByteDev& b, int F, const float* dets, const int* ndets, const float* feats, float* out, int* nout,
                          hipStream_t st)
{
    if (b.reid) {
        hipLaunchKernelGGL(k_byte_feats, dim3(SS_MAXD / 4, b.S, F), dim3(256), 0, st, b, feats, ndets);
        if (b.gmc) hipLaunchKernelGGL((k_byte_group<true, true, true, false>), dim3(b.S), dim3(256), 0, st, b, F, dets, ndets, out, nout);
        else hipLaunchKernelGGL((k_byte_group<true, false, true, false>), dim3(b.S), dim3(256), 0, st, b, F, dets, ndets, out, nout);
    }
    else if (b.xywh && b.gmc) hipLaunchKernelGGL((k_byte_group<true, true, false, false>), dim3(b.S), dim3(256), 0, st, b, F, dets, ndets, out, nout);
    else if (b.xywh) hipLaunchKernelGGL((k_byte_group<true, false, false, false>), dim3(b.S), dim3(256), 0, st, b, F, dets, ndets, out, nout);
    else hipLaunchKernelGGL((k_byte_group<false, false, false, false>), dim3(b.S), dim3(256), 0, st, b, F, dets, ndets, out, nout);
}

// §1e: the group with the rows' keypoints (b.pose: xywh only, ss_byte_set_pose); kpts / stride / off / geom as k_byte_kpts
void ss_launch_byte_group_kpts(const SSByteDev& b, int F, const float* dets, const int* ndets, const float* kpts, long long stride, int off,
                               const float* geom, float* out, int* nout, hipStream_t st)
{
    hipLaunchKernelGGL(k_byte_kpts, dim3(SS_MAXD / 8, b.S, F), dim3(256), 0, st, b, kpts, stride, off, geom, ndets);
    if (b.gmc) hipLaunchKernelGGL((k_byte_group<true, true, false, true>), dim3(b.S), dim3(256), 0, st, b, F, dets, ndets, out, nout);
    else hipLaunchKernelGGL((k_byte_group<true, false, false, true>), dim3(b.S), dim3(256), 0, st, b, F, dets, ndets, out, nout);
}

// docs/OBB.md §4: the group on 11-column rows (b.obb: ss_byte_set_obb); rbox [F][S][MAXT][5] goes with the launch arguments
void ss_launch_byte_group_obb(const SSByteDev& b0, int F, const float* dets, const int* ndets, float* out, float* rbox, int* nout, hipStream_t st)
{
    SSByteDev b = b0;
    b.rbox = rbox;
    if (b.xywh) hipLaunchKernelGGL((k_byte_group<true, false, false, false, true>), dim3(b.S), dim3(256), 0, st, b, F, dets, ndets, out, nout);
    else hipLaunchKernelGGL((k_byte_group<false, false, false, false, true>), dim3(b.S), dim3(256), 0, st, b, F, dets, ndets, out, nout);
}

// ---- host side: the state of a context ------------------------------------------------------------------------------------------
struct SSByte {
    SSByteDev dev;
    SsBuf<SS_DEVICE> base;              // the tables every mode has
    SsBuf<SS_DEVICE> reid, pose, obb;   // a mode's own, carved when it is first switched on (pose: again for another n_kpt)
};

void ss_byte_free(SSByte* b) { delete b; }
const SSByteDev& ss_byte_dev(const SSByte* b) { return b->dev; }
int ss_byte_pending_impl(SSByte* B, hipStream_t st, std::string& err) { return B ? ss_tracker_pending_impl(B->dev.err, B->dev.S, st, "BYTE tracker", err) : (int)SS_OK; }

int ss_byte_create_check_impl(const ss_byte_config* cfg, std::string& err)
{
    if (!cfg) { err = "ss_byte_create: null argument"; return SS_ERR_INVALID; }
    if (cfg->max_tracks < 1 || cfg->max_tracks > SS_MAXT || cfg->max_dets < 1 || cfg->max_dets > SS_MAXD || cfg->frame_rate < 1 ||
        cfg->track_buffer < 0 || (cfg->kalman_xywh != 0 && cfg->kalman_xywh != 1))
        { err = "ss_byte_create: 1 <= max_tracks <= 256, 1 <= max_dets <= 128, frame_rate >= 1, kalman_xywh 0 / 1"; return SS_ERR_INVALID; }
    return SS_OK;
}

// the streams' lists, counters, error words, warp flags and what the modes keep per track restart; synchronises
static int byte_reset(const SSByteDev& b, hipStream_t st, SsWarpFlags wf, int stream, const char* who, std::string& err)
{
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? b.S : stream + 1;
    const std::vector<int> ones(b.S, 1);
    SS_HIPCHK(who, hipMemsetAsync(b.frame + s0, 0, (s1 - s0) * 4, st));
    SS_HIPCHK(who, hipMemsetAsync(b.err + s0, 0, (s1 - s0) * 4, st));
    SS_HIPCHK(who, hipMemsetAsync(b.n_trk + s0, 0, (s1 - s0) * 4, st));
    SS_HIPCHK(who, hipMemsetAsync(b.n_lost + s0, 0, (s1 - s0) * 4, st));
    SS_HIPCHK(who, hipMemcpyAsync(b.next_id + s0, ones.data(), (s1 - s0) * 4, hipMemcpyHostToDevice, st));
    SS_HIPCHK(who, hipMemsetAsync(wf.cmc + s0, 0, (s1 - s0) * 4, st));
    SS_HIPCHK(who, hipMemsetAsync(wf.gmc + s0, 0, (s1 - s0) * 4, st));
    if (b.smooth)                                                                        // §1c: the streams' track features
        SS_HIPCHK(who, hipMemsetAsync(b.smooth + (size_t)s0 * SS_MAXT * SS_F, 0, (size_t)(s1 - s0) * SS_MAXT * SS_F * 4, st));
    if (b.tpose) {                                                                       // §1e: the streams' track poses
        SS_HIPCHK(who, hipMemsetAsync(b.tpose + (size_t)s0 * SS_MAXT * b.nk * 2, 0, (size_t)(s1 - s0) * SS_MAXT * b.nk * 2 * 8, st));
        SS_HIPCHK(who, hipMemsetAsync(b.tvis + (size_t)s0 * SS_MAXT, 0, (size_t)(s1 - s0) * SS_MAXT * 4, st));
    }
    SS_HIPCHK(who, hipStreamSynchronize(st));
    return SS_OK;
}

int ss_byte_reset_impl(SSByte* B, hipStream_t st, SsWarpFlags wf, int stream, std::string& err) { return byte_reset(B->dev, st, wf, stream, "ss_byte_reset: ", err); }

// the caller has drained the stream and freed the state this one replaces: a failure leaves none attached
int ss_byte_create_impl(SSByte** pb, hipStream_t st, SsWarpFlags wf, int n_streams, const ss_byte_config* cfg, std::string& err)
{
    std::unique_ptr<SSByte> B(new SSByte());
    SSByteDev& b = B->dev;
    memset(&b, 0, sizeof b);
    b.S = n_streams;
    b.xywh = cfg->kalman_xywh; b.fuse = cfg->fuse_score != 0;
    b.max_time_lost = (int)(cfg->frame_rate / 30.0 * cfg->track_buffer);
    b.max_tracks = cfg->max_tracks; b.max_dets = cfg->max_dets;
    b.high = (float)cfg->track_high_thresh; b.low = (float)cfg->track_low_thresh; b.new_thresh = (float)cfg->new_track_thresh;
    b.match = cfg->match_thresh; b.wp = cfg->std_weight_position; b.wv = cfg->std_weight_velocity;
    const size_t S = b.S, T = SS_MAXT;
    SsCarve c;
    c.add(&b.frame, S); c.add(&b.next_id, S); c.add(&b.err, S); c.add(&b.n_trk, S); c.add(&b.n_lost, S);
    c.add(&b.trk, S * T); c.add(&b.lost, S * T);
    c.add(&b.state, S * T); c.add(&b.act, S * T); c.add(&b.tid, S * T); c.add(&b.start, S * T); c.add(&b.end, S * T); c.add(&b.len, S * T);
    c.add(&b.det, S * T); c.add(&b.score, S * T); c.add(&b.cls, S * T);
    c.add(&b.mean, S * T * 8); c.add(&b.cov, S * T * 64); c.add(&b.spill, S * T * SS_MAXD);
    SS_HIPCHK("ss_byte_create: ", c.carve(B->base, st));
    if (const int rc = byte_reset(b, st, wf, -1, "ss_byte_create: ", err)) return rc;
    *pb = B.release();
    return SS_OK;
}

// The mode switches (ReID §1c, the keypoint term §1e, oriented boxes docs/OBB.md §4), on != 0 or off; either way every stream restarts.
// A mode's tables are carved when it is first switched on, and kept.  The modes are not combined, and xyah has none but obb.
int ss_byte_set_reid_impl(SSByte* B, hipStream_t st, SsWarpFlags wf, int on, double proximity_thresh, double appearance_thresh, double alpha, std::string& err)
{
    const char* who = "ss_byte_set_reid: ";
    SSByteDev& b = B->dev;
    auto bad = [&](const char* why) { err = std::string(who) + why; return (int)SS_ERR_INVALID; };
    if (on && !b.xywh) return bad("ReID needs the xywh (BoT-SORT) state");
    if (on && b.pose) return bad("the keypoint term is on (ss_byte_set_pose): the two are not combined");
    if (on && b.obb) return bad("oriented boxes are on (ss_byte_set_obb): the two are not combined");
    if (on && !b.smooth) {
        SsCarve c;
        c.add(&b.smooth, (size_t)b.S * SS_MAXT * SS_F); c.add(&b.ufeat, (size_t)SS_FMAX * b.S * SS_MAXD * SS_F);
        SS_HIPCHK(who, c.carve(B->reid, st));
    }
    b.reid = on != 0;
    b.prox = proximity_thresh; b.appear = appearance_thresh;
    b.alpha = (float)alpha; b.one_minus_alpha = (float)(1.0 - alpha);
    return byte_reset(b, st, wf, -1, who, err);
}

// (another n_kpt carves the pose tables again out of the same buffer, which grows only when it has to; the stream is drained first,
// so nothing reads the old tables any more)
int ss_byte_set_pose_impl(SSByte* B, hipStream_t st, SsWarpFlags wf, int on, int n_kpt, const double* sigmas, double proximity_thresh, double pose_thresh,
                          double vis_thresh, int min_common, std::string& err)
{
    const char* who = "ss_byte_set_pose: ";
    SSByteDev& b = B->dev;
    auto bad = [&](const char* why) { err = std::string(who) + why; return (int)SS_ERR_INVALID; };
    if (on) {
        if (!b.xywh) return bad("the keypoint term needs the xywh (BoT-SORT) state");
        if (b.reid) return bad("ReID is on (ss_byte_set_reid): the two are not combined");
        if (b.obb) return bad("oriented boxes are on (ss_byte_set_obb): the two are not combined");
        if (n_kpt < 1 || n_kpt > SS_BYTE_MAXK) return bad("1 <= n_kpt <= 32");
        if (!sigmas) return bad("sigmas is NULL");
        b.pose = 0;                                                // a failure below leaves the term off, never half set up
        SS_HIPCHK(who, hipStreamSynchronize(st));
        if (!b.tpose || b.nk != n_kpt) {
            const size_t nt = (size_t)b.S * SS_MAXT, nd = (size_t)SS_FMAX * b.S * SS_MAXD;
            SsCarve c;
            c.add(&b.tpose, nt * n_kpt * 2); c.add(&b.tvis, nt); c.add(&b.kp, nd * n_kpt * 2); c.add(&b.kvis, nd); c.add(&b.ks2, (size_t)SS_BYTE_MAXK);
            b.tpose = nullptr; b.kp = nullptr;                     // a carve that fails may have released the old tables
            SS_HIPCHK(who, c.carve(B->pose, st));
            b.nk = n_kpt;
        }
        double s2[SS_BYTE_MAXK] = {0.0};
        for (int k = 0; k < n_kpt; ++k) s2[k] = 2.0 * sigmas[k];
        SS_HIPCHK(who, hipMemcpyAsync((void*)b.ks2, s2, sizeof s2, hipMemcpyHostToDevice, st));      // on st: behind the carve's memset of the range
        SS_HIPCHK(who, hipStreamSynchronize(st));                  // s2 is this frame's
        b.prox = proximity_thresh; b.pose_thresh = pose_thresh; b.vis = (float)vis_thresh; b.min_common = min_common;
    }
    b.pose = on != 0;
    return byte_reset(b, st, wf, -1, who, err);
}

int ss_byte_set_obb_impl(SSByte* B, hipStream_t st, SsWarpFlags wf, int on, std::string& err)
{
    SSByteDev& b = B->dev;
    if (on && (b.reid || b.pose || b.gmc)) { err = "ss_byte_set_obb: ReID, the keypoint term or GMC is on: oriented boxes are not combined with them"; return SS_ERR_INVALID; }
    if (on && !b.angle) {
        const size_t nt = (size_t)b.S * SS_MAXT, nd = (size_t)b.S * SS_MAXD;
        SsCarve c;
        c.add(&b.angle, nt); c.add(&b.tbox, nt * 6); c.add(&b.dbox, nd * 6);
        SS_HIPCHK("ss_byte_set_obb: ", c.carve(B->obb, st));
    }
    b.obb = on != 0;
    return byte_reset(b, st, wf, -1, "ss_byte_set_obb: ", err);
}

// BoT-SORT GMC (docs/BYTETRACK.md §1b): the pointer goes into the launch arguments.  NULL: off.  xyah (ByteTrack) has no GMC (G-05).
int ss_byte_set_gmc_impl(SSByte* B, const double* d_warps, std::string& err)
{
    if (d_warps && !B->dev.xywh) { err = "ss_byte_set_gmc: GMC needs the xywh (BoT-SORT) state"; return SS_ERR_INVALID; }
    if (d_warps && B->dev.obb) { err = "ss_byte_set_gmc: oriented boxes are on (ss_byte_set_obb): GMC does not move rotated tracks"; return SS_ERR_INVALID; }
    B->dev.gmc = d_warps;
    return SS_OK;
}

// Synchronous: one stream's lists and, in list order (tracked, then lost), the per-track tables r asks for (SsByteRows, ss_launch.h)
int ss_byte_get_impl(SSByte* B, hipStream_t st, const char* entry, int s, int cap, const SsByteRows& r, std::string& err)
{
    const std::string who = std::string(entry) + ": ";
    const SSByteDev& b = B->dev;
    auto bad = [&](int rc, const char* why) { err = who + why; return rc; };
    if (r.smooth && !b.smooth) return bad(SS_ERR_INVALID, "ReID was never switched on (ss_byte_set_reid)");
    if ((r.pose || r.offsets || r.visible) && !b.tpose) return bad(SS_ERR_INVALID, "the keypoint term was never switched on (ss_byte_set_pose)");
    if (r.angles && !b.angle) return bad(SS_ERR_INVALID, "oriented boxes were never switched on (ss_byte_set_obb)");
    SS_HIPCHK(who, hipStreamSynchronize(st));
    int nt = 0, nl = 0, nid = 0, fr = 0;
    SS_HIPCHK(who, hipMemcpy(&nid, b.next_id + s, 4, hipMemcpyDeviceToHost));
    SS_HIPCHK(who, hipMemcpy(&fr, b.frame + s, 4, hipMemcpyDeviceToHost));
    SS_HIPCHK(who, hipMemcpy(&nt, b.n_trk + s, 4, hipMemcpyDeviceToHost));
    SS_HIPCHK(who, hipMemcpy(&nl, b.n_lost + s, 4, hipMemcpyDeviceToHost));
    if (r.n_tracked) *r.n_tracked = nt;
    if (r.n_lost) *r.n_lost = nl;
    if (r.next_id) *r.next_id = nid;
    if (r.frame_id) *r.frame_id = fr;
    if (nt < 0 || nl < 0) return bad(SS_ERR_CAPACITY, "corrupt list");
    const int n = nt + nl;
    if (n > cap) return bad(SS_ERR_CAPACITY, "cap too small");
    const size_t T = SS_MAXT, sb = (size_t)s * T;
    std::vector<int> trk(T), lost(T), slots(n);
    SS_HIPCHK(who, hipMemcpy(trk.data(), b.trk + sb, T * 4, hipMemcpyDeviceToHost));
    SS_HIPCHK(who, hipMemcpy(lost.data(), b.lost + sb, T * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        slots[i] = i < nt ? trk[i] : lost[i - nt];
        if (slots[i] < 0 || slots[i] >= SS_MAXT) return bad(SS_ERR_CAPACITY, "corrupt list");
    }
    SS_HIPCHK(who, ss_gather_device(slots.data(), n, b.tid + sb, T, 1, r.track_id));
    SS_HIPCHK(who, ss_gather_device(slots.data(), n, b.state + sb, T, 1, r.state));
    SS_HIPCHK(who, ss_gather_device(slots.data(), n, b.act + sb, T, 1, r.activated));
    SS_HIPCHK(who, ss_gather_device(slots.data(), n, b.mean + sb * 8, T, 8, r.mean));
    if (r.smooth) SS_HIPCHK(who, ss_gather_device(slots.data(), n, b.smooth + sb * SS_F, T, SS_F, r.smooth));
    if (r.offsets) SS_HIPCHK(who, ss_gather_device(slots.data(), n, b.tpose + sb * b.nk * 2, T, b.nk * 2, r.offsets));
    if (r.visible) SS_HIPCHK(who, ss_gather_device(slots.data(), n, b.tvis + sb, T, 1, r.visible));
    if (r.angles) SS_HIPCHK(who, ss_gather_device(slots.data(), n, b.angle + sb, T, 1, r.angles));
    return SS_OK;
}

// Synchronous: what k_byte_kpts wrote for image (frame, stream) of the last ss_byte_update_group_kpts call
int ss_byte_get_det_keypoints_impl(SSByte* B, hipStream_t st, int frame, int s, float* xy, unsigned* visible, std::string& err)
{
    const char* who = "ss_byte_get_det_keypoints: ";
    const SSByteDev& b = B->dev;
    if (!b.kp) { err = std::string(who) + "the keypoint term was never switched on (ss_byte_set_pose)"; return SS_ERR_INVALID; }
    SS_HIPCHK(who, hipStreamSynchronize(st));
    const size_t fs = (size_t)frame * b.S + s;
    SS_HIPCHK(who, hipMemcpy(xy, b.kp + fs * SS_MAXD * b.nk * 2, (size_t)SS_MAXD * b.nk * 2 * 4, hipMemcpyDeviceToHost));
    SS_HIPCHK(who, hipMemcpy(visible, b.kvis + fs * SS_MAXD, (size_t)SS_MAXD * 4, hipMemcpyDeviceToHost));
    return SS_OK;
}
