// ss_ocsort_body.h — the OC-SORT frame procedure on the device (docs/OCSORT.md), shared by k_ocsort_group (csrc/ss_ocsort.hip) and
// k_deepoc_group (csrc/ss_deepoc.hip, docs/DEEPOCSORT.md): the LDS layout, the step bodies (oc_iou, oc_box_to_z, oc_predict, oc_update,
// oc_assign, oc_second) and oc_group<DEEP>, the walk of one stream over the group's frames by one workgroup of 256 threads.
// DEEP = false is OC-SORT; DEEP = true adds Deep OC-SORT's steps at three places (camera motion before the predict, the appearance
// cost before the LSAP, the tracks' features after the updates) and compiles to the same code elsewhere.
//
// The list logic and the frame's rows live in LDS; the filters (x, P, their frozen copies), the observation rings and the
// velocities stay in global memory, one thread per track for the f64 Kalman work.  tests/ocsort_ref.py restates every step in the
// same order (rows and tables are compared bit for bit).  The library is built with -ffp-contract=off: only the explicit fma()
// calls of ss_kalman.h's 4x4 solve fuse.
#pragma once
#include "ss_common.h"
#include "ss_launch.h"
#include "ss_lsap.h"
#include "ss_asin.h"

#define SS_OC_COST_CAP 2048            // LDS-resident cost entries (f64); a larger matrix lives in the stream's global spill area
#define SS_OC_DEAD (-2)                // mdet of a track whose predicted box is not finite (O-10)

struct OcLds {
    // slot fields (copies of the global table for the duration of the launch)
    int id[SS_MAXT], age[SS_MAXT], tsu[SS_MAXT], streak[SS_MAXT], hasobs[SS_MAXT], det[SS_MAXT];
    float score[SS_MAXT], cls[SS_MAXT];
    float lobs[SS_MAXT][4];
    int trk[SS_MAXT];                  // the list, in order
    // per list position, this frame
    double pbox[SS_MAXT][4];           // predicted box xyxy
    double kc[SS_MAXT][2];             // centre of the observation delta_t ages back (O-07)
    double vel[SS_MAXT][2];
    int mdet[SS_MAXT];                 // detection matched this frame, -1, or SS_OC_DEAD
    // the frame's detections
    double dbox[SS_MAXD][4];
    float dsc[SS_MAXD], dcls[SS_MAXD];
    int hi[SS_MAXD], lo[SS_MAXD], used[SS_MAXD], ud[SS_MAXD], rowc[SS_MAXD], cand[SS_MAXD];
    // work lists
    int ut[SS_MAXT], asg[SS_MAXT], col4row[SS_MAXT], freel[SS_MAXT], born[SS_MAXT], colc[SS_MAXT];
    double cost[SS_OC_COST_CAP];
    int wtot[4];
    int any, multi;
    int n_trk, frame, next_id;
};

// IoU of two xyxy boxes; 0 where the union is not positive (tests/ocsort_ref.py iou_matrix)
__device__ inline double oc_iou(const double* d, const double* t)
{
    double w = fmin(d[2], t[2]) - fmax(d[0], t[0]);
    double h = fmin(d[3], t[3]) - fmax(d[1], t[1]);
    w = w > 0.0 ? w : 0.0;
    h = h > 0.0 ? h : 0.0;
    const double inter = w * h;
    const double u = (d[2] - d[0]) * (d[3] - d[1]) + (t[2] - t[0]) * (t[3] - t[1]) - inter;
    return u > 0.0 ? inter / u : 0.0;
}

// xyxy -> (x, y, s, r) (upstream's convert_bbox_to_z)
__device__ inline void oc_box_to_z(const double* b, double* z)
{
    const double w = b[2] - b[0], h = b[3] - b[1];
    z[0] = b[0] + w / 2.0; z[1] = b[1] + h / 2.0; z[2] = w * h; z[3] = w / (h + 1e-6);
}

// x = F x, P = F P F^T + Q: F adds the velocity of x, y, s (additions only)
__device__ inline void oc_predict(double* x, double* P)
{
    const double Q[7] = {1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 0.0001};
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) P[i * 7 + j] = P[i * 7 + j] + P[i * 7 + j + 4];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 7; ++j) P[i * 7 + j] = P[i * 7 + j] + P[(i + 4) * 7 + j];
#pragma unroll
    for (int i = 0; i < 7; ++i) P[i * 7 + i] = P[i * 7 + i] + Q[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = x[i] + x[i + 4];
}

// The Joseph-form update with H = [I4 0] (docs/OCSORT.md O-09): S = P[:4,:4] + R, K = P[:, :4] S^-1 by ss_kalman.h's Cholesky solves,
// x += K (z - x[:4]), P = (I - K H) P (I - K H)^T + K R K^T row by row: b = P[r] - K[r] P[:4, :], then b - b[:4] K^T + (K[r] R) K^T.
__device__ inline void oc_update(double* x, double* P, const double* z)
{
    const double R[4] = {1.0, 1.0, 10.0, 10.0};
    double S[16], L[16], K[28], top[28], y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) S[i * 4 + j] = P[i * 7 + j];
#pragma unroll
    for (int i = 0; i < 4; ++i) S[i * 4 + i] = S[i * 4 + i] + R[i];
    ss_chol4(S, L);
#pragma unroll
    for (int r = 0; r < 7; ++r) ss_kf_gain_row(L, P + r * 7, K + r * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = z[i] - x[i];
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc = acc + K[r * 4 + k] * y[k];
        x[r] = x[r] + acc;
    }
#pragma unroll
    for (int i = 0; i < 28; ++i) top[i] = P[i];
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        double b[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = acc + K[r * 4 + k] * top[k * 7 + c];
            b[c] = P[r * 7 + c] - acc;
        }
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = acc + b[k] * K[c * 4 + k];
            const double t = b[c] - acc;
            acc = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = acc + (K[r * 4 + k] * R[k]) * K[c * 4 + k];
            P[r * 7 + c] = t + acc;
        }
    }
}

// LSAP of an n_rows x n_cols matrix already stored by lsap_cidx -> m.asg[row] = column or -1 (all threads call it).
__device__ inline void oc_assign(int n_rows, int n_cols, const double* cost, bool glb, OcLds& m, int* err)
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

// The BYTE stage and OCR share a shape: rows (detections rd[r]) x the unmatched tracks m.ut[k], cost -IoU against the tracks'
// predicted boxes (LAST = false) or last observations (LAST = true); solved only when some IoU exceeds the threshold; a pair is
// kept when its IoU >= the threshold.  A kept pair sets m.mdet of the track and, with `mark`, m.used of the row's high position.
template <bool LAST>
__device__ inline void oc_second(int nR, const int* rd, const int* mark, int nU, const SSOcDev& o, double* spill, OcLds& m, int* err)
{
    const int tid = threadIdx.x;
    if (nR == 0 || nU == 0) return;                                // uniform
    const bool glb = nR * nU > SS_OC_COST_CAP;
    double* cost = glb ? spill : m.cost;
    if (tid == 0) m.any = 0;
    __syncthreads();
    auto iou_of = [&](int r, int k) {
        const int p = m.ut[k];
        if (LAST) {
            const int slot = m.trk[p];
            if (!m.hasobs[slot]) return 0.0;
            const double t[4] = {(double)m.lobs[slot][0], (double)m.lobs[slot][1], (double)m.lobs[slot][2], (double)m.lobs[slot][3]};
            return oc_iou(m.dbox[rd[r]], t);
        }
        return oc_iou(m.dbox[rd[r]], m.pbox[p]);
    };
    for (int e = tid; e < nR * nU; e += 256) {
        const int r = e / nU, k = e - r * nU;
        const double iou = iou_of(r, k);
        cost[lsap_cidx(r, k, nR, nU)] = -iou;
        if (iou > o.iou_thr) m.any = 1;
    }
    __syncthreads();
    if (!m.any) return;                                            // uniform: read after the barrier, written before it
    oc_assign(nR, nU, cost, glb, m, err);
    if (tid < nR) {
        const int k = m.asg[tid];
        if (k >= 0 && !(iou_of(tid, k) < o.iou_thr)) {
            m.mdet[m.ut[k]] = rd[tid];
            if (mark) m.used[mark[tid]] = 1;
        }
    }
    __syncthreads();
}

// Deep OC-SORT's three additions (csrc/ss_deepoc.hip defines them; oc_group names them only with DEEP)
struct DeepLds {
    double rf[SS_MAXD], cf[SS_MAXT];   // adaptive weighting: the factor of every row and of every track of the first association
};
__device__ inline void deepoc_cmc(const SSOcDev& o, const double* w, size_t sb, int nT, OcLds& m);
__device__ inline void deepoc_appearance(const SSDeepOcDev& x, int nHi, int nT, double* cost, size_t s, size_t fs, OcLds& m, DeepLds& dl);
__device__ inline void deepoc_features(const SSDeepOcDev& x, size_t sb, size_t fs, int nT, int nB, OcLds& m);

template <bool DEEP>
__device__ __forceinline__ void oc_group(const SSOcDev& o, const SSDeepOcDev* deep, DeepLds* dl, int F, const float* __restrict__ dets,
                                         const int* __restrict__ ndets, float* __restrict__ out, int* __restrict__ nout, OcLds& m)
{
    const int s = blockIdx.x, tid = threadIdx.x, S = o.S, D = o.delta_t;
    const size_t sb = (size_t)s * SS_MAXT;
    double* spill = o.spill + (size_t)s * SS_MAXT * SS_MAXD;
    int* err = o.err + s;
    // ---- the stream's table into LDS ----
    m.id[tid] = o.tid[sb + tid]; m.age[tid] = o.age[sb + tid]; m.tsu[tid] = o.tsu[sb + tid]; m.streak[tid] = o.streak[sb + tid];
    m.hasobs[tid] = o.hasobs[sb + tid]; m.det[tid] = o.det[sb + tid]; m.score[tid] = o.score[sb + tid]; m.cls[tid] = o.cls[sb + tid];
#pragma unroll
    for (int i = 0; i < 4; ++i) m.lobs[tid][i] = o.lobs[(sb + tid) * 4 + i];
    m.trk[tid] = o.trk[sb + tid];
    if (tid == 0) { m.n_trk = o.n_trk[s]; m.frame = o.frame[s]; m.next_id = o.next_id[s]; }
    __syncthreads();

    for (int f = 0; f < F; ++f) {
        const size_t fs = (size_t)f * S + s;
        const int nraw = ndets[fs];
        const int N = min(max(nraw, 0), o.max_dets);
        const int nT = m.n_trk;
        const int fid = m.frame + 1;
        if (tid == 0 && (nraw < 0 || nraw > o.max_dets)) *err = SS_ERR_CAPACITY;
        // ---- 1. detections and the score split ----
        int isHi = 0, isLo = 0;
        if (tid < N) {
            const float* d = dets + (fs * SS_MAXD + tid) * 6;
            const float sc = d[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) m.dbox[tid][i] = (double)d[i];
            m.dsc[tid] = sc; m.dcls[tid] = d[5];
            isHi = sc > o.det_thresh;
            isLo = o.use_byte && sc > o.low_thresh && sc < o.det_thresh;
        }
        if (tid < SS_MAXD) { m.used[tid] = 0; m.rowc[tid] = 0; }
        m.colc[tid] = 0;
        if (tid == 0) { m.any = 0; m.multi = 0; }
        int pos, nHi, nLo;
        block_scan256(isHi, m.wtot, pos, nHi);
        if (isHi) m.hi[pos] = tid;
        block_scan256(isLo, m.wtot, pos, nLo);
        if (isLo) m.lo[pos] = tid;
        // ---- 1b. Deep OC-SORT: camera-motion compensation of filters and observations (warp [6] < 0: none) ----
        if constexpr (DEEP) {
            if (deep->gmc && deep->gmc[fs * 8 + 6] >= 0.0) deepoc_cmc(o, deep->gmc + fs * 8, sb, nT, m);
        }
        // ---- 2. predict every track (thread = list position) ----
        if (tid < nT) {
            const int slot = m.trk[tid];
            const size_t g = sb + slot;
            double x[7], P[49];
#pragma unroll
            for (int i = 0; i < 7; ++i) x[i] = o.x[g * 7 + i];
#pragma unroll
            for (int i = 0; i < 49; ++i) P[i] = o.P[g * 49 + i];
            if (x[6] + x[2] <= 0.0) x[6] = 0.0;
            oc_predict(x, P);
#pragma unroll
            for (int i = 0; i < 7; ++i) o.x[g * 7 + i] = x[i];
#pragma unroll
            for (int i = 0; i < 49; ++i) o.P[g * 49 + i] = P[i];
            const int age = m.age[slot] + 1;
            m.age[slot] = age;
            if (m.tsu[slot] > 0) m.streak[slot] = 0;
            m.tsu[slot] += 1;
            const double w = sqrt(x[2] * x[3]), h = x[2] / w;
            double* pb = m.pbox[tid];
            pb[0] = x[0] - w / 2.0; pb[1] = x[1] - h / 2.0; pb[2] = x[0] + w / 2.0; pb[3] = x[1] + h / 2.0;
            const bool ok = isfinite(pb[0]) && isfinite(pb[1]) && isfinite(pb[2]) && isfinite(pb[3]);
            m.mdet[tid] = ok ? -1 : SS_OC_DEAD;
            // the observation delta_t ages back, else the nearest later one, else the last
            double k0 = 0.0, k1 = 0.0, k2 = 0.0, k3 = 0.0;
            if (m.hasobs[slot]) {
                k0 = (double)m.lobs[slot][0]; k1 = (double)m.lobs[slot][1]; k2 = (double)m.lobs[slot][2]; k3 = (double)m.lobs[slot][3];
                for (int dt = D; dt >= 1; --dt) {
                    const int a = age - dt;
                    if (a < 0) continue;
                    const int e = a % D;
                    if (o.rage[g * SS_OC_MAXDT + e] == a) {
                        const float* q = o.ring + (g * SS_OC_MAXDT + e) * 4;
                        k0 = (double)q[0]; k1 = (double)q[1]; k2 = (double)q[2]; k3 = (double)q[3];
                        break;
                    }
                }
            }
            m.kc[tid][0] = (k0 + k2) / 2.0; m.kc[tid][1] = (k1 + k3) / 2.0;
            m.vel[tid][0] = o.vel[g * 2]; m.vel[tid][1] = o.vel[g * 2 + 1];
        }
        __syncthreads();
        // ---- 3. first association: high rows x all tracks, -(IoU + momentum term) ----
        if (nHi > 0 && nT > 0) {
            const bool glb = nHi * nT > SS_OC_COST_CAP;
            double* cost = glb ? spill : m.cost;
            for (int e = tid; e < nHi * nT; e += 256) {
                const int r = e / nT, k = e - r * nT, d = m.hi[r];
                const bool live = m.mdet[k] != SS_OC_DEAD;
                const double* db = m.dbox[d];
                const double iou = live ? oc_iou(db, m.pbox[k]) : 0.0;
                double term = 0.0;
                if (live && m.hasobs[m.trk[k]]) {
                    const double dx = (db[0] + db[2]) / 2.0 - m.kc[k][0], dy = (db[1] + db[3]) / 2.0 - m.kc[k][1];
                    const double n = sqrt(dx * dx + dy * dy) + 1e-6;
                    const double ux = dx / n, uy = dy / n;
                    double c = m.vel[k][0] * ux + m.vel[k][1] * uy;
                    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
                    term = ss_asin(c) / 3.141592653589793;
                    term = term * o.inertia;
                    term = term * (double)m.dsc[d];
                }
                cost[lsap_cidx(r, k, nHi, nT)] = -(iou + term);
                if (iou > o.iou_thr) {
                    m.any = 1;
                    m.cand[r] = k;
                    if (atomicAdd(&m.rowc[r], 1) > 0) m.multi = 1;
                    if (atomicAdd(&m.colc[k], 1) > 0) m.multi = 1;
                }
            }
            __syncthreads();
            if (m.any && !m.multi) {                               // upstream's shortcut: the pairs above the threshold are the match
                __syncthreads();
                m.asg[tid] = (tid < nHi && m.rowc[tid]) ? m.cand[tid] : -1;
                __syncthreads();
            } else {
                if constexpr (DEEP) {                                        // the appearance cost joins only a matrix that the LSAP solves
                    if (deep->appearance) deepoc_appearance(*deep, nHi, nT, cost, s, fs, m, *dl);
                }
                oc_assign(nHi, nT, cost, glb, m, err);
            }
            if (tid < nHi) {
                const int k = m.asg[tid];
                if (k >= 0 && m.mdet[k] != SS_OC_DEAD && !(oc_iou(m.dbox[m.hi[tid]], m.pbox[k]) < o.iou_thr)) {
                    m.mdet[k] = m.hi[tid];
                    m.used[tid] = 1;
                }
            }
        }
        __syncthreads();
        // ---- 4. BYTE stage: the low-score rows x the unmatched tracks' predicted boxes ----
        int nU;
        if (nLo > 0) {
            const int isU = tid < nT && m.mdet[tid] == -1;
            block_scan256(isU, m.wtot, pos, nU);
            if (isU) m.ut[pos] = tid;
            __syncthreads();
            oc_second<false>(nLo, m.lo, nullptr, nU, o, spill, m, err);
        }
        // ---- 5. OCR: the high rows left over x the remaining tracks' last observations ----
        int nD;
        {
            const int isU = tid < nT && m.mdet[tid] == -1, isD = tid < nHi && !m.used[tid];
            block_scan256(isU, m.wtot, pos, nU);
            if (isU) m.ut[pos] = tid;
            block_scan256(isD, m.wtot, pos, nD);
            if (isD) { m.ud[pos] = m.hi[tid]; m.cand[pos] = tid; }
            __syncthreads();
            oc_second<true>(nD, m.ud, m.cand, nU, o, spill, m, err);
        }
        // ---- 6. births: the high rows still unmatched, ascending, into the free slots ascending ----
        int nB;
        {
            const int isB = tid < nHi && !m.used[tid];
            int rank, nCand, fpos, nFree;
            m.asg[tid] = 0;
            __syncthreads();
            if (tid < nT) m.asg[m.trk[tid]] = 1;                   // a slot is free when the list at the frame's start does not hold it
            __syncthreads();
            const int isF = !m.asg[tid];
            block_scan256(isF, m.wtot, fpos, nFree);
            if (isF) m.freel[fpos] = tid;
            block_scan256(isB, m.wtot, rank, nCand);
            const int allowed = max(0, o.max_tracks - nT);
            nB = min(nCand, allowed);
            if (tid == 0 && nCand > allowed) *err = SS_ERR_CAPACITY;
            __syncthreads();
            if (isB && rank < nB) m.born[rank] = m.freel[rank];
        }
        // ---- 7. updates (thread = list position): velocity, observation, counters, the filter with ORU; a miss freezes ----
        if (tid < nT) {
            const int slot = m.trk[tid], d = m.mdet[tid];
            const size_t g = sb + slot;
            if (d >= 0) {
                const double* db = m.dbox[d];
                double z1[4] = {0.0, 0.0, 0.0, 0.0}, z2[4];
                if (m.hasobs[slot]) {
                    const double dx = (db[0] + db[2]) / 2.0 - m.kc[tid][0], dy = (db[1] + db[3]) / 2.0 - m.kc[tid][1];
                    const double n = sqrt(dx * dx + dy * dy) + 1e-6;
                    o.vel[g * 2] = dx / n; o.vel[g * 2 + 1] = dy / n;
                    const double lb[4] = {(double)m.lobs[slot][0], (double)m.lobs[slot][1], (double)m.lobs[slot][2], (double)m.lobs[slot][3]};
                    oc_box_to_z(lb, z1);
                }
                oc_box_to_z(db, z2);
                const int age = m.age[slot], e = age % D, gap = m.tsu[slot];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = (float)db[i];                  // exact: the row's float32 value
                    m.lobs[slot][i] = v;
                    o.ring[(g * SS_OC_MAXDT + e) * 4 + i] = v;
                }
                o.rage[g * SS_OC_MAXDT + e] = age;
                m.hasobs[slot] = 1; m.tsu[slot] = 0; m.streak[slot] += 1;
                o.hits[g] += 1;
                m.score[slot] = m.dsc[d]; m.cls[slot] = m.dcls[d]; m.det[slot] = d;
                const bool frozen = o.frozen[g] != 0;
                const double* xs = frozen ? o.xf : o.x;
                const double* Ps = frozen ? o.Pf : o.P;
                double x[7], P[49];
#pragma unroll
                for (int i = 0; i < 7; ++i) x[i] = xs[g * 7 + i];
#pragma unroll
                for (int i = 0; i < 49; ++i) P[i] = Ps[g * 49 + i];
                // ORU: `gap` virtual observations on the line z1 -> z2 from the frozen filter, then the ordinary update
                const int nv = frozen ? gap : 0;
                const double w1 = sqrt(z1[2] * z1[3]), h1 = sqrt(z1[2] / z1[3]), w2 = sqrt(z2[2] * z2[3]), h2 = sqrt(z2[2] / z2[3]);
                const double gf = (double)(nv > 0 ? nv : 1);
                const double ddx = (z2[0] - z1[0]) / gf, ddy = (z2[1] - z1[1]) / gf, ddw = (w2 - w1) / gf, ddh = (h2 - h1) / gf;
                for (int j = 0; j <= nv; ++j) {
                    double z[4];
                    if (j < nv) {
                        const double fi = (double)(j + 1);
                        const double vw = w1 + fi * ddw, vh = h1 + fi * ddh;
                        z[0] = z1[0] + fi * ddx; z[1] = z1[1] + fi * ddy; z[2] = vw * vh; z[3] = vw / vh;
                    } else { z[0] = z2[0]; z[1] = z2[1]; z[2] = z2[2]; z[3] = z2[3]; }
                    oc_update(x, P, z);
                    if (j + 1 < nv) oc_predict(x, P);
                }
#pragma unroll
                for (int i = 0; i < 7; ++i) o.x[g * 7 + i] = x[i];
#pragma unroll
                for (int i = 0; i < 49; ++i) o.P[g * 49 + i] = P[i];
                o.frozen[g] = 0; o.obsd[g] = 1;
            } else if (o.obsd[g]) {                                // the first miss after an observation freezes the filter
                for (int i = 0; i < 7; ++i) o.xf[g * 7 + i] = o.x[g * 7 + i];
                for (int i = 0; i < 49; ++i) o.Pf[g * 49 + i] = o.P[g * 49 + i];
                o.frozen[g] = 1; o.obsd[g] = 0;
            }
        }
        __syncthreads();
        // ---- births' fields (thread = birth rank; m.used / m.hi are stable since stage 5) ----
        {
            const int isB = tid < nHi && !m.used[tid];
            int rank, nCand;
            block_scan256(isB, m.wtot, rank, nCand);
            if (isB && rank < nB) {
                const int slot = m.born[rank], d = m.hi[tid];
                const size_t g = sb + slot;
                double z[4];
                oc_box_to_z(m.dbox[d], z);
                const double P0[7] = {10.0, 10.0, 10.0, 10.0, 1e4, 1e4, 1e4};
#pragma unroll
                for (int i = 0; i < 7; ++i) o.x[g * 7 + i] = i < 4 ? z[i < 4 ? i : 0] : 0.0;
#pragma unroll
                for (int i = 0; i < 49; ++i) o.P[g * 49 + i] = (i / 7 == i % 7) ? P0[i / 7] : 0.0;
                for (int i = 0; i < SS_OC_MAXDT; ++i) o.rage[g * SS_OC_MAXDT + i] = -1;
                o.vel[g * 2] = 0.0; o.vel[g * 2 + 1] = 0.0;
                o.frozen[g] = 0; o.obsd[g] = 0; o.hits[g] = 0;
                m.id[slot] = m.next_id + rank;
                m.age[slot] = 0; m.tsu[slot] = 0; m.streak[slot] = 0; m.hasobs[slot] = 0;   // O-06: the birth row is shown, not observed
#pragma unroll
                for (int i = 0; i < 4; ++i) m.lobs[slot][i] = (float)m.dbox[d][i];
                m.score[slot] = m.dsc[d]; m.cls[slot] = m.dcls[d]; m.det[slot] = d;
            }
        }
        __syncthreads();
        if constexpr (DEEP) {                                                // the births' and the matched tracks' features (m.mdet is by list position)
            if (deep->appearance) deepoc_features(*deep, sb, fs, nT, nB, m);
            __syncthreads();
        }
        // ---- 8. the list: the tracks within max_age whose box was finite, then the births; rows newest first ----
        {
            const int old = tid < nT ? m.trk[tid] : 0;
            const int keep = tid < nT && !(m.tsu[old] > o.max_age) && m.mdet[tid] != SS_OC_DEAD;
            int p0, t0;
            block_scan256(keep, m.wtot, p0, t0);
            __syncthreads();
            if (keep) m.trk[p0] = old;
            if (tid < nB) m.trk[t0 + tid] = m.born[tid];
            const int nT2 = t0 + nB;
            __syncthreads();
            const int slot = tid < nT2 ? m.trk[tid] : 0;
            const int emit = tid < nT2 && m.tsu[slot] < 1 && (m.streak[slot] >= o.min_hits || fid <= o.min_hits);
            int row, nRow;
            block_scan256(emit, m.wtot, row, nRow);
            if (emit) {
                float* q = out + (fs * SS_MAXT + (nRow - 1 - row)) * 8;
                q[0] = m.lobs[slot][0]; q[1] = m.lobs[slot][1]; q[2] = m.lobs[slot][2]; q[3] = m.lobs[slot][3];
                q[4] = (float)m.id[slot]; q[5] = m.cls[slot]; q[6] = m.score[slot]; q[7] = (float)m.det[slot];
            }
            if (tid == 0) {
                nout[fs] = nRow;
                m.n_trk = nT2; m.frame = fid; m.next_id += nB;
            }
        }
        __syncthreads();
    }
    // ---- the table back to global memory ----
    o.tid[sb + tid] = m.id[tid]; o.age[sb + tid] = m.age[tid]; o.tsu[sb + tid] = m.tsu[tid]; o.streak[sb + tid] = m.streak[tid];
    o.hasobs[sb + tid] = m.hasobs[tid]; o.det[sb + tid] = m.det[tid]; o.score[sb + tid] = m.score[tid]; o.cls[sb + tid] = m.cls[tid];
#pragma unroll
    for (int i = 0; i < 4; ++i) o.lobs[(sb + tid) * 4 + i] = m.lobs[tid][i];
    o.trk[sb + tid] = m.trk[tid];
    if (tid == 0) { o.n_trk[s] = m.n_trk; o.frame[s] = m.frame; o.next_id[s] = m.next_id; }
}

