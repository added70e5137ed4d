// ss_hybrid.hip — the Hybrid-SORT tracker on the device (docs/HYBRIDSORT.md): S independent streams, a GROUP of F <= SS_FMAX frames per call.
//
//   k_hybrid_group  one workgroup (256 threads) per stream walks the group's frames in order inside the launch: OC-SORT's frame procedure
//                   (csrc/ss_ocsort_body.h) with Hybrid-SORT's three cues — the confidence as a Kalman state and a cost term (TCM) in
//                   the first association and the BYTE stage, the height-modulated IoU, and the direction term over the four box corners
//                   and delta_t time offsets.  One launch per call, no host round trip: capturable.
//
// The 9-state filter is block diagonal for ever (F over the pairs (x, vx), (y, vy), (s, vs), (c, vc) and r alone, H selects the first
// of each, Q, R and the initial P diagonal), so it is kept as what it is: four 2-state filters and one scalar filter, SS_HY_FLT = 26
// doubles a track, in registers of the track's thread (H-02).  tests/hybridsort_ref.py restates every step in the same order (rows and
// tables are compared bit for bit); the library is built with -ffp-contract=off.
#include "ss_ocsort_body.h"

struct HyLds {
    // slot fields (copies of the global table for the duration of the launch)
    int id[SS_MAXT], age[SS_MAXT], tsu[SS_MAXT], streak[SS_MAXT], hasobs[SS_MAXT], det[SS_MAXT], hasprev[SS_MAXT];
    float score[SS_MAXT], cls[SS_MAXT], cprev[SS_MAXT];
    float lobs[SS_MAXT][4];
    int trk[SS_MAXT];                  // the list, in order
    // per list position, this frame
    double pbox[SS_MAXT][4];           // predicted box xyxy
    float kobs[SS_MAXT][4];            // the observation delta_t ages back (O-07): a stored row, float32
    double vel[SS_MAXT][8];            // the corners' velocities lt, rt, lb, rb
    double ckal[SS_MAXT], clin[SS_MAXT];   // the two confidences (TCM)
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

// A of two xyxy boxes: IoU, with hmiou times the ratio of the heights' overlap to their span; 0 where IoU is 0 (H-04)
__device__ inline double hy_assoc(const double* d, const double* t, bool hmiou)
{
    const double iou = oc_iou(d, t);
    if (!hmiou) return iou;
    const double den = fmax(d[3], t[3]) - fmin(d[1], t[1]);
    if (!(iou > 0.0 && den > 0.0)) return 0.0;
    const double num = fmin(d[3], t[3]) - fmax(d[1], t[1]);
    return iou * (num / den);
}

// corner k (lt, rt, lb, rb) of an xyxy box
__device__ inline void hy_corner(const double* b, int k, double& x, double& y) { x = b[(k & 1) ? 2 : 0]; y = b[(k & 2) ? 3 : 1]; }

// xyxy and the score -> the measurement (x, y, s, c, r)
__device__ inline void hy_box_to_z(const double* b, double score, double* z)
{
    const double w = b[2] - b[0], h = b[3] - b[1];
    z[0] = b[0] + w / 2.0; z[1] = b[1] + h / 2.0; z[2] = w * h; z[3] = score; z[4] = w / (h + 1e-6);
}

// Each pair: p += v, P = F P F^T + Q by additions (columns, rows, diagonal); r's variance grows by 1
__device__ inline void hy_predict(double* f)
{
    const double Q0[4] = {1.0, 1.0, 1.0, 1.0}, Q1[4] = {0.01, 0.01, 1e-4, 1e-4};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double* q = f + i * 6;
        q[0] = q[0] + q[1];
        q[2] = q[2] + q[3];
        q[4] = q[4] + q[5];
        q[2] = q[2] + q[4];
        q[3] = q[3] + q[5];
        q[2] = q[2] + Q0[i];
        q[5] = q[5] + Q1[i];
    }
    f[25] = f[25] + 1.0;
}

// Every component on its own (H-03): k = P[:, 0] / (P00 + R), x += k (z - x0), the Joseph form as B = P - k P[0, :], then
// (B - B[:, 0] k^T) + (k R) k^T
__device__ inline void hy_update(double* f, const double* z)
{
    const double Rp[4] = {1.0, 1.0, 10.0, 10.0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double* q = f + i * 6;
        const double R = Rp[i], p00 = q[2], p01 = q[3], p10 = q[4], p11 = q[5];
        const double S = p00 + R;
        const double k0 = p00 / S, k1 = p10 / S;
        const double y = z[i] - q[0];
        q[0] = q[0] + k0 * y;
        q[1] = q[1] + k1 * y;
        const double b00 = p00 - k0 * p00, b01 = p01 - k0 * p01, b10 = p10 - k1 * p00, b11 = p11 - k1 * p01;
        const double r0 = k0 * R, r1 = k1 * R;
        q[2] = (b00 - b00 * k0) + r0 * k0;
        q[3] = (b01 - b00 * k1) + r0 * k1;
        q[4] = (b10 - b10 * k0) + r1 * k0;
        q[5] = (b11 - b10 * k1) + r1 * k1;
    }
    const double P = f[25];
    const double k = P / (P + 10.0);
    f[24] = f[24] + k * (z[4] - f[24]);
    const double b = P - k * P;
    f[25] = (b - b * k) + (k * 10.0) * k;
}

__device__ inline double hy_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// LSAP of an n_rows x n_cols matrix already stored by lsap_cidx -> m.asg[row] = column or -1 (all threads call it).
__device__ inline void hy_assign(int n_rows, int n_cols, const double* cost, bool glb, HyLds& m, int* err)
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

// The BYTE stage (LAST = false: the tracks' predicted boxes, A minus the TCM term on the linear confidence) and OCR (LAST = true: the
// tracks' last observations, A alone) share a shape: rows rd[r] x the unmatched tracks m.ut[k]; solved only when some entry exceeds the
// threshold; a pair is kept when its entry >= the threshold.  A kept pair sets m.mdet of the track and, with `mark`, m.used.
template <bool LAST>
__device__ inline void hy_second(int nR, const int* rd, const int* mark, int nU, const SSHyDev& o, double* spill, HyLds& m, int* err)
{
    const int tid = threadIdx.x;
    if (nR == 0 || nU == 0) return;                                // uniform
    const bool glb = nR * nU > SS_OC_COST_CAP;
    double* cost = glb ? spill : m.cost;
    if (tid == 0) m.any = 0;
    __syncthreads();
    auto entry = [&](int r, int k) {
        const int p = m.ut[k];
        const double* db = m.dbox[rd[r]];
        if (LAST) {
            const int slot = m.trk[p];
            if (!m.hasobs[slot]) return 0.0;
            const double t[4] = {(double)m.lobs[slot][0], (double)m.lobs[slot][1], (double)m.lobs[slot][2], (double)m.lobs[slot][3]};
            return hy_assoc(db, t, o.hmiou != 0);
        }
        return hy_assoc(db, m.pbox[p], o.hmiou != 0) - fabs((double)m.dsc[rd[r]] - m.clin[p]) * o.tcm_byte;
    };
    for (int e = tid; e < nR * nU; e += 256) {
        const int r = e / nU, k = e - r * nU;
        const double b = entry(r, k);
        cost[lsap_cidx(r, k, nR, nU)] = -b;
        if (b > o.iou_thr) m.any = 1;
    }
    __syncthreads();
    if (!m.any) return;                                            // uniform: read after the barrier, written before it
    hy_assign(nR, nU, cost, glb, m, err);
    if (tid < nR) {
        const int k = m.asg[tid];
        if (k >= 0 && !(entry(tid, k) < o.iou_thr)) {
            m.mdet[m.ut[k]] = rd[tid];
            if (mark) m.used[mark[tid]] = 1;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_hybrid_group(SSHyDev o, int F, const float* __restrict__ dets, const int* __restrict__ ndets,
                                                      float* __restrict__ out, int* __restrict__ nout)
{
    __shared__ HyLds m;
    const int s = blockIdx.x, tid = threadIdx.x, S = o.S, D = o.delta_t;
    const bool hm = o.hmiou != 0;
    const size_t sb = (size_t)s * SS_MAXT;
    double* spill = o.spill + (size_t)s * SS_MAXT * SS_MAXD;
    int* err = o.err + s;
    // ---- the stream's table into LDS ----
    m.id[tid] = o.tid[sb + tid]; m.age[tid] = o.age[sb + tid]; m.tsu[tid] = o.tsu[sb + tid]; m.streak[tid] = o.streak[sb + tid];
    m.hasobs[tid] = o.hasobs[sb + tid]; m.det[tid] = o.det[sb + tid]; m.score[tid] = o.score[sb + tid]; m.cls[tid] = o.cls[sb + tid];
    m.hasprev[tid] = o.hasprev[sb + tid]; m.cprev[tid] = o.cprev[sb + tid];
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
        // ---- 2. predict every track (thread = list position), its two confidences ----
        if (tid < nT) {
            const int slot = m.trk[tid];
            const size_t g = sb + slot;
            double q[SS_HY_FLT];
#pragma unroll
            for (int i = 0; i < SS_HY_FLT; ++i) q[i] = o.flt[g * SS_HY_FLT + i];
            if (q[13] + q[12] <= 0.0) q[13] = 0.0;
            hy_predict(q);
#pragma unroll
            for (int i = 0; i < SS_HY_FLT; ++i) o.flt[g * SS_HY_FLT + i] = q[i];
            const int age = m.age[slot] + 1;
            m.age[slot] = age;
            if (m.tsu[slot] > 0) m.streak[slot] = 0;
            m.tsu[slot] += 1;
            const double w = sqrt(q[12] * q[24]), h = q[12] / w;
            double* pb = m.pbox[tid];
            pb[0] = q[0] - w / 2.0; pb[1] = q[6] - h / 2.0; pb[2] = q[0] + w / 2.0; pb[3] = q[6] + h / 2.0;
            const bool ok = isfinite(pb[0]) && isfinite(pb[1]) && isfinite(pb[2]) && isfinite(pb[3]) && isfinite(q[18]);
            m.mdet[tid] = ok ? -1 : SS_OC_DEAD;
            m.ckal[tid] = hy_clip(q[18], o.det_thr64, 1.0);
            const double conf = (double)m.score[slot];
            m.clin[tid] = hy_clip(m.hasprev[slot] ? conf + (conf - (double)m.cprev[slot]) : conf, o.low_thr64, o.det_thr64);
            // the observation delta_t ages back, else the nearest later one, else the last
            float k0 = 0.0f, k1 = 0.0f, k2 = 0.0f, k3 = 0.0f;
            if (m.hasobs[slot]) {
                k0 = m.lobs[slot][0]; k1 = m.lobs[slot][1]; k2 = m.lobs[slot][2]; k3 = m.lobs[slot][3];
                for (int dt = D; dt >= 1; --dt) {
                    const int a = age - dt;
                    if (a < 0) continue;
                    const int e = a % D;
                    if (o.rage[g * SS_OC_MAXDT + e] == a) {
                        const float* r = o.ring + (g * SS_OC_MAXDT + e) * 4;
                        k0 = r[0]; k1 = r[1]; k2 = r[2]; k3 = r[3];
                        break;
                    }
                }
            }
            m.kobs[tid][0] = k0; m.kobs[tid][1] = k1; m.kobs[tid][2] = k2; m.kobs[tid][3] = k3;
#pragma unroll
            for (int i = 0; i < 8; ++i) m.vel[tid][i] = o.vel[g * 8 + i];
        }
        __syncthreads();
        // ---- 3. first association: high rows x all tracks, -((A + the corners' direction term) - the TCM term) ----
        if (nHi > 0 && nT > 0) {
            const bool glb = nHi * nT > SS_OC_COST_CAP;
            double* cost = glb ? spill : m.cost;
            for (int e = tid; e < nHi * nT; e += 256) {
                const int r = e / nT, k = e - r * nT, d = m.hi[r];
                const bool live = m.mdet[k] != SS_OC_DEAD;
                const double* db = m.dbox[d];
                const double sc = (double)m.dsc[d];
                const double a = live ? hy_assoc(db, m.pbox[k], hm) : 0.0;
                double term = 0.0;
                if (live && m.hasobs[m.trk[k]]) {
                    const double kb[4] = {(double)m.kobs[k][0], (double)m.kobs[k][1], (double)m.kobs[k][2], (double)m.kobs[k][3]};
                    double sum = 0.0;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {                              // lt, rt, lb, rb: the order of the sum (H-05)
                        double x0, y0, x1, y1;
                        hy_corner(kb, c, x0, y0); hy_corner(db, c, x1, y1);
                        const double dx = x1 - x0, dy = y1 - y0;
                        const double n = sqrt(dx * dx + dy * dy) + 1e-6;
                        double cs = m.vel[k][2 * c] * (dx / n) + m.vel[k][2 * c + 1] * (dy / n);
                        cs = cs < -1.0 ? -1.0 : (cs > 1.0 ? 1.0 : cs);
                        sum = sum + ss_asin(cs);
                    }
                    term = sum / 3.141592653589793;
                    term = term * o.inertia;
                    term = term * sc;
                }
                const double tcm = live ? fabs(sc - m.ckal[k]) * o.tcm_first : 0.0;
                cost[lsap_cidx(r, k, nHi, nT)] = -((a + term) - tcm);
                if (a > o.iou_thr) {
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
                hy_assign(nHi, nT, cost, glb, m, err);
            }
            if (tid < nHi) {
                const int k = m.asg[tid];
                if (k >= 0 && m.mdet[k] != SS_OC_DEAD && !(hy_assoc(m.dbox[m.hi[tid]], m.pbox[k], hm) < o.iou_thr)) {
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
            hy_second<false>(nLo, m.lo, nullptr, nU, o, spill, m, err);
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
            hy_second<true>(nD, m.ud, m.cand, nU, o, spill, m, err);
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
        // ---- 7. updates (thread = list position): velocities, observation, confidences, counters, the filter with ORU; a miss freezes ----
        if (tid < nT) {
            const int slot = m.trk[tid], d = m.mdet[tid];
            const size_t g = sb + slot;
            if (d >= 0) {
                const double* db = m.dbox[d];
                const double sc2 = (double)m.dsc[d];
                const int age = m.age[slot], gap = m.tsu[slot];
                double z1[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, z2[5];
                if (m.hasobs[slot]) {
                    const double lb[4] = {(double)m.lobs[slot][0], (double)m.lobs[slot][1], (double)m.lobs[slot][2], (double)m.lobs[slot][3]};
                    double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                    int found = 0;
                    for (int dt = D; dt >= 1; --dt) {                         // H-06: the sum over the stored observations, oldest first
                        const int a = age - dt;
                        if (a < 0) continue;
                        const int e = a % D;
                        if (o.rage[g * SS_OC_MAXDT + e] != a) continue;
                        const float* r = o.ring + (g * SS_OC_MAXDT + e) * 4;
                        const double pb[4] = {(double)r[0], (double)r[1], (double)r[2], (double)r[3]};
                        ++found;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            double x0, y0, x1, y1;
                            hy_corner(pb, c, x0, y0); hy_corner(db, c, x1, y1);
                            const double dx = x1 - x0, dy = y1 - y0;
                            const double n = sqrt(dx * dx + dy * dy) + 1e-6;
                            v[2 * c] = v[2 * c] + dx / n; v[2 * c + 1] = v[2 * c + 1] + dy / n;
                        }
                    }
                    if (!found) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            double x0, y0, x1, y1;
                            hy_corner(lb, c, x0, y0); hy_corner(db, c, x1, y1);
                            const double dx = x1 - x0, dy = y1 - y0;
                            const double n = sqrt(dx * dx + dy * dy) + 1e-6;
                            v[2 * c] = dx / n; v[2 * c + 1] = dy / n;
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) o.vel[g * 8 + i] = v[i];
                    hy_box_to_z(lb, (double)m.score[slot], z1);
                }
                hy_box_to_z(db, sc2, z2);
                const int e = age % D;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = (float)db[i];                  // exact: the row's float32 value
                    m.lobs[slot][i] = v;
                    o.ring[(g * SS_OC_MAXDT + e) * 4 + i] = v;
                }
                o.rage[g * SS_OC_MAXDT + e] = age;
                m.hasobs[slot] = 1; m.tsu[slot] = 0; m.streak[slot] += 1;
                o.hits[g] += 1;
                m.cprev[slot] = m.score[slot]; m.hasprev[slot] = 1;            // H-07
                m.score[slot] = m.dsc[d]; m.cls[slot] = m.dcls[d]; m.det[slot] = d;
                const bool frozen = o.frozen[g] != 0;
                const double* src = frozen ? o.fltf : o.flt;
                double q[SS_HY_FLT];
#pragma unroll
                for (int i = 0; i < SS_HY_FLT; ++i) q[i] = src[g * SS_HY_FLT + i];
                // ORU: `gap` virtual observations on the line z1 -> z2 from the frozen filter, then the ordinary update
                const int nv = frozen ? gap : 0;
                const double w1 = sqrt(z1[2] * z1[4]), h1 = sqrt(z1[2] / z1[4]), w2 = sqrt(z2[2] * z2[4]), h2 = sqrt(z2[2] / z2[4]);
                const double gf = (double)(nv > 0 ? nv : 1);
                const double ddx = (z2[0] - z1[0]) / gf, ddy = (z2[1] - z1[1]) / gf, ddw = (w2 - w1) / gf, ddh = (h2 - h1) / gf,
                             ddc = (z2[3] - z1[3]) / gf;
                for (int j = 0; j <= nv; ++j) {
                    double z[5];
                    if (j < nv) {
                        const double fi = (double)(j + 1);
                        const double vw = w1 + fi * ddw, vh = h1 + fi * ddh;
                        z[0] = z1[0] + fi * ddx; z[1] = z1[1] + fi * ddy; z[2] = vw * vh; z[3] = z1[3] + fi * ddc; z[4] = vw / vh;
                    } else {
#pragma unroll
                        for (int i = 0; i < 5; ++i) z[i] = z2[i];
                    }
                    hy_update(q, z);
                    if (j + 1 < nv) hy_predict(q);
                }
#pragma unroll
                for (int i = 0; i < SS_HY_FLT; ++i) o.flt[g * SS_HY_FLT + i] = q[i];
                o.frozen[g] = 0; o.obsd[g] = 1;
            } else if (o.obsd[g]) {                                // the first miss after an observation freezes the filter
#pragma unroll
                for (int i = 0; i < SS_HY_FLT; ++i) o.fltf[g * SS_HY_FLT + i] = o.flt[g * SS_HY_FLT + i];
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
                double z[5];
                hy_box_to_z(m.dbox[d], (double)m.dsc[d], z);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    double* q = o.flt + g * SS_HY_FLT + i * 6;
                    q[0] = z[i]; q[1] = 0.0; q[2] = 10.0; q[3] = 0.0; q[4] = 0.0; q[5] = 1e4;
                }
                o.flt[g * SS_HY_FLT + 24] = z[4]; o.flt[g * SS_HY_FLT + 25] = 10.0;
                for (int i = 0; i < SS_OC_MAXDT; ++i) o.rage[g * SS_OC_MAXDT + i] = -1;
#pragma unroll
                for (int i = 0; i < 8; ++i) o.vel[g * 8 + i] = 0.0;
                o.frozen[g] = 0; o.obsd[g] = 0; o.hits[g] = 0;
                m.id[slot] = m.next_id + rank;
                m.age[slot] = 0; m.tsu[slot] = 0; m.streak[slot] = 0; m.hasobs[slot] = 0;   // O-06: the birth row is shown, not observed
                m.hasprev[slot] = 0; m.cprev[slot] = 0.0f;
#pragma unroll
                for (int i = 0; i < 4; ++i) m.lobs[slot][i] = (float)m.dbox[d][i];
                m.score[slot] = m.dsc[d]; m.cls[slot] = m.dcls[d]; m.det[slot] = d;
            }
        }
        __syncthreads();
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
    o.hasprev[sb + tid] = m.hasprev[tid]; o.cprev[sb + tid] = m.cprev[tid];
#pragma unroll
    for (int i = 0; i < 4; ++i) o.lobs[(sb + tid) * 4 + i] = m.lobs[tid][i];
    o.trk[sb + tid] = m.trk[tid];
    if (tid == 0) { o.n_trk[s] = m.n_trk; o.frame[s] = m.frame; o.next_id[s] = m.next_id; }
}

void ss_launch_hybrid_group(const SSHyDev& o, int F, const float* dets, const int* ndets, float* out, int* nout, hipStream_t st)
{
    hipLaunchKernelGGL(k_hybrid_group, dim3(o.S), dim3(256), 0, st, o, F, dets, ndets, out, nout);
}

// ---- host side: the state of a context ------------------------------------------------------------------------------------------------
struct SSHybrid {
    SSHyDev dev;
    SsBuf<SS_DEVICE> buf;               // every table of dev
};

void ss_hybrid_free(SSHybrid* h) { delete h; }
const SSHyDev& ss_hybrid_dev(const SSHybrid* h) { return h->dev; }

int ss_hybrid_pending_impl(SSHybrid* h, hipStream_t st, std::string& err)
{
    return h ? ss_tracker_pending_impl(h->dev.err, h->dev.S, st, "Hybrid-SORT tracker", err) : (int)SS_OK;
}

// the streams' lists, counters and error words restart; synchronises
int ss_hybrid_reset_impl(SSHybrid* h, hipStream_t st, int stream, std::string& err)
{
    const SSHyDev& o = h->dev;
    const char* who = "ss_hybridsort_reset: ";
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? o.S : stream + 1;
    const std::vector<int> ones(o.S, 1);
    SS_HIPCHK(who, hipMemsetAsync(o.frame + s0, 0, (s1 - s0) * 4, st));
    SS_HIPCHK(who, hipMemsetAsync(o.err + s0, 0, (s1 - s0) * 4, st));
    SS_HIPCHK(who, hipMemsetAsync(o.n_trk + s0, 0, (s1 - s0) * 4, st));
    SS_HIPCHK(who, hipMemcpyAsync(o.next_id + s0, ones.data(), (s1 - s0) * 4, hipMemcpyHostToDevice, st));
    SS_HIPCHK(who, hipStreamSynchronize(st));
    return SS_OK;
}

int ss_hybrid_create_check_impl(const ss_hybridsort_config* cfg, std::string& err)
{
    if (!cfg) { err = "ss_hybridsort_create: null argument"; return SS_ERR_INVALID; }
    if (cfg->max_tracks < 1 || cfg->max_tracks > SS_MAXT || cfg->max_dets < 1 || cfg->max_dets > SS_MAXD || cfg->delta_t < 1 ||
        cfg->delta_t > SS_OC_MAXDT || cfg->max_age < 1 || cfg->min_hits < 0 || !(cfg->iou_threshold > 0.0 && cfg->iou_threshold <= 1.0) ||
        !(cfg->inertia >= 0.0) || !(cfg->tcm_first_weight >= 0.0) || !(cfg->tcm_byte_weight >= 0.0) || !(cfg->low_thresh <= cfg->det_thresh) ||
        (cfg->use_byte != 0 && cfg->use_byte != 1) || (cfg->hmiou != 0 && cfg->hmiou != 1)) {
        err = "ss_hybridsort_create: 1 <= max_tracks <= 256, 1 <= max_dets <= 128, 1 <= delta_t <= 8, max_age >= 1, min_hits >= 0, "
              "0 < iou_threshold <= 1, inertia >= 0, tcm weights >= 0, low_thresh <= det_thresh, use_byte and hmiou 0 / 1";
        return SS_ERR_INVALID;
    }
    return SS_OK;
}

// the caller has drained the stream and freed the state this one replaces: a failure leaves none attached
int ss_hybrid_create_impl(SSHybrid** ph, hipStream_t st, int S_, const ss_hybridsort_config* cfg, std::string& err)
{
    std::unique_ptr<SSHybrid> H(new SSHybrid());
    SSHyDev& o = H->dev;
    memset(&o, 0, sizeof o);
    o.S = S_;
    o.max_age = cfg->max_age; o.min_hits = cfg->min_hits; o.delta_t = cfg->delta_t; o.use_byte = cfg->use_byte; o.hmiou = cfg->hmiou;
    o.max_tracks = cfg->max_tracks; o.max_dets = cfg->max_dets;
    o.det_thresh = (float)cfg->det_thresh; o.low_thresh = (float)cfg->low_thresh;
    o.det_thr64 = cfg->det_thresh; o.low_thr64 = cfg->low_thresh;
    o.iou_thr = cfg->iou_threshold; o.inertia = cfg->inertia; o.tcm_first = cfg->tcm_first_weight; o.tcm_byte = cfg->tcm_byte_weight;
    const size_t S = o.S, T = SS_MAXT;
    SsCarve c;
    c.add(&o.frame, S); c.add(&o.next_id, S); c.add(&o.err, S); c.add(&o.n_trk, S);
    c.add(&o.trk, S * T);
    c.add(&o.tid, S * T); c.add(&o.age, S * T); c.add(&o.tsu, S * T); c.add(&o.hits, S * T); c.add(&o.streak, S * T); c.add(&o.hasobs, S * T);
    c.add(&o.obsd, S * T); c.add(&o.frozen, S * T); c.add(&o.det, S * T); c.add(&o.hasprev, S * T);
    c.add(&o.score, S * T); c.add(&o.cls, S * T); c.add(&o.cprev, S * T); c.add(&o.lobs, S * T * 4);
    c.add(&o.ring, S * T * SS_OC_MAXDT * 4); c.add(&o.rage, S * T * SS_OC_MAXDT); c.add(&o.vel, S * T * 8);
    c.add(&o.flt, S * T * SS_HY_FLT); c.add(&o.fltf, S * T * SS_HY_FLT); c.add(&o.spill, S * T * SS_MAXD);
    SS_HIPCHK("ss_hybridsort_create: ", c.carve(H->buf, st));
    if (const int rc = ss_hybrid_reset_impl(H.get(), st, -1, err)) return rc;
    *ph = H.release();
    return SS_OK;
}

// Synchronous: the table of one stream in list order; the filter's components are laid out as upstream's x[9] and dense P[81]
int ss_hybrid_get_tracks_impl(SSHybrid* h, hipStream_t st, int s, int cap, int* n_tracks, int* next_id, int* frame_count, int* track_id,
                              int* age, int* time_since_update, int* hits, int* hit_streak, int* frozen, double* x, double* P,
                              float* last_obs, double* velocity, float* conf, float* conf_prev, std::string& err)
{
    const SSHyDev& o = h->dev;
    const std::string who = "ss_hybridsort_get_tracks: ";
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
    std::vector<int> trk(T), flag(nt);
    SS_HIPCHK(who, hipMemcpy(trk.data(), o.trk + sb, T * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < nt; ++i)
        if (trk[i] < 0 || trk[i] >= SS_MAXT) { err = who + "corrupt list"; return SS_ERR_CAPACITY; }
    const int* const isrc[6] = {o.tid, o.age, o.tsu, o.hits, o.streak, o.frozen};
    int* const idst[6] = {track_id, age, time_since_update, hits, hit_streak, frozen};
    for (int k = 0; k < 6; ++k) SS_HIPCHK(who, ss_gather_device(trk.data(), nt, isrc[k] + sb, T, 1, idst[k]));
    if (x || P) {
        std::vector<double> q((size_t)nt * SS_HY_FLT);
        SS_HIPCHK(who, ss_gather_device(trk.data(), nt, o.flt + sb * SS_HY_FLT, T, SS_HY_FLT, q.data()));
        for (int i = 0; i < nt; ++i) {
            const double* f = q.data() + (size_t)i * SS_HY_FLT;
            if (x) {
                double* xi = x + (size_t)i * 9;
                for (int c = 0; c < 4; ++c) { xi[c] = f[c * 6]; xi[5 + c] = f[c * 6 + 1]; }
                xi[4] = f[24];
            }
            if (P) {
                double* Pi = P + (size_t)i * 81;
                for (int k = 0; k < 81; ++k) Pi[k] = 0.0;
                for (int c = 0; c < 4; ++c) {
                    Pi[c * 9 + c] = f[c * 6 + 2]; Pi[c * 9 + 5 + c] = f[c * 6 + 3];
                    Pi[(5 + c) * 9 + c] = f[c * 6 + 4]; Pi[(5 + c) * 9 + 5 + c] = f[c * 6 + 5];
                }
                Pi[4 * 9 + 4] = f[25];
            }
        }
    }
    SS_HIPCHK(who, ss_gather_device(trk.data(), nt, o.vel + sb * 8, T, 8, velocity));
    SS_HIPCHK(who, ss_gather_device(trk.data(), nt, o.score + sb, T, 1, conf));
    SS_HIPCHK(who, ss_gather_device(trk.data(), nt, o.cprev + sb, T, 1, conf_prev));
    if (conf_prev) SS_HIPCHK(who, ss_gather_device(trk.data(), nt, o.hasprev + sb, T, 1, flag.data()));
    for (int i = 0; conf_prev && i < nt; ++i)                        // a track matched less than twice: -1
        if (!flag[i]) conf_prev[i] = -1.0f;
    SS_HIPCHK(who, ss_gather_device(trk.data(), nt, o.lobs + sb * 4, T, 4, last_obs));
    if (last_obs) SS_HIPCHK(who, ss_gather_device(trk.data(), nt, o.hasobs + sb, T, 1, flag.data()));
    for (int i = 0; last_obs && i < nt; ++i)                         // a track without an observation: -1
        if (!flag[i]) for (int k = 0; k < 4; ++k) last_obs[i * 4 + k] = -1.0f;
    return SS_OK;
}
