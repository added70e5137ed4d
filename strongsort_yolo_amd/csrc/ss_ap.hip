// ss_ap.hip — scoring detections against ground truth (docs/DETEVAL.md): COCO's precision [T,R,K,A,M] and recall [T,K,A,M] arrays
// for boxes (IoU) or oriented boxes (ProbIoU).  Every float is a fixed elementwise f64 expression and every sum an integer sum, in
// the order of docs/DETEVAL.md §1, which tests/deteval_ref.py restates; the file is built with -ffp-contract=off.
//
//   k_ap_sort_local  one workgroup per 256 detections of a class: the stable order by descending score inside the chunk, by counting
//                    in LDS (a detection's place is the number of chunk members that come before it).
//   k_ap_sort_merge  one launch per pass, runs of w detections of a class merged in pairs: an element's place is its index in its
//                    own run plus the number of the sibling run's elements that come before it (a binary search).  Runs are
//                    contiguous ranges of the packed order, so "before" needs no index compare: the earlier run wins ties.
//   k_ap_rank        rank[packed detection] = its place in its class.
//   k_ap_match       one wave per (image, class) cell: the cell's ground truth in LDS, its detections walked serially in position
//                    order with the lanes over the ground-truth rows; two bits per (area range, threshold, kept detection).
//   k_ap_accum       one workgroup per (class, area range, max_dets entry): integer counts forward, then a backward walk over the
//                    class's order that carries the suffix counts and the running maximum of the precision and drops it at the
//                    recall thresholds.
// The kernel boundary is the only synchronisation between workgroups; no workgroup reads what another one of its launch writes.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "ss_common.h"
#include "ss_host.h"
#include "ss_launch.h"
#include "ss_lsap.h"
#include "ss_mot_sim.h"
#include "ss_probiou.h"

#define AP_MAX_GTS 1024                     // ground-truth rows a cell: the rows k_ap_match keeps in LDS
#define AP_MAX_CELL_DETS 4096               // detections a cell before the cut
#define AP_MAX_KEEP 1024                    // max_dets[-1]
#define AP_MAX_DETS (1 << 22)               // detections a call
#define AP_MAX_THRS 16                      // two bits each in a 32-bit record word
#define AP_MAX_AREAS 8
#define AP_MAX_MAXDETS 4
#define AP_MAX_RECS 1024                    // recall thresholds: k_ap_accum's LDS row
#define AP_MAX_RECORD (1ll << 28)           // entries of the match record when the caller asks for it
#define AP_EPS 0x1p-52
#define AP_CHUNK 256

struct ApArgs {
    // upload image
    const double *gt_box, *dt_box;          // [rows][W]
    const double* score;                    // [N]
    const int* gt_crowd;                    // [ground-truth rows]
    const int *cell_gt, *cell_dt;           // [cells + 1]
    const int *cls_cell, *cls_dt;           // [K + 1] first cell / first detection of a class
    const int* kept_off;                    // [cells + 1] first kept detection of a cell
    const int2* blk;                        // k_ap_sort_local's chunks: {first detection, count}
    const double *thr, *rthr, *area;        // [T], [R], [A][2]
    const int* maxdet;                      // [Mn]
    // work
    unsigned long long* key[2];             // [N] ping-pong
    unsigned* idx[2];                       // [N] packed detection index
    int *dpos, *dslot;                      // [N] position in the cell; kept index or -1
    // download image
    double *prec, *recall;
    int* rank;                              // [N]
    unsigned* rec;                          // [A][kept]: bit 2t matched, bit 2t + 1 ignored
    int* midx;                              // [A][T][kept] or NULL
    int N, K, T, R, A, Mn, W, nkept, fin;   // fin: which of key / idx holds the final order
    int ngc, ndc, keepc;                    // k_ap_match's LDS capacities: ground-truth rows (a multiple of 64), detections, kept
};

// descending score as a rising unsigned key; -0.0 and 0.0 tie
__device__ __forceinline__ unsigned long long ap_key(double s)
{
    unsigned long long u = (unsigned long long)__double_as_longlong(s);
    if ((u << 1) == 0ull) u = 0ull;
    u = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    return ~u;
}

// the class k with cls_dt[k] <= e < cls_dt[k + 1]
__device__ __forceinline__ int ap_class_of(const int* __restrict__ cls_dt, int K, int e)
{
    int lo = 0, hi = K;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cls_dt[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(AP_CHUNK) void k_ap_sort_local(const ApArgs a)
{
    __shared__ unsigned long long sk[AP_CHUNK];
    const int tid = threadIdx.x;
    const int2 b = a.blk[blockIdx.x];
    unsigned long long key = 0ull;
    if (tid < b.y) { key = ap_key(a.score[b.x + tid]); sk[tid] = key; }
    __syncthreads();
    if (tid >= b.y) return;
    int c = 0;
    for (int u = 0; u < b.y; ++u) {
        const unsigned long long o = sk[u];
        c += (o < key || (o == key && u < tid)) ? 1 : 0;
    }
    a.key[0][b.x + c] = key;
    a.idx[0][b.x + c] = (unsigned)(b.x + tid);
}

// src -> 1 - src, runs of w merged into runs of 2w inside every class
__global__ __launch_bounds__(256) void k_ap_sort_merge(const ApArgs a, int src, int w)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.N) return;
    const unsigned long long* __restrict__ ki = a.key[src];
    const unsigned* __restrict__ ii = a.idx[src];
    const int k = ap_class_of(a.cls_dt, a.K, e);
    const int s0 = a.cls_dt[k], n = a.cls_dt[k + 1] - s0, j = e - s0;
    const unsigned long long key = ki[e];
    int pos = j;
    if (n > w) {
        const int base = (j / (2 * w)) * (2 * w), mid = min(base + w, n), end = min(base + 2 * w, n);
        const bool first = j < mid;
        int lo = first ? mid : base, hi = first ? end : mid;        // the sibling run
        const int from = lo;
        while (lo < hi) {                                           // first: keys < key; second: keys <= key
            const int m = (lo + hi) >> 1;
            const unsigned long long o = ki[s0 + m];
            if (first ? o < key : o <= key) lo = m + 1; else hi = m;
        }
        pos = first ? j + (lo - from) : base + (j - mid) + (lo - from);
    }
    a.key[1 - src][s0 + pos] = key;
    a.idx[1 - src][s0 + pos] = ii[e];
}

__global__ __launch_bounds__(256) void k_ap_rank(const ApArgs a)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.N) return;
    const int k = ap_class_of(a.cls_dt, a.K, e);
    a.rank[a.idx[a.fin][e]] = e - a.cls_dt[k];
}

// similarity against a crowd region: the overlap over the detection's own area (the steps of mot_sim)
__device__ __forceinline__ double ap_sim_crowd(const double* __restrict__ D, const double* __restrict__ G)
{
    const double ax1 = D[0], ay1 = D[1], ax2 = D[2], ay2 = D[3], bx1 = G[0], by1 = G[1], bx2 = G[2], by2 = G[3];
    const double w = fmax(0.0, fmin(ax2, bx2) - fmax(ax1, bx1)), h = fmax(0.0, fmin(ay2, by2) - fmax(ay1, by1));
    const double inter = w * h;
    return inter / ((ax2 - ax1) * (ay2 - ay1));
}

// One wave per cell.  Dynamic LDS: the ground-truth boxes (or ProbIoU terms), their areas, the current detection's similarities,
// the matched bits per (area range, threshold), the cell's ranks, the kept detections by position, the crowd flags.
__global__ __launch_bounds__(64) void k_ap_match(const ApArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ap_lds[];
    const int c = blockIdx.x, lane = threadIdx.x;
    const int g0 = a.cell_gt[c], ng = a.cell_gt[c + 1] - g0, d0 = a.cell_dt[c], nd = a.cell_dt[c + 1] - d0;
    if (nd <= 0) return;
    const bool obb = a.W == 5;
    const int GW = obb ? 6 : 4, nqc = a.ngc >> 6, nq = (ng + 63) >> 6, T = a.T, A = a.A;
    double* gbox = (double*)ap_lds;
    double* garea = gbox + (size_t)a.ngc * GW;
    double* sim = garea + a.ngc;
    unsigned long long* matched = (unsigned long long*)(sim + a.ngc);
    int* ranks = (int*)(matched + (size_t)A * T * nqc);
    int* kept = ranks + a.ndc;
    unsigned char* crowd = (unsigned char*)(kept + a.keepc);
    for (int g = lane; g < ng; g += 64) {
        const double* __restrict__ b = a.gt_box + (size_t)(g0 + g) * a.W;
        if (obb) {
            const ss_pbox p = ss_probiou_box((float)b[0], (float)b[1], (float)b[2], (float)b[3], (float)b[4]);
            double* o = gbox + (size_t)g * 6;
            o[0] = p.x; o[1] = p.y; o[2] = p.A; o[3] = p.B; o[4] = p.C; o[5] = p.D;
            garea[g] = b[2] * b[3];
        } else {
            double* o = gbox + (size_t)g * 4;
            o[0] = b[0]; o[1] = b[1]; o[2] = b[2]; o[3] = b[3];
            garea[g] = (b[2] - b[0]) * (b[3] - b[1]);
        }
        crowd[g] = a.gt_crowd[g0 + g] ? 1 : 0;
    }
    for (int i = lane; i < A * T * nqc; i += 64) matched[i] = 0ull;
    for (int j = lane; j < nd; j += 64) ranks[j] = a.rank[d0 + j];
    __syncthreads();
    const int keep_max = a.maxdet[a.Mn - 1], k0 = a.kept_off[c];
    for (int j = lane; j < nd; j += 64) {
        const int r = ranks[j];
        int p = 0;
        for (int u = 0; u < nd; ++u) p += ranks[u] < r ? 1 : 0;
        a.dpos[d0 + j] = p;
        a.dslot[d0 + j] = p < keep_max ? k0 + p : -1;
        if (p < keep_max) kept[p] = j;
    }
    __syncthreads();
    const int nk = min(nd, keep_max);
    for (int p = 0; p < nk; ++p) {
        const double* __restrict__ db = a.dt_box + (size_t)(d0 + kept[p]) * a.W;
        double darea;
        if (obb) {
            const ss_pbox dp = ss_probiou_box((float)db[0], (float)db[1], (float)db[2], (float)db[3], (float)db[4]);
            darea = db[2] * db[3];
            for (int g = lane; g < ng; g += 64) {
                const double* o = gbox + (size_t)g * 6;
                ss_pbox q;
                q.x = o[0]; q.y = o[1]; q.A = o[2]; q.B = o[3]; q.C = o[4]; q.D = o[5];
                sim[g] = ss_probiou_pair(dp, q);
            }
        } else {
            const double d4[4] = { db[0], db[1], db[2], db[3] };
            darea = (d4[2] - d4[0]) * (d4[3] - d4[1]);
            for (int g = lane; g < ng; g += 64) sim[g] = crowd[g] ? ap_sim_crowd(d4, gbox + (size_t)g * 4) : mot_sim(d4, gbox + (size_t)g * 4);
        }
        for (int ai = 0; ai < A; ++ai) {
            const double lo = a.area[2 * ai], hi = a.area[2 * ai + 1];
            const bool dout = darea < lo || darea > hi;
            unsigned word = 0u;
            for (int t = 0; t < T; ++t) {
                const double lim = fmin(a.thr[t], 1.0 - 1e-10);
                unsigned long long* mw = matched + (size_t)(ai * T + t) * nqc;
                int m = -1, mig = 0;
                for (int ph = 0; ph < 2 && m < 0; ++ph) {               // the not-ignored rows are tried before the ignored ones
                    unsigned long long key = 0ull;
                    int bg = -1;
                    for (int q = 0; q < nq; ++q) {
                        const int g = lane + 64 * q;
                        if (g >= ng) break;
                        const bool cr = crowd[g] != 0;
                        const bool gi = cr || garea[g] < lo || garea[g] > hi;
                        const bool taken = (mw[q] >> lane) & 1ull;
                        const double s = sim[g];
                        const bool cand = (ph == 0 ? (!gi && !taken) : (gi && (cr || !taken))) && s >= lim;
                        const unsigned long long bits = (unsigned long long)__double_as_longlong(s);
                        if (cand && bits >= key) { key = bits; bg = g; }                // among equal similarities the later row wins
                    }
                    const unsigned long long best = ~wave_min_u64(~key);
                    if (best != 0ull) {
                        m = wave_minmax_i32<true>(key == best ? bg : -1);
                        mig = ph;
                    }
                }
                if (m >= 0) {
                    word |= (1u | (mig ? 2u : 0u)) << (2 * t);
                    if (lane == (m & 63)) mw[m >> 6] |= 1ull << (m & 63);
                } else if (dout) word |= 2u << (2 * t);
                if (a.midx && lane == 0) a.midx[(size_t)(ai * T + t) * a.nkept + k0 + p] = m;
                __syncthreads();
            }
            if (lane == 0) a.rec[(size_t)ai * a.nkept + k0 + p] = word;
        }
    }
}

// inclusive running maximum over the workgroup in thread order; wm: LDS[4]; -> the value at this thread, the workgroup's maximum
__device__ inline void block_scan_max256(double v, double* wm, double& incl, double& total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const double t = __shfl_up(inc, off); if (lane >= off) inc = fmax(inc, t); }
    __syncthreads();
    if (lane == 63) wm[w] = inc;
    __syncthreads();
    double tot = wm[0];
#pragma unroll
    for (int i = 0; i < 4; ++i) { const double c = wm[i]; if (i < w) inc = fmax(inc, c); tot = fmax(tot, c); }
    incl = inc;
    total = tot;
}

// bit 0: counts as a true positive, bit 1: as a false positive, bit 2: is in the list (position < M)
__device__ __forceinline__ int ap_flags(const ApArgs& a, const unsigned* __restrict__ order, int i, int ai, int t, int M)
{
    const unsigned d = order[i];
    if (a.dpos[d] >= M) return 0;
    const unsigned w = a.rec[(size_t)ai * a.nkept + a.dslot[d]] >> (2 * t);
    const int m = w & 1u, ig = (w >> 1) & 1u;
    return 4 | ((m && !ig) ? 1 : 0) | ((!m && !ig) ? 2 : 0);
}

__global__ __launch_bounds__(256) void k_ap_accum(const ApArgs a)
{
    __shared__ int wtot[4];
    __shared__ double wmax[4];
    __shared__ double pres[AP_MAX_RECS];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int mi = b % a.Mn; b /= a.Mn;
    const int ai = b % a.A, k = b / a.A;
    const int M = a.maxdet[mi], R = a.R;
    const double lo = a.area[2 * ai], hi = a.area[2 * ai + 1];
    const int s0 = a.cls_dt[k], n = a.cls_dt[k + 1] - s0;
    const int g0 = a.cell_gt[a.cls_cell[k]], g1 = a.cell_gt[a.cls_cell[k + 1]];
    int cnt = 0;
    for (int g = g0 + tid; g < g1; g += 256) {
        const double* __restrict__ bx = a.gt_box + (size_t)g * a.W;
        const double ar = a.W == 5 ? bx[2] * bx[3] : (bx[2] - bx[0]) * (bx[3] - bx[1]);
        cnt += (!a.gt_crowd[g] && !(ar < lo) && !(ar > hi)) ? 1 : 0;
    }
    int excl, npig;
    block_scan_sum256(cnt, wtot, excl, npig);
    const unsigned* __restrict__ order = n > 0 ? a.idx[a.fin] + s0 : nullptr;
    for (int t = 0; t < a.T; ++t) {
        double* __restrict__ out = a.prec + ((size_t)t * R * a.K + k) * a.A * a.Mn + (size_t)ai * a.Mn + mi;      // + r K A Mn
        const size_t rstride = (size_t)a.K * a.A * a.Mn;
        double* __restrict__ rout = a.recall + (((size_t)t * a.K + k) * a.A + ai) * a.Mn + mi;
        if (npig == 0) {
            for (int r = tid; r < R; r += 256) out[r * rstride] = -1.0;
            if (tid == 0) *rout = -1.0;
            continue;
        }
        int ltp = 0, lfp = 0;
        for (int i = tid; i < n; i += 256) { const int f = ap_flags(a, order, i, ai, t, M); ltp += f & 1; lfp += (f >> 1) & 1; }
        int TP, FP;
        block_scan_sum256(ltp, wtot, excl, TP);
        block_scan_sum256(lfp, wtot, excl, FP);
        for (int r = tid; r < R; r += 256) pres[r] = 0.0;
        __syncthreads();
        int ctp = 0, cfp = 0;                                           // true / false positives behind the chunk
        double cenv = -1.0;                                             // the maximum of pr behind the chunk
        for (int end = n; end > 0; end -= AP_CHUNK) {
            const int i = end - 1 - tid;                                // thread order walks the class order backwards
            const int f = i >= 0 ? ap_flags(a, order, i, ai, t, M) : 0;
            int tot;
            block_scan_sum256((f & 1) | ((f & 2) << 15), wtot, excl, tot);
            const int tp = TP - ctp - (excl & 0xffff), fp = FP - cfp - (excl >> 16);       // the inclusive counts at i
            const double pr = (f & 4) ? (double)tp / ((double)(fp + tp) + AP_EPS) : -1.0;
            double env, cmax;
            block_scan_max256(pr, wmax, env, cmax);
            env = fmax(env, cenv);
            if ((f & 4) && ((f & 1) || i == 0)) {
                const double rc = (double)tp / (double)npig;
                int r0 = 0;
                if (i != 0) {                                           // the first threshold above the recall before this detection
                    const double rp = (double)(tp - 1) / (double)npig;
                    int l = 0, h = R;
                    while (l < h) { const int m = (l + h) >> 1; if (a.rthr[m] > rp) h = m; else l = m + 1; }
                    r0 = l;
                }
                int l = r0, h = R;
                while (l < h) { const int m = (l + h) >> 1; if (a.rthr[m] > rc) h = m; else l = m + 1; }
                for (int r = r0; r < l; ++r) pres[r] = env;
            }
            cenv = fmax(cenv, cmax);
            ctp += tot & 0xffff;
            cfp += tot >> 16;
        }
        __syncthreads();
        for (int r = tid; r < R; r += 256) out[r * rstride] = pres[r];
        if (tid == 0) *rout = n > 0 ? (double)TP / (double)npig : 0.0;
        __syncthreads();
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct SSAp {
    SsBuf<SS_PINNED> host;                              // the upload image, then the download image
    SsBuf<SS_DEVICE> dev;                               // upload image | work | download image
    SsEvent ev;
    bool attr = false;
};

void ss_ap_free(SSAp* p) { delete p; }

int ss_ap_max_gts_impl() { return AP_MAX_GTS; }
int ss_ap_max_cell_dets_impl() { return AP_MAX_CELL_DETS; }
int ss_ap_max_keep_impl() { return AP_MAX_KEEP; }
int ss_ap_max_dets_impl() { return AP_MAX_DETS; }

static size_t ap_match_lds(int ngc, int ndc, int keepc, int A, int T, int GW)
{
    return (size_t)ngc * GW * 8 + (size_t)ngc * 16 + (size_t)A * T * (ngc / 64) * 8 + (size_t)ndc * 4 + (size_t)keepc * 4 + (size_t)ngc;
}

// Every refusal that needs neither a context nor the device.
int ss_ap_check_impl(int similarity, int n_classes, int n_cells, const int* class_cell_off, const int* cell_image, const int* cell_gt_off,
                     const int* cell_det_off, const double* gt_boxes, const int* gt_crowd, const double* det_boxes, const double* det_scores,
                     int n_thrs, const double* iou_thrs, int n_recs, const double* rec_thrs, int n_areas, const double* areas, int n_max_dets,
                     const int* max_dets, const double* precision, const double* recall, const int* det_rank, const int* rec_match,
                     const int* rec_ignored, std::string& err)
{
    const std::string who = "ss_ap_eval: ";
    if (!class_cell_off || !cell_image || !cell_gt_off || !cell_det_off || !gt_boxes || !gt_crowd || !det_boxes || !det_scores || !iou_thrs ||
        !rec_thrs || !areas || !max_dets || !precision || !recall) { err = who + "null argument"; return SS_ERR_INVALID; }
    if (!rec_match != !rec_ignored) { err = who + "rec_match and rec_ignored come together"; return SS_ERR_INVALID; }
    (void)det_rank;
    if (similarity != 0 && similarity != 1) { err = who + "similarity must be 0 (iou) or 1 (probiou)"; return SS_ERR_INVALID; }
    if (n_classes < 1 || n_cells < 0) { err = who + "n_classes must be at least 1 and n_cells at least 0"; return SS_ERR_INVALID; }
    if (n_thrs < 1 || n_recs < 1 || n_areas < 1 || n_max_dets < 1) { err = who + "a parameter array is empty"; return SS_ERR_INVALID; }
    if (n_thrs > AP_MAX_THRS) { err = who + std::to_string(n_thrs) + " thresholds: at most " + std::to_string(AP_MAX_THRS); return SS_ERR_CAPACITY; }
    if (n_areas > AP_MAX_AREAS) { err = who + std::to_string(n_areas) + " area ranges: at most " + std::to_string(AP_MAX_AREAS); return SS_ERR_CAPACITY; }
    if (n_max_dets > AP_MAX_MAXDETS) { err = who + std::to_string(n_max_dets) + " max_dets entries: at most " + std::to_string(AP_MAX_MAXDETS); return SS_ERR_CAPACITY; }
    if (n_recs > AP_MAX_RECS) { err = who + std::to_string(n_recs) + " recall thresholds: at most " + std::to_string(AP_MAX_RECS); return SS_ERR_CAPACITY; }
    for (int t = 0; t < n_thrs; ++t)
        if (!(iou_thrs[t] > 0.0) || !(iou_thrs[t] <= 1.0)) { err = who + "iou_thrs must be in (0, 1]"; return SS_ERR_INVALID; }
    for (int r = 0; r < n_recs; ++r)
        if (!std::isfinite(rec_thrs[r]) || (r && rec_thrs[r] < rec_thrs[r - 1])) { err = who + "rec_thrs must be finite and must not decrease"; return SS_ERR_INVALID; }
    for (int i = 0; i < n_areas; ++i)
        if (!std::isfinite(areas[2 * i]) || !std::isfinite(areas[2 * i + 1]) || areas[2 * i + 1] < areas[2 * i]) { err = who + "an area range is not finite or has hi < lo"; return SS_ERR_INVALID; }
    for (int i = 0; i < n_max_dets; ++i)
        if (max_dets[i] < 1 || (i && max_dets[i] <= max_dets[i - 1])) { err = who + "max_dets must be at least 1 and rising"; return SS_ERR_INVALID; }
    if (max_dets[n_max_dets - 1] > AP_MAX_KEEP) { err = who + "max_dets " + std::to_string(max_dets[n_max_dets - 1]) + ": at most " + std::to_string(AP_MAX_KEEP); return SS_ERR_CAPACITY; }
    if (class_cell_off[0] != 0 || cell_gt_off[0] != 0 || cell_det_off[0] != 0) { err = who + "offsets must start at 0"; return SS_ERR_INVALID; }
    for (int k = 0; k < n_classes; ++k)
        if (class_cell_off[k + 1] < class_cell_off[k] || class_cell_off[k + 1] > n_cells) { err = who + "class " + std::to_string(k) + ": cell offsets decrease or pass n_cells"; return SS_ERR_INVALID; }
    if (class_cell_off[n_classes] != n_cells) { err = who + "class_cell_off must end at n_cells"; return SS_ERR_INVALID; }
    const int W = similarity ? 5 : 4;
    long long kept = 0;
    for (int k = 0; k < n_classes; ++k)
        for (int c = class_cell_off[k]; c < class_cell_off[k + 1]; ++c) {
            const auto at = [&] { return "class " + std::to_string(k) + ": image " + std::to_string(cell_image[c]) + ": "; };     // (formed only for a refusal)
            if (cell_image[c] < 0 || (c > class_cell_off[k] && cell_image[c] <= cell_image[c - 1])) { err = who + at() + "the images of a class must be non-negative and rising"; return SS_ERR_INVALID; }
            if (cell_gt_off[c + 1] < cell_gt_off[c]) { err = who + at() + "ground-truth row offsets decrease"; return SS_ERR_INVALID; }
            if (cell_det_off[c + 1] < cell_det_off[c]) { err = who + at() + "detection offsets decrease"; return SS_ERR_INVALID; }
            const int ng = cell_gt_off[c + 1] - cell_gt_off[c], nd = cell_det_off[c + 1] - cell_det_off[c];
            if (ng > AP_MAX_GTS) { err = who + at() + std::to_string(ng) + " ground-truth rows: at most " + std::to_string(AP_MAX_GTS) + " a cell"; return SS_ERR_CAPACITY; }
            if (nd > AP_MAX_CELL_DETS) { err = who + at() + std::to_string(nd) + " detections: at most " + std::to_string(AP_MAX_CELL_DETS) + " a cell"; return SS_ERR_CAPACITY; }
            if (cell_det_off[c + 1] > AP_MAX_DETS) { err = who + at() + "more than " + std::to_string(AP_MAX_DETS) + " detections a call"; return SS_ERR_CAPACITY; }
            kept += std::min(nd, max_dets[n_max_dets - 1]);
            for (int side = 0; side < 2; ++side) {
                const int* off = side ? cell_det_off : cell_gt_off;
                const double* box = side ? det_boxes : gt_boxes;
                const char* name = side ? "detection" : "ground-truth";
                for (int r = off[c]; r < off[c + 1]; ++r) {
                    const double* b = box + (size_t)r * W;
                    bool fin = true;
                    for (int i = 0; i < W; ++i) fin = fin && std::isfinite(b[i]);
                    if (!fin) { err = who + at() + "a " + name + " box is NaN or infinite"; return SS_ERR_INVALID; }
                    if (W == 4 ? (!(b[2] > b[0]) || !(b[3] > b[1])) : (!(b[2] > 0.0) || !(b[3] > 0.0))) {
                        err = who + at() + "a " + name + (W == 4 ? " box has x2 <= x1 or y2 <= y1" : " box has w <= 0 or h <= 0"); return SS_ERR_INVALID;
                    }
                    if (side && !std::isfinite(det_scores[r])) { err = who + at() + "a score is NaN or infinite"; return SS_ERR_INVALID; }
                    if (!side && gt_crowd[r] != 0 && gt_crowd[r] != 1) { err = who + at() + "a crowd flag is neither 0 nor 1"; return SS_ERR_INVALID; }
                    if (!side && gt_crowd[r] && similarity) { err = who + at() + "a crowd region cannot be scored with probiou"; return SS_ERR_INVALID; }
                }
            }
        }
    if (rec_match && kept * n_areas * n_thrs > AP_MAX_RECORD) {
        err = who + std::to_string(kept * n_areas * n_thrs) + " record entries: at most " + std::to_string(AP_MAX_RECORD) + " a call"; return SS_ERR_CAPACITY;
    }
    return SS_OK;
}

int ss_ap_eval_impl(SSAp** pp, hipStream_t stream, int similarity, int n_classes, int n_cells, const int* class_cell_off, const int* cell_gt_off,
                    const int* cell_det_off, const double* gt_boxes, const int* gt_crowd, const double* det_boxes, const double* det_scores,
                    int n_thrs, const double* iou_thrs, int n_recs, const double* rec_thrs, int n_areas, const double* areas, int n_max_dets,
                    const int* max_dets, double* precision, double* recall, int* det_rank, int* rec_match, int* rec_ignored, std::string& err)
{
    const char* const who = "ss_ap_eval: ";
    if (!pp) { err = "ss_ap_eval: null context"; return SS_ERR_INVALID; }
    const int K = n_classes, C = n_cells, T = n_thrs, R = n_recs, A = n_areas, Mn = n_max_dets, W = similarity ? 5 : 4;
    const size_t Ng = (size_t)cell_gt_off[C], N = (size_t)cell_det_off[C];
    const int keep_max = max_dets[Mn - 1];
    // ---- what the host derives: the classes' detection ranges, the kept ranges, the sort's chunks, the LDS capacities ----
    std::vector<int> cls_dt((size_t)K + 1), kept_off((size_t)C + 1);
    std::vector<int2> blk;
    int max_ng = 0, max_nd = 0, max_cls = 0;
    kept_off[0] = 0;
    for (int c = 0; c < C; ++c) {
        const int ng = cell_gt_off[c + 1] - cell_gt_off[c], nd = cell_det_off[c + 1] - cell_det_off[c];
        max_ng = std::max(max_ng, ng);
        max_nd = std::max(max_nd, nd);
        kept_off[c + 1] = kept_off[c] + std::min(nd, keep_max);
    }
    for (int k = 0; k <= K; ++k) cls_dt[k] = cell_det_off[class_cell_off[k]];
    for (int k = 0; k < K; ++k) {
        const int n = cls_dt[k + 1] - cls_dt[k];
        max_cls = std::max(max_cls, n);
        for (int at = 0; at < n; at += AP_CHUNK) blk.push_back(make_int2(cls_dt[k] + at, std::min(AP_CHUNK, n - at)));
    }
    const size_t nkept = (size_t)kept_off[C];
    const int ngc = std::max(64, (max_ng + 63) & ~63), ndc = std::max(64, (max_nd + 63) & ~63), keepc = std::min(ndc, AP_MAX_KEEP);
    const size_t n_prec = (size_t)T * R * K * A * Mn, n_rec = (size_t)T * K * A * Mn;
    // ---- the layout of the upload image, the work area and the download image ----
    SsLayout lay;
    const size_t o_gbox = lay.take(Ng * W * sizeof(double)), o_dbox = lay.take(N * W * sizeof(double)), o_score = lay.take(N * sizeof(double));
    const size_t o_crowd = lay.take(Ng * sizeof(int)), o_cgt = lay.take(((size_t)C + 1) * sizeof(int)), o_cdt = lay.take(((size_t)C + 1) * sizeof(int));
    const size_t o_ccell = lay.take(((size_t)K + 1) * sizeof(int)), o_cdet = lay.take(((size_t)K + 1) * sizeof(int)), o_kept = lay.take(((size_t)C + 1) * sizeof(int));
    const size_t o_blk = lay.take(blk.size() * sizeof(int2));
    const size_t o_thr = lay.take((size_t)T * sizeof(double)), o_rthr = lay.take((size_t)R * sizeof(double)), o_area = lay.take((size_t)A * 2 * sizeof(double));
    const size_t o_maxdet = lay.take((size_t)Mn * sizeof(int));
    const size_t up = lay.at;
    const size_t o_key0 = lay.take(N * sizeof(unsigned long long)), o_key1 = lay.take(N * sizeof(unsigned long long));
    const size_t o_idx0 = lay.take(N * sizeof(unsigned)), o_idx1 = lay.take(N * sizeof(unsigned));
    const size_t o_dpos = lay.take(N * sizeof(int)), o_dslot = lay.take(N * sizeof(int));
    const size_t o_prec = lay.take(n_prec * sizeof(double)), o_recall = lay.take(n_rec * sizeof(double));
    const size_t o_rank = lay.take(N * sizeof(int)), o_rec = lay.take((size_t)A * nkept * sizeof(unsigned));
    const size_t down_short = lay.at;
    const size_t o_midx = lay.take(rec_match ? (size_t)A * T * nkept * sizeof(int) : 0);
    const size_t total = lay.at;
    const size_t down = (rec_match ? total : down_short) - o_prec;
    const size_t host_need = up + down;

    if (!*pp) *pp = new SSAp();
    SSAp& s = **pp;
    SS_HIPCHK(who, s.ev.ensure());
    SS_HIPCHK(who, s.host.reserve(host_need, SS_QUARTER));
    SS_HIPCHK(who, s.dev.reserve(total, SS_QUARTER));
    const size_t lds_cap = ap_match_lds(AP_MAX_GTS, AP_MAX_CELL_DETS, AP_MAX_KEEP, AP_MAX_AREAS, AP_MAX_THRS, 6);
    if (!s.attr) {
        SS_HIPCHK(who, hipFuncSetAttribute((const void*)k_ap_match, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_cap));
        s.attr = true;
    }
    // ---- the upload image ----
    char* h = s.host.as();
    memcpy(h + o_gbox, gt_boxes, Ng * W * sizeof(double));
    memcpy(h + o_dbox, det_boxes, N * W * sizeof(double));
    memcpy(h + o_score, det_scores, N * sizeof(double));
    memcpy(h + o_crowd, gt_crowd, Ng * sizeof(int));
    memcpy(h + o_cgt, cell_gt_off, ((size_t)C + 1) * sizeof(int));
    memcpy(h + o_cdt, cell_det_off, ((size_t)C + 1) * sizeof(int));
    memcpy(h + o_ccell, class_cell_off, ((size_t)K + 1) * sizeof(int));
    memcpy(h + o_cdet, cls_dt.data(), ((size_t)K + 1) * sizeof(int));
    memcpy(h + o_kept, kept_off.data(), ((size_t)C + 1) * sizeof(int));
    if (!blk.empty()) memcpy(h + o_blk, blk.data(), blk.size() * sizeof(int2));
    memcpy(h + o_thr, iou_thrs, (size_t)T * sizeof(double));
    memcpy(h + o_rthr, rec_thrs, (size_t)R * sizeof(double));
    memcpy(h + o_area, areas, (size_t)A * 2 * sizeof(double));
    memcpy(h + o_maxdet, max_dets, (size_t)Mn * sizeof(int));
    char* d = s.dev.as();
    ApArgs a;
    a.gt_box = (const double*)(d + o_gbox); a.dt_box = (const double*)(d + o_dbox); a.score = (const double*)(d + o_score);
    a.gt_crowd = (const int*)(d + o_crowd); a.cell_gt = (const int*)(d + o_cgt); a.cell_dt = (const int*)(d + o_cdt);
    a.cls_cell = (const int*)(d + o_ccell); a.cls_dt = (const int*)(d + o_cdet); a.kept_off = (const int*)(d + o_kept);
    a.blk = (const int2*)(d + o_blk);
    a.thr = (const double*)(d + o_thr); a.rthr = (const double*)(d + o_rthr); a.area = (const double*)(d + o_area); a.maxdet = (const int*)(d + o_maxdet);
    a.key[0] = (unsigned long long*)(d + o_key0); a.key[1] = (unsigned long long*)(d + o_key1);
    a.idx[0] = (unsigned*)(d + o_idx0); a.idx[1] = (unsigned*)(d + o_idx1);
    a.dpos = (int*)(d + o_dpos); a.dslot = (int*)(d + o_dslot);
    a.prec = (double*)(d + o_prec); a.recall = (double*)(d + o_recall); a.rank = (int*)(d + o_rank); a.rec = (unsigned*)(d + o_rec);
    a.midx = rec_match ? (int*)(d + o_midx) : nullptr;
    a.N = (int)N; a.K = K; a.T = T; a.R = R; a.A = A; a.Mn = Mn; a.W = W; a.nkept = (int)nkept; a.fin = 0;
    a.ngc = ngc; a.ndc = ndc; a.keepc = keepc;

    SS_HIPCHK(who, hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, stream));
    if (N > 0) {
        const unsigned grid = (unsigned)((N + 255) / 256);
        hipLaunchKernelGGL(k_ap_sort_local, dim3((unsigned)blk.size()), dim3(AP_CHUNK), 0, stream, a);
        SS_HIPCHK(who, hipGetLastError());
        int src = 0;
        for (long long w = AP_CHUNK; w < max_cls; w *= 2) {               // one launch per pass
            hipLaunchKernelGGL(k_ap_sort_merge, dim3(grid), dim3(256), 0, stream, a, src, (int)w);
            SS_HIPCHK(who, hipGetLastError());
            src = 1 - src;
        }
        a.fin = src;
        hipLaunchKernelGGL(k_ap_rank, dim3(grid), dim3(256), 0, stream, a);
        SS_HIPCHK(who, hipGetLastError());
        hipLaunchKernelGGL(k_ap_match, dim3((unsigned)C), dim3(64), ap_match_lds(ngc, ndc, keepc, A, T, W == 5 ? 6 : 4), stream, a);
        SS_HIPCHK(who, hipGetLastError());
    }
    hipLaunchKernelGGL(k_ap_accum, dim3((unsigned)(K * A * Mn)), dim3(256), 0, stream, a);
    SS_HIPCHK(who, hipGetLastError());
    SS_HIPCHK(who, hipMemcpyAsync(h + up, d + o_prec, down, hipMemcpyDeviceToHost, stream));
    SS_HIPCHK(who, hipEventRecord(s.ev, stream));
    SS_HIPCHK(who, hipEventSynchronize(s.ev));
    const char* hd = h + up - o_prec;                    // hd + o_x is field x of the download image
    memcpy(precision, hd + o_prec, n_prec * sizeof(double));
    memcpy(recall, hd + o_recall, n_rec * sizeof(double));
    if (det_rank) memcpy(det_rank, hd + o_rank, N * sizeof(int));
    if (rec_match) {
        memcpy(rec_match, hd + o_midx, (size_t)A * T * nkept * sizeof(int));
        const unsigned* rw = (const unsigned*)(hd + o_rec);
        for (int ai = 0; ai < A; ++ai)
            for (int t = 0; t < T; ++t)
                for (size_t i = 0; i < nkept; ++i) rec_ignored[((size_t)ai * T + t) * nkept + i] = (int)((rw[(size_t)ai * nkept + i] >> (2 * t + 1)) & 1u);
    }
    return SS_OK;
}
