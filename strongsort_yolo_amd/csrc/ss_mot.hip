// ss_mot.hip — scoring tracks against ground truth (docs/MOTEVAL.md): HOTA's global alignment and per-frame matching and the
// CLEAR MOT walk, for up to MOT_MAX_PAIRS (ground truth, tracker) pairs a call.  All arithmetic is plain f64 VALU in the element
// order of docs/MOTEVAL.md §1, which tests/moteval_ref.py restates; the file is built with -ffp-contract=off, `/` is correctly rounded.
//
//   k_mot_sim    one workgroup per frame: S (the boxes' IoU) packed per frame into scratch, the row and column sums, si.
//   k_mot_align  one wave per ground-truth id: walks that id's rows in rising frame order, lanes over the frame's tracker boxes;
//                every cell of the id's row of `pot` gets at most one addend per frame, from this wave, in order.  Then GA in place.
//   k_mot_hota   one wave per frame: -GA S into LDS (or the frame's scratch when it does not fit), lsap_wave, the per-row record.
//   k_mot_clear  one wave per pair, persistent over the pair's frames: needs only S, so it runs on the context's second stream
//                beside k_mot_align and k_mot_hota.  prev_t lives in device memory as {tracker id, number of the processed frame
//                that set it}: "reset everywhere" is the frame number moving on.
//   k_id_count   one workgroup per frame: the identity metrics' counts, pot[g][t] += 1 where S >= thr - eps (integer atomics).
//   k_id_solve   one workgroup of 1024 threads per pair: the maximum-weight matching of ground-truth ids to tracker ids under
//                those counts, shortest augmenting paths with the columns spread over the workgroup, integer arithmetic.
// A matrix is solved with the smaller side as rows (SciPy transposes a tall matrix): lsap_wave wants nr <= nc.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "ss_common.h"
#include "ss_host.h"
#include "ss_launch.h"
#include "ss_lsap.h"
#include "ss_mot_sim.h"

#define MOT_MAX_BOXES 256
#define MOT_MAX_PAIRS 64
#define MOT_MAX_FRAMES 65536
#define MOT_MAX_ID_CELLS (1ll << 26)        // ground-truth ids x tracker ids summed over the pairs of a call: 512 MB of pot
#define MOT_MAX_SIM_CELLS (1ll << 27)       // ground-truth boxes x tracker boxes summed over the frames of a call: 1 GB each of S and si
#define MOT_LDS_CELLS 20000                 // cost entries a wave keeps in LDS: 160 000 of the 163 840 bytes a workgroup may declare
#define MOT_EPS 0x1p-52
#define MOT_MAX_IDS 4096                    // ids of one side of a pair in ss_mot_identity: k_id_solve's columns
#define MOT_ID_THREADS 1024                 // k_id_solve's workgroup; thread t owns columns t, t + 1024, ...
#define MOT_ID_Q 4                          // MOT_MAX_IDS / MOT_ID_THREADS columns a thread

struct MotArgs {
    // upload image
    const double *gt_box, *tr_box;          // [rows][4]
    const long long* s_off;                 // [frames + 1] first cell of a frame in S / si
    const long long* pot_off;               // [pairs + 1] first cell of a pair in pot
    const int *gt_off, *tr_off;             // [frames + 1]
    const int *gt_id, *tr_id;               // [rows] dense per pair
    const int* frame_off;                   // [pairs + 1]
    const int* pair_of;                     // [frames]
    const int* n_tid;                       // [pairs]
    const int* gbase;                       // [pairs + 1] first ground-truth id of a pair among all ids of the call
    const int* tbase;                       // [pairs + 1]
    const int* gid_off;                     // [all ground-truth ids + 1] into gid_rows
    const int* gid_rows;                    // ground-truth rows by (pair, id, frame)
    const int* gid_pair;                    // [all ground-truth ids]
    const int* row_frame;                   // [ground-truth rows]
    const int* cnt_t;                       // [all tracker ids] rows per id
    // work
    double *S, *si;                         // packed per frame [n_gt][n_tr]; si doubles as k_mot_hota's spill
    double* pot;                            // per pair [gt ids][tracker ids]: pot, then GA
    int2* prev_t;                           // [all ground-truth ids]
    double* clear_spill;                    // [pairs][spill_cells] or NULL
    long long spill_cells;
    // download image
    int *hota_idx, *clear_idx;              // [ground-truth rows]
    double *hota_s, *clear_s;
    int* err;
    int lds_cells;                          // cost entries of the launch's dynamic LDS
    int n_gids;
    double thr;
    // the identity metrics (ss_mot_identity): pot_off, gbase and the upload image's boxes, offsets and ids as above
    const int* n_gid;                       // [pairs]
    unsigned* id_pot;                       // per pair [rows][columns], the side with fewer ids as rows (ground truth when equal)
    int* id_match;                          // [all ground-truth ids] dense tracker id or -1
    int* id_tp;                             // [pairs]
};

__global__ __launch_bounds__(256) void k_mot_sim(const MotArgs a)
{
    __shared__ double R[MOT_MAX_BOXES], Cs[MOT_MAX_BOXES];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int g0 = a.gt_off[f], ng = a.gt_off[f + 1] - g0, t0 = a.tr_off[f], nt = a.tr_off[f + 1] - t0;
    if (ng <= 0 || nt <= 0) return;
    double* S = a.S + a.s_off[f];
    double* __restrict__ si = a.si + a.s_off[f];
    const int cells = ng * nt;
    for (int e = tid; e < cells; e += 256) {
        const int i = e / nt, j = e - i * nt;
        S[e] = mot_sim(a.gt_box + (size_t)(g0 + i) * 4, a.tr_box + (size_t)(t0 + j) * 4);
    }
    __syncthreads();
    if (tid < ng) {
        double r = 0.0;
        for (int j = 0; j < nt; ++j) r = r + S[tid * nt + j];
        R[tid] = r;
    }
    if (tid < nt) {
        double c = 0.0;
        for (int i = 0; i < ng; ++i) c = c + S[i * nt + tid];
        Cs[tid] = c;
    }
    __syncthreads();
    for (int e = tid; e < cells; e += 256) {
        const int i = e / nt, j = e - i * nt;
        const double s = S[e];
        const double den = (Cs[j] + R[i]) - s;
        si[e] = den > MOT_EPS ? s / den : 0.0;
    }
}

// one wave per ground-truth id (workgroups of four waves)
__global__ __launch_bounds__(256) void k_mot_align(const MotArgs a)
{
    const int gid = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (gid >= a.n_gids) return;
    const int p = a.gid_pair[gid], nT = a.n_tid[p];
    if (nT <= 0) return;
    double* row = a.pot + a.pot_off[p] + (long long)(gid - a.gbase[p]) * nT;
    const int r0 = a.gid_off[gid], r1 = a.gid_off[gid + 1];
    for (int k = r0; k < r1; ++k) {
        const int r = a.gid_rows[k], f = a.row_frame[r];
        const int i = r - a.gt_off[f], t0 = a.tr_off[f], nt = a.tr_off[f + 1] - t0;
        const double* __restrict__ si = a.si + a.s_off[f] + (long long)i * nt;
        for (int j = lane; j < nt; j += 64) {
            const int t = a.tr_id[t0 + j];
            row[t] = row[t] + si[j];
        }
        __threadfence();                    // the next frame's lane of a cell is another one: its load follows this store
    }
    const int cnt_g = r1 - r0;
    const int* __restrict__ cnt_t = a.cnt_t + a.tbase[p];
    for (int t = lane; t < nT; t += 64) {
        const double pot = row[t];
        row[t] = pot / ((double)(cnt_g + cnt_t[t]) - pot);
    }
}

// One wave per frame.  LDS: the cost matrix (dynamic), col4row and its inverse.
__global__ __launch_bounds__(64) void k_mot_hota(const MotArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double mot_cost[];
    __shared__ int col4row[MOT_MAX_BOXES], row4col[MOT_MAX_BOXES];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int g0 = a.gt_off[f], ng = a.gt_off[f + 1] - g0, t0 = a.tr_off[f], nt = a.tr_off[f + 1] - t0;
    if (ng <= 0) return;
    if (nt <= 0) {
        for (int i = lane; i < ng; i += 64) { a.hota_idx[g0 + i] = -1; a.hota_s[g0 + i] = 0.0; }
        return;
    }
    const int p = a.pair_of[f], nT = a.n_tid[p];
    const double* __restrict__ S = a.S + a.s_off[f];
    const double* __restrict__ GA = a.pot + a.pot_off[p];
    const int cells = ng * nt;
    double* cost = cells <= a.lds_cells ? mot_cost : a.si + a.s_off[f];
    const bool tall = nt < ng;              // fewer tracker boxes: they are the rows
    const int nr = tall ? nt : ng, nc = tall ? ng : nt;
    for (int e = lane; e < cells; e += 64) {
        const int i = e / nt, j = e - i * nt;
        const double score = GA[(long long)a.gt_id[g0 + i] * nT + a.tr_id[t0 + j]] * S[e];
        cost[tall ? j * ng + i : e] = -score;
    }
    __threadfence_block();
    __syncthreads();
    LsapLds L;
    L.col4row = col4row;
    if (lsap_wave(nr, nc, cost, L) != 0) {
        if (lane == 0) atomicMax(a.err, f + 1);
        return;
    }
    __syncthreads();
    if (!tall) {
        for (int i = lane; i < ng; i += 64) { const int j = col4row[i]; a.hota_idx[g0 + i] = j; a.hota_s[g0 + i] = S[i * nt + j]; }
        return;
    }
    for (int i = lane; i < ng; i += 64) row4col[i] = -1;
    __syncthreads();
    for (int j = lane; j < nt; j += 64) row4col[col4row[j]] = j;
    __syncthreads();
    for (int i = lane; i < ng; i += 64) {
        const int j = row4col[i];
        a.hota_idx[g0 + i] = j;
        a.hota_s[g0 + i] = j >= 0 ? S[i * nt + j] : 0.0;
    }
}

// One wave per pair, walking the pair's frames in rising order.
__global__ __launch_bounds__(64) void k_mot_clear(const MotArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double mot_cost[];
    __shared__ int col4row[MOT_MAX_BOXES], row4col[MOT_MAX_BOXES];
    const int p = blockIdx.x, lane = threadIdx.x;
    int2* prev_t = a.prev_t + a.gbase[p];
    const double lim = a.thr - MOT_EPS;
    int processed = 1;                      // 1 + processed frames so far; a table entry is live when its stamp equals this number (0: never set)
    for (int f = a.frame_off[p]; f < a.frame_off[p + 1]; ++f) {
        const int g0 = a.gt_off[f], ng = a.gt_off[f + 1] - g0, t0 = a.tr_off[f], nt = a.tr_off[f + 1] - t0;
        if (ng <= 0) continue;
        if (nt <= 0) {
            for (int i = lane; i < ng; i += 64) { a.clear_idx[g0 + i] = -1; a.clear_s[g0 + i] = 0.0; }
            continue;
        }
        const double* __restrict__ S = a.S + a.s_off[f];
        const int cells = ng * nt;
        double* cost = cells <= a.lds_cells ? mot_cost : a.clear_spill + (long long)p * a.spill_cells;
        const bool tall = nt < ng;
        const int nr = tall ? nt : ng, nc = tall ? ng : nt;
        for (int e = lane; e < cells; e += 64) {
            const int i = e / nt, j = e - i * nt;
            const int2 pt = prev_t[a.gt_id[g0 + i]];
            const double s = S[e];
            double score = ((pt.y == processed && pt.x == a.tr_id[t0 + j]) ? 1000.0 : 0.0) + s;
            if (s < lim) score = 0.0;
            cost[tall ? j * ng + i : e] = -score;
        }
        __threadfence();                    // the table was read; the matrix is written
        __syncthreads();
        LsapLds L;
        L.col4row = col4row;
        if (lsap_wave(nr, nc, cost, L) != 0) {
            if (lane == 0) atomicMax(a.err, f + 1);
            return;
        }
        __syncthreads();
        for (int i = lane; i < ng; i += 64) row4col[i] = tall ? -1 : col4row[i];
        __syncthreads();
        if (tall) {
            for (int j = lane; j < nt; j += 64) row4col[col4row[j]] = j;
            __syncthreads();
        }
        ++processed;
        for (int i = lane; i < ng; i += 64) {
            int j = row4col[i];
            if (j >= 0 && !(-cost[tall ? j * ng + i : i * nt + j] > MOT_EPS)) j = -1;
            a.clear_idx[g0 + i] = j;
            a.clear_s[g0 + i] = j >= 0 ? S[i * nt + j] : 0.0;
            if (j >= 0) prev_t[a.gt_id[g0 + i]] = make_int2(a.tr_id[t0 + j], processed);
        }
        __threadfence();                    // the next frame reads the table (and rewrites the matrix) with other lanes
        __syncthreads();
    }
}

// ---- the identity metrics: IDTP is the weight of a maximum-weight matching of ground-truth ids to tracker ids -----------------
// One workgroup per frame.  A cell of pot gets at most one addend per frame (ids are unique within a frame) and integer addition
// does not depend on the order, so the counts are deterministic.  S is not stored.
__global__ __launch_bounds__(256) void k_id_count(const MotArgs a)
{
    const int f = blockIdx.x, tid = threadIdx.x;
    const int g0 = a.gt_off[f], ng = a.gt_off[f + 1] - g0, t0 = a.tr_off[f], nt = a.tr_off[f + 1] - t0;
    if (ng <= 0 || nt <= 0) return;
    const int p = a.pair_of[f], nG = a.n_gid[p], nT = a.n_tid[p];
    const bool tall = nT < nG;              // fewer tracker ids: they are the solver's rows
    unsigned* pot = a.id_pot + a.pot_off[p];
    const double lim = a.thr - MOT_EPS;
    const int cells = ng * nt;
    for (int e = tid; e < cells; e += 256) {
        const int i = e / nt, j = e - i * nt;
        const double s = mot_sim(a.gt_box + (size_t)(g0 + i) * 4, a.tr_box + (size_t)(t0 + j) * 4);
        if (s >= lim) {
            const int g = a.gt_id[g0 + i], t = a.tr_id[t0 + j];
            atomicAdd(pot + (tall ? (size_t)t * nG + g : (size_t)g * nT + t), 1u);
        }
    }
}

// One workgroup per pair: shortest augmenting paths on the cost -pot (the algorithm of so_lsap / lsap_wave) with nr <= nc <= 4096,
// thread t owning columns t, t + 1024, ...  Per column the path cost and the dual v sit in registers, the predecessor and row4col
// in LDS (the augmentation walks them), the rows' dual u and col4row in LDS.  One scan step is a coalesced read of the current
// row's counts, the relaxations, a wave minimum (the DPP reduction of ss_lsap.h) and a 16-slot minimum through LDS, with one
// barrier: the slots alternate between two sets, so a wave that writes the next step's slot cannot overtake a reader of this one.
// The minimum is taken of the key {path cost, column assigned?, column}: among equal path costs an unassigned column wins (the
// path ends there), then the lowest column.  That is the fixed tie rule; it is not SciPy's, and the optimum value does not depend
// on it.  A row without a positive count is skipped: it can add nothing to the weight.
// Integer width.  A count is at most 65 536 = 2^16 (the frames a pair may have) and an alternating path has at most 4096 forward
// and 4095 matched edges, so every path length is below 8191 * 2^16 < 2^29 in magnitude.  The duals v and the scan's minVal are such
// path lengths, u = cost - v of a matched cell is below 2^29 + 2^16, a reduced cost cost - u - v is below 2^30 + 2^17, and
// a path cost minVal + reduced cost is below 2^29 + 2^30 + 2^17 < 2^31: int holds all of them.  A row's u starts at -2^16, at
// most every cost, so reduced costs and with them path costs are never negative, and the key
// {path cost << 13 | assigned << 12 | column} is below 2^44 and orders as the triple does.
__global__ __launch_bounds__(MOT_ID_THREADS) void k_id_solve(const MotArgs a)
{
    __shared__ int u[MOT_MAX_IDS], col4row[MOT_MAX_IDS], row4col[MOT_MAX_IDS], pred[MOT_MAX_IDS];
    __shared__ unsigned long long slot[2][MOT_ID_THREADS / 64];
    __shared__ unsigned weight;
    const int p = blockIdx.x, t = threadIdx.x, wave = t >> 6;
    const int nG = a.n_gid[p], nT = a.n_tid[p];
    const bool tall = nT < nG;
    const int nr = tall ? nT : nG, nc = tall ? nG : nT;
    int* match = a.id_match + a.gbase[p];
    for (int g = t; g < nG; g += MOT_ID_THREADS) match[g] = -1;
    if (nr <= 0) {
        if (t == 0) a.id_tp[p] = 0;
        return;
    }
    const unsigned* __restrict__ pot = a.id_pot + a.pot_off[p];
    for (int k = t; k < nc; k += MOT_ID_THREADS) row4col[k] = -1;
    for (int k = t; k < nr; k += MOT_ID_THREADS) { u[k] = -MOT_MAX_FRAMES; col4row[k] = -1; }      // cost - u - v >= 0 from the start
    if (t == 0) weight = 0u;
    int v[MOT_ID_Q], r4c[MOT_ID_Q];
#pragma unroll
    for (int q = 0; q < MOT_ID_Q; ++q) { v[q] = 0; r4c[q] = -1; }
    unsigned mine = 0u;                     // bit q: column t + 1024 q exists
#pragma unroll
    for (int q = 0; q < MOT_ID_Q; ++q) if (t + MOT_ID_THREADS * q < nc) mine |= 1u << q;
    int par = 0;
    __syncthreads();
    for (int cur = 0; cur < nr; ++cur) {
        {
            const unsigned* __restrict__ row = pot + (size_t)cur * nc;
            int any = 0;
#pragma unroll
            for (int q = 0; q < MOT_ID_Q; ++q) if (mine >> q & 1u) any |= row[t + MOT_ID_THREADS * q] != 0u;
            if (!__syncthreads_or(any)) continue;
        }
        int sp[MOT_ID_Q];
#pragma unroll
        for (int q = 0; q < MOT_ID_Q; ++q) sp[q] = 0x7fffffff;
        unsigned active = mine, scanned = 0u;
        int minVal = 0, i = cur, sink = -1;
        for (;;) {
            const unsigned* __restrict__ row = pot + (size_t)i * nc;
            unsigned c[MOT_ID_Q];
#pragma unroll
            for (int q = 0; q < MOT_ID_Q; ++q) c[q] = (active >> q & 1u) ? row[t + MOT_ID_THREADS * q] : 0u;
            const int base = minVal - u[i];
            unsigned long long key = ~0ull;
#pragma unroll
            for (int q = 0; q < MOT_ID_Q; ++q)
                if (active >> q & 1u) {
                    const int j = t + MOT_ID_THREADS * q;
                    const int r = base - (int)c[q] - v[q];
                    if (r < sp[q]) { sp[q] = r; pred[j] = i; }
                    const unsigned long long k = ((unsigned long long)(unsigned)sp[q] << 13) | (r4c[q] >= 0 ? 4096ull : 0ull) | (unsigned)j;
                    key = k < key ? k : key;
                }
            key = wave_min_u64(key);
            if ((t & 63) == 0) slot[par][wave] = key;
            __syncthreads();
            unsigned long long m = slot[par][0];
#pragma unroll
            for (int w = 1; w < MOT_ID_THREADS / 64; ++w) { const unsigned long long o = slot[par][w]; m = o < m ? o : m; }
            par ^= 1;
            const int w = (int)(m & 4095ull);
            minVal = (int)(m >> 13);
            if ((w & (MOT_ID_THREADS - 1)) == t) { active &= ~(1u << (w >> 10)); scanned |= 1u << (w >> 10); }
            if (!(m & 4096ull)) { sink = w; break; }
            i = row4col[w];
        }
        // the duals: v[j] -= minVal - sp[j] for the scanned columns, u[r] += minVal - sp[col4row[r]] for the rows reached through
        // them (every visited row but `cur`, each from its own column), u[cur] += minVal
#pragma unroll
        for (int q = 0; q < MOT_ID_Q; ++q)
            if (scanned >> q & 1u) {
                const int d = minVal - sp[q];
                v[q] -= d;
                if (r4c[q] >= 0) u[r4c[q]] += d;
            }
        if (t == 0) u[cur] += minVal;
        __syncthreads();
        if (t == 0) {                       // augment along the predecessors
            int j = sink;
            for (;;) {
                const int r = pred[j];
                row4col[j] = r;
                const int next = col4row[r];
                col4row[r] = j;
                j = next;
                if (r == cur) break;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < MOT_ID_Q; ++q) if (mine >> q & 1u) r4c[q] = row4col[t + MOT_ID_THREADS * q];
    }
    // a solved pair of count 0 is no match: the id stays -1
    for (int r = t; r < nr; r += MOT_ID_THREADS) {
        const int j = col4row[r];
        if (j < 0) continue;
        const unsigned w = pot[(size_t)r * nc + j];
        if (w == 0u) continue;
        atomicAdd(&weight, w);
        if (tall) match[j] = r; else match[r] = j;
    }
    __syncthreads();
    if (t == 0) a.id_tp[p] = (int)weight;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct SSMot {
    SsBuf<SS_PINNED> host;                              // the upload image, then the download image
    SsBuf<SS_DEVICE> dev;                               // upload image | prev_t | pot | download image
    SsBuf<SS_DEVICE> sim;                               // S and si, grown when a call needs more
    SsBuf<SS_DEVICE> spill;                             // k_mot_clear's matrices that do not fit the LDS
    hipStream_t side = nullptr;                         // k_mot_clear's stream
    SsEvent ev, ev_sim, ev_clear;
    bool attr = false;
};

void ss_mot_free(SSMot* m)
{
    if (m && m->side) (void)hipStreamDestroy(m->side);
    delete m;
}

int ss_mot_max_boxes_impl() { return MOT_MAX_BOXES; }
int ss_mot_max_ids_impl() { return MOT_MAX_IDS; }

// Every refusal of ss_mot_eval and ss_mot_identity that needs neither a context nor the device: SS_ERR_INVALID for arguments
// that make no sense, SS_ERR_CAPACITY for a call that is too large.  `identity`: at most MOT_MAX_IDS ids a side of a pair, and no
// cap on the box x box cells (S is not stored).  any_null: one of the call's own output pointers is NULL.
static int mot_check(const std::string& who, bool identity, bool any_null, int n_pairs, const int* frame_off, const int* gt_off, const int* tr_off,
                     const int* gt_id, const int* tr_id, const double* gt_box, const double* tr_box, const int* n_gt_ids, const int* n_tr_ids,
                     double thr, std::string& err)
{
    if (!frame_off || !gt_off || !tr_off || !gt_id || !tr_id || !gt_box || !tr_box || !n_gt_ids || !n_tr_ids || any_null) {
        err = who + "null argument"; return SS_ERR_INVALID;
    }
    if (n_pairs < 1) { err = who + "n_pairs must be at least 1"; return SS_ERR_INVALID; }
    if (!(thr > 0.0) || !(thr <= 1.0)) { err = who + "thr must be in (0, 1]"; return SS_ERR_INVALID; }
    if (n_pairs > MOT_MAX_PAIRS) { err = who + std::to_string(n_pairs) + " pairs: at most " + std::to_string(MOT_MAX_PAIRS) + " a call"; return SS_ERR_CAPACITY; }
    if (frame_off[0] != 0 || gt_off[0] != 0 || tr_off[0] != 0) { err = who + "offsets must start at 0"; return SS_ERR_INVALID; }
    for (int p = 0; p < n_pairs; ++p) {
        const std::string pr = "pair " + std::to_string(p) + ": ";
        if (frame_off[p + 1] < frame_off[p]) { err = who + pr + "frame offsets decrease"; return SS_ERR_INVALID; }
        if (n_gt_ids[p] < 0 || n_tr_ids[p] < 0) { err = who + pr + "an id count is negative"; return SS_ERR_INVALID; }
        if (frame_off[p + 1] - frame_off[p] > MOT_MAX_FRAMES) {
            err = who + pr + std::to_string(frame_off[p + 1] - frame_off[p]) + " frames: at most " + std::to_string(MOT_MAX_FRAMES) + " a pair"; return SS_ERR_CAPACITY;
        }
        if (identity && (n_gt_ids[p] > MOT_MAX_IDS || n_tr_ids[p] > MOT_MAX_IDS)) {
            const bool g = n_gt_ids[p] > MOT_MAX_IDS;
            err = who + pr + std::to_string(g ? n_gt_ids[p] : n_tr_ids[p]) + (g ? " ground-truth" : " tracker") + " ids: at most " + std::to_string(MOT_MAX_IDS) + " a side";
            return SS_ERR_CAPACITY;
        }
    }
    for (int p = 0; p < n_pairs; ++p) {               // (every frame offset is sound by now)
        const std::string pr = "pair " + std::to_string(p) + ": ";
        for (int f = frame_off[p]; f < frame_off[p + 1]; ++f) {
            const std::string fr = pr + "frame " + std::to_string(f - frame_off[p]) + ": ";
            if (gt_off[f + 1] < gt_off[f]) { err = who + fr + "ground-truth row offsets decrease"; return SS_ERR_INVALID; }
            if (tr_off[f + 1] < tr_off[f]) { err = who + fr + "tracker row offsets decrease"; return SS_ERR_INVALID; }
        }
        // dense ids: a pair cannot name more ids than it has rows (this also bounds what is allocated here and for the device)
        if (n_gt_ids[p] > gt_off[frame_off[p + 1]] - gt_off[frame_off[p]] || n_tr_ids[p] > tr_off[frame_off[p + 1]] - tr_off[frame_off[p]]) {
            err = who + pr + "more ids than rows"; return SS_ERR_INVALID;
        }
    }
    std::vector<int> seen_g, seen_t;
    long long id_cells = 0, sim_cells = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const std::string pr = "pair " + std::to_string(p) + ": ";
        seen_g.assign((size_t)n_gt_ids[p], -1);
        seen_t.assign((size_t)n_tr_ids[p], -1);
        id_cells += (long long)n_gt_ids[p] * n_tr_ids[p];
        for (int f = frame_off[p]; f < frame_off[p + 1]; ++f) {
            const std::string fr = pr + "frame " + std::to_string(f - frame_off[p]) + ": ";
            for (int side = 0; side < 2; ++side) {
                const int* off = side ? tr_off : gt_off;
                const int* id = side ? tr_id : gt_id;
                const double* box = side ? tr_box : gt_box;
                std::vector<int>& seen = side ? seen_t : seen_g;
                const char* name = side ? "tracker" : "ground-truth";
                if (off[f + 1] - off[f] > MOT_MAX_BOXES) {
                    err = who + fr + std::to_string(off[f + 1] - off[f]) + " " + name + " boxes: at most " + std::to_string(MOT_MAX_BOXES) + " a frame"; return SS_ERR_CAPACITY;
                }
                for (int r = off[f]; r < off[f + 1]; ++r) {
                    if (id[r] < 0 || id[r] >= (int)seen.size()) { err = who + fr + "a " + name + " id is out of range"; return SS_ERR_INVALID; }
                    if (seen[id[r]] == f) { err = who + fr + "a " + name + " id appears twice"; return SS_ERR_INVALID; }
                    seen[id[r]] = f;
                    const double* b = box + (size_t)r * 4;
                    if (!std::isfinite(b[0]) || !std::isfinite(b[1]) || !std::isfinite(b[2]) || !std::isfinite(b[3])) { err = who + fr + "a " + name + " box is NaN or infinite"; return SS_ERR_INVALID; }
                    if (!(b[2] > b[0]) || !(b[3] > b[1])) { err = who + fr + "a " + name + " box has x2 <= x1 or y2 <= y1"; return SS_ERR_INVALID; }
                }
            }
            sim_cells += (long long)(gt_off[f + 1] - gt_off[f]) * (tr_off[f + 1] - tr_off[f]);
        }
    }
    if (id_cells > MOT_MAX_ID_CELLS) { err = who + std::to_string(id_cells) + " ground-truth id x tracker id cells: at most " + std::to_string(MOT_MAX_ID_CELLS) + " a call"; return SS_ERR_CAPACITY; }
    if (!identity && sim_cells > MOT_MAX_SIM_CELLS) { err = who + std::to_string(sim_cells) + " box x box cells: at most " + std::to_string(MOT_MAX_SIM_CELLS) + " a call"; return SS_ERR_CAPACITY; }
    return SS_OK;
}

int ss_mot_check_impl(int n_pairs, const int* frame_off, const int* gt_off, const int* tr_off, const int* gt_id, const int* tr_id,
                      const double* gt_box, const double* tr_box, const int* n_gt_ids, const int* n_tr_ids, double thr,
                      const int* hota_idx, const double* hota_s, const int* clear_idx, const double* clear_s, std::string& err)
{
    return mot_check("ss_mot_eval: ", false, !hota_idx || !hota_s || !clear_idx || !clear_s, n_pairs, frame_off, gt_off, tr_off, gt_id, tr_id, gt_box,
                     tr_box, n_gt_ids, n_tr_ids, thr, err);
}

int ss_mot_identity_check_impl(int n_pairs, const int* frame_off, const int* gt_off, const int* tr_off, const int* gt_id, const int* tr_id,
                               const double* gt_box, const double* tr_box, const int* n_gt_ids, const int* n_tr_ids, double thr,
                               const int* idtp, const int* gt_to_tr, std::string& err)
{
    return mot_check("ss_mot_identity: ", true, !idtp || !gt_to_tr, n_pairs, frame_off, gt_off, tr_off, gt_id, tr_id, gt_box, tr_box, n_gt_ids,
                     n_tr_ids, thr, err);
}

int ss_mot_eval_impl(SSMot** pm, hipStream_t stream, int n_pairs, const int* frame_off, const int* gt_off, const int* tr_off, const int* gt_id,
                     const int* tr_id, const double* gt_box, const double* tr_box, const int* n_gt_ids, const int* n_tr_ids, double thr,
                     int* hota_idx, double* hota_s, int* clear_idx, double* clear_s, double* ga, std::string& err)
{
    const char* const who = "ss_mot_eval: ";
    if (!pm) { err = "ss_mot_eval: null context"; return SS_ERR_INVALID; }
    const int F = frame_off[n_pairs];
    const size_t Ng = (size_t)gt_off[F], Nt = (size_t)tr_off[F];
    size_t nG = 0, nT = 0;
    for (int p = 0; p < n_pairs; ++p) { nG += n_gt_ids[p]; nT += n_tr_ids[p]; }
    // ---- the layout of the upload image, the work area and the download image ----
    SsLayout lay;
    const size_t o_gbox = lay.take(Ng * 4 * sizeof(double)), o_tbox = lay.take(Nt * 4 * sizeof(double));
    const size_t o_soff = lay.take((size_t)(F + 1) * sizeof(long long)), o_poff = lay.take((size_t)(n_pairs + 1) * sizeof(long long));
    const size_t o_goff = lay.take((size_t)(F + 1) * sizeof(int)), o_toff = lay.take((size_t)(F + 1) * sizeof(int));
    const size_t o_gid = lay.take(Ng * sizeof(int)), o_tid = lay.take(Nt * sizeof(int));
    const size_t o_foff = lay.take((size_t)(n_pairs + 1) * sizeof(int)), o_pairof = lay.take((size_t)F * sizeof(int)), o_ntid = lay.take((size_t)n_pairs * sizeof(int));
    const size_t o_gbase = lay.take((size_t)(n_pairs + 1) * sizeof(int)), o_tbase = lay.take((size_t)(n_pairs + 1) * sizeof(int));
    const size_t o_gidoff = lay.take((nG + 1) * sizeof(int)), o_gidrows = lay.take(Ng * sizeof(int)), o_gidpair = lay.take(nG * sizeof(int));
    const size_t o_rowframe = lay.take(Ng * sizeof(int)), o_cntt = lay.take(nT * sizeof(int));
    const size_t up = lay.at;
    const size_t o_prev = lay.take(nG * sizeof(int2));
    size_t id_cells = 0;
    for (int p = 0; p < n_pairs; ++p) id_cells += (size_t)n_gt_ids[p] * n_tr_ids[p];
    const size_t o_pot = lay.take(id_cells * sizeof(double));
    const size_t o_hs = lay.take(Ng * sizeof(double)), o_cs = lay.take(Ng * sizeof(double));
    const size_t o_hi = lay.take(Ng * sizeof(int)), o_ci = lay.take(Ng * sizeof(int)), o_err = lay.take(sizeof(int));
    const size_t total = lay.at;
    const size_t down_from = ga ? o_pot : o_hs, down = total - down_from;
    const size_t host_need = up + down;

    if (!*pm) *pm = new SSMot();
    SSMot& m = **pm;
    SS_HIPCHK(who, m.ev.ensure());
    SS_HIPCHK(who, m.ev_sim.ensure());
    SS_HIPCHK(who, m.ev_clear.ensure());
    if (!m.side) SS_HIPCHK(who, hipStreamCreateWithFlags(&m.side, hipStreamNonBlocking));
    SS_HIPCHK(who, m.host.reserve(host_need, SS_QUARTER));
    SS_HIPCHK(who, m.dev.reserve(total, SS_QUARTER));
    // ---- the upload image ----
    char* h = m.host.as();
    memcpy(h + o_gbox, gt_box, Ng * 4 * sizeof(double));
    memcpy(h + o_tbox, tr_box, Nt * 4 * sizeof(double));
    memcpy(h + o_goff, gt_off, (size_t)(F + 1) * sizeof(int));
    memcpy(h + o_toff, tr_off, (size_t)(F + 1) * sizeof(int));
    memcpy(h + o_gid, gt_id, Ng * sizeof(int));
    memcpy(h + o_tid, tr_id, Nt * sizeof(int));
    memcpy(h + o_foff, frame_off, (size_t)(n_pairs + 1) * sizeof(int));
    memcpy(h + o_ntid, n_tr_ids, (size_t)n_pairs * sizeof(int));
    long long* h_soff = (long long*)(h + o_soff); long long* h_poff = (long long*)(h + o_poff);
    int* h_pairof = (int*)(h + o_pairof); int* h_gbase = (int*)(h + o_gbase); int* h_tbase = (int*)(h + o_tbase);
    int* h_gidoff = (int*)(h + o_gidoff); int* h_gidrows = (int*)(h + o_gidrows); int* h_gidpair = (int*)(h + o_gidpair);
    int* h_rowframe = (int*)(h + o_rowframe); int* h_cntt = (int*)(h + o_cntt);
    long long sim_cells = 0, max_cells = 0;
    h_poff[0] = 0; h_gbase[0] = 0; h_tbase[0] = 0;
    memset(h_cntt, 0, nT * sizeof(int));
    std::vector<int> cnt_g(nG + 1, 0);
    for (int p = 0; p < n_pairs; ++p) {
        h_poff[p + 1] = h_poff[p] + (long long)n_gt_ids[p] * n_tr_ids[p];
        h_gbase[p + 1] = h_gbase[p] + n_gt_ids[p];
        h_tbase[p + 1] = h_tbase[p] + n_tr_ids[p];
        for (int g = 0; g < n_gt_ids[p]; ++g) h_gidpair[h_gbase[p] + g] = p;
        for (int f = frame_off[p]; f < frame_off[p + 1]; ++f) {
            h_pairof[f] = p;
            h_soff[f] = sim_cells;
            const long long c = (long long)(gt_off[f + 1] - gt_off[f]) * (tr_off[f + 1] - tr_off[f]);
            sim_cells += c;
            if (c > max_cells) max_cells = c;
            for (int r = gt_off[f]; r < gt_off[f + 1]; ++r) { h_rowframe[r] = f; ++cnt_g[h_gbase[p] + gt_id[r]]; }
            for (int r = tr_off[f]; r < tr_off[f + 1]; ++r) ++h_cntt[h_tbase[p] + tr_id[r]];
        }
    }
    h_soff[F] = sim_cells;
    h_gidoff[0] = 0;
    for (size_t g = 0; g < nG; ++g) h_gidoff[g + 1] = h_gidoff[g] + cnt_g[g];
    {
        std::vector<int> fill(h_gidoff, h_gidoff + nG);
        for (int p = 0; p < n_pairs; ++p)
            for (int r = gt_off[frame_off[p]]; r < gt_off[frame_off[p + 1]]; ++r) h_gidrows[fill[h_gbase[p] + gt_id[r]]++] = r;      // rows come by frame
    }
    // ---- scratch of the context ----
    SS_HIPCHK(who, m.sim.reserve((size_t)sim_cells * 2 * sizeof(double), SS_EXACT));
    const int lds_cells = (int)std::min<long long>(max_cells, MOT_LDS_CELLS);
    const long long spill_cells = max_cells > MOT_LDS_CELLS ? max_cells : 0;
    SS_HIPCHK(who, m.spill.reserve((size_t)spill_cells * n_pairs * sizeof(double), SS_EXACT));
    if (!m.attr) {
        SS_HIPCHK(who, hipFuncSetAttribute((const void*)k_mot_hota, hipFuncAttributeMaxDynamicSharedMemorySize, MOT_LDS_CELLS * (int)sizeof(double)));
        SS_HIPCHK(who, hipFuncSetAttribute((const void*)k_mot_clear, hipFuncAttributeMaxDynamicSharedMemorySize, MOT_LDS_CELLS * (int)sizeof(double)));
        m.attr = true;
    }
    char* d = m.dev.as();
    MotArgs a;
    a.gt_box = (const double*)(d + o_gbox); a.tr_box = (const double*)(d + o_tbox);
    a.s_off = (const long long*)(d + o_soff); a.pot_off = (const long long*)(d + o_poff);
    a.gt_off = (const int*)(d + o_goff); a.tr_off = (const int*)(d + o_toff); a.gt_id = (const int*)(d + o_gid); a.tr_id = (const int*)(d + o_tid);
    a.frame_off = (const int*)(d + o_foff); a.pair_of = (const int*)(d + o_pairof); a.n_tid = (const int*)(d + o_ntid);
    a.gbase = (const int*)(d + o_gbase); a.tbase = (const int*)(d + o_tbase);
    a.gid_off = (const int*)(d + o_gidoff); a.gid_rows = (const int*)(d + o_gidrows); a.gid_pair = (const int*)(d + o_gidpair);
    a.row_frame = (const int*)(d + o_rowframe); a.cnt_t = (const int*)(d + o_cntt);
    a.S = m.sim.as<double>(); a.si = a.S + sim_cells;
    a.pot = (double*)(d + o_pot); a.prev_t = (int2*)(d + o_prev);
    a.clear_spill = spill_cells ? m.spill.as<double>() : nullptr; a.spill_cells = spill_cells;
    a.hota_idx = (int*)(d + o_hi); a.clear_idx = (int*)(d + o_ci); a.hota_s = (double*)(d + o_hs); a.clear_s = (double*)(d + o_cs);
    a.err = (int*)(d + o_err);
    a.lds_cells = lds_cells; a.n_gids = (int)nG; a.thr = thr;

    SS_HIPCHK(who, hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, stream));
    if (o_hs > o_prev) SS_HIPCHK(who, hipMemsetAsync(d + o_prev, 0, o_hs - o_prev, stream));        // prev_t (stamp 0: none) and pot
    SS_HIPCHK(who, hipMemsetAsync(d + o_err, 0, sizeof(int), stream));
    if (F > 0 && Ng > 0) {
        if (sim_cells > 0) {
            hipLaunchKernelGGL(k_mot_sim, dim3((unsigned)F), dim3(256), 0, stream, a);
            SS_HIPCHK(who, hipGetLastError());
        }
        SS_HIPCHK(who, hipEventRecord(m.ev_sim, stream));
        SS_HIPCHK(who, hipStreamWaitEvent(m.side, m.ev_sim, 0));
        hipLaunchKernelGGL(k_mot_clear, dim3((unsigned)n_pairs), dim3(64), (size_t)lds_cells * sizeof(double), m.side, a);
        SS_HIPCHK(who, hipGetLastError());
        SS_HIPCHK(who, hipEventRecord(m.ev_clear, m.side));
        if (sim_cells > 0 && nG > 0) {
            hipLaunchKernelGGL(k_mot_align, dim3((unsigned)((nG + 3) / 4)), dim3(256), 0, stream, a);
            SS_HIPCHK(who, hipGetLastError());
        }
        hipLaunchKernelGGL(k_mot_hota, dim3((unsigned)F), dim3(64), (size_t)lds_cells * sizeof(double), stream, a);
        SS_HIPCHK(who, hipGetLastError());
        SS_HIPCHK(who, hipStreamWaitEvent(stream, m.ev_clear, 0));
    }
    SS_HIPCHK(who, hipMemcpyAsync(h + up, d + down_from, down, hipMemcpyDeviceToHost, stream));
    SS_HIPCHK(who, hipEventRecord(m.ev, stream));
    SS_HIPCHK(who, hipEventSynchronize(m.ev));
    const char* hd = h + up - down_from;                 // hd + o_x is field x of the download image
    const int bad = *(const int*)(hd + o_err);
    if (bad) {
        const int f = bad - 1, p = h_pairof[f];
        err = "ss_mot_eval: pair " + std::to_string(p) + ": frame " + std::to_string(f - frame_off[p]) + ": the assignment problem was infeasible";
        return SS_ERR_INFEASIBLE;
    }
    memcpy(hota_s, hd + o_hs, Ng * sizeof(double));
    memcpy(clear_s, hd + o_cs, Ng * sizeof(double));
    memcpy(hota_idx, hd + o_hi, Ng * sizeof(int));
    memcpy(clear_idx, hd + o_ci, Ng * sizeof(int));
    if (ga) memcpy(ga, hd + o_pot, id_cells * sizeof(double));
    return SS_OK;
}

// The identity metrics' counts and matching.  The staging areas are the context's, shared with ss_mot_eval (a call owns them until
// its event has passed): upload image | pot | download image (gt_to_tr, idtp), pot downloaded with it when the caller wants it.
int ss_mot_identity_impl(SSMot** pm, hipStream_t stream, int n_pairs, const int* frame_off, const int* gt_off, const int* tr_off, const int* gt_id,
                         const int* tr_id, const double* gt_box, const double* tr_box, const int* n_gt_ids, const int* n_tr_ids, double thr,
                         int* idtp, int* gt_to_tr, int* pot, std::string& err)
{
    const char* const who = "ss_mot_identity: ";
    if (!pm) { err = "ss_mot_identity: null context"; return SS_ERR_INVALID; }
    const int F = frame_off[n_pairs];
    const size_t Ng = (size_t)gt_off[F], Nt = (size_t)tr_off[F];
    size_t nG = 0, id_cells = 0;
    for (int p = 0; p < n_pairs; ++p) { nG += n_gt_ids[p]; id_cells += (size_t)n_gt_ids[p] * n_tr_ids[p]; }
    SsLayout lay;
    const size_t o_gbox = lay.take(Ng * 4 * sizeof(double)), o_tbox = lay.take(Nt * 4 * sizeof(double));
    const size_t o_poff = lay.take((size_t)(n_pairs + 1) * sizeof(long long));
    const size_t o_goff = lay.take((size_t)(F + 1) * sizeof(int)), o_toff = lay.take((size_t)(F + 1) * sizeof(int));
    const size_t o_gid = lay.take(Ng * sizeof(int)), o_tid = lay.take(Nt * sizeof(int));
    const size_t o_pairof = lay.take((size_t)F * sizeof(int)), o_ngid = lay.take((size_t)n_pairs * sizeof(int)), o_ntid = lay.take((size_t)n_pairs * sizeof(int));
    const size_t o_gbase = lay.take((size_t)(n_pairs + 1) * sizeof(int));
    const size_t up = lay.at;
    const size_t o_pot = lay.take(id_cells * sizeof(unsigned));
    const size_t o_match = lay.take(nG * sizeof(int)), o_tp = lay.take((size_t)n_pairs * sizeof(int));
    const size_t total = lay.at;
    const size_t down_from = pot ? o_pot : o_match, down = total - down_from;
    const size_t host_need = up + down;

    if (!*pm) *pm = new SSMot();
    SSMot& m = **pm;
    SS_HIPCHK(who, m.ev.ensure());
    SS_HIPCHK(who, m.host.reserve(host_need, SS_QUARTER));
    SS_HIPCHK(who, m.dev.reserve(total, SS_QUARTER));
    char* h = m.host.as();
    memcpy(h + o_gbox, gt_box, Ng * 4 * sizeof(double));
    memcpy(h + o_tbox, tr_box, Nt * 4 * sizeof(double));
    memcpy(h + o_goff, gt_off, (size_t)(F + 1) * sizeof(int));
    memcpy(h + o_toff, tr_off, (size_t)(F + 1) * sizeof(int));
    memcpy(h + o_gid, gt_id, Ng * sizeof(int));
    memcpy(h + o_tid, tr_id, Nt * sizeof(int));
    memcpy(h + o_ngid, n_gt_ids, (size_t)n_pairs * sizeof(int));
    memcpy(h + o_ntid, n_tr_ids, (size_t)n_pairs * sizeof(int));
    long long* h_poff = (long long*)(h + o_poff);
    int* h_pairof = (int*)(h + o_pairof); int* h_gbase = (int*)(h + o_gbase);
    h_poff[0] = 0; h_gbase[0] = 0;
    bool cells = false;                                  // some frame has boxes on both sides
    for (int p = 0; p < n_pairs; ++p) {
        h_poff[p + 1] = h_poff[p] + (long long)n_gt_ids[p] * n_tr_ids[p];
        h_gbase[p + 1] = h_gbase[p] + n_gt_ids[p];
        for (int f = frame_off[p]; f < frame_off[p + 1]; ++f) {
            h_pairof[f] = p;
            cells = cells || (gt_off[f + 1] > gt_off[f] && tr_off[f + 1] > tr_off[f]);
        }
    }
    char* d = m.dev.as();
    MotArgs a;
    memset(&a, 0, sizeof a);
    a.gt_box = (const double*)(d + o_gbox); a.tr_box = (const double*)(d + o_tbox);
    a.pot_off = (const long long*)(d + o_poff);
    a.gt_off = (const int*)(d + o_goff); a.tr_off = (const int*)(d + o_toff); a.gt_id = (const int*)(d + o_gid); a.tr_id = (const int*)(d + o_tid);
    a.pair_of = (const int*)(d + o_pairof); a.n_gid = (const int*)(d + o_ngid); a.n_tid = (const int*)(d + o_ntid);
    a.gbase = (const int*)(d + o_gbase);
    a.id_pot = (unsigned*)(d + o_pot); a.id_match = (int*)(d + o_match); a.id_tp = (int*)(d + o_tp);
    a.thr = thr;

    SS_HIPCHK(who, hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, stream));
    if (id_cells) SS_HIPCHK(who, hipMemsetAsync(d + o_pot, 0, id_cells * sizeof(unsigned), stream));       // every call
    if (cells) {
        hipLaunchKernelGGL(k_id_count, dim3((unsigned)F), dim3(256), 0, stream, a);
        SS_HIPCHK(who, hipGetLastError());
    }
    hipLaunchKernelGGL(k_id_solve, dim3((unsigned)n_pairs), dim3(MOT_ID_THREADS), 0, stream, a);
    SS_HIPCHK(who, hipGetLastError());
    SS_HIPCHK(who, hipMemcpyAsync(h + up, d + down_from, down, hipMemcpyDeviceToHost, stream));
    SS_HIPCHK(who, hipEventRecord(m.ev, stream));
    SS_HIPCHK(who, hipEventSynchronize(m.ev));
    const char* hd = h + up - down_from;                 // hd + o_x is field x of the download image
    memcpy(idtp, hd + o_tp, (size_t)n_pairs * sizeof(int));
    memcpy(gt_to_tr, hd + o_match, nG * sizeof(int));
    if (pot) {                                           // the device's rows are the side with fewer ids: hand out [n_gt_ids][n_tr_ids]
        const unsigned* src = (const unsigned*)(hd + o_pot);
        for (int p = 0; p < n_pairs; ++p) {
            const int G = n_gt_ids[p], T = n_tr_ids[p];
            const unsigned* s = src + h_poff[p];
            int* o = pot + h_poff[p];
            if (T < G) {
                for (int g = 0; g < G; ++g)
                    for (int t = 0; t < T; ++t) o[(size_t)g * T + t] = (int)s[(size_t)t * G + g];
            } else memcpy(o, s, (size_t)G * T * sizeof(int));
        }
    }
    return SS_OK;
}
