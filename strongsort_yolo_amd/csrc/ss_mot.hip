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
// A matrix is solved with the smaller side as rows (SciPy transposes a tall matrix): lsap_wave wants nr <= nc.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "ss_common.h"
#include "ss_launch.h"
#include "ss_lsap.h"

#define MOT_MAX_BOXES 256
#define MOT_MAX_PAIRS 64
#define MOT_MAX_FRAMES 65536
#define MOT_MAX_ID_CELLS (1ll << 26)        // ground-truth ids x tracker ids summed over the pairs of a call: 512 MB of pot
#define MOT_MAX_SIM_CELLS (1ll << 27)       // ground-truth boxes x tracker boxes summed over the frames of a call: 1 GB each of S and si
#define MOT_LDS_CELLS 20000                 // cost entries a wave keeps in LDS: 160 000 of the 163 840 bytes a workgroup may declare
#define MOT_EPS 0x1p-52

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
        const double* A = a.gt_box + (size_t)(g0 + i) * 4;
        const double* B = a.tr_box + (size_t)(t0 + j) * 4;
        const double ax1 = A[0], ay1 = A[1], ax2 = A[2], ay2 = A[3], bx1 = B[0], by1 = B[1], bx2 = B[2], by2 = B[3];
        const double w = fmax(0.0, fmin(ax2, bx2) - fmax(ax1, bx1)), h = fmax(0.0, fmin(ay2, by2) - fmax(ay1, by1));
        const double inter = w * h;
        const double uni = ((ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1)) - inter;
        S[e] = inter / uni;
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

// ---- host ------------------------------------------------------------------------------------------------------------------
struct SSMot {
    void* host = nullptr; size_t host_cap = 0;          // pinned: the upload image, then the download image
    void* dev = nullptr; size_t dev_cap = 0;            // upload image | prev_t | pot | download image
    double* sim = nullptr; size_t sim_cap = 0;          // doubles: S and si, grown when a call needs more
    double* spill = nullptr; size_t spill_cap = 0;      // doubles: k_mot_clear's matrices that do not fit the LDS
    hipStream_t side = nullptr;                         // k_mot_clear's stream
    hipEvent_t ev = nullptr, ev_sim = nullptr, ev_clear = nullptr;
    bool attr = false;
};

void ss_mot_free(SSMot* m)
{
    if (!m) return;
    if (m->ev) (void)hipEventDestroy(m->ev);
    if (m->ev_sim) (void)hipEventDestroy(m->ev_sim);
    if (m->ev_clear) (void)hipEventDestroy(m->ev_clear);
    if (m->side) (void)hipStreamDestroy(m->side);
    if (m->host) (void)hipHostFree(m->host);
    if (m->dev) (void)hipFree(m->dev);
    if (m->sim) (void)hipFree(m->sim);
    if (m->spill) (void)hipFree(m->spill);
    delete m;
}

int ss_mot_max_boxes_impl() { return MOT_MAX_BOXES; }

// Every refusal of ss_mot_eval that needs neither a context nor the device: SS_ERR_INVALID for arguments that make no sense,
// SS_ERR_CAPACITY for a call that is too large.
int ss_mot_check_impl(int n_pairs, const int* frame_off, const int* gt_off, const int* tr_off, const int* gt_id, const int* tr_id,
                      const double* gt_box, const double* tr_box, const int* n_gt_ids, const int* n_tr_ids, double thr,
                      const int* hota_idx, const double* hota_s, const int* clear_idx, const double* clear_s, std::string& err)
{
    const std::string who = "ss_mot_eval: ";
    if (!frame_off || !gt_off || !tr_off || !gt_id || !tr_id || !gt_box || !tr_box || !n_gt_ids || !n_tr_ids || !hota_idx || !hota_s || !clear_idx || !clear_s) {
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
    if (sim_cells > MOT_MAX_SIM_CELLS) { err = who + std::to_string(sim_cells) + " box x box cells: at most " + std::to_string(MOT_MAX_SIM_CELLS) + " a call"; return SS_ERR_CAPACITY; }
    return SS_OK;
}

#define MCHK(x)                                                                                     \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) { err = std::string("ss_mot_eval: " #x ": ") + hipGetErrorString(e_); return SS_ERR_HIP; } \
    } while (0)

static size_t mot_up16(size_t b) { return (b + 15) & ~(size_t)15; }

int ss_mot_eval_impl(SSMot** pm, hipStream_t stream, int n_pairs, const int* frame_off, const int* gt_off, const int* tr_off, const int* gt_id,
                     const int* tr_id, const double* gt_box, const double* tr_box, const int* n_gt_ids, const int* n_tr_ids, double thr,
                     int* hota_idx, double* hota_s, int* clear_idx, double* clear_s, double* ga, std::string& err)
{
    if (!pm) { err = "ss_mot_eval: null context"; return SS_ERR_INVALID; }
    const int F = frame_off[n_pairs];
    const size_t Ng = (size_t)gt_off[F], Nt = (size_t)tr_off[F];
    size_t nG = 0, nT = 0;
    for (int p = 0; p < n_pairs; ++p) { nG += n_gt_ids[p]; nT += n_tr_ids[p]; }
    // ---- the layout of the upload image, the work area and the download image ----
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = mot_up16(at + bytes); return o; };
    const size_t o_gbox = take(Ng * 4 * sizeof(double)), o_tbox = take(Nt * 4 * sizeof(double));
    const size_t o_soff = take((size_t)(F + 1) * sizeof(long long)), o_poff = take((size_t)(n_pairs + 1) * sizeof(long long));
    const size_t o_goff = take((size_t)(F + 1) * sizeof(int)), o_toff = take((size_t)(F + 1) * sizeof(int));
    const size_t o_gid = take(Ng * sizeof(int)), o_tid = take(Nt * sizeof(int));
    const size_t o_foff = take((size_t)(n_pairs + 1) * sizeof(int)), o_pairof = take((size_t)F * sizeof(int)), o_ntid = take((size_t)n_pairs * sizeof(int));
    const size_t o_gbase = take((size_t)(n_pairs + 1) * sizeof(int)), o_tbase = take((size_t)(n_pairs + 1) * sizeof(int));
    const size_t o_gidoff = take((nG + 1) * sizeof(int)), o_gidrows = take(Ng * sizeof(int)), o_gidpair = take(nG * sizeof(int));
    const size_t o_rowframe = take(Ng * sizeof(int)), o_cntt = take(nT * sizeof(int));
    const size_t up = at;
    const size_t o_prev = take(nG * sizeof(int2));
    size_t id_cells = 0;
    for (int p = 0; p < n_pairs; ++p) id_cells += (size_t)n_gt_ids[p] * n_tr_ids[p];
    const size_t o_pot = take(id_cells * sizeof(double));
    const size_t o_hs = take(Ng * sizeof(double)), o_cs = take(Ng * sizeof(double));
    const size_t o_hi = take(Ng * sizeof(int)), o_ci = take(Ng * sizeof(int)), o_err = take(sizeof(int));
    const size_t total = at;
    const size_t down_from = ga ? o_pot : o_hs, down = total - down_from;
    const size_t host_need = up + down;

    if (!*pm) *pm = new SSMot();
    SSMot& m = **pm;
    if (!m.ev) MCHK(hipEventCreateWithFlags(&m.ev, hipEventDisableTiming));
    if (!m.ev_sim) MCHK(hipEventCreateWithFlags(&m.ev_sim, hipEventDisableTiming));
    if (!m.ev_clear) MCHK(hipEventCreateWithFlags(&m.ev_clear, hipEventDisableTiming));
    if (!m.side) MCHK(hipStreamCreateWithFlags(&m.side, hipStreamNonBlocking));
    if (m.host_cap < host_need) {
        if (m.host) { MCHK(hipHostFree(m.host)); m.host = nullptr; m.host_cap = 0; }
        const size_t cap = host_need + host_need / 4;
        MCHK(hipHostMalloc(&m.host, cap, hipHostMallocDefault));
        m.host_cap = cap;
    }
    if (m.dev_cap < total) {
        if (m.dev) { MCHK(hipFree(m.dev)); m.dev = nullptr; m.dev_cap = 0; }
        const size_t cap = total + total / 4;
        MCHK(hipMalloc(&m.dev, cap));
        m.dev_cap = cap;
    }
    // ---- the upload image ----
    char* h = (char*)m.host;
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
    if (m.sim_cap < (size_t)sim_cells * 2) {
        if (m.sim) { MCHK(hipFree(m.sim)); m.sim = nullptr; m.sim_cap = 0; }
        MCHK(hipMalloc((void**)&m.sim, (size_t)sim_cells * 2 * sizeof(double)));
        m.sim_cap = (size_t)sim_cells * 2;
    }
    const int lds_cells = (int)std::min<long long>(max_cells, MOT_LDS_CELLS);
    const long long spill_cells = max_cells > MOT_LDS_CELLS ? max_cells : 0;
    if (m.spill_cap < (size_t)spill_cells * n_pairs) {
        if (m.spill) { MCHK(hipFree(m.spill)); m.spill = nullptr; m.spill_cap = 0; }
        MCHK(hipMalloc((void**)&m.spill, (size_t)spill_cells * n_pairs * sizeof(double)));
        m.spill_cap = (size_t)spill_cells * n_pairs;
    }
    if (!m.attr) {
        MCHK(hipFuncSetAttribute((const void*)k_mot_hota, hipFuncAttributeMaxDynamicSharedMemorySize, MOT_LDS_CELLS * (int)sizeof(double)));
        MCHK(hipFuncSetAttribute((const void*)k_mot_clear, hipFuncAttributeMaxDynamicSharedMemorySize, MOT_LDS_CELLS * (int)sizeof(double)));
        m.attr = true;
    }
    char* d = (char*)m.dev;
    MotArgs a;
    a.gt_box = (const double*)(d + o_gbox); a.tr_box = (const double*)(d + o_tbox);
    a.s_off = (const long long*)(d + o_soff); a.pot_off = (const long long*)(d + o_poff);
    a.gt_off = (const int*)(d + o_goff); a.tr_off = (const int*)(d + o_toff); a.gt_id = (const int*)(d + o_gid); a.tr_id = (const int*)(d + o_tid);
    a.frame_off = (const int*)(d + o_foff); a.pair_of = (const int*)(d + o_pairof); a.n_tid = (const int*)(d + o_ntid);
    a.gbase = (const int*)(d + o_gbase); a.tbase = (const int*)(d + o_tbase);
    a.gid_off = (const int*)(d + o_gidoff); a.gid_rows = (const int*)(d + o_gidrows); a.gid_pair = (const int*)(d + o_gidpair);
    a.row_frame = (const int*)(d + o_rowframe); a.cnt_t = (const int*)(d + o_cntt);
    a.S = m.sim; a.si = m.sim + sim_cells;
    a.pot = (double*)(d + o_pot); a.prev_t = (int2*)(d + o_prev);
    a.clear_spill = spill_cells ? m.spill : nullptr; a.spill_cells = spill_cells;
    a.hota_idx = (int*)(d + o_hi); a.clear_idx = (int*)(d + o_ci); a.hota_s = (double*)(d + o_hs); a.clear_s = (double*)(d + o_cs);
    a.err = (int*)(d + o_err);
    a.lds_cells = lds_cells; a.n_gids = (int)nG; a.thr = thr;

    MCHK(hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, stream));
    if (o_hs > o_prev) MCHK(hipMemsetAsync(d + o_prev, 0, o_hs - o_prev, stream));        // prev_t (stamp 0: none) and pot
    MCHK(hipMemsetAsync(d + o_err, 0, sizeof(int), stream));
    if (F > 0 && Ng > 0) {
        if (sim_cells > 0) {
            hipLaunchKernelGGL(k_mot_sim, dim3((unsigned)F), dim3(256), 0, stream, a);
            MCHK(hipGetLastError());
        }
        MCHK(hipEventRecord(m.ev_sim, stream));
        MCHK(hipStreamWaitEvent(m.side, m.ev_sim, 0));
        hipLaunchKernelGGL(k_mot_clear, dim3((unsigned)n_pairs), dim3(64), (size_t)lds_cells * sizeof(double), m.side, a);
        MCHK(hipGetLastError());
        MCHK(hipEventRecord(m.ev_clear, m.side));
        if (sim_cells > 0 && nG > 0) {
            hipLaunchKernelGGL(k_mot_align, dim3((unsigned)((nG + 3) / 4)), dim3(256), 0, stream, a);
            MCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_mot_hota, dim3((unsigned)F), dim3(64), (size_t)lds_cells * sizeof(double), stream, a);
        MCHK(hipGetLastError());
        MCHK(hipStreamWaitEvent(stream, m.ev_clear, 0));
    }
    MCHK(hipMemcpyAsync(h + up, d + down_from, down, hipMemcpyDeviceToHost, stream));
    MCHK(hipEventRecord(m.ev, stream));
    MCHK(hipEventSynchronize(m.ev));
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
