// ss_common.h — shared definitions of the gfx950 StrongSORT hot path (device math + layouts).
//
// Every arithmetic helper here follows the operation order frozen in oracle/DECISIONS.md
// ("exactness contract"); the library is compiled with -ffp-contract=off so only the explicit
// fma()/fmaf()/MFMA calls fuse, exactly as in the CPU oracle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/strongsort_hip.h"
#include "ss_kalman.h"

#define SS_F 512              // feature width (OSNet)
#define SS_SEG 64             // dot-product segment (one wave of the cosine kernel per segment)
#define SS_NSEG (SS_F / SS_SEG)
#define SS_TILE 16            // MFMA 16x16 tile edge (v_mfma_f32_16x16x4_f32)
#define SS_NRT 8              // gallery row tiles per track  (capacity 128 rows >= nn_budget)
#define SS_TILE_FLOATS (SS_F * SS_TILE)   // 8192 floats = 32 KiB per (track,row tile) / (col tile)
#define SS_MAXT 256           // track slots per stream
#define SS_MAXD 128           // detections per stream per frame
#define SS_NCT (SS_MAXD / SS_TILE)
#define SS_COST_CAP 12288     // LDS-resident cost entries (f64) of the per-frame kernel; larger matrices spill to HBM
#define SS_FMAX 32            // frames of a stream that one tracker call (group) may carry
#define SS_TLMAX (SS_MAXT * SS_NRT)          // gallery tiles of a stream
#define SS_PLMAX (SS_FMAX * SS_NCT / 2)      // column-tile pairs of a stream's group
#define SS_NCTP (SS_FMAX * SS_NCT)           // packed column tiles of a stream's group at most (every detection of every frame)
#define SS_RECT 32            // gallery tiles per association work record at most (the record carries their tile words)
#define SS_RECW (4 + SS_RECT) // ints per record: {stream, frame, pair word, tiles<<16 | composite<<31} + SS_RECT words (144 bytes)
#define SS_RECI4 (SS_RECW / 4)

#define SS_TENTATIVE 1
#define SS_CONFIRMED 2
#define SS_DELETED 3

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// Fragment-major feature layout (16-row gallery tiles and 16-detection column tiles):
//   float index = ((q*4 + ks)*16 + i)*4 + c   holds element k = 16q + 4c + ks of row i of the tile
// (q = k/16, ks = k%4, c = (k%16)/4), so lane l = ks*16+i of a wave reads float4 #(q*64 + l):
// 1 KiB contiguous per wave instruction, and component c of that float4 is the A (or B) operand of
// v_mfma_f32_16x16x4_f32 number 4*(q%4)+c of k-segment q/4 — the instruction consumes k = 16q+4c+{0..3}
// in ascending order, i.e. the fmaf chain of oracle so_dot().
__host__ __device__ inline int ss_frag_index(int i, int k)
{
    return (((k >> 4) * 4 + (k & 3)) * 16 + i) * 4 + ((k & 15) >> 2);
}

struct SSParams {
    double max_dist, max_iou_distance, mc_lambda, gating_threshold, gated_cost, wp, wv;
    float ema_alpha, ema_one_minus_alpha;
    int max_age, n_init, nn_budget;
    int debug;
};

// Device-resident tracker state + per-group scratch for S streams (all pointers device memory).
// One tracker call carries a GROUP of F <= SS_FMAX consecutive frames of every stream; arrays marked [F] are indexed
// by the frame's position in the group, in the caller's layout [F][S][...].
struct SSDev {
    int S, F;
    int budget;                 // nn_budget (ring length of a gallery)
    int cos_grid;               // workgroups of the persistent association kernel
    int comp_rows;              // ragged last gallery tiles of <= comp_rows rows are cut into 4-row groups (composite tiles)
    int xcd_map;                // work-list placement: 0 a gallery range per XCD, 1 a detection column-tile pair per XCD
    int assoc_stage;            // how k_assoc stages a record's detection operand: 0 registers, 1 / 2 / 4 LDS-DMA in that many pieces
    // persistent per stream
    int *n_tracks, *next_id, *frame, *err;
    int* order;                 // [S][MAXT] slot ids in track-list order
    // persistent per slot  [S][MAXT]
    int *slot_used, *track_id, *state, *hits, *age, *tsu, *class_id, *det_idx, *gal_count, *gal_head;
    float* conf;
    double *mean, *cov;         // [S][MAXT][8], [S][MAXT][64]: a track's state after its last frame
    double *mean_p, *cov_p;     // the same PREDICTED one frame ahead (written by post_track for every live track): with pred_ahead and no
                                //   camera motion k_frame only reads the 24 values its gate needs instead of loading, predicting and storing 72
                                //   INVARIANT: post_track of the previous frame is the ONLY writer of mean_p / cov_p and the device chain the only owner of
                                //   smooth_sel.  Nothing imports track state from the host today; a path that ever writes mean / cov / smooth from outside
                                //   (track import, checkpoint restore) must also rebuild mean_p / cov_p (ss_kf_predict) and reset smooth_sel, or switch
                                //   pred_ahead off for the next frame — k_frame would otherwise gate on stale predictions without any error.
    int pred_ahead;             // ss_set_option "pred_ahead" (default 1)
    float* smooth;              // [S][MAXT][2][512] EMA feature, double-buffered: the row in use is [smooth_sel]; an update reads it and
                                //   writes the other half, so the new-row units of the SAME launch (k_postnew) can still read the old one
    int* smooth_sel;            // [S][MAXT] 0 / 1
    float* gallery;             // [S][MAXT][NRT][TILE_FLOATS]  fragment-major ring of nn_budget rows
    // group inputs / outputs (caller's buffers)
    const float* dets;          // [F][S][MAXD][6]
    const int* n_dets;          // [F][S]
    const float* feats_raw;     // [F][S][MAXD][512]
    float* out_rows;            // [F][S][MAXT][8]
    int* n_out;                 // [F][S]
    int* img_hw;                // [S][2]
    // group scratch
    float* feat_unit;           // [FMAX][S][MAXD][512]
    float* feat_frag;           // [FMAX][S][NCT][TILE_FLOATS]
    float* feat_pack;           // [S][NCTP][TILE_FLOATS] the group's detections PACKED across frames (column g = detections of the earlier
                                //   frames + d): k_assoc's B operand when assoc_pack — 28 column-tile pairs instead of 32 at ~28 det/frame
    int* colmap;                // [S][FMAX*MAXD + 64] packed column g -> frame<<8 | detection, -1 behind the last one
    int assoc_pack;             // 1: k_assoc works on packed pairs (ss_set_option "assoc_pack"), 0: pairs of one frame's column tiles
    double *tlwh, *xyah;        // [FMAX][S][MAXD][4]
    int* M;                     // [S][MAXT][FMAX][MAXD] ordered-int keys (ss_fkey) of the appearance distance
                                //   min over the gallery rows of (slot) that are valid in frame f of the group
    int2* pl;                   // [S][PLMAX] column-tile pairs of the group {frame, ct0 | two<<8 | D<<16}, by frame
    int* n_pl;                  // [S]
    int* pf;                    // [S][FMAX+1] first pair of frame f (pf[F] = n_pl)
    int4* items;                // [8][items_cap][SS_RECI4] association work records per XCD: {stream, frame, pair word, tiles<<16 |
                                //   composite<<31} + SS_RECT words: packed tiles (slot | row tile<<8 | count<<12 | ring head<<20) or, in a
                                //   composite record, 4 packed row groups per tile (slot | row tile<<8 | r4<<11 | count<<13 | head<<21);
                                //   snapshot at group start
    int items_cap;
    int* n_items;               // [8] (re-armed by k_frame)
    // per-frame hand-off k_frame -> k_post -> k_newrow
    int4* post;                 // [S][MAXT] surviving tracks in list order {slot, det or -1, flags, aux}
    int* n_post;                // [S]
    int* rowlist;               // [S][MAXT] every gallery row appended this frame: slot | first_row<<16 | smooth_sel at frame start<<17 |
                                //   matched<<18 | matched detection<<19 (the row = EMA(smooth[sel], feature of that detection), or smooth[sel] itself)
    int chain_merge;            // 1: k_post and k_newrow of a frame as ONE launch (k_postnew), 0: two launches (A/B, ss_set_option "chain_merge")
    int* n_rows;                // [S]
    const double* cmc;          // [F][S][8] camera-motion warps of the group (ss_track_set_cmc) or NULL
    double* cost_spill;         // [S][MAXT*MAXD] cost matrices that do not fit the LDS
    double* frame_scratch;      // [S][MAXT*18 + MAXD*8] k_frame's per-track / per-detection f64 work arrays when they exceed cap_t / cap_d
    int cap_cost, cap_t, cap_d; // what k_frame keeps in LDS: cost entries, tracks, detections (ss_set_option "frame_caps")
    unsigned long long* tstamp; // [4] in-kernel timing of the association kernel: min start, max end (100 MHz), sum, count
    int ts_enable;              // 1: first-start / last-end stamps; 2: + per-workgroup timeline
    long long* timeline;        // [4096 workgroups][16] stamps of each workgroup's first item (profiling aid)
    // debug (stage intermediates, per frame of the group)
    float* dbg_cos;             // [FMAX][S][MAXT][MAXD]
    double *dbg_maha, *dbg_cost_a, *dbg_cost_b;
    uint8_t* dbg_gated;
    int* dbg_lists;             // [FMAX][S][4][MAXT]: pairs_a(det per conf row), cand, cols_b, pairs_b
    int* dbg_counts;            // [FMAX][S][4]: n_conf, n_cand, n_cols, n_dets
};

// post[] flags
#define SS_P_MATCHED 1          // Kalman update + EMA with detection .y
#define SS_P_BIRTH 2            // new track from detection .y
#define SS_P_APPEND 4           // append the EMA feature at ring position aux & 0xff
#define SS_P_FIRSTROW 8         // ... and it is the gallery's first row
#define SS_P_EMIT 16            // output row number aux >> 8

// order-preserving int image of a float (signed compare == float compare, also for negative values)
__host__ __device__ inline int ss_fkey(float v)
{
    union { float f; int i; } u; u.f = v;
    return u.i ^ ((u.i >> 31) & 0x7fffffff);
}
__host__ __device__ inline float ss_fkey_inv(int k)
{
    union { float f; int i; } u; u.i = k ^ ((k >> 31) & 0x7fffffff);
    return u.f;
}
#define SS_KEY_INF 0x7f800000

// ---------------------------------------------------------------------------------------------
// wave helpers
// ---------------------------------------------------------------------------------------------
#define SS_WAVE_SYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

__device__ inline float ss_wave_sumsq_reduce(float p)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_xor(p, off);
    return p;
}

// Unit feature of a 512-float row held by a wave, lane l = elements l + 64 j (oracle so_normalize): every lane chains fmaf over its
// eight elements, the xor butterfly adds the lanes, sqrtf (ss_norm8); then every element is divided — or zero for an all-zero row,
// D-17 (ss_unit_elem).  ss_unit8 -> out[l + 64 j] (LDS or global); a caller that stores an element more than once uses the two parts.
__device__ __forceinline__ float ss_norm8(const float v[8])
{
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = fmaf(v[j], v[j], acc);
    return sqrtf(ss_wave_sumsq_reduce(acc));
}
__device__ __forceinline__ float ss_unit_elem(float v, float n) { return n > 0.0f ? v / n : 0.0f; }
__device__ __forceinline__ void ss_unit8(const float v[8], float* out)
{
    const int l = threadIdx.x & 63;
    const float n = ss_norm8(v);
#pragma unroll
    for (int j = 0; j < 8; ++j) out[l + 64 * j] = ss_unit_elem(v[j], n);
}

// oracle so_ema of a smoothed row sv and a unit feature fv in registers (lane l = elements l + 64 j): a * sv + b * fv, then its unit row
__device__ __forceinline__ void ss_ema_regs(const float sv[8], const float fv[8], float a, float b, float* out)
{
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float t1 = a * sv[j];
        const float t2 = b * fv[j];
        v[j] = t1 + t2;
    }
    ss_unit8(v, out);
}

// ---------------------------------------------------------------------------------------------
// block helpers (256 threads)
// ---------------------------------------------------------------------------------------------
// Flag scans: position of a thread's flag among the set ones, and their number.  block_scan256_3 is three independent scans for the
// price of one (two barriers; k_frame ran ten scans of two barriers each: 20 of its ~30 barriers); block_scan256 is the same code
// for one flag, with 4 instead of 12 ints of LDS.
__device__ inline void block_scan256(int flag, int* wtot /*LDS[4]*/, int& pos, int& total)
{
    unsigned long long m = __ballot(flag);
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inwave = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                       // protect wtot from the previous scan's readers
    if (lane == 0) wtot[w] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { int c = wtot[i]; if (i < w) off += c; tot += c; }
    pos = off + inwave;
    total = tot;
}

__device__ inline void block_scan256_3(int f0, int f1, int f2, int* wtot /*LDS[12]*/, int& p0, int& p1, int& p2, int& t0, int& t1, int& t2)
{
    const unsigned long long m0 = __ballot(f0), m1 = __ballot(f1), m2 = __ballot(f2);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int i0 = __popcll(m0 & below), i1 = __popcll(m1 & below), i2 = __popcll(m2 & below);
    __syncthreads();                       // protect wtot from the previous scan's readers
    if (lane == 0) { wtot[w] = __popcll(m0); wtot[4 + w] = __popcll(m1); wtot[8 + w] = __popcll(m2); }
    __syncthreads();
    int o0 = 0, o1 = 0, o2 = 0, s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c0 = wtot[i], c1 = wtot[4 + i], c2 = wtot[8 + i];
        if (i < w) { o0 += c0; o1 += c1; o2 += c2; }
        s0 += c0; s1 += c1; s2 += c2;
    }
    p0 = o0 + i0; p1 = o1 + i1; p2 = o2 + i2;
    t0 = s0; t1 = s1; t2 = s2;
}

// exclusive prefix sum of small non-negative ints over the 256 threads of a block
__device__ inline void block_scan_sum256(int v, int* wtot /*LDS[4]*/, int& excl, int& total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { int t = __shfl_up(inc, off); if (lane >= off) inc += t; }
    __syncthreads();
    if (lane == 63) wtot[w] = inc;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { int c = wtot[i]; if (i < w) off += c; tot += c; }
    excl = off + inc - v;
    total = tot;
}

// ---------------------------------------------------------------------------------------------
// Kalman filter (float64): the thread forms, the noise model and the gain row are in ss_kalman.h; here the wave-cooperative
// forms of the xyah filter (StrongSORT's post_track), lane l = covariance entry (r, c) = (l >> 3, l & 7).  Every lane performs
// exactly the operations the thread form performs for its entry, so every result bit equals the one-thread form.
// ---------------------------------------------------------------------------------------------
// ss_kf_initiate<false>: -> gmean / gcov (global) and ws = 72 doubles of per-wave LDS (covariance, then mean)
__device__ inline void ss_kf_initiate_wave(const double* z, double wp, double wv, double* gmean, double* gcov, double* ws)
{
    const int l = threadIdx.x & 63, r = l >> 3, c = l & 7;
    const double sd = ss_kf_sd_initiate<false>(r, wp, wv, z);
    const double c0 = (r == c) ? sd * sd : 0.0;
    gcov[l] = c0; ws[l] = c0;
    if (l < 8) { const double m0 = (l < 4) ? z[l] : 0.0; gmean[l] = m0; ws[64 + l] = m0; }
}

// ss_kf_update<false>: the gain rows r and c, column c of S K^T.  The new state goes to gmean / gcov and is left in ws
// (covariance in ws[0..63], mean in ws[64..71]).  imean / icov: the state it starts from — gmean / gcov, or the predicted copies.
__device__ inline void ss_kf_update_wave(const double* imean, const double* icov, double* gmean, double* gcov, const double z[4], double conf,
                                         double wp, double* ws)
{
    const int l = threadIdx.x & 63, r = l >> 3, c = l & 7;
    const double p = icov[l];
    ws[l] = p;
    if (l < 8) ws[64 + l] = imean[l];
    SS_WAVE_SYNC();
    const double* cov = ws;
    const double* mean = ws + 64;
    double m4[4], S[16], L[16];
    ss_kf_project<false>(mean, cov, conf, wp, m4, S);
    ss_chol4(S, L);
    double Kr[4], Kc[4];
    ss_kf_gain_row(L, cov + r * 8, Kr);
    ss_kf_gain_row(L, cov + c * 8, Kc);
    double Mc[4];                                   // column c of M = S K^T
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc = fma(S[i * 4 + k], Kc[k], acc);
        Mc[i] = acc;
    }
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc = fma(Kr[k], Mc[k], acc);
    const double mr = mean[r];
    double a2 = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) a2 = fma(z[k] - m4[k], Kr[k], a2);
    SS_WAVE_SYNC();                                 // every lane has read the old state
    const double pn = p - acc;
    gcov[l] = pn;
    ws[l] = pn;
    if (c == 0) { const double nm = mr + a2; gmean[r] = nm; ws[64 + r] = nm; }
    SS_WAVE_SYNC();
}

// ss_kf_predict<false> of the state in ws (A = P F^T on the left half, B = F A on the top half, + Q on the diagonal; the noise from
// the mean BEFORE the step).  -> pmean[8], pcov[64] (global).
__device__ inline void ss_kf_predict_wave(const double* ws, double wp, double wv, double* pmean, double* pcov)
{
    const int l = threadIdx.x & 63, i = l >> 3, j = l & 7;
    const double* P = ws;
    const double* mean = ws + 64;
    double a = P[i * 8 + j];
    if (j < 4) a = a + P[i * 8 + j + 4];
    if (i < 4) {
        double a4 = P[(i + 4) * 8 + j];
        if (j < 4) a4 = a4 + P[(i + 4) * 8 + j + 4];
        a = a + a4;
    }
    if (i == j) {
        const double sd = ss_kf_sd_predict<false>(i, wp, wv, mean);
        a = a + sd * sd;
    }
    pcov[l] = a;
    if (l < 8) pmean[l] = l < 4 ? mean[l] + mean[l + 4] : mean[l];
}

// Device state of the BYTE tracker family (csrc/ss_byte.hip), hung off a context by ss_byte_create.  Per stream: two ordered
// lists of slots (tracked = activated and unconfirmed tracks, lost), per slot the track's fields; all pointers device memory.
#define SS_BYTE_TRACKED 1
#define SS_BYTE_LOST 2
#define SS_BYTE_REMOVED 3
#define SS_BYTE_MAXK 32                 // keypoints per row: one visibility word, one lane of a half wave each
struct SSByteDev {
    int S;
    int xywh, fuse, max_time_lost, max_tracks, max_dets;
    float high, low, new_thresh;        // score thresholds, compared in float32 (B-04)
    double match, wp, wv;
    int *frame, *next_id, *err;         // [S]
    int *n_trk, *n_lost;                // [S]
    int *trk, *lost;                    // [S][MAXT] slots in list order
    int *state, *act, *tid, *start, *end, *len, *det;    // [S][MAXT] by slot
    float *score, *cls;                 // [S][MAXT]
    double *mean, *cov;                 // [S][MAXT][8], [S][MAXT][64]
    double* spill;                      // [S][MAXT * MAXD] cost matrices that do not fit the LDS
    const double* gmc;                  // [F][S][8] BoT-SORT GMC warps (ss_byte_set_gmc, xywh only), NULL: off
    // the keypoint term (docs/BYTETRACK.md §1e, ss_byte_set_pose; xywh only, not with ReID), allocated when first switched on
    int pose, nk, min_common;           // on / keypoints per row (1..SS_BYTE_MAXK) / fewest keypoints visible on both sides
    float vis;                          // (float)kpt_vis_thresh, compared in float32
    double pose_thresh;                 // on (1 - OKS) / 2; the proximity mask is `prox` above
    const double* ks2;                  // [SS_BYTE_MAXK] 2 sigma_k (device memory: the argument struct stays small)
    double* tpose;                      // [S][MAXT][nk][2] track poses by slot: offsets from the box centre in box widths / heights
    unsigned* tvis;                     // [S][MAXT] bit k: keypoint k of the track's pose is visible
    float* kp;                          // [FMAX][S][MAXD][nk][2] the group's detection keypoints in original pixels (k_byte_kpts)
    unsigned* kvis;                     // [FMAX][S][MAXD] bit k: keypoint k of the row is visible
    // BoT-SORT's ReID branch (docs/BYTETRACK.md §1c, ss_byte_set_reid; xywh only), allocated when first switched on
    int reid;
    float alpha, one_minus_alpha;       // so_ema weights: (float)alpha, (float)(1 - alpha)
    double prox, appear;                // proximity_thresh (on 1 - IoU), appearance_thresh (on the halved cosine distance)
    float* smooth;                      // [S][MAXT][F] unit track features by slot
    float* ufeat;                       // [FMAX][S][MAXD][F] unit detection features of the group (k_byte_feats)
    // oriented boxes (docs/OBB.md §4, ss_byte_set_obb; not with GMC, ReID or the keypoint term), allocated when first switched on
    int obb;
    float* angle;                       // [S][MAXT] by slot: the angle of the track's last detection (R-06)
    double* tbox;                       // [S][MAXT][6] by slot: ProbIoU terms (x, y, A, B, C, D) of the track's current box
    double* dbox;                       // [S][MAXD][6] the same of the frame's detection rows
    float* rbox;                        // [F][S][MAXT][5] the call's d_out_rbox (set by the launcher on its copy of this struct)
};

// Device state of the OC-SORT tracker (csrc/ss_ocsort.hip, docs/OCSORT.md), hung off a context by ss_ocsort_create.  Per stream: one
// ordered list of slots, per slot the track's fields; all pointers device memory.
#define SS_OC_MAXDT 8                   // largest delta_t: the depth of a track's ring of observations
struct SSOcDev {
    int S;
    int max_age, min_hits, delta_t, use_byte, max_tracks, max_dets;
    float det_thresh, low_thresh;       // score thresholds, compared in float32
    double iou_thr, inertia;
    int *frame, *next_id, *err, *n_trk; // [S]
    int* trk;                           // [S][MAXT] slots in list order
    int *tid, *age, *tsu, *hits, *streak, *hasobs, *obsd, *frozen, *det;     // [S][MAXT] by slot
    float *score, *cls;                 // [S][MAXT]
    float* lobs;                        // [S][MAXT][4] last observation (the birth row while hasobs is 0)
    float* ring;                        // [S][MAXT][SS_OC_MAXDT][4] observations, entry age % delta_t
    int* rage;                          // [S][MAXT][SS_OC_MAXDT] the age an entry was stored at, -1: empty
    double* vel;                        // [S][MAXT][2] unit velocity (x, y); zero: none
    double *x, *P, *xf, *Pf;            // [S][MAXT][7], [S][MAXT][49]: the filter and its frozen copy
    double* spill;                      // [S][MAXT * MAXD] cost matrices that do not fit the LDS
};

// Device state of the Deep OC-SORT tracker (csrc/ss_deepoc.hip, docs/DEEPOCSORT.md), hung off a context by ss_deepoc_create: an OC-SORT
// state of its own (use_byte 0) and what the appearance and camera-motion steps add.
struct SSDeepOcDev {
    SSOcDev oc;
    int appearance, dynamic, adaptive;  // 0 / 1
    double det_thresh;                  // the f64 threshold of the score's trust (oc.det_thresh is its float32 value for the split)
    double w_emb, alpha_fixed, aw;      // w_association_emb, alpha_fixed_emb, aw_param
    float* emb;                         // [S][MAXT][F] unit track features by slot
    float* ufeat;                       // [FMAX][S][MAXD][F] unit features of the group's high rows (k_deepoc_feats)
    double* E;                          // [S][MAXD * MAXT] the first association's similarities, row-major rows x tracks
    const double* gmc;                  // [F][S][8] warps (ss_deepoc_set_gmc), NULL: off
};

// Device state of the Hybrid-SORT tracker (csrc/ss_hybrid.hip, docs/HYBRIDSORT.md), hung off a context by ss_hybridsort_create.  The
// list and slot fields are OC-SORT's; the filter is kept as its five independent components (H-02).
#define SS_HY_FLT 26                    // doubles per filter: [p, v, P00, P01, P10, P11] of x, y, s, c, then r and its variance
struct SSHyDev {
    int S;
    int max_age, min_hits, delta_t, use_byte, hmiou, max_tracks, max_dets;
    float det_thresh, low_thresh;       // score thresholds of the split, compared in float32
    double det_thr64, low_thr64;        // the same as configured: the bounds of the two confidences
    double iou_thr, inertia, tcm_first, tcm_byte;
    int *frame, *next_id, *err, *n_trk; // [S]
    int* trk;                           // [S][MAXT] slots in list order
    int *tid, *age, *tsu, *hits, *streak, *hasobs, *obsd, *frozen, *det, *hasprev;   // [S][MAXT] by slot
    float *score, *cls, *cprev;         // [S][MAXT]; score is the confidence of the last match, cprev of the one before (hasprev)
    float* lobs;                        // [S][MAXT][4] last observation (the birth row while hasobs is 0)
    float* ring;                        // [S][MAXT][SS_OC_MAXDT][4] observations, entry age % delta_t
    int* rage;                          // [S][MAXT][SS_OC_MAXDT] the age an entry was stored at, -1: empty
    double* vel;                        // [S][MAXT][8] the corners' velocities (lt, rt, lb, rb; x, y); zero: none
    double *flt, *fltf;                 // [S][MAXT][SS_HY_FLT] the filter and its frozen copy
    double* spill;                      // [S][MAXT * MAXD] cost matrices that do not fit the LDS
};

// Device state of the sparse-optical-flow camera-motion estimator (csrc/ss_gmc.hip, docs/BYTETRACK.md §1f), hung off a context by
// the first ss_gmc_sparse_estimate call for a frame size.  Image slot 0 of a stream is the remembered frame, slots 1..F the group's.
#define SS_GMC_MAXC 1000                // corners per image (S-05)
#define SS_GMC_LEVELS 4                 // pyramid levels 0..3 (S-03)
#define SS_GMC_MIN_SIDE 64              // smallest frame side: level 3 is at least 4 x 4
struct SSGmcDev {
    int S, h, w;                        // streams, frame size
    int lw[SS_GMC_LEVELS], lh[SS_GMC_LEVELS];
    long long loff[SS_GMC_LEVELS];      // byte offset of a level inside an image's pyramid
    long long pyr_stride;               // bytes per pyramid (multiple of 16)
    uint8_t* pyr;                       // [FMAX+1][S][pyr_stride] grey half image and its three lower levels
    float* eig;                         // [FMAX][S][lw0*lh0] smaller eigenvalue per pixel
    unsigned* cand;                     // [FMAX][S][lw0*lh0] its bits where the pixel is a corner candidate, else 0
    unsigned* emax;                     // [FMAX][S] bits of the image's largest eigenvalue
    int *corners, *ncorner, *ncand;     // [FMAX+1][S][MAXC] pixel indices in order, [FMAX+1][S] kept, [FMAX+1][S] candidates
    double* pts;                        // [FMAX][S][MAXC][2] tracked corners of the previous image, half-size pixels
    uint8_t *status, *inlier;           // [FMAX][S][MAXC]
    int* prev_valid;                    // [S] the stream has a remembered frame
    int* last;                          // slot of the last real frame of the previous call (0: none new)
};

// camera-motion warp m (2x3, full-frame pixels) applied to a track's box (oracle so_camera_update, D-18)
__device__ inline void ss_camera_update(double* mean, const double* m)
{
    const double w = mean[2] * mean[3], h = mean[3];
    const double x1 = mean[0] - w / 2, y1 = mean[1] - h / 2, x2 = x1 + w, y2 = y1 + h;
    const double ax = (m[0] * x1 + m[1] * y1) + m[2], ay = (m[3] * x1 + m[4] * y1) + m[5];
    const double bx = (m[0] * x2 + m[1] * y2) + m[2], by = (m[3] * x2 + m[4] * y2) + m[5];
    const double nw = bx - ax, nh = by - ay;
    mean[0] = ax + nw / 2; mean[1] = ay + nh / 2; mean[2] = nw / nh; mean[3] = nh;
}

// gate + blend + threshold of one entry (oracle so_blend)
__device__ inline double ss_blend(float cosd, double maha, const SSParams& p, int* gated)
{
    double oml = 1.0 - p.mc_lambda, repl = p.max_dist + 1e-5;
    int g = maha > p.gating_threshold;
    double c = g ? p.gated_cost : (double)cosd;
    double t1 = p.mc_lambda * c, t2 = oml * maha;
    double v = t1 + t2;
    if (v > p.max_dist) v = repl;
    *gated = g;
    return v;
}

// IoU cost of one (track tlwh, det tlwh) pair (oracle so_iou_cost)
__device__ inline double ss_iou_cost(const double t[4], const double c[4], double max_dist)
{
    double repl = max_dist + 1e-5;
    double tbr0 = t[0] + t[2], tbr1 = t[1] + t[3], tarea = t[2] * t[3];
    double cbr0 = c[0] + c[2], cbr1 = c[1] + c[3];
    double tl0 = fmax(t[0], c[0]), tl1 = fmax(t[1], c[1]);
    double br0 = fmin(tbr0, cbr0), br1 = fmin(tbr1, cbr1);
    double w = fmax(0.0, br0 - tl0), h = fmax(0.0, br1 - tl1);
    double inter = w * h, carea = c[2] * c[3];
    double iou = inter / (tarea + carea - inter);
    double v = 1.0 - iou;
    if (v > max_dist) v = repl;
    return v;
}
