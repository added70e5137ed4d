// ss_aflink.hip — AFLink, the tracklet-linking half of StrongSORT++'s post-processing (docs/AFLINK.md), on the device.
//
//   k_afl_gate<false> / k_afl_scan / k_afl_gate<true>   the gate over n x n tracklet ends: one wave per earlier tracklet i counts
//                     its later partners j, one wave scans the counts, one wave per i fills its slice in rising j (ballot ranks, no
//                     atomic cursor): the list is row-major and the same on every run.  f64, no fma (the file is built
//                     -ffp-contract=off).  A pair also needs (first frame, number) of i below that of j: the links cannot form a cycle.
//   k_afl_prep        per (pair, column): gather the last 30 rows of i and the first 30 of j, pad with zeros, min / max over the 60,
//                     (v - (max + min) / 2) / ((max - min) / 2 + 1e-5) in f64, rounded to f32 once.
//   k_afl_l1          the first temporal layer (1 -> 32 channels, K = 7: too thin for the matrix cores) + BatchNorm + ReLU on VALU.
//   k_afl_gemm        the three wide temporal layers and the fusion layer as f32 GEMMs on v_mfma_f32_16x16x4_f32 over all pairs of
//                     a chunk: GEMM row = (pair, column, step) of a channel-last activation [pair][column][step][cin], whose K =
//                     7 cin inputs are contiguous there (no im2col buffer); the fourth layer writes [pair][step][column][256] so the
//                     fusion layer's K = 3 x 256 is contiguous too.  Epilogue: per-(column, channel) scale and bias, ReLU.
//   k_afl_head        per pair: mean over the 6 steps, Linear(512, 128) + ReLU, Linear(128, 2), softmax in f64, cost = 1 - p[1].
//   k_afl_match       one wave per connected component of the surviving pairs: lsap_wave (ss_lsap.h) on the component's matrix.
//
// Operand convention of the GEMM (as ss_ops32.hip): lane (kq = lane >> 4, n = lane & 15) reads the 16-byte chunk kq + 4 jj of row n
// of a 64-wide K slab; component s of it is k-slot kq of MFMA (jj, s) for both operands.  A = weights [cout][K] (M = output channel),
// B = activation rows (N = GEMM row), so lane (q, n) ends with output channels 16 ct + 4 q .. + 3 of row n: one 16-byte store.
// Sums are f32 in a fixed order: a call is reproducible; the order is not PyTorch's, so costs agree to rounding (docs/AFLINK.md §5).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>
#include "ss_common.h"
#include "ss_host.h"
#include "ss_launch.h"
#include "ss_lsap.h"

#define AFL_LEN 30              // rows of a tracklet the network sees
#define AFL_MAX_TRACKLETS 65535
#define AFL_MAX_COMPONENT 256   // lsap_wave's side
#define AFL_BM 64               // GEMM rows per workgroup
#define AFL_BK 64               // K slab
#define AFL_PITCH 72            // LDS row pitch in floats: 16-byte reads of lane (kq, n) at 8 n + 4 kq (mod 64 banks) do not collide
#define AFL_FILL 1e5            // upstream's cost of a cell that is no surviving pair

// blob layout in floats (docs/AFLINK.md §3); per branch: w1 [32][7], sb1 [2][3][32], w2 [64][7*32], sb2 [2][3][64], w3 [128][7*64],
// sb3 [2][3][128], w4 [256][7*128], sb4 [2][3][256], wf [256][3*256], sbf [2][256];  then fc1^T [512][128], b1 [128], fc2 [2][128], b2 [2]
#define AFL_O_W1 0
#define AFL_O_SB1 (AFL_O_W1 + 32 * 7)
#define AFL_O_W2 (AFL_O_SB1 + 2 * 3 * 32)
#define AFL_O_SB2 (AFL_O_W2 + 64 * 224)
#define AFL_O_W3 (AFL_O_SB2 + 2 * 3 * 64)
#define AFL_O_SB3 (AFL_O_W3 + 128 * 448)
#define AFL_O_W4 (AFL_O_SB3 + 2 * 3 * 128)
#define AFL_O_SB4 (AFL_O_W4 + 256 * 896)
#define AFL_O_WF (AFL_O_SB4 + 2 * 3 * 256)
#define AFL_O_SBF (AFL_O_WF + 256 * 768)
#define AFL_BRANCH (AFL_O_SBF + 2 * 256)
#define AFL_O_FC1 (2 * AFL_BRANCH)
#define AFL_O_B1 (AFL_O_FC1 + 512 * 128)
#define AFL_O_FC2 (AFL_O_B1 + 128)
#define AFL_O_B2 (AFL_O_FC2 + 2 * 128)
#define AFL_FLOATS (AFL_O_B2 + 2)
// activations of a chunk, floats per pair: x [2][30][3]; buffer A holds layer 1 [2][3][24][32], then layer 3 [2][3][12][128], then the
// fusion output [2][6][256]; buffer B holds layer 2 [2][3][18][64], then layer 4 [2][6][3][256]
#define AFL_X_FLOATS (2 * AFL_LEN * 3)
#define AFL_BUF_FLOATS 9216

int g_opt_aflink_chunk = 1024;  // ss_op_set_option "aflink_chunk": pairs per pass of the network (the scratch follows it)

typedef float afl4 __attribute__((ext_vector_type(4)));
static __device__ __forceinline__ afl4 afl_ld4(const float* p) { return *reinterpret_cast<const afl4*>(p); }
static __device__ __forceinline__ void afl_st4(float* p, const afl4 v) { *reinterpret_cast<afl4*>(p) = v; }

// ---- gate ---------------------------------------------------------------------------------------------------------------------
struct AflGate {
    const int* offsets;         // [n + 1]
    const double* feats;        // [rows][3]: frame, x1, y1
    long long* row_off;         // [n + 1]: counts, then their exclusive scan
    int* pair_i;
    int* pair_j;
    double thr_s;
    int t0, t1, n;
};

static __device__ __forceinline__ bool afl_gate(const AflGate& a, int i, long long first_i, long long fi, double xi, double yi, int j)
{
    if (j >= a.n || j == i) return false;
    const double* fj = a.feats + (size_t)a.offsets[j] * 3;
    const long long first_j = (long long)fj[0];
    if (first_i > first_j || (first_i == first_j && i > j)) return false;       // i starts first (ties: the smaller number): no cycles
    const long long gap = first_j - fi;
    if (gap < a.t0 || gap >= a.t1) return false;
    const double dx = fj[1] - xi, dy = fj[2] - yi;
    return sqrt(dx * dx + dy * dy) <= a.thr_s;
}

template <bool FILL>
__global__ __launch_bounds__(64) void k_afl_gate(const AflGate a)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    const double* li = a.feats + (size_t)(a.offsets[i + 1] - 1) * 3;
    const long long fi = (long long)li[0], first_i = (long long)a.feats[(size_t)a.offsets[i] * 3];
    const double xi = li[1], yi = li[2];
    long long at = FILL ? a.row_off[i] : 0;
    for (int j0 = 0; j0 < a.n; j0 += 64) {
        const bool ok = afl_gate(a, i, first_i, fi, xi, yi, j0 + lane);
        const unsigned long long b = __ballot(ok);
        if (FILL && ok) {
            const long long k = at + __popcll(b & ((1ull << lane) - 1ull));
            a.pair_i[k] = i;
            a.pair_j[k] = j0 + lane;
        }
        at += __popcll(b);
    }
    if (!FILL && lane == 0) a.row_off[i] = at;
}

// one wave: row_off[0 .. n) counts -> exclusive scan, row_off[n] = total
__global__ __launch_bounds__(64) void k_afl_scan(long long* row_off, int n)
{
    const int lane = threadIdx.x;
    long long base = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const long long c = i0 + lane < n ? row_off[i0 + lane] : 0;
        long long s = c;
        for (int d = 1; d < 64; d <<= 1) {
            const long long o = __shfl_up(s, d);
            if (lane >= d) s += o;
        }
        if (i0 + lane < n) row_off[i0 + lane] = base + s - c;
        base += __shfl(s, 63);
    }
    if (lane == 0) row_off[n] = base;
}

// ---- input transform ----------------------------------------------------------------------------------------------------------
// thread = (pair of the chunk, column).  x [pair][branch][30][3] f32
__global__ __launch_bounds__(256) void k_afl_prep(const int* __restrict__ offsets, const double* __restrict__ feats, const int* __restrict__ pair_i,
                                                  const int* __restrict__ pair_j, float* __restrict__ x, int n_pairs)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_pairs * 3) return;
    const int p = e / 3, c = e - p * 3;
    const int i = pair_i[p], j = pair_j[p];
    const int i1 = offsets[i + 1], ni = min(i1 - offsets[i], AFL_LEN);          // rows i1 - ni .. i1 - 1, padded in front
    const int j0 = offsets[j], nj = min(offsets[j + 1] - j0, AFL_LEN);          // rows j0 .. j0 + nj - 1, padded behind
    const double* __restrict__ a = feats + (size_t)(i1 - ni) * 3 + c;
    const double* __restrict__ b = feats + (size_t)j0 * 3 + c;
    double mn = a[0], mx = a[0];
    for (int r = 0; r < ni; ++r) { const double v = a[(size_t)r * 3]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    for (int r = 0; r < nj; ++r) { const double v = b[(size_t)r * 3]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    if (ni < AFL_LEN || nj < AFL_LEN) { mn = 0.0 < mn ? 0.0 : mn; mx = 0.0 > mx ? 0.0 : mx; }
    const double mid = (mx + mn) / 2.0, half = (mx - mn) / 2.0 + 1e-5;
    float* __restrict__ xo = x + (size_t)p * AFL_X_FLOATS + c;
    for (int r = 0; r < AFL_LEN; ++r) {
        const double v = r >= AFL_LEN - ni ? a[(size_t)(r - (AFL_LEN - ni)) * 3] : 0.0;
        xo[r * 3] = (float)((v - mid) / half);
    }
    for (int r = 0; r < AFL_LEN; ++r) {
        const double v = r < nj ? b[(size_t)r * 3] : 0.0;
        xo[(AFL_LEN + r) * 3] = (float)((v - mid) / half);
    }
}

// ---- layer 1: 1 -> 32 channels, kernel 7 along time, on VALU ---------------------------------------------------------------------
// thread = (branch, pair, column, step, 4 channels);  out [branch][pair][column][24][32]
__global__ __launch_bounds__(256) void k_afl_l1(const float* __restrict__ x, const float* __restrict__ blob, float* __restrict__ out, int n_pairs)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long per_branch = (long long)n_pairs * 3 * 24 * 8;
    if (e >= 2 * per_branch) return;
    const int br = (int)(e / per_branch);
    const long long r = e - br * per_branch;
    const int c4 = (int)(r & 7);
    const long long row = r >> 3;                                               // (pair, column, step)
    const int t = (int)(row % 24), col = (int)((row / 24) % 3);
    const long long p = row / 72;
    const float* __restrict__ w = blob + (size_t)br * AFL_BRANCH + AFL_O_W1 + c4 * 4 * 7;
    const float* __restrict__ sb = blob + (size_t)br * AFL_BRANCH + AFL_O_SB1;
    const float* __restrict__ xi = x + (size_t)p * AFL_X_FLOATS + br * AFL_LEN * 3 + t * 3 + col;
    afl4 acc = { 0.f, 0.f, 0.f, 0.f };
#pragma unroll
    for (int dt = 0; dt < 7; ++dt) {
        const float v = xi[dt * 3];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = __builtin_fmaf(w[s * 7 + dt], v, acc[s]);
    }
    const afl4 sc = afl_ld4(sb + col * 32 + c4 * 4), bi = afl_ld4(sb + 96 + col * 32 + c4 * 4);
    afl4 v = acc * sc + bi;
#pragma unroll
    for (int s = 0; s < 4; ++s) v[s] = v[s] > 0.f ? v[s] : 0.f;
    afl_st4(out + ((size_t)br * n_pairs * 72 + (size_t)row) * 32 + c4 * 4, v);
}

// ---- the wide layers: out[row][0 .. N) = relu(scale * (W in[row][0 .. K)) + bias) ---------------------------------------------------
// MODE 0: temporal layer, row = (pair, column, step of TOUT), the K = 7 CIN inputs start at step `step` of [pair][column][TIN][CIN];
//         out [pair][column][TOUT][N].   MODE 1: the same rows, out [pair][TOUT][column][N] (layer 4).
// MODE 2: fusion layer, row = (pair, step), in [pair][6][3][256] (K = 768), out [pair][6][N], one scale / bias set.
// grid (row tiles of 64, N / BN, branch); 4 waves: wave (wr, wc) owns rows 32 wr .. + 31 and channels BN / 2 wc .. + BN / 2 - 1.
template <int CIN, int N, int BN, int TIN, int TOUT, int MODE>
__global__ __launch_bounds__(256) void k_afl_gemm(const float* __restrict__ in, const float* __restrict__ blob, float* __restrict__ out, int n_pairs,
                                                  int o_w, int o_sb)
{
    constexpr int K = MODE == 2 ? 3 * CIN : 7 * CIN, NK = (K + AFL_BK - 1) / AFL_BK, CT = BN / 32;
    constexpr int RPP = MODE == 2 ? TOUT : 3 * TOUT;                            // GEMM rows per pair
    constexpr int IN_PP = 3 * TIN * CIN, WL = BN * 16 / 256;                    // input floats per pair; weight vectors a thread stages
    static_assert(K % 4 == 0 && N % BN == 0 && (BN == 64 || BN == 128), "tile shapes");
    __shared__ __attribute__((aligned(16))) float As[AFL_BM * AFL_PITCH];
    __shared__ __attribute__((aligned(16))) float Ws[BN * AFL_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4, n = lane & 15;
    const int wr = wave & 1, wc = wave >> 1, br = blockIdx.z, n0 = blockIdx.y * BN;
    const long long M = (long long)n_pairs * RPP, m0 = (long long)blockIdx.x * AFL_BM;
    const float* __restrict__ inb = in + (size_t)br * n_pairs * IN_PP;
    const float* __restrict__ W = blob + (size_t)br * AFL_BRANCH + o_w + (size_t)n0 * K;
    const float* __restrict__ sb = blob + (size_t)br * AFL_BRANCH + o_sb;
    float* __restrict__ outb = out + (size_t)br * n_pairs * RPP * N;

    // what this thread stages: 4 vectors of the rows' slab (row = (tid + 256 u) >> 4, chunk = tid & 15), WL of the weights'
    const int ch = tid & 15;
    const float* arow[4];
    bool aval[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long long r = m0 + ((tid + 256 * u) >> 4);
        aval[u] = r < M;
        const long long rc = aval[u] ? r : 0;
        if constexpr (MODE == 2) arow[u] = inb + (size_t)rc * K;
        else {
            const long long p = rc / RPP;
            const int rem = (int)(rc - p * RPP), col = rem / TOUT, t = rem - col * TOUT;
            arow[u] = inb + (size_t)p * IN_PP + (size_t)(col * TIN + t) * CIN;
        }
    }
    afl4 ra[4], rw[WL];
    auto fetch = [&](int k0) {
        const bool kin = k0 + 4 * ch < K;
#pragma unroll
        for (int u = 0; u < 4; ++u) ra[u] = (aval[u] && kin) ? afl_ld4(arow[u] + k0 + 4 * ch) : afl4{ 0.f, 0.f, 0.f, 0.f };
#pragma unroll
        for (int u = 0; u < WL; ++u) rw[u] = kin ? afl_ld4(W + (size_t)((tid + 256 * u) >> 4) * K + k0 + 4 * ch) : afl4{ 0.f, 0.f, 0.f, 0.f };
    };
    afl4 acc[CT][2];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) { acc[ct][0] = afl4{ 0.f, 0.f, 0.f, 0.f }; acc[ct][1] = afl4{ 0.f, 0.f, 0.f, 0.f }; }
    fetch(0);
    for (int ks = 0; ks < NK; ++ks) {
#pragma unroll
        for (int u = 0; u < 4; ++u) afl_st4(As + ((tid + 256 * u) >> 4) * AFL_PITCH + 4 * ch, ra[u]);
#pragma unroll
        for (int u = 0; u < WL; ++u) afl_st4(Ws + ((tid + 256 * u) >> 4) * AFL_PITCH + 4 * ch, rw[u]);
        __syncthreads();
        if (ks + 1 < NK) fetch((ks + 1) * AFL_BK);                              // the next slab travels while this one is multiplied
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            if (ks * AFL_BK + 16 * jj >= K) break;                              // (uniform: the ragged last slab of K = 224)
            afl4 b[2], a[CT];
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) b[rt] = afl_ld4(As + (32 * wr + 16 * rt + n) * AFL_PITCH + 4 * (kq + 4 * jj));
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) a[ct] = afl_ld4(Ws + (BN / 2 * wc + 16 * ct + n) * AFL_PITCH + 4 * (kq + 4 * jj));
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt) acc[ct][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ct][s], b[rt][s], acc[ct][rt], 0, 0, 0);
        }
        __syncthreads();
    }
    // epilogue: lane (kq, n) holds channels n0 + BN / 2 wc + 16 ct + 4 kq .. + 3 of row m0 + 32 wr + 16 rt + n
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const long long r = m0 + 32 * wr + 16 * rt + n;
        if (r >= M) continue;
        int col = 0;
        size_t o = (size_t)r * N;
        if constexpr (MODE != 2) {
            const long long p = r / RPP;
            const int rem = (int)(r - p * RPP);
            col = rem / TOUT;
            if constexpr (MODE == 1) o = ((size_t)(p * TOUT + (rem - col * TOUT)) * 3 + col) * N;
        }
        constexpr int NB = MODE == 2 ? N : 3 * N;                               // floats of the scale table; the bias table follows
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int oc = n0 + BN / 2 * wc + 16 * ct + 4 * kq;
            afl4 v = acc[ct][rt] * afl_ld4(sb + col * N + oc) + afl_ld4(sb + NB + col * N + oc);
#pragma unroll
            for (int s = 0; s < 4; ++s) v[s] = v[s] > 0.f ? v[s] : 0.f;
            afl_st4(outb + o + oc, v);
        }
    }
}

// ---- head: one workgroup of 128 threads per pair ---------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void k_afl_head(const float* __restrict__ fus, const float* __restrict__ blob, double* __restrict__ cost, int n_pairs)
{
    __shared__ float pooled[512], hid[128], logit[2];
    const int p = blockIdx.x, tid = threadIdx.x;
    for (int e = tid; e < 512; e += 128) {
        const int br = e >> 8, c = e & 255;
        const float* __restrict__ f = fus + ((size_t)br * n_pairs + p) * 6 * 256 + c;
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < 6; ++t) s = s + f[t * 256];
        pooled[e] = s / 6.0f;
    }
    __syncthreads();
    float h = blob[AFL_O_B1 + tid];
    const float* __restrict__ w1 = blob + AFL_O_FC1 + tid;
    for (int k = 0; k < 512; ++k) h = __builtin_fmaf(w1[(size_t)k * 128], pooled[k], h);
    hid[tid] = h > 0.f ? h : 0.f;
    __syncthreads();
    if (tid < 2) {
        float l = blob[AFL_O_B2 + tid];
        const float* __restrict__ w2 = blob + AFL_O_FC2 + tid * 128;
        for (int k = 0; k < 128; ++k) l = __builtin_fmaf(w2[k], hid[k], l);
        logit[tid] = l;
    }
    __syncthreads();
    if (tid == 0) {
        const double l0 = logit[0], l1 = logit[1], m = l0 > l1 ? l0 : l1;
        const double e0 = exp(l0 - m), e1 = exp(l1 - m);
        cost[p] = 1.0 - e1 / (e0 + e1);
    }
}

// ---- matching: one wave per component -----------------------------------------------------------------------------------------
// desc {first double of the matrix, rows, columns (rows <= columns), first int of the result}
__global__ __launch_bounds__(64) void k_afl_match(const int4* __restrict__ desc, const double* __restrict__ mats, int* __restrict__ col4row_out, int* __restrict__ err)
{
    __shared__ int col4row[AFL_MAX_COMPONENT];
    const int4 d = desc[blockIdx.x];
    const int lane = threadIdx.x;
    LsapLds L;
    L.col4row = col4row;
    if (lsap_wave(d.y, d.z, mats + d.x, L) != 0) {
        if (lane == 0) atomicMax(err, (int)blockIdx.x + 1);
        return;
    }
    __syncthreads();
    for (int i = lane; i < d.y; i += 64) col4row_out[d.w + i] = col4row[i];
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct SSAflink {
    SsBuf<SS_DEVICE> blob;                              // the weights (ss_aflink_set_weights)
    SsBuf<SS_DEVICE> dev;                               // the call's uploads and results
    SsBuf<SS_DEVICE> scratch;                           // a chunk's x and the two activation buffers, grown when a call needs more
    SsEvent ev;
};

void ss_aflink_free(SSAflink* g) { delete g; }

long long ss_aflink_weight_floats_impl() { return AFL_FLOATS; }
int ss_aflink_max_component_impl() { return AFL_MAX_COMPONENT; }
int ss_aflink_chunk_option(int value)
{
    if (value < 1 || value > 65536) return SS_ERR_INVALID;
    g_opt_aflink_chunk = value;
    return SS_OK;
}

static int afl_state(SSAflink** pg, SSAflink*& g, const std::string& who, std::string& err)
{
    if (!pg) { err = who + "null context"; return SS_ERR_INVALID; }
    if (!*pg) *pg = new SSAflink();
    g = *pg;
    SS_HIPCHK(who, g->ev.ensure());
    return SS_OK;
}

int ss_aflink_set_weights_check_impl(const float* blob, long long n, std::string& err)
{
    const std::string who = "ss_aflink_set_weights: ";
    if (!blob) { err = who + "null argument"; return SS_ERR_INVALID; }
    if (n != AFL_FLOATS) { err = who + "the blob holds " + std::to_string(n) + " floats, not ss_aflink_weight_floats() = " + std::to_string(AFL_FLOATS); return SS_ERR_INVALID; }
    for (long long i = 0; i < n; ++i)
        if (!std::isfinite(blob[i])) { err = who + "float " + std::to_string(i) + " is NaN or infinite"; return SS_ERR_INVALID; }
    return SS_OK;
}

int ss_aflink_set_weights_impl(SSAflink** pg, hipStream_t stream, const float* blob, std::string& err)
{
    const std::string who = "ss_aflink_set_weights: ";
    SSAflink* g = nullptr;
    if (int rc = afl_state(pg, g, who, err)) return rc;
    SS_HIPCHK(who, g->blob.reserve((size_t)AFL_FLOATS * sizeof(float), SS_EXACT));
    SS_HIPCHK(who, hipMemcpyAsync(g->blob.as(), blob, (size_t)AFL_FLOATS * sizeof(float), hipMemcpyHostToDevice, stream));
    SS_HIPCHK(who, hipStreamSynchronize(stream));
    return SS_OK;
}

// every refusal of ss_aflink_cost that needs no context
int ss_aflink_cost_check_impl(int n, const int* offsets, const double* feats, int t0, int t1, double thr_s, long long cap, const int* pair_i,
                              const int* pair_j, const double* cost, const long long* n_pairs, std::string& err)
{
    const std::string who = "ss_aflink_cost: ";
    if (!offsets || !feats || !n_pairs) { err = who + "null argument"; return SS_ERR_INVALID; }
    if (n < 1 || n > AFL_MAX_TRACKLETS) { err = who + "n_tracklets must be 1 .. " + std::to_string(AFL_MAX_TRACKLETS); return SS_ERR_INVALID; }
    if (t1 <= t0) { err = who + "thr_t0 < thr_t1 required"; return SS_ERR_INVALID; }
    if (!std::isfinite(thr_s) || !(thr_s >= 0.0)) { err = who + "thr_s must be finite and >= 0"; return SS_ERR_INVALID; }
    if (cap < 0 || (cap > 0 && (!pair_i || !pair_j || !cost))) { err = who + "cap >= 0, and with cap > 0 pair_i, pair_j and cost"; return SS_ERR_INVALID; }
    if (offsets[0] != 0) { err = who + "offsets[0] must be 0"; return SS_ERR_INVALID; }
    for (int t = 0; t < n; ++t) {
        const std::string tr = "tracklet " + std::to_string(t) + ": ";
        if (offsets[t + 1] <= offsets[t]) { err = who + tr + "no rows"; return SS_ERR_INVALID; }
        for (int i = offsets[t]; i < offsets[t + 1]; ++i) {
            const double* f = feats + (size_t)i * 3;
            if (!std::isfinite(f[0]) || !std::isfinite(f[1]) || !std::isfinite(f[2])) { err = who + tr + "a value is NaN or infinite"; return SS_ERR_INVALID; }
            if (f[0] != std::floor(f[0]) || std::fabs(f[0]) > 1e9) { err = who + tr + "a frame is not an integer of at most 1e9"; return SS_ERR_INVALID; }
            if (i > offsets[t] && f[0] <= f[-3]) { err = who + tr + "frames must increase strictly"; return SS_ERR_INVALID; }
        }
    }
    return SS_OK;
}

template <int CIN, int N, int BN, int TIN, int TOUT, int MODE>
static void afl_launch_gemm(const float* in, const float* blob, float* out, int P, int o_w, int o_sb, hipStream_t stream)
{
    const long long M = (long long)P * (MODE == 2 ? TOUT : 3 * TOUT);
    hipLaunchKernelGGL((k_afl_gemm<CIN, N, BN, TIN, TOUT, MODE>), dim3((unsigned)((M + AFL_BM - 1) / AFL_BM), N / BN, 2), dim3(256), 0, stream,
                       in, blob, out, P, o_w, o_sb);
}

int ss_aflink_cost_impl(SSAflink** pg, hipStream_t stream, int n, const int* offsets, const double* feats, int t0, int t1, double thr_s, long long cap,
                        int* pair_i, int* pair_j, double* cost, float* inputs, long long* n_pairs, std::string& err)
{
    const std::string who = "ss_aflink_cost: ";
    SSAflink* gp = nullptr;
    if (int rc = afl_state(pg, gp, who, err)) return rc;
    SSAflink& g = *gp;
    const float* const w = g.blob.as<float>();
    if (!w) { err = who + "no weights (ss_aflink_set_weights)"; return SS_ERR_INVALID; }
    const size_t rows = (size_t)offsets[n];
    // device image: feats | row_off | offsets, then (a sized call) pair_i | pair_j | cost
    SsLayout lay;
    lay.take(rows * 3 * sizeof(double));                // feats at 0
    const size_t o_ro = lay.take((size_t)(n + 1) * sizeof(long long)), o_off = lay.take((size_t)(n + 1) * sizeof(int));
    const size_t head = lay.at;
    // a sized call makes room before the gate runs, so the gate is counted once per call: for `cap` candidates, or for the n (n - 1) / 2
    // pairs that n tracklets can give at most (one direction of every pair), whichever is less
    const size_t room = (size_t)std::min<long long>(cap, (long long)n * (n - 1) / 2);
    if (room > 0x7fffffffull / 256) { err = who + "room for " + std::to_string(room) + " candidates asked: more than one call takes"; return SS_ERR_CAPACITY; }
    const size_t o_pi = lay.take(room * sizeof(int)), o_pj = lay.take(room * sizeof(int)), o_cost = lay.take(room * sizeof(double));
    SS_HIPCHK(who, g.dev.reserve(room ? lay.at : head, SS_QUARTER));
    char* const d = g.dev.as();
    SS_HIPCHK(who, hipMemcpyAsync(d, feats, rows * 3 * sizeof(double), hipMemcpyHostToDevice, stream));
    SS_HIPCHK(who, hipMemcpyAsync(d + o_off, offsets, (size_t)(n + 1) * sizeof(int), hipMemcpyHostToDevice, stream));
    AflGate a;
    a.offsets = (const int*)(d + o_off); a.feats = (const double*)d; a.row_off = (long long*)(d + o_ro);
    a.pair_i = a.pair_j = nullptr; a.thr_s = thr_s; a.t0 = t0; a.t1 = t1; a.n = n;
    hipLaunchKernelGGL((k_afl_gate<false>), dim3(n), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(k_afl_scan, dim3(1), dim3(64), 0, stream, a.row_off, n);
    SS_HIPCHK(who, hipGetLastError());
    long long total = 0;
    SS_HIPCHK(who, hipMemcpyAsync(&total, a.row_off + n, sizeof(long long), hipMemcpyDeviceToHost, stream));
    SS_HIPCHK(who, hipStreamSynchronize(stream));
    *n_pairs = total;
    if (cap == 0 || total == 0) return SS_OK;           // the count alone: the caller sizes its arrays by it
    if (total > cap) { err = who + std::to_string(total) + " candidates, cap " + std::to_string(cap); return SS_ERR_CAPACITY; }
    a.pair_i = (int*)(d + o_pi); a.pair_j = (int*)(d + o_pj);
    double* d_cost = (double*)(d + o_cost);
    hipLaunchKernelGGL((k_afl_gate<true>), dim3(n), dim3(64), 0, stream, a);
    SS_HIPCHK(who, hipGetLastError());
    const int chunk = (int)std::min<long long>(g_opt_aflink_chunk, total);
    const size_t need = (size_t)chunk * (AFL_X_FLOATS + 2 * AFL_BUF_FLOATS);
    SS_HIPCHK(who, g.scratch.reserve(need * sizeof(float), SS_EXACT));
    float* x = g.scratch.as<float>();
    float* bufA = x + (size_t)chunk * AFL_X_FLOATS;
    float* bufB = bufA + (size_t)chunk * AFL_BUF_FLOATS;
    for (long long c0 = 0; c0 < total; c0 += chunk) {
        const int P = (int)std::min<long long>(chunk, total - c0);
        hipLaunchKernelGGL(k_afl_prep, dim3((P * 3 + 255) / 256), dim3(256), 0, stream, a.offsets, a.feats, a.pair_i + c0, a.pair_j + c0, x, P);
        hipLaunchKernelGGL(k_afl_l1, dim3((unsigned)(((long long)P * 2 * 3 * 24 * 8 + 255) / 256)), dim3(256), 0, stream, x, w, bufA, P);
        afl_launch_gemm<32, 64, 64, 24, 18, 0>(bufA, w, bufB, P, AFL_O_W2, AFL_O_SB2, stream);
        afl_launch_gemm<64, 128, 128, 18, 12, 0>(bufB, w, bufA, P, AFL_O_W3, AFL_O_SB3, stream);
        afl_launch_gemm<128, 256, 128, 12, 6, 1>(bufA, w, bufB, P, AFL_O_W4, AFL_O_SB4, stream);
        afl_launch_gemm<256, 256, 128, 6, 6, 2>(bufB, w, bufA, P, AFL_O_WF, AFL_O_SBF, stream);
        hipLaunchKernelGGL(k_afl_head, dim3(P), dim3(128), 0, stream, bufA, w, d_cost + c0, P);
        SS_HIPCHK(who, hipGetLastError());
        if (inputs) SS_HIPCHK(who, hipMemcpyAsync(inputs + (size_t)c0 * AFL_X_FLOATS, x, (size_t)P * AFL_X_FLOATS * sizeof(float), hipMemcpyDeviceToHost, stream));
    }
    SS_HIPCHK(who, hipMemcpyAsync(pair_i, a.pair_i, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, stream));
    SS_HIPCHK(who, hipMemcpyAsync(pair_j, a.pair_j, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, stream));
    SS_HIPCHK(who, hipMemcpyAsync(cost, d_cost, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, stream));
    SS_HIPCHK(who, hipEventRecord(g.ev, stream));
    SS_HIPCHK(who, hipEventSynchronize(g.ev));
    return SS_OK;
}

int ss_aflink_match_check_impl(int n, long long n_pairs, const int* pair_i, const int* pair_j, const double* cost, double thr_p, const int* successor,
                               std::string& err)
{
    const std::string who = "ss_aflink_match: ";
    if (!successor || (n_pairs > 0 && (!pair_i || !pair_j || !cost))) { err = who + "null argument"; return SS_ERR_INVALID; }
    if (n < 1 || n > AFL_MAX_TRACKLETS) { err = who + "n_tracklets must be 1 .. " + std::to_string(AFL_MAX_TRACKLETS); return SS_ERR_INVALID; }
    if (n_pairs < 0) { err = who + "n_pairs < 0"; return SS_ERR_INVALID; }
    if (std::isnan(thr_p)) { err = who + "thr_p is NaN"; return SS_ERR_INVALID; }
    for (long long k = 0; k < n_pairs; ++k) {
        const std::string pr = "pair " + std::to_string(k) + ": ";
        if (pair_i[k] < 0 || pair_i[k] >= n || pair_j[k] < 0 || pair_j[k] >= n || pair_i[k] == pair_j[k]) { err = who + pr + "tracklets out of range or equal"; return SS_ERR_INVALID; }
        if (std::isnan(cost[k])) { err = who + pr + "the cost is NaN"; return SS_ERR_INVALID; }
        if (k && (pair_i[k] < pair_i[k - 1] || (pair_i[k] == pair_i[k - 1] && pair_j[k] <= pair_j[k - 1]))) { err = who + pr + "pairs must be row-major and distinct"; return SS_ERR_INVALID; }
    }
    return SS_OK;
}

int ss_aflink_match_impl(SSAflink** pg, hipStream_t stream, int n, long long n_pairs, const int* pair_i, const int* pair_j, const double* cost,
                         double thr_p, int* successor, std::string& err)
{
    const std::string who = "ss_aflink_match: ";
    std::fill(successor, successor + n, -1);
    // connected components of the survivors; node i = tracklet i as the earlier one, node n + j = tracklet j as the later one
    std::vector<int> parent(2 * (size_t)n);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int v) { while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; } return v; };
    std::vector<long long> surv;
    for (long long k = 0; k < n_pairs; ++k)
        if (cost[k] < thr_p) {
            surv.push_back(k);
            const int ra = find(pair_i[k]), rb = find(n + pair_j[k]);
            if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);     // the root is the component's smallest earlier tracklet
        }
    if (surv.empty()) return SS_OK;
    struct Comp { std::vector<int> rows, cols; std::vector<long long> cells; };
    std::vector<Comp> comps;
    std::vector<int> comp_of(n, -1), pos(2 * (size_t)n, -1);
    for (long long k : surv) {                          // row-major: the components come by rising root, their rows rise
        const int root = find(pair_i[k]);
        if (comp_of[root] < 0) { comp_of[root] = (int)comps.size(); comps.emplace_back(); }
        Comp& c = comps[comp_of[root]];
        if (pos[pair_i[k]] < 0) { pos[pair_i[k]] = (int)c.rows.size(); c.rows.push_back(pair_i[k]); }
        if (pos[n + pair_j[k]] < 0) { pos[n + pair_j[k]] = 0; c.cols.push_back(pair_j[k]); }
        c.cells.push_back(k);
    }
    size_t cells = 0, res = 0;
    for (Comp& c : comps) {
        std::sort(c.cols.begin(), c.cols.end());
        for (size_t q = 0; q < c.cols.size(); ++q) pos[n + c.cols[q]] = (int)q;
        if (c.rows.size() > AFL_MAX_COMPONENT || c.cols.size() > AFL_MAX_COMPONENT) {
            err = who + "a component of " + std::to_string(c.rows.size()) + " x " + std::to_string(c.cols.size()) + " tracklets, more than ss_aflink_max_component() = " +
                  std::to_string(AFL_MAX_COMPONENT) + " a side";
            std::fill(successor, successor + n, -1);
            return SS_ERR_CAPACITY;
        }
        cells += c.rows.size() * c.cols.size();
        res += std::min(c.rows.size(), c.cols.size());
    }
    if (cells > 0x7fffffffull) { err = who + "the components' matrices hold " + std::to_string(cells) + " cells, more than 2^31"; return SS_ERR_CAPACITY; }
    SSAflink* gp = nullptr;
    if (int rc = afl_state(pg, gp, who, err)) return rc;
    SSAflink& g = *gp;
    // image: matrices | desc | err | results
    SsLayout lay;
    lay.take(cells * sizeof(double));                   // matrices at 0
    const size_t nc = comps.size(), o_desc = lay.take(nc * sizeof(int4)), o_err = lay.take(sizeof(int)), o_res = lay.take(res * sizeof(int));
    SS_HIPCHK(who, g.dev.reserve(lay.at, SS_QUARTER));
    char* const dev = g.dev.as();
    std::vector<char> h(o_res, 0);
    double* mats = (double*)h.data();
    int4* desc = (int4*)(h.data() + o_desc);
    size_t at = 0, rat = 0;
    for (size_t q = 0; q < nc; ++q) {
        const Comp& c = comps[q];
        const int R = (int)c.rows.size(), Cn = (int)c.cols.size();
        const bool tall = Cn < R;                       // SciPy transposes a tall matrix: the smaller side is lsap_wave's rows
        std::fill(mats + at, mats + at + (size_t)R * Cn, AFL_FILL);
        for (long long k : c.cells) {
            const int r = pos[pair_i[k]], cc = pos[n + pair_j[k]];
            mats[at + (tall ? (size_t)cc * R + r : (size_t)r * Cn + cc)] = cost[k];
        }
        desc[q] = make_int4((int)at, tall ? Cn : R, tall ? R : Cn, (int)rat);
        at += (size_t)R * Cn;
        rat += std::min(R, Cn);
    }
    SS_HIPCHK(who, hipMemcpyAsync(dev, h.data(), o_res, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_afl_match, dim3((unsigned)nc), dim3(64), 0, stream, (const int4*)(dev + o_desc), (const double*)dev, (int*)(dev + o_res),
                       (int*)(dev + o_err));
    SS_HIPCHK(who, hipGetLastError());
    std::vector<int> out(res + 4);
    SS_HIPCHK(who, hipMemcpyAsync(out.data() + res, dev + o_err, sizeof(int), hipMemcpyDeviceToHost, stream));
    if (res) SS_HIPCHK(who, hipMemcpyAsync(out.data(), dev + o_res, res * sizeof(int), hipMemcpyDeviceToHost, stream));
    SS_HIPCHK(who, hipEventRecord(g.ev, stream));
    SS_HIPCHK(who, hipEventSynchronize(g.ev));
    if (out[res] != 0) { err = who + "component " + std::to_string(out[res] - 1) + " has no assignment"; return SS_ERR_INFEASIBLE; }
    for (size_t q = 0; q < nc; ++q) {
        const Comp& c = comps[q];
        const int R = (int)c.rows.size(), Cn = (int)c.cols.size();
        const bool tall = Cn < R;
        const int4 d = desc[q];
        for (int r = 0; r < d.y; ++r) {
            const int cc = out[d.w + r];
            if (cc < 0 || cc >= d.z) continue;
            if (!(mats[d.x + (size_t)r * d.z + cc] < thr_p)) continue;      // an assigned cell that is no survivor (the fill) is no link
            successor[c.rows[tall ? cc : r]] = c.cols[tall ? r : cc];
        }
        (void)R;
    }
    return SS_OK;
}
