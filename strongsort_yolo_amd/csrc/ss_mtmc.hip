// ss_mtmc.hip — identities across cameras (docs/MTMC.md): a bank of one pooled appearance descriptor per track id, kept on the
// device while a tracker runs, and the linking of the cameras' tracklets after the run: cosine distances, the same-camera
// constraint and a constrained average-linkage clustering.  tests/mtmc_ref.py is the definition; the device gives its bits.
//
// k_bank_update_group: one launch per group.  A stream's ids are dealt out to the BK_WAVES waves that serve it (id % BK_WAVES), so
// every add to an id's sums is made by one wave in program order, the frames in order: no barrier, no atomic, and the order of the
// adds is the frame order.  Every workgroup keeps its own copy of the stream's frame counter (they all see the same counts), so no
// workgroup reads what another one writes.  A row is one wave's work: lane l holds features l, l + 64, ... l + 448, the squared
// norm is eight f64 products a lane, added in rising order, and the xor butterfly 32, 16, ... 1 over the lanes.
//
// k_bank_desc: one wave per listed id, the same 8 x 64 butterfly over the squared sums, desc = (float)(sum / sqrt(total)).
//
// k_mtmc_dist: D = 1 - desc desc^T on v_mfma_f32_16x16x4_f32, one workgroup of four waves per 64 x 64 tile of the upper triangle,
// operands staged through LDS 32 k at a time, one accumulator per output over rising k.  Only i < j is written.
//
// k_mtmc_init / k_mtmc_cluster: the f64 matrix (upper triangle in use) and the symmetric conflict bit matrix in context scratch;
// the clustering is serial in the merges and runs as ONE workgroup of 1024 threads.  Every live row a keeps the smallest (d, b) of its
// admissible pairs b > a in LDS; a merge of b into a recomputes the pairs (k, a), rescans row a and the rows whose cached partner
// was a or b, and sets every other row's cache against its one changed pair, so what is cached always equals a full scan.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "ss_common.h"
#include "ss_host.h"
#include "ss_launch.h"

#define BK_MAX_IDS 65536               // the most ids a bank may be made for
#define BK_BLOCKS 8                    // workgroups a stream
#define BK_THREADS 256
#define BK_WAVES (BK_BLOCKS * BK_THREADS / 64)
#define MT_MAX 2048                    // tracklets of one ss_mtmc_link
#define MT_TILE 64                     // k_mtmc_dist's workgroup tile
#define MT_KC 32                       // k of one LDS stage
#define MT_LD (MT_KC + 1)
#define MT_THREADS 1024

struct SSBankDev {
    int S, max_ids;
    double* sum;                       // [S][max_ids][512]
    int *n, *first, *last, *cls;       // [S][max_ids]
    int* frame;                        // [S][BK_BLOCKS]
    int* err;                          // [S]
};

__device__ __forceinline__ double bk_wave_sum(double p)
{
    for (int off = 32; off >= 1; off >>= 1) p = __dadd_rn(p, __shfl_xor(p, off));
    return p;
}

__global__ __launch_bounds__(BK_THREADS) void k_bank_update_group(SSBankDev z, int F, const float* __restrict__ rows, const int* __restrict__ nrows,
                                                                  const float* __restrict__ feats)
{
    const int s = blockIdx.x, lane = threadIdx.x & 63;
    const int w = blockIdx.y * (BK_THREADS / 64) + (threadIdx.x >> 6);
    const size_t base = (size_t)s * z.max_ids;
    int f = z.frame[s * BK_BLOCKS + blockIdx.y];
    __syncthreads();                                             // every wave has the counter before thread 0 moves it
    for (int fi = 0; fi < F; ++fi) {
        int n = nrows[fi * z.S + s];
        if (n < 0) continue;                                     // uniform: the stream sits this frame out
        n = min(n, SS_MAXT);
        const size_t fs = (size_t)fi * z.S + s;
        for (int c = 0; c < n; c += 64) {
            const int r = c + lane;
            float idf = 0.f, df = -1.f;
            if (r < n) { const float* p = rows + (fs * SS_MAXT + r) * 8; idf = p[4]; df = p[7]; }
            const bool ok = r < n && df >= 0.f && df < (float)SS_MAXD && idf >= 1.0f && idf < 2147483648.0f;
            const int id = ok ? (int)idf : 0;
            const bool mine = ok && (id % BK_WAVES) == w;
            if (mine && id > z.max_ids) z.err[s] = SS_ERR_CAPACITY;
            unsigned long long mask = __ballot(mine && id <= z.max_ids);
            while (mask) {
                const int r2 = c + __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const float* p = rows + (fs * SS_MAXT + r2) * 8;
                const int id2 = (int)p[4], det = (int)p[7];
                const float* ft = feats + (fs * SS_MAXD + det) * SS_F;
                float v[8];
                double q = 0.0;
#pragma unroll
                for (int j = 0; j < 8; ++j) { v[j] = ft[lane + 64 * j]; q = __dadd_rn(q, __dmul_rn((double)v[j], (double)v[j])); }
                q = bk_wave_sum(q);
                if (!(q > 0.0) || !__builtin_isfinite(q)) continue;          // a row without a direction: not counted
                const double rs = sqrt(q);
                const size_t e = base + (size_t)(id2 - 1);
                double* sm = z.sum + e * SS_F;
#pragma unroll
                for (int j = 0; j < 8; ++j) sm[lane + 64 * j] = __dadd_rn(sm[lane + 64 * j], (double)v[j] / rs);
                if (lane == 0) {
                    const int cnt = z.n[e];
                    if (cnt == 0) z.first[e] = f;
                    z.n[e] = cnt + 1;
                    z.last[e] = f;
                    z.cls[e] = (int)p[5];
                }
            }
        }
        ++f;
    }
    if (threadIdx.x == 0) z.frame[s * BK_BLOCKS + blockIdx.y] = f;
}

__global__ __launch_bounds__(256) void k_bank_desc(const double* __restrict__ sum, const int* __restrict__ ids, int n, float* __restrict__ desc)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const double* sm = sum + (size_t)(ids[i] - 1) * SS_F;
    double v[8], q = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { v[j] = sm[lane + 64 * j]; q = __dadd_rn(q, __dmul_rn(v[j], v[j])); }
    q = bk_wave_sum(q);
    const double rs = sqrt(q);
#pragma unroll
    for (int j = 0; j < 8; ++j) desc[(size_t)i * SS_F + lane + 64 * j] = (float)(v[j] / rs);
}

// ---- distances ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mtmc_dist(const float* __restrict__ desc, int T, int nt, float* __restrict__ D)
{
    __shared__ float sa[MT_TILE * MT_LD], sb[MT_TILE * MT_LD];
    // tile (ti, tj), ti <= tj, from the linear index over the upper triangle of tiles
    int ti = 0, rest = blockIdx.x;
    while (rest >= nt - ti) { rest -= nt - ti; ++ti; }
    const int tj = ti + rest;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i0 = ti * MT_TILE, j0 = tj * MT_TILE;
    f32x4 acc[4];
    for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int lr = tid >> 3, lc = (tid & 7) * 4;                 // this thread's float4 of a 32-row half of a stage
    const int m = lane & 15, kq = lane >> 4;
    for (int k0 = 0; k0 < SS_F; k0 += MT_KC) {
        for (int h = 0; h < 2; ++h) {
            const int row = lr + 32 * h;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (i0 + row < T) a = *reinterpret_cast<const float4*>(desc + (size_t)(i0 + row) * SS_F + k0 + lc);
            if (j0 + row < T) b = *reinterpret_cast<const float4*>(desc + (size_t)(j0 + row) * SS_F + k0 + lc);
            float* pa = sa + row * MT_LD + lc;
            float* pb = sb + row * MT_LD + lc;
            pa[0] = a.x; pa[1] = a.y; pa[2] = a.z; pa[3] = a.w;
            pb[0] = b.x; pb[1] = b.y; pb[2] = b.z; pb[3] = b.w;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < MT_KC; kk += 4) {
            const float av = sa[(16 * wv + m) * MT_LD + kk + kq];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, sb[(16 * c + m) * MT_LD + kk + kq], acc[c], 0, 0, 0);
        }
        __syncthreads();
    }
    for (int c = 0; c < 4; ++c)
        for (int i = 0; i < 4; ++i) {
            const int gi = i0 + 16 * wv + 4 * kq + i, gj = j0 + 16 * c + m;
            if (gi < gj && gj < T) D[(size_t)gi * T + gj] = 1.0f - acc[c][i];
        }
}

// ---- clustering ---------------------------------------------------------------------------------------------------------------
struct MtArgs {
    int T, W, min_rows;                // W: 64-bit words of a conflict row
    double thr;
    const float* D;                    // [T][T], i < j in use
    const int *cam, *first, *last, *n; // [T]
    double* d;                         // [T][T], i < j in use
    unsigned long long* conf;          // [T][W], symmetric
    int* root;                         // [T]
    double* merges;                    // [T][3]
    int* n_merges;
};

__global__ __launch_bounds__(256) void k_mtmc_init(MtArgs a)
{
    const int T = a.T;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)T * T; e += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(e / T), j = (int)(e - (size_t)i * T);
        a.d[e] = i < j ? (double)a.D[e] : 0.0;
    }
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)T * a.W; e += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(e / a.W), w = (int)(e - (size_t)i * a.W);
        const int ci = a.cam[i], fi = a.first[i], li = a.last[i];
        const bool small_i = a.n[i] < a.min_rows;
        unsigned long long bits = 0;
        for (int b = 0; b < 64; ++b) {
            const int j = 64 * w + b;
            if (j >= T || j == i) continue;
            if (small_i || a.n[j] < a.min_rows || (a.cam[j] == ci && fi <= a.last[j] && a.first[j] <= li)) bits |= 1ull << b;
        }
        a.conf[e] = bits;
    }
}

struct MtKey { double d; int a, b; };

__device__ __forceinline__ bool mt_less(double d1, int a1, int b1, double d2, int a2, int b2)
{
    return d1 < d2 || (d1 == d2 && (a1 < a2 || (a1 == a2 && b1 < b2)));
}

// the wave's smallest (d, a, b) in every lane; b < 0: none
__device__ __forceinline__ MtKey mt_wave_min(MtKey k)
{
    for (int off = 32; off >= 1; off >>= 1) {
        const double d2 = __shfl_xor(k.d, off);
        const int a2 = __shfl_xor(k.a, off), b2 = __shfl_xor(k.b, off);
        if (b2 >= 0 && (k.b < 0 || mt_less(d2, a2, b2, k.d, k.a, k.b))) { k.d = d2; k.a = a2; k.b = b2; }
    }
    return k;
}

// row r's smallest admissible (d, b), b > r, by one wave; the result in every lane
__device__ __forceinline__ MtKey mt_scan_row(const MtArgs& a, const unsigned char* live, int r, int lane)
{
    MtKey k{0.0, r, -1};
    const double* dr = a.d + (size_t)r * a.T;
    const unsigned long long* cr = a.conf + (size_t)r * a.W;
    for (int b = r + 1 + lane; b < a.T; b += 64) {
        if (!live[b] || (cr[b >> 6] >> (b & 63) & 1ull)) continue;
        const double v = dr[b];
        if (v < a.thr && (k.b < 0 || v < k.d)) { k.d = v; k.b = b; }          // b rises: the first of equals stays
    }
    return mt_wave_min(k);
}

__global__ __launch_bounds__(MT_THREADS) void k_mtmc_cluster(MtArgs a)
{
    __shared__ double min_d[MT_MAX];
    __shared__ int min_b[MT_MAX], size[MT_MAX];
    __shared__ unsigned char live[MT_MAX], need[MT_MAX];
    __shared__ MtKey part[MT_THREADS / 64];
    __shared__ MtKey best;
    const int T = a.T, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < T; i += MT_THREADS) { live[i] = 1; size[i] = 1; need[i] = 0; a.root[i] = i; }
    __syncthreads();
    for (int r = wv; r < T; r += MT_THREADS / 64) {
        const MtKey k = mt_scan_row(a, live, r, lane);
        if (lane == 0) { min_d[r] = k.d; min_b[r] = k.b; }
    }
    __syncthreads();
    int nm = 0;
    for (;;) {
        // ---- the smallest (d, a, b) over the rows
        MtKey k{0.0, 0, -1};
        for (int r = tid; r < T; r += MT_THREADS)
            if (live[r] && min_b[r] >= 0 && (k.b < 0 || mt_less(min_d[r], r, min_b[r], k.d, k.a, k.b))) { k.d = min_d[r]; k.a = r; k.b = min_b[r]; }
        k = mt_wave_min(k);
        if (lane == 0) part[wv] = k;
        __syncthreads();
        if (wv == 0) {
            MtKey q = lane < MT_THREADS / 64 ? part[lane] : MtKey{0.0, 0, -1};
            q = mt_wave_min(q);
            if (lane == 0) best = q;
        }
        __syncthreads();
        const MtKey m = best;
        if (m.b < 0) break;                                      // uniform
        const int A = m.a, B = m.b;
        const double sa = (double)size[A], sb = (double)size[B], st = (double)(size[A] + size[B]);
        // ---- the pairs of A: values, conflicts, and what the rows below B have cached
        for (int k2 = tid; k2 < T; k2 += MT_THREADS) {
            if (!live[k2] || k2 == A || k2 == B) continue;
            double* pa = k2 < A ? a.d + (size_t)k2 * T + A : a.d + (size_t)A * T + k2;
            const double db = k2 < B ? a.d[(size_t)k2 * T + B] : a.d[(size_t)B * T + k2];
            const double nv = __ddiv_rn(__dadd_rn(__dmul_rn(sa, *pa), __dmul_rn(sb, db)), st);
            *pa = nv;
            unsigned long long* ck = a.conf + (size_t)k2 * a.W;
            const bool cf = (ck[A >> 6] >> (A & 63) & 1ull) || (ck[B >> 6] >> (B & 63) & 1ull);
            if (cf) ck[A >> 6] |= 1ull << (A & 63);
            if (k2 < B) {
                if (min_b[k2] == A || min_b[k2] == B) need[k2] = 1;
                else if (k2 < A && !cf && nv < a.thr && (min_b[k2] < 0 || nv < min_d[k2] || (nv == min_d[k2] && A < min_b[k2]))) { min_d[k2] = nv; min_b[k2] = A; }
            }
        }
        for (int w2 = tid; w2 < a.W; w2 += MT_THREADS) a.conf[(size_t)A * a.W + w2] |= a.conf[(size_t)B * a.W + w2];
        __syncthreads();                                         // every thread has read the sizes
        if (tid == 0) {
            live[B] = 0; size[A] += size[B]; need[A] = 1; a.root[B] = A;
            a.merges[3 * nm] = (double)A; a.merges[3 * nm + 1] = (double)B; a.merges[3 * nm + 2] = m.d;
        }
        ++nm;
        __threadfence_block();
        __syncthreads();
        // ---- the rows whose cache no longer holds
        for (int r = wv; r < B; r += MT_THREADS / 64) {
            if (!need[r]) continue;                              // uniform within the wave
            const MtKey q = mt_scan_row(a, live, r, lane);
            if (lane == 0) { min_d[r] = q.d; min_b[r] = q.b; need[r] = 0; }
        }
        __syncthreads();
    }
    if (tid == 0) *a.n_merges = nm;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct SSBank {
    SSBankDev dev;
    SsBuf<SS_DEVICE> sum, ints, frame, err, ids, desc;           // ids, desc: ss_bank_get's scratch, grown on demand
};

struct SSMtmc {
    SsBuf<SS_DEVICE> desc, D, d, conf, ints, merges;             // grown on demand
};

int ss_bank_max_ids_impl() { return BK_MAX_IDS; }
int ss_mtmc_max_tracklets_impl() { return MT_MAX; }
void ss_bank_free(SSBank* b) { delete b; }
void ss_mtmc_free(SSMtmc* g) { delete g; }

int ss_bank_reset_impl(SSBank* b, hipStream_t st, int stream, std::string& err)
{
    const char* who = "ss_bank_reset: ";
    const SSBankDev& d = b->dev;
    const size_t s0 = stream < 0 ? 0 : stream, ns = stream < 0 ? d.S : 1, M = d.max_ids;
    SS_HIPCHK(who, hipMemsetAsync(d.sum + s0 * M * SS_F, 0, ns * M * SS_F * sizeof(double), st));
    for (int* p : {d.n, d.first, d.last, d.cls}) SS_HIPCHK(who, hipMemsetAsync(p + s0 * M, 0, ns * M * sizeof(int), st));
    SS_HIPCHK(who, hipMemsetAsync(d.frame + s0 * BK_BLOCKS, 0, ns * BK_BLOCKS * sizeof(int), st));
    SS_HIPCHK(who, hipMemsetAsync(d.err + s0, 0, ns * sizeof(int), st));
    SS_HIPCHK(who, hipStreamSynchronize(st));
    return SS_OK;
}

int ss_bank_create_impl(SSBank** pb, hipStream_t st, int S, int max_ids, std::string& err)
{
    const char* who = "ss_bank_create: ";
    SSBank* b = new SSBank();
    SSBankDev& d = b->dev;
    memset(&d, 0, sizeof d);
    d.S = S; d.max_ids = max_ids;
    const size_t M = (size_t)S * max_ids;
    hipError_t e = b->sum.reserve(M * SS_F * sizeof(double), SS_EXACT);
    if (e == hipSuccess) e = b->ints.reserve(4 * M * sizeof(int), SS_EXACT);
    if (e == hipSuccess) e = b->frame.reserve((size_t)S * BK_BLOCKS * sizeof(int), SS_EXACT);
    if (e == hipSuccess) e = b->err.reserve((size_t)S * sizeof(int), SS_EXACT);
    if (e != hipSuccess) { delete b; err = std::string(who) + hipGetErrorString(e); return SS_ERR_HIP; }
    d.sum = b->sum.as<double>();
    d.n = b->ints.as<int>(); d.first = d.n + M; d.last = d.first + M; d.cls = d.last + M;
    d.frame = b->frame.as<int>(); d.err = b->err.as<int>();
    *pb = b;
    return ss_bank_reset_impl(b, st, -1, err);
}

int ss_bank_update_check_impl(int n_frames, const float* d_rows, const int* d_nrows, const float* d_feats, std::string& err)
{
    const std::string who = "ss_bank_update_group: ";
    if (n_frames < 1 || n_frames > SS_FMAX) { err = who + "n_frames " + std::to_string(n_frames) + " outside 1.." + std::to_string(SS_FMAX); return SS_ERR_INVALID; }
    if (!d_rows || !d_nrows || !d_feats) { err = who + "null rows, counts or features"; return SS_ERR_INVALID; }
    if (((uintptr_t)d_rows | (uintptr_t)d_nrows | (uintptr_t)d_feats) & 3) { err = who + "rows, counts and features must be 4-byte aligned"; return SS_ERR_INVALID; }
    return SS_OK;
}

int ss_bank_update_impl(SSBank* b, hipStream_t st, int n_frames, const float* d_rows, const int* d_nrows, const float* d_feats, std::string& err)
{
    hipLaunchKernelGGL(k_bank_update_group, dim3(b->dev.S, BK_BLOCKS), dim3(BK_THREADS), 0, st, b->dev, n_frames, d_rows, d_nrows, d_feats);
    SS_HIPCHK("ss_bank_update_group: ", hipGetLastError());
    return SS_OK;
}

// the capacity flags, for ss_check_errors
int ss_bank_pending_impl(SSBank* b, hipStream_t st, std::string& err)
{
    if (!b) return SS_OK;
    const char* who = "ss_check_errors: ";
    std::vector<int> e(b->dev.S);
    SS_HIPCHK(who, hipMemcpyAsync(e.data(), b->dev.err, e.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    SS_HIPCHK(who, hipStreamSynchronize(st));
    for (size_t s = 0; s < e.size(); ++s)
        if (e[s]) { err = "track bank: a track id above max_ids " + std::to_string(b->dev.max_ids) + " on stream " + std::to_string(s); return e[s]; }
    return SS_OK;
}

int ss_bank_get_impl(SSBank* b, hipStream_t st, int stream, int cap, int* n, int* ids, int* counts, int* first, int* last, int* cls, float* desc,
                     std::string& err)
{
    const char* who = "ss_bank_get: ";
    const SSBankDev& d = b->dev;
    const size_t M = d.max_ids, S = d.S;
    std::vector<int> h(4 * M);
    SS_HIPCHK(who, hipStreamSynchronize(st));
    for (int a = 0; a < 4; ++a) SS_HIPCHK(who, hipMemcpy(h.data() + a * M, d.n + a * S * M + stream * M, M * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<int> list;
    for (size_t i = 0; i < M; ++i)
        if (h[i] > 0) list.push_back((int)i + 1);
    *n = (int)list.size();
    if (cap == 0) return SS_OK;                                  // a count only
    if ((size_t)cap < list.size()) { err = std::string(who) + "cap " + std::to_string(cap) + " is below the " + std::to_string(list.size()) + " ids of the stream"; return SS_ERR_INVALID; }
    for (size_t i = 0; i < list.size(); ++i) {
        const size_t e = list[i] - 1;
        ids[i] = list[i]; counts[i] = h[e]; first[i] = h[M + e]; last[i] = h[2 * M + e]; cls[i] = h[3 * M + e];
    }
    if (list.empty()) return SS_OK;
    hipError_t e = b->ids.reserve(list.size() * sizeof(int), SS_QUARTER);
    if (e == hipSuccess) e = b->desc.reserve(list.size() * SS_F * sizeof(float), SS_QUARTER);
    if (e != hipSuccess) { err = std::string(who) + hipGetErrorString(e); return SS_ERR_HIP; }
    SS_HIPCHK(who, hipMemcpyAsync(b->ids.as<int>(), list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bank_desc, dim3((unsigned)((list.size() + 3) / 4)), dim3(256), 0, st, d.sum + (size_t)stream * M * SS_F, b->ids.as<int>(),
                       (int)list.size(), b->desc.as<float>());
    SS_HIPCHK(who, hipGetLastError());
    SS_HIPCHK(who, hipMemcpyAsync(desc, b->desc.as<float>(), list.size() * SS_F * sizeof(float), hipMemcpyDeviceToHost, st));
    SS_HIPCHK(who, hipStreamSynchronize(st));
    return SS_OK;
}

int ss_mtmc_link_check_impl(int T, const float* desc, const int* cam, const int* first, const int* last, const int* n, double thr, int min_rows,
                            const int* global_id, const double* merges, const int* n_merges, std::string& err)
{
    const std::string who = "ss_mtmc_link: ";
    if (T < 1) { err = who + "T " + std::to_string(T) + " tracklets, at least 1"; return SS_ERR_INVALID; }
    if (T > MT_MAX) { err = who + "T " + std::to_string(T) + " tracklets is over the cap of " + std::to_string(MT_MAX); return SS_ERR_CAPACITY; }
    if (!desc || !cam || !first || !last || !n || !global_id || !n_merges || (T > 1 && !merges)) { err = who + "null argument"; return SS_ERR_INVALID; }
    if (!(thr == thr) || std::isinf(thr)) { err = who + "thr must be finite"; return SS_ERR_INVALID; }
    return SS_OK;
}

int ss_mtmc_link_impl(SSMtmc** pg, hipStream_t st, int T, const float* desc, const int* cam, const int* first, const int* last, const int* n, double thr,
                      int min_rows, int* global_id, double* merges, int* n_merges, float* dist_out, std::string& err)
{
    const char* who = "ss_mtmc_link: ";
    if (!pg) { err = std::string(who) + "null context"; return SS_ERR_INVALID; }
    if (!*pg) *pg = new SSMtmc();
    SSMtmc* g = *pg;
    const size_t TT = (size_t)T * T;
    const int W = (T + 63) / 64;
    hipError_t e = g->desc.reserve((size_t)T * SS_F * sizeof(float), SS_QUARTER);
    if (e == hipSuccess) e = g->D.reserve(TT * sizeof(float), SS_QUARTER);
    if (e == hipSuccess) e = g->d.reserve(TT * sizeof(double), SS_QUARTER);
    if (e == hipSuccess) e = g->conf.reserve((size_t)T * W * sizeof(unsigned long long), SS_QUARTER);
    if (e == hipSuccess) e = g->ints.reserve(((size_t)5 * T + 1) * sizeof(int), SS_QUARTER);
    if (e == hipSuccess) e = g->merges.reserve((size_t)3 * T * sizeof(double), SS_QUARTER);
    if (e != hipSuccess) { err = std::string(who) + hipGetErrorString(e); return SS_ERR_HIP; }
    int* di = g->ints.as<int>();
    std::vector<int> hi((size_t)4 * T);
    memcpy(hi.data(), cam, T * sizeof(int)); memcpy(hi.data() + T, first, T * sizeof(int));
    memcpy(hi.data() + 2 * (size_t)T, last, T * sizeof(int)); memcpy(hi.data() + 3 * (size_t)T, n, T * sizeof(int));
    SS_HIPCHK(who, hipMemcpyAsync(di, hi.data(), hi.size() * sizeof(int), hipMemcpyHostToDevice, st));
    SS_HIPCHK(who, hipMemcpyAsync(g->desc.as<float>(), desc, (size_t)T * SS_F * sizeof(float), hipMemcpyHostToDevice, st));
    SS_HIPCHK(who, hipMemsetAsync(g->D.as<float>(), 0, TT * sizeof(float), st));
    const int nt = (T + MT_TILE - 1) / MT_TILE;
    hipLaunchKernelGGL(k_mtmc_dist, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, st, g->desc.as<float>(), T, nt, g->D.as<float>());
    SS_HIPCHK(who, hipGetLastError());
    MtArgs a;
    a.T = T; a.W = W; a.min_rows = min_rows; a.thr = thr; a.D = g->D.as<float>();
    a.cam = di; a.first = di + T; a.last = di + 2 * (size_t)T; a.n = di + 3 * (size_t)T;
    a.d = g->d.as<double>(); a.conf = g->conf.as<unsigned long long>(); a.root = di + 4 * (size_t)T; a.n_merges = di + 5 * (size_t)T;
    a.merges = g->merges.as<double>();
    const size_t want = (TT + 255) / 256;
    hipLaunchKernelGGL(k_mtmc_init, dim3((unsigned)(want < 1024 ? want : 1024)), dim3(256), 0, st, a);
    SS_HIPCHK(who, hipGetLastError());
    hipLaunchKernelGGL(k_mtmc_cluster, dim3(1), dim3(MT_THREADS), 0, st, a);
    SS_HIPCHK(who, hipGetLastError());
    std::vector<int> root((size_t)T + 1);
    SS_HIPCHK(who, hipMemcpyAsync(root.data(), a.root, ((size_t)T + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
    if (dist_out) SS_HIPCHK(who, hipMemcpyAsync(dist_out, g->D.as<float>(), TT * sizeof(float), hipMemcpyDeviceToHost, st));
    SS_HIPCHK(who, hipStreamSynchronize(st));
    const int nm = root[T];
    if (nm < 0 || nm >= T) { err = std::string(who) + "merge count out of range"; return SS_ERR_HIP; }
    if (nm) SS_HIPCHK(who, hipMemcpy(merges, a.merges, (size_t)3 * nm * sizeof(double), hipMemcpyDeviceToHost));
    *n_merges = nm;
    // a cluster's root is its smallest tracklet; global ids count the roots in rising order
    int next = 0;
    for (int i = 0; i < T; ++i) {
        int r = i;
        while (root[r] >= 0 && root[r] < r) r = root[r];         // (roots point down: r only falls)
        global_id[i] = r == i ? ++next : global_id[r];
    }
    return SS_OK;
}
