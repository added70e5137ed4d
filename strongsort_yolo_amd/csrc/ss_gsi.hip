// ss_gsi.hip — GSI post-processing (docs/GSI.md): the Gaussian-process smoothing of every track of a finished run, one workgroup
// per track.  Per track of n rows: A = K + alpha I with K_ij = ss_expneg(d d / (2 l l)), the Cholesky factor of A, the forward and
// backward solves of four right-hand sides (x1, y1, w, h) and the posterior mean K a — all plain f64 VALU in the element order of
// docs/GSI.md §3, which tests/gsi_ref.py restates; the file is built with -ffp-contract=off, `/` and sqrt are correctly rounded.
//
// Storage: the packed lower triangle by rows (row i at i (i + 1) / 2) followed by the four right-hand sides as rows n .. n+3 of
// length n: the forward solve z_i = (y_i - sum_k L_ik z_k) / L_ii is the Cholesky recurrence of an extra row, so it rides along.
//   G = false  n <= GSI_LDS_MAX: the whole image in LDS (up to 160 512 bytes), 256 threads.
//   G = true   n <= GSI_MAX_LEN: the image in a scratch slot of device memory (at most 4.2 MB), 1024 threads; the panel being
//              factorised is staged in LDS column by column (k-major), so the trailing update reads whole 32-byte runs.
// Both run the same schedule: panels of GSI_PANEL columns, factorised right-looking column by column (pivot, scale, update of the
// panel's later columns), then the trailing GSI_TILE x GSI_TILE tiles behind the panel take the panel's k in rising order in
// registers.  Every element therefore sees s = s - L_ik L_jk for k = 0, 1, .. j-1, each product rounded before it is subtracted.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "ss_common.h"
#include "ss_host.h"
#include "ss_launch.h"
#include "ss_expneg.h"

#define GSI_MAX_LEN 1024
#define GSI_LDS_MAX 192         // (192 * 193 / 2 + 8 * 192) * 8 = 160 512 bytes of the 163 840 a workgroup may declare
#define GSI_PANEL 16
#define GSI_TILE 4
#define GSI_RS 1048             // rows of the staged panel image: GSI_MAX_LEN + 4 right-hand sides + the ragged last tile, a multiple of 4
#define GSI_SLOTS 256           // scratch slots = workgroups of the long-track launch at most (one per compute unit)
#define GSI_NT_LDS 256
#define GSI_NT_GLB 1024

struct GsiArgs {
    const int2* desc;           // per track of the launch {first packed row, rows}, by falling length
    const int* frames;          // packed rows
    const double* vals;         // [rows][4]
    const double* len;          // per track
    double* out;                // [rows][4]
    int* status;                // per track
    double* scratch;            // G: gridDim.x slots of slot_doubles
    size_t slot_doubles;
    double alpha;
    int n_tracks;
};

template <bool G, int NT>
__device__ inline void gsi_track(const GsiArgs& a, const int t, double* __restrict__ lds)
{
    static_assert(NT >= (G ? GSI_MAX_LEN : GSI_LDS_MAX), "one thread per row in the backward solve");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = a.desc[t].x, n = a.desc[t].y;
    const int* __restrict__ fr = a.frames + base;
    const double* __restrict__ y = a.vals + (size_t)base * 4;
    double* __restrict__ out = a.out + (size_t)base * 4;
    const double l = a.len[t], alpha = a.alpha;
    const double den = (2.0 * l) * l;
    const int R = n + 4, tri_n = n * (n + 1) / 2;
    double* __restrict__ gT = G ? a.scratch + (size_t)blockIdx.x * a.slot_doubles : nullptr;
    double* abuf = G ? lds : lds + tri_n + 4 * n;        // [n][4] the weights a, once the factor is final
    auto off = [&](int i) { return i < n ? i * (i + 1) / 2 : tri_n + (i - n) * n; };
    // the image: element (i, j), j <= i or i >= n
    auto ldT = [&](int i, int j) -> double { if constexpr (G) return gT[off(i) + j]; else return lds[off(i) + j]; };
    auto stT = [&](int i, int j, double v) { if constexpr (G) gT[off(i) + j] = v; else lds[off(i) + j] = v; };

    // ---- A and the right-hand sides ----
    for (int i = wave; i < n; i += NT / 64) {
        const long long fi = fr[i];
        for (int j = lane; j <= i; j += 64) {
            const double d = (double)(fi - (long long)fr[j]);
            double v = ss_expneg((d * d) / den);
            if (j == i) v = v + alpha;
            stT(i, j, v);
        }
    }
    for (int i = tid; i < n; i += NT)
#pragma unroll
        for (int r = 0; r < 4; ++r) stT(n + r, i, y[(size_t)i * 4 + r]);
    __syncthreads();

    // ---- Cholesky with the forward solve riding along, panel by panel ----
    bool failed = false;
    for (int p0 = 0; p0 < n && !failed; p0 += GSI_PANEL) {
        const int p1 = min(p0 + GSI_PANEL, n);
        // the panel: element (i, k), p0 <= k < p1, i >= k
        auto ldP = [&](int i, int k) -> double { if constexpr (G) return lds[(k - p0) * GSI_RS + (i - p0)]; else return lds[off(i) + k]; };
        auto stP = [&](int i, int k, double v) { if constexpr (G) lds[(k - p0) * GSI_RS + (i - p0)] = v; else lds[off(i) + k] = v; };
        if constexpr (G) {
            for (int e = tid; e < (R - p0) * GSI_PANEL; e += NT) {
                const int i = p0 + (e >> 4), k = p0 + (e & 15);
                if (k < p1 && k <= i) stP(i, k, gT[off(i) + k]);
            }
            __syncthreads();
        }
        for (int c = p0; c < p1; ++c) {
            const double s = ldP(c, c);                 // the same value in every thread: the exit is uniform
            if (!(s > 0.0)) { failed = true; break; }
            const double d = sqrt(s);
            for (int i = c + 1 + tid; i < R; i += NT) stP(i, c, ldP(i, c) / d);
            __syncthreads();
            if (tid == 0) stP(c, c, d);
            for (int c2 = c + 1; c2 < p1; ++c2) {
                const double ljk = ldP(c2, c);
                for (int i = c2 + tid; i < R; i += NT) stP(i, c2, ldP(i, c2) - ldP(i, c) * ljk);
            }
            __syncthreads();
        }
        if (failed) break;
        if constexpr (G) {
            for (int e = tid; e < (R - p0) * GSI_PANEL; e += NT) {
                const int i = p0 + (e >> 4), k = p0 + (e & 15);
                if (k < p1 && k <= i) gT[off(i) + k] = ldP(i, k);
            }
        }
        if (p1 < n) {                                   // a whole panel: GSI_PANEL products per trailing element, rising k
            const int nbj = (n - p1 + GSI_TILE - 1) / GSI_TILE, nbi = (R - p1 + GSI_TILE - 1) / GSI_TILE;
            for (int tix = tid; tix < nbi * nbj; tix += NT) {
                const int bi = tix / nbj, bj = tix - bi * nbj;
                if (bj > bi) continue;
                const int i0 = p1 + GSI_TILE * bi, j0 = p1 + GSI_TILE * bj;
                double acc[GSI_TILE][GSI_TILE];
#pragma unroll
                for (int qi = 0; qi < GSI_TILE; ++qi)
#pragma unroll
                    for (int qj = 0; qj < GSI_TILE; ++qj) {
                        const int i = i0 + qi, j = j0 + qj;
                        acc[qi][qj] = (i < R && j < n && j <= i) ? ldT(i, j) : 0.0;
                    }
#pragma unroll 4
                for (int k = p0; k < p0 + GSI_PANEL; ++k) {
                    double li[GSI_TILE], lj[GSI_TILE];
#pragma unroll
                    for (int q = 0; q < GSI_TILE; ++q) {
                        if constexpr (G) { li[q] = ldP(i0 + q, k); lj[q] = ldP(j0 + q, k); }          // rows past R: unused slack of the image
                        else { li[q] = ldP(min(i0 + q, R - 1), k); lj[q] = ldP(min(j0 + q, n - 1), k); }
                    }
#pragma unroll
                    for (int qi = 0; qi < GSI_TILE; ++qi)
#pragma unroll
                        for (int qj = 0; qj < GSI_TILE; ++qj) acc[qi][qj] = acc[qi][qj] - li[qi] * lj[qj];
                }
#pragma unroll
                for (int qi = 0; qi < GSI_TILE; ++qi)
#pragma unroll
                    for (int qj = 0; qj < GSI_TILE; ++qj) {
                        const int i = i0 + qi, j = j0 + qj;
                        if (i < R && j < n && j <= i) stT(i, j, acc[qi][qj]);
                    }
            }
        }
        __syncthreads();
    }
    if (failed) {                                       // status 1: the rows pass through
        for (int i = tid; i < n; i += NT)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)i * 4 + r] = y[(size_t)i * 4 + r];
        if (tid == 0) a.status[t] = 1;
        return;
    }

    // ---- backward solve: thread i keeps z_i of the four columns; a_k leaves through abuf, rows of L come a step ahead ----
    double z[4] = { 0.0, 0.0, 0.0, 0.0 }, lii = 1.0;
    if (tid < n) {
#pragma unroll
        for (int r = 0; r < 4; ++r) z[r] = ldT(n + r, tid);
        lii = ldT(tid, tid);
    }
    __syncthreads();                                    // G: abuf overlays the panel image, whose last readers are done
    for (int k = n - 1; k >= 0; --k) {
        if (tid == k) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { z[r] = z[r] / lii; abuf[k * 4 + r] = z[r]; }
        }
        const double lk = tid < k ? ldT(k, tid) : 0.0;
        __syncthreads();
        if (tid < k) {
#pragma unroll
            for (int r = 0; r < 4; ++r) z[r] = z[r] - lk * abuf[k * 4 + r];
        }
    }

    // ---- posterior mean: m_i = sum_k K_ik a_k, k rising from 0.0 ----
    if (tid < n) {
        const long long fi = fr[tid];
        double m[4] = { 0.0, 0.0, 0.0, 0.0 };
        for (int k = 0; k < n; ++k) {
            const double d = (double)(fi - (long long)fr[k]);
            const double kv = ss_expneg((d * d) / den);
#pragma unroll
            for (int r = 0; r < 4; ++r) m[r] = m[r] + kv * abuf[k * 4 + r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(size_t)tid * 4 + r] = m[r];
    }
    if (tid == 0) a.status[t] = 0;
}

// One workgroup per track (G: per scratch slot, walking the long tracks grid-strided), tracks by falling length.
template <bool G, int NT>
__global__ __launch_bounds__(NT) void k_gsi_smooth(const GsiArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double gsi_lds[];
    for (int t = blockIdx.x; t < a.n_tracks; t += gridDim.x) {
        gsi_track<G, NT>(a, t, gsi_lds);
        __syncthreads();                                // the next track reuses the LDS and the slot
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct SSGsi {
    SsBuf<SS_PINNED> host;                              // the upload image, then the download image
    SsBuf<SS_DEVICE> dev;
    SsBuf<SS_DEVICE> scratch;                           // the long tracks' slots, grown when a call needs more
    SsEvent ev;
    bool attr = false;
};

void ss_gsi_free(SSGsi* g) { delete g; }

int ss_gsi_max_len_impl() { return GSI_MAX_LEN; }

// every refusal of ss_gsi_smooth, made on the host before a context or the device is looked at
int ss_gsi_check_impl(int n_tracks, const int* offsets, const int* frames, const double* vals, const double* len_scale, double alpha,
                      const double* out, const int* status, std::string& err)
{
    const std::string who = "ss_gsi_smooth: ";
    if (!offsets || !frames || !vals || !len_scale || !out || !status) { err = who + "null argument"; return SS_ERR_INVALID; }
    if (n_tracks < 1 || n_tracks > 65536) { err = who + "n_tracks must be 1 .. 65536"; return SS_ERR_INVALID; }
    if (!std::isfinite(alpha) || !(alpha >= 0.0)) { err = who + "alpha must be finite and >= 0"; return SS_ERR_INVALID; }
    if (offsets[0] != 0) { err = who + "offsets[0] must be 0"; return SS_ERR_INVALID; }
    for (int t = 0; t < n_tracks; ++t) {
        const std::string tr = "track " + std::to_string(t) + ": ";
        if (offsets[t + 1] < offsets[t]) { err = who + tr + "offsets decrease"; return SS_ERR_INVALID; }
        if (!std::isfinite(len_scale[t]) || !(len_scale[t] > 0.0)) { err = who + tr + "len_scale must be finite and > 0"; return SS_ERR_INVALID; }
        for (int i = offsets[t]; i < offsets[t + 1]; ++i) {
            if (i > offsets[t] && frames[i] <= frames[i - 1]) { err = who + tr + "frames must increase strictly"; return SS_ERR_INVALID; }
            for (int r = 0; r < 4; ++r)
                if (!std::isfinite(vals[(size_t)i * 4 + r])) { err = who + tr + "a value is NaN or infinite"; return SS_ERR_INVALID; }
        }
    }
    return SS_OK;
}

static size_t gsi_image_doubles(int n) { return (size_t)n * (n + 1) / 2 + (size_t)4 * n; }

int ss_gsi_smooth_impl(SSGsi** pg, hipStream_t stream, int n_tracks, const int* offsets, const int* frames, const double* vals,
                       const double* len_scale, double alpha, double* out, int* status, std::string& err)
{
    // tracks the device takes, by falling length (stable: equal lengths keep the caller's order); the others are settled here
    std::vector<int> order;
    for (int t = 0; t < n_tracks; ++t) {
        const int n = offsets[t + 1] - offsets[t];
        if (n > GSI_MAX_LEN) {
            status[t] = 2;
            memcpy(out + (size_t)offsets[t] * 4, vals + (size_t)offsets[t] * 4, (size_t)n * 4 * sizeof(double));
        } else if (n == 0) status[t] = 0;
        else order.push_back(t);
    }
    if (order.empty()) return SS_OK;
    if (!pg) { err = "ss_gsi_smooth: null context"; return SS_ERR_INVALID; }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return offsets[a + 1] - offsets[a] > offsets[b + 1] - offsets[b]; });
    const size_t nd = order.size();
    size_t rows = 0, n_glb = 0;
    for (int t : order) { const int n = offsets[t + 1] - offsets[t]; rows += n; n_glb += n > GSI_LDS_MAX; }
    // upload image: vals | len | desc | frames;  download image: out | status
    SsLayout lay{0, 8};
    lay.take(rows * 4 * sizeof(double));                // vals at 0
    const size_t o_len = lay.take(nd * sizeof(double)), o_desc = lay.take(nd * sizeof(int2)), o_fr = lay.take(rows * sizeof(int));
    const size_t up = lay.at;
    const size_t o_stat = rows * 4 * sizeof(double), down = ss_align_up(o_stat + nd * sizeof(int), 8);
    if (!*pg) *pg = new SSGsi();
    SSGsi& g = **pg;
    const char* const who = "ss_gsi_smooth: ";
    SS_HIPCHK(who, g.ev.ensure());
    SS_HIPCHK(who, g.host.reserve(up + down, SS_QUARTER));
    SS_HIPCHK(who, g.dev.reserve(up + down, SS_QUARTER));
    const int slots = (int)std::min<size_t>(n_glb, GSI_SLOTS);
    const size_t slot_doubles = n_glb ? gsi_image_doubles(offsets[order[0] + 1] - offsets[order[0]]) : 0;
    SS_HIPCHK(who, g.scratch.reserve(slot_doubles * slots * sizeof(double), SS_EXACT));
    if (!g.attr) {
        SS_HIPCHK(who, hipFuncSetAttribute((const void*)k_gsi_smooth<false, GSI_NT_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        SS_HIPCHK(who, hipFuncSetAttribute((const void*)k_gsi_smooth<true, GSI_NT_GLB>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        g.attr = true;
    }
    char* h = g.host.as();
    double* h_vals = (double*)h; double* h_len = (double*)(h + o_len); int2* h_desc = (int2*)(h + o_desc); int* h_fr = (int*)(h + o_fr);
    size_t at = 0;
    for (size_t k = 0; k < nd; ++k) {
        const int t = order[k], n = offsets[t + 1] - offsets[t];
        memcpy(h_vals + at * 4, vals + (size_t)offsets[t] * 4, (size_t)n * 4 * sizeof(double));
        memcpy(h_fr + at, frames + offsets[t], (size_t)n * sizeof(int));
        h_len[k] = len_scale[t];
        h_desc[k] = make_int2((int)at, n);
        at += n;
    }
    char* d = g.dev.as();
    SS_HIPCHK(who, hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, stream));
    GsiArgs a;
    a.frames = (const int*)(d + o_fr); a.vals = (const double*)d; a.out = (double*)(d + up); a.alpha = alpha;
    a.scratch = g.scratch.as<double>(); a.slot_doubles = slot_doubles;
    if (n_glb) {                                        // the long tracks first
        a.desc = (const int2*)(d + o_desc); a.len = (const double*)(d + o_len); a.status = (int*)(d + up + o_stat); a.n_tracks = (int)n_glb;
        hipLaunchKernelGGL((k_gsi_smooth<true, GSI_NT_GLB>), dim3(slots), dim3(GSI_NT_GLB), GSI_PANEL * GSI_RS * sizeof(double), stream, a);
        SS_HIPCHK(who, hipGetLastError());
    }
    if (nd > n_glb) {
        const int nmax = offsets[order[n_glb] + 1] - offsets[order[n_glb]];
        a.desc = (const int2*)(d + o_desc) + n_glb; a.len = (const double*)(d + o_len) + n_glb; a.status = (int*)(d + up + o_stat) + n_glb;
        a.n_tracks = (int)(nd - n_glb);
        hipLaunchKernelGGL((k_gsi_smooth<false, GSI_NT_LDS>), dim3((unsigned)(nd - n_glb)), dim3(GSI_NT_LDS), (gsi_image_doubles(nmax) + (size_t)4 * nmax) * sizeof(double),
                           stream, a);
        SS_HIPCHK(who, hipGetLastError());
    }
    SS_HIPCHK(who, hipMemcpyAsync(h + up, d + up, down, hipMemcpyDeviceToHost, stream));
    SS_HIPCHK(who, hipEventRecord(g.ev, stream));
    SS_HIPCHK(who, hipEventSynchronize(g.ev));
    const double* h_out = (const double*)(h + up); const int* h_stat = (const int*)(h + up + o_stat);
    at = 0;
    for (size_t k = 0; k < nd; ++k) {
        const int t = order[k], n = offsets[t + 1] - offsets[t];
        memcpy(out + (size_t)offsets[t] * 4, h_out + at * 4, (size_t)n * 4 * sizeof(double));
        status[t] = h_stat[k];
        at += n;
    }
    return SS_OK;
}
