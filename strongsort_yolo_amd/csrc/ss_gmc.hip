// ss_gmc.hip — sparse-optical-flow camera motion (docs/BYTETRACK.md §1f, decisions S-01..): this project's restatement of
// Ultralytics' `gmc_method: sparseOptFlow` — Shi-Tomasi corners on a half-size grey frame, pyramidal Lucas-Kanade from the previous
// frame, a RANSAC similarity fit.  Arithmetic = tests/sparse_gmc_ref.py operation for operation: the image stages are integer, the
// eigenvalue is one float32 formula, Lucas-Kanade and the fit are float64 with the sums in a fixed lane order (the library is built
// with -ffp-contract=off) -> bit-identical warps.  Like ECC (ss_cmc.hip) the estimate is stateless per frame pair: a whole group is
// one batch of launches beside the detector, and the warps go to k_byte_group's GMC variant in ss_cmc_estimate's layout.
#include "ss_common.h"
#include "ss_launch.h"

#define GMC_WIN 21
#define GMC_WIN_N (GMC_WIN * GMC_WIN)
#define GMC_EL 7                        // window elements per lane: lane l takes l, l + 64, ..
#define GMC_NHYP 1024                   // S-09: hypotheses, one per thread of the fit's workgroup

__device__ inline int gmc_r101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
__device__ inline int gmc_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }
__device__ inline int gmc_grey(const uint8_t* p) { return (p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + 8192) >> 14; }

// S-02.  grid = (ceil(w0*h0 / 256), images); image i of the group goes to pyramid slot i + S (slots 0..S-1: the remembered frames)
__global__ __launch_bounds__(256) void k_gmc_half(SSGmcDev g, const uint8_t* __restrict__ src, long long src_stride, int row_stride)
{
    const int p = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
    if (p == 0) g.emax[img] = 0u;
    if (p >= g.lw[0] * g.lh[0]) return;
    const int y = p / g.lw[0], x = p - y * g.lw[0];
    const uint8_t* r0 = src + (size_t)img * src_stride + (size_t)(2 * y) * row_stride + 6 * x;
    const uint8_t* r1 = r0 + row_stride;
    g.pyr[(size_t)(img + g.S) * g.pyr_stride + p] = (uint8_t)((gmc_grey(r0) + gmc_grey(r0 + 3) + gmc_grey(r1) + gmc_grey(r1 + 3) + 2) >> 2);
}

// S-03: level L -> L + 1.  grid = (ceil(ow*oh / 256), images)
__global__ __launch_bounds__(256) void k_gmc_pyrdown(SSGmcDev g, int L)
{
    const int ow = g.lw[L + 1], oh = g.lh[L + 1], w = g.lw[L], h = g.lh[L];
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= ow * oh) return;
    uint8_t* base = g.pyr + (size_t)(blockIdx.y + g.S) * g.pyr_stride;
    const uint8_t* __restrict__ a = base + g.loff[L];
    const int y = p / ow, x = p - y * ow;
    const int k[5] = { 1, 4, 6, 4, 1 };
    int acc = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const uint8_t* row = a + (size_t)gmc_r101(2 * y + i - 2, h) * w;
        int t = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) t += k[j] * row[gmc_r101(2 * x + j - 2, w)];
        acc += k[i] * t;
    }
    base[g.loff[L + 1] + p] = (uint8_t)((acc + 128) >> 8);
}

// S-04: the smaller eigenvalue of the 3x3 box sums of the Sobel products, and the image's maximum (non-negative floats order as
// their bits).  grid = (ceil(w0*h0 / 256), images)
__global__ __launch_bounds__(256) void k_gmc_eig(SSGmcDev g)
{
    const int w = g.lw[0], h = g.lh[0], npix = w * h;
    const int p = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
    float lam = 0.0f;
    if (p < npix) {
        const uint8_t* __restrict__ a = g.pyr + (size_t)(img + g.S) * g.pyr_stride;
        const int y = p / w, x = p - y * w;
        int P[5][5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const uint8_t* row = a + (size_t)gmc_r101(y + i - 2, h) * w;
#pragma unroll
            for (int j = 0; j < 5; ++j) P[i][j] = row[gmc_r101(x + j - 2, w)];
        }
        int sxx = 0, sxy = 0, syy = 0;
#pragma unroll
        for (int i = 1; i < 4; ++i)
#pragma unroll
            for (int j = 1; j < 4; ++j) {
                const int gx = (P[i - 1][j + 1] - P[i - 1][j - 1]) + 2 * (P[i][j + 1] - P[i][j - 1]) + (P[i + 1][j + 1] - P[i + 1][j - 1]);
                const int gy = (P[i + 1][j - 1] - P[i - 1][j - 1]) + 2 * (P[i + 1][j] - P[i - 1][j]) + (P[i + 1][j + 1] - P[i - 1][j + 1]);
                sxx += gx * gx; sxy += gx * gy; syy += gy * gy;
            }
        const float fa = (float)sxx * 0.5f, fc = (float)syy * 0.5f, fb = (float)sxy;
        const float d = fa - fc;
        lam = (fa + fc) - sqrtf(d * d + fb * fb);
        g.eig[(size_t)img * npix + p] = lam;
    }
    float m = fmaxf(lam, 0.0f);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(g.emax + img, __float_as_uint(m));
}

// S-05: candidates = positive, >= 0.01f * max, and equal to the maximum of their in-frame 3x3 neighbourhood
__global__ __launch_bounds__(256) void k_gmc_cand(SSGmcDev g)
{
    const int w = g.lw[0], h = g.lh[0], npix = w * h;
    const int p = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
    if (p >= npix) return;
    const float* __restrict__ e = g.eig + (size_t)img * npix;
    const float thr = 0.01f * __uint_as_float(g.emax[img]);
    const float lam = e[p];
    bool ok = lam > 0.0f && lam >= thr;
    if (ok) {
        const int y = p / w, x = p - y * w;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int yy = y + dy, xx = x + dx;
                if (yy >= 0 && yy < h && xx >= 0 && xx < w && e[yy * w + xx] > lam) ok = false;
            }
    }
    g.cand[(size_t)img * npix + p] = ok ? __float_as_uint(lam) : 0u;
}

// S-05: the first SS_GMC_MAXC candidates under (value descending, pixel index ascending).  One workgroup of 1024 per image: a
// radix select on the float bits finds the value of the last kept candidate, a pass in index order collects what is kept (ties at
// that value by index), a bitonic sort on (bits, ~index) orders them.  A total order: any selection algorithm gives this list.
__global__ __launch_bounds__(1024) void k_gmc_select(SSGmcDev g)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned sh_prefix, sh_k, sh_all, sh_total;
    __shared__ int w_gt[16], w_eq[16];
    __shared__ unsigned long long keys[1024];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, img = blockIdx.x;
    const int npix = g.lw[0] * g.lh[0];
    const unsigned* __restrict__ cm = g.cand + (size_t)img * npix;
    if (tid == 0) { sh_prefix = 0u; sh_k = SS_GMC_MAXC; sh_all = 0u; sh_total = 0u; }
    keys[tid] = 0ull;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        const unsigned prefix = sh_prefix;
        for (int p = tid; p < npix; p += 1024) {
            const unsigned v = cm[p];
            if (v && (pass == 0 || (v >> (shift + 8)) == prefix)) atomicAdd(&hist[(v >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned cum = 0u, k = sh_k;
            int b = 255;
            for (; b >= 0; --b) {
                if (cum + hist[b] >= k) break;
                cum += hist[b];
            }
            if (pass == 0) {
                unsigned tot = 0u;
                for (int q = 0; q < 256; ++q) tot += hist[q];
                sh_total = tot;
            }
            if (b < 0) sh_all = 1u;                         // fewer candidates than MAXC: all are kept (only pass 0 can see this)
            else { sh_k = k - cum; sh_prefix = (prefix << 8) | (unsigned)b; }
        }
        __syncthreads();
        if (sh_all) break;
    }
    const unsigned T = sh_all ? 0u : sh_prefix;
    // index order: wave wv owns a contiguous range, 64 consecutive pixels per step
    const int wchunk = ((npix + 15) / 16 + 63) / 64 * 64;
    const int lo = wv * wchunk, hi = min(npix, lo + wchunk);
    int n_gt = 0, n_eq = 0;
    for (int b0 = lo; b0 < hi; b0 += 64) {
        const int p = b0 + lane;
        const unsigned v = p < hi ? cm[p] : 0u;
        n_gt += __popcll(__ballot(v > T));
        n_eq += __popcll(__ballot(T > 0u && v == T));
    }
    if (lane == 0) { w_gt[wv] = n_gt; w_eq[wv] = n_eq; }
    __syncthreads();
    int off_gt = 0, off_eq = 0, tot_gt = 0, tot_eq = 0;
    for (int q = 0; q < 16; ++q) {
        if (q < wv) { off_gt += w_gt[q]; off_eq += w_eq[q]; }
        tot_gt += w_gt[q]; tot_eq += w_eq[q];
    }
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int b0 = lo; b0 < hi; b0 += 64) {
        const int p = b0 + lane;
        const unsigned v = p < hi ? cm[p] : 0u;
        const bool gt = v > T, eq = T > 0u && v == T;
        const unsigned long long mg = __ballot(gt), me = __ballot(eq);
        int pos = -1;
        if (gt) pos = off_gt + __popcll(mg & lt);
        else if (eq) pos = tot_gt + off_eq + __popcll(me & lt);
        if (pos >= 0 && pos < SS_GMC_MAXC) keys[pos] = ((unsigned long long)v << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)p);
        off_gt += __popcll(mg); off_eq += __popcll(me);
    }
    const int n = min(SS_GMC_MAXC, tot_gt + tot_eq);
    __syncthreads();
    for (int k = 2; k <= 1024; k <<= 1)                       // bitonic sort, descending
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int q = tid ^ j;
            if (q > tid) {
                const unsigned long long a = keys[tid], b = keys[q];
                const bool desc = (tid & k) == 0;
                if (desc ? a < b : a > b) { keys[tid] = b; keys[q] = a; }
            }
            __syncthreads();
        }
    const size_t slot = (size_t)img + g.S;
    if (tid < SS_GMC_MAXC) g.corners[slot * SS_GMC_MAXC + tid] = tid < n ? (int)(0xFFFFFFFFu - (unsigned)(keys[tid] & 0xFFFFFFFFull)) : 0;
    if (tid == 0) { g.ncorner[slot] = n; g.ncand[slot] = (int)sh_total; }
}

// pair (f, s): previous = slot f*S + s, current = slot (f+1)*S + s.  A warp needs a remembered or in-group predecessor, a real
// frame, and at least one corner in either image (S-12).
__device__ inline bool gmc_pair_valid(const SSGmcDev& g, int f, int s, const int* n_valid)
{
    if (f == 0 && !g.prev_valid[s]) return false;
    if (n_valid && f >= *n_valid) return false;
    return g.ncorner[f * g.S + s] > 0 && g.ncorner[(f + 1) * g.S + s] > 0;
}

__device__ inline double gmc_wave_sum(double p)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_xor(p, off);
    return p;
}
__device__ inline double gmc_bilerp(double v00, double v01, double v10, double v11, double fx, double fy)
{
    const double a = v00 + fx * (v01 - v00);
    const double b = v10 + fx * (v11 - v10);
    return a + fy * (b - a);
}

// S-06..S-08: pyramidal Lucas-Kanade, one wave per (pair, corner); grid = (MAXC / 4, pairs), 256 threads.  Lane l holds window
// elements l, l + 64, .. of the template and its two derivative patches in registers across the iterations.
__global__ __launch_bounds__(256) void k_gmc_lk(SSGmcDev g, const int* __restrict__ n_valid)
{
    const int lane = threadIdx.x & 63, pt = blockIdx.x * 4 + (threadIdx.x >> 6), pair = blockIdx.y;
    const int f = pair / g.S, s = pair - f * g.S;
    const size_t o = (size_t)pair * SS_GMC_MAXC + pt;
    const bool run = gmc_pair_valid(g, f, s, n_valid) && pt < g.ncorner[f * g.S + s];
    if (!run) {
        if (lane == 0) { g.pts[o * 2] = 0.0; g.pts[o * 2 + 1] = 0.0; g.status[o] = 0; }
        return;
    }
    const uint8_t* __restrict__ pyr0 = g.pyr + (size_t)(f * g.S + s) * g.pyr_stride;
    const uint8_t* __restrict__ pyr1 = g.pyr + (size_t)((f + 1) * g.S + s) * g.pyr_stride;
    const int cidx = g.corners[(size_t)(f * g.S + s) * SS_GMC_MAXC + pt];
    const int cy = cidx / g.lw[0], cx = cidx - cy * g.lw[0];
    int ei[GMC_EL], ej[GMC_EL];
#pragma unroll
    for (int k = 0; k < GMC_EL; ++k) { const int e = lane + 64 * k; ei[k] = e / GMC_WIN; ej[k] = e - ei[k] * GMC_WIN; }
    double nx = 0.0, ny = 0.0;
    int status = 1;
    for (int L = SS_GMC_LEVELS - 1; L >= 0 && status; --L) {
        const int w = g.lw[L], h = g.lh[L];
        const uint8_t* __restrict__ I = pyr0 + g.loff[L];
        const uint8_t* __restrict__ J = pyr1 + g.loff[L];
        const double scale = 1.0 / (double)(1 << L);
        const double px = (double)cx * scale, py = (double)cy * scale;
        const double xmax = (double)(g.lw[0] - 1) * scale, ymax = (double)(g.lh[0] - 1) * scale;
        if (L == SS_GMC_LEVELS - 1) { nx = px; ny = py; } else { nx = nx * 2.0; ny = ny * 2.0; }
        double Iw[GMC_EL], Dx[GMC_EL], Dy[GMC_EL];
        {
            const double bx = px - 10.0, by = py - 10.0;
            const double fbx = floor(bx), fby = floor(by);
            const double fx = bx - fbx, fy = by - fby;
            const int ix = (int)fbx, iy = (int)fby;
#pragma unroll
            for (int k = 0; k < GMC_EL; ++k) {
                Iw[k] = 0.0; Dx[k] = 0.0; Dy[k] = 0.0;
                if (lane + 64 * k < GMC_WIN_N) {
                    int P[4][4];                                      // the replicate-extended level around the element's 2x2 cell
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const uint8_t* row = I + (size_t)gmc_clamp(iy + ei[k] + a - 1, h) * w;
#pragma unroll
                        for (int b = 0; b < 4; ++b) P[a][b] = row[gmc_clamp(ix + ej[k] + b - 1, w)];
                    }
                    double vi[4], vx[4], vy[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int a = c >> 1, b = c & 1;              // cell corner (row a, column b)
                        vi[c] = (double)P[a + 1][b + 1];
                        vx[c] = (double)(3 * (P[a][b + 2] - P[a][b]) + 10 * (P[a + 1][b + 2] - P[a + 1][b]) + 3 * (P[a + 2][b + 2] - P[a + 2][b])) * 0.03125;
                        vy[c] = (double)(3 * (P[a + 2][b] - P[a][b]) + 10 * (P[a + 2][b + 1] - P[a][b + 1]) + 3 * (P[a + 2][b + 2] - P[a][b + 2])) * 0.03125;
                    }
                    Iw[k] = gmc_bilerp(vi[0], vi[1], vi[2], vi[3], fx, fy);
                    Dx[k] = gmc_bilerp(vx[0], vx[1], vx[2], vx[3], fx, fy);
                    Dy[k] = gmc_bilerp(vy[0], vy[1], vy[2], vy[3], fx, fy);
                }
            }
        }
        double a11 = 0.0, a12 = 0.0, a22 = 0.0;
#pragma unroll
        for (int k = 0; k < GMC_EL; ++k) { a11 = a11 + Dx[k] * Dx[k]; a12 = a12 + Dx[k] * Dy[k]; a22 = a22 + Dy[k] * Dy[k]; }
        const double A11 = gmc_wave_sum(a11), A12 = gmc_wave_sum(a12), A22 = gmc_wave_sum(a22);
        const double dA = A11 - A22;
        const double min_eig = ((A22 + A11) - sqrt(dA * dA + 4.0 * A12 * A12)) / 882.0;
        const double D = A11 * A22 - A12 * A12;
        const bool ok = min_eig >= 1e-4 && D >= 1.1920928955078125e-07;
        if (!ok) {
            if (L == 0) status = 0;                                   // S-07: at a coarser level the guess passes through
        } else {
            for (int it = 0; it < 30; ++it) {
                if (!(nx >= 0.0 && nx <= xmax && ny >= 0.0 && ny <= ymax)) { status = 0; break; }     // S-08
                const double bx = nx - 10.0, by = ny - 10.0;
                const double fbx = floor(bx), fby = floor(by);
                const double fx = bx - fbx, fy = by - fby;
                const int ix = (int)fbx, iy = (int)fby;
                double b1 = 0.0, b2 = 0.0;
#pragma unroll
                for (int k = 0; k < GMC_EL; ++k) {
                    double diff = 0.0;
                    if (lane + 64 * k < GMC_WIN_N) {
                        const uint8_t* r0 = J + (size_t)gmc_clamp(iy + ei[k], h) * w;
                        const uint8_t* r1 = J + (size_t)gmc_clamp(iy + ei[k] + 1, h) * w;
                        const int x0 = gmc_clamp(ix + ej[k], w), x1 = gmc_clamp(ix + ej[k] + 1, w);
                        diff = gmc_bilerp((double)r0[x0], (double)r0[x1], (double)r1[x0], (double)r1[x1], fx, fy) - Iw[k];
                    }
                    b1 = b1 + diff * Dx[k]; b2 = b2 + diff * Dy[k];
                }
                const double B1 = gmc_wave_sum(b1), B2 = gmc_wave_sum(b2);
                const double ddx = (A12 * B2 - A22 * B1) / D, ddy = (A12 * B1 - A11 * B2) / D;
                nx = nx + ddx; ny = ny + ddy;
                if (ddx * ddx + ddy * ddy < 1e-4) break;
            }
        }
        if (status && !(nx >= 0.0 && nx <= xmax && ny >= 0.0 && ny <= ymax)) status = 0;
    }
    if (lane == 0) { g.pts[o * 2] = status ? nx : 0.0; g.pts[o * 2 + 1] = status ? ny : 0.0; g.status[o] = (uint8_t)status; }
}

__device__ inline unsigned gmc_mix32(unsigned u)
{
    u = u * 0x9E3779B9u + 0x7F4A7C15u;
    u ^= u >> 16; u *= 0x85EBCA6Bu; u ^= u >> 13; u *= 0xC2B2AE35u; u ^= u >> 16;
    return u;
}

// block-wide sums in the reference's order: 64-lane xor butterflies, then the 16 wave sums added left to right
template <int NS>
__device__ inline void gmc_block_sum(double (&a)[NS], double (*red)[4], double (&out)[NS])
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NS; ++k) a[k] = gmc_wave_sum(a[k]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) red[wv][k] = a[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        double tot = red[0][k];
        for (int q = 1; q < 16; ++q) tot = tot + red[q][k];
        out[k] = tot;
    }
}

// S-09..S-11: one workgroup of 1024 per pair.  Matches compacted into LDS in corner order; thread k scores hypothesis k against all
// of them; the best one's inliers are refitted in closed form.  warps[pair*8 ..]: ss_cmc_estimate's layout.
__global__ __launch_bounds__(1024) void k_gmc_fit(SSGmcDev g, const int* __restrict__ n_valid, double* __restrict__ warps)
{
    __shared__ double mx[SS_GMC_MAXC], my[SS_GMC_MAXC], mu[SS_GMC_MAXC], mv[SS_GMC_MAXC];
    __shared__ uint8_t inl_flag[SS_GMC_MAXC];
    __shared__ int wcnt[16];
    __shared__ unsigned best;
    __shared__ double hyp[4], red[16][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, pair = blockIdx.x;
    const int f = pair / g.S, s = pair - f * g.S;
    double* out = warps + (size_t)pair * 8;
    const size_t o = (size_t)pair * SS_GMC_MAXC;
    int M = 0;
    bool have = false;
    int st = 0, pos = 0;
    if (gmc_pair_valid(g, f, s, n_valid)) {
        const int n = g.ncorner[f * g.S + s];
        st = tid < n ? g.status[o + tid] : 0;
        const unsigned long long m = __ballot(st != 0);
        if (lane == 0) wcnt[wv] = __popcll(m);
        if (tid == 0) best = 0u;
        __syncthreads();
        for (int q = 0; q < 16; ++q) { if (q < wv) pos += wcnt[q]; M += wcnt[q]; }
        pos += __popcll(m & ((1ull << lane) - 1ull));
        if (st) {
            const int c = g.corners[(size_t)(f * g.S + s) * SS_GMC_MAXC + tid];
            const int cy = c / g.lw[0];
            mx[pos] = (double)(c - cy * g.lw[0]); my[pos] = (double)cy;
            mu[pos] = g.pts[(o + tid) * 2]; mv[pos] = g.pts[(o + tid) * 2 + 1];
        }
        __syncthreads();
        if (M >= 5) {
            // hypothesis tid: two distinct matches from the counter-based generator, the similarity through them
            const int i1 = (int)(((unsigned long long)gmc_mix32(2u * tid) * (unsigned)M) >> 32);
            int i2 = (int)(((unsigned long long)gmc_mix32(2u * tid + 1u) * (unsigned)(M - 1)) >> 32);
            if (i2 >= i1) ++i2;
            const double dx = mx[i2] - mx[i1], dy = my[i2] - my[i1], ex = mu[i2] - mu[i1], ey = mv[i2] - mv[i1];
            double den = dx * dx + dy * dy;
            const bool good = den > 0.0;
            if (!good) den = 1.0;
            const double a = (dx * ex + dy * ey) / den, b = (dx * ey - dy * ex) / den;
            const double tx = mu[i1] - (a * mx[i1] - b * my[i1]), ty = mv[i1] - (b * mx[i1] + a * my[i1]);
            int cnt = 0;
            for (int q = 0; q < M; ++q) {
                const double rx = ((a * mx[q] - b * my[q]) + tx) - mu[q], ry = ((b * mx[q] + a * my[q]) + ty) - mv[q];
                cnt += (rx * rx + ry * ry <= 9.0) ? 1 : 0;
            }
            if (!good) cnt = 0;
            const unsigned key = ((unsigned)cnt << 10) | (unsigned)(GMC_NHYP - 1 - tid);       // most inliers, lowest index on a tie
            atomicMax(&best, key);
            __syncthreads();
            const unsigned bk = best;
            if (tid == GMC_NHYP - 1 - (int)(bk & 1023u)) { hyp[0] = a; hyp[1] = b; hyp[2] = tx; hyp[3] = ty; }
            __syncthreads();
            const int n_in = (int)(bk >> 10);
            bool inl = false;
            double x = 0.0, y = 0.0, u = 0.0, v = 0.0;
            if (tid < M) {
                x = mx[tid]; y = my[tid]; u = mu[tid]; v = mv[tid];
                const double rx = ((hyp[0] * x - hyp[1] * y) + hyp[2]) - u, ry = ((hyp[1] * x + hyp[0] * y) + hyp[3]) - v;
                inl = rx * rx + ry * ry <= 9.0;
            }
            if (n_in >= 2) {
                double s4[4] = { inl ? x : 0.0, inl ? y : 0.0, inl ? u : 0.0, inl ? v : 0.0 }, t4[4];
                gmc_block_sum<4>(s4, red, t4);
                const double nn = (double)n_in;
                const double cxm = t4[0] / nn, cym = t4[1] / nn, cum = t4[2] / nn, cvm = t4[3] / nn;
                const double xc = x - cxm, yc = y - cym, uc = u - cum, vc = v - cvm;
                double s3[3] = { inl ? xc * xc + yc * yc : 0.0, inl ? xc * uc + yc * vc : 0.0, inl ? xc * vc - yc * uc : 0.0 }, t3[3];
                gmc_block_sum<3>(s3, red, t3);
                if (t3[0] > 0.0) {
                    have = true;
                    if (tid < M) inl_flag[tid] = inl ? 1 : 0;
                    if (tid == 0) {
                        const double ra = t3[1] / t3[0], rb = t3[2] / t3[0];
                        const double rtx = cum - (ra * cxm - rb * cym), rty = cvm - (rb * cxm + ra * cym);
                        out[0] = ra; out[1] = -rb; out[2] = 2.0 * rtx; out[3] = rb; out[4] = ra; out[5] = 2.0 * rty;
                        out[6] = nn; out[7] = (double)M;
                    }
                }
            }
        }
    }
    __syncthreads();
    if (tid < SS_GMC_MAXC) g.inlier[o + tid] = (have && st) ? inl_flag[pos] : 0;
    if (!have && tid == 0) {
        out[0] = 1.0; out[1] = 0.0; out[2] = 0.0; out[3] = 0.0; out[4] = 1.0; out[5] = 0.0; out[6] = -1.0; out[7] = (double)M;
    }
}

// start of a call: the previous call's last real frame (pyramid, corner list, counts) becomes slot 0 of its stream (a kernel, not a
// memcpy node: graph-capture safe).  grid = (blocks, S)
__global__ __launch_bounds__(256) void k_gmc_roll(SSGmcDev g)
{
    const int n = *g.last, s = blockIdx.y;
    if (n <= 0) return;
    const size_t src = (size_t)n * g.S + s, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i * 16 < (size_t)g.pyr_stride)
        reinterpret_cast<uint4*>(g.pyr + (size_t)s * g.pyr_stride)[i] = reinterpret_cast<const uint4*>(g.pyr + src * g.pyr_stride)[i];
    if (i < SS_GMC_MAXC) g.corners[(size_t)s * SS_GMC_MAXC + i] = g.corners[src * SS_GMC_MAXC + i];
    if (i == 0) { g.ncorner[s] = g.ncorner[src]; g.ncand[s] = g.ncand[src]; }
}

// end of a call: which slot the next call rolls (n_valid: device count of real frames, NULL = n_frames; a group without real
// frames leaves the remembered one alone), and the streams now have a predecessor
__global__ void k_gmc_mark(SSGmcDev g, int n_frames, const int* __restrict__ n_valid)
{
    int n = n_valid ? *n_valid : n_frames;
    if (n > n_frames) n = n_frames;
    if (n < 0) n = 0;
    if (threadIdx.x == 0) *g.last = n;
    if (n > 0) for (int s = threadIdx.x; s < g.S; s += blockDim.x) g.prev_valid[s] = 1;
}

void ss_launch_gmc_sparse(const SSGmcDev& g, const uint8_t* frames, int n_frames, long long frame_stride, int row_stride,
                          const int* n_valid, double* warps, hipStream_t st)
{
    const int n_img = n_frames * g.S, npix = g.lw[0] * g.lh[0];
    const unsigned roll_blocks = (unsigned)(((size_t)g.pyr_stride / 16 + 255) / 256);
    hipLaunchKernelGGL(k_gmc_roll, dim3(roll_blocks < 4 ? 4 : roll_blocks, g.S), dim3(256), 0, st, g);
    hipLaunchKernelGGL(k_gmc_half, dim3((npix + 255) / 256, n_img), dim3(256), 0, st, g, frames, frame_stride, row_stride);
    for (int L = 0; L < SS_GMC_LEVELS - 1; ++L)
        hipLaunchKernelGGL(k_gmc_pyrdown, dim3((g.lw[L + 1] * g.lh[L + 1] + 255) / 256, n_img), dim3(256), 0, st, g, L);
    hipLaunchKernelGGL(k_gmc_eig, dim3((npix + 255) / 256, n_img), dim3(256), 0, st, g);
    hipLaunchKernelGGL(k_gmc_cand, dim3((npix + 255) / 256, n_img), dim3(256), 0, st, g);
    hipLaunchKernelGGL(k_gmc_select, dim3(n_img), dim3(1024), 0, st, g);
    hipLaunchKernelGGL(k_gmc_lk, dim3(SS_GMC_MAXC / 4, n_img), dim3(256), 0, st, g, n_valid);
    hipLaunchKernelGGL(k_gmc_fit, dim3(n_img), dim3(1024), 0, st, g, n_valid, warps);
    hipLaunchKernelGGL(k_gmc_mark, dim3(1), dim3(64), 0, st, g, n_frames, n_valid);
}
