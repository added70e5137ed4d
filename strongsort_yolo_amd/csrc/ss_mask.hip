// ss_mask.hip — instance masks of a segmentation head and their outlines on the device (opt-in, YOLO(device_masks=True)).
//
// k_mask_assemble: the published recipe `process_mask(..., upsample=True)` that strongsort_yolo_amd/yolo.py assemble_masks runs on
// the host — linear combination of the prototypes, crop to the box on the prototype grid, bilinear (align_corners=False) up to the
// network input, > 0 — in a fixed float32 order (no contraction, -ffp-contract=off) that a NumPy restatement reproduces bit for bit
// (tests/test_masks_device_cpu.py).  Output: bit-packed planes, bit x % 32 of word x / 32 of row y = pixel (y, x).
//
// k_mask_outline: what yolo.mask_polygon returns for one packed mask — 8-connected components (union-find over a global label
// plane, min-index roots = each component's first raster pixel), the 16 largest (ties: first pixel in raster order), each traced by
// yolo.trace_outline's Moore walk over the bits held in LDS, the first outline of maximal length kept.  Points are int32 (x, y).
#include <hip/hip_fp16.h>
#include "ss_common.h"
#include "ss_launch.h"

#define MK_BAND 32            // output rows per assembly workgroup
#define MK_BAND_PROTO 12      // prototype rows a band reads at most (MK_BAND / 4 + 2, rounded up)
#define MK_MAX_MW 256         // prototype width at most (network input width <= 1024)
#define MK_MAX_NM 64          // mask coefficients at most
#define MK_MAX_WORDS 12800    // packed words of one plane the outline kernel holds in LDS (50 KiB: 640 x 640 fits)
#define MK_ROOTS 1024         // components ranked from an LDS list; a mask with more is ranked by scanning its label plane
#define MK_TOP 16             // components traced per mask (yolo.mask_polygon)
#define MK_OUTLINE_THREADS 512

// ---- assembly ----------------------------------------------------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(256) void k_mask_assemble(const T* __restrict__ proto, long long proto_fs, int nm, int mh, int mw,
                                                       const float* __restrict__ dets, long long dets_fs, int ld, int coef_off,
                                                       const int* __restrict__ counts, int R, const float* __restrict__ geom,
                                                       long long geom_fs, int ih, int iw, uint32_t* __restrict__ bits, long long bits_fs)
{
    __shared__ float coef[MK_MAX_NM];
    __shared__ float cell[MK_BAND_PROTO][MK_MAX_MW];
    const int r = blockIdx.y, s = blockIdx.z, tid = threadIdx.x;
    if (r >= min(counts[s], R)) return;
    const float* row = dets + s * dets_fs + (long long)r * ld;
    const float* g = geom + s * geom_fs;
    const T* P = proto + s * proto_fs;
    for (int k = tid; k < nm; k += blockDim.x) coef[k] = row[coef_off + k];
    // the box in input pixels (x * gain + pad, as YOLO._results), then on the prototype grid (* mw / iw, as assemble_masks)
    const float gain = g[0], padx = g[1], pady = g[2];
    const float fx = (float)((double)mw / (double)iw), fy = (float)((double)mh / (double)ih);
    const float x1 = (row[0] * gain + padx) * fx, y1 = (row[1] * gain + pady) * fy;
    const float x2 = (row[2] * gain + padx) * fx, y2 = (row[3] * gain + pady) * fy;
    const float sy = (float)mh / (float)ih, sx = (float)mw / (float)iw;
    const int wpr = (iw + 31) >> 5;
    const int yb0 = blockIdx.x * MK_BAND, yb1 = min(yb0 + MK_BAND, ih);
    // prototype rows of the band: i0 of its first row .. i1 of its last
    const int lo = (int)fmaxf(0.0f, ((float)yb0 + 0.5f) * sy - 0.5f);
    const int hi = min((int)fmaxf(0.0f, ((float)(yb1 - 1) + 0.5f) * sy - 0.5f) + 1, mh - 1);
    __syncthreads();
    const int ncell = (hi - lo + 1) * mw;
    for (int i = tid; i < ncell; i += blockDim.x) {
        const int py = lo + i / mw, px = i % mw;
        const float fpx = (float)px, fpy = (float)py;
        float acc = 0.0f;
        if (fpx >= x1 && fpx < x2 && fpy >= y1 && fpy < y2) {
            const T* q = P + (long long)py * mw + px;
            for (int k = 0; k < nm; ++k) acc = acc + coef[k] * (float)q[(long long)k * mh * mw];
        }
        cell[py - lo][px] = acc;
    }
    __syncthreads();
    uint32_t* out = bits + s * bits_fs + (long long)r * ih * wpr;
    const int nword = (yb1 - yb0) * wpr;
    for (int i = tid; i < nword; i += blockDim.x) {
        const int y = yb0 + i / wpr, w = i % wpr;
        const float srcy = fmaxf(0.0f, ((float)y + 0.5f) * sy - 0.5f);
        const int iy0 = (int)srcy, iy1 = min(iy0 + 1, mh - 1);
        const float ly1 = srcy - (float)iy0, ly0 = 1.0f - ly1;
        const float* c0 = cell[iy0 - lo];
        const float* c1 = cell[iy1 - lo];
        uint32_t word = 0;
        for (int b = 0; b < 32; ++b) {
            const int x = w * 32 + b;
            if (x >= iw) break;
            const float srcx = fmaxf(0.0f, ((float)x + 0.5f) * sx - 0.5f);
            const int ix0 = (int)srcx, ix1 = min(ix0 + 1, mw - 1);
            const float lx1 = srcx - (float)ix0, lx0 = 1.0f - lx1;
            const float v = (c0[ix0] * lx0 + c0[ix1] * lx1) * ly0 + (c1[ix0] * lx0 + c1[ix1] * lx1) * ly1;
            word |= (uint32_t)(v > 0.0f) << b;
        }
        out[(long long)y * wpr + w] = word;
    }
}

// ---- outline ----------------------------------------------------------------------------------------------------------------
// The label plane lives in global scratch and is read and written by many waves of one workgroup around atomics: every access
// bypasses the CU's L1 (agent-scope relaxed atomics), so no wave reads a stale copy of a label another wave changed.

__device__ __forceinline__ int mk_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mk_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int mk_find(int* L, int x)     // with path halving: a non-root may point to any ancestor (only roots are linked)
{
    while (true) {
        const int y = mk_ld(L + x);
        if (y == x) return x;
        const int z = mk_ld(L + y);
        if (z == y) return y;
        mk_st(L + x, z);
        x = z;
    }
}

__device__ void mk_merge(int* L, int a, int b)          // link the larger root under the smaller (roots stay component minima)
{
    while (true) {
        a = mk_find(L, a);
        b = mk_find(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(L + b, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == b) return;
        b = old;                                          // b was linked meanwhile: join a with what it was linked to
    }
}

__device__ __forceinline__ bool mk_bit(const uint32_t* sb, int wpr, int h, int w, int x, int y)
{
    return x >= 0 && x < w && y >= 0 && y < h && ((sb[y * wpr + (x >> 5)] >> (x & 31)) & 1u);
}

// yolo.trace_outline from (sx, sy), the component's first raster pixel.  Every set 8-neighbour of a component pixel belongs to the
// component, so the walk tests bits only.  The CHAIN_APPROX_SIMPLE reduction (keep point i when its incoming and outgoing steps
// differ, cyclically) is applied while walking: point i is decided when point i + 1 is appended; the last point and the first
// are decided at the end.  Counting pass: out == nullptr, returns the polygon's length and *keep0.  Writing pass: keep0 from the
// counting pass, writes the points (the caller has checked the length against cap).
__device__ int mk_trace(const uint32_t* sb, int wpr, int h, int w, int sx, int sy, int* keep0, int* out, int cap)
{
    const int RX[8] = {-1, -1, 0, 1, 1, 1, 0, -1}, RY[8] = {0, -1, -1, -1, 0, 1, 1, 1};     // yolo._RING, clockwise from west
    const int BK[8] = {6, 6, 0, 0, 2, 2, 4, 4};            // ring index of ring[j - 1] - ring[j]: the background seen before step j
    int x = sx, y = sy, back = 0, fx = 0, fy = 0, n = 1, pdx = 0, pdy = 0, d0x = 0, d0y = 0, kept = 0;
    bool have_first = false, popped = false;
    int wpos = 0;
    if (out && *keep0) { out[0] = sx; out[1] = sy; wpos = 1; }
    const long long steps = 4LL * ((long long)h * w + 4);
    for (long long it = 0; it < steps; ++it) {
        int j = -1;
        for (int k = 1; k <= 8; ++k) {
            const int jj = (back + k) & 7;
            if (mk_bit(sb, wpr, h, w, x + RX[jj], y + RY[jj])) { j = jj; break; }
        }
        if (j < 0) break;                                  // an isolated pixel
        const int qx = x + RX[j], qy = y + RY[j];
        if (x == sx && y == sy && have_first && qx == fx && qy == fy) { popped = true; break; }   // back at the start, leaving as the first time
        if (!have_first) { have_first = true; fx = qx; fy = qy; }
        const int dx = qx - x, dy = qy - y;
        if (n == 1) { d0x = dx; d0y = dy; }
        else if (dx != pdx || dy != pdy) {                 // point n - 1 = (x, y) is a corner
            if (out && wpos < cap) { out[2 * wpos] = x; out[2 * wpos + 1] = y; }
            ++wpos; ++kept;
        }
        pdx = dx; pdy = dy; x = qx; y = qy; back = BK[j]; ++n;
    }
    int N = n, wdx, wdy;                                   // raw points; the closing step (last point -> first)
    if (popped) { N = n - 1; wdx = pdx; wdy = pdy; }       // the start appended last is dropped: the step into it closes the polygon
    else {
        wdx = sx - x; wdy = sy - y;
        if (N >= 2 && (wdx != pdx || wdy != pdy)) {        // the last point
            if (out && wpos < cap) { out[2 * wpos] = x; out[2 * wpos + 1] = y; }
            ++wpos; ++kept;
        }
    }
    if (N < 3) {                                           // no reduction: the raw points
        if (out) { out[0] = sx; out[1] = sy; if (N == 2) { out[2] = fx; out[3] = fy; } }
        return N;
    }
    if (!out) *keep0 = (wdx != d0x || wdy != d0y);
    return *keep0 + kept;
}

// persistent workgroups; work item t = the t-th kept row over the frames (rows below each frame's count, frame-major)
__global__ __launch_bounds__(MK_OUTLINE_THREADS) void k_mask_outline(const uint32_t* __restrict__ bits, long long bits_fs, const int* __restrict__ counts,
                                                                     int S, int R, int ih, int iw, int cap, int* __restrict__ pts, long long pts_fs,
                                                                     int* __restrict__ npts, long long npts_fs, uint32_t* __restrict__ copy,
                                                                     long long copy_fs, int* __restrict__ scratch)
{
    __shared__ uint32_t sb[MK_MAX_WORDS];
    __shared__ int s_nroots, s_sel[MK_TOP], s_len[MK_TOP], s_keep0[MK_TOP], s_f, s_r;
    __shared__ int s_root[MK_ROOTS], s_size[MK_ROOTS];
    __shared__ unsigned long long s_best;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int wpr = (iw + 31) >> 5, nwords = ih * wpr;
    const uint32_t tail = (iw & 31) ? ((1u << (iw & 31)) - 1u) : 0xffffffffu;
    int* L = scratch + (long long)blockIdx.x * ih * iw;
    for (int t = blockIdx.x;; t += gridDim.x) {
        if (tid == 0) {
            int f = 0, rem = t;
            for (; f < S; ++f) { const int c = min(max(counts[f], 0), R); if (rem < c) break; rem -= c; }
            s_f = f; s_r = rem; s_nroots = 0;
        }
        __syncthreads();
        const int f = s_f, r = s_r;
        if (f >= S) break;
        const uint32_t* src = bits + f * bits_fs + (long long)r * nwords;
        uint32_t* cp = copy ? copy + f * copy_fs + (long long)r * nwords : nullptr;
        for (int i = tid; i < nwords; i += nt) {
            uint32_t v = src[i];
            if (i % wpr == wpr - 1) v &= tail;             // pixels right of the image are background
            sb[i] = v;
            if (cp) cp[i] = v;
        }
        __syncthreads();
#define MK_FOR_SET(BODY)                                                                      \
        for (int i = tid; i < nwords; i += nt) {                                              \
            uint32_t m = sb[i];                                                               \
            const int y = i / wpr, xb = (i - y * wpr) * 32;                                   \
            while (m) {                                                                       \
                const int x = xb + __builtin_ctz(m);                                          \
                m &= m - 1u;                                                                  \
                const int p = y * iw + x;                                                     \
                BODY                                                                          \
            }                                                                                 \
        }
        MK_FOR_SET(mk_st(L + p, p);)
        __syncthreads();
        MK_FOR_SET(
            if (mk_bit(sb, wpr, ih, iw, x - 1, y)) mk_merge(L, p, p - 1);
            if (mk_bit(sb, wpr, ih, iw, x - 1, y - 1)) mk_merge(L, p, p - iw - 1);
            if (mk_bit(sb, wpr, ih, iw, x, y - 1)) mk_merge(L, p, p - iw);
            if (mk_bit(sb, wpr, ih, iw, x + 1, y - 1)) mk_merge(L, p, p - iw + 1);)
        __syncthreads();
        MK_FOR_SET(const int q = mk_find(L, p); if (q != p) mk_st(L + p, q);)
        __syncthreads();
        MK_FOR_SET(if (mk_ld(L + p) == p) {                                                    // roots: -size from here on
                       mk_st(L + p, -1);
                       const int j = atomicAdd(&s_nroots, 1);
                       if (j < MK_ROOTS) s_root[j] = p; })
        __syncthreads();
        MK_FOR_SET(const int q = mk_ld(L + p); if (q >= 0) __hip_atomic_fetch_add(L + q, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);)
        __syncthreads();
        const int nroots = s_nroots;
        const bool listed = nroots <= MK_ROOTS;             // every root is in s_root: rank from LDS, not from the plane
        if (listed)
            for (int j = tid; j < nroots; j += nt) s_size[j] = -mk_ld(L + s_root[j]);
        __syncthreads();
        // the MK_TOP largest components, ties to the first pixel in raster order: key = size << 32 | ~root, descending
        const int nsel = min(nroots, MK_TOP);
        unsigned long long prev = ~0ull;
        for (int k = 0; k < nsel; ++k) {
            if (tid == 0) s_best = 0;
            __syncthreads();
            unsigned long long best = 0;
            if (listed)
                for (int j = tid; j < nroots; j += nt) {
                    const unsigned long long key = ((unsigned long long)(unsigned)s_size[j] << 32) | (unsigned long long)(0xffffffffu - (unsigned)s_root[j]);
                    if (key < prev && key > best) best = key;
                }
            else
                MK_FOR_SET(const int q = mk_ld(L + p);
                           if (q < 0) {
                               const unsigned long long key = ((unsigned long long)(unsigned)(-q) << 32) | (unsigned long long)(0xffffffffu - (unsigned)p);
                               if (key < prev && key > best) best = key;
                           })
            if (best) atomicMax(&s_best, best);
            __syncthreads();
            prev = s_best;
            if (tid == 0) s_sel[k] = (int)(0xffffffffu - (unsigned)(prev & 0xffffffffull));
            __syncthreads();
        }
#undef MK_FOR_SET
        if (tid < nsel) {
            const int root = s_sel[tid];
            int k0 = 0;
            s_len[tid] = mk_trace(sb, wpr, ih, iw, root % iw, root / iw, &k0, nullptr, 0);
            s_keep0[tid] = k0;
        }
        __syncthreads();
        if (tid == 0) {
            int* np = npts + f * npts_fs + r;
            if (nsel == 0) *np = 0;
            else {
                int b = 0;
                for (int k = 1; k < nsel; ++k) if (s_len[k] > s_len[b]) b = k;      // the first of maximal length
                const int len = s_len[b];
                if (len <= cap) {
                    int k0 = s_keep0[b];
                    mk_trace(sb, wpr, ih, iw, s_sel[b] % iw, s_sel[b] / iw, &k0, pts + f * pts_fs + (long long)r * cap * 2, cap);
                    *np = len;
                } else *np = -len;                         // longer than cap: no points, the caller traces this mask on the host
            }
        }
        __syncthreads();                                   // sb, s_* are reused by the next work item
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------

int ss_mask_max_words() { return MK_MAX_WORDS; }

void ss_launch_mask_assemble(const void* proto, int f16, long long proto_fs, int nm, int mh, int mw, const float* dets, long long dets_fs,
                             int ld, int coef_off, const int* counts, int S, int R, const float* geom, long long geom_fs, int ih, int iw,
                             uint32_t* bits, long long bits_fs, hipStream_t st)
{
    const dim3 grid((ih + MK_BAND - 1) / MK_BAND, R, S);
    if (f16)
        hipLaunchKernelGGL(k_mask_assemble<__half>, grid, dim3(256), 0, st, (const __half*)proto, proto_fs, nm, mh, mw, dets, dets_fs, ld,
                           coef_off, counts, R, geom, geom_fs, ih, iw, bits, bits_fs);
    else
        hipLaunchKernelGGL(k_mask_assemble<float>, grid, dim3(256), 0, st, (const float*)proto, proto_fs, nm, mh, mw, dets, dets_fs, ld,
                           coef_off, counts, R, geom, geom_fs, ih, iw, bits, bits_fs);
}

void ss_launch_mask_outline(const uint32_t* bits, long long bits_fs, const int* counts, int S, int R, int ih, int iw, int cap, int* pts,
                            long long pts_fs, int* npts, long long npts_fs, uint32_t* copy, long long copy_fs, int* scratch, int slots,
                            hipStream_t st)
{
    const long long items = (long long)S * R;
    const int grid = (int)(items < slots ? items : slots);
    hipLaunchKernelGGL(k_mask_outline, dim3(grid), dim3(MK_OUTLINE_THREADS), 0, st, bits, bits_fs, counts, S, R, ih, iw, cap, pts, pts_fs,
                       npts, npts_fs, copy, copy_fs, scratch);
}
