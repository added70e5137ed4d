// ss_slice.hip — sliced inference (docs/SLICE.md): the frame cut into overlapping tiles in front of the detector, the tiles' NMS rows
// merged back into one row list per frame behind it.
//   k_slice_letterbox  every tile of every resident frame into the detector's input, ONE launch; k_letterbox's arithmetic on a source
//                      window offset by the tile's origin, so a tile's output is ss_letterbox_batch's on a cropped copy, bit for bit
//   k_slice_merge      T per-tile row lists -> one per-frame row list (greedy NMS or SAHI's GREEDYNMM), one workgroup per frame
// The bits are those of tests/slice_ref.py.
#include <hip/hip_fp16.h>
#include <cmath>
#include <cstring>
#include "ss_common.h"
#include "ss_host.h"
#include "ss_launch.h"
#include "ss_bilerp.h"

#define SL_TILES 64            // tiles of a frame, the full-frame tile included
#define SL_CAND 8192           // candidates of a frame: T * rows_per_tile
#define SL_LINES 4             // output lines per workgroup of the letterbox

struct SlTile { int x0, y0, tw, th, new_w, new_h, pad_left, pad_top; };     // a row of ss_slice_config's table

// =================================================================================================
// tiled letterbox.  grid = (chunks of a line, groups of SL_LINES lines, batch * T), image = frame * T + tile.
// A line is what is contiguous in the output: a row of out_w * 3 values (channels-last) or a row of out_w values of one plane.
// A thread owns one 16-byte chunk of the line (8 halves / 4 floats, i.e. a run of pixels), aligned on the ADDRESS, and writes it
// with one 16-byte store; the chunks that hang over the line's ends are written value by value (as k_zone_heat_blend's head
// and tail bytes).  The rounded bilinear value is an integer 0..255, so value / 255 comes from a 256-entry table filled with exactly
// that expression (k_crop_hwc8 does the same): one correctly rounded division per thread instead of one per value.
// Identity tiles (new size == tile size, 640 on 640): scale 1 gives frac == 0 and both taps on the pixel itself on both axes, the
// bilinear value IS the source byte; that path reads one byte per value instead of four and skips the arithmetic.
// =================================================================================================
template <typename T, int HWC>
__global__ __launch_bounds__(256) void k_slice_letterbox(const uint8_t* __restrict__ src, long long src_batch_stride, int stride,
                                                         const SlTile* __restrict__ tiles, int n_tiles, T* __restrict__ dst, int out_h,
                                                         int out_w, float padv)
{
    __shared__ T lut[256];
    constexpr int EPC = 16 / (int)sizeof(T);
    const int tid = threadIdx.x;
    lut[tid] = ss_cvt<T>((float)tid / 255.0f);
    __syncthreads();
    const int img = blockIdx.z, b = img / n_tiles;
    const SlTile tl = tiles[img - b * n_tiles];
    src += (size_t)b * src_batch_stride + (size_t)tl.y0 * stride + (size_t)tl.x0 * 3;
    T* img_dst = dst + (size_t)img * 3 * out_h * out_w;
    const int n_lines = HWC ? out_h : 3 * out_h, n_el = HWC ? 3 * out_w : out_w;
    const bool ident = tl.new_w == tl.tw && tl.new_h == tl.th;
    const float sx = (float)tl.tw / (float)tl.new_w, sy = (float)tl.th / (float)tl.new_h;
    const T pv = ss_cvt<T>(padv);
    const int ln_end = min(n_lines, ((int)blockIdx.y + 1) * SL_LINES);
    for (int ln = blockIdx.y * SL_LINES; ln < ln_end; ++ln) {
        const int cpl = HWC ? 0 : ln / out_h, y = HWC ? ln : ln - cpl * out_h;       // planes: line = plane * out_h + row
        T* line = img_dst + (size_t)ln * n_el;
        const int mis = (int)(((uintptr_t)line & 15) / sizeof(T));                   // values of the first chunk that lie before the line
        const int nch = (mis + n_el + EPC - 1) / EPC;
        const int ry = y - tl.pad_top;
        const bool row_in = ry >= 0 && ry < tl.new_h;
        int y0 = 0, y1 = 0; float fy = 0.0f;
        if (row_in) { if (ident) y0 = y1 = ry; else ss_axis(ry, sy, tl.th, y0, y1, fy); }
        const uint8_t* r0 = src + (size_t)y0 * stride;
        const uint8_t* r1 = src + (size_t)y1 * stride;
        for (int k = blockIdx.x * 256 + tid; k < nch; k += gridDim.x * 256) {
            const int e0 = k * EPC - mis;
            __attribute__((aligned(16))) T v[EPC];
#pragma unroll
            for (int j = 0; j < EPC; ++j) {
                const int e = e0 + j;
                T o = pv;
                if (row_in && e >= 0 && e < n_el) {
                    const int x = HWC ? e / 3 : e, c = HWC ? e - 3 * x : cpl;
                    const int rx = x - tl.pad_left, sc = 2 - c;
                    if (rx >= 0 && rx < tl.new_w) {
                        if (ident) o = lut[r0[rx * 3 + sc]];
                        else {
                            int x0, x1; float fx;
                            ss_axis(rx, sx, tl.tw, x0, x1, fx);
                            const float p00 = r0[x0 * 3 + sc], p01 = r0[x1 * 3 + sc], p10 = r1[x0 * 3 + sc], p11 = r1[x1 * 3 + sc];
                            o = lut[(int)ss_bilerp_u8(p00, p01, p10, p11, fx, fy)];
                        }
                    }
                }
                v[j] = o;
            }
            if (e0 >= 0 && e0 + EPC <= n_el) *reinterpret_cast<uint4*>(line + e0) = *reinterpret_cast<const uint4*>(v);
            else {
#pragma unroll
                for (int j = 0; j < EPC; ++j) if (e0 + j >= 0 && e0 + j < n_el) line[e0 + j] = v[j];
            }
        }
    }
}

// =================================================================================================
// merge.  One workgroup of 1024 threads per frame:
//   A  candidates = rows r < min(max(count_t, 0), R) of every tile, key (~score bits, tile * R + row); sorted in LDS (bitonic)
//   B  match bit matrix (metric >= thr, same class unless agnostic) of the sorted candidates, one wave per 64 x 64 block pair
//   C  greedy scan on wave 0: kept list, and for every removed candidate its owner = the first kept candidate that matches it
//   D  (nmm) one thread per kept box walks its candidates in order: metric(box so far, candidate) > thr -> box becomes the union
//   E  all threads write the rows; keypoint x, y re-expressed in the whole frame's letterbox
// n <= 64: one wave does A..D in registers and LDS (k_nms_rest's small form), no workspace.
// =================================================================================================
struct SlMerge {
    const float* rows; const int* counts; const SlTile* tiles; const float* geom;
    int T, R, ld; long long tile_stride, frame_stride;
    int n_extra, n_kpt; float kg, kpx, kpy;
    int nmm, ios, agnostic; float thr; int out_cap;
    float* out; int out_ld; long long out_frame_stride; int* out_count; int* out_src; long long src_frame_stride;
    char* ws; long long ws_stride; int cap, words, np2;
};

struct SlWs { unsigned long long* mask; float* box; float* area; float* cls; int* owner; int* kept; };

__host__ __device__ inline size_t sl_ws_bytes(int cap, int words)
{
    return ((size_t)cap * words * 8 + (size_t)cap * (16 + 4 + 4 + 4 + 4) + 15) & ~(size_t)15;
}

__device__ inline SlWs sl_carve(char* p, int cap, int words)
{
    SlWs w;
    w.mask = (unsigned long long*)p; p += (size_t)cap * words * 8;
    w.box = (float*)p; p += (size_t)cap * 16;
    w.area = (float*)p; p += (size_t)cap * 4;
    w.cls = (float*)p; p += (size_t)cap * 4;
    w.owner = (int*)p; p += (size_t)cap * 4;
    w.kept = (int*)p;
    return w;
}

// inter as k_nms_mask computes it; a NaN metric compares false either way
__device__ inline bool sl_match(float x1, float y1, float x2, float y2, float ai, float bx1, float by1, float bx2, float by2, float aj, int ios,
                                float thr, bool strict)
{
    float xx1 = fmaxf(x1, bx1), yy1 = fmaxf(y1, by1);
    float xx2 = fminf(x2, bx2), yy2 = fminf(y2, by2);
    float iw = fmaxf(0.0f, xx2 - xx1), ih = fmaxf(0.0f, yy2 - yy1);
    float inter = iw * ih;
    float m = ios ? inter / fminf(ai, aj) : inter / (ai + aj - inter);
    return strict ? m > thr : m >= thr;
}

__global__ __launch_bounds__(1024) void k_slice_merge(SlMerge a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long* k = (unsigned long long*)smem;                         // [np2] sort keys
    float* sbw = (float*)(smem + (size_t)a.np2 * 8);                           // [16 waves][64][4] boxes of a column block
    float* saw = sbw + 16 * 64 * 4;                                            // [16][64] areas
    float* scw = saw + 16 * 64;                                                // [16][64] class columns
    __shared__ int s_n, s_kept;
    __shared__ int s_owner[64], s_keptl[64];
    __shared__ unsigned long long s_bits[64];
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6, fr = blockIdx.x;
    const float* __restrict__ rows = a.rows + (size_t)fr * a.frame_stride;
    const int* __restrict__ counts = a.counts + (size_t)fr * a.T;
    float* __restrict__ out = a.out + (size_t)fr * a.out_frame_stride;
    int* __restrict__ out_src = a.out_src + (size_t)fr * a.src_frame_stride;
    const SlWs w = sl_carve(a.ws + (size_t)fr * a.ws_stride, a.cap, a.words);
    const int W = a.words;
    // candidate s = tile * R + row: its shifted box (one f32 add per corner), area, class column
    auto cand = [&](int s, float& x1, float& y1, float& x2, float& y2, float& ar, float& cl) {
        const int t = s / a.R, r = s - t * a.R;
        const float* row = rows + (size_t)t * a.tile_stride + (size_t)r * a.ld;
        const float ox = (float)a.tiles[t].x0, oy = (float)a.tiles[t].y0;
        x1 = row[0] + ox; y1 = row[1] + oy; x2 = row[2] + ox; y2 = row[3] + oy;
        ar = (x2 - x1) * (y2 - y1);
        cl = row[5];
    };
    // ---- phase A: candidates ----
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int s = tid; s < a.T * a.R; s += 1024) {
        const int t = s / a.R, r = s - t * a.R;
        if (r < min(max(counts[t], 0), a.R)) {
            const float score = rows[(size_t)t * a.tile_stride + (size_t)r * a.ld + 4];
            k[atomicAdd(&s_n, 1)] = ((unsigned long long)(~__float_as_uint(score)) << 32) | (unsigned)s;
        }
    }
    __syncthreads();
    const int n = s_n;
    const int* kl;                                                             // kept list (sorted positions)
    if (n <= 64) {
        kl = s_keptl;
        if (wv == 0) {
            unsigned long long key = l < n ? k[l] : ~0ull;
            auto shfl64 = [](unsigned long long v, int src) {
                const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src);
                return ((unsigned long long)hi << 32) | lo;
            };
#pragma unroll
            for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
                for (int strd = size >> 1; strd > 0; strd >>= 1) {
                    const unsigned long long other = shfl64(key, l ^ strd);
                    const bool lower = (l & strd) == 0, up = (l & size) == 0;
                    const bool take_min = lower == up;
                    key = take_min ? (key < other ? key : other) : (key > other ? key : other);
                }
            float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, ai = 0.f, ci = 0.f;
            SS_WAVE_SYNC();                                                    // every lane has read its unsorted key
            if (l < n) {
                k[l] = key;
                cand((int)(key & 0xffffffffu), x1, y1, x2, y2, ai, ci);
                sbw[l * 4] = x1; sbw[l * 4 + 1] = y1; sbw[l * 4 + 2] = x2; sbw[l * 4 + 3] = y2; saw[l] = ai; scw[l] = ci;
            }
            SS_WAVE_SYNC();
            unsigned long long bits = 0;
            if (l < n)
                for (int q = l + 1; q < n; ++q)
                    if ((a.agnostic || ci == scw[q]) &&
                        sl_match(x1, y1, x2, y2, ai, sbw[q * 4], sbw[q * 4 + 1], sbw[q * 4 + 2], sbw[q * 4 + 3], saw[q], a.ios, a.thr, false))
                        bits |= 1ull << q;
            s_bits[l] = bits;
            unsigned long long rw = 0;
            int kept = 0, owner = -1;
            for (int q = 0; q < n; ++q) {
                if (!((rw >> q) & 1ull)) {
                    if (l == 0) s_keptl[kept] = q;
                    ++kept;
                    const unsigned long long bq = shfl64(bits, q);
                    if (((bq & ~rw) >> l) & 1ull) owner = q;
                    rw |= bq;
                }
            }
            s_owner[l] = owner;
            if (l == 0) s_kept = kept;
            SS_WAVE_SYNC();
            if (l < min(kept, a.out_cap)) {                                    // phase D: lane = kept box
                const int i = s_keptl[l];
                float cx1 = sbw[i * 4], cy1 = sbw[i * 4 + 1], cx2 = sbw[i * 4 + 2], cy2 = sbw[i * 4 + 3];
                if (a.nmm) {
                    const unsigned long long bi = s_bits[i];
                    for (int j = i + 1; j < n; ++j) {
                        if (!((bi >> j) & 1ull) || s_owner[j] != i) continue;
                        const float ac = (cx2 - cx1) * (cy2 - cy1);
                        if (sl_match(cx1, cy1, cx2, cy2, ac, sbw[j * 4], sbw[j * 4 + 1], sbw[j * 4 + 2], sbw[j * 4 + 3], saw[j], a.ios, a.thr, true)) {
                            cx1 = fminf(cx1, sbw[j * 4]); cy1 = fminf(cy1, sbw[j * 4 + 1]);
                            cx2 = fmaxf(cx2, sbw[j * 4 + 2]); cy2 = fmaxf(cy2, sbw[j * 4 + 3]);
                        }
                    }
                }
                float* r = out + (size_t)l * a.out_ld;
                r[0] = cx1; r[1] = cy1; r[2] = cx2; r[3] = cy2;
            }
        }
        __threadfence_block();
        __syncthreads();
    } else {
        kl = w.kept;
        int np = 1; while (np < n) np <<= 1;
        for (int i = n + tid; i < np; i += 1024) k[i] = ~0ull;
        __syncthreads();
        for (int size = 2; size <= np; size <<= 1)
            for (int strd = size >> 1; strd > 0; strd >>= 1) {
                for (int i = tid; i < np / 2; i += 1024) {
                    int lo = 2 * i - (i & (strd - 1)), hi = lo + strd;
                    bool up = (lo & size) == 0;
                    unsigned long long ka = k[lo], kb = k[hi];
                    if ((ka > kb) == up) { k[lo] = kb; k[hi] = ka; }
                }
                __syncthreads();
            }
        for (int i = tid; i < n; i += 1024) {
            float x1, y1, x2, y2, ar, cl;
            cand((int)(k[i] & 0xffffffffu), x1, y1, x2, y2, ar, cl);
            w.box[i * 4] = x1; w.box[i * 4 + 1] = y1; w.box[i * 4 + 2] = x2; w.box[i * 4 + 3] = y2;
            w.area[i] = ar; w.cls[i] = cl;
        }
        __threadfence_block();
        __syncthreads();
        // ---- phase B ----
        {
            float* sb = sbw + wv * 256;
            float* sa = saw + wv * 64;
            float* sc = scw + wv * 64;
            const int nblk = (n + 63) / 64, npair = nblk * (nblk + 1) / 2, t = l;
            for (int pr = wv; pr < npair; pr += 16) {
                int ib = 0, rem = pr;
                while (rem >= nblk - ib) { rem -= nblk - ib; ++ib; }
                const int jb = ib + rem;
                const int j = jb * 64 + t;
                SS_WAVE_SYNC();                                          // the previous pair's reads of the tiles are done
                if (j < n) { sb[t * 4] = w.box[j * 4]; sb[t * 4 + 1] = w.box[j * 4 + 1]; sb[t * 4 + 2] = w.box[j * 4 + 2]; sb[t * 4 + 3] = w.box[j * 4 + 3]; sa[t] = w.area[j]; sc[t] = w.cls[j]; }
                SS_WAVE_SYNC();
                const int i = ib * 64 + t;
                if (i >= n) continue;
                const float x1 = w.box[i * 4], y1 = w.box[i * 4 + 1], x2 = w.box[i * 4 + 2], y2 = w.box[i * 4 + 3], ai = w.area[i], ci = w.cls[i];
                unsigned long long bits = 0;
                const int jn = min(64, n - jb * 64);
                for (int q = 0; q < jn; ++q) {
                    if (jb * 64 + q <= i) continue;
                    if ((a.agnostic || ci == sc[q]) &&
                        sl_match(x1, y1, x2, y2, ai, sb[q * 4], sb[q * 4 + 1], sb[q * 4 + 2], sb[q * 4 + 3], sa[q], a.ios, a.thr, false))
                        bits |= 1ull << q;
                }
                w.mask[(size_t)i * W + jb] = bits;
            }
        }
        __threadfence_block();
        __syncthreads();
        // ---- phase C: greedy scan on wave 0; lane l owns the removed words l and l + 64 ----
        if (wv == 0) {
            const int nw = (n + 63) / 64;
            unsigned long long rem0 = 0, rem1 = 0;
            int kept = 0;
            for (int ib = 0; ib < nw; ++ib) {
                unsigned long long rw = __shfl((ib < 64) ? rem0 : rem1, ib & 63);
                const int i0 = ib * 64;
                const int cnt = min(64, n - i0);
                const unsigned long long diag = (l < cnt) ? w.mask[(size_t)(i0 + l) * W + ib] : 0ull;
                unsigned long long keptbits = 0;
                int owner = -1;
                for (int q = 0; q < cnt; ++q) {
                    if (!((rw >> q) & 1ull)) {
                        keptbits |= 1ull << q;
                        if (l == 0) w.kept[kept] = i0 + q;
                        ++kept;
                        const unsigned long long dq = __shfl(diag, q);
                        if (((dq & ~rw) >> l) & 1ull) owner = i0 + q;
                        rw |= dq;
                    }
                }
                if (owner >= 0) w.owner[i0 + l] = owner;                // removed inside its own block: no earlier block matched it
                // the rows of this block's kept boxes, in order, into the removed words of the later blocks: a newly set bit's owner is
                // that box.  Four independent row loads in flight per step.
                unsigned long long kb = keptbits;
                while (kb) {
                    int q[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) { q[u] = kb ? __builtin_ctzll(kb) : -1; if (kb) kb &= kb - 1; }
                    unsigned long long a0[4], a1[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        a0[u] = a1[u] = 0ull;
                        if (q[u] >= 0) {
                            const unsigned long long* mr = w.mask + (size_t)(i0 + q[u]) * W;
                            if (l > ib && l < nw) a0[u] = mr[l];
                            if (l + 64 > ib && l + 64 < nw) a1[u] = mr[l + 64];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        unsigned long long nb = a0[u] & ~rem0;
                        while (nb) { const int t = __builtin_ctzll(nb); nb &= nb - 1; w.owner[l * 64 + t] = i0 + q[u]; }
                        rem0 |= a0[u];
                        nb = a1[u] & ~rem1;
                        while (nb) { const int t = __builtin_ctzll(nb); nb &= nb - 1; w.owner[(l + 64) * 64 + t] = i0 + q[u]; }
                        rem1 |= a1[u];
                    }
                }
            }
            if (l == 0) s_kept = kept;
        }
        __threadfence_block();
        __syncthreads();
        // ---- phase D: one thread per kept box ----
        const int m = min(s_kept, a.out_cap), nw = (n + 63) / 64;
        for (int kk = tid; kk < m; kk += 1024) {
            const int i = w.kept[kk];
            float cx1 = w.box[i * 4], cy1 = w.box[i * 4 + 1], cx2 = w.box[i * 4 + 2], cy2 = w.box[i * 4 + 3];
            if (a.nmm)
                for (int wd = i >> 6; wd < nw; ++wd) {
                    unsigned long long bits = w.mask[(size_t)i * W + wd];
                    while (bits) {
                        const int j = wd * 64 + __builtin_ctzll(bits);
                        bits &= bits - 1;
                        if (w.owner[j] != i) continue;
                        const float ac = (cx2 - cx1) * (cy2 - cy1);
                        if (sl_match(cx1, cy1, cx2, cy2, ac, w.box[j * 4], w.box[j * 4 + 1], w.box[j * 4 + 2], w.box[j * 4 + 3], w.area[j], a.ios, a.thr, true)) {
                            cx1 = fminf(cx1, w.box[j * 4]); cy1 = fminf(cy1, w.box[j * 4 + 1]);
                            cx2 = fmaxf(cx2, w.box[j * 4 + 2]); cy2 = fmaxf(cy2, w.box[j * 4 + 3]);
                        }
                    }
                }
            float* r = out + (size_t)kk * a.out_ld;
            r[0] = cx1; r[1] = cy1; r[2] = cx2; r[3] = cy2;
        }
        __syncthreads();
    }
    // ---- phase E: score, class, extras of the kept rows; source indices; count ----
    const int m = min(s_kept, a.out_cap), ncol = 2 + a.n_extra, kend = 6 + 3 * a.n_kpt;
    if (tid == 0) a.out_count[fr] = m;
    for (int idx = tid; idx < m * ncol; idx += 1024) {
        const int kk = idx / ncol, c = 4 + (idx - kk * ncol);
        const int s = (int)(k[kl[kk]] & 0xffffffffu);
        const int t = s / a.R, r = s - t * a.R;
        float v = rows[(size_t)t * a.tile_stride + (size_t)r * a.ld + c];
        if (c >= 6 && c < kend) {
            const int comp = (c - 6) % 3;
            const float* g = a.geom + t * 5;
            if (comp == 0) v = ((v - g[1]) / g[0] + (float)a.tiles[t].x0) * a.kg + a.kpx;
            else if (comp == 1) v = ((v - g[2]) / g[0] + (float)a.tiles[t].y0) * a.kg + a.kpy;
        }
        out[(size_t)kk * a.out_ld + c] = v;
        if (c == 4) out_src[kk] = s;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
struct SSSlice {
    int T = 0, H = 0, W = 0, ch = 0, cw = 0, R = 0, n_extra = 0, n_kpt = 0;
    float kg = 1.0f, kpx = 0.0f, kpy = 0.0f;
    float geom[SL_TILES][5];
    SsBuf<SS_DEVICE> tiles, dgeom, ws;
    int ws_frames = 0;
};

int ss_slice_max_tiles_impl() { return SL_TILES; }
int ss_slice_max_candidates_impl() { return SL_CAND; }
void ss_slice_free(SSSlice* s) { delete s; }

int ss_slice_config_check_impl(const int* h_tiles, int n_tiles, int frame_h, int frame_w, int canvas_h, int canvas_w, int rows_per_tile, int n_extra,
                               int n_kpt, float kpt_gain, float kpt_pad_x, float kpt_pad_y, std::string& err)
{
    const std::string who = "ss_slice_config: ";
    auto num = [](long long v) { return std::to_string(v); };
    if (!h_tiles) { err = who + "null tile table"; return SS_ERR_INVALID; }
    if (n_tiles < 1 || n_tiles > SL_TILES) { err = who + num(n_tiles) + " tiles, 1 to " + num(SL_TILES) + " allowed"; return SS_ERR_INVALID; }
    if (frame_h < 1 || frame_w < 1 || frame_h > 32768 || frame_w > 32768) { err = who + "frame size outside 1..32768"; return SS_ERR_INVALID; }
    if (canvas_h < 1 || canvas_w < 1 || canvas_h > 16384 || canvas_w > 16384) { err = who + "canvas size outside 1..16384"; return SS_ERR_INVALID; }
    if (rows_per_tile < 1) { err = who + "rows_per_tile " + num(rows_per_tile) + " below 1"; return SS_ERR_INVALID; }
    if ((long long)n_tiles * rows_per_tile > SL_CAND) { err = who + num(n_tiles) + " tiles x " + num(rows_per_tile) + " rows is over the cap of " + num(SL_CAND) + " candidates"; return SS_ERR_INVALID; }
    if (n_extra < 0 || n_extra > 4096) { err = who + "n_extra outside 0..4096"; return SS_ERR_INVALID; }
    if (n_kpt < 0 || 3 * (long long)n_kpt > n_extra) { err = who + num(n_kpt) + " keypoint triples do not fit " + num(n_extra) + " extra columns"; return SS_ERR_INVALID; }
    if (n_kpt && !(std::isfinite(kpt_gain) && kpt_gain > 0.0f && std::isfinite(kpt_pad_x) && std::isfinite(kpt_pad_y))) { err = who + "keypoint geometry must be finite, gain above 0"; return SS_ERR_INVALID; }
    for (int t = 0; t < n_tiles; ++t) {
        const int* q = h_tiles + 8 * t;
        const std::string tile = who + "tile " + num(t) + ": ";
        if (q[2] < 1 || q[3] < 1 || q[0] < 0 || q[1] < 0 || (long long)q[0] + q[2] > frame_w || (long long)q[1] + q[3] > frame_h) { err = tile + "window leaves the frame"; return SS_ERR_INVALID; }
        if (q[4] < 1 || q[5] < 1 || q[6] < 0 || q[7] < 0 || (long long)q[6] + q[4] > canvas_w || (long long)q[7] + q[5] > canvas_h) { err = tile + "resized image leaves the canvas"; return SS_ERR_INVALID; }
    }
    return SS_OK;
}

int ss_slice_config_impl(SSSlice** ps, const int* h_tiles, int n_tiles, int frame_h, int frame_w, int canvas_h, int canvas_w, int rows_per_tile, int n_extra,
                         int n_kpt, float kpt_gain, float kpt_pad_x, float kpt_pad_y, std::string& err)
{
    const char* who = "ss_slice_config: ";
    ss_slice_free(*ps);
    *ps = nullptr;
    SSSlice* s = new SSSlice();
    s->T = n_tiles; s->H = frame_h; s->W = frame_w; s->ch = canvas_h; s->cw = canvas_w; s->R = rows_per_tile; s->n_extra = n_extra; s->n_kpt = n_kpt;
    s->kg = kpt_gain; s->kpx = kpt_pad_x; s->kpy = kpt_pad_y;
    for (int t = 0; t < n_tiles; ++t) {          // scale_boxes geometry of a tile on the canvas (engine.scale_geometry, in double)
        const double tw = h_tiles[8 * t + 2], th = h_tiles[8 * t + 3];
        const double gain = std::fmin((double)canvas_h / th, (double)canvas_w / tw);
        s->geom[t][0] = (float)gain;
        s->geom[t][1] = (float)(std::nearbyint((canvas_w - tw * gain) / 2 - 0.1) + 0.0);      // + 0.0: a rounded -0.1 is -0, Python's round gives 0
        s->geom[t][2] = (float)(std::nearbyint((canvas_h - th * gain) / 2 - 0.1) + 0.0);
        s->geom[t][3] = (float)tw; s->geom[t][4] = (float)th;
    }
    hipError_t e = s->tiles.reserve((size_t)n_tiles * sizeof(SlTile), SS_EXACT);
    if (e == hipSuccess) e = s->dgeom.reserve((size_t)n_tiles * 5 * sizeof(float), SS_EXACT);
    if (e == hipSuccess) e = hipMemcpy(s->tiles.as<>(), h_tiles, (size_t)n_tiles * sizeof(SlTile), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->dgeom.as<>(), s->geom, (size_t)n_tiles * 5 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_slice_merge, hipFuncAttributeMaxDynamicSharedMemorySize, SL_CAND * 8 + 24576);
    if (e != hipSuccess) { delete s; err = std::string(who) + hipGetErrorString(e); return SS_ERR_HIP; }
    *ps = s;
    return SS_OK;
}

int ss_slice_nms_geom_impl(const SSSlice* s, float* d_geom, int batch, std::string& err)
{
    for (int b = 0; b < batch; ++b)
        SS_HIPCHK("ss_slice_nms_geom: ", hipMemcpy(d_geom + (size_t)b * s->T * 5, s->geom, (size_t)s->T * 5 * sizeof(float), hipMemcpyHostToDevice));
    return SS_OK;
}

int ss_slice_letterbox_check_impl(const uint8_t* d_src, int batch, long long src_batch_stride, int row_stride, const void* d_dst, int dst_flags,
                                  int pad_value, std::string& err)
{
    const std::string who = "ss_slice_letterbox_batch: ";
    const char* bad = nullptr;
    if (!d_src || !d_dst) bad = "null pointer";
    else if (batch < 0 || batch > 65535) bad = "batch outside 0..65535";
    else if (src_batch_stride < 0 || row_stride < 3) bad = "negative frame stride or row_stride below 3";
    else if (dst_flags < 0 || dst_flags > 3) bad = "dst_flags outside 0..3 (SS_DST_F16 | SS_DST_HWC)";
    else if (pad_value < 0 || pad_value > 255) bad = "pad_value outside 0..255";
    else if ((uintptr_t)d_dst & ((dst_flags & 1) ? 1 : 3)) bad = "output not aligned to its element";
    if (bad) { err = who + bad; return SS_ERR_INVALID; }
    return SS_OK;
}

int ss_slice_letterbox_impl(SSSlice* s, hipStream_t st, const uint8_t* d_src, int batch, long long src_batch_stride, int row_stride, void* d_dst,
                            int dst_flags, int pad_value, std::string& err)
{
    const std::string who = "ss_slice_letterbox_batch: ";
    if (row_stride < 3 * s->W) { err = who + "row_stride below 3 * frame width"; return SS_ERR_INVALID; }
    if (batch > 1 && src_batch_stride < (long long)s->H * row_stride) { err = who + "frames overlap (src_batch_stride below h * row_stride)"; return SS_ERR_INVALID; }
    if ((long long)batch * s->T > 65535) { err = who + "batch * tiles above 65535"; return SS_ERR_INVALID; }
    if (batch == 0) return SS_OK;
    const int hwc = (dst_flags & 2) != 0, epc = (dst_flags & 1) ? 8 : 4;
    const int n_lines = hwc ? s->ch : 3 * s->ch, n_el = hwc ? 3 * s->cw : s->cw;
    const int nch = (n_el + epc - 1) / epc + 1;
    dim3 grid((nch + 255) / 256, (n_lines + SL_LINES - 1) / SL_LINES, batch * s->T), block(256);
    const float padv = (float)pad_value / 255.0f;
#define SS_SLB(TY, L) hipLaunchKernelGGL((k_slice_letterbox<TY, L>), grid, block, 0, st, d_src, src_batch_stride, row_stride, s->tiles.as<SlTile>(), s->T, \
                                        (TY*)d_dst, s->ch, s->cw, padv)
    switch (dst_flags & 3) {
    case 0: SS_SLB(float, 0); break;
    case 1: SS_SLB(__half, 0); break;
    case 2: SS_SLB(float, 1); break;
    default: SS_SLB(__half, 1); break;
    }
#undef SS_SLB
    SS_HIPCHK(who, hipGetLastError());
    return SS_OK;
}

int ss_slice_merge_check_impl(const float* d_rows, const int* d_counts, int batch, int row_stride, long long tile_stride, long long frame_stride, int mode,
                              int metric, float thr, int agnostic, int out_cap, const float* d_out, int out_row_stride, long long out_frame_stride,
                              const int* d_out_count, const int* d_out_src, long long src_frame_stride, std::string& err)
{
    const std::string who = "ss_slice_merge: ";
    const char* bad = nullptr;
    if (!d_rows || !d_counts || !d_out || !d_out_count || !d_out_src) bad = "null pointer";
    else if (batch < 0 || batch > 65535) bad = "batch outside 0..65535";
    else if (row_stride < 6 || tile_stride < 0 || frame_stride < 0) bad = "row_stride below 6 or a negative stride";
    else if (mode != 0 && mode != 1) bad = "mode must be 0 (nms) or 1 (nmm)";
    else if (metric != 0 && metric != 1) bad = "metric must be 0 (iou) or 1 (ios)";
    else if (!std::isfinite(thr)) bad = "threshold is not finite";
    else if (agnostic != 0 && agnostic != 1) bad = "agnostic must be 0 or 1";
    else if (out_cap < 1 || out_cap > SL_CAND) bad = "out_cap outside 1..8192";
    else if (out_row_stride < 6) bad = "out_row_stride below 6";
    else if (batch > 1 && (out_frame_stride < (long long)out_cap * out_row_stride || src_frame_stride < out_cap)) bad = "output frames overlap";
    if (bad) { err = who + bad; return SS_ERR_INVALID; }
    return SS_OK;
}

int ss_slice_merge_impl(SSSlice* s, hipStream_t st, const float* d_rows, const int* d_counts, int batch, int row_stride, long long tile_stride,
                        long long frame_stride, int mode, int metric, float thr, int agnostic, int out_cap, float* d_out, int out_row_stride,
                        long long out_frame_stride, int* d_out_count, int* d_out_src, long long src_frame_stride, std::string& err)
{
    const std::string who = "ss_slice_merge: ";
    if (row_stride < 6 + s->n_extra || out_row_stride < 6 + s->n_extra) { err = who + "a row stride is below 6 + n_extra"; return SS_ERR_INVALID; }
    if (s->T > 1 && tile_stride < (long long)s->R * row_stride) { err = who + "tiles overlap (tile_stride below rows_per_tile * row_stride)"; return SS_ERR_INVALID; }
    if (batch > 1 && frame_stride < (s->T - 1) * tile_stride + (long long)s->R * row_stride) { err = who + "frames overlap (frame_stride)"; return SS_ERR_INVALID; }
    if (batch == 0) return SS_OK;
    const int cap = s->T * s->R, words = (cap + 63) / 64;
    int np2 = 64; while (np2 < cap) np2 <<= 1;
    const size_t unit = sl_ws_bytes(cap, words);
    if (batch > s->ws_frames) {                  // growing allocates, which a stream capture does not allow
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (st) SS_HIPCHK(who, hipStreamIsCapturing(st, &cs));
        if (cs != hipStreamCaptureStatusNone) { err = who + "the first call with this batch size must not be inside a graph capture"; return SS_ERR_INVALID; }
        SS_HIPCHK(who, hipStreamSynchronize(st));
        s->ws_frames = 0;
        SS_HIPCHK(who, s->ws.reserve(unit * (size_t)batch, SS_EXACT));
        s->ws_frames = batch;
    }
    SlMerge a;
    a.rows = d_rows; a.counts = d_counts; a.tiles = s->tiles.as<SlTile>(); a.geom = s->dgeom.as<float>();
    a.T = s->T; a.R = s->R; a.ld = row_stride; a.tile_stride = tile_stride; a.frame_stride = frame_stride;
    a.n_extra = s->n_extra; a.n_kpt = s->n_kpt; a.kg = s->kg; a.kpx = s->kpx; a.kpy = s->kpy;
    a.nmm = mode; a.ios = metric; a.agnostic = agnostic; a.thr = thr; a.out_cap = out_cap;
    a.out = d_out; a.out_ld = out_row_stride; a.out_frame_stride = out_frame_stride; a.out_count = d_out_count; a.out_src = d_out_src;
    a.src_frame_stride = src_frame_stride;
    a.ws = s->ws.as<char>(); a.ws_stride = (long long)unit; a.cap = cap; a.words = words; a.np2 = np2;
    hipLaunchKernelGGL(k_slice_merge, dim3(batch), dim3(1024), (size_t)np2 * 8 + 24576, st, a);
    SS_HIPCHK(who, hipGetLastError());
    return SS_OK;
}
