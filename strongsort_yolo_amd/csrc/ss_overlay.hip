// ss_overlay.hip — annotation overlay on device frames: boxes, label plates and text, keypoint dots,
// trajectory lines, the blended class-count plate.  Replaces the cv2 drawing of /root/reference/yolo_multi_model.py:58-162
// and :311-331 (per-box rectangle / putText / circle / line calls and the addWeighted count plate), which the reference
// runs on the CPU on a copy of every frame.
//
// A frame's annotation is an ORDERED list of primitives (painter's algorithm: a later primitive overwrites an earlier
// one).  The kernel is pixel-centric so that the order is kept without atomics: one 32x8 pixel tile per workgroup; per
// chunk of 256 primitives every thread tests one primitive's bounding box against the tile, the hits are compacted in
// order into LDS, and every pixel walks the hits in order with exact integer coverage tests (no floating point, so the
// NumPy rasteriser used as the oracle reproduces every pixel).  Pixels no primitive covers are not touched.
#include "ss_common.h"
#include "ss_cover.h"
#include "ss_launch.h"

__device__ __forceinline__ int ov_mix(int top, int under)        // 0.7 : 0.3 in 8-bit fixed point (179 : 77), per channel
{
    int out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int t = (top >> (8 * c)) & 255, u = (under >> (8 * c)) & 255;
        out |= ((179 * t + 77 * u + 128) >> 8) << (8 * c);
    }
    return out;
}

__device__ __forceinline__ int ov_half(int a, int b)             // (a + b) / 2 per channel, ties to even (cv2.addWeighted 0.5 / 0.5 + saturate_cast)
{
    int out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int t = ((a >> (8 * c)) & 255) + ((b >> (8 * c)) & 255);
        out |= ((t >> 1) + ((t & 1) & ((t >> 1) & 1))) << (8 * c);
    }
    return out;
}

// grid = (ceil(W/32), ceil(H/8), batch); prim_off[b] .. prim_off[b+1] = primitives of frame b
__global__ __launch_bounds__(256) void k_overlay(uint8_t* __restrict__ frames, long long frame_stride, int H, int W, int row_stride,
                                                 const OvPrim* __restrict__ prims, const int* __restrict__ prim_off,
                                                 const uint8_t* __restrict__ chars, const uint8_t* __restrict__ font)
{
    __shared__ OvPrim hits[256];
    __shared__ int wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tx0 = blockIdx.x * 32, ty0 = blockIdx.y * 8;
    const int x = tx0 + (tid & 31), y = ty0 + (tid >> 5);
    const bool inside = x < W && y < H;
    uint8_t* px = frames + (size_t)blockIdx.z * frame_stride + (size_t)y * row_stride + (size_t)x * 3;
    const int p0 = prim_off[blockIdx.z], p1 = prim_off[blockIdx.z + 1];
    int cur = 0, grp = 0;
    bool touched = false, in_grp = false, loaded = false;
    for (int base = p0; base < p1; base += 256) {
        // ordered compaction of the primitives of this chunk whose bounding box meets the tile
        OvPrim p;
        bool hit = false;
        if (base + tid < p1) {
            p = prims[base + tid];
            int bx0, by0, bx1, by1;
            ov_bbox(p, bx0, by0, bx1, by1);
            hit = bx1 >= tx0 && bx0 < tx0 + 32 && by1 >= ty0 && by0 < ty0 + 8;
        }
        const unsigned long long m = __ballot(hit);
        __syncthreads();                                   // the previous chunk's readers are done with hits / wtot
        if (lane == 0) wtot[wv] = __popcll(m);
        __syncthreads();
        int off = 0, n = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const int c = wtot[i]; if (i < wv) off += c; n += c; }
        if (hit) hits[off + __popcll(m & ((1ull << lane) - 1ull))] = p;
        __syncthreads();
        if (inside)
            for (int i = 0; i < n; ++i) {
                const OvPrim& q = hits[i];
                if (!ov_covers(q, x, y, chars, font)) continue;
                if (!loaded) { cur = px[0] | (px[1] << 8) | (px[2] << 16); loaded = true; }
                if (q.type == OV_POLY) { if (in_grp) { cur = ov_mix(grp, cur); in_grp = false; } cur = ov_half(cur, q.color); }
                else if (q.b & 1) { grp = q.color; in_grp = true; }
                else { if (in_grp) { cur = ov_mix(grp, cur); in_grp = false; } cur = q.color; }
                touched = true;
            }
    }
    if (touched) {
        if (in_grp) cur = ov_mix(grp, cur);
        px[0] = (uint8_t)cur; px[1] = (uint8_t)(cur >> 8); px[2] = (uint8_t)(cur >> 16);
    }
}

void ss_launch_overlay(uint8_t* frames, int batch, long long frame_stride, int h, int w, int row_stride, const void* prims,
                       const int* prim_off, const uint8_t* chars, const uint8_t* font, hipStream_t st)
{
    if (batch <= 0 || h <= 0 || w <= 0) return;
    hipLaunchKernelGGL(k_overlay, dim3((w + 31) / 32, (h + 7) / 8, batch), dim3(256), 0, st, frames, frame_stride, h, w, row_stride,
                       (const OvPrim*)prims, prim_off, chars, font);
}
