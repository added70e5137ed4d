// ss_native.hip — BoT-SORT's `model: auto` ReID features on the gfx950 (docs/BYTETRACK.md §1d, decisions N-01..N-05).
//
// The appearance vector of a kept detection is read from the detector's own head inputs (the neck maps P3, P4, P5) at the
// detection's anchor: Ultralytics' get_obj_feats with s = the common group count,
//   raw[j] = (m[j*g] + m[j*g+1] + ... + m[j*g+g-1]) / (float)g,   g = C_l / s,   j < s;   raw[s..512) = 0.
// Each map element is converted to float exactly, the sum runs in ascending channel order from the first term (the library
// is compiled with -ffp-contract=off: no fma) and the divide is correctly rounded.  tests/native_feats_ref.py restates it.
//
//   k_native_feats  one wave per kept row (four per workgroup), grid [SS_MAXD / 4][n_img]: lane l owns the groups l, l+64, ...
//                   (its g channels are contiguous in the channels-last map) and writes the columns l, l+64, ...; rows at or
//                   past the image's count are not touched.
#include "ss_common.h"
#include "ss_launch.h"
#include <hip/hip_fp16.h>

struct SSNativeMaps {
    const void *p0, *p1, *p2;                  // level maps, channel stride 1
    long long is0, is1, is2, rs0, rs1, rs2, ps0, ps1, ps2;     // image / row / pixel strides (elements)
    int g0, g1, g2;                            // channels per group (C_l / s)
    int w0, w1, w2;                            // widths
    int e0, e1, e2;                            // anchor index one past each level (level by level, row-major inside a level)
};

__device__ inline float ss_native_tof(float v) { return v; }
__device__ inline float ss_native_tof(__half v) { return __half2float(v); }

template <typename T>
__global__ __launch_bounds__(256) void k_native_feats(SSNativeMaps m, int s, const int* __restrict__ keep, long long keep_stride,
                                                      const int* __restrict__ counts, float* __restrict__ out)
{
    const int v = blockIdx.y, r = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    const int N = min(max(counts[v], 0), SS_MAXD);
    if (r >= N) return;                                          // whole waves
    const int a = keep[(size_t)v * keep_stride + r];
    // the anchor's level (wave-uniform); an index outside the maps gives a zero row
    const T* px = nullptr;
    int g = 0;
    if (a >= 0 && a < m.e2) {
        const int lv = a < m.e0 ? 0 : (a < m.e1 ? 1 : 2);
        const int i = a - (lv == 0 ? 0 : (lv == 1 ? m.e0 : m.e1));
        const int w = lv == 0 ? m.w0 : (lv == 1 ? m.w1 : m.w2);
        const int y = i / w, x = i - y * w;
        const long long off = (long long)v * (lv == 0 ? m.is0 : (lv == 1 ? m.is1 : m.is2))
                            + (long long)y * (lv == 0 ? m.rs0 : (lv == 1 ? m.rs1 : m.rs2))
                            + (long long)x * (lv == 0 ? m.ps0 : (lv == 1 ? m.ps1 : m.ps2));
        px = (const T*)(lv == 0 ? m.p0 : (lv == 1 ? m.p1 : m.p2)) + off;
        g = lv == 0 ? m.g0 : (lv == 1 ? m.g1 : m.g2);
    }
    float* o = out + ((size_t)v * SS_MAXD + r) * SS_F;
#pragma unroll
    for (int k = 0; k < SS_F / 64; ++k) {
        const int j = l + 64 * k;
        float val = 0.0f;
        if (px && j < s) {
            const T* q = px + (size_t)j * g;
            float acc = ss_native_tof(q[0]);
            for (int c = 1; c < g; ++c) acc += ss_native_tof(q[c]);
            val = acc / (float)g;
        }
        o[j] = val;
    }
}

// Arguments were checked by ss_native_feats (ss_api.hip).  maps: the three levels' pointers; strides in elements.
void ss_launch_native_feats(int n_img, int half, const void* const* p, const long long* img_stride, const long long* row_stride,
                            const long long* pix_stride, const int* channels, const int* height, const int* width, int s,
                            const int* keep, long long keep_stride, const int* counts, float* out, hipStream_t st)
{
    SSNativeMaps m;
    m.p0 = p[0]; m.p1 = p[1]; m.p2 = p[2];
    m.is0 = img_stride[0]; m.is1 = img_stride[1]; m.is2 = img_stride[2];
    m.rs0 = row_stride[0]; m.rs1 = row_stride[1]; m.rs2 = row_stride[2];
    m.ps0 = pix_stride[0]; m.ps1 = pix_stride[1]; m.ps2 = pix_stride[2];
    m.g0 = channels[0] / s; m.g1 = channels[1] / s; m.g2 = channels[2] / s;
    m.w0 = width[0]; m.w1 = width[1]; m.w2 = width[2];
    m.e0 = height[0] * width[0];
    m.e1 = m.e0 + height[1] * width[1];
    m.e2 = m.e1 + height[2] * width[2];
    const dim3 grid(SS_MAXD / 4, n_img), block(256);
    if (half) hipLaunchKernelGGL(k_native_feats<__half>, grid, block, 0, st, m, s, keep, keep_stride, counts, out);
    else hipLaunchKernelGGL(k_native_feats<float>, grid, block, 0, st, m, s, keep, keep_stride, counts, out);
}
