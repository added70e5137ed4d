// ss_bilerp.h — the bilinear helpers of the frame-side kernels (oracle so_axis / so_bilerp_u8), shared by ss_front.hip (letterbox,
// ReID crop) and ss_slice.hip (tiled letterbox): one body, so the two files cannot drift apart in a bit.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

__device__ inline void ss_axis(int d, float scale, int n_src, int& i0, int& i1, float& frac)
{
    float t = (float)d + 0.5f;
    float s = t * scale;
    float f = s - 0.5f;
    int i = (int)floorf(f);
    float fr = f - (float)i;
    if (i < 0) { i = 0; fr = 0.0f; }
    if (i >= n_src - 1) { i = n_src - 1; fr = 0.0f; i1 = i; } else i1 = i + 1;
    i0 = i; frac = fr;
}

__device__ inline float ss_bilerp_u8(float p00, float p01, float p10, float p11, float fx, float fy)
{
    float a = fmaf(fx, p01 - p00, p00);
    float b = fmaf(fx, p11 - p10, p10);
    float v = fmaf(fy, b - a, a);
    float q = floorf(v + 0.5f);
    return fminf(fmaxf(q, 0.0f), 255.0f);
}

template <typename T> __device__ inline T ss_cvt(float v);
template <> __device__ inline float ss_cvt<float>(float v) { return v; }
template <> __device__ inline __half ss_cvt<__half>(float v) { return __float2half(v); }
