// ss_redact_div.h — the rounded division of the box blur (ss_redact.hip, docs/REDACT.md) as one multiply and a shift.  No HIP in
// here: tests/redact_div_host_main.cpp includes it and proves the divider exact for every radius and every sum.
//
// k = 2r + 1, d = k * k <= 3969.  The blur's byte is (sum + d / 2) / d with sum in [0, 255 d], so the dividend n is at most
// 255 d + d / 2.  With m = ceil(2^32 / d) and e = m d - 2^32 (0 <= e < d), floor(n m / 2^32) = floor(n / d) whenever n e < 2^32;
// here n e < 255.5 d^2 <= 255.5 * 3969^2 < 2^32.  m < 2^29 fits 32 bits, so the device takes the high word of a 32 x 32 product.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SS_RD_FN __host__ __device__ inline
#else
#define SS_RD_FN inline
#endif

#define SS_REDACT_MAX_RADIUS 31

SS_RD_FN uint32_t ss_redact_div_magic(int r)               // 1 <= r <= SS_REDACT_MAX_RADIUS
{
    const uint64_t d = (uint64_t)(2 * r + 1) * (uint64_t)(2 * r + 1);
    return (uint32_t)((((uint64_t)1 << 32) + d - 1) / d);
}

SS_RD_FN uint32_t ss_redact_div(uint32_t n, uint32_t magic) { return (uint32_t)(((uint64_t)n * magic) >> 32); }

// the byte a window sum becomes: (sum + d / 2) / d
SS_RD_FN uint32_t ss_redact_mean(uint32_t sum, uint32_t d, uint32_t magic) { return ss_redact_div(sum + d / 2, magic); }

// reflect-101 by repeated reflection: period 2 (n - 1), index 0 when n == 1 (any i, any n >= 1)
SS_RD_FN int ss_redact_reflect(int i, int n)
{
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int t = i % p;
    if (t < 0) t += p;
    return t < n ? t : p - t;
}
