// ss_probiou.h — ProbIoU of two oriented boxes (cx, cy, w, h, theta) as one fixed sequence of float64 operations (docs/OBB.md §1).
// The rotated NMS (ss_front.hip) thresholds this value, the BYTE tracker (ss_byte.hip) associates on it and the test entry ss_probiou returns it, and tests/obb_ref.py must form it bit for
// bit: libm's log / sin / cos and the device's round differently, so the three elementary functions are fixed sequences too.
//
//   ss_log(x)     x = m 2^e with m in [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1), log m = 2 s (1 + z/3 + z^2/5 + ..), z = s^2, twelve terms;
//                 e LN2_HI + (2 s p + e LN2_LO).  Domain: positive normal finite x; anything else gives NaN.
//   ss_sincos(t)  k = floor(t 2/pi + 1/2), r = (((t - k P1) - k P2) - k P3) - k P3T (Cody-Waite: P1..P3 hold 33 bits each, the products with
//                 |k| < 2^20 are exact), Taylor polynomials of sin and cos in r^2 on |r| <= pi/4, quadrant by k mod 4.
//                 Domain: |t| <= 2^20; outside it (and for a NaN) both results are NaN, which makes the box degenerate (R-01).
//   ss_expneg     csrc/ss_expneg.h, as it is.
//
// Every step is one multiplication, one addition, one division or one square root, rounded once (the library is built with
// -ffp-contract=off; no fma here); sqrt and division are correctly rounded on both sides.  Plain C++: a host compiler can include this
// header on its own (tests/probiou_host_main.cpp).
#pragma once
#include <math.h>
#include "ss_expneg.h"

#if defined(__HIPCC__)
#define SS_PROBIOU_FN __host__ __device__ inline
#else
#define SS_PROBIOU_FN inline
#endif

#define SS_PROBIOU_EPS 1e-7
#define SS_SINCOS_MAX 1048576.0
#define SS_LOG_TERMS 12
#define SS_SIN_TERMS 9
#define SS_COS_TERMS 10

SS_PROBIOU_FN double ss_log(double x)
{
    // 1 / (2k + 1), k = 0 .. 11
    const double L[SS_LOG_TERMS] = {
        1.0, 0.3333333333333333, 0.2, 0.14285714285714285, 0.1111111111111111, 0.09090909090909091, 0.07692307692307693,
        0.06666666666666667, 0.058823529411764705, 0.05263157894736842, 0.047619047619047616, 0.043478260869565216};
    if (!(x >= 2.2250738585072014e-308) || x > 1.7976931348623157e308) return NAN;
    unsigned long long u;
    __builtin_memcpy(&u, &x, 8);
    int e = (int)(u >> 52) - 1023;
    u = (u & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    double m;
    __builtin_memcpy(&m, &u, 8);                                  // [1, 2)
    if (m > 1.4142135623730951) { m = m * 0.5; e = e + 1; }         // [sqrt(1/2), sqrt(2)); the halving is exact
    const double f = m - 1.0;                                      // exact
    const double s = f / (2.0 + f);
    const double z = s * s;
    double p = L[SS_LOG_TERMS - 1];
#pragma unroll
    for (int k = SS_LOG_TERMS - 2; k >= 0; --k) { p = p * z; p = p + L[k]; }
    double r = 2.0 * s;
    r = r * p;
    const double de = (double)e;
    double lo = de * 0x1.a39ef35793c76p-33;
    lo = r + lo;
    const double hi = de * 0x1.62e42feep-1;                        // exact: 32 bits times at most 11
    return hi + lo;
}

SS_PROBIOU_FN void ss_sincos(double t, double* sn, double* cs)
{
    // (-1)^k / (2k + 1)!, k = 0 .. 8  and  (-1)^k / (2k)!, k = 0 .. 9
    const double S[SS_SIN_TERMS] = {
        1.0, -0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06, -2.505210838544172e-08,
        1.6059043836821613e-10, -7.647163731819816e-13, 2.8114572543455206e-15};
    const double Cc[SS_COS_TERMS] = {
        1.0, -0.5, 0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05, -2.755731922398589e-07,
        2.08767569878681e-09, -1.1470745597729725e-11, 4.779477332387385e-14, -1.5619206968586225e-16};
    if (!(fabs(t) <= SS_SINCOS_MAX)) { *sn = NAN; *cs = NAN; return; }
    const double k = floor(t * 0.6366197723675814 + 0.5);
    double r = t - k * 1.57079632673412561417e+00;                 // P1: the first 33 bits of pi/2
    r = r - k * 6.07710050630396597660e-11;                        // P2: the next 33
    r = r - k * 2.02226624871116645580e-21;                        // P3: the next 33
    r = r - k * 8.47842766036889956997e-32;                        // P3T: pi/2 - P1 - P2 - P3
    const double z = r * r;
    double ps = S[SS_SIN_TERMS - 1];
#pragma unroll
    for (int i = SS_SIN_TERMS - 2; i >= 0; --i) { ps = ps * z; ps = ps + S[i]; }
    double pc = Cc[SS_COS_TERMS - 1];
#pragma unroll
    for (int i = SS_COS_TERMS - 2; i >= 0; --i) { pc = pc * z; pc = pc + Cc[i]; }
    ps = r * ps;
    const int q = (int)((long long)k & 3);
    *sn = q == 0 ? ps : q == 1 ? pc : q == 2 ? -ps : -pc;
    *cs = q == 0 ? pc : q == 1 ? -ps : q == 2 ? -pc : ps;
}

// Per-box terms, formed once per box.  D < 0 marks a degenerate box (R-01): a non-finite field, w <= 0 or h <= 0, an angle outside
// ss_sincos's domain.  Such a box has ProbIoU 0 with everything.
struct ss_pbox { double x, y, A, B, C, D; };

SS_PROBIOU_FN ss_pbox ss_probiou_box(float cx, float cy, float w, float h, float th)
{
    ss_pbox p;
    p.x = (double)cx; p.y = (double)cy;
    const double dw = (double)w, dh = (double)h;
    const bool fin = fabs(p.x) <= 3.5e38 && fabs(p.y) <= 3.5e38 && fabs(dw) <= 3.5e38 && fabs(dh) <= 3.5e38;     // false for inf and NaN
    double s, c;
    ss_sincos((double)th, &s, &c);
    if (!fin || !(dw > 0.0) || !(dh > 0.0) || s != s) { p.A = p.B = p.C = 0.0; p.D = -1.0; return p; }
    const double a = dw * dw / 12.0, b = dh * dh / 12.0;
    const double cc = c * c, ss = s * s;
    p.A = a * cc + b * ss;
    p.B = a * ss + b * cc;
    p.C = (a - b) * c * s;
    double D = p.A * p.B - p.C * p.C;
    if (!(D > 0.0)) D = 0.0;
    p.D = D;
    return p;
}

SS_PROBIOU_FN double ss_probiou_pair(const ss_pbox& p, const ss_pbox& q)
{
    if (p.D < 0.0 || q.D < 0.0) return 0.0;
    const double eps = SS_PROBIOU_EPS;
    const double sa = p.A + q.A, sb = p.B + q.B, sc = p.C + q.C;
    const double dx = p.x - q.x, dy = p.y - q.y;
    const double den = sa * sb - sc * sc;
    const double de = den + eps;
    const double t1 = (sa * dy * dy + sb * dx * dx) / de * 0.25;
    const double t2 = sc * (-dx) * dy / de * 0.5;
    const double t3 = 0.5 * ss_log(den / (4.0 * sqrt(p.D * q.D) + eps) + eps);
    double bd = t1 + t2 + t3;
    if (bd != bd) return 0.0;                                      // R-01: a NaN result is 0
    if (bd < eps) bd = eps;
    if (bd > 100.0) bd = 100.0;
    return 1.0 - sqrt(1.0 - ss_expneg(bd) + eps);
}

SS_PROBIOU_FN double ss_probiou_xywhr(const float a[5], const float b[5])
{
    return ss_probiou_pair(ss_probiou_box(a[0], a[1], a[2], a[3], a[4]), ss_probiou_box(b[0], b[1], b[2], b[3], b[4]));
}

// The axis-aligned envelope (x1, y1, x2, y2) of a rotated box: the four corners ctr +- (w/2)(cos, sin) +- (h/2)(-sin, cos) in float64,
// their min / max; the caller rounds to float32 (and clips, where it has an image).
SS_PROBIOU_FN void ss_rbox_envelope(float cx, float cy, float bw, float bh, float th, double e[4])
{
    double s, c;
    ss_sincos((double)th, &s, &c);
    const double hw = (double)bw / 2.0, hh = (double)bh / 2.0;
    const double vx = hw * c, vy = hw * s, ux = hh * s, uy = hh * c;
    const double dcx = (double)cx, dcy = (double)cy;
    const double px[4] = { dcx + vx - ux, dcx + vx + ux, dcx - vx + ux, dcx - vx - ux };
    const double py[4] = { dcy + vy + uy, dcy + vy - uy, dcy - vy - uy, dcy - vy + uy };
    double x1 = px[0], x2 = px[0], y1 = py[0], y2 = py[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        if (px[i] < x1) x1 = px[i];
        if (px[i] > x2) x2 = px[i];
        if (py[i] < y1) y1 = py[i];
        if (py[i] > y2) y2 = py[i];
    }
    e[0] = x1; e[1] = y1; e[2] = x2; e[3] = y2;
}
