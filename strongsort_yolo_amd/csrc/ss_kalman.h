// ss_kalman.h — the constant-velocity Kalman filter (float64) of every tracker, one thread per track: plain C++, no HIP builtins.
//
// Mirrors oracle so_kf_* line by line (operation order frozen in oracle/DECISIONS.md); tests/bytetrack_ref.py restates both
// parameterisations.  XYWH = false: the xyah filter of StrongSORT (NSA measurement noise, `conf`) and ByteTrack (conf = 0);
// XYWH = true: BoT-SORT's xywh filter (docs/BYTETRACK.md B-03): the same model with every noise term scaled by the box width
// (x, w rows) or height (y, h rows) and no NSA.  Compiled with -ffp-contract=off: only the explicit fma() calls fuse.
// A host compiler can include this header on its own (tests/test_kalman_host_cpu.py); the wave-cooperative forms, which take
// their noise model and gain rows from here, are in ss_common.h.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SS_KF_FN __host__ __device__ inline
#else
#define SS_KF_FN inline
#endif

// ---- the noise model: standard deviation of state row i (0..7; the projection: 0..3), squared by its user ----
// s = the box size a row's noise scales with, from the measurement (initiate) or the mean BEFORE the step (predict, project)
template <bool XYWH> SS_KF_FN double ss_kf_scale(int i, const double* m) { return (XYWH && !(i & 1)) ? m[2] : m[3]; }

template <bool XYWH> SS_KF_FN double ss_kf_sd_initiate(int i, double wp, double wv, const double* z)
{
    if (!XYWH && (i == 2 || i == 6)) return i == 2 ? 1e-2 : 1e-5;
    const double s = ss_kf_scale<XYWH>(i, z);
    return i < 4 ? 2.0 * wp * s : 10.0 * wv * s;
}

template <bool XYWH> SS_KF_FN double ss_kf_sd_predict(int i, double wp, double wv, const double* mean)
{
    if (!XYWH && (i == 2 || i == 6)) return i == 2 ? 1e-2 : 1e-5;
    const double s = ss_kf_scale<XYWH>(i, mean);
    return i < 4 ? wp * s : wv * s;
}

template <bool XYWH> SS_KF_FN double ss_kf_sd_project(int i, double wp, const double* mean)
{
    if (!XYWH && i == 2) return 1e-1;
    return wp * ss_kf_scale<XYWH>(i, mean);
}

// ---- thread forms ----
template <bool XYWH> SS_KF_FN void ss_kf_initiate(const double z[4], double wp, double wv, double* mean, double* cov)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) { mean[i] = z[i]; mean[4 + i] = 0.0; }
    for (int i = 0; i < 64; ++i) cov[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { const double sd = ss_kf_sd_initiate<XYWH>(i, wp, wv, z); cov[i * 8 + i] = sd * sd; }
}

template <bool XYWH> SS_KF_FN void ss_kf_predict(double* mean, double* cov, double wp, double wv)
{
    double sd[8], P[64];
#pragma unroll
    for (int i = 0; i < 8; ++i) sd[i] = ss_kf_sd_predict<XYWH>(i, wp, wv, mean);
#pragma unroll
    for (int i = 0; i < 64; ++i) P[i] = cov[i];
    // A = P F^T (in place on the left half), B = F A (in place on the top half)
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) P[i * 8 + j] = P[i * 8 + j] + P[i * 8 + j + 4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) P[i * 8 + j] = P[i * 8 + j] + P[(i + 4) * 8 + j];
#pragma unroll
    for (int i = 0; i < 8; ++i) P[i * 8 + i] = P[i * 8 + i] + sd[i] * sd[i];
#pragma unroll
    for (int i = 0; i < 64; ++i) cov[i] = P[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) mean[i] = mean[i] + mean[i + 4];
}

// projected mean m4 = H x and innovation covariance S = H P H^T + R; xyah: R scaled by (1 - conf) (NSA), xywh: conf is not used
template <bool XYWH> SS_KF_FN void ss_kf_project(const double* mean, const double* cov, double conf, double wp, double m4[4], double S[16])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        m4[i] = mean[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) S[i * 4 + j] = cov[i * 8 + j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double sd = ss_kf_sd_project<XYWH>(i, wp, mean);
        const double s = XYWH ? sd : (1.0 - conf) * sd;
        S[i * 4 + i] = S[i * 4 + i] + s * s;
    }
}

SS_KF_FN void ss_chol4(const double S[16], double L[16])
{
#pragma unroll
    for (int i = 0; i < 16; ++i) L[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double sum = S[i * 4 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) sum = fma(-L[i * 4 + k], L[j * 4 + k], sum);
            L[i * 4 + j] = (i == j) ? sqrt(sum) : sum / L[j * 4 + j];
        }
}

// squared Mahalanobis distance given L (lower Cholesky of the projected covariance) and m4
SS_KF_FN double ss_maha(const double L[16], const double m4[4], const double z[4])
{
    double y[4], acc = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sum = z[i] - m4[i];
#pragma unroll
        for (int k = 0; k < i; ++k) sum = fma(-L[i * 4 + k], y[k], sum);
        y[i] = sum / L[i * 4 + i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = fma(y[i], y[i], acc);
    return acc;
}

// one row of the gain K = P H^T S^-1: x = (L L^T)^-1 p for the first four entries p of a covariance row (forward, then back substitution)
SS_KF_FN void ss_kf_gain_row(const double L[16], const double* p, double x[4])
{
    double w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sum = p[i];
#pragma unroll
        for (int k = 0; k < i; ++k) sum = fma(-L[i * 4 + k], w[k], sum);
        w[i] = sum / L[i * 4 + i];
    }
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        double sum = w[i];
#pragma unroll
        for (int k = 3; k > i; --k) sum = fma(-L[k * 4 + i], x[k], sum);
        x[i] = sum / L[i * 4 + i];
    }
}

// the correction half of the update (gain by Cholesky solves, mean and covariance) for a projection m4 / S
SS_KF_FN void ss_kf_correct(double* mean, double* cov, const double z[4], const double m4[4], const double S[16])
{
    double L[16], K[32], M[32], y[4];
    ss_chol4(S, L);
#pragma unroll
    for (int r = 0; r < 8; ++r) ss_kf_gain_row(L, cov + r * 8, K + r * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = z[i] - m4[i];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = fma(S[i * 4 + k], K[c * 4 + k], acc);
            M[i * 8 + c] = acc;
        }
    double nm[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc = fma(y[k], K[r * 4 + k], acc);
        nm[r] = mean[r] + acc;
    }
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = fma(K[r * 4 + k], M[k * 8 + c], acc);
            cov[r * 8 + c] = cov[r * 8 + c] - acc;
        }
#pragma unroll
    for (int r = 0; r < 8; ++r) mean[r] = nm[r];
}

template <bool XYWH> SS_KF_FN void ss_kf_update(double* mean, double* cov, const double z[4], double conf, double wp)
{
    double m4[4], S[16];
    ss_kf_project<XYWH>(mean, cov, conf, wp, m4, S);
    ss_kf_correct(mean, cov, z, m4, S);
}
