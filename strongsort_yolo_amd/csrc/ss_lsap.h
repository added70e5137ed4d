// ss_lsap.h — the one-wave LSAP in SciPy's scan order and the assignment wrapper around it (rows = the smaller side), shared by the
// StrongSORT kernels (ss_track.hip), the BYTE tracker (ss_byte.hip) and the MOT scorer (ss_mot.hip).
#pragma once
#include "ss_common.h"

// =================================================================================================
// LSAP on one wave — shortest augmenting path in SciPy's scan order (oracle so_lsap)
// =================================================================================================
struct LsapLds {
    int* col4row;                                // [256] result: column of every row (LDS)
};

// ---- wave-64 reductions on the DPP path (gfx9 row shifts + row broadcasts: an inclusive scan whose lane 63 holds
// the reduction; ~6 VALU steps instead of 6 LDS-crossbar shuffles) ----------------------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v, unsigned long long identity)
{
    const int lo = __builtin_amdgcn_update_dpp((int)(identity & 0xffffffffu), (int)(v & 0xffffffffu), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(identity >> 32), (int)(v >> 32), CTRL, ROW_MASK, 0xf, false);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long m)
{
    const unsigned long long ID = ~0ull;
    unsigned long long o;
    o = dpp_u64<0x111, 0xf>(m, ID); m = o < m ? o : m;          // row_shr:1
    o = dpp_u64<0x112, 0xf>(m, ID); m = o < m ? o : m;          // row_shr:2
    o = dpp_u64<0x114, 0xf>(m, ID); m = o < m ? o : m;          // row_shr:4
    o = dpp_u64<0x118, 0xf>(m, ID); m = o < m ? o : m;          // row_shr:8
    o = dpp_u64<0x142, 0xa>(m, ID); m = o < m ? o : m;          // row_bcast:15 -> rows 1,3
    o = dpp_u64<0x143, 0xc>(m, ID); m = o < m ? o : m;          // row_bcast:31 -> rows 2,3
    const int lo = __builtin_amdgcn_readlane((int)(m & 0xffffffffu), 63), hi = __builtin_amdgcn_readlane((int)(m >> 32), 63);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}

template <bool MAX>
__device__ __forceinline__ int wave_minmax_i32(int p)
{
    const int ID = MAX ? (int)0x80000000 : 0x7fffffff;
    int o;
#define SS_STEP(CTRL, RM) o = __builtin_amdgcn_update_dpp(ID, p, CTRL, RM, 0xf, false); p = MAX ? max(p, o) : min(p, o)
    SS_STEP(0x111, 0xf); SS_STEP(0x112, 0xf); SS_STEP(0x114, 0xf); SS_STEP(0x118, 0xf); SS_STEP(0x142, 0xa); SS_STEP(0x143, 0xc);
#undef SS_STEP
    return __builtin_amdgcn_readlane(p, 63);
}

// ---- register-resident form for nr <= nc <= 64 (the common case: <= 64 tracks x <= 64 detections) --------
// lane j owns column j (v, shortest path cost, path, row4col, position in SciPy's `remaining` list), lane i owns
// row i (u, col4row).  One LDS read (the cost entry) per scan step; the arg-min is a 64-bit unsigned wave-min of an
// order-preserving image of the double, ties resolved with ballots by scan position exactly as the sequential code
// does (last unassigned column among the minima, else the first minimum).
__device__ __forceinline__ unsigned long long ss_f64_key(double v)
{
    unsigned long long b = (unsigned long long)__double_as_longlong(v + 0.0);      // +0.0: -0 and +0 share a key
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ inline int lsap_wave_small(int nr, int nc, const double* cost, const LsapLds& L)
{
    const int l = threadIdx.x & 63;
    double u = 0.0, v = 0.0;
    int c4r = -1, r4c = -1, path = -1;
    const unsigned long long KINF = ss_f64_key(INFINITY);
    for (int cur = 0; cur < nr; ++cur) {
        int pos = nc - 1 - l;
        bool active = l < nc, scj = false, sr = false;
        double sp = INFINITY, minVal = 0.0;
        int num_remaining = nc, sink = -1, i = cur;
        while (sink == -1) {
            if (l == i) sr = true;
            const double ui = __longlong_as_double(((long long)__builtin_amdgcn_readlane((int)(__double_as_longlong(u) & 0xffffffff), i) & 0xffffffffll) |
                                                   ((long long)__builtin_amdgcn_readlane((int)(__double_as_longlong(u) >> 32), i) << 32));
            if (active) {
                const double r = minVal + cost[i * nc + l] - ui - v;
                if (r < sp) { path = i; sp = r; }
            }
            const unsigned long long key = active ? ss_f64_key(sp) : ~0ull;
            const unsigned long long m = wave_min_u64(key);
            if (m >= KINF) return -1;                                              // infeasible (or nothing active)
            const unsigned long long tied = __ballot(active && key == m);
            int w;
            if (__popcll(tied) == 1) w = __builtin_ctzll(tied);
            else {
                const unsigned long long tu = __ballot(active && key == m && r4c == -1);
                const bool wantmax = tu != 0ull;
                const bool insel = active && key == m && (!wantmax || r4c == -1);
                const int p0 = insel ? pos : (wantmax ? -1 : 0x3fffffff);
                const int p = wantmax ? wave_minmax_i32<true>(p0) : wave_minmax_i32<false>(p0);
                w = __builtin_ctzll(__ballot(insel && pos == p));
            }
            w = __builtin_amdgcn_readfirstlane(w);
            {
                const long long bits = __double_as_longlong(sp);
                minVal = __longlong_as_double(((long long)__builtin_amdgcn_readlane((int)(bits >> 32), w) << 32) |
                                              ((long long)__builtin_amdgcn_readlane((int)(bits & 0xffffffff), w) & 0xffffffffll));
            }
            const int rj = __builtin_amdgcn_readlane(r4c, w);
            const int pj = __builtin_amdgcn_readlane(pos, w);
            if (rj == -1) sink = w; else i = rj;
            --num_remaining;
            if (active && l != w && pos == num_remaining) pos = pj;               // remaining[index] = remaining[--n]
            if (l == w) { active = false; scj = true; }
        }
        // dual variables
        const int src = c4r >= 0 ? c4r : 0;
        const double spc = __shfl(sp, src);
        if (l == cur) u += minVal;
        else if (sr) u += minVal - spc;
        if (scj) v -= minVal - sp;
        // augment along the path (uniform walk; every step is a pair of readlanes)
        int j = sink;
        for (;;) {
            const int r = __builtin_amdgcn_readlane(path, j);
            if (l == j) r4c = r;
            const int t = __builtin_amdgcn_readlane(c4r, r);
            if (l == r) c4r = j;
            j = t;
            if (r == cur) break;
        }
    }
    if (l < nr) L.col4row[l] = c4r;
    SS_WAVE_SYNC();
    return 0;
}

// ---- register-resident form for 64 < nc <= 64*Q: lane l owns columns l, l+64, ... and rows l, l+64, ... -----------
// Same algorithm and tie rule as lsap_wave_small; indexed accesses use a uniform (lane, q) split and statically
// unrolled selects so that the per-column arrays stay in registers.
template <int Q> __device__ __forceinline__ double rl_f64(const double (&a)[Q], int idx)
{
    const int ln = idx & 63, qi = idx >> 6;
    double out = 0.0;
#pragma unroll
    for (int q = 0; q < Q; ++q)
        if (q == qi) {
            const long long b = __double_as_longlong(a[q]);
            out = __longlong_as_double(((long long)__builtin_amdgcn_readlane((int)(b >> 32), ln) << 32) |
                                       ((long long)__builtin_amdgcn_readlane((int)(b & 0xffffffff), ln) & 0xffffffffll));
        }
    return out;
}
template <int Q> __device__ __forceinline__ int rl_i32(const int (&a)[Q], int idx)
{
    const int ln = idx & 63, qi = idx >> 6;
    int out = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) if (q == qi) out = __builtin_amdgcn_readlane(a[q], ln);
    return out;
}

template <int Q>
__device__ inline int lsap_wave_regs(int nr, int nc, const double* cost, const LsapLds& L)
{
    const int l = threadIdx.x & 63;
    double u[Q], v[Q], sp[Q];
    int c4r[Q], r4c[Q], path[Q], pos[Q];
    bool active[Q], scj[Q], sr[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) { u[q] = 0.0; v[q] = 0.0; c4r[q] = -1; r4c[q] = -1; path[q] = -1; }
    const unsigned long long KINF = ss_f64_key(INFINITY);
    for (int cur = 0; cur < nr; ++cur) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int j = l + 64 * q;
            pos[q] = nc - 1 - j; active[q] = j < nc; scj[q] = false; sr[q] = false; sp[q] = INFINITY;
        }
        double minVal = 0.0;
        int num_remaining = nc, sink = -1, i = cur;
        while (sink == -1) {
#pragma unroll
            for (int q = 0; q < Q; ++q) if (l + 64 * q == i) sr[q] = true;
            const double ui = rl_f64<Q>(u, i);
            unsigned long long key[Q], kmin = ~0ull;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                if (active[q]) {
                    const double r = minVal + cost[i * nc + l + 64 * q] - ui - v[q];
                    if (r < sp[q]) { path[q] = i; sp[q] = r; }
                }
                key[q] = active[q] ? ss_f64_key(sp[q]) : ~0ull;
                kmin = key[q] < kmin ? key[q] : kmin;
            }
            const unsigned long long m = wave_min_u64(kmin);
            if (m >= KINF) return -1;
            unsigned long long tied[Q];
            int ntied = 0;
#pragma unroll
            for (int q = 0; q < Q; ++q) { tied[q] = __ballot(active[q] && key[q] == m); ntied += __popcll(tied[q]); }
            int w = 0;
            if (ntied == 1) {
#pragma unroll
                for (int q = 0; q < Q; ++q) if (tied[q]) w = 64 * q + __builtin_ctzll(tied[q]);
            } else {
                bool wantmax = false;
#pragma unroll
                for (int q = 0; q < Q; ++q) wantmax = wantmax || __ballot(active[q] && key[q] == m && r4c[q] == -1) != 0ull;
                int p0 = wantmax ? -1 : 0x3fffffff;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const bool insel = active[q] && key[q] == m && (!wantmax || r4c[q] == -1);
                    if (insel) p0 = wantmax ? max(p0, pos[q]) : min(p0, pos[q]);
                }
                const int pbest = wantmax ? wave_minmax_i32<true>(p0) : wave_minmax_i32<false>(p0);
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const bool insel = active[q] && key[q] == m && (!wantmax || r4c[q] == -1);
                    const unsigned long long b = __ballot(insel && pos[q] == pbest);
                    if (b) w = 64 * q + __builtin_ctzll(b);
                }
            }
            w = __builtin_amdgcn_readfirstlane(w);
            minVal = rl_f64<Q>(sp, w);
            const int rj = rl_i32<Q>(r4c, w);
            const int pj = rl_i32<Q>(pos, w);
            if (rj == -1) sink = w; else i = rj;
            --num_remaining;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int j = l + 64 * q;
                if (active[q] && j != w && pos[q] == num_remaining) pos[q] = pj;
                if (j == w) { active[q] = false; scj[q] = true; }
            }
        }
        // dual variables: u[r] += minVal - sp[col4row[r]] (r in SR, r != cur); v[j] -= minVal - sp[j] (j in SC)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int c = c4r[q] >= 0 ? c4r[q] : 0;
            double spc = 0.0;
#pragma unroll
            for (int qq = 0; qq < Q; ++qq) {
                const double t = __shfl(sp[qq], c & 63);
                if ((c >> 6) == qq) spc = t;
            }
            if (l + 64 * q == cur) u[q] += minVal;
            else if (sr[q]) u[q] += minVal - spc;
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) if (scj[q]) v[q] -= minVal - sp[q];
        // augment
        int j = sink;
        for (;;) {
            const int r = rl_i32<Q>(path, j);
#pragma unroll
            for (int q = 0; q < Q; ++q) if (l + 64 * q == j) r4c[q] = r;
            const int t = rl_i32<Q>(c4r, r);
#pragma unroll
            for (int q = 0; q < Q; ++q) if (l + 64 * q == r) c4r[q] = j;
            j = t;
            if (r == cur) break;
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) if (l + 64 * q < nr) L.col4row[l + 64 * q] = c4r[q];
    SS_WAVE_SYNC();
    return 0;
}

// cost: [nr][nc] (nr <= nc <= 256) in LDS or global.  Result col4row[0..nr).  Returns 0 / -1.
#ifndef SS_LSAP_WAVE_INLINE
#define SS_LSAP_WAVE_INLINE inline                // a file may ask for __noinline__ before it includes this header (ss_track.hip)
#endif
__device__ SS_LSAP_WAVE_INLINE int lsap_wave(int nr, int nc, const double* cost, const LsapLds& L)
{
    if (nc <= 64) return lsap_wave_small(nr, nc, cost, L);
    if (nc <= 128) return lsap_wave_regs<2>(nr, nc, cost, L);
    if (nc <= 256) return lsap_wave_regs<4>(nr, nc, cost, L);
    return -1;                       // callers cap both dimensions at 256 (SS_MAX_TRACKS)
}

// ---- assignment of an n_rows x n_cols matrix in its natural orientation (rows = tracks) -----------------------------------------
// SciPy transposes a tall matrix: the LSAP's rows are the smaller side.  Entry (r, c) is stored at lsap_cidx.
__device__ inline int lsap_cidx(int r, int c, int n_rows, int n_cols)
{
    return n_cols < n_rows ? c * n_rows + r : r * n_cols + c;
}

// One wave: lsap_wave of the matrix stored by lsap_cidx, then asg[row] = its column, back through the transposition (rows without
// a column keep what asg held: the caller presets -1).  Returns lsap_wave's status; asg is untouched when it is not 0.
__device__ inline int lsap_wave_assign(int n_rows, int n_cols, const double* cost, const LsapLds& L, int* asg)
{
    const int l = threadIdx.x & 63;
    const bool tr = n_cols < n_rows;
    const int nr = tr ? n_cols : n_rows, nc = tr ? n_rows : n_cols;
    const int rc = lsap_wave(nr, nc, cost, L);
    if (rc) return rc;
    for (int i = l; i < nr; i += 64) { if (tr) asg[L.col4row[i]] = i; else asg[i] = L.col4row[i]; }
    return 0;
}
