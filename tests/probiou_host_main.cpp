// Host build of csrc/ss_probiou.h (tests/test_obb_cpu.py).  stdin: four int64 counts (n_log, n_ang, n_exp, n_box), then n_log + n_ang +
// n_exp float64 arguments and n_box float32 boxes (cx, cy, w, h, theta).  stdout, raw float64: ss_log of each, ss_sincos of each (sine
// then cosine), ss_expneg of each, the per-box terms [n_box][6] and the n_box x n_box ProbIoU matrix.
#include <cstdio>
#include <vector>

#include "../strongsort_yolo_amd/csrc/ss_probiou.h"

template <class T> static bool rd(std::vector<T>& v, long long n)
{
    v.resize((size_t)n);
    return n == 0 || fread(v.data(), sizeof(T), (size_t)n, stdin) == (size_t)n;
}

int main()
{
    long long cnt[4];
    if (fread(cnt, sizeof cnt[0], 4, stdin) != 4) return 2;
    for (long long c : cnt) if (c < 0 || c > (1 << 24)) return 2;
    std::vector<double> lg, an, ex, out;
    std::vector<float> bx;
    if (!rd(lg, cnt[0]) || !rd(an, cnt[1]) || !rd(ex, cnt[2]) || !rd(bx, cnt[3] * 5)) return 2;
    for (double x : lg) out.push_back(ss_log(x));
    for (double t : an) { double s, c; ss_sincos(t, &s, &c); out.push_back(s); out.push_back(c); }
    for (double x : ex) out.push_back(ss_expneg(x));
    const size_t n = (size_t)cnt[3];
    std::vector<ss_pbox> pb(n);
    for (size_t i = 0; i < n; ++i) {
        const float* b = &bx[i * 5];
        pb[i] = ss_probiou_box(b[0], b[1], b[2], b[3], b[4]);
        const double t[6] = { pb[i].x, pb[i].y, pb[i].A, pb[i].B, pb[i].C, pb[i].D };
        out.insert(out.end(), t, t + 6);
    }
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j) out.push_back(ss_probiou_xywhr(&bx[i * 5], &bx[j * 5]));
    return fwrite(out.data(), sizeof(double), out.size(), stdout) == out.size() ? 0 : 1;
}
