// Host driver of csrc/ss_kalman.h for tests/test_kalman_host_cpu.py: the thread forms of the device filter, compiled by the host
// compiler.  stdin: records of 81 doubles {op, xywh, wp, wv, mean[8], cov[64], z[4], conf}; op 0 initiate (from z), 1 predict,
// 2 project, 3 update.  stdout: per record 92 doubles {mean[8], cov[64], m4[4], S[16]} (what the op does not produce is zero).
#include <cstdio>
#include <cstring>
#include "../strongsort_yolo_amd/csrc/ss_kalman.h"

template <bool XYWH> static void run(int op, double wp, double wv, double* mean, double* cov, const double* z, double conf, double* m4, double* S)
{
    if (op == 0) ss_kf_initiate<XYWH>(z, wp, wv, mean, cov);
    else if (op == 1) ss_kf_predict<XYWH>(mean, cov, wp, wv);
    else if (op == 2) ss_kf_project<XYWH>(mean, cov, conf, wp, m4, S);
    else ss_kf_update<XYWH>(mean, cov, z, conf, wp);
}

int main()
{
    double in[81], out[92];
    while (fread(in, sizeof(double), 81, stdin) == 81) {
        memset(out, 0, sizeof out);
        memcpy(out, in + 4, 72 * sizeof(double));
        const int op = (int)in[0];
        if (op < 0 || op > 3) return 2;
        if (in[1] != 0.0) run<true>(op, in[2], in[3], out, out + 8, in + 76, in[80], out + 72, out + 76);
        else run<false>(op, in[2], in[3], out, out + 8, in + 76, in[80], out + 72, out + 76);
        if (fwrite(out, sizeof(double), 92, stdout) != 92) return 1;
    }
    return 0;
}
