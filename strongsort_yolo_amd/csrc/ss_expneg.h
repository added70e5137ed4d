// ss_expneg.h — exp(-x) as one fixed sequence of f64 operations, shared by the BoT-SORT keypoint term (ss_byte.hip, docs/BYTETRACK.md §1e),
// the GSI kernel (ss_gsi.hip, docs/GSI.md §2) and ProbIoU (ss_probiou.h, docs/OBB.md §1): the CPU restatements run the same sequence with
// the same constants.  A host compiler can include this header on its own.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SS_EXPNEG_FN __host__ __device__ inline
#else
#include <math.h>
#define SS_EXPNEG_FN inline
#endif

// §1e: exp(-x), x >= 0, as ONE fixed sequence of f64 operations (tests/botsort_pose_ref.ss_expneg runs the same one with the same
// constants; the file is built with -ffp-contract=off): k = floor(-x log2(e) + 1/2), r = (-x - k LN2_HI) - k LN2_LO with
// |r| <= ln2 / 2, the degree-12 Taylor polynomial by Horner, ldexp.  Above the cut-off (and for a NaN) the result is 0.
SS_EXPNEG_FN double ss_expneg(double x)
{
    if (!(x <= 700.0)) return 0.0;
    const double y = -x;
    const double k = floor(y * 0x1.71547652b82fep+0 + 0.5);
    const double r = (y - k * 0x1.62e42feep-1) - k * 0x1.a39ef35793c76p-33;
    double p = 0x1.1eed8eff8d898p-29;             // 1 / 12!
    p = p * r + 0x1.ae64567f544e4p-26;            // 1 / 11!
    p = p * r + 0x1.27e4fb7789f5cp-22;
    p = p * r + 0x1.71de3a556c734p-19;
    p = p * r + 0x1.a01a01a01a01ap-16;
    p = p * r + 0x1.a01a01a01a01ap-13;
    p = p * r + 0x1.6c16c16c16c17p-10;
    p = p * r + 0x1.1111111111111p-7;
    p = p * r + 0x1.5555555555555p-5;
    p = p * r + 0x1.5555555555555p-3;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return ldexp(p, (int)k);
}
