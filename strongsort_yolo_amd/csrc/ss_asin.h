// ss_asin.h — arcsine on [-1, 1] as one fixed sequence of float64 operations (docs/OCSORT.md, decision O-04): libm's asin and the
// device's round differently, and OC-SORT's momentum term goes into a cost that both sides must form bit for bit.
//
//   a = |c|;  a <= 0.5:  asin(a) = a p(a^2)
//             a >  0.5:  asin(a) = pi/2 - 2 x p(x^2),  x = sqrt((1 - a) / 2)          ((1 - a) and the halving are exact)
//   p: the first 22 terms of the series of asin(x) / x in x^2, (2n)! / (4^n n!^2 (2n + 1)), by Horner from the last.
//
// Every step is one multiplication or one addition, rounded once (the library is built with -ffp-contract=off; no fma here);
// sqrt is correctly rounded on both sides.  tests/ocsort_ref.py holds the same constants in the same order.  Plain C++: a host
// compiler can include this header on its own.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SS_ASIN_FN __host__ __device__ inline
#else
#define SS_ASIN_FN inline
#endif

#define SS_ASIN_TERMS 22

SS_ASIN_FN double ss_asin(double c)
{
    const double C[SS_ASIN_TERMS] = {
        1.0, 0.16666666666666666, 0.075, 0.044642857142857144, 0.030381944444444444, 0.022372159090909092,
        0.017352764423076924, 0.01396484375, 0.011551800896139705, 0.009761609529194078, 0.008390335809616815,
        0.0073125258735988454, 0.006447210311889649, 0.005740037670841924, 0.005153309682319905, 0.004660143486915096,
        0.004240907093679363, 0.003880964558837669, 0.0035692053938259347, 0.003297059503473485, 0.0030578216492580306,
        0.002846178401108942};
    const double a = fabs(c);
    const bool big = a > 0.5;
    const double x = big ? sqrt((1.0 - a) / 2.0) : a;
    const double z = x * x;
    double p = C[SS_ASIN_TERMS - 1];
#pragma unroll
    for (int k = SS_ASIN_TERMS - 2; k >= 0; --k) { p = p * z; p = p + C[k]; }
    double r = x * p;
    if (big) { r = 2.0 * r; r = 1.5707963267948966 - r; }
    return c < 0.0 ? -r : r;
}
