// ss_mot_sim.h — the box similarity of the scoring files: ss_mot.hip (HOTA, CLEAR MOT, the identity counts) and ss_ap.hip (COCO AP)
// take it from this one body.  Device code; the including file is built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

// S of docs/MOTEVAL.md section 1 by its four written steps
__device__ __forceinline__ double mot_sim(const double* __restrict__ A, const double* __restrict__ B)
{
    const double ax1 = A[0], ay1 = A[1], ax2 = A[2], ay2 = A[3], bx1 = B[0], by1 = B[1], bx2 = B[2], by2 = B[3];
    const double w = fmax(0.0, fmin(ax2, bx2) - fmax(ax1, bx1)), h = fmax(0.0, fmin(ay2, by2) - fmax(ay1, by1));
    const double inter = w * h;
    const double uni = ((ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1)) - inter;
    return inter / uni;
}
