// ss_ocsort.hip — the OC-SORT tracker on the device (docs/OCSORT.md): S independent streams, a GROUP of F <= SS_FMAX frames per call.
//
//   k_ocsort_group  one workgroup (256 threads) per stream walks the group's frames in order inside the launch: score split,
//                   predict of every track (7-state SORT filter), the first association (IoU + the momentum term; upstream's
//                   shortcut when every row and track has at most one partner, else the one-wave LSAP), the optional BYTE stage
//                   on the low-score rows, the recovery stage (OCR) against the tracks' last observations, the Kalman updates
//                   with the observation-centric re-update (ORU) of a track re-found after a gap, births, the list rebuild and
//                   the output rows.  One launch per call, no host round trip: capturable.
//
// The frame procedure and its step bodies are ss_ocsort_body.h's, shared with Deep OC-SORT (csrc/ss_deepoc.hip); this kernel is the
// instantiation without the appearance and camera-motion steps.
#include "ss_ocsort_body.h"

__global__ __launch_bounds__(256) void k_ocsort_group(SSOcDev o, int F, const float* __restrict__ dets, const int* __restrict__ ndets,
                                                      float* __restrict__ out, int* __restrict__ nout)
{
    __shared__ OcLds m;
    oc_group<false>(o, nullptr, nullptr, F, dets, ndets, out, nout, m);
}

void ss_launch_ocsort_group(const SSOcDev& o, int F, const float* dets, const int* ndets, float* out, int* nout, hipStream_t st)
{
    hipLaunchKernelGGL(k_ocsort_group, dim3(o.S), dim3(256), 0, st, o, F, dets, ndets, out, nout);
}
