// ss_oplaunch.h — what the launchers of the stateless operators (ss_ops.hip: f16, ss_ops32.hip: fp32) share: the status of
// a launch and the once-per-device raise of a kernel's dynamic LDS limit.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/strongsort_hip.h"

// status of the launches an entry point has just enqueued: its return value ...
static inline int op_launched() { return hipGetLastError() == hipSuccess ? SS_OK : SS_ERR_HIP; }
// ... or a check in the middle of one
#define OP_CHECK() do { if (hipGetLastError() != hipSuccess) return SS_ERR_HIP; } while (0)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies per DEVICE: `done` is a per-kernel bit set indexed by the current device
// (a process-wide bool left the second GPU of a process without the attribute: launches asking for > 64 KB of LDS failed there)
static inline bool lds_attr_once(const void* fn, unsigned long long& done, int limit_bytes)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return false;
    if (done >> dev & 1) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, limit_bytes) != hipSuccess) return false;
    done |= 1ull << dev;
    return true;
}
