// Host-side launch helpers shared by mlp.hip, cross.hip and cross_lr.hip.
#pragma once

#include <hip/hip_runtime.h>

// CUs of the current device (256, the MI355X, when the query fails), asked
// once per translation unit: the row-tile rules compare block counts to it.
static inline int device_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess
            || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount,
                                     dev) != hipSuccess || n <= 0)
            n = 256;
        cus = n;
    }
    return cus;
}

// a kernel gets 64 KB of dynamic LDS by default; more has to be asked for
template <typename K>
static inline void allow_lds(K kernel, size_t bytes) {
    if (bytes > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)bytes);
}
