// What the fused wgrads share (mlp.hip: k_mlp3_wgrad, tower.hip:
// k_tower_wgrad): the LDS layout of a staged 128-row chunk and its
// transposed fragment read. The data path is described in mlp.hip, "fused
// wgrads": row-major staging, the row permutation inside each 32-row step,
// row stride 80, ds_read_b64_tr_b16.
#pragma once

#include <hip/hip_runtime.h>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

#define WG_KC 128           // m-chunk staged per LDS round
#define WG_LD 80            // LDS row stride (elements), see mlp.hip

// LDS row of logical chunk row r: logical row 8g + 4h + q of a 32-row step
// lives at LDS row 16h + 4g + q
static __device__ __forceinline__ int wg_lds_row(int r) {
    return (r & ~31) | ((r & 4) << 2) | ((r & 24) >> 1) | (r & 3);
}

// Transposed fragment read. Preconditions (ISA): every lane supplies an
// in-bounds 8-byte-aligned address and EXEC is all ones — call it only
// from wave-uniform control flow. T: a 2-byte element type.
template <typename T>
static __device__ __forceinline__ bf16x8 lds_tr_frag(const T* p) {
    static_assert(sizeof(T) == 2, "bf16 elements");
    union { s16x4 h[2]; bf16x8 v; } u;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) s16x4* lds_p;
    u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)p);
    u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (lds_p)(p + 16 * WG_LD));
#else
    u.h[0] = u.h[1] = s16x4{0, 0, 0, 0};
#endif
    return u.v;
}
