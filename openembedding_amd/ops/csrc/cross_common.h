// What the two DCN-v2 cross networks, cross.hip (full-rank W_l) and
// cross_lr.hip (W_l = U_l V_l), share: the bf16 bit helpers, the staging of
// x_0 into the LDS tiles, and the BM x KSM launch.
//
// The epilogues (forward, logit head, backward initialisation, backward,
// dx0 write) are the same text in both files and stay there: moved into
// force-inlined helpers here they compile to different code (the inliner
// runs after the first scalar-replacement and CSE passes, so the kernels no
// longer see their register arrays as scalars from the start), +2 % on the
// dp = 448 forward and +1 % on the backwards at unchanged occupancy. What
// is here compiles to the instruction stream it gave in place.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

#include "launch_common.h"

typedef __hip_bfloat16 xbf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

static __device__ __forceinline__ float cross_f32(unsigned bits16) {
    return __uint_as_float(bits16 << 16);
}
static __device__ __forceinline__ unsigned cross_rne(float v) {
    return __bfloat16_as_ushort((xbf16)v);      // round to nearest even
}
static __device__ __forceinline__ void cross_unpack(uint2 p, float (&f)[4]) {
    f[0] = __uint_as_float(p.x << 16);
    f[1] = __uint_as_float(p.x & 0xffff0000u);
    f[2] = __uint_as_float(p.y << 16);
    f[3] = __uint_as_float(p.y & 0xffff0000u);
}
static __device__ __forceinline__ uint2 cross_pack(const unsigned (&h)[4]) {
    return make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
}
static __device__ __forceinline__ bf16x8 cross_frag(const uint16_t* p) {
    return *reinterpret_cast<const bf16x8*>(__builtin_assume_aligned(p, 16));
}

// The block's rows of x0 [M, dp] -> t0 (and t1): every (row < BM, k < dp) is
// written, rows >= M and the pad columns k >= d as zeros. 16-byte pieces.
template <int BM>
static __device__ __forceinline__ void cross_stage_x0(
        const uint16_t* __restrict__ x0, int m0, int M, int d, int dp,
        int LD, uint16_t* t0, uint16_t* t1) {
    const int ppr = dp >> 3;                 // pieces per row
    for (int i = threadIdx.x; i < BM * ppr; i += blockDim.x) {
        const int row = i / ppr, k = (i - row * ppr) * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        const int nv = d - k;                // valid elements of the piece
        if (m0 + row < M && nv > 0) {
            v = *reinterpret_cast<const uint4*>(__builtin_assume_aligned(
                x0 + (m0 + row) * dp + k, 16));
            if (nv < 8) {
                unsigned w[4] = {v.x, v.y, v.z, v.w};
                #pragma unroll
                for (int j = 0; j < 4; ++j)
                    w[j] = (2 * j < nv ? w[j] & 0xffffu : 0u)
                         | (2 * j + 1 < nv ? w[j] & 0xffff0000u : 0u);
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        *reinterpret_cast<uint4*>(t0 + row * LD + k) = v;
        if (t1) *reinterpret_cast<uint4*>(t1 + row * LD + k) = v;
    }
}

// kernel<BM, KSM> for the row tile bm in {16, 32} and the smallest KSM in
// {4, 8, 16} that holds ks = dp / 32 k-steps. The caller has in scope int
// bm, ks, grid, block, size_t lds and hipStream_t stream: launch configs
// are plain variables, hipify mis-rewrites anything else (docs/hacking.md).
#define CROSS_ONE(kernel, BM_, KSM_, ...)                                   \
    allow_lds(&kernel<BM_, KSM_>, lds);                                     \
    kernel<BM_, KSM_><<<grid, block, lds, stream>>>(__VA_ARGS__);

#define CROSS_LAUNCH(kernel, ...)                                           \
    do {                                                                    \
        if (bm == 16) {                                                     \
            if (ks <= 4) { CROSS_ONE(kernel, 16, 4, __VA_ARGS__) }          \
            else if (ks <= 8) { CROSS_ONE(kernel, 16, 8, __VA_ARGS__) }     \
            else { CROSS_ONE(kernel, 16, 16, __VA_ARGS__) }                 \
        } else {                                                            \
            if (ks <= 4) { CROSS_ONE(kernel, 32, 4, __VA_ARGS__) }          \
            else if (ks <= 8) { CROSS_ONE(kernel, 32, 8, __VA_ARGS__) }     \
            else { CROSS_ONE(kernel, 32, 16, __VA_ARGS__) }                 \
        }                                                                   \
    } while (0)
