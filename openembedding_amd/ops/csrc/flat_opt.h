// The flat dense optimizers' per-element update, shared by the flat kernels
// (embops.hip: k_flat_opt_f32 / k_flat_opt_bf16) and the fused dense tail
// (mlp.hip: k_dense_tail), so both run the same operations in the same
// order. Device code: include from .hip files only.
#pragma once

#include <hip/hip_runtime.h>

enum { FLAT_SGD = 0, FLAT_ADAGRAD = 1, FLAT_ADAM = 2 };

// Does the optimizer keep a first state value per element? (plain SGD has
// none and its s1 pointer is null)
template <int OPT>
__device__ __forceinline__ bool flat_opt_has_s1(float c0) {
    return OPT != FLAT_SGD || c0 != 0.0f;
}

// The update on values in registers: x1 / x2 are the element's state, read
// and written in place (x2: Adam only); sc1 / sc2 Adam's 1-b1^t, 1-b2^t.
// Semantics match torch.optim defaults (dampening 0, no weight decay /
// amsgrad).
template <int OPT>
__device__ __forceinline__ float flat_opt_math(
        float w, float gi, float& x1, float& x2, float sc1, float sc2,
        float lr, float c0, float c1, float c2) {
    if (OPT == FLAT_ADAGRAD) {
        float a = x1 + gi * gi;
        x1 = a;
        return w - lr * gi / (sqrtf(a) + c0);
    }
    if (OPT == FLAT_SGD) {
        if (c0 == 0.0f) return w - lr * gi;     // plain
        float b = c0 * x1 + gi;                 // momentum, dampening 0
        x1 = b;
        float d = (c1 != 0.0f) ? gi + c0 * b : b;   // c1 = nesterov
        return w - lr * d;
    }
    // FLAT_ADAM: c0=beta1, c1=beta2, c2=eps
    float m = c0 * x1 + (1.0f - c0) * gi;
    float v = c1 * x2 + (1.0f - c1) * gi * gi;
    x1 = m;
    x2 = v;
    float mh = m / sc1;
    float vh = v / sc2;
    return w - lr * mh / (sqrtf(vh) + c2);
}

// The same on element i of the state arrays. Adam's bias correction reads
// DEVICE scalars prepared by k_flat_step_scalars (sc[1]=1-b1^t,
// sc[2]=1-b2^t) so a hipGraph-captured step keeps correcting (a host-side
// 1-beta^t would freeze at capture).
template <int OPT>
__device__ __forceinline__ float flat_opt_step(
        float w, float gi, float* __restrict__ s1, float* __restrict__ s2,
        long i, const float* __restrict__ sc, float lr, float c0, float c1,
        float c2) {
    const bool has1 = flat_opt_has_s1<OPT>(c0);
    float x1 = has1 ? s1[i] : 0.0f;
    float x2 = OPT == FLAT_ADAM ? s2[i] : 0.0f;
    float sc1 = OPT == FLAT_ADAM ? sc[1] : 1.0f;
    float sc2 = OPT == FLAT_ADAM ? sc[2] : 1.0f;
    float r = flat_opt_math<OPT>(w, gi, x1, x2, sc1, sc2, lr, c0, c1, c2);
    if (has1) s1[i] = x1;
    if (OPT == FLAT_ADAM) s2[i] = x2;
    return r;
}
