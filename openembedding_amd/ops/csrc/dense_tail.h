// Argument block of the fused dense-parameter tail (mlp.hip: k_dense_tail),
// passed by value to the kernel. Plain types only: bindings.cpp fills it,
// mlp.hip reads it.
#pragma once

// One of w1, w2, w3: the [rows, cols] parameter lives row-major at `off` in
// the flat bf16 group; its fp32 wgrad scratch is [rows, sld] (sld = K0p for
// w1, whose columns >= cols belong to no parameter; H for w2, w3).
struct DenseTailMat {
    float* scratch;
    void* img;      // fragment-major image of W   [rows, 32 * ks]
    void* timg;     // fragment-major image of W^T [>= cols, 32 * tks]
    int off, rows, cols, sld, ks, tks;
};

struct DenseTailArgs {
    DenseTailMat m[3];
    // b1, b2, b3, w4 (H each) and b4 (1): offsets in the flat bf16 group;
    // their grads sit in bscratch [4H + 1] in this order
    int so0, so1, so2, so3, so4;
    int H;
    float* bscratch;
    // the flat bf16 group: fp32 master and state, bf16 grads and weights
    float* master;
    float* s1;
    float* s2;
    void* grad;
    void* flat;
    // the flat fp32 group (n32 may be 0)
    float* p32;
    float* s1_32;
    float* s2_32;
    float* g32;
    int n32;
    const float* sc;        // Adam's device scalars, else null
    float lr, c0, c1, c2;
};
