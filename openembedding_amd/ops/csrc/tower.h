// Argument block of the fused MLP tower (tower.hip: k_tower_fwd,
// k_tower_bwd), passed by value to the kernels. Plain types only:
// bindings.cpp fills it, tower.hip reads it.
#pragma once

#define TOWER_MAXL 4

// One GEMM stage of a launch: out [M, n] = tile [BM, 32 ks] x image^T.
// Forward, layer l: image of W_l [H_l, ceil32(H_{l-1})], vec = b_l [n],
// out = the mirror of a_l (or null). Backward, in run order l = L .. 1:
// image of W_l^T [n, ceil32(H_l)] with n = H_{l-1} (K0p for l = 1), vec =
// the mirror of a_{l-1} [M, n] that masks the stage (null for l = 1), out =
// dz_{l-1} (dx0 for l = 1). split > 1: the contraction is cut into `split`
// runs of kper k-steps (emb_tower_fwd / emb_tower_bwd set both).
struct TowerStage {
    const void* img;
    const void* vec;
    void* out;
    int n, ks, split, kper;
};

struct TowerArgs {
    TowerStage st[TOWER_MAXL];
    int L;
};
