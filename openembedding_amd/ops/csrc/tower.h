// Argument blocks of the fused MLP tower (tower.hip: k_tower_fwd,
// k_tower_bwd, k_tower_wgrad), passed by value to the kernels. Plain types only:
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

// ---- fused wgrad (k_tower_wgrad, k_tower_wgrad_fold) ---------------------
// bindings.cpp fills the pointers and the shapes, emb_tower_wgrad the rest
// (marked "launcher").

// Layer l of the wgrad: dW_l [h, jdim] = dz^T a, contracted over the rows.
// a is x0 [M, K0p] for l = 1 (jdim = K0p: the pad columns are computed and
// dropped by the fold), else the mirror of a_{l-1} [M, H_{l-1}]; both are
// dense, so jdim is the contraction operand's row stride too.
struct TowerWgradLayer {
    const void* dz;      // [M, h]
    const void* a;       // [M, jdim]
    int h, jdim;
    // launcher: row stride of the partial tile in the slab (ceil32(jdim)),
    // j-tiles, first tile of the layer in blockIdx.x, offsets of dW_l and
    // db_l in a slab
    int ldo, tj, tile0, off, boff;
};

struct TowerWgradArgs {
    TowerWgradLayer ly[TOWER_MAXL];
    const void* al;      // the mirror of a_L [M, hl]: the head's operand
    int L, M, hl;
    // launcher: 64 x 64 tiles of all layers (blockIdx.x == tiles: the head
    // role), 128-row chunks per M-slice, floats per slab, the head's offset
    int tiles, cps, per, hoff;
};

#define TOWER_FOLDN (2 * TOWER_MAXL + 2)

// One gradient of the fold, [rows, cols] dense at dst: W_1 .. W_L, b_1 ..
// b_L, w_out, b_out in this order.
struct TowerFoldOne {
    void* dst;
    int vec;             // dst is 16-byte aligned (launcher: and cols % 8 == 0)
    // launcher: offset in a slab, shape, the slab's row stride, first piece
    int src, rows, cols, ld, p0;
};

struct TowerFoldArgs {
    TowerFoldOne g[TOWER_FOLDN];
    int n, K0, accumulate;
    int S, per, pieces;  // launcher
};
