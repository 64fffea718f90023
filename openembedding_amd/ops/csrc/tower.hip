// Fused MLP tower (gfx950 / MI355X): 1 <= L <= 4 hidden layers of unequal
// widths H_1 .. H_L (H_0 = K0) and the logit head,
//   a_l = relu(W_l a_{l-1} + b_l)      out = w_out . a_L + b_out (+ partial)
// forward and the dgrad chain of the backward, ONE launch each, every layer
// inside the kernel. mlp.hip serves the one shape H x 3 (H <= 416) with its
// fused wgrad and dense tail; everything else that fits the limits below
// comes here: H_l % 16 == 0, 16 <= H_l <= 512, K0p = ceil32(K0) <= 512.
//
// Operands are bf16, every sum and product is fp32 (mfma_f32_16x16x32_bf16,
// -ffp-contract=off), values are rounded to bf16 (nearest even) exactly
// where they are written below.
//
// Forward, per row and layer l = 1 .. L:
//   acc[o] = sum_k W_l[o,k] a_{l-1}[k]     over the 32-padded k
//   t = acc + b_l[o]                       a_l[o] = bf16(max(t, 0))
//   a_l is mirrored to HBM as [M, H_l] when a backward follows
//   out = sum_k a_L[k] w_out[k], + b_out, + partial
// Backward:
//   dz_L[o] = bf16(dout * w_out[o]) where a_L[o] > 0, else 0
//   for l = L .. 2:  dz_{l-1}[k] = bf16(sum_o dz_l[o] W_l[o,k])
//                                   where a_{l-1}[k] > 0, else 0
//   dx0[k] = bf16(sum_o dz_1[o] W_1[o,k])   as [M, K0p], pad columns 0
//   dz_1 .. dz_L are mirrored to HBM as [M, H_l]
// No atomics: each element is written once, in one fixed order of sums, so
// both kernels are bitwise reproducible. dW_l = dz_l^T a_{l-1}, db_l =
// sum_m dz_l and the head's gradients come from the mirrors in one more
// launch and a fold (k_tower_wgrad, k_tower_wgrad_fold, below), again without
// atomics; ops/dispatch.py keeps library ops for a partly frozen tower.
//
// Both directions are chains of the same stage, out [BM, n] = tile [BM, 32
// ks] x image^T: the forward with the images of W_l and the bias + ReLU
// epilogue, the backward with the images of W_l^T and the mask epilogue (the
// last stage, dx0, unmasked). n and ks are run-time values of a by-value
// table (tower.h).
//
// Work split: a block of 8 waves owns BM in {16, 32} consecutive rows for
// all layers. Two LDS tiles [BM][512 + 8] bf16 swap roles per stage; the
// stride is 16 j + 4 dwords (cross.hip: the 16 rows of a fragment read start
// on 16 distinct 4-bank groups). x0's rows are staged by cross_stage_x0
// (rows >= M and the pad columns as zeros); each stage writes columns
// 0 .. ceil32(n) of every row of the other tile - the 16 columns behind an
// n that is no multiple of 32 as zeros, by the wave that owns the last
// chunk - before the barrier that lets the next stage read them. No element
// a fragment reads is ever uninitialised LDS (0 * inf = NaN: docs/kernels.md,
// mlp.hip).
//
// Weights stream through L2 as fragment-major images (k_mlp3_pack_frag):
// a 16-column chunk is one run of ks KB. A wave takes chunks wave, wave + 8,
// .. (the index through readfirstlane), double-buffered in registers; bias
// and mask are loaded BEFORE the next chunk's prefetch is issued, and a
// stage's first chunk before the barrier that ends the previous stage. The
// weight fragment is MFMA operand A and the activation fragment operand B
// (cross.hip's transposed-accumulator map): a lane holds out columns
// o0 .. o0+3 of ONE row and writes LDS and HBM in 8-byte pieces; the mask is
// 8 bytes of the a_{l-1} mirror. The activation fragments of a row tile
// live in registers for a stage while RT * KSM <= 16 and KSM < 16 (BM = 16
// at KSM = 16 would spill beside the 128 VGPRs of the two weight buffers),
// else they are re-read from the tile per chunk (conflict-free).
//
// Narrow stages: with n < 128 there are fewer chunks than waves. While
// n <= 64 and ks >= 2 the contraction is cut into W = min(8 / (n/16), ks)
// runs of kper = ceil(ks / W) k-steps (W = ceil(ks / kper) after that, so no
// run is empty); wave = g * (n/16) + c takes chunk c, run g, and leaves its
// fp32 accumulators in LDS [W][BM][n + 4]. After one barrier the waves share
// the (row tile, chunk) pairs, sum the W partials in the fixed order
// ((p0 + p1) + p2) + .., and run the epilogue once (cross_lr.hip's down
// GEMM). 80 <= n <= 112 stays unsplit with 1 to 3 waves idle in that stage.

#include "cross_common.h"
#include "tower.h"
#include "wgrad_common.h"

#define TW_WAVES 8
#define TW_LD 520            // a tile row: 512 + 8 bf16
#define TW_NIT 4             // chunks of a wave at most: 512 / 16 / 8
#define TW_PROW 160          // floats of partials per row: W (n + 4) at most

// the lane's pieces of chunk c (wave-uniform), k-steps s0 <= s < s1
template <int KSM>
static __device__ __forceinline__ void tower_ld_w(bf16x8 (&b)[KSM],
                                                  const uint16_t* img, int c,
                                                  int ks, int s0, int s1,
                                                  int lane) {
    const uint16_t* pb = img + __builtin_amdgcn_readfirstlane(c) * (ks * 512)
                             + (unsigned)(lane * 8);
    #pragma unroll
    for (int s = 0; s < KSM; ++s)
        if (s >= s0 && s < s1) b[s] = cross_frag(pb + 512 * s);
}

// activation fragments of one row tile, from an LDS tile
template <int KSM>
static __device__ __forceinline__ void tower_ld_a(bf16x8 (&a)[KSM],
                                                  const uint16_t* tile, int rt,
                                                  int s0, int s1, int lane) {
    const uint16_t* pa = tile + (rt * 16 + (lane & 15)) * TW_LD
                              + (lane >> 4) * 8;
    #pragma unroll
    for (int s = 0; s < KSM; ++s)
        if (s >= s0 && s < s1) a[s] = cross_frag(pa + 32 * s);
}

// acc[r] = sum_{32 s0 <= k < 32 s1} W[o0 + r][k] * A[row][k]
template <int KSM, bool AREG>
static __device__ __forceinline__ f32x4 tower_mma(const bf16x8 (&b)[KSM],
                                                  const bf16x8 (&a)[KSM],
                                                  const uint16_t* tile, int rt,
                                                  int s0, int s1, int lane) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const uint16_t* pa = tile + (rt * 16 + (lane & 15)) * TW_LD
                              + (lane >> 4) * 8;
    #pragma unroll
    for (int s = 0; s < KSM; ++s)
        if (s >= s0 && s < s1)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                b[s], AREG ? a[s] : cross_frag(pa + 32 * s), acc, 0, 0, 0);
    return acc;
}

// What a lane does with its four columns o0 .. o0+3 of row `row`. FWD: bv =
// the bias; else mk = the mask's 8 bytes (masked) or nothing. zpad: the
// chunk is the last of an n that is no multiple of 32.
template <bool FWD>
static __device__ __forceinline__ void tower_epilogue(
        const f32x4 acc, const unsigned (&bv)[4], uint2 mk, bool masked,
        uint16_t* nxt, uint16_t* __restrict__ out, int n, int row, int o0,
        int gm, int M, bool zpad) {
    unsigned h[4];
    if (FWD) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float t = acc[r] + cross_f32(bv[r]);
            h[r] = cross_rne(t > 0.f ? t : 0.f);
        }
    } else {
        float mv[4];
        cross_unpack(mk, mv);
        #pragma unroll
        for (int r = 0; r < 4; ++r)
            h[r] = !masked || mv[r] > 0.f ? cross_rne(acc[r]) : 0u;
    }
    const uint2 pk = cross_pack(h);
    const int at = row * TW_LD + o0;
    *reinterpret_cast<uint2*>(nxt + at) = pk;
    if (zpad) *reinterpret_cast<uint2*>(nxt + at + 16) = make_uint2(0u, 0u);
    if (out && gm < M) *reinterpret_cast<uint2*>(out + gm * n + o0) = pk;
}

// One stage for the block's rows: reads tile `cur` (complete after the
// barrier inside), writes tile `nxt` and the stage's HBM output.
template <int BM, int KSM, bool FWD>
static __device__ __forceinline__ void tower_stage(
        const TowerStage st, const uint16_t* cur, uint16_t* nxt, float* part,
        int m0, int M, int wave, int lane) {
    constexpr int RT = BM / 16;
    constexpr bool AREG = RT * KSM <= 16 && KSM < 16;
    const uint16_t* const img = static_cast<const uint16_t*>(st.img);
    const uint16_t* const vec = static_cast<const uint16_t*>(st.vec);
    uint16_t* const out = static_cast<uint16_t*>(st.out);
    const int n = st.n, ks = st.ks, nch = n >> 4, split = st.split;
    const bool odd = (n & 16) != 0;
    const int rl = lane & 15, g4 = lane >> 4;

    // the wave's first chunk and its run of k-steps
    int c0 = wave, g = 0, s0 = 0, s1 = ks;
    if (split > 1) {
        while (c0 >= nch) { c0 -= nch; ++g; }
        s0 = g * st.kper;
        s1 = s0 + st.kper < ks ? s0 + st.kper : ks;
        if (g >= split) c0 = nch;            // no run left for this wave
    }
    bf16x8 bb[2][KSM];
    if (c0 < nch) tower_ld_w<KSM>(bb[0], img, c0, ks, s0, s1, lane);
    __syncthreads();          // `cur` is complete, old partials are consumed
    bf16x8 af[AREG ? RT : 1][KSM];
    if (AREG) {
        #pragma unroll
        for (int rt = 0; rt < RT; ++rt)
            tower_ld_a<KSM>(af[AREG ? rt : 0], cur, rt, s0, s1, lane);
    }

    if (split > 1) {
        const int pn = n + 4;                // floats per row of one partial
        if (c0 < nch) {
            #pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const f32x4 acc = tower_mma<KSM, AREG>(
                    bb[0], af[AREG ? rt : 0], cur, rt, s0, s1, lane);
                *reinterpret_cast<f32x4*>(
                    part + (g * BM + rt * 16 + rl) * pn + c0 * 16 + g4 * 4)
                    = acc;
            }
        }
        __syncthreads();      // the partials are complete
        for (int p = wave; p < RT * nch; p += TW_WAVES) {
            const int rt = p % RT, c = p / RT;
            const int row = rt * 16 + rl, gm = m0 + row, o0 = c * 16 + g4 * 4;
            unsigned bv[4] = {0u, 0u, 0u, 0u};
            uint2 mk = make_uint2(0u, 0u);
            if (FWD) {
                #pragma unroll
                for (int r = 0; r < 4; ++r) bv[r] = vec[o0 + r];
            } else if (vec && gm < M) {
                mk = *reinterpret_cast<const uint2*>(vec + gm * n + o0);
            }
            const float* pp = part + row * pn + o0;
            f32x4 acc = *reinterpret_cast<const f32x4*>(pp);
            for (int w = 1; w < split; ++w)
                acc = acc + *reinterpret_cast<const f32x4*>(pp + w * BM * pn);
            tower_epilogue<FWD>(acc, bv, mk, vec != nullptr, nxt, out, n,
                                row, o0, gm, M, odd && c == nch - 1);
        }
        return;
    }

    #pragma unroll
    for (int it = 0; it < TW_NIT; ++it) {
        const int c = wave + TW_WAVES * it;
        if (c < nch) {
            const int o0 = c * 16 + g4 * 4;
            unsigned bv[4] = {0u, 0u, 0u, 0u};
            uint2 mk[RT];
            #pragma unroll
            for (int rt = 0; rt < RT; ++rt) mk[rt] = make_uint2(0u, 0u);
            if (FWD) {
                #pragma unroll
                for (int r = 0; r < 4; ++r) bv[r] = vec[o0 + r];
            } else if (vec) {
                #pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const int gm = m0 + rt * 16 + rl;
                    if (gm < M)
                        mk[rt] = *reinterpret_cast<const uint2*>(
                            vec + gm * n + o0);
                }
            }
            if (it + 1 < TW_NIT && c + TW_WAVES < nch)
                tower_ld_w<KSM>(bb[(it + 1) & 1], img, c + TW_WAVES, ks, 0,
                                ks, lane);
            #pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const f32x4 acc = tower_mma<KSM, AREG>(
                    bb[it & 1], af[AREG ? rt : 0], cur, rt, 0, ks, lane);
                const int row = rt * 16 + rl;
                tower_epilogue<FWD>(acc, bv, mk[rt],
                                    vec != nullptr, nxt, out, n, row, o0,
                                    m0 + row, M, odd && c == nch - 1);
            }
        }
    }
}

// ---- forward ----------------------------------------------------------
template <int BM, int KSM>
__global__ __launch_bounds__(64 * TW_WAVES)
void k_tower_fwd(const TowerArgs a,
                 const uint16_t* __restrict__ x0,     // [M, K0p]
                 int M, int K0, int K0p,
                 const uint16_t* __restrict__ w_out,  // [H_L]
                 const uint16_t* __restrict__ b_out,  // [1]
                 const float* __restrict__ partial,   // [M] or null
                 float* __restrict__ outv) {          // [M]
    extern __shared__ uint4 tower_smem[];
    uint16_t* cur = reinterpret_cast<uint16_t*>(tower_smem);
    uint16_t* nxt = cur + BM * TW_LD;
    float* const part = reinterpret_cast<float*>(nxt + BM * TW_LD);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m0 = (int)blockIdx.x * BM;

    cross_stage_x0<BM>(x0, m0, M, K0, K0p, TW_LD, cur, nullptr);

    for (int l = 0; l < a.L; ++l) {
        tower_stage<BM, KSM, true>(a.st[l], cur, nxt, part, m0, M, wave,
                                   lane);
        uint16_t* const sw = cur;
        cur = nxt;
        nxt = sw;
    }

    // out[row] = <w_out, a_L[row]>: a wave per row, lanes stride the columns,
    // then a shuffle tree - a fixed order (k_mlp3_fwd's form)
    const int nl = a.st[a.L - 1].n;
    __syncthreads();
    for (int row = wave; row < BM && m0 + row < M; row += TW_WAVES) {
        float s = 0.f;
        for (int k = lane; k < nl; k += 64)
            s += cross_f32(cur[row * TW_LD + k]) * cross_f32(w_out[k]);
        #pragma unroll
        for (int off = 32; off; off >>= 1)
            s += __shfl_down(s, off, 64);
        if (lane == 0) {
            float v = s + cross_f32(b_out[0]);
            if (partial) v = v + partial[m0 + row];
            outv[m0 + row] = v;
        }
    }
}

// ---- backward ---------------------------------------------------------
// a.st in run order (l = L .. 1, tower.h). al, dzl: the mirrors of a_L and
// dz_L, [M, nl].
template <int BM, int KSM>
__global__ __launch_bounds__(64 * TW_WAVES)
void k_tower_bwd(const TowerArgs a,
                 const float* __restrict__ dout,      // [M]
                 const uint16_t* __restrict__ w_out,  // [nl]
                 const uint16_t* __restrict__ al,
                 uint16_t* __restrict__ dzl, int nl, int M) {
    constexpr int RT = BM / 16;
    extern __shared__ uint4 tower_smem[];
    uint16_t* cur = reinterpret_cast<uint16_t*>(tower_smem);
    uint16_t* nxt = cur + BM * TW_LD;
    float* const part = reinterpret_cast<float*>(nxt + BM * TW_LD);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m0 = (int)blockIdx.x * BM;
    const int rl = lane & 15, g4 = lane >> 4;

    // dz_L into `cur`, the waves sharing the (row tile, chunk) pairs
    const int nchl = nl >> 4;
    for (int p = wave; p < RT * nchl; p += TW_WAVES) {
        const int rt = p % RT, c = p / RT;
        const int row = rt * 16 + rl, gm = m0 + row, o0 = c * 16 + g4 * 4;
        unsigned h[4] = {0u, 0u, 0u, 0u};
        if (gm < M) {
            const float dv = dout[gm];
            float av[4];
            cross_unpack(*reinterpret_cast<const uint2*>(al + gm * nl + o0),
                         av);
            #pragma unroll
            for (int r = 0; r < 4; ++r)
                if (av[r] > 0.f)
                    h[r] = cross_rne(dv * cross_f32(w_out[o0 + r]));
        }
        const uint2 pk = cross_pack(h);
        const int at = row * TW_LD + o0;
        *reinterpret_cast<uint2*>(cur + at) = pk;
        if ((nl & 16) && c == nchl - 1)
            *reinterpret_cast<uint2*>(cur + at + 16) = make_uint2(0u, 0u);
        if (gm < M) *reinterpret_cast<uint2*>(dzl + gm * nl + o0) = pk;
    }

    for (int i = 0; i < a.L; ++i) {
        tower_stage<BM, KSM, false>(a.st[i], cur, nxt, part, m0, M, wave,
                                    lane);
        uint16_t* const sw = cur;
        cur = nxt;
        nxt = sw;
    }
}

// ---- wgrad ------------------------------------------------------------
// Every parameter gradient of the tower from the mirrors, two launches:
//   dW_l[i,j] = sum_m dz_l[m,i] a_{l-1}[m,j]      db_l[i] = sum_m dz_l[m,i]
//   dw_out[k] = sum_m dout[m] a_L[m,k]            db_out  = sum_m dout[m]
// (a_0 = x0; fp32 products and sums, the head's product rounded once), then
// grad = bf16(float(base) + s) or bf16(s): one rounding per gradient.
//
// k_tower_wgrad: grid (tiles + 1, S). blockIdx.x walks the 64 x 64 output
// tiles of all layers (a layer narrower than 64 is one partial tile),
// blockIdx.y is the M-slice, `cps` whole 128-row chunks. The data path is
// k_mlp3_wgrad's (wgrad_common.h): both operands staged row-major with
// 16-byte loads, rows permuted inside each 32-row step, transposed fragment
// reads, the next chunk's loads in flight under the MFMAs. Wave w owns
// subtiles {w, w + 8} of the 4 x 4 grid of 16 x 16; a subtile that lies
// outside the matrix is skipped (wave-uniform). Blocks with tj == 0 also sum
// the columns of the dz tile they staged (db_l). The block with blockIdx.x
// == tiles is the slice's head role. Everything lands in the slice's slab of
// the scratch with plain stores, each element written by one thread: no
// atomics and nothing to zero. k_tower_wgrad_fold sums the slabs in the order
// ((p0 + p1) + p2) + .. and rounds, so a tower's wgrad is bitwise
// reproducible like its forward and backward.

// The head role: column sums of dout[m] * a_L[m, :] and sum dout over the
// slice. Thread (r, c) takes columns 8c .. 8c+7 of rows mbeg + r, + rg, ..;
// the rg row groups meet in LDS [rg][hl + 1] and are added r = 0, 1, ...
static __device__ __forceinline__ void tower_wgrad_head(
        const uint16_t* __restrict__ al, const float* __restrict__ dout,
        int hl, int mbeg, int mend, float* red, float* __restrict__ out) {
    const int cg = hl >> 3;
    int rg = 512 / cg;                   // rg (hl + 1) <= 4160 floats of LDS
    if (rg > 64) rg = 64;
    const int t = threadIdx.x, r = t / cg, c = t - r * cg;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ds = 0.f;
    if (r < rg) {
        for (int m = mbeg + r; m < mend; m += rg) {
            const float dv = dout[m];
            const uint4 v = *reinterpret_cast<const uint4*>(
                __builtin_assume_aligned(al + m * hl + 8 * c, 16));
            float lo[4], hi[4];
            cross_unpack(make_uint2(v.x, v.y), lo);
            cross_unpack(make_uint2(v.z, v.w), hi);
            #pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[e] = acc[e] + dv * lo[e];
                acc[4 + e] = acc[4 + e] + dv * hi[e];
            }
            ds = ds + dv;
        }
        float* const pr = red + r * (hl + 1);
        #pragma unroll
        for (int e = 0; e < 8; ++e) pr[8 * c + e] = acc[e];
        if (c == 0) pr[hl] = ds;
    }
    __syncthreads();
    for (int k = t; k <= hl; k += 512) {
        float s = red[k];
        for (int q = 1; q < rg; ++q) s = s + red[q * (hl + 1) + k];
        out[k] = s;
    }
}

__global__ __launch_bounds__(512, 2)
void k_tower_wgrad(const TowerWgradArgs a,
                   const float* __restrict__ dout,      // [M]
                   float* __restrict__ scratch) {       // [S][per]
    __shared__ __attribute__((aligned(16))) uint16_t lds[2 * WG_KC * WG_LD];
    uint16_t* const ldsA = lds;
    uint16_t* const ldsB = lds + WG_KC * WG_LD;
    const int bt = (int)blockIdx.x;
    const int mbeg = (int)blockIdx.y * a.cps * WG_KC;
    const int mend = mbeg + a.cps * WG_KC < a.M ? mbeg + a.cps * WG_KC : a.M;
    float* const slab = scratch + (size_t)blockIdx.y * a.per;

    if (bt == a.tiles) {                 // block-uniform
        tower_wgrad_head(static_cast<const uint16_t*>(a.al), dout, a.hl,
                         mbeg, mend, reinterpret_cast<float*>(lds),
                         slab + a.hoff);
        return;
    }

    // block -> (layer, i-tile, j-tile)
    TowerWgradLayer ly = a.ly[0];
    #pragma unroll
    for (int l = 1; l < TOWER_MAXL; ++l)
        if (l < a.L && bt >= a.ly[l].tile0) ly = a.ly[l];
    const int h = ly.h, jdim = ly.jdim;
    const int ti = (bt - ly.tile0) / ly.tj, tj = bt - ly.tile0 - ti * ly.tj;
    const int i0 = ti * 64, j0 = tj * 64;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));

    // staging: thread t owns piece (t & 7) of rows (t >> 3) and (t >> 3) + 64
    // of both operands. h and jdim are multiples of 16, so a 16-byte piece is
    // inside or outside the matrix; outside pieces and rows >= mend are
    // zeros, never read from memory.
    const int srow = (int)threadIdx.x >> 3, scol = ((int)threadIdx.x & 7) * 8;
    const bool okA = i0 + scol < h, okB = j0 + scol < jdim;
    const uint16_t* gA = static_cast<const uint16_t*>(ly.dz) + i0 + scol;
    const uint16_t* gB = static_cast<const uint16_t*>(ly.a) + j0 + scol;
    uint4 ra[2], rb[2];
    auto load_chunk = [&](int m0) {
        #pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int m = m0 + srow + 64 * p;
            ra[p] = make_uint4(0u, 0u, 0u, 0u);
            rb[p] = make_uint4(0u, 0u, 0u, 0u);
            if (m < mend) {
                if (okA)
                    ra[p] = *reinterpret_cast<const uint4*>(
                        __builtin_assume_aligned(gA + m * h, 16));
                if (okB)
                    rb[p] = *reinterpret_cast<const uint4*>(
                        __builtin_assume_aligned(gB + m * jdim, 16));
            }
        }
    };

    f32x4 acc[2];
    acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int si = (wave >> 2) * 16, sj = (wave & 3) * 16;
    // the wave's subtiles that hold any element of dW_l (wave-uniform)
    const bool do0 = i0 + si < h && j0 + sj < jdim;
    const bool do1 = do0 && i0 + si + 32 < h;
    // lane 4q+p of a 16-lane group g addresses LDS row 4g+q, columns 4p..4p+3
    const int toff = (4 * (lane >> 4) + ((lane & 15) >> 2)) * WG_LD
                   + 4 * (lane & 3);
    const bool rider = tj == 0;          // block-uniform
    float bsum = 0.f;

    load_chunk(mbeg);
    for (int m0 = mbeg; m0 < mend; m0 += WG_KC) {
        __syncthreads();                 // the previous chunk's reads are done
        #pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int o = wg_lds_row(srow + 64 * p) * WG_LD + scol;
            *reinterpret_cast<uint4*>(ldsA + o) = ra[p];
            *reinterpret_cast<uint4*>(ldsB + o) = rb[p];
        }
        __syncthreads();
        if (m0 + WG_KC < mend) load_chunk(m0 + WG_KC);
        if (rider) {
            // db_l rides along (k_mlp3_wgrad's rider): 8 threads per column,
            // each every 8th row, a shuffle tree inside the 8-lane group,
            // then chunk by chunk - a fixed order. Zeros were staged beyond
            // mend and h.
            const int cc = (int)threadIdx.x >> 3, sub = (int)threadIdx.x & 7;
            float s = 0.f;
            for (int mm = sub; mm < WG_KC; mm += 8)
                s += cross_f32(ldsA[wg_lds_row(mm) * WG_LD + cc]);
            s += __shfl_down(s, 4);
            s += __shfl_down(s, 2);
            s += __shfl_down(s, 1);
            bsum = bsum + s;
        }
        if (do0) {
            #pragma unroll
            for (int ks = 0; ks < WG_KC; ks += 32) {
                const bf16x8 bv = lds_tr_frag(ldsB + ks * WG_LD + toff + sj);
                const bf16x8 a0 = lds_tr_frag(ldsA + ks * WG_LD + toff + si);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    a0, bv, acc[0], 0, 0, 0);
                if (do1) {
                    const bf16x8 a1 = lds_tr_frag(ldsA + ks * WG_LD + toff
                                                  + si + 32);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a1, bv, acc[1], 0, 0, 0);
                }
            }
        }
    }
    if (rider) {
        const int cc = (int)threadIdx.x >> 3;
        if ((threadIdx.x & 7) == 0 && i0 + cc < h)
            slab[ly.boff + i0 + cc] = bsum;
    }
    // C row = the A operand's column i, C column = j
    float* const out = slab + ly.off;
    const int j = j0 + sj + (lane & 15);
    #pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int i = i0 + si + 32 * t + (lane >> 4) * 4;
        #pragma unroll
        for (int r = 0; r < 4; ++r)
            if (j < jdim && i + r < h) out[(i + r) * ly.ldo + j] = acc[t][r];
    }
}

// One thread per piece of 8 consecutive columns of one gradient row: the S
// partials in slab order, one rounding, 16-byte loads and stores where the
// gradient allows them (vec), else element by element with 2-byte stores
// (dW_1 with an odd K0, b_out). Columns at and beyond `cols` of a slab row,
// x0's pad columns, are not read.
__global__ __launch_bounds__(256)
void k_tower_wgrad_fold(const TowerFoldArgs f,
                        const float* __restrict__ scratch) {
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (p >= f.pieces) return;
    TowerFoldOne g = f.g[0];
    #pragma unroll
    for (int i = 1; i < TOWER_FOLDN; ++i)
        if (i < f.n && p >= f.g[i].p0) g = f.g[i];
    const int ppr = (g.cols + 7) >> 3;
    const int q = p - g.p0, row = q / ppr, col = (q - row * ppr) * 8;
    const float* src = scratch + g.src + row * g.ld + col;
    uint16_t* dst = static_cast<uint16_t*>(g.dst) + row * g.cols + col;
    const int nv = g.cols - col < 8 ? g.cols - col : 8;
    if (g.vec) {
        f32x4 s0 = *reinterpret_cast<const f32x4*>(src);
        f32x4 s1 = *reinterpret_cast<const f32x4*>(src + 4);
        for (int s = 1; s < f.S; ++s) {
            const float* ps = src + (size_t)s * f.per;
            s0 = s0 + *reinterpret_cast<const f32x4*>(ps);
            s1 = s1 + *reinterpret_cast<const f32x4*>(ps + 4);
        }
        if (f.accumulate) {
            const uint4 b = *reinterpret_cast<const uint4*>(dst);
            float lo[4], hi[4];
            cross_unpack(make_uint2(b.x, b.y), lo);
            cross_unpack(make_uint2(b.z, b.w), hi);
            #pragma unroll
            for (int e = 0; e < 4; ++e) {
                s0[e] = lo[e] + s0[e];
                s1[e] = hi[e] + s1[e];
            }
        }
        unsigned h0[4], h1[4];
        #pragma unroll
        for (int e = 0; e < 4; ++e) {
            h0[e] = cross_rne(s0[e]);
            h1[e] = cross_rne(s1[e]);
        }
        const uint2 lo2 = cross_pack(h0), hi2 = cross_pack(h1);
        *reinterpret_cast<uint4*>(dst) = make_uint4(lo2.x, lo2.y, hi2.x,
                                                    hi2.y);
        return;
    }
    for (int e = 0; e < nv; ++e) {
        float s = src[e];
        for (int k = 1; k < f.S; ++k) s = s + src[(size_t)k * f.per + e];
        if (f.accumulate) s = cross_f32(dst[e]) + s;
        dst[e] = (uint16_t)cross_rne(s);
    }
}

// ---- launchers --------------------------------------------------------

// Rows per block. As in cross.hip a block streams every weight image
// whatever BM is, so BM = 32 halves the bytes streamed per row and the
// number of blocks: cross_pick_bm's rule, 16 while ceil(M / 16) <= CUs, else
// 32 (docs/kernels.md, tower.hip, for what was measured).
static int tower_pick_bm(long M, int bm) {
    if (bm == 16 || bm == 32) return bm;
    return (M + 15) / 16 <= device_cus() ? 16 : 32;
}

// two tiles and the partials: 43,520 bytes at BM = 16, 87,040 at BM = 32,
// past the 64 KB a kernel gets by default (allow_lds)
static size_t tower_lds(int bm) {
    return (size_t)bm * (2 * TW_LD * 2 + TW_PROW * 4);
}

// the k-split of a narrow stage (head of the file)
static void tower_set_split(TowerStage* st) {
    const int nch = st->n / 16;
    int w = nch < TW_WAVES ? TW_WAVES / nch : 1;
    if (w > st->ks) w = st->ks;
    st->kper = (st->ks + w - 1) / w;
    st->split = (st->ks + st->kper - 1) / st->kper;
}

static int tower_prepare(TowerArgs* a) {
    int ks = 1;
    for (int i = 0; i < a->L; ++i) {
        tower_set_split(&a->st[i]);
        if (a->st[i].ks > ks) ks = a->st[i].ks;
    }
    return ks;
}

extern "C" {

// The shapes the kernels take; the bindings refuse everything else. h: the
// L hidden widths.
int emb_tower_fits(long M, long K0, long K0p, long L, const long* h) {
    if (!(K0 >= 1 && K0p == (K0 + 31) / 32 * 32 && K0p <= 512 && L >= 1
          && L <= TOWER_MAXL && M >= 0 && M * 512 * (L + 1) < (1L << 31)))
        return 0;
    for (long l = 0; l < L; ++l)
        if (h[l] % 16 != 0 || h[l] < 16 || h[l] > 512) return 0;
    return 1;
}

int emb_tower_bm(long M, int bm) { return tower_pick_bm(M, bm); }

// the k-split the launchers give a stage of n columns over ks k-steps
int emb_tower_split(int n, int ks) {
    TowerStage st = {nullptr, nullptr, nullptr, n, ks, 1, ks};
    tower_set_split(&st);
    return st.split;
}

void emb_tower_fwd(const TowerArgs* args, const void* x0, long M, long K0,
                   long K0p, const void* w_out, const void* b_out,
                   const float* partial, float* out, int bm,
                   hipStream_t stream) {
    if (M == 0) return;
    TowerArgs a = *args;
    const int ks = tower_prepare(&a);
    bm = tower_pick_bm(M, bm);
    const size_t lds = tower_lds(bm);
    const int grid = (int)((M + bm - 1) / bm), block = 64 * TW_WAVES;
    CROSS_LAUNCH(k_tower_fwd, a, (const uint16_t*)x0, (int)M, (int)K0,
                 (int)K0p, (const uint16_t*)w_out, (const uint16_t*)b_out,
                 partial, out);
}

void emb_tower_bwd(const TowerArgs* args, const float* dout,
                   const void* w_out, const void* al, void* dzl, long nl,
                   long M, int bm, hipStream_t stream) {
    if (M == 0) return;
    TowerArgs a = *args;
    const int ks = tower_prepare(&a);
    bm = tower_pick_bm(M, bm);
    const size_t lds = tower_lds(bm);
    const int grid = (int)((M + bm - 1) / bm), block = 64 * TW_WAVES;
    CROSS_LAUNCH(k_tower_bwd, a, dout, (const uint16_t*)w_out,
                 (const uint16_t*)al, (uint16_t*)dzl, (int)nl, (int)M);
}

}  // extern "C"

// The wgrad's tables: tiles, slab offsets and the M-slices. S (m_split; 0 =
// the rule) is a function of M and the widths alone, not of the device, so
// the bits of a gradient do not change between machines. Slices are whole
// 128-row chunks, `cps` each; S is then ceil(chunks / cps), so no slice is
// empty and the fold reads only what this launch wrote.
// The rule: enough slices that tiles x S fills 256 CUs twice (2 blocks fit
// a CU; the WDL tower over K0p = 256 has 32 + 32 + 8 + 2 = 74 tiles and gets
// 7, (256, 128, 64) has 26), at most 8, and at least 4 chunks a slice. The
// last two come from the table: measured on an MI355X, us for this kernel +
// its fold (scripts/bench_tower.py --sweep, K0 = 247, median of 7 blocks of
// 200; the blocks of a figure differ by at most 0.5), with the first form of
// the rule (fill twice, at most 16) in the last column and its S:
//   M     widths           S = 1     2      4      8     16    first rule
//   1024  512-256-128-32   22.8   16.3   16.7   22.1   22.0*   16.7 (4)
//   1024  256-128-64       22.4   15.8   14.9   18.3   18.3*   18.3 (8)
//   2048  512-256-128-32   37.7   23.8   20.7   23.9   33.8    21.9 (6)
//   2048  256-128-64       37.3   23.1   18.5   20.1   29.4    29.4 (16)
//   4096  512-256-128-32   67.3   38.6   29.9   30.0   37.7    28.9 (7)
//   4096  256-128-64       66.8   38.0   26.0   23.7   31.2    31.2 (16)
//   8192  512-256-128-32  126.6   68.2   47.3   41.2   48.5    41.0 (7)
//   8192  256-128-64      125.9   67.5   40.6   31.0   35.8    35.9 (16)
// (* M = 1024 has 8 chunks, so 16 is 8.) 16 slices lose everywhere - the
// fold reads every slab - and below 512 rows a slice the launch is mostly
// the slabs' traffic, hence the two caps; the rule now picks 2, 4, 7, 7 and
// 2, 4, 8, 8 slices down the two columns of towers.
static int tower_wgrad_plan(TowerWgradArgs* a, int m_split) {
    int tiles = 0, off = 0, boff = 0;
    for (int l = 0; l < a->L; ++l) {
        TowerWgradLayer* y = &a->ly[l];
        y->ldo = (y->jdim + 31) / 32 * 32;
        y->tj = (y->jdim + 63) / 64;
        y->tile0 = tiles;
        y->off = off;
        tiles += (y->h + 63) / 64 * y->tj;
        off += y->h * y->ldo;
    }
    for (int l = 0; l < a->L; ++l) {
        a->ly[l].boff = off + boff;
        boff += a->ly[l].h;
    }
    a->tiles = tiles;
    a->hoff = off + boff;
    a->per = (a->hoff + a->hl + 1 + 3) / 4 * 4;
    const int nch = a->M > 0 ? (a->M + WG_KC - 1) / WG_KC : 1;
    int s = m_split;
    if (s <= 0) {
        s = (2 * 256 + tiles - 1) / tiles;
        if (s > 8) s = 8;
        if (s > nch / 4) s = nch / 4;
        if (s < 1) s = 1;
    }
    if (s > 16) s = 16;
    if (s > nch) s = nch;
    a->cps = (nch + s - 1) / s;
    return (nch + a->cps - 1) / a->cps;
}

extern "C" {

// -> S, the slices the launcher cuts M into, and through `floats` the size
// of the scratch it needs (S slabs). Only the shapes of `args` are read.
int emb_tower_wgrad_plan(const TowerWgradArgs* args, int m_split,
                         long* floats) {
    TowerWgradArgs a = *args;
    const int S = tower_wgrad_plan(&a, m_split);
    if (floats) *floats = (long)S * a.per;
    return S;
}

void emb_tower_wgrad(const TowerWgradArgs* args, const TowerFoldArgs* fold,
                     const float* dout, float* scratch, int m_split,
                     hipStream_t stream) {
    TowerWgradArgs a = *args;
    TowerFoldArgs f = *fold;
    const int S = tower_wgrad_plan(&a, m_split), L = a.L;
    dim3 grid((unsigned)(a.tiles + 1), (unsigned)S);
    k_tower_wgrad<<<grid, 512, 0, stream>>>(a, dout, scratch);

    int pieces = 0;
    for (int i = 0; i < f.n; ++i) {
        TowerFoldOne* g = &f.g[i];
        if (i < L) {
            const TowerWgradLayer& y = a.ly[i];
            g->src = y.off;
            g->rows = y.h;
            g->cols = i ? y.jdim : f.K0;
            g->ld = y.ldo;
        } else {
            g->rows = 1;
            g->ld = 0;
            g->src = i < 2 * L ? a.ly[i - L].boff
                               : i == 2 * L ? a.hoff : a.hoff + a.hl;
            g->cols = i < 2 * L ? a.ly[i - L].h : i == 2 * L ? a.hl : 1;
        }
        g->vec = g->vec && g->cols % 8 == 0;
        g->p0 = pieces;
        pieces += g->rows * ((g->cols + 7) / 8);
    }
    f.S = S;
    f.per = a.per;
    f.pieces = pieces;
    const int fgrid = (pieces + 255) / 256;
    k_tower_wgrad_fold<<<fgrid, 256, 0, stream>>>(f, scratch);
}

}  // extern "C"
