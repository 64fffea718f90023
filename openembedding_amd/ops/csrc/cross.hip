// DCN-v2 cross network (gfx950 / MI355X): L layers of
//   x_{l+1} = x_0 * (W_l x_l + b_l) + x_l        x in R^d, W_l [d, d]
// forward and the dgrad chain of the backward, ONE launch each, all L layers
// inside the kernel.
//
// Operands are bf16, every sum and product is fp32 (mfma_f32_16x16x32_bf16,
// -ffp-contract=off), values are rounded to bf16 (nearest even) exactly
// where they are written below.
//
// Forward, per row and layer:
//   acc[o] = sum_k W_l[o,k] x_l[k]         t = acc + b_l[o]
//   u_l[o] = bf16(t)                        (mirrored when a backward follows)
//   y = x_0[o] * t;  y = y + x_l[o];  x_{l+1}[o] = bf16(y)     (t unrounded)
//   logit form: out = sum_o w_out[o] x_L[o], + b_out, + partial
// Backward, g_L = bf16(dout * w_out[o]) or the incoming bf16 gradient:
//   for l = L-1 .. 0:   q_l = bf16(g_{l+1} * x_0)      -> HBM [L, M, dp]
//                       a  += g_{l+1} * u_l             (fp32, this order)
//                       g_l = bf16(sum_o q_l[o] W_l[o,k] + g_{l+1}[k])
//   dx0 = bf16(a + g_0)
// Pad columns (d <= o < dp) of every output are exactly zero. No atomics:
// each element is written once, both kernels are bitwise reproducible.
// dW_l = q_l^T x_l, db_l = sum_m q_l and the head's gradients are library
// ops on what the kernels wrote (models/ctr.py, ops/dispatch.py).
//
// Work split: a block of 8 waves owns BM in {16, 32} consecutive rows for
// all L layers. Three LDS tiles [BM][dp + 8] bf16: x_0, and two that swap
// roles per layer (forward: x_l / x_{l+1}; backward: q_l / q_{l-1}). The
// stride dp + 8 is 16 j + 4 dwords, gcd(stride, 64) = 4: the 16 rows of a
// fragment read start on 16 distinct 4-bank groups (as in dlrm.hip). The
// staging pass writes every (row, k < dp) of the tiles it fills - rows past
// M and x_0's pad columns as zeros - and each layer writes the whole of the
// other tile before anybody reads it, so no element a fragment reads is
// ever uninitialised LDS, and nothing is ever multiplied into a pad that is
// not an exact zero (0 * inf = NaN: docs/kernels.md, mlp.hip).
//
// Weights stream through L2 in the fragment-major image of W_l padded to
// [dp, dp] (forward) and of W_l^T (backward: g_l = q_l W_l is then the same
// row-tile x [out, in] GEMM); both are written by k_mlp3_pack_frag, element
// (n, k) at ((n/16 * KS + k/32) * 64 + (k%32)/8 * 16 + n%16) * 8 + k%8,
// KS = dp / 32. A 16-column chunk is one run of KS KB; a wave takes chunks
// wave, wave + 8, .., the first rotated by blockIdx.x, double-buffered in
// registers. What the epilogue needs from HBM (bias; u_l in the backward) is
// loaded BEFORE the next chunk's prefetch is issued, and a layer's first
// chunk before the barrier that ends the previous layer (one barrier per
// layer).
//
// MFMA operand order: the WEIGHT fragment is operand A and the activation
// fragment operand B, so the accumulator is the transposed tile: a lane
// holds out columns o0 .. o0+3 (o0 = 16 c + (lane>>4) * 4) of ONE row
// (lane & 15). The k-order of every sum is the same as with the operands
// the other way round; the epilogue, which runs in this map, then reads
// x_0 / x_l and writes x_{l+1}, u_l, q_l as 8-byte pieces (LDS and HBM)
// where the usual map gives 2-byte ones. For the same reason the lane that
// produces g_l[row, k] in one layer produces it in every layer: g and the
// accumulator a of dx0 stay in that lane's registers for the whole
// backward, and q_{l-1} = bf16(g_l x_0) is formed in the same epilogue -
// the elementwise work never gets a pass of its own.
//
// KS is a run-time value below the template bound KSM in {4, 8, 16}: the
// unrolled k-loops skip steps s >= KS with a wave-uniform test. A fragments
// of the block's rows live in registers for a whole layer while
// RT * KSM <= 16 (64 VGPRs; the backward, which also keeps g and a: <= 8),
// beyond that they are re-read from the LDS tile per chunk (conflict-free);
// the backward at BM = 32, KSM = 16 keeps 64 VGPRs of g and a and therefore
// streams its weights single-buffered.

#include "cross_common.h"

#define CROSS_WAVES 8
#define CROSS_PAD 8          // elements behind a tile row (16 bytes)

// logical chunk li of the block -> the chunk it streams
static __device__ __forceinline__ int cross_rot(int li, int rot, int nch) {
    const int c = li + rot;
    return c >= nch ? c - nch : c;
}

// the lane's pieces of chunk c (wave-uniform) of one weight image
template <int KSM>
static __device__ __forceinline__ void cross_ld_b(bf16x8 (&b)[KSM],
                                                  const uint16_t* W, int c,
                                                  int ks, int lane) {
    const uint16_t* pb = W + __builtin_amdgcn_readfirstlane(c) * (ks * 512)
                           + (unsigned)(lane * 8);
    #pragma unroll
    for (int s = 0; s < KSM; ++s)
        if (s < ks) b[s] = cross_frag(pb + 512 * s);
}

// A fragments of one row tile, from an LDS tile
template <int KSM>
static __device__ __forceinline__ void cross_ld_a(bf16x8 (&a)[KSM],
                                                  const uint16_t* tile,
                                                  int LD, int rt, int ks,
                                                  int lane) {
    const uint16_t* pa = tile + (rt * 16 + (lane & 15)) * LD
                              + (lane >> 4) * 8;
    #pragma unroll
    for (int s = 0; s < KSM; ++s)
        if (s < ks) a[s] = cross_frag(pa + 32 * s);
}

// acc[r] = sum_k W[o0 + r][k] * A[row][k] for the lane's row of row tile rt
template <int KSM, bool AREG>
static __device__ __forceinline__ f32x4 cross_tile(const bf16x8 (&b)[KSM],
                                                   const bf16x8 (&a)[KSM],
                                                   const uint16_t* tile,
                                                   int LD, int rt, int ks,
                                                   int lane) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const uint16_t* pa = tile + (rt * 16 + (lane & 15)) * LD
                              + (lane >> 4) * 8;
    #pragma unroll
    for (int s = 0; s < KSM; ++s)
        if (s < ks)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                b[s], AREG ? a[s] : cross_frag(pa + 32 * s), acc, 0, 0, 0);
    return acc;
}

// ---- forward ----------------------------------------------------------
// xs: mirrors of x_1 .. x_L as [L, M, dp] (save_all), or of x_L alone as
// [1, M, dp], or null (logit form without a backward); us: [L, M, dp] or
// null. w_out null: the x_L form.
template <int BM, int KSM>
__global__ __launch_bounds__(64 * CROSS_WAVES)
void k_cross_fwd(const uint16_t* __restrict__ x0,
                 const uint16_t* __restrict__ wimg,   // [L] images [dp, dp]
                 const uint16_t* __restrict__ bias,   // [L, d]
                 int M, int d, int ks, int L,
                 uint16_t* __restrict__ xs, uint16_t* __restrict__ us,
                 int save_all,
                 const uint16_t* __restrict__ w_out,  // [d] or null
                 const uint16_t* __restrict__ b_out,  // [1]
                 const float* __restrict__ partial,   // [M] or null
                 float* __restrict__ out) {           // [M]
    constexpr int RT = BM / 16;
    constexpr int NIT = KSM / 4;     // chunks of a wave: 2 KSM / 8 at most
    constexpr bool AREG = RT * KSM <= 16;
    extern __shared__ uint4 cross_smem[];
    const int dp = ks * 32, LD = dp + CROSS_PAD, nch = ks * 2;
    uint16_t* const tx0 = reinterpret_cast<uint16_t*>(cross_smem);
    uint16_t* cur = tx0 + BM * LD;
    uint16_t* nxt = cur + BM * LD;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m0 = (int)blockIdx.x * BM;
    const int rot = (int)(blockIdx.x % (unsigned)nch);
    const int rl = lane & 15, g4 = lane >> 4;
    const int MD = M * dp;           // one layer of a mirror

    cross_stage_x0<BM>(x0, m0, M, d, dp, LD, tx0, cur);

    for (int l = 0; l < L; ++l) {
        const uint16_t* W = wimg + l * dp * dp;
        const uint16_t* bl = bias + l * d;
        const bool keep = xs != nullptr && (save_all || l == L - 1);
        uint16_t* const xm = xs + (save_all ? l * MD : 0);
        bf16x8 bb[2][KSM];
        if (wave < nch)
            cross_ld_b<KSM>(bb[0], W, cross_rot(wave, rot, nch), ks, lane);
        __syncthreads();             // the tile `cur` is complete
        bf16x8 a[AREG ? RT : 1][KSM];
        if (AREG) {
            #pragma unroll
            for (int rt = 0; rt < RT; ++rt)
                cross_ld_a<KSM>(a[AREG ? rt : 0], cur, LD, rt, ks, lane);
        }
        #pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int li = wave + CROSS_WAVES * it;
            if (li < nch) {
                const int o0 = cross_rot(li, rot, nch) * 16 + g4 * 4;
                unsigned bv[4];
                #pragma unroll
                for (int r = 0; r < 4; ++r)
                    bv[r] = o0 + r < d ? (unsigned)bl[o0 + r] : 0u;
                if (it + 1 < NIT && li + CROSS_WAVES < nch)
                    cross_ld_b<KSM>(bb[(it + 1) & 1], W,
                                    cross_rot(li + CROSS_WAVES, rot, nch),
                                    ks, lane);
                #pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const f32x4 acc = cross_tile<KSM, AREG>(
                        bb[it & 1], a[AREG ? rt : 0], cur, LD, rt, ks, lane);
                    const int row = rt * 16 + rl;
                    const int at = row * LD + o0;
                    float x0v[4], xlv[4];
                    cross_unpack(*reinterpret_cast<const uint2*>(tx0 + at),
                                 x0v);
                    cross_unpack(*reinterpret_cast<const uint2*>(cur + at),
                                 xlv);
                    unsigned uh[4], xh[4];
                    #pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float t = acc[r] + cross_f32(bv[r]);
                        float y = x0v[r] * t;
                        y = y + xlv[r];
                        const bool live = o0 + r < d;
                        uh[r] = live ? cross_rne(t) : 0u;
                        xh[r] = live ? cross_rne(y) : 0u;
                    }
                    const uint2 xp = cross_pack(xh);
                    *reinterpret_cast<uint2*>(nxt + at) = xp;
                    const int gm = m0 + row;
                    if (gm < M) {
                        const int go = gm * dp + o0;
                        if (keep) *reinterpret_cast<uint2*>(xm + go) = xp;
                        if (us)
                            *reinterpret_cast<uint2*>(us + l * MD + go)
                                = cross_pack(uh);
                    }
                }
            }
        }
        uint16_t* const sw = cur;
        cur = nxt;
        nxt = sw;
    }

    if (w_out) {
        // out[row] = <w_out, x_L[row]>: a wave per row, lanes stride the
        // columns, then a shuffle tree - a fixed order
        __syncthreads();
        for (int row = wave; row < BM && m0 + row < M; row += CROSS_WAVES) {
            float s = 0.f;
            for (int k = lane; k < d; k += 64)
                s += cross_f32(w_out[k]) * cross_f32(cur[row * LD + k]);
            #pragma unroll
            for (int off = 32; off; off >>= 1)
                s += __shfl_down(s, off, 64);
            if (lane == 0) {
                float v = s + cross_f32(b_out[0]);
                if (partial) v = v + partial[m0 + row];
                out[m0 + row] = v;
            }
        }
    }
}

// ---- backward ---------------------------------------------------------
// g_L from (dout [M] fp32, w_out [d]) in the logit form, else from gl
// [M, dp] bf16. wtimg: the images of W_l^T. qs [L, M, dp], dx0 [M, dp].
template <int BM, int KSM>
__global__ __launch_bounds__(64 * CROSS_WAVES)
void k_cross_bwd(const uint16_t* __restrict__ x0,
                 const uint16_t* __restrict__ us,     // [L, M, dp]
                 const uint16_t* __restrict__ wtimg,  // [L] images [dp, dp]
                 int M, int d, int ks, int L,
                 const float* __restrict__ dout,      // [M] or null
                 const uint16_t* __restrict__ w_out,  // [d] or null
                 const uint16_t* __restrict__ gl,     // [M, dp] or null
                 uint16_t* __restrict__ qs, uint16_t* __restrict__ dx0) {
    constexpr int RT = BM / 16;
    constexpr int NIT = KSM / 4;
    constexpr bool AREG = RT * KSM <= 8;   // g and a need the registers
    constexpr bool DBUF = RT * KSM < 32;   // see the head of the file
    extern __shared__ uint4 cross_smem[];
    const int dp = ks * 32, LD = dp + CROSS_PAD, nch = ks * 2;
    uint16_t* const tx0 = reinterpret_cast<uint16_t*>(cross_smem);
    uint16_t* cur = tx0 + BM * LD;
    uint16_t* nxt = cur + BM * LD;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m0 = (int)blockIdx.x * BM;
    const int rot = (int)(blockIdx.x % (unsigned)nch);
    const int rl = lane & 15, g4 = lane >> 4;
    const int MD = M * dp;

    cross_stage_x0<BM>(x0, m0, M, d, dp, LD, tx0, nullptr);
    __syncthreads();

    // g_L, a = 0 and q_{L-1} for the elements this lane owns
    float a[NIT][RT][4], g[NIT][RT][4];
    #pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int li = wave + CROSS_WAVES * it;
        if (li < nch) {
            const int k0 = cross_rot(li, rot, nch) * 16 + g4 * 4;
            float wv[4] = {0.f, 0.f, 0.f, 0.f};
            if (w_out) {
                #pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (k0 + r < d) wv[r] = cross_f32(w_out[k0 + r]);
            }
            #pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const int row = rt * 16 + rl, gm = m0 + row;
                const int at = row * LD + k0;
                float gv[4] = {0.f, 0.f, 0.f, 0.f}, x0v[4];
                if (gm < M) {
                    if (w_out) {
                        const float dv = dout[gm];
                        #pragma unroll
                        for (int r = 0; r < 4; ++r)
                            gv[r] = cross_f32(cross_rne(dv * wv[r]));
                    } else {
                        cross_unpack(*reinterpret_cast<const uint2*>(
                            gl + gm * dp + k0), gv);
                    }
                }
                cross_unpack(*reinterpret_cast<const uint2*>(tx0 + at), x0v);
                unsigned qh[4];
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (k0 + r >= d) gv[r] = 0.f;
                    a[it][rt][r] = 0.f;
                    g[it][rt][r] = gv[r];
                    qh[r] = k0 + r < d ? cross_rne(gv[r] * x0v[r]) : 0u;
                }
                const uint2 qp = cross_pack(qh);
                *reinterpret_cast<uint2*>(cur + at) = qp;
                if (gm < M)
                    *reinterpret_cast<uint2*>(qs + (L - 1) * MD + gm * dp
                                              + k0) = qp;
            }
        }
    }

    for (int l = L - 1; l >= 0; --l) {
        const uint16_t* W = wtimg + l * dp * dp;
        const uint16_t* ul = us + l * MD;
        bf16x8 bb[DBUF ? 2 : 1][KSM];
        if (wave < nch)
            cross_ld_b<KSM>(bb[0], W, cross_rot(wave, rot, nch), ks, lane);
        __syncthreads();             // the tile `cur` (q_l) is complete
        bf16x8 af[AREG ? RT : 1][KSM];
        if (AREG) {
            #pragma unroll
            for (int rt = 0; rt < RT; ++rt)
                cross_ld_a<KSM>(af[AREG ? rt : 0], cur, LD, rt, ks, lane);
        }
        #pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int li = wave + CROSS_WAVES * it;
            if (li < nch) {
                const int k0 = cross_rot(li, rot, nch) * 16 + g4 * 4;
                uint2 up[RT];
                #pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const int gm = m0 + rt * 16 + rl;
                    up[rt] = gm < M ? *reinterpret_cast<const uint2*>(
                                          ul + gm * dp + k0)
                                    : make_uint2(0u, 0u);
                }
                if (DBUF) {
                    if (it + 1 < NIT && li + CROSS_WAVES < nch)
                        cross_ld_b<KSM>(bb[DBUF ? (it + 1) & 1 : 0], W,
                                        cross_rot(li + CROSS_WAVES, rot, nch),
                                        ks, lane);
                } else if (it > 0) {
                    cross_ld_b<KSM>(bb[0], W, cross_rot(li, rot, nch), ks,
                                    lane);
                }
                #pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const f32x4 acc = cross_tile<KSM, AREG>(
                        bb[DBUF ? it & 1 : 0], af[AREG ? rt : 0], cur, LD,
                        rt, ks, lane);
                    const int row = rt * 16 + rl, gm = m0 + row;
                    const int at = row * LD + k0;
                    float uv[4], x0v[4];
                    cross_unpack(up[rt], uv);
                    cross_unpack(*reinterpret_cast<const uint2*>(tx0 + at),
                                 x0v);
                    unsigned qh[4];
                    #pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float gv = g[it][rt][r];
                        const float p = gv * uv[r];
                        a[it][rt][r] = a[it][rt][r] + p;
                        const float gn = k0 + r < d
                            ? cross_f32(cross_rne(acc[r] + gv)) : 0.f;
                        g[it][rt][r] = gn;
                        qh[r] = k0 + r < d ? cross_rne(gn * x0v[r]) : 0u;
                    }
                    if (l > 0) {
                        const uint2 qp = cross_pack(qh);
                        *reinterpret_cast<uint2*>(nxt + at) = qp;
                        if (gm < M)
                            *reinterpret_cast<uint2*>(qs + (l - 1) * MD
                                                      + gm * dp + k0) = qp;
                    }
                }
            }
        }
        uint16_t* const sw = cur;
        cur = nxt;
        nxt = sw;
    }

    #pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int li = wave + CROSS_WAVES * it;
        if (li < nch) {
            const int k0 = cross_rot(li, rot, nch) * 16 + g4 * 4;
            #pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const int gm = m0 + rt * 16 + rl;
                unsigned h[4];
                #pragma unroll
                for (int r = 0; r < 4; ++r)
                    h[r] = k0 + r < d
                        ? cross_rne(a[it][rt][r] + g[it][rt][r]) : 0u;
                if (gm < M)
                    *reinterpret_cast<uint2*>(dx0 + gm * dp + k0)
                        = cross_pack(h);
            }
        }
    }
}

// ---- launchers --------------------------------------------------------

// Rows per block. A block streams all L weight images (L dp^2 x 2 bytes)
// whatever BM is, so BM = 32 halves the bytes streamed per row but also the
// number of blocks: it pays only once BM = 16 would need more than one
// block per CU. Rule (as mlp_pick_bm): 16 while ceil(M / 16) <= CUs, else
// 32. MI355X (256 CUs), L = 3, logit form with mirrors, us per launch, best
// of 3 x 200 back-to-back launches (scripts/bench_dcn.py), fwd / bwd:
//   M       dp 256 BM=16   BM=32          dp 448 BM=16    BM=32
//   1024    14.8 / 10.8    20.5 / 16.8    34.1 / 27.1     50.5 / 47.6
//   4096    16.5 / 11.6    21.5 / 17.6    37.1 / 32.1     52.9 / 52.9
//   8192    29.7 / 21.4    22.5 / 18.3    73.7 / 63.4     56.2 / 55.6
//   16384   57.9 / 43.0    43.9 / 36.3   146.6 / 126.4   109.4 / 108.3
static int cross_pick_bm(long M, int bm) {
    if (bm == 16 || bm == 32) return bm;
    return (M + 15) / 16 <= device_cus() ? 16 : 32;
}

// the three tiles: BM = 32 at dp > 256 needs more than the 64 KB a kernel
// gets by default (allow_lds)
static size_t cross_lds(int bm, long dp) {
    return (size_t)3 * bm * (dp + CROSS_PAD) * 2;
}

extern "C" {

// The shapes the kernels take; the binding refuses everything else.
int emb_cross_fits(long M, long d, long dp, long L) {
    return d >= 1 && dp == (d + 31) / 32 * 32 && dp >= 32 && dp <= 512
        && L >= 1 && L <= 6 && M >= 0 && M * dp * (L + 1) < (1L << 31);
}

int emb_cross_bm(long M, int bm) { return cross_pick_bm(M, bm); }

void emb_cross_fwd(const void* x0, const void* wimg, const void* bias,
                   long M, long d, long dp, long L, void* xs, void* us,
                   int save_all, const void* w_out, const void* b_out,
                   const float* partial, float* out, int bm,
                   hipStream_t stream) {
    if (M == 0) return;
    bm = cross_pick_bm(M, bm);
    const size_t lds = cross_lds(bm, dp);
    const int ks = (int)(dp / 32), grid = (int)((M + bm - 1) / bm);
    const int block = 64 * CROSS_WAVES;
    CROSS_LAUNCH(k_cross_fwd, (const uint16_t*)x0, (const uint16_t*)wimg,
                 (const uint16_t*)bias, (int)M, (int)d, ks, (int)L,
                 (uint16_t*)xs, (uint16_t*)us, save_all,
                 (const uint16_t*)w_out, (const uint16_t*)b_out, partial,
                 out);
}

void emb_cross_bwd(const void* x0, const void* us, const void* wtimg, long M,
                   long d, long dp, long L, const float* dout,
                   const void* w_out, const void* gl, void* qs, void* dx0,
                   int bm, hipStream_t stream) {
    if (M == 0) return;
    bm = cross_pick_bm(M, bm);
    const size_t lds = cross_lds(bm, dp);
    const int ks = (int)(dp / 32), grid = (int)((M + bm - 1) / bm);
    const int block = 64 * CROSS_WAVES;
    CROSS_LAUNCH(k_cross_bwd, (const uint16_t*)x0, (const uint16_t*)us,
                 (const uint16_t*)wtimg, (int)M, (int)d, ks, (int)L, dout,
                 (const uint16_t*)w_out, (const uint16_t*)gl, (uint16_t*)qs,
                 (uint16_t*)dx0);
}

}  // extern "C"
