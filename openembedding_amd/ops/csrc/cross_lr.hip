// DCN-v2 low-rank cross network (gfx950 / MI355X): L layers of
//   x_{l+1} = x_0 * (U_l (V_l x_l) + b_l) + x_l
// x in R^d, V_l [r, d] the down-projection, U_l [d, r] the up-projection,
// forward and the dgrad chain of the backward, ONE launch each, all L layers
// inside the kernel.
//
// Operands are bf16, every sum and product is fp32 (mfma_f32_16x16x32_bf16,
// -ffp-contract=off), values are rounded to bf16 (nearest even) exactly
// where they are written below.
//
// Forward, per row and layer:
//   pa[j] = sum_k V_l[j,k] x_l[k]          p_l = bf16(pa)   (mirrored)
//   t[o] = sum_j U_l[o,j] p_l[j];  t = t + b_l[o]
//   u_l[o] = bf16(t)                                         (mirrored)
//   y = x_0[o] * t;  y = y + x_l[o];  x_{l+1}[o] = bf16(y)   (t unrounded)
//   logit form: out = sum_o w_out[o] x_L[o], + b_out, + partial
// Backward, g_L = bf16(dout * w_out[o]) or the incoming bf16 gradient:
//   for l = L-1 .. 0:   q_l = bf16(g_{l+1} * x_0)       -> HBM [L, M, dp]
//                       a  += g_{l+1} * u_l              (fp32, this order)
//                       sa[j] = sum_o q_l[o] U_l[o,j]    s_l = bf16(sa)
//                                                        -> HBM [L, M, rp]
//                       g_l = bf16(sum_j s_l[j] V_l[j,k] + g_{l+1}[k])
//   dx0 = bf16(a + g_0)
// Pad columns (d <= o < dp, r <= j < rp) of every output are exactly zero.
// No atomics: each element is written once, both kernels are bitwise
// reproducible. dU_l = q_l^T p_l, dV_l = s_l^T x_l, db_l = sum_m q_l and the
// head's gradients are library ops on what the kernels wrote
// (ops/dispatch.py).
//
// Both directions are the same pair of dependent GEMMs per layer: a skinny
// "down" GEMM (N = rp <= 128, K = dp) on an LDS tile and an "up" GEMM
// (N = dp, K = rp: one to four k-steps) whose epilogue is the elementwise
// part of the layer. The four weight images per layer - V_l [rp, dp] and
// U_l [dp, rp] forward, U_l^T [rp, dp] and V_l^T [dp, rp] backward - are
// fragment-major (k_mlp3_pack_frag, mlp.hip): element (n, k) of an [N, Kp]
// image at ((n/16 * KS + k/32) * 64 + (k%32)/8 * 16 + n%16) * 8 + k%8,
// KS = Kp / 32. A layer's images are 4 dp rp bytes (64 KB at 256 x 64) and
// stay in L2; the waves read their fragments from there straight into
// registers (docs/kernels.md has the reasons and the resource report).
//
// Work split: a block of 8 waves owns BM in {16, 32} consecutive rows for
// all L layers. LDS: three tiles [BM][dp + 8] bf16 - x_0 and two that swap
// roles per layer (forward x_l / x_{l+1}, backward q_l / q_{l-1}), row
// stride 16 j + 4 dwords as in cross.hip - and the fp32 partial sums of the
// down GEMM, [W][BM][rp + 4] (row stride = 4 mod 32 dwords: the 16 rows of
// a fragment start on 16 distinct 4-bank groups).
//
// Down GEMM: rp / 16 column chunks are fewer than the waves, so the
// contraction is split W ways over k (W = 4, 2, 4, 1 at rp = 32, 64, 96,
// 128): task (chunk c, part w) covers k-steps [w KS / W, (w + 1) KS / W)
// for both row tiles and stores its fp32 accumulators; tasks go round the
// waves. After one barrier EVERY wave sums the W partials of the whole
// rank tile in the fixed order ((p0 + p1) + p2) + p3, rounds once, and so
// holds p_l (s_l) as the B fragments of its up GEMM directly in registers:
// RT * rp / 32 fragments, <= 32 VGPRs. The rank activation never gets an
// LDS tile or a pass of its own; fragment (rt, s) is mirrored to HBM by
// wave (4 rt + s) % 8 in 16-byte pieces.
//
// Up GEMM: dp / 16 column chunks, wave takes chunks wave, wave + 8, ..,
// weights double-buffered in registers. As in cross.hip the WEIGHT
// fragment is MFMA operand A, so a lane holds four consecutive columns
// o0 .. o0+3 (o0 = 16 c + (lane>>4) * 4) of ONE row (lane & 15), moves
// 8-byte pieces, and owns the same (row, columns) in every layer: g and a
// stay in its registers for the whole backward.
//
// Two barriers per layer: one before the down GEMM (the tile it reads is
// complete, the partials of the previous layer are consumed) and one
// before the up GEMM (the partials are complete). Every (row < BM, k < dp)
// of a tile and every (w, row, j < rp) of the partials is written before
// it is read: no zeroing pass, no uninitialised LDS.

#include "cross_common.h"

#define CLR_WAVES 8
#define CLR_PAD 8            // bf16 elements behind a tile row (16 bytes)
#define CLR_PPAD 4           // floats behind a row of the partials
#define CLR_RSM 4            // k-steps of the up GEMM at most (rp <= 128)

// Down GEMM: part[w][row][j] = sum over the k-steps of part w of
// img[j][k] * tile[row][k], img one [rp, dp] image, nc = rp / 16 chunks.
template <int BM>
static __device__ __forceinline__ void clr_down(
        const uint16_t* __restrict__ img, const uint16_t* tile, int LD,
        int ks, int nc, int nsplit, float* part, int LDP, int wave,
        int lane) {
    constexpr int RT = BM / 16;
    const int rl = lane & 15, g4 = lane >> 4;
    const int ntask = nc * nsplit;
    for (int t = wave; t < ntask; t += CLR_WAVES) {      // wave-uniform
        const int w = t / nc, c = t - w * nc;
        const int s0 = w * ks / nsplit, s1 = (w + 1) * ks / nsplit;
        f32x4 acc[RT];
        #pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const uint16_t* pb = img + c * ks * 512 + lane * 8;
        const uint16_t* pa = tile + rl * LD + g4 * 8;
        // two k-steps a trip, both weight loads in flight before the MFMAs
        for (int s = s0; s < s1; s += 2) {
            const bool two = s + 1 < s1;
            const bf16x8 b0 = cross_frag(pb + s * 512);
            const bf16x8 b1 = cross_frag(pb + (two ? s + 1 : s) * 512);
            #pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const uint16_t* par = pa + rt * 16 * LD + s * 32;
                acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    b0, cross_frag(par), acc[rt], 0, 0, 0);
                if (two)
                    acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        b1, cross_frag(par + 32), acc[rt], 0, 0, 0);
            }
        }
        #pragma unroll
        for (int rt = 0; rt < RT; ++rt)
            *reinterpret_cast<f32x4*>(part + (w * BM + rt * 16 + rl) * LDP
                                      + c * 16 + g4 * 4) = acc[rt];
    }
}

// The rank tile as B fragments of the up GEMM: the partials summed in the
// order w = 0, 1, .., rounded once, pad columns j >= r zero. mir: this
// layer's [M, rp] mirror or null.
template <int BM>
static __device__ __forceinline__ void clr_rank_frags(
        bf16x8 (&pf)[BM / 16][CLR_RSM], const float* part, int LDP,
        int nsplit, int ksr, int r, uint16_t* __restrict__ mir, int m0,
        int M, int wave, int lane) {
    constexpr int RT = BM / 16;
    const int rl = lane & 15, g4 = lane >> 4, rp = ksr * 32;
    #pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        #pragma unroll
        for (int s = 0; s < CLR_RSM; ++s) {
            if (s < ksr) {
                const int j0 = s * 32 + g4 * 8;
                const float* pp = part + (rt * 16 + rl) * LDP + j0;
                f32x4 lo = *reinterpret_cast<const f32x4*>(pp);
                f32x4 hi = *reinterpret_cast<const f32x4*>(pp + 4);
                for (int w = 1; w < nsplit; ++w) {
                    const float* pw = pp + w * BM * LDP;
                    const f32x4 l2 = *reinterpret_cast<const f32x4*>(pw);
                    const f32x4 h2 = *reinterpret_cast<const f32x4*>(pw + 4);
                    #pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        lo[i] = lo[i] + l2[i];
                        hi[i] = hi[i] + h2[i];
                    }
                }
                unsigned h[8];
                #pragma unroll
                for (int i = 0; i < 4; ++i) {
                    h[i] = j0 + i < r ? cross_rne(lo[i]) : 0u;
                    h[4 + i] = j0 + 4 + i < r ? cross_rne(hi[i]) : 0u;
                }
                const uint4 v = make_uint4(h[0] | (h[1] << 16),
                                           h[2] | (h[3] << 16),
                                           h[4] | (h[5] << 16),
                                           h[6] | (h[7] << 16));
                pf[rt][s] = __builtin_bit_cast(bf16x8, v);
                const int gm = m0 + rt * 16 + rl;
                if (mir && ((rt * CLR_RSM + s) & (CLR_WAVES - 1)) == wave
                        && gm < M)
                    *reinterpret_cast<uint4*>(mir + gm * rp + j0) = v;
            }
        }
    }
}

// the lane's pieces of chunk c (wave-uniform) of one [dp, rp] image
static __device__ __forceinline__ void clr_ld_w(bf16x8 (&b)[CLR_RSM],
                                                const uint16_t* img, int c,
                                                int ksr, int lane) {
    const uint16_t* pb = img + __builtin_amdgcn_readfirstlane(c) * (ksr * 512)
                             + (unsigned)(lane * 8);
    #pragma unroll
    for (int s = 0; s < CLR_RSM; ++s)
        if (s < ksr) b[s] = cross_frag(pb + 512 * s);
}

static __device__ __forceinline__ f32x4 clr_up(const bf16x8 (&b)[CLR_RSM],
                                               const bf16x8 (&p)[CLR_RSM],
                                               int ksr) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    #pragma unroll
    for (int s = 0; s < CLR_RSM; ++s)
        if (s < ksr)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[s], p[s], acc,
                                                          0, 0, 0);
    return acc;
}

// ---- forward ----------------------------------------------------------
// xs: mirrors of x_1 .. x_L as [L, M, dp] (save_all, with us [L, M, dp] and
// ps [L, M, rp]), or of x_L alone as [1, M, dp], or null (logit form
// without a backward). w_out null: the x_L form.
template <int BM, int KSM>
__global__ __launch_bounds__(64 * CLR_WAVES)
void k_cross_lr_fwd(const uint16_t* __restrict__ x0,
                    const uint16_t* __restrict__ vimg,  // [L] images [rp, dp]
                    const uint16_t* __restrict__ uimg,  // [L] images [dp, rp]
                    const uint16_t* __restrict__ bias,  // [L, d]
                    int M, int d, int ks, int r, int ksr, int nsplit, int L,
                    uint16_t* __restrict__ xs, uint16_t* __restrict__ us,
                    uint16_t* __restrict__ ps, int save_all,
                    const uint16_t* __restrict__ w_out,  // [d] or null
                    const uint16_t* __restrict__ b_out,  // [1]
                    const float* __restrict__ partial,   // [M] or null
                    float* __restrict__ out) {           // [M]
    constexpr int RT = BM / 16;
    constexpr int NIT = KSM / 4;     // chunks of a wave: 2 KSM / 8 at most
    extern __shared__ uint4 clr_smem[];
    const int dp = ks * 32, LD = dp + CLR_PAD, nch = ks * 2;
    const int rp = ksr * 32, LDP = rp + CLR_PPAD;
    uint16_t* const tx0 = reinterpret_cast<uint16_t*>(clr_smem);
    uint16_t* cur = tx0 + BM * LD;
    uint16_t* nxt = cur + BM * LD;
    float* const part = reinterpret_cast<float*>(nxt + BM * LD);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m0 = (int)blockIdx.x * BM;
    const int rl = lane & 15, g4 = lane >> 4;
    const int MD = M * dp;           // one layer of a [.., M, dp] mirror

    cross_stage_x0<BM>(x0, m0, M, d, dp, LD, tx0, cur);

    for (int l = 0; l < L; ++l) {
        const uint16_t* Ul = uimg + l * dp * rp;
        const uint16_t* bl = bias + l * d;
        const bool keep = xs != nullptr && (save_all || l == L - 1);
        uint16_t* const xm = xs + (save_all ? l * MD : 0);
        __syncthreads();             // `cur` complete, the partials consumed
        clr_down<BM>(vimg + l * rp * dp, cur, LD, ks, ksr * 2, nsplit, part,
                     LDP, wave, lane);
        bf16x8 bb[2][CLR_RSM];
        if (wave < nch) clr_ld_w(bb[0], Ul, wave, ksr, lane);
        __syncthreads();             // the partials are complete
        bf16x8 pf[RT][CLR_RSM];
        clr_rank_frags<BM>(pf, part, LDP, nsplit, ksr, r,
                           ps ? ps + l * M * rp : nullptr, m0, M, wave, lane);
        #pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int li = wave + CLR_WAVES * it;
            if (li < nch) {
                const int o0 = li * 16 + g4 * 4;
                unsigned bv[4];
                #pragma unroll
                for (int i = 0; i < 4; ++i)
                    bv[i] = o0 + i < d ? (unsigned)bl[o0 + i] : 0u;
                if (it + 1 < NIT && li + CLR_WAVES < nch)
                    clr_ld_w(bb[(it + 1) & 1], Ul, li + CLR_WAVES, ksr, lane);
                #pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const f32x4 acc = clr_up(bb[it & 1], pf[rt], ksr);
                    const int row = rt * 16 + rl;
                    const int at = row * LD + o0;
                    float x0v[4], xlv[4];
                    cross_unpack(*reinterpret_cast<const uint2*>(tx0 + at),
                                 x0v);
                    cross_unpack(*reinterpret_cast<const uint2*>(cur + at),
                                 xlv);
                    unsigned uh[4], xh[4];
                    #pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float t = acc[i] + cross_f32(bv[i]);
                        float y = x0v[i] * t;
                        y = y + xlv[i];
                        const bool live = o0 + i < d;
                        uh[i] = live ? cross_rne(t) : 0u;
                        xh[i] = live ? cross_rne(y) : 0u;
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
        // columns, then a shuffle tree - a fixed order (as k_cross_fwd)
        __syncthreads();
        for (int row = wave; row < BM && m0 + row < M; row += CLR_WAVES) {
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
// [M, dp] bf16. utimg: the images of U_l^T [rp, dp], vtimg: of V_l^T
// [dp, rp]. Writes qs [L, M, dp], ss [L, M, rp], dx0 [M, dp].
template <int BM, int KSM>
__global__ __launch_bounds__(64 * CLR_WAVES)
void k_cross_lr_bwd(const uint16_t* __restrict__ x0,
                    const uint16_t* __restrict__ us,     // [L, M, dp]
                    const uint16_t* __restrict__ utimg,
                    const uint16_t* __restrict__ vtimg,
                    int M, int d, int ks, int r, int ksr, int nsplit, int L,
                    const float* __restrict__ dout,      // [M] or null
                    const uint16_t* __restrict__ w_out,  // [d] or null
                    const uint16_t* __restrict__ gl,     // [M, dp] or null
                    uint16_t* __restrict__ qs, uint16_t* __restrict__ ss,
                    uint16_t* __restrict__ dx0) {
    constexpr int RT = BM / 16;
    constexpr int NIT = KSM / 4;
    extern __shared__ uint4 clr_smem[];
    const int dp = ks * 32, LD = dp + CLR_PAD, nch = ks * 2;
    const int rp = ksr * 32, LDP = rp + CLR_PPAD;
    uint16_t* const tx0 = reinterpret_cast<uint16_t*>(clr_smem);
    uint16_t* cur = tx0 + BM * LD;
    uint16_t* nxt = cur + BM * LD;
    float* const part = reinterpret_cast<float*>(nxt + BM * LD);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m0 = (int)blockIdx.x * BM;
    const int rl = lane & 15, g4 = lane >> 4;
    const int MD = M * dp;

    cross_stage_x0<BM>(x0, m0, M, d, dp, LD, tx0, nullptr);
    __syncthreads();

    // g_L, a = 0 and q_{L-1} for the elements this lane owns
    float a[NIT][RT][4], g[NIT][RT][4];
    #pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int li = wave + CLR_WAVES * it;
        if (li < nch) {
            const int k0 = li * 16 + g4 * 4;
            float wv[4] = {0.f, 0.f, 0.f, 0.f};
            if (w_out) {
                #pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (k0 + i < d) wv[i] = cross_f32(w_out[k0 + i]);
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
                        for (int i = 0; i < 4; ++i)
                            gv[i] = cross_f32(cross_rne(dv * wv[i]));
                    } else {
                        cross_unpack(*reinterpret_cast<const uint2*>(
                            gl + gm * dp + k0), gv);
                    }
                }
                cross_unpack(*reinterpret_cast<const uint2*>(tx0 + at), x0v);
                unsigned qh[4];
                #pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (k0 + i >= d) gv[i] = 0.f;
                    a[it][rt][i] = 0.f;
                    g[it][rt][i] = gv[i];
                    qh[i] = k0 + i < d ? cross_rne(gv[i] * x0v[i]) : 0u;
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
        const uint16_t* Vt = vtimg + l * dp * rp;
        const uint16_t* ul = us + l * MD;
        __syncthreads();             // `cur` (q_l) complete, partials consumed
        clr_down<BM>(utimg + l * rp * dp, cur, LD, ks, ksr * 2, nsplit, part,
                     LDP, wave, lane);
        bf16x8 bb[2][CLR_RSM];
        if (wave < nch) clr_ld_w(bb[0], Vt, wave, ksr, lane);
        __syncthreads();             // the partials are complete
        bf16x8 sf[RT][CLR_RSM];
        clr_rank_frags<BM>(sf, part, LDP, nsplit, ksr, r, ss + l * M * rp,
                           m0, M, wave, lane);
        #pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int li = wave + CLR_WAVES * it;
            if (li < nch) {
                const int k0 = li * 16 + g4 * 4;
                uint2 up[RT];
                #pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const int gm = m0 + rt * 16 + rl;
                    up[rt] = gm < M ? *reinterpret_cast<const uint2*>(
                                          ul + gm * dp + k0)
                                    : make_uint2(0u, 0u);
                }
                if (it + 1 < NIT && li + CLR_WAVES < nch)
                    clr_ld_w(bb[(it + 1) & 1], Vt, li + CLR_WAVES, ksr, lane);
                #pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const f32x4 acc = clr_up(bb[it & 1], sf[rt], ksr);
                    const int row = rt * 16 + rl, gm = m0 + row;
                    const int at = row * LD + k0;
                    float uv[4], x0v[4];
                    cross_unpack(up[rt], uv);
                    cross_unpack(*reinterpret_cast<const uint2*>(tx0 + at),
                                 x0v);
                    unsigned qh[4];
                    #pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float gv = g[it][rt][i];
                        const float p = gv * uv[i];
                        a[it][rt][i] = a[it][rt][i] + p;
                        const float gn = k0 + i < d
                            ? cross_f32(cross_rne(acc[i] + gv)) : 0.f;
                        g[it][rt][i] = gn;
                        qh[i] = k0 + i < d ? cross_rne(gn * x0v[i]) : 0u;
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
        const int li = wave + CLR_WAVES * it;
        if (li < nch) {
            const int k0 = li * 16 + g4 * 4;
            #pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const int gm = m0 + rt * 16 + rl;
                unsigned h[4];
                #pragma unroll
                for (int i = 0; i < 4; ++i)
                    h[i] = k0 + i < d
                        ? cross_rne(a[it][rt][i] + g[it][rt][i]) : 0u;
                if (gm < M)
                    *reinterpret_cast<uint2*>(dx0 + gm * dp + k0)
                        = cross_pack(h);
            }
        }
    }
}

// ---- launchers --------------------------------------------------------

// Rows per block: 16 while ceil(M / 16) <= 2 CUs, else 32. The weight
// stream is d / 2r smaller than cross.hip's, so BM = 32 saves little, and
// two BM = 16 blocks share a CU (34 KB of LDS, <= 128 VGPRs at dp = 256).
// MI355X, dp 256, L = 3, us per launch, fwd / bwd (scripts/bench_dcn_lr.py,
// profiles/dcn_cross_lr.md), r = 32 and r = 64:
//   M      BM=16 r32     BM=32 r32      BM=16 r64     BM=32 r64
//   4096   15.9 / 11.8   21.5 / 17.2    17.2 / 13.2   23.2 / 18.7
//   8192   20.3 / 15.9   22.5 / 18.3    22.1 / 18.2   24.6 / 19.9
// M > 8192 has not been measured: 32 there is cross.hip's experience.
static int clr_pick_bm(long M, int bm) {
    if (bm == 16 || bm == 32) return bm;
    return (M + 15) / 16 <= 2L * device_cus() ? 16 : 32;
}

// k-split of the down GEMM: tasks = rp / 16 chunks x W parts over 8 waves
static int clr_split(long rp) {
    const int nc = (int)(rp / 16);
    return CLR_WAVES % nc == 0 ? CLR_WAVES / nc : 4;
}

// tiles + partials: past the 64 KB a kernel gets by default at dp > 256
// (allow_lds)
static size_t clr_lds(int bm, long dp, long rp, int nsplit) {
    return (size_t)3 * bm * (dp + CLR_PAD) * 2
        + (size_t)nsplit * bm * (rp + CLR_PPAD) * 4;
}

extern "C" {

// The shapes the kernels take; the binding refuses everything else. The
// [L, M, rp] mirrors are indexed in 32 bits like the [L, M, dp] ones.
int emb_cross_lr_fits(long M, long d, long dp, long r, long rp, long L) {
    return d >= 1 && dp == (d + 31) / 32 * 32 && dp >= 32 && dp <= 512
        && r >= 1 && rp == (r + 31) / 32 * 32 && rp <= 128
        && L >= 1 && L <= 6 && M >= 0
        && M * (dp > rp ? dp : rp) * (L + 1) < (1L << 31);
}

int emb_cross_lr_bm(long M, int bm) { return clr_pick_bm(M, bm); }

void emb_cross_lr_fwd(const void* x0, const void* vimg, const void* uimg,
                      const void* bias, long M, long d, long dp, long r,
                      long rp, long L, void* xs, void* us, void* ps,
                      int save_all, const void* w_out, const void* b_out,
                      const float* partial, float* out, int bm,
                      hipStream_t stream) {
    if (M == 0) return;
    bm = clr_pick_bm(M, bm);
    const int ks = (int)(dp / 32), ksr = (int)(rp / 32);
    const int nsplit = clr_split(rp), grid = (int)((M + bm - 1) / bm);
    const int block = 64 * CLR_WAVES;
    const size_t lds = clr_lds(bm, dp, rp, nsplit);
    CROSS_LAUNCH(k_cross_lr_fwd, (const uint16_t*)x0, (const uint16_t*)vimg,
               (const uint16_t*)uimg, (const uint16_t*)bias, (int)M, (int)d,
               ks, (int)r, ksr, nsplit, (int)L, (uint16_t*)xs, (uint16_t*)us,
               (uint16_t*)ps, save_all, (const uint16_t*)w_out,
               (const uint16_t*)b_out, partial, out);
}

void emb_cross_lr_bwd(const void* x0, const void* us, const void* utimg,
                      const void* vtimg, long M, long d, long dp, long r,
                      long rp, long L, const float* dout, const void* w_out,
                      const void* gl, void* qs, void* ss, void* dx0, int bm,
                      hipStream_t stream) {
    if (M == 0) return;
    bm = clr_pick_bm(M, bm);
    const int ks = (int)(dp / 32), ksr = (int)(rp / 32);
    const int nsplit = clr_split(rp), grid = (int)((M + bm - 1) / bm);
    const int block = 64 * CLR_WAVES;
    const size_t lds = clr_lds(bm, dp, rp, nsplit);
    CROSS_LAUNCH(k_cross_lr_bwd, (const uint16_t*)x0, (const uint16_t*)us,
               (const uint16_t*)utimg, (const uint16_t*)vtimg, (int)M, (int)d,
               ks, (int)r, ksr, nsplit, (int)L, dout, (const uint16_t*)w_out,
               (const uint16_t*)gl, (uint16_t*)qs, (uint16_t*)ss,
               (uint16_t*)dx0);
}

}  // extern "C"
