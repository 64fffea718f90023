// DLRM pairwise dot interaction (gfx950 / MI355X), forward and backward,
// one launch each way.
//
// Per sample, v_0 = x (the bottom-MLP output, [D]) and v_1 .. v_F are the
// embedding rows; T = F + 1 <= 32. The output row is
//   out[c]                     = x[c]                 c < D
//   out[D + i(i-1)/2 + j]      = <v_i, v_j>           0 <= j < i < T
//   zeros up to the row stride W (ceil32 of the above when padded),
// the order of torch.tril_indices(T, T, -1). x and e are rounded to bf16
// (nearest even) once; the rounded values are the operands of every dot and
// of the backward, sums are fp32 (mfma_f32_16x16x32_bf16), the output is
// rounded once to its dtype. Columns c < D carry the UNROUNDED x.
//
// Backward, from g = d_out (fp32 is rounded to bf16 once):
//   S[i][j] = S[j][i] = g[D + i(i-1)/2 + j], zero diagonal,  dV = S * V,
//   de[f] = dV[f + 1],  dx = dV[0] + g[:D].
//
// Work split: one wave per sample, S_blk = blockDim.x / 64 consecutive
// samples per block. The block's span of e (S_blk * F * D floats) is
// contiguous: it is fetched in 16-byte pieces, DOT_U loads of a thread in
// flight, converted and scattered into the per-sample LDS tiles. Outputs
// (the out rows, de) are composed in an LDS image of the block's
// contiguous output span and leave in 16-byte pieces.
//
// Forward tile: V as [32][Dp + 8] bf16, Dp = ceil32(D), rows T..31 and
// columns D..Dp-1 zero. For V * V^T a lane's A fragment of rows r..r+15
// and its B fragment of columns r..r+15 are the same 16 bytes (lane & 15 =
// row or column, (lane >> 4) * 8 = first of eight consecutive k): a row
// tile is read from LDS once per k-step and serves as both operands. Only
// tiles (0,0), (1,0), (1,1) are computed, the last two when T > 16.
//
// Backward tile: dV = S * V contracts over the VECTOR index, so the B
// operand wants V column-wise. The backward never needs V row-wise, so it
// stages V transposed from the start, Vt as [Dp][32 + 8] bf16, with the
// same 2-byte scatter stores that an odd D needs anyway; a B fragment is
// then the same plain 16-byte row read as everywhere else (no transposing
// LDS read with its all-lanes-active and alignment preconditions). S is a
// [32][32 + 8] bf16 matrix in LDS, every element written exactly once.
//
// Row strides Dp + 8 and 40 elements are 20, 36, 52, 68 dwords, each with
// gcd(stride, 64) = 4: the 16 rows of a fragment read start on 16 distinct
// 4-bank groups, and a lane reads exactly 4 banks.
//
// No atomics: every output element is written exactly once, both kernels
// are bitwise reproducible. All index math is 32-bit (the launcher refuses
// B*F*D or B*W >= 2^31); row/column of a flat element come from one
// multiply by a host-computed reciprocal, exact for i < 4096 (see
// dot_magic), never from a division.
//
// Fragment maps as in mlp.hip: A[m][k]: m = lane&15, k = (lane>>4)*8 + e;
// B[k][n]: n = lane&15, same k; C: col = lane&15, row = (lane>>4)*4 + r.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

typedef __hip_bfloat16 bf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define DOT_U 4              // 16-byte loads in flight per thread
#define DOT_PAD 8             // elements behind a tile row (16 bytes)
#define DOT_SLD (32 + DOT_PAD)  // row stride of S and of Vt
#define DOT_S_MAX 4           // samples (= waves) per block, at most
#define DOT_LDS_MAX 65536     // dynamic LDS per block

static __device__ __forceinline__ uint16_t dot_bits(bf16 v) {
    return __bfloat16_as_ushort(v);
}
static __device__ __forceinline__ uint16_t dot_bits(float v) {
    return __bfloat16_as_ushort((bf16)v);   // round to nearest even
}
static __device__ __forceinline__ float dot_rounded(float v) {
    return __bfloat162float((bf16)v);
}
static __device__ __forceinline__ float dot_rounded(bf16 v) {
    return __bfloat162float(v);
}

// element i of the block's e span -> (sample, row f, column c) -> its tile.
// TRANS: Vt[c][f + 1], else V[f + 1][c].
template <bool TRANS>
static __device__ __forceinline__ uint16_t* dot_slot(uint16_t* tiles,
                                                     int tile_elems, int ld,
                                                     int i, int R, int D,
                                                     unsigned magic) {
    while (i >= R) {          // at most DOT_S_MAX - 1 rounds
        i -= R;
        tiles += tile_elems;
    }
    const int f = (int)(((unsigned)i * magic) >> 20);
    const int c = i - f * D;
    return tiles + (TRANS ? c * ld + f + 1 : (f + 1) * ld + c);
}

// The block's span of e (total floats at ge) -> bf16 in the tiles. Whole
// 16-byte chunks move as uint4, DOT_U per thread issued back to back (a
// thread past the end re-reads the last whole chunk instead of branching);
// the fewer than four floats on either ragged edge move one by one. When a
// chunk cannot straddle a row (D % 4 == 0, aligned span) and the tile is
// row-major, its four values leave as one 8-byte LDS store.
template <bool TRANS>
static __device__ __forceinline__ void dot_stage_v(const float* ge, int total,
                                                   uint16_t* tiles,
                                                   int tile_elems, int ld,
                                                   int R, int D,
                                                   unsigned magic) {
    const int mis = (int)(((uintptr_t)ge & 15) >> 2);
    const int head = min((4 - mis) & 3, total);
    const int nq = (total - head) >> 2;
    const uint4* gq = (const uint4*)(ge + head);
    const int bd = blockDim.x;
    const bool rowwise = !TRANS && head == 0 && (D & 3) == 0;
    for (int q0 = threadIdx.x; q0 < nq; q0 += DOT_U * bd) {
        uint4 v[DOT_U];
        #pragma unroll
        for (int u = 0; u < DOT_U; ++u)
            v[u] = gq[min(q0 + u * bd, nq - 1)];
        #pragma unroll
        for (int u = 0; u < DOT_U; ++u) {
            const int q = q0 + u * bd;
            if (q >= nq) break;
            const float f0 = __uint_as_float(v[u].x);
            const float f1 = __uint_as_float(v[u].y);
            const float f2 = __uint_as_float(v[u].z);
            const float f3 = __uint_as_float(v[u].w);
            const int i = head + 4 * q;
            if (rowwise) {
                uint2 p;
                p.x = dot_bits(f0) | ((uint32_t)dot_bits(f1) << 16);
                p.y = dot_bits(f2) | ((uint32_t)dot_bits(f3) << 16);
                *(uint2*)dot_slot<TRANS>(tiles, tile_elems, ld, i, R, D,
                                         magic) = p;
            } else {
                *dot_slot<TRANS>(tiles, tile_elems, ld, i, R, D, magic)
                    = dot_bits(f0);
                *dot_slot<TRANS>(tiles, tile_elems, ld, i + 1, R, D, magic)
                    = dot_bits(f1);
                *dot_slot<TRANS>(tiles, tile_elems, ld, i + 2, R, D, magic)
                    = dot_bits(f2);
                *dot_slot<TRANS>(tiles, tile_elems, ld, i + 3, R, D, magic)
                    = dot_bits(f3);
            }
        }
    }
    const int t = threadIdx.x;
    if (t < head)
        *dot_slot<TRANS>(tiles, tile_elems, ld, t, R, D, magic)
            = dot_bits(ge[t]);
    const int tail = head + 4 * nq + t;
    if (tail < total)
        *dot_slot<TRANS>(tiles, tile_elems, ld, tail, R, D, magic)
            = dot_bits(ge[tail]);
}

// LDS image -> global bytes [lo, hi) of the 16-byte chunk space based at
// gb (gb is 16-byte aligned; the image has the span's offset inside its
// first chunk, so chunk q is bytes [16q, 16q + 16) of both). Whole chunks
// as uint4, the ragged edges element by element.
template <int ESZ>
static __device__ __forceinline__ void dot_stage_out(const char* lds,
                                                     char* gb, int lo,
                                                     int hi) {
    const int q_lo = (lo + 15) >> 4, q_hi = hi >> 4;
    for (int q = q_lo + threadIdx.x; q < q_hi; q += blockDim.x)
        *(uint4*)(gb + 16 * q) = *(const uint4*)(lds + 16 * q);
    const int head_end = min(16 * q_lo, hi);
    const int tail = max(16 * q_hi, head_end);
    const int t = threadIdx.x * ESZ;
    if (lo + t < head_end) {
        if (ESZ == 4)
            *(uint32_t*)(gb + lo + t) = *(const uint32_t*)(lds + lo + t);
        else
            *(uint16_t*)(gb + lo + t) = *(const uint16_t*)(lds + lo + t);
    }
    if (tail + t < hi) {
        if (ESZ == 4)
            *(uint32_t*)(gb + tail + t) = *(const uint32_t*)(lds + tail + t);
        else
            *(uint16_t*)(gb + tail + t) = *(const uint16_t*)(lds + tail + t);
    }
}

static __device__ __forceinline__ bf16x8 dot_frag(const uint16_t* p) {
    return *reinterpret_cast<const bf16x8*>(__builtin_assume_aligned(p, 16));
}

// ---- forward ----------------------------------------------------------
// KS = Dp / 32 k-steps. LDS: S_blk tiles of 32 * (Dp + 8) bf16, then the
// image of the block's out rows.
template <typename OutT, int KS>
__global__ __launch_bounds__(64 * DOT_S_MAX)
void k_dot_interact_fwd(const float* __restrict__ e,
                        const float* __restrict__ x,
                        OutT* __restrict__ out, int B, int F, int D, int W,
                        unsigned magic) {
    extern __shared__ uint4 dot_smem[];
    constexpr int LD = 32 * KS + DOT_PAD;
    constexpr int TILE = 32 * LD;
    const int S = blockDim.x >> 6;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint16_t* const tiles = (uint16_t*)dot_smem;
    char* const img = (char*)(tiles + S * TILE);
    const int T = F + 1, R = F * D;
    const int b0 = blockIdx.x * S;
    const int n = min(S, B - b0);
    const float* ge = e + (size_t)b0 * R;
    OutT* go = out + (size_t)b0 * W;
    const int mis_o = (int)((uintptr_t)go & 15);
    const bool live = wave < n;
    const bool two = T > 16;              // second row tile in use
    uint16_t* const tile = tiles + wave * TILE;
    OutT* const o = (OutT*)(img + mis_o) + wave * W;

    if (live) {
        // x: row 0 of the tile (rounded) and the front of the out row
        // (cast of the unrounded value); its loads travel with e's
        const float* gx = x + (size_t)(b0 + wave) * D;
        for (int c = lane; c < D; c += 64) {
            const float xv = gx[c];
            tile[c] = dot_bits(xv);
            o[c] = (OutT)xv;
        }
        // zeros nobody else writes: columns D..Dp-1 of the live rows, the
        // rows T.. of the row tiles in use, the tail of the out row
        if (lane < T)
            for (int c = D; c < 32 * KS; ++c) tile[lane * LD + c] = 0;
        if ((lane & 15) < 4 * KS)
            for (int r = T + (lane >> 4); r < (two ? 32 : 16); r += 4)
                *(uint4*)(tile + r * LD + (lane & 15) * 8)
                    = make_uint4(0, 0, 0, 0);
        for (int j = D + ((T * (T - 1)) >> 1) + lane; j < W; j += 64)
            o[j] = (OutT)0.0f;
    }
    dot_stage_v<false>(ge, n * R, tiles, TILE, LD, R, D, magic);
    __syncthreads();

    if (live) {                           // wave-uniform: EXEC is full
        const uint16_t* p0 = tile + (lane & 15) * LD + (lane >> 4) * 8;
        f32x4 a00 = {0.f, 0.f, 0.f, 0.f}, a10 = a00, a11 = a00;
        #pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 f0 = dot_frag(p0 + 32 * ks);
            a00 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f0, f0, a00,
                                                          0, 0, 0);
            if (two) {
                const bf16x8 f1 = dot_frag(p0 + 16 * LD + 32 * ks);
                a10 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f1, f0, a10,
                                                              0, 0, 0);
                a11 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f1, f1, a11,
                                                              0, 0, 0);
            }
        }
        // the strictly lower triangle -> the image of the out row
        const int jc = lane & 15, i0 = (lane >> 4) * 4;
        #pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q;
            if (jc < i && i < T)
                o[D + ((i * (i - 1)) >> 1) + jc] = (OutT)a00[q];
        }
        if (two) {
            #pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = 16 + i0 + q;
                const int row = D + ((i * (i - 1)) >> 1);
                if (i < T) {
                    o[row + jc] = (OutT)a10[q];
                    if (16 + jc < i) o[row + 16 + jc] = (OutT)a11[q];
                }
            }
        }
    }
    __syncthreads();
    dot_stage_out<(int)sizeof(OutT)>(img, (char*)go - mis_o, mis_o,
                                     mis_o + n * W * (int)sizeof(OutT));
}

// ---- backward ---------------------------------------------------------
// LDS: S_blk transposed tiles Vt [Dp][40], S_blk matrices S [32][40], then
// the image of the block's de rows. 2 * Dp/16 MFMAs per sample (half of
// them when T <= 16), one k-step each.
template <typename GT, int KS>
__global__ __launch_bounds__(64 * DOT_S_MAX)
void k_dot_interact_bwd(const float* __restrict__ e,
                        const float* __restrict__ x,
                        const GT* __restrict__ g, float* __restrict__ de,
                        float* __restrict__ dx, int B, int F, int D, int W,
                        unsigned magic) {
    extern __shared__ uint4 dot_smem[];
    constexpr int DP = 32 * KS;
    constexpr int VT = DP * DOT_SLD;
    constexpr int SM = 32 * DOT_SLD;
    const int S = blockDim.x >> 6;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint16_t* const vts = (uint16_t*)dot_smem;
    uint16_t* const sms = vts + S * VT;
    char* const img = (char*)(sms + S * SM);
    const int T = F + 1, R = F * D;
    const int b0 = blockIdx.x * S;
    const int n = min(S, B - b0);
    const float* ge = e + (size_t)b0 * R;
    float* gd = de + (size_t)b0 * R;
    const int mis_d = (int)((uintptr_t)gd & 15);
    const bool live = wave < n;
    const bool two = T > 16;
    uint16_t* const vt = vts + wave * VT;
    uint16_t* const sm = sms + wave * SM;
    float* const im = (float*)(img + mis_d) + wave * R;
    const GT* gr = g + (size_t)(b0 + wave) * W;   // used when live

    if (live) {
        // S: lane = (row parity, column), rows i = 2 * it + (lane >> 5).
        // All 16 loads are issued first (an index outside the triangle is
        // clamped to its first element, which exists: T >= 2). The lane
        // below the diagonal writes its value on both sides, the lane on
        // it the zero: each of the 32 x 32 elements is written once.
        const int j = lane & 31, half = lane >> 5;
        uint16_t gv[16];
        #pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int i = 2 * it + half;
            const bool ok = j < i && i < T;
            gv[it] = dot_bits((bf16)gr[D + (ok ? ((i * (i - 1)) >> 1) + j
                                               : 0)]);
        }
        #pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int i = 2 * it + half;
            const uint16_t v = i < T ? gv[it] : (uint16_t)0;
            if (j < i) {
                sm[i * DOT_SLD + j] = v;
                sm[j * DOT_SLD + i] = v;
            } else if (j == i) {
                sm[i * DOT_SLD + i] = 0;
            }
        }
        // Vt: x in column 0, zeros in the columns T..31 of the live rows
        // and in the rows D..Dp-1
        const float* gx = x + (size_t)(b0 + wave) * D;
        for (int d = lane; d < DP; d += 64) {
            uint16_t* row = vt + d * DOT_SLD;
            if (d < D) {
                row[0] = dot_bits(gx[d]);
                for (int jj = T; jj < 32; ++jj) row[jj] = 0;
            } else {
                #pragma unroll
                for (int q = 0; q < 4; ++q)
                    ((uint4*)row)[q] = make_uint4(0, 0, 0, 0);
            }
        }
    }
    dot_stage_v<true>(ge, n * R, vts, VT, DOT_SLD, R, D, magic);
    __syncthreads();

    if (live) {                           // wave-uniform: EXEC is full
        const int r = lane & 15, k0 = (lane >> 4) * 8, i0 = (lane >> 4) * 4;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        const bf16x8 s0 = dot_frag(sm + r * DOT_SLD + k0);
        const bf16x8 s1 = dot_frag(sm + (two ? 16 + r : r) * DOT_SLD + k0);
        #pragma unroll
        for (int nt = 0; nt < 2 * KS; ++nt) {
            const bf16x8 vb = dot_frag(vt + (16 * nt + r) * DOT_SLD + k0);
            const f32x4 c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                s0, vb, zero, 0, 0, 0);
            f32x4 c1 = zero;
            if (two)
                c1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(s1, vb, zero,
                                                             0, 0, 0);
            const int d = 16 * nt + r;
            if (d < D) {
                #pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = i0 + q;
                    if (i == 0)
                        dx[(size_t)(b0 + wave) * D + d]
                            = c0[q] + dot_rounded(gr[d]);
                    else if (i < T)
                        im[(i - 1) * D + d] = c0[q];
                    if (two && 16 + i < T) im[(15 + i) * D + d] = c1[q];
                }
            }
        }
    }
    __syncthreads();
    dot_stage_out<4>(img, (char*)gd - mis_d, mis_d, mis_d + n * R * 4);
}

// ---- launchers --------------------------------------------------------

extern "C" {

static long dot_ceil32(long v) { return (v + 31) / 32 * 32; }

// bytes of the LDS image of S rows of row_bytes each: whole 16-byte chunks
// plus one for the span's offset inside its first chunk
static long dot_img_bytes(long S, long row_bytes) {
    return (S * row_bytes + 15) / 16 * 16 + 16;
}

// ceil(2^20 / D): (i * magic) >> 20 == i / D for 0 <= i < 4096, D <= 128.
// With magic * D = 2^20 + r, 0 <= r < D, the product overshoots i / D by
// i * r / (D * 2^20) < 2^-8, less than the 1 / D >= 2^-7 that separates
// i / D from the next integer; i * magic < 31 * 2^20 + 4096 fits 32 bits.
static unsigned dot_magic(long D) {
    return (unsigned)(((1L << 20) + D - 1) / D);
}

// columns of an out row: D + T(T-1)/2, 32-padded on request
long emb_dot_interact_width(long F, long D, int pad32) {
    const long w = D + (F + 1) * F / 2;
    return pad32 ? dot_ceil32(w) : w;
}

static long dot_lds_bytes(long S, long F, long D, long W, long esz,
                          int bwd) {
    const long Dp = dot_ceil32(D);
    if (bwd)
        return S * (Dp + 32) * DOT_SLD * 2 + dot_img_bytes(S, F * D * 4);
    return S * 32 * (Dp + DOT_PAD) * 2 + dot_img_bytes(S, W * esz);
}

// Samples (= waves) per block, or 0 when the shape is outside the kernels:
// the largest power of two up to DOT_S_MAX whose tiles and image fit
// DOT_LDS_MAX. esz: bytes of an out / d_out element.
int emb_dot_interact_waves(long B, long F, long D, long W, long esz,
                           int bwd) {
    if (F < 1 || F > 31 || D < 1 || D > 128 || B < 0) return 0;
    if (B * F * D >= (1L << 31) || B * W >= (1L << 31)) return 0;
    for (int S = DOT_S_MAX; S >= 1; S >>= 1)
        if (dot_lds_bytes(S, F, D, W, esz, bwd) <= DOT_LDS_MAX) return S;
    return 0;
}

#define DOT_LAUNCH(kernel, ET, ...)                                         \
    switch (KS) {                                                           \
    case 1: kernel<ET, 1><<<grid, 64 * S, lds, stream>>>(__VA_ARGS__);      \
        break;                                                              \
    case 2: kernel<ET, 2><<<grid, 64 * S, lds, stream>>>(__VA_ARGS__);      \
        break;                                                              \
    case 3: kernel<ET, 3><<<grid, 64 * S, lds, stream>>>(__VA_ARGS__);      \
        break;                                                              \
    default: kernel<ET, 4><<<grid, 64 * S, lds, stream>>>(__VA_ARGS__);     \
        break;                                                              \
    }

// S from emb_dot_interact_waves(.., 0), > 0
void emb_dot_interact_fwd(const float* e, const float* x, void* out, long B,
                          long F, long D, long W, int out_bf16, int S,
                          hipStream_t stream) {
    if (B == 0) return;
    const int KS = (int)(dot_ceil32(D) / 32);
    const long lds = dot_lds_bytes(S, F, D, W, out_bf16 ? 2 : 4, 0);
    const int grid = (int)((B + S - 1) / S);
    const unsigned magic = dot_magic(D);
    if (out_bf16) {
        DOT_LAUNCH(k_dot_interact_fwd, bf16, e, x, (bf16*)out, (int)B,
                   (int)F, (int)D, (int)W, magic)
    } else {
        DOT_LAUNCH(k_dot_interact_fwd, float, e, x, (float*)out, (int)B,
                   (int)F, (int)D, (int)W, magic)
    }
}

// S from emb_dot_interact_waves(.., 1), > 0
void emb_dot_interact_bwd(const float* e, const float* x, const void* g,
                          float* de, float* dx, long B, long F, long D,
                          long W, int g_bf16, int S, hipStream_t stream) {
    if (B == 0) return;
    const int KS = (int)(dot_ceil32(D) / 32);
    const long lds = dot_lds_bytes(S, F, D, W, g_bf16 ? 2 : 4, 1);
    const int grid = (int)((B + S - 1) / S);
    const unsigned magic = dot_magic(D);
    if (g_bf16) {
        DOT_LAUNCH(k_dot_interact_bwd, bf16, e, x, (const bf16*)g, de, dx,
                   (int)B, (int)F, (int)D, (int)W, magic)
    } else {
        DOT_LAUNCH(k_dot_interact_bwd, float, e, x, (const float*)g, de, dx,
                   (int)B, (int)F, (int)D, (int)W, magic)
    }
}

}  // extern "C"
