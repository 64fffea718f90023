// Fused CTR interaction head (gfx950 / MI355X).
//
// The DeepFM/WDL "glue" between the embedding gather and the MLP GEMMs was
// ~320 us/step of small elementwise/reduce kernels + ~110 us of autocast
// casts (profiles/bench_deepfm_1gpu_kernels.md). These two kernels fuse, in
// one pass over the gathered rows:
//
//   forward:  e_all [B, F, D1] (D1 = dim+1: dim embedding cols + the merged
//             first-order/"wide" column — see models/ctr.py) and dense
//             [B, ND] ->
//               deep_in  bf16 [B, F*dim + ND]   (cast fused into the write)
//               partial  f32  [B] = sum_f e[.,dim]            (first order)
//                              + 0.5*sum_d((sum_f e)^2 - sum_f e^2)  (FM)
//                              + dense @ w + b             (dense linear)
//   backward: d_deep_in bf16, d_partial f32 ->
//               de_all f32 (FM + first-order + deep contributions),
//               d_dense f32, dw/db accumulated with atomics.
//
// One 64-lane wave per sample; lane c covers column c of the row (D1 <= 64
// enforced host-side), so the per-field row load is one coalesced segment.
// Reference math: DeepFM second order 0.5*((sum e)^2 - sum e^2) — the same
// formula the TF/DeepCTR models of the reference benchmark compute
// (test/benchmark/criteo_deepctr.py DeepFM).

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

typedef long long i64;
typedef unsigned long long u64;
typedef __hip_bfloat16 bf16;

// lanes c < dim: embedding columns; lane dim: wide column; F fields.
// use_fm: 0 for WDL/LR-style heads.
template <typename OutT>
__global__ void k_ctr_head_fwd(const float* __restrict__ e_all,
                               const float* __restrict__ dense,
                               const float* __restrict__ w,  // [nd]
                               const float* __restrict__ bias,  // [1]
                               long B, long F, long dim, long nd,
                               long out_stride,
                               OutT* __restrict__ deep_in,
                               float* __restrict__ partial,
                               float* __restrict__ s_out,  // [B, dim] for bwd
                               int use_fm) {
    const long D1 = dim + 1;
    const int lane = threadIdx.x & 63;
    const long b = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (b >= B) return;
    const float* e = e_all + b * F * D1;
    OutT* di = deep_in + b * out_stride;
    // zero the alignment pad tail (the fused MLP reads 16-byte fragments)
    for (long j = F * dim + nd + lane; j < out_stride; j += 64)
        di[j] = (OutT)0.0f;

    // lane covers columns lane and lane+64 (D1 <= 128 — covers the
    // reference's dim-64 benchmark config, D1 = 65)
    float s[2] = {0.0f, 0.0f}, sq[2] = {0.0f, 0.0f};
    for (long f = 0; f < F; ++f) {
        #pragma unroll
        for (int t = 0; t < 2; ++t) {
            const long cc = lane + 64 * t;
            if (cc >= D1) break;
            float v = e[f * D1 + cc];
            if (cc < dim) {
                s[t] += v;
                sq[t] += v * v;
                di[f * dim + cc] = (OutT)v;
            } else {
                s[t] += v;                // first-order (wide) column
            }
        }
    }
    // dense tail: cast + dot
    float dsum = 0.0f;
    for (long j = lane; j < nd; j += 64) {
        float v = dense[b * nd + j];
        di[F * dim + j] = (OutT)v;
        dsum += v * w[j];
    }
    float fm = 0.0f, lin = 0.0f;
    #pragma unroll
    for (int t = 0; t < 2; ++t) {
        const long cc = lane + 64 * t;
        if (cc >= D1) break;
        if (cc < dim) {
            if (use_fm) fm += s[t] * s[t] - sq[t];
            if (s_out) s_out[b * dim + cc] = s[t];
        } else {
            lin = s[t];
        }
    }
    float acc = 0.5f * fm + lin + dsum;
    for (int off = 32; off; off >>= 1)
        acc += __shfl_down(acc, off, 64);
    if (lane == 0) partial[b] = acc + bias[0];
}

// backward, fully parallel: one thread per element of de_all [B, F, D1]
// (the wave-per-sample version serialized F iterations over ~D1 active
// lanes and measured 69 us/step; with s saved by the forward this is a pure
// elementwise pass at memory speed).
template <typename OutT>
__global__ void k_ctr_head_bwd_e(const float* __restrict__ e_all,
                                 const OutT* __restrict__ d_deep_in,
                                 const float* __restrict__ d_partial,
                                 const float* __restrict__ s_in, // [B, dim]
                                 long B, long F, long dim,
                                 long nd, long out_stride,
                                 float* __restrict__ de_all,
                                 int use_fm,
                                 float* __restrict__ dw,
                                 float* __restrict__ db) {
    const long D1 = dim + 1;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    // zero the tiny dense-linear grad accumulators consumed by the
    // bwd_d kernel that follows on this stream (two torch::zeros
    // allocations were ~4 us of launch each for ~56 bytes)
    if (i < nd) dw[i] = 0.0f;
    if (i == nd) *db = 0.0f;
    if (i >= B * F * D1) return;
    const long c = i % D1;
    const long f = (i / D1) % F;
    const long b = i / (D1 * F);
    const float gp = d_partial[b];
    if (c == dim) { de_all[i] = gp; return; }        // wide column
    float g = (float)d_deep_in[b * out_stride + f * dim + c];
    if (use_fm) g += gp * (s_in[b * dim + c] - e_all[i]);
    de_all[i] = g;
}

// dense tail, one thread per (sample, feature): coalesced d_dense/dense/
// d_deep_in traffic, dw/db via LDS block partials then nd+1 global atomics
// per block (the thread-per-sample version had only B/256 blocks in flight
// and measured 34.6 us; this shape is ~population-bound).
#define ND_MAX 32
template <typename OutT>
__global__ void k_ctr_head_bwd_d(const float* __restrict__ dense,
                                 const float* __restrict__ w,
                                 const OutT* __restrict__ d_deep_in,
                                 const float* __restrict__ d_partial,
                                 long B, long F, long dim, long nd,
                                 long out_stride,
                                 float* __restrict__ d_dense,
                                 float* __restrict__ dw,   // [nd] atomic
                                 float* __restrict__ db) { // [1] atomic
    __shared__ float lacc[ND_MAX + 1];
    for (int t = threadIdx.x; t < nd + 1; t += blockDim.x) lacc[t] = 0.0f;
    __syncthreads();
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * nd) {
        const long b = i / nd;
        const long j = i % nd;
        const float gp = d_partial[b];
        const float dv = dense[i];
        d_dense[i] = (float)d_deep_in[b * out_stride + F * dim + j]
                     + gp * w[j];
        atomicAdd(&lacc[j], gp * dv);
        if (j == 0) atomicAdd(&lacc[nd], gp);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nd + 1; t += blockDim.x) {
        if (t < nd) atomicAdd(&dw[t], lacc[t]);
        else atomicAdd(db, lacc[nd]);
    }
}

// ---- row-staged kernels -------------------------------------------------
//
// One wave per sample, S = blockDim.x / 64 consecutive samples per block.
// The block's span of e_all (S * F * D1 floats, contiguous) is fetched into
// LDS in 16-byte pieces, every load of a thread issued before the first is
// waited on; the per-field work then runs out of LDS, and the outputs
// (deep_in / de_all) are composed in LDS and leave in 16-byte pieces too.
//
// Alignment: an LDS image is laid out with the same offset inside a 16-byte
// chunk as its global span ("mis"), so chunk q of the image is bytes
// [16q, 16q + 16) of both; a chunk that lies wholly inside the span moves
// as one uint4, the bytes on the ragged edges (fewer than 16 on either
// side) move element by element. All indices are 32-bit; the launcher sends shapes whose
// B * F * D1 or B * stride reach 2^31 to the per-field kernels.

#define ROWS_U 4              // 16-byte loads in flight per thread
#define ROWS_LDS_MAX 65280    // dynamic LDS per block (64 KiB less lacc)

// bytes [lo, hi) of the chunk space that lie outside the whole chunks
// q_lo .. q_hi - 1: fewer than 16 on either side, element by element
template <int ESZ>
__device__ __forceinline__ void rows_copy_edges(const char* src, char* dst,
                                                int lo, int hi, int q_lo,
                                                int q_hi) {
    const int head_end = min(16 * q_lo, hi);
    const int tail = max(16 * q_hi, head_end);
    const int t = threadIdx.x * ESZ;
    if (lo + t < head_end) {
        if (ESZ == 4)
            *(uint32_t*)(dst + lo + t) = *(const uint32_t*)(src + lo + t);
        else
            *(uint16_t*)(dst + lo + t) = *(const uint16_t*)(src + lo + t);
    }
    if (tail + t < hi) {
        if (ESZ == 4)
            *(uint32_t*)(dst + tail + t) = *(const uint32_t*)(src + tail + t);
        else
            *(uint16_t*)(dst + tail + t) = *(const uint16_t*)(src + tail + t);
    }
}

// ROWS_U whole chunks per thread, i0 + u * blockDim.x of n_full. The load
// of a thread that has run out of chunks is clamped to the last whole
// chunk instead of branched around (only a block-uniform branch skips a
// round nobody needs), so the loads are issued back to back.
__device__ __forceinline__ void rows_load(const char* g0, int n_full, int i0,
                                          uint4 (&v)[ROWS_U]) {
    const int i_blk = i0 - threadIdx.x;             // block-uniform
    const int bd = blockDim.x;
    #pragma unroll
    for (int u = 0; u < ROWS_U; ++u) {
        v[u] = make_uint4(0, 0, 0, 0);
        if (i_blk + u * bd < n_full)
            v[u] = *(const uint4*)(g0 + 16 * min(i0 + u * bd, n_full - 1));
    }
}

// keeps the loads above the LDS stores: without it the compiler sinks each
// load into its store's branch and waits once per load
__device__ __forceinline__ void rows_hold(uint4 (&v)[ROWS_U]) {
    #pragma unroll
    for (int u = 0; u < ROWS_U; ++u)
        asm volatile("" : "+v"(v[u].x), "+v"(v[u].y), "+v"(v[u].z),
                     "+v"(v[u].w));
}

__device__ __forceinline__ void rows_store(char* l0, int n_full, int i0,
                                           const uint4 (&v)[ROWS_U]) {
    const int bd = blockDim.x;
    #pragma unroll
    for (int u = 0; u < ROWS_U; ++u)
        if (i0 + u * bd < n_full)
            *(uint4*)(l0 + 16 * (i0 + u * bd)) = v[u];
}

// global bytes [lo, hi) of the chunk space based at gb -> the LDS image
template <int ESZ>
__device__ __forceinline__ void rows_stage_in(const char* gb, char* lds,
                                              int lo, int hi) {
    const int q_lo = (lo + 15) >> 4, q_hi = hi >> 4;
    const int n_full = q_hi - q_lo;
    for (int i0 = threadIdx.x; i0 < n_full; i0 += ROWS_U * blockDim.x) {
        uint4 v[ROWS_U];
        rows_load(gb + 16 * q_lo, n_full, i0, v);
        rows_hold(v);
        rows_store(lds + 16 * q_lo, n_full, i0, v);
    }
    rows_copy_edges<ESZ>(gb, lds, lo, hi, q_lo, q_hi);
}

// two spans at once, the loads of both issued before either is stored
template <int ESZ_A, int ESZ_B>
__device__ __forceinline__ void rows_stage_in2(const char* gb_a, char* lds_a,
                                               int lo_a, int hi_a,
                                               const char* gb_b, char* lds_b,
                                               int lo_b, int hi_b) {
    const int qa = (lo_a + 15) >> 4, na = (hi_a >> 4) - qa;
    const int qb = (lo_b + 15) >> 4, nb = (hi_b >> 4) - qb;
    for (int i0 = threadIdx.x; i0 < max(na, nb);
         i0 += ROWS_U * blockDim.x) {
        uint4 va[ROWS_U], vb[ROWS_U];
        rows_load(gb_a + 16 * qa, na, i0, va);
        rows_load(gb_b + 16 * qb, nb, i0, vb);
        rows_hold(va);
        rows_hold(vb);
        rows_store(lds_a + 16 * qa, na, i0, va);
        rows_store(lds_b + 16 * qb, nb, i0, vb);
    }
    rows_copy_edges<ESZ_A>(gb_a, lds_a, lo_a, hi_a, qa, hi_a >> 4);
    rows_copy_edges<ESZ_B>(gb_b, lds_b, lo_b, hi_b, qb, hi_b >> 4);
}

// the LDS image -> global bytes [lo, hi) of the chunk space based at gb
template <int ESZ>
__device__ __forceinline__ void rows_stage_out(const char* lds, char* gb,
                                               int lo, int hi) {
    const int q_lo = (lo + 15) >> 4, q_hi = hi >> 4;
    for (int q = q_lo + threadIdx.x; q < q_hi; q += blockDim.x)
        *(uint4*)(gb + 16 * q) = *(const uint4*)(lds + 16 * q);
    rows_copy_edges<ESZ>(lds, gb, lo, hi, q_lo, q_hi);
}

// Forward. s, sq and the first-order sum are taken in field order, one
// fp32 add per field, and the lane value 0.5*fm + lin + dsum enters the
// same 64-lane tree as in k_ctr_head_fwd: deep_in, s and partial are bit
// for bit what that kernel writes.
template <typename OutT>
__global__ void k_ctr_head_fwd_rows(const float* __restrict__ e_all,
                                    const float* __restrict__ dense,
                                    const float* __restrict__ w,
                                    const float* __restrict__ bias,
                                    int B, int F, int dim, int nd,
                                    int out_stride,
                                    OutT* __restrict__ deep_in,
                                    float* __restrict__ partial,
                                    float* __restrict__ s_out,
                                    int use_fm, int img_b, int p_shift) {
    extern __shared__ uint4 rows_smem[];
    char* const img_e = (char*)rows_smem;
    char* const img_o = img_e + img_b;
    const int S = blockDim.x >> 6;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D1 = dim + 1, R = F * D1;
    const int c0 = p_shift < 6 ? lane & ((1 << p_shift) - 1) : lane;
    const int f_first = p_shift < 6 ? lane >> p_shift : 0;
    const int f_step = p_shift < 6 ? 64 >> p_shift : 1;
    const int b0 = blockIdx.x * S;
    const int n = min(S, B - b0);
    const float* ge = e_all + (size_t)b0 * R;
    OutT* go = deep_in + (size_t)b0 * out_stride;
    const int mis_e = (int)((uintptr_t)ge & 15);
    const int mis_o = (int)((uintptr_t)go & 15);
    const int b = b0 + wave;
    const bool live = wave < n;

    // the dense tail's operands travel with the row loads
    float dv = 0.0f, wv = 0.0f;
    if (live && lane < nd) {
        dv = dense[(size_t)b * nd + lane];
        wv = w[lane];
    }
    rows_stage_in<4>((const char*)ge - mis_e, img_e, mis_e,
                     mis_e + n * R * 4);
    __syncthreads();

    if (live) {
        const float* e = (const float*)(img_e + mis_e) + wave * R;
        OutT* o = (OutT*)(img_o + mis_o) + wave * out_stride;
        float s[2] = {0.0f, 0.0f}, sq[2] = {0.0f, 0.0f};
        #pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int cc = lane + 64 * t;
            if (cc >= D1) break;
            const bool emb = cc < dim;
            // 8 LDS reads in flight, consumed in field order
            for (int f0 = 0; f0 < F; f0 += 8) {
                float v[8];
                #pragma unroll
                for (int u = 0; u < 8; ++u)
                    v[u] = e[min(f0 + u, F - 1) * D1 + cc];
                #pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (f0 + u >= F) break;
                    s[t] += v[u];
                    if (emb) sq[t] += v[u] * v[u];
                }
            }
        }
        // deep_in's embedding columns: cast and compaction (D1 -> dim
        // columns per field) with all lanes busy, lane = (field, column) as
        // in the backward — the field loop above has D1 of 64 lanes active
        // and is kept to the three operations whose order is fixed
        #pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int c = c0 + 64 * t;
            if (c >= dim) break;
            for (int f = f_first; f < F; f += 4 * f_step) {
                float v[4];
                #pragma unroll
                for (int u = 0; u < 4; ++u)
                    v[u] = e[min(f + u * f_step, F - 1) * D1 + c];
                #pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (f + u * f_step < F)
                        o[(f + u * f_step) * dim + c] = (OutT)v[u];
            }
        }
        // dense tail (nd <= ND_MAX < 64: one feature per lane), zero pad
        float dsum = 0.0f;
        if (lane < nd) {
            o[F * dim + lane] = (OutT)dv;
            dsum += dv * wv;
        }
        for (int j = F * dim + nd + lane; j < out_stride; j += 64)
            o[j] = (OutT)0.0f;
        float fm = 0.0f, lin = 0.0f;
        #pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int cc = lane + 64 * t;
            if (cc >= D1) break;
            if (cc < dim) {
                if (use_fm) fm += s[t] * s[t] - sq[t];
                if (s_out) s_out[(size_t)b * dim + cc] = s[t];
            } else {
                lin = s[t];
            }
        }
        float acc = 0.5f * fm + lin + dsum;
        for (int off = 32; off; off >>= 1)
            acc += __shfl_down(acc, off, 64);
        if (lane == 0) partial[b] = acc + bias[0];
    }
    __syncthreads();
    rows_stage_out<(int)sizeof(OutT)>(img_o, (char*)go - mis_o, mis_o,
                                      mis_o + n * out_stride
                                      * (int)sizeof(OutT));
}

// Backward, bwd_e and bwd_d in one launch: groups of S samples, taken in a
// block-stride loop so that a launch has at most ceil(B * nd / 256) blocks
// — the number of global atomics per dw/db address that bwd_d issues. The
// e_all image is overwritten in place with de_all. Lanes cover (field,
// column) pairs: column = lane & (P - 1), P the power of two >= D1, and
// 64 / P fields per pass (one field and two columns per lane past P = 64).
// dw/db: LDS partials per block, then nd + 1 global atomics into the
// caller's buffers; nothing is zeroed here.
template <typename OutT>
__global__ void k_ctr_head_bwd_rows(const float* __restrict__ e_all,
                                    const float* __restrict__ dense,
                                    const float* __restrict__ w,
                                    const OutT* __restrict__ d_deep_in,
                                    const float* __restrict__ d_partial,
                                    const float* __restrict__ s_in,
                                    int B, int F, int dim, int nd,
                                    int out_stride,
                                    float* __restrict__ de_all,
                                    float* __restrict__ d_dense, // or null
                                    float* __restrict__ dw,
                                    float* __restrict__ db,
                                    int use_fm, int img_b, int p_shift,
                                    int n_groups) {
    extern __shared__ uint4 rows_smem[];
    __shared__ float lacc[ND_MAX + 1];
    char* const img_e = (char*)rows_smem;
    char* const img_d = img_e + img_b;
    const int S = blockDim.x >> 6;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D1 = dim + 1, R = F * D1;
    const int c0 = p_shift < 6 ? lane & ((1 << p_shift) - 1) : lane;
    const int f_first = p_shift < 6 ? lane >> p_shift : 0;
    const int f_step = p_shift < 6 ? 64 >> p_shift : 1;
    for (int t = threadIdx.x; t < nd + 1; t += blockDim.x) lacc[t] = 0.0f;

    for (int g = blockIdx.x; g < n_groups; g += gridDim.x) {
        // the previous group's image is still being stored
        if (g != (int)blockIdx.x) __syncthreads();
        const int b0 = g * S;
        const int n = min(S, B - b0);
        const float* ge = e_all + (size_t)b0 * R;
        const OutT* gd = d_deep_in + (size_t)b0 * out_stride;
        float* gde = de_all + (size_t)b0 * R;
        const int mis_e = (int)((uintptr_t)ge & 15);
        const int mis_d = (int)((uintptr_t)gd & 15);
        const int mis_de = (int)((uintptr_t)gde & 15);
        const int b = b0 + wave;
        const bool live = wave < n;

        float gp = 0.0f, dv = 0.0f, wv = 0.0f, sv[2] = {0.0f, 0.0f};
        if (live) {
            gp = d_partial[b];
            if (lane < nd) {
                dv = dense[(size_t)b * nd + lane];
                wv = w[lane];
            }
            if (use_fm) {
                #pragma unroll
                for (int t = 0; t < 2; ++t)
                    if (c0 + 64 * t < dim)
                        sv[t] = s_in[(size_t)b * dim + c0 + 64 * t];
            }
        }
        // the image is laid out for the de_all store; an e_all span that
        // sits differently in its 16-byte chunks (a sliced input) comes in
        // float by float
        const int hi_d = mis_d + n * out_stride * (int)sizeof(OutT);
        if (mis_e == mis_de) {
            rows_stage_in2<4, (int)sizeof(OutT)>(
                (const char*)ge - mis_e, img_e, mis_e, mis_e + n * R * 4,
                (const char*)gd - mis_d, img_d, mis_d, hi_d);
        } else {
            float* e = (float*)(img_e + mis_de);
            for (int i = threadIdx.x; i < n * R; i += blockDim.x)
                e[i] = ge[i];
            rows_stage_in<(int)sizeof(OutT)>((const char*)gd - mis_d, img_d,
                                             mis_d, hi_d);
        }
        __syncthreads();

        if (live) {
            float* e = (float*)(img_e + mis_de) + wave * R;
            const OutT* d = (const OutT*)(img_d + mis_d) + wave * out_stride;
            #pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int c = c0 + 64 * t;
                if (c >= D1) break;
                // 4 fields' reads in flight; d is read for the wide
                // column too (index <= F * dim, inside the row) and unused
                for (int f = f_first; f < F; f += 4 * f_step) {
                    float dv4[4], ev[4];
                    #pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int fu = min(f + u * f_step, F - 1);
                        dv4[u] = (float)d[fu * dim + c];
                        ev[u] = e[fu * D1 + c];
                    }
                    #pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (f + u * f_step >= F) break;
                        const int i = (f + u * f_step) * D1 + c;
                        if (c == dim) {
                            e[i] = gp;                // wide column
                        } else {
                            float gv = dv4[u];
                            if (use_fm) gv += gp * (sv[t] - ev[u]);
                            e[i] = gv;
                        }
                    }
                }
            }
            if (lane < nd) {
                if (d_dense)
                    d_dense[(size_t)b * nd + lane] =
                        (float)d[F * dim + lane] + gp * wv;
                atomicAdd(&lacc[lane], gp * dv);
            }
            if (lane == 0) atomicAdd(&lacc[nd], gp);
        }
        __syncthreads();
        rows_stage_out<4>(img_e, (char*)gde - mis_de, mis_de,
                          mis_de + n * R * 4);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nd + 1; t += blockDim.x) {
        if (t < nd) atomicAdd(&dw[t], lacc[t]);
        else atomicAdd(db, lacc[nd]);
    }
}

extern "C" {

void emb_ctr_head_fwd(const float* e_all, const float* dense, const float* w,
                      const float* bias, long B, long F, long dim, long nd,
                      long out_stride, void* deep_in, float* partial,
                      float* s_out, int use_fm, int out_bf16,
                      hipStream_t stream) {
    if (B == 0) return;
    int block = 256;                    // 4 waves per block
    long grid = (B * 64 + block - 1) / block;
    if (out_bf16)
        k_ctr_head_fwd<bf16><<<(int)grid, block, 0, stream>>>(
            e_all, dense, w, bias, B, F, dim, nd, out_stride,
            (bf16*)deep_in, partial, s_out, use_fm);
    else
        k_ctr_head_fwd<float><<<(int)grid, block, 0, stream>>>(
            e_all, dense, w, bias, B, F, dim, nd, out_stride,
            (float*)deep_in, partial, s_out, use_fm);
}

void emb_ctr_head_bwd(const float* e_all, const float* dense, const float* w,
                      const void* d_deep_in, const float* d_partial,
                      const float* s_in,
                      long B, long F, long dim, long nd, long out_stride,
                      float* de_all, float* d_dense, float* dw, float* db,
                      int use_fm, int out_bf16, hipStream_t stream) {
    if (B == 0) return;
    int block = 256;
    long grid_e = (B * F * (dim + 1) + block - 1) / block;
    long grid_d = (B * nd + block - 1) / block;
    if (out_bf16) {
        k_ctr_head_bwd_e<bf16><<<(int)grid_e, block, 0, stream>>>(
            e_all, (const bf16*)d_deep_in, d_partial, s_in, B, F, dim, nd,
            out_stride, de_all, use_fm, dw, db);
        k_ctr_head_bwd_d<bf16><<<(int)grid_d, block, 0, stream>>>(
            dense, w, (const bf16*)d_deep_in, d_partial, B, F, dim, nd,
            out_stride, d_dense, dw, db);
    } else {
        k_ctr_head_bwd_e<float><<<(int)grid_e, block, 0, stream>>>(
            e_all, (const float*)d_deep_in, d_partial, s_in, B, F, dim, nd,
            out_stride, de_all, use_fm, dw, db);
        k_ctr_head_bwd_d<float><<<(int)grid_d, block, 0, stream>>>(
            dense, w, (const float*)d_deep_in, d_partial, B, F, dim, nd,
            out_stride, d_dense, dw, db);
    }
}

// ---- row-staged launchers ----------------------------------------------

// bytes of one LDS image of S rows of row_bytes each: whole 16-byte chunks
// plus one chunk for the span's offset inside its first chunk
static long rows_img_bytes(long S, long row_bytes) {
    return (S * row_bytes + 15) / 16 * 16 + 16;
}

// log2 of the power of two >= D1: the lanes' (field, column) split
static int rows_p_shift(long D1) {
    int p_shift = 0;
    while ((1L << p_shift) < D1) ++p_shift;
    return p_shift;
}

// Samples (= waves) per block of the row-staged kernels, or 0 when the
// shape has to take the per-field kernels: the largest power of two up to
// 4 (forward) / 16 (backward) whose two images fit ROWS_LDS_MAX.
// bwd = 2 asks for the launcher's choice instead of "does it fit": the
// merged backward only with all 16 samples per block. With fewer (rows
// past 4 KB: dim 64 has S = 4) its block-stride loop makes 5 dependent
// load - barrier - store rounds on 208 blocks and measured 8 us slower per
// step than bwd_e + bwd_d (docs/benchmark.md), which at that size are
// bandwidth-bound and well populated.
int emb_ctr_head_rows_waves(long B, long F, long dim, long nd,
                            long out_stride, int out_bf16, int bwd) {
    const long D1 = dim + 1, R = F * D1, osz = out_bf16 ? 2 : 4;
    if (nd < 1 || nd > ND_MAX || dim < 0 || D1 > 128 || F < 1) return 0;
    // 32-bit element and byte offsets inside the kernels
    if (B * R >= (1L << 31) || B * out_stride >= (1L << 31)) return 0;
    for (int S = bwd ? 16 : 4; S >= 1; S >>= 1)
        if (rows_img_bytes(S, R * 4) + rows_img_bytes(S, out_stride * osz)
            <= ROWS_LDS_MAX)
            return bwd == 2 && S < 16 ? 0 : S;
    return 0;
}

// blocks of the merged backward: one per group of S samples, but no more
// than bwd_d launches (one global atomic per address and block)
long emb_ctr_head_rows_bwd_grid(long B, long nd, int S) {
    const long groups = (B + S - 1) / S;
    const long cap = (B * nd + 255) / 256;
    return groups < cap ? groups : (cap < 1 ? 1 : cap);
}

void emb_ctr_head_fwd_rows(const float* e_all, const float* dense,
                           const float* w, const float* bias, long B, long F,
                           long dim, long nd, long out_stride, void* deep_in,
                           float* partial, float* s_out, int use_fm,
                           int out_bf16, int S, hipStream_t stream) {
    if (B == 0) return;
    const long img_b = rows_img_bytes(S, F * (dim + 1) * 4);
    const long lds = img_b + rows_img_bytes(S, out_stride
                                            * (out_bf16 ? 2 : 4));
    const long grid = (B + S - 1) / S;
    const int p_shift = rows_p_shift(dim + 1);
    if (out_bf16)
        k_ctr_head_fwd_rows<bf16><<<(int)grid, 64 * S, lds, stream>>>(
            e_all, dense, w, bias, (int)B, (int)F, (int)dim, (int)nd,
            (int)out_stride, (bf16*)deep_in, partial, s_out, use_fm,
            (int)img_b, p_shift);
    else
        k_ctr_head_fwd_rows<float><<<(int)grid, 64 * S, lds, stream>>>(
            e_all, dense, w, bias, (int)B, (int)F, (int)dim, (int)nd,
            (int)out_stride, (float*)deep_in, partial, s_out, use_fm,
            (int)img_b, p_shift);
}

// d_dense may be null (no gradient wanted); dw/db are accumulated into
void emb_ctr_head_bwd_rows(const float* e_all, const float* dense,
                           const float* w, const void* d_deep_in,
                           const float* d_partial, const float* s_in,
                           long B, long F, long dim, long nd,
                           long out_stride, float* de_all, float* d_dense,
                           float* dw, float* db, int use_fm, int out_bf16,
                           int S, hipStream_t stream) {
    if (B == 0) return;
    const long img_b = rows_img_bytes(S, F * (dim + 1) * 4);
    const long lds = img_b + rows_img_bytes(S, out_stride
                                            * (out_bf16 ? 2 : 4));
    const long groups = (B + S - 1) / S;
    const long grid = emb_ctr_head_rows_bwd_grid(B, nd, S);
    const int p_shift = rows_p_shift(dim + 1);
    if (out_bf16)
        k_ctr_head_bwd_rows<bf16><<<(int)grid, 64 * S, lds, stream>>>(
            e_all, dense, w, (const bf16*)d_deep_in, d_partial, s_in,
            (int)B, (int)F, (int)dim, (int)nd, (int)out_stride, de_all,
            d_dense, dw, db, use_fm, (int)img_b, p_shift, (int)groups);
    else
        k_ctr_head_bwd_rows<float><<<(int)grid, 64 * S, lds, stream>>>(
            e_all, dense, w, (const float*)d_deep_in, d_partial, s_in,
            (int)B, (int)F, (int)dim, (int)nd, (int)out_stride, de_all,
            d_dense, dw, db, use_fm, (int)img_b, p_shift, (int)groups);
}

}  // extern "C"
