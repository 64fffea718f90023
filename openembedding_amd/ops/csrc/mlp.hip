// Fused 3-hidden-layer MLP (gfx950, bf16 MFMA 16x16x32) — forward and the
// dgrad-chain backward, each in ONE kernel.
//
// Why: at M=4096, H=400 the per-layer library GEMMs are skinny (measured
// ~43 TF fp32, ~26 us each) and the bias/ReLU/cast glue adds ~20 more
// launches. Here activations flow layer-to-layer through LDS; weights
// stream from L2 (1 MB bf16, L2-resident per XCD); bias+ReLU fuse into the
// MFMA epilogue; hidden activations mirror to HBM for the backward.
//
// EVERY contraction length is padded to a multiple of 32 host-side (padded
// weight copies with zeroed tails; x0 zero-padded by the head kernel): the
// fragment load is then one unconditional 16-byte load, which is what lets
// hipcc software-pipeline the k-loop (the earlier bounds-checked version
// scalarized to 2-byte loads and serialized load->mfma per k-step:
// 93 us/step; see git history).
//
// Fragment maps (mfma_f32_16x16x32_bf16, verified by tests/test_gpu_mlp.py
// against a torch reference with asymmetric data):
//   A[m][k]: m = lane&15, k = (lane>>4)*8 + e
//   B[k][n]: n = lane&15, k = (lane>>4)*8 + e   (B = W[n][k] row-major)
//   C/D:     col = lane&15, row = (lane>>4)*4 + r

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

typedef __hip_bfloat16 mbf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// LDS row stride (elements): 424*2B = 212 dwords; 212 % 64 = 20,
// gcd(20,64)=4 -> the 16 rows of a fragment read land on 16 distinct banks.
#define MLP_LD 424

static __device__ __forceinline__ bf16x8 ld_frag(const mbf16* p) {
    return *reinterpret_cast<const bf16x8*>(
        __builtin_assume_aligned(p, 16));
}

// Weight layouts. The fragment map above fixes which lane holds which
// (n, k), not where the element lives in memory, and the kernels take the
// padded weights [N, Kp] in either of two images (template flag FRAG):
//   row-major      lane's piece of k-step s of column chunk c at
//                  (c + lane&15) * Kp + (lane>>4)*8 + 32*s: the 16 lanes of
//                  a quarter-wave sit in 16 rows = 16 cache lines, a wave
//                  load is 64 separate 16-byte L1 accesses;
//   fragment-major element (n, k) at
//                  ((n/16 * KS + k/32) * 64 + (k%32)/8 * 16 + n%16) * 8 + k%8
//                  (KS = Kp/32), i.e. [N/16][KS][4][16][8]: lane l's piece of
//                  k-step s of chunk c is the 16 bytes at
//                  ((c/16 * KS + s) * 64 + l) * 8 — a wave load is one
//                  contiguous 1 KB block (8 full lines), a chunk one KS KB
//                  run. Written by k_mlp3_pack_frag.
// Both start a chunk at c * Kp; they differ in the lane's offset inside it
// and in the stride between k-steps. The (lane, element) <-> (n, k) map and
// the k-order are the same, so every fp32 sum is too.
#define MLP_BSTEP(frag) ((frag) ? 512 : 32)   // elements between k-steps

// 16x16 tile over a padded contraction: A [.., lda] row-major, W [N, ldw]
// (B = W[n][k]; row-major or fragment-major, ldw = Kp); Kp % 32 == 0.
//
// M=16 per block means the W stream has NO reuse inside the block — the
// "decode-GEMV" regime of the perf guide: load straight to VGPRs with a
// DEEP UNROLL and late counted waits, so all K-steps' loads are in flight
// before the first MFMA needs its operands (a 2-deep pipeline left ~200
// cycles of L2 latency exposed per step: 80-90 us/kernel measured).
template <int KS, int BST>
static __device__ __forceinline__ f32x4 tile16_u(
        const mbf16* __restrict__ pa, const mbf16* __restrict__ pb) {
    bf16x8 a[KS], b[KS];
    #pragma unroll
    for (int s = 0; s < KS; ++s) {
        a[s] = ld_frag(pa + 32 * s);
        b[s] = ld_frag(pb + BST * s);
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    #pragma unroll
    for (int s = 0; s < KS; ++s)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[s], b[s], acc,
                                                      0, 0, 0);
    return acc;
}

template <bool FRAG>
static __device__ __forceinline__ f32x4 tile16(
        const mbf16* Arow, const mbf16* W, long ldw, long n0,
        long Kp, int lane) {      // Arow: the lane's A row (m = lane&15)
    constexpr int BST = MLP_BSTEP(FRAG);
    const long koff = (lane >> 4) * 8;
    const mbf16* pa = Arow + koff;
    const mbf16* pb = FRAG ? W + n0 * ldw + lane * 8
                           : W + (n0 + (lane & 15)) * ldw + koff;
    if (Kp == 256) return tile16_u<8, BST>(pa, pb);    // K0 = 247 padded
    if (Kp == 416) return tile16_u<13, BST>(pa, pb);   // H = 400 padded
    if (Kp == 128) return tile16_u<4, BST>(pa, pb);
    // generic fallback: 2-stage pipeline
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    bf16x8 a0 = ld_frag(pa), b0 = ld_frag(pb);
    for (long kb = 32; kb < Kp; kb += 32) {
        bf16x8 a1 = ld_frag(pa + kb);
        bf16x8 b1 = ld_frag(pb + kb * (BST / 32));
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc, 0, 0, 0);
        a0 = a1; b0 = b1;
    }
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc, 0, 0, 0);
}

#define MLP_WAVES 8   // 8 waves/block = 2 per SIMD: the partner wave hides
                      // the other's W-stream latency (1 block/CU grid)

// Row tile BM in {16, 32, 64} is a template parameter of both kernels: a
// block owns RT = BM/16 MFMA row tiles and every weight fragment a wave
// loads is used for all of them, so the weight bytes streamed per row fall
// by RT (at BM=16 every block streams the full 0.87 MB for 16 rows).
// LDS is 2 x BM x 424 x 2 B (27/54/108 KB, dynamic).

// bf16 bit patterns stay raw until they are used: a conversion right after
// the load would pull the load's wait in front of the MFMAs
static __device__ __forceinline__ float bf16_bits_f32(unsigned short b) {
    return __uint_as_float((unsigned)b << 16);
}

// write one 16x16 accumulator tile: bias, ReLU, backward mask, bf16 mirror
// to LDS (next layer's A side) and to HBM (rows < M only)
static __device__ __forceinline__ void mlp_epilogue(
        f32x4 acc, float bv, bool relu, bool masked,
        const unsigned short (&mk)[4], int rt, long m0, long M, int c,
        int lane, mbf16* lds_out, mbf16* save, long save_ld) {
    const int col = lane & 15;
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = rt * 16 + (lane >> 4) * 4 + r;
        const long gm = m0 + row;
        float v = acc[r] + bv;
        if (relu) v = v > 0.f ? v : 0.f;
        if (masked && !(bf16_bits_f32(mk[r]) > 0.f)) v = 0.f;
        mbf16 hv = (mbf16)v;
        if (lds_out) lds_out[row * MLP_LD + c + col] = hv;
        if (gm < M) save[gm * save_ld + c + col] = hv;
    }
}

// backward ReLU mask bits of one 16-column chunk for the lane's 4 rows of
// every row tile (rows >= M read as 0: their outputs are never saved)
template <int RT>
static __device__ __forceinline__ void mlp_load_mask(
        unsigned short (&mk)[RT][4], const mbf16* mask_act, long mask_ld,
        long m0, long M, int c, int lane) {
    const int ld = (int)mask_ld;
    #pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const long g0 = m0 + rt * 16 + (lane >> 4) * 4;
        const unsigned short* mp =
            reinterpret_cast<const unsigned short*>(mask_act)
            + g0 * mask_ld + c + (lane & 15);
        #pragma unroll
        for (int r = 0; r < 4; ++r)
            mk[rt][r] = g0 + r < M ? mp[r * ld] : (unsigned short)0;
    }
}

// fragment-major: the lane's piece of k-step 0 of column chunk c/16. c is
// wave-uniform, which the compiler cannot see (it derives from
// threadIdx.x >> 6). The 1 KB k-step stride leaves the load's immediate-
// offset range after 4 steps, so a chunk needs a base per 4 k-steps where
// the row-major form needs one; with readfirstlane the chunk part of them
// is scalar arithmetic. Without it bwd<32> spilled 16 B/lane and the BM=64
// kernels grew by 1-2 VGPRs; with it every instantiation is at or below
// its row-major twin (docs/kernels.md).
template <int KS>
static __device__ __forceinline__ const mbf16* mlp_frag_chunk(
        const mbf16* W, int c, int lane) {
    return W + __builtin_amdgcn_readfirstlane(c) * (KS * 32)
             + (unsigned)(lane * 8);
}

// one layer: lds_out/save <- relu(A @ W^T + b) (relu/bias optional) for
// the block's RT row tiles and N output columns.
//
// Pipelining (PMC showed 86% SQ_WAIT_ANY with per-chunk batched loads):
// the A fragments depend only on (row, k) — identical for every column
// chunk — so for RT <= 2 they load ONCE per layer into registers (RT=4
// would need 208 VGPRs for them alone: there they are re-read from the LDS
// tile per chunk, conflict-free at stride 424); the B (weight) stream
// double-buffers across chunks: chunk i+1's fragment loads are in flight
// while chunk i's MFMAs run.
//
// Everything the epilogue reads from global memory (bias, backward mask)
// is loaded BEFORE the next chunk's weight prefetch is issued: loads
// return in order, so a bias load issued after the MFMAs would also wait
// for the whole prefetched next chunk; issued in front of it, its wait
// leaves the prefetch in flight.
//
// sync_first: the barrier that separates this layer from the previous one
// sits AFTER this layer's first weight-chunk loads are issued (they depend
// only on the wave), so they fly while the block drains the last layer.
//
// rot: the block's first column chunk is rotated by blockIdx.x, so that
// concurrent blocks stream different weight rows instead of all walking
// the same addresses in lockstep. Each output column sees the same k-order.
template <int KS, int RT, bool FRAG>
static __device__ __forceinline__ void mlp_layer_u(
        const mbf16* A, int lda, int a_rows, long m0, long M,
        const mbf16* W, int ldw, const mbf16* bias, int N,
        const mbf16* mask_act, long mask_ld,
        mbf16* lds_out, mbf16* save, long save_ld,
        int wave, int lane, bool relu, bool sync_first) {
    constexpr int AR = RT <= 2 ? RT : 1;
    constexpr int BST = MLP_BSTEP(FRAG);
    const int koff = (lane >> 4) * 8, col = lane & 15;
    const int nch = N >> 4;
    const int rot = (int)(blockIdx.x % (unsigned)nch);
    const unsigned short* bp = reinterpret_cast<const unsigned short*>(bias);
    const bool masked = mask_act != nullptr;

    bf16x8 b0[KS], b1[KS];
    unsigned short bb = 0;
    unsigned short mk[RT][4] = {};
    int li = wave;                       // logical chunk; wave-uniform
    int c = li + rot;
    if (c >= nch) c -= nch;
    c *= 16;
    if (li < nch) {
        const mbf16* pb = FRAG ? mlp_frag_chunk<KS>(W, c, lane)
                               : W + (c + col) * ldw + koff;
        #pragma unroll
        for (int s = 0; s < KS; ++s) b0[s] = ld_frag(pb + BST * s);
    }
    if (sync_first) __syncthreads();

    bf16x8 a[AR][KS];
    if (RT <= 2) {
        #pragma unroll
        for (int rt = 0; rt < AR; ++rt) {
            // a_rows: rows of A that exist (the global x0 tile of a partial
            // last block is shorter than 16; clamped rows are never saved)
            const int ar = min(rt * 16 + col, a_rows - 1);
            const mbf16* pa = A + ar * lda + koff;
            #pragma unroll
            for (int s = 0; s < KS; ++s) a[rt][s] = ld_frag(pa + 32 * s);
        }
    }
    for (; li < nch; li += MLP_WAVES) {
        if (bp) bb = bp[c + col];
        if (masked) mlp_load_mask<RT>(mk, mask_act, mask_ld, m0, M, c, lane);
        int cn = li + MLP_WAVES + rot;
        if (cn >= nch) cn -= nch;
        cn *= 16;
        if (li + MLP_WAVES < nch) {
            const mbf16* pb = FRAG ? mlp_frag_chunk<KS>(W, cn, lane)
                                   : W + (cn + col) * ldw + koff;
            #pragma unroll
            for (int s = 0; s < KS; ++s) b1[s] = ld_frag(pb + BST * s);
        }
        #pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if (RT <= 2) {
                #pragma unroll
                for (int s = 0; s < KS; ++s)
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a[rt][s], b0[s], acc, 0, 0, 0);
            } else {
                const mbf16* pa = A + (rt * 16 + col) * lda + koff;
                #pragma unroll
                for (int s = 0; s < KS; ++s)
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        ld_frag(pa + 32 * s), b0[s], acc, 0, 0, 0);
            }
            mlp_epilogue(acc, bp ? bf16_bits_f32(bb) : 0.f, relu, masked,
                         mk[rt], rt, m0, M, c, lane, lds_out, save, save_ld);
            // keep the scheduler from hoisting all RT x KS LDS fragment
            // reads to the top (208 VGPRs at RT=4: it spilled)
            if (RT > 2) __builtin_amdgcn_sched_barrier(0);
        }
        #pragma unroll
        for (int s = 0; s < KS; ++s) b0[s] = b1[s];
        c = cn;
    }
}

template <int RT, bool FRAG>
static __device__ __forceinline__ void mlp_layer(
        const mbf16* A, int lda, int a_rows, long m0, long M,
        const mbf16* W, int ldw, const mbf16* bias, int N, int Kp,
        const mbf16* mask_act, long mask_ld,
        mbf16* lds_out, mbf16* save, long save_ld,
        int wave, int lane, bool relu, bool sync_first) {
    if (Kp == 256)
        return mlp_layer_u<8, RT, FRAG>(A, lda, a_rows, m0, M, W, ldw, bias,
                                        N, mask_act, mask_ld, lds_out, save,
                                        save_ld, wave, lane, relu,
                                        sync_first);
    if (Kp == 416)
        return mlp_layer_u<13, RT, FRAG>(A, lda, a_rows, m0, M, W, ldw, bias,
                                         N, mask_act, mask_ld, lds_out, save,
                                         save_ld, wave, lane, relu,
                                         sync_first);
    // generic (unpipelined) fallback for other shapes
    if (sync_first) __syncthreads();
    const bool masked = mask_act != nullptr;
    for (int c = wave * 16; c < N; c += 16 * MLP_WAVES) {
        const float bv = bias ? (float)bias[c + (lane & 15)] : 0.f;
        unsigned short mk[RT][4] = {};
        if (masked) mlp_load_mask<RT>(mk, mask_act, mask_ld, m0, M, c, lane);
        #pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int ar = min(rt * 16 + (lane & 15), a_rows - 1);
            f32x4 acc = tile16<FRAG>(A + ar * lda, W, ldw, c, Kp, lane);
            mlp_epilogue(acc, bv, relu, masked, mk[rt], rt, m0, M, c, lane,
                         lds_out, save, save_ld);
        }
    }
}

// zero n16 16-byte pieces of LDS. LDS starts with arbitrary bits; the pad
// columns [H, MLP_LD) are read by the next stage's fragments against ZERO
// weight pads — but 0 * inf-garbage = NaN, so they must be zeroed (found
// the hard way: NaN from step ~3 once other kernels had dirtied the LDS)
static __device__ __forceinline__ void mlp_zero_lds(mbf16* p, int n16) {
    u32x4* z = reinterpret_cast<u32x4*>(p);
    for (int i = threadIdx.x; i < n16; i += blockDim.x)
        z[i] = u32x4{0u, 0u, 0u, 0u};
}

template <int BM, bool FRAG>
__global__ __launch_bounds__(64 * MLP_WAVES, 2)
void k_mlp3_fwd(const mbf16* __restrict__ x0, long M, long K0p,
                const mbf16* __restrict__ w1,   // [H, K0p] padded; the
                                                // weights row-major or
                                                // fragment-major (FRAG)
                const mbf16* __restrict__ b1,
                const mbf16* __restrict__ w2,   // [H, Hp] padded
                const mbf16* __restrict__ b2,
                const mbf16* __restrict__ w3,   // [H, Hp] padded
                const mbf16* __restrict__ b3,
                const mbf16* __restrict__ w4,   // [H]
                const mbf16* __restrict__ b4,
                const float* __restrict__ partial,  // [M] logit carry-in or null
                long H, long Hp,
                mbf16* __restrict__ a1, mbf16* __restrict__ a2,
                mbf16* __restrict__ a3, float* __restrict__ out) {
    constexpr int RT = BM / 16;
    extern __shared__ __attribute__((aligned(16))) mbf16 mlp_smem[];
    mbf16* act0 = mlp_smem;
    mbf16* act1 = mlp_smem + BM * MLP_LD;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const long m0 = (long)blockIdx.x * BM;
    if (m0 >= M) return;
    mlp_zero_lds(mlp_smem, 2 * BM * MLP_LD / 8);

    const mbf16* A1 = x0 + m0 * K0p;
    int lda1 = (int)K0p;
    int a_rows1 = (int)(M - m0 < BM ? M - m0 : BM);
    if (RT > 1) {
        // more than one row tile: the A fragments of layer 1 are read per
        // row tile, so x0's BM x K0p tile is staged into LDS once (16-byte
        // pieces; rows >= M stay zero). The launcher guarantees
        // K0p <= MLP_LD - 8 here.
        __syncthreads();                  // zeroing done before the overlay
        const int ppr = (int)(K0p >> 3);  // pieces per row
        for (int i = threadIdx.x; i < BM * ppr; i += blockDim.x) {
            const int row = i / ppr, pc = i - row * ppr;
            if (m0 + row < M)
                *reinterpret_cast<u32x4*>(act1 + row * MLP_LD + pc * 8) =
                    *reinterpret_cast<const u32x4*>(__builtin_assume_aligned(
                        A1 + (long)row * K0p + pc * 8, 16));
        }
        A1 = act1;
        lda1 = MLP_LD;
        a_rows1 = BM;
    }
    mlp_layer<RT, FRAG>(A1, lda1, a_rows1, m0, M, w1, (int)K0p, b1, (int)H,
                        (int)K0p, nullptr, 0, act0, a1, H, wave, lane, true,
                        true);
    mlp_layer<RT, FRAG>(act0, MLP_LD, BM, m0, M, w2, (int)Hp, b2, (int)H,
                        (int)Hp, nullptr, 0, act1, a2, H, wave, lane, true,
                        true);
    mlp_layer<RT, FRAG>(act1, MLP_LD, BM, m0, M, w3, (int)Hp, b3, (int)H,
                        (int)Hp, nullptr, 0, act0, a3, H, wave, lane, true,
                        true);
    __syncthreads();

    // final Linear(H, 1): VALU dot per row
    constexpr int rows_per_wave = BM / MLP_WAVES;
    for (int r = 0; r < rows_per_wave; ++r) {
        const int row = wave * rows_per_wave + r;
        const long gm = m0 + row;
        if (gm >= M) continue;
        float s = 0.f;
        for (int k = lane; k < (int)H; k += 64)
            s += (float)act0[row * MLP_LD + k] * (float)w4[k];
        #pragma unroll
        for (int off = 32; off; off >>= 1)
            s += __shfl_down(s, off, 64);
        if (lane == 0)
            out[gm] = s + (float)b4[0] + (partial ? partial[gm] : 0.f);
    }
}

template <int BM, bool FRAG>
__global__ __launch_bounds__(64 * MLP_WAVES, 2)
void k_mlp3_bwd(const float* __restrict__ dout, long M, long K0p,
                const mbf16* __restrict__ a1, const mbf16* __restrict__ a2,
                const mbf16* __restrict__ a3,
                const mbf16* __restrict__ w4,    // [H]
                const mbf16* __restrict__ w3t,   // [H, Hp] padded transposed
                const mbf16* __restrict__ w2t,   // [H, Hp]
                const mbf16* __restrict__ w1t,   // [K0p, Hp]
                long H, long Hp,
                mbf16* __restrict__ dz1, mbf16* __restrict__ dz2,
                mbf16* __restrict__ dz3, mbf16* __restrict__ dx0,
                float* __restrict__ bias_out) {  // optional [4H+1] scratch
    constexpr int RT = BM / 16;
    extern __shared__ __attribute__((aligned(16))) mbf16 mlp_smem[];
    mbf16* dzA = mlp_smem;
    mbf16* dzB = mlp_smem + BM * MLP_LD;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const long m0 = (long)blockIdx.x * BM;
    if (m0 >= M) return;
    // see mlp_zero_lds: 0 * LDS-garbage-inf = NaN. dzA is written in full
    // (pad columns too) by the loop below, so only dzB needs the zeroing.
    mlp_zero_lds(dzB, BM * MLP_LD / 8);

    // dz3 = dout ⊗ w4 ⊙ relu'(a3), elementwise; zero the LDS pad columns
    // once (the B-side pads are zero too, but dz tiles are the A side of
    // the NEXT stage whose pads multiply W pads — either side zero is
    // enough; zeroing here keeps the invariant simple).
    // 32-bit indices and a compile-time divisor: i / MLP_LD is a multiply
    // (a 64-bit div/mod per element is a long emulated sequence).
    const int Hi = (int)H;
    for (int i = threadIdx.x; i < BM * MLP_LD; i += blockDim.x) {
        const int row = i / MLP_LD, n = i - row * MLP_LD;
        const long gm = m0 + row;
        float v = 0.f;
        if (n < Hi && gm < M && (float)a3[gm * H + n] > 0.f)
            v = dout[gm] * (float)w4[n];
        mbf16 hv = (mbf16)v;
        dzA[i] = hv;
        if (n < Hi && gm < M) dz3[gm * H + n] = hv;
    }
    if (bias_out) {
        // head wgrad dw4[n] = sum_m dout[m]*a3[m,n] and db4 ride along as
        // a SECOND walk over the a3 tile the loop above just pulled into
        // L1/L2 (BM rows x H x 2B — hot): the separate head pass
        // over a3 (3 MB/step HBM) disappears, while the main loop keeps
        // its linear-index ILP (a fused column-walk version cost ~4 us)
        for (int n = threadIdx.x; n < Hi; n += blockDim.x) {
            float sw = 0.f, s4 = 0.f;
            for (int row = 0; row < BM; ++row) {
                long gm = m0 + row;
                if (gm < M) {
                    float dv = dout[gm];
                    sw += dv * (float)a3[gm * H + n];
                    if (n == 0) s4 += dv;
                }
            }
            atomicAdd(&bias_out[3 * H + n], sw);
            if (n == 0 && s4 != 0.f) atomicAdd(&bias_out[4 * H], s4);
        }
    }
    // NOTE: dz tiles' pad columns [H, Hp) may hold garbage after a GEMM
    // stage — harmless, because the B side (padded weight copies) is zero
    // there, so pad products vanish.
    mlp_layer<RT, FRAG>(dzA, MLP_LD, BM, m0, M, w3t, (int)Hp, nullptr, Hi,
                        (int)Hp, a2, H, dzB, dz2, H, wave, lane, false, true);
    mlp_layer<RT, FRAG>(dzB, MLP_LD, BM, m0, M, w2t, (int)Hp, nullptr, Hi,
                        (int)Hp, a1, H, dzA, dz1, H, wave, lane, false, true);
    mlp_layer<RT, FRAG>(dzA, MLP_LD, BM, m0, M, w1t, (int)Hp, nullptr,
                        (int)K0p, (int)Hp, nullptr, 0, nullptr, dx0, K0p,
                        wave, lane, false, true);
}

// Bias grads for all 3 hidden layers + the head scalar in one pass over
// the dz mirrors k_mlp3_bwd already writes (torch did them as 3 GEMV
// launches + a reduce + an add, ~35 us/step at B=4096 H=400). Partials
// accumulate into a persistent fp32 scratch [3H+1] via atomics; the
// finisher below folds the scratch into the (bf16) grad buffers and
// re-zeros it, so the scratch is zero again before the next step's
// launch — the whole pair is hipGraph-capturable with no per-step fill.
extern "C" __global__ void k_mlp3_bias_bwd(
        const float* __restrict__ dout,
        const mbf16* __restrict__ dz1, const mbf16* __restrict__ dz2,
        const mbf16* __restrict__ dz3, const mbf16* __restrict__ a3,
        long M, long H, long rows_per_blk,
        float* __restrict__ scratch, int with_dz, int with_head) {
    const long r0 = (long)blockIdx.x * rows_per_blk;
    if (r0 >= M) return;
    const long r1 = min(M, r0 + rows_per_blk);
    // column sums: thread t covers columns t, t+blockDim.x, ... of each dz
    // (+ the head wgrad dw4[c] = sum_r dout[r]*a3[r,c] — same access shape).
    // with_dz == 0: the fused wgrad kernel already accumulated the three
    // dz column sums from its LDS-staged tiles; with_head == 0: the dgrad
    // kernel carried dw4/db4 (it reads dout/a3 anyway). Both 0: the
    // launcher never starts this kernel, only the finisher.
    for (long c = threadIdx.x; c < H; c += blockDim.x) {
        float sw = 0.f;
        if (with_dz) {
            float s1 = 0.f, s2 = 0.f, s3 = 0.f;
            for (long r = r0; r < r1; ++r) {
                s1 += (float)dz1[r * H + c];
                s2 += (float)dz2[r * H + c];
                s3 += (float)dz3[r * H + c];
                if (with_head) sw += dout[r] * (float)a3[r * H + c];
            }
            atomicAdd(scratch + c, s1);
            atomicAdd(scratch + H + c, s2);
            atomicAdd(scratch + 2 * H + c, s3);
        } else if (with_head) {
            for (long r = r0; r < r1; ++r)
                sw += dout[r] * (float)a3[r * H + c];
        }
        if (with_head) atomicAdd(scratch + 3 * H + c, sw);
    }
    if (with_head) {
        // head bias: sum of dout rows, one atomic per wave
        float s4 = 0.f;
        for (long r = r0 + threadIdx.x; r < r1; r += blockDim.x)
            s4 += dout[r];
        #pragma unroll
        for (int off = 32; off; off >>= 1) s4 += __shfl_down(s4, off, 64);
        if ((threadIdx.x & 63) == 0 && s4 != 0.f)
            atomicAdd(scratch + 4 * H, s4);
    }
}

extern "C" __global__ void k_mlp3_bias_finish(
        float* __restrict__ scratch, long H,
        mbf16* __restrict__ db1, mbf16* __restrict__ db2,
        mbf16* __restrict__ db3, mbf16* __restrict__ dw4,
        mbf16* __restrict__ db4) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > 4 * H) return;
    float v = scratch[i];
    scratch[i] = 0.f;               // self-cleaning for the next step
    mbf16* dst = i < H        ? db1 + i
               : i < 2 * H    ? db2 + (i - H)
               : i < 3 * H    ? db3 + (i - 2 * H)
               : i < 4 * H    ? dw4 + (i - 3 * H)
               :                db4;
    *dst = (mbf16)((float)*dst + v);    // zero_grad zeroed it; += matches
}                                       // torch's beta=1 accumulation

extern "C" void emb_mlp3_bias_bwd(const float* dout, const void* dz1,
                                  const void* dz2, const void* dz3,
                                  const void* a3,
                                  long M, long H, float* scratch,
                                  void* db1, void* db2, void* db3,
                                  void* dw4, void* db4, int with_dz,
                                  int with_head, hipStream_t stream) {
    if (M == 0) return;
    const long rows_per_blk = 32;
    int ga = (int)((M + rows_per_blk - 1) / rows_per_blk);
    if (with_dz || with_head)
        k_mlp3_bias_bwd<<<ga, 256, 0, stream>>>(
            dout, (const mbf16*)dz1, (const mbf16*)dz2, (const mbf16*)dz3,
            (const mbf16*)a3, M, H, rows_per_blk, scratch, with_dz,
            with_head);
    int gb = (int)((4 * H + 1 + 255) / 256);
    k_mlp3_bias_finish<<<gb, 256, 0, stream>>>(
        scratch, H, (mbf16*)db1, (mbf16*)db2, (mbf16*)db3, (mbf16*)dw4,
        (mbf16*)db4);
}

// Row tile choice. bm = 0: automatic; 16/32/64 force a variant (tests).
// BM > 16 stages x0 in the LDS tile, so it needs K0p <= MLP_LD - 8; wider
// inputs (dim 64: K0p 1696) always run BM = 16.
//
// The rule. A block's time is set by streaming the whole weight set
// through its CU and barely depends on its rows, and blocks run one per CU
// (8 waves x ~190 VGPRs), so a launch costs waves-of-blocks x block time:
//   cost(BM) = ceil(ceil(M / BM) / CUs) * t[BM].
// Measured on MI355X (256 CUs), H=400 K0p=256, us per kernel, fwd / bwd:
//   M      BM=16          BM=32          BM=64
//   1024   24.5 / 26.6    27.5 / 35.7    39.8 / 58.4
//   2048   24.8 / 28.4    27.8 / 36.5    40.2 / 58.8
//   4096   25.3 / 32.2    28.2 / 39.1    40.8 / 61.8
//   8192   48.2 / 61.9    29.1 / 45.4    41.7 / 68.0
// (parent commit, BM=16 only: 25.5/29.1, 25.6/31.0, 26.3/35.7, 50.4/71.0).
// Up to 16 rows x 256 CUs = 4096 rows BM=16 is fastest and keeps the most
// blocks for small M; past it a second wave of blocks doubles its time
// and the larger tile wins. t[] below are the one-wave times at M=4096.
//
// The table above is the ROW-MAJOR weight layout (frag = false), where the
// block time is the L1 access rate of the 16-byte fragment pieces. With the
// fragment-major images (frag = true; same method: back-to-back launches,
// best of 3 x 300, device events) the stream costs a quarter of the L1
// accesses and every cell falls, BM=16 the most:
//   M      BM=16          BM=32          BM=64
//   1024   15.1 / 20.1    19.4 / 30.2    34.4 / 55.4
//   2048   15.3 / 21.8    19.6 / 30.9    34.8 / 55.7
//   4096   16.1 / 26.0    20.2 / 35.3    35.2 / 58.8
//   8192   29.8 / 49.9    21.5 / 39.9    36.4 / 65.5
// (row-major re-measured in the same run: within 0.3 us of the table
// above, bwd BM=64 within 1.0). "BM = 16 while M/16 <= CUs" still holds,
// by a wider margin (4096: 16.1 vs 20.2, 26.0 vs 35.3), and BM=32 still
// wins past it (8192: 21.5 vs 29.8, 39.9 vs 49.9): the rule is unchanged,
// the two layouts keep their own t[].
static int mlp_pick_bm(long M, long K0p, int bm, bool bwd, bool frag) {
    if (K0p > MLP_LD - 8) return 16;
    if (bm == 16 || bm == 32 || bm == 64) return bm;
    static int cus = 0;
    if (!cus) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess
            || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount,
                                     dev) != hipSuccess || n <= 0)
            n = 256;
        cus = n;
    }
    static const float t_fwd[3] = {25.3f, 28.2f, 40.8f};
    static const float t_bwd[3] = {32.2f, 39.1f, 61.8f};
    static const float t_fwd_frag[3] = {16.1f, 20.2f, 35.2f};
    static const float t_bwd_frag[3] = {26.0f, 35.3f, 58.8f};
    const float* t = frag ? (bwd ? t_bwd_frag : t_fwd_frag)
                          : (bwd ? t_bwd : t_fwd);
    int best = 16;
    float best_cost = 0.f;
    for (int i = 0; i < 3; ++i) {
        const long b = 16L << i;
        const long blocks = (M + b - 1) / b;
        const float cost = (float)((blocks + cus - 1) / cus) * t[i];
        if (i == 0 || cost < best_cost) { best = (int)b; best_cost = cost; }
    }
    return best;
}

// BM = 64 needs 108 KB of LDS, above the 64 KB a kernel gets by default
template <typename K>
static void mlp_allow_lds(K kernel, size_t bytes) {
    if (bytes > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)bytes);
}

template <int BM, bool FRAG>
static void mlp_launch_fwd(const void* x0, long M, long K0p,
                           const void* w1, const void* b1,
                           const void* w2, const void* b2,
                           const void* w3, const void* b3,
                           const void* w4, const void* b4,
                           const float* partial, long H, long Hp,
                           void* a1, void* a2, void* a3, float* out,
                           hipStream_t stream) {
    const size_t lds = 2 * BM * MLP_LD * sizeof(mbf16);
    mlp_allow_lds(&k_mlp3_fwd<BM, FRAG>, lds);
    const long grid = (M + BM - 1) / BM;
    k_mlp3_fwd<BM, FRAG><<<(int)grid, 64 * MLP_WAVES, lds, stream>>>(
        (const mbf16*)x0, M, K0p, (const mbf16*)w1, (const mbf16*)b1,
        (const mbf16*)w2, (const mbf16*)b2, (const mbf16*)w3,
        (const mbf16*)b3, (const mbf16*)w4, (const mbf16*)b4, partial, H, Hp,
        (mbf16*)a1, (mbf16*)a2, (mbf16*)a3, out);
}

extern "C" void emb_mlp3_fwd(const void* x0, long M, long K0p,
                             const void* w1, const void* b1,
                             const void* w2, const void* b2,
                             const void* w3, const void* b3,
                             const void* w4, const void* b4,
                             const float* partial,
                             long H, long Hp,
                             void* a1, void* a2, void* a3, float* out,
                             int bm, int frag, hipStream_t stream) {
    if (M == 0) return;
    bm = mlp_pick_bm(M, K0p, bm, false, frag != 0);
    auto fn = frag ? (bm == 64 ? mlp_launch_fwd<64, true>
                      : bm == 32 ? mlp_launch_fwd<32, true>
                                 : mlp_launch_fwd<16, true>)
                   : (bm == 64 ? mlp_launch_fwd<64, false>
                      : bm == 32 ? mlp_launch_fwd<32, false>
                                 : mlp_launch_fwd<16, false>);
    fn(x0, M, K0p, w1, b1, w2, b2, w3, b3, w4, b4, partial, H, Hp, a1, a2,
       a3, out, stream);
}

template <int BM, bool FRAG>
static void mlp_launch_bwd(const float* dout, long M, long K0p,
                           const void* a1, const void* a2, const void* a3,
                           const void* w4, const void* w3t,
                           const void* w2t, const void* w1t,
                           long H, long Hp,
                           void* dz1, void* dz2, void* dz3, void* dx0,
                           float* bias_out, hipStream_t stream) {
    const size_t lds = 2 * BM * MLP_LD * sizeof(mbf16);
    mlp_allow_lds(&k_mlp3_bwd<BM, FRAG>, lds);
    const long grid = (M + BM - 1) / BM;
    k_mlp3_bwd<BM, FRAG><<<(int)grid, 64 * MLP_WAVES, lds, stream>>>(
        dout, M, K0p, (const mbf16*)a1, (const mbf16*)a2, (const mbf16*)a3,
        (const mbf16*)w4, (const mbf16*)w3t, (const mbf16*)w2t,
        (const mbf16*)w1t, H, Hp, (mbf16*)dz1, (mbf16*)dz2, (mbf16*)dz3,
        (mbf16*)dx0, bias_out);
}

extern "C" void emb_mlp3_bwd(const float* dout, long M, long K0p,
                             const void* a1, const void* a2, const void* a3,
                             const void* w4, const void* w3t,
                             const void* w2t, const void* w1t,
                             long H, long Hp,
                             void* dz1, void* dz2, void* dz3, void* dx0,
                             float* bias_out, int bm, int frag,
                             hipStream_t stream) {
    if (M == 0) return;
    // the backward has no x0 tile in LDS: any K0p works with every BM
    bm = mlp_pick_bm(M, 0, bm, true, frag != 0);
    auto fn = frag ? (bm == 64 ? mlp_launch_bwd<64, true>
                      : bm == 32 ? mlp_launch_bwd<32, true>
                                 : mlp_launch_bwd<16, true>)
                   : (bm == 64 ? mlp_launch_bwd<64, false>
                      : bm == 32 ? mlp_launch_bwd<32, false>
                                 : mlp_launch_bwd<16, false>);
    fn(dout, M, K0p, a1, a2, a3, w4, w3t, w2t, w1t, H, Hp, dz1, dz2, dz3,
       dx0, bias_out, stream);
}

// ---------------------------------------------------------- fused wgrads
// dW_L[i,j] += sum_m dz_L[m,i] * a_{L-1}[m,j] for the 3 hidden layers in
// ONE launch. hipBLASLt ran these [H x M]@[M x H'] shapes at ~64 TF
// (64x16 macro tiles, 182 workgroups): here a block computes a 64x64
// fp32 tile, M split m_split ways into an fp32 scratch that a finisher
// folds into the bf16 grads (+=, self-cleaning — the same capture-safe
// pattern as the bias pass).
//
// Both operands are contracted over their ROW index m, so the MFMA wants
// them column-wise. They are staged ROW-major ([m][64 cols], 16-byte
// global loads -> ds_write_b128, one piece = 8 columns of one row) and the
// transpose happens in the LDS read: gfx950's ds_read_b64_tr_b16 hands a
// 16-lane group a 4-row x 16-column block column-major. (The first version
// transposed on the STORE side with 2-byte loads and 2-byte LDS stores:
// 32 load + 32 store instructions per wave and chunk against 8 MFMAs, the
// stores 4-way bank conflicted — staging-bound by instruction count.)
//
// A lane of group g (lane>>4) needs k = 8g..8g+7 of a 32-row MFMA step:
// two transposed reads, rows 8g..8g+3 (elements 0..3) and 8g+4..8g+7
// (elements 4..7) — the same (lane, element) <-> row map as the first
// version, so the fp32 sums, and with them the bf16 grads, come out
// bit-identical to it. Read from plain row order, a 32-lane half (groups
// g, g+1) would touch rows {0..3, 8..11}, which collide pairwise for every
// 16-byte-aligned row stride (8 rows apart = a multiple of 64 banks or of
// 32). So the rows are PERMUTED inside each 32-row step on the store side
// (free: it only changes the store address): logical row 8g + 4h + q
// lives at LDS row 16h + 4g + q. A half then reads 8 CONSECUTIVE LDS rows
// per instruction.
//
// LDS row stride 80 elements = 40 dwords: rows r..r+7 start at banks
// 40r % 64 = {0,40,16,56,32,8,48,24}, eight disjoint 8-bank windows (a
// 16-column block is 32 B = 8 banks), so the transposed reads are
// conflict-free per half; the b128 stores (8 lanes = one 128-B row, next
// row 8 banks on) are too. Columns 64..79 are never read.

#define WG_KC 128           // m-chunk staged per LDS round
#define WG_LD 80            // LDS row stride (elements), see above

// LDS row of logical chunk row r (see above)
static __device__ __forceinline__ int wg_lds_row(int r) {
    return (r & ~31) | ((r & 4) << 2) | ((r & 24) >> 1) | (r & 3);
}

// Transposed fragment read. Preconditions (ISA): every lane supplies an
// in-bounds 8-byte-aligned address and EXEC is all ones — call it only
// from block-uniform control flow.
static __device__ __forceinline__ bf16x8 lds_tr_frag(const mbf16* p) {
    union { s16x4 h[2]; bf16x8 v; } u;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) s16x4* lds_p;
    u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)p);
    u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (lds_p)(p + 16 * WG_LD));
#else
    u.h[0] = u.h[1] = s16x4{0, 0, 0, 0};
#endif
    return u.v;
}

extern "C" __global__ __launch_bounds__(512, 2)
void k_mlp3_wgrad(const mbf16* __restrict__ dz1,   // [M, H]
                  const mbf16* __restrict__ dz2,   // [M, H]
                  const mbf16* __restrict__ dz3,   // [M, H]
                  const mbf16* __restrict__ x0,    // [M, K0p]
                  const mbf16* __restrict__ a1,    // [M, H]
                  const mbf16* __restrict__ a2,    // [M, H]
                  long M, long H, long K0p,
                  long t1, long tk, long th,       // L1 tiles, K0p/H tiles
                  float* __restrict__ scratch,     // [H*K0p + 2*H*H]
                  long m_split,
                  float* __restrict__ bias_out) {  // optional [3*H] bias
    // block -> (layer, i-tile, j-tile)
    long bt = blockIdx.x;
    const mbf16 *dz, *a;
    float* out;
    long ti, tj, jdim, bseg;
    if (bt < t1) {                    // L1: dz1^T @ x0 -> [H, K0p]
        dz = dz1; a = x0; out = scratch; jdim = K0p; bseg = 0;
        ti = bt / tk; tj = bt - ti * tk;
    } else if (bt < t1 + th * th) {   // L2: dz2^T @ a1 -> [H, H]
        bt -= t1;
        dz = dz2; a = a1; out = scratch + H * K0p; jdim = H; bseg = H;
        ti = bt / th; tj = bt - ti * th;
    } else {                          // L3: dz3^T @ a2 -> [H, H]
        bt -= t1 + th * th;
        dz = dz3; a = a2; out = scratch + H * K0p + H * H; jdim = H;
        bseg = 2 * H;
        ti = bt / th; tj = bt - ti * th;
    }
    const long i0 = ti * 64, j0 = tj * 64;
    const long msz = ((M / 32 + m_split - 1) / m_split) * 32;
    const long mbeg = (long)blockIdx.y * msz;
    const long mend = (mbeg + msz < M) ? (mbeg + msz) : M;
    if (mbeg >= M) return;            // block-uniform (tr reads need EXEC=~0)

    __shared__ __attribute__((aligned(16))) mbf16 ldsA[WG_KC * WG_LD];
    __shared__ __attribute__((aligned(16))) mbf16 ldsB[WG_KC * WG_LD];
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;

    // staging: a chunk of one operand is 128 rows x 8 pieces of 16 B;
    // thread t owns piece (t & 7) of rows (t >> 3) and (t >> 3) + 64 of
    // BOTH operands. H and jdim are multiples of 8, so a piece is entirely
    // inside or outside the matrix; outside pieces and rows >= mend stay
    // zero in the registers.
    const int srow = (int)threadIdx.x >> 3, scol = ((int)threadIdx.x & 7) * 8;
    const bool okA = i0 + scol < H, okB = j0 + scol < jdim;
    const mbf16* gA = dz + i0 + scol;
    const mbf16* gB = a + j0 + scol;
    u32x4 ra[2], rb[2];
    auto load_chunk = [&](long m0) {
        #pragma unroll
        for (int h = 0; h < 2; ++h) {
            const long m = m0 + srow + 64 * h;
            ra[h] = u32x4{0u, 0u, 0u, 0u};
            rb[h] = u32x4{0u, 0u, 0u, 0u};
            if (m < mend) {
                if (okA)
                    ra[h] = *reinterpret_cast<const u32x4*>(
                        __builtin_assume_aligned(gA + m * H, 16));
                if (okB)
                    rb[h] = *reinterpret_cast<const u32x4*>(
                        __builtin_assume_aligned(gB + m * jdim, 16));
            }
        }
    };

    // wave w owns output subtiles {w, w+8} of the 4x4 16x16 grid: the two
    // share their column block, so one B fragment feeds both
    f32x4 acc[2];
    acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int si = (wave >> 2) * 16, sj = (wave & 3) * 16;
    // lane 4q+p of a 16-lane group g addresses LDS row 4g+q (logical row
    // 8g+q; +16 LDS rows = logical 8g+4+q), columns 4p..4p+3
    const int toff = (4 * (lane >> 4) + ((lane & 15) >> 2)) * WG_LD
                   + 4 * (lane & 3);
    const bool rider = bias_out != nullptr && tj == 0;   // block-uniform

    load_chunk(mbeg);
    for (long m0 = mbeg; m0 < mend; m0 += WG_KC) {
        __syncthreads();              // previous chunk's reads are done
        #pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int o = wg_lds_row(srow + 64 * h) * WG_LD + scol;
            *reinterpret_cast<u32x4*>(ldsA + o) = ra[h];
            *reinterpret_cast<u32x4*>(ldsB + o) = rb[h];
        }
        __syncthreads();
        // next chunk's global loads fly under this chunk's MFMAs
        if (m0 + WG_KC < mend) load_chunk(m0 + WG_KC);
        if (rider) {
            // bias grads ride along: the dz tile this block just staged IS
            // the operand k_mlp3_bias_bwd used to re-read from HBM — sum
            // its columns here instead (tj==0 blocks only: each (layer,
            // i-tile, m-split) contributes once). 8 threads per column,
            // each walking every 8th row, tree-reduced within the 8-lane
            // group — the first version's summation order, kept so the
            // bias grads stay bit-identical; zeros were staged beyond
            // mend/H so no bounds handling is needed in the sum.
            const int cc = (int)threadIdx.x >> 3, sub = (int)threadIdx.x & 7;
            float s = 0.f;
            for (int mm = sub; mm < WG_KC; mm += 8)
                s += (float)ldsA[wg_lds_row(mm) * WG_LD + cc];
            s += __shfl_down(s, 4);
            s += __shfl_down(s, 2);
            s += __shfl_down(s, 1);
            if (sub == 0 && i0 + cc < H)
                atomicAdd(&bias_out[bseg + i0 + cc], s);
        }
        #pragma unroll
        for (int ks = 0; ks < WG_KC; ks += 32) {
            bf16x8 bv = lds_tr_frag(ldsB + ks * WG_LD + toff + sj);
            bf16x8 a0 = lds_tr_frag(ldsA + ks * WG_LD + toff + si);
            bf16x8 a1v = lds_tr_frag(ldsA + ks * WG_LD + toff + si + 32);
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a0, bv, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a1v, bv, acc[1], 0, 0, 0);
        }
    }
    #pragma unroll
    for (int t = 0; t < 2; ++t) {
        long i = i0 + si + 32 * t + (lane >> 4) * 4;   // C row = A's m-dim = i
        long j = j0 + sj + (lane & 15);
        if (j >= jdim) continue;
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (i + r >= H) break;
            atomicAdd(&out[(i + r) * jdim + j], acc[t][r]);
        }
    }
}

extern "C" __global__ void k_mlp3_wgrad_finish(
        float* __restrict__ scratch, long H, long K0p, long K0,
        mbf16* __restrict__ dw1, mbf16* __restrict__ dw2,
        mbf16* __restrict__ dw3) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long n1 = H * K0p, n23 = H * H;
    if (i >= n1 + 2 * n23) return;
    float v = scratch[i];
    scratch[i] = 0.f;                    // self-cleaning for the next step
    mbf16* dst;
    if (i < n1) {
        long row = i / K0p, col = i - row * K0p;
        if (col >= K0) return;           // x0 pad columns: zero, unfolded
        dst = dw1 + row * K0 + col;      // the PARAM is [H, K0] unpadded
    } else if (i < n1 + n23) {
        dst = dw2 + (i - n1);
    } else {
        dst = dw3 + (i - n1 - n23);
    }
    *dst = (mbf16)((float)*dst + v);     // += matches torch beta=1 accum
}

extern "C" void emb_mlp3_wgrad(const void* dz1, const void* dz2,
                               const void* dz3, const void* x0,
                               const void* a1, const void* a2,
                               long M, long H, long K0p, long K0,
                               float* scratch,
                               void* dw1, void* dw2, void* dw3,
                               float* bias_out, long m_split,
                               hipStream_t stream) {
    if (!M) return;
    // m_split: each split adds a full 64x64 fp32 tile with float atomics
    // (tiles x m_split x 16 KB per step), fewer splits leave CUs idle
    // (126 tiles at the flagship shapes, 2 blocks fit a CU). Measured on
    // MI355X, us for this kernel + its finisher, H=400 K0p=256:
    //   M      split 1   2      4      8      16     (parent, split 8)
    //   1024   14.1    11.9   12.3   16.8   26.6    21.7
    //   2048   21.8    16.8   16.7   20.0   28.3    30.1
    //   4096   37.6    25.4   24.4   26.6   31.9    48.4
    //   8192   69.4    42.8   42.8   45.5   44.7    87.3
    // (table taken with a k-order permuted inside the MFMA step; the
    // committed order measures the same 26.6 at M=4096, 8 splits.)
    // 4 splits are the fastest (2.2 us at the flagship M=4096), but the
    // default stays 8: with the same splits, chunks and k-order as the
    // first version the fp32 sums are bit-identical to it, so a training
    // run differs from that version only by float-atomic order; 4 splits
    // flip an occasional bf16 last bit of a grad in every run
    // (docs/benchmark.md).
    if (m_split <= 0) m_split = 8;
    long th = (H + 63) / 64, tk = (K0p + 63) / 64;
    long t1 = th * tk;
    long tiles = t1 + 2 * th * th;
    dim3 grid((unsigned)tiles, (unsigned)m_split);
    k_mlp3_wgrad<<<grid, 512, 0, stream>>>(
        (const mbf16*)dz1, (const mbf16*)dz2, (const mbf16*)dz3,
        (const mbf16*)x0, (const mbf16*)a1, (const mbf16*)a2, M, H, K0p,
        t1, tk, th, scratch, m_split, bias_out);
    long total = H * K0p + 2 * H * H;
    k_mlp3_wgrad_finish<<<(int)((total + 255) / 256), 256, 0, stream>>>(
        scratch, H, K0p, K0, (mbf16*)dw1, (mbf16*)dw2, (mbf16*)dw3);
}

// ---- fused weight repack ----------------------------------------------
// The train step refreshes six padded weight copies per iteration (three
// plain pads before mlp3_fwd, three transposed pads before mlp3_bwd); as
// separate aten::copy_ launches they cost ~3.8 us EACH while moving <1 MB
// (profiles/step_attrib_r2.txt) — pure launch/ramp. One kernel packs all
// three matrices of a phase. gridDim.y selects the matrix; the valid
// region only is written (padded tails were zeroed once at alloc and
// never change).

struct PackOne {
    const mbf16* src;   // [rows, src_ld] row-major, valid [rows, cols]
    mbf16* dst;         // plain: [rows, dst_ld]; trans: [cols, dst_ld]
    int rows, cols, src_ld, dst_ld, trans;
};

// 2-D mapping: blockIdx.x is a DESTINATION row, threads walk its columns —
// no per-element division (the first version decomposed a 64-bit linear
// index by a runtime divisor, a multi-hundred-instruction emulation per
// element), all indices 32-bit (H, K0p <= a few thousand).
extern "C" __global__ void k_mlp3_pack(PackOne p0, PackOne p1, PackOne p2) {
    PackOne p = blockIdx.y == 0 ? p0 : (blockIdx.y == 1 ? p1 : p2);
    const int d = (int)blockIdx.x;
    if (p.trans) {
        // dst row d = src column d: consecutive threads -> consecutive
        // dst elements (coalesced writes); the strided reads ride L2
        // (matrices are ~100s KB)
        if (d >= p.cols) return;
        const mbf16* src = p.src + d;
        mbf16* dst = p.dst + d * p.dst_ld;
        for (int r = (int)threadIdx.x; r < p.rows; r += (int)blockDim.x)
            dst[r] = src[r * p.src_ld];
    } else {
        if (d >= p.rows) return;
        const mbf16* src = p.src + d * p.src_ld;
        mbf16* dst = p.dst + d * p.dst_ld;
        for (int c = (int)threadIdx.x; c < p.cols; c += (int)blockDim.x)
            dst[c] = src[c];
    }
}

extern "C" void emb_mlp3_pack(const void* w1, void* d1, long r1, long c1,
                              long sld1, long dld1, int t1,
                              const void* w2, void* d2, long r2, long c2,
                              long sld2, long dld2, int t2,
                              const void* w3, void* d3, long r3, long c3,
                              long sld3, long dld3, int t3,
                              hipStream_t stream) {
    PackOne p0{(const mbf16*)w1, (mbf16*)d1, (int)r1, (int)c1, (int)sld1,
               (int)dld1, t1};
    PackOne p1{(const mbf16*)w2, (mbf16*)d2, (int)r2, (int)c2, (int)sld2,
               (int)dld2, t2};
    PackOne p2{(const mbf16*)w3, (mbf16*)d3, (int)r3, (int)c3, (int)sld3,
               (int)dld3, t3};
    // grid.x = most destination rows of the three; block = the longest
    // destination row rounded up to a wave, at most 256
    long mx = 0, mc = 0;
    const PackOne* ps[3] = {&p0, &p1, &p2};
    for (const PackOne* p : ps) {
        if (!p->rows || !p->cols) continue;
        long dr = p->trans ? p->cols : p->rows;
        long dc = p->trans ? p->rows : p->cols;
        if (dr > mx) mx = dr;
        if (dc > mc) mc = dc;
    }
    if (!mx) return;
    int threads = (int)((mc + 63) / 64 * 64);
    if (threads > 256) threads = 256;
    dim3 grid((unsigned)mx, 3);
    k_mlp3_pack<<<grid, threads, 0, stream>>>(p0, p1, p2);
}

// ---- fragment-major weight images -------------------------------------
// One launch writes up to six fragment-major images (layout: top of this
// file): the train step's w1, w2, w3 and the dgrad operands w3^T, w2^T,
// w1^T. gridDim.y selects the matrix, blockIdx.x a 16-column chunk of it,
// and the block's threads walk the chunk's KS x 64 16-byte pieces in
// destination order — thread t writes piece t of a contiguous KS KB run,
// s = t >> 6 and lane = t & 63 are shifts, all indices 32-bit.
//
// The WHOLE destination is written: a piece is assembled in registers and
// every (n, k) outside the source's valid region becomes zero, so the pads
// do not depend on how the buffer was allocated (0 x garbage = NaN).
// Source reads are 2-byte (w1 has 247 columns: its rows are not 16-byte
// aligned) except where a plain source's piece is aligned and entirely
// inside the row; transposed sources read 16 consecutive n per quarter-
// wave and element. Both ride L2 (the matrices are 100s of KB).

struct PackFragOne {
    const mbf16* src;   // [rows, src_ld] row-major, valid [rows, cols]
    mbf16* dst;         // fragment-major image of [N, Kp]
    int rows, cols, src_ld, nch, ks, trans;   // nch = N/16, ks = Kp/32
};

extern "C" __global__ void k_mlp3_pack_frag(
        PackFragOne p0, PackFragOne p1, PackFragOne p2,
        PackFragOne p3, PackFragOne p4, PackFragOne p5) {
    const int y = (int)blockIdx.y;
    PackFragOne p = y == 0 ? p0 : y == 1 ? p1 : y == 2 ? p2
                  : y == 3 ? p3 : y == 4 ? p4 : p5;
    const int ch = (int)blockIdx.x;
    if (ch >= p.nch) return;
    const unsigned short* src =
        reinterpret_cast<const unsigned short*>(p.src);
    u32x4* dst = reinterpret_cast<u32x4*>(p.dst) + ch * p.ks * 64;
    // the image is of W' = src (plain) or src^T (trans): W'[n][k]
    const int nmax = p.trans ? p.cols : p.rows;
    const int kmax = p.trans ? p.rows : p.cols;
    const bool vec = !p.trans && (p.src_ld & 7) == 0
                  && (reinterpret_cast<uintptr_t>(p.src) & 15) == 0;
    for (int t = (int)threadIdx.x; t < p.ks * 64; t += (int)blockDim.x) {
        const int lane = t & 63;
        const int n = ch * 16 + (lane & 15);
        const int k = (t >> 6) * 32 + (lane >> 4) * 8;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (n < nmax && k < kmax) {
            if (vec && k + 8 <= kmax) {
                v = *reinterpret_cast<const u32x4*>(
                    __builtin_assume_aligned(src + n * p.src_ld + k, 16));
            } else {
                const unsigned short* sp =
                    p.trans ? src + k * p.src_ld + n : src + n * p.src_ld + k;
                const int step = p.trans ? p.src_ld : 1;
                unsigned e[8];
                #pragma unroll
                for (int i = 0; i < 8; ++i)
                    e[i] = k + i < kmax ? (unsigned)sp[i * step] : 0u;
                v = u32x4{e[0] | e[1] << 16, e[2] | e[3] << 16,
                          e[4] | e[5] << 16, e[6] | e[7] << 16};
            }
        }
        dst[t] = v;
    }
}

// n <= 6 matrices; rows/cols/src_ld describe the source, N/Kp the image
extern "C" void emb_mlp3_pack_frag(int n, const void* const* srcs,
                                   void* const* dsts, const long* rows,
                                   const long* cols, const long* src_ld,
                                   const long* N, const long* Kp,
                                   const int* trans, hipStream_t stream) {
    PackFragOne p[6] = {};
    int mx = 0, mk = 0;
    for (int i = 0; i < n && i < 6; ++i) {
        p[i] = PackFragOne{(const mbf16*)srcs[i], (mbf16*)dsts[i],
                           (int)rows[i], (int)cols[i], (int)src_ld[i],
                           (int)(N[i] / 16), (int)(Kp[i] / 32), trans[i]};
        if (p[i].nch > mx) mx = p[i].nch;
        if (p[i].ks > mk) mk = p[i].ks;
    }
    if (!mx || !mk) return;
    // one thread per piece of the longest chunk, at most 1024
    int threads = mk * 64 > 1024 ? 1024 : mk * 64;
    dim3 grid((unsigned)mx, (unsigned)n);
    k_mlp3_pack_frag<<<grid, threads, 0, stream>>>(p[0], p[1], p[2], p[3],
                                                   p[4], p[5]);
}
