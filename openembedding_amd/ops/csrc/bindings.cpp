// Torch bindings for the openembedding_amd CDNA4 kernels (embops.hip).
// Tensor-level API consumed by ops/dispatch.py and core/variable_gpu.py.
//
// Two calling modes:
//   exact   — unique_inverse() syncs once to return a tightly-sized unique
//             tensor (needed for the multi-GPU all_to_all splits anyway);
//   bounded — unique_bounded() returns an n-sized buffer + device count and
//             every downstream kernel takes the count as a device pointer,
//             so a whole train step runs with ZERO host syncs (and is
//             hipGraph-capturable).

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>  // ROCm torch masquerades HIP as CUDA here
#include <c10/cuda/CUDAGuard.h>

#include <cstdint>
#include <tuple>
#include <vector>

// torch instantiates data_ptr<int64_t> (long on LP64); the kernel TU uses
// long long — same width, C linkage, so the pointer casts below are safe.
typedef unsigned long long u64;
typedef int64_t i64;
typedef struct ihipStream_t* hipStream_t_;

extern "C" {
void emb_unique(const i64*, long, u64*, int*, long, int*, unsigned char*,
                i64*, i64*, int*, const i64*, int, hipStream_t_);
void emb_unique_indexed(const i64*, long, u64*, int*, long, int*,
                        unsigned char*, i64*, i64*, int*, const i64*, int,
                        int*, int*, int*, int*, int*, int*, int*, long, int*,
                        int*, hipStream_t_);
void emb_unique_indexed_assign(const i64*, long, u64*, int*, long, int*,
                               unsigned char*, i64*, i64*, int*, const i64*,
                               int, int*, int*, int*, int*, int*, int*, int*,
                               long, int*, int*, unsigned char*, long, long,
                               i64*, unsigned char*, hipStream_t_);
void emb_pull_merged(float*, float*, long, long, const i64*, const i64*, int,
                     long, const int*, const int*, const int*, const int*,
                     i64*, int*, i64*, unsigned char*, int, long, long,
                     float*, int, float, float, float, u64, const float*,
                     const int*, hipStream_t_);
int emb_seg_threshold();
int emb_seg_max_dim();
void emb_reduce_by_index(const int*, const int*, const int*, const int*,
                         const int*, long, const float*, long, long,
                         const int*, float*, u64*, hipStream_t_);
void emb_reduce_apply_by_index(int, const int*, const int*, const int*,
                               const int*, const int*, long, const float*,
                               long, long, const int*, const i64*, float*,
                               float*, long, const float*, hipStream_t_);
void emb_ht_lookup(u64*, int*, long, const i64*, long, int*, i64*, i64*,
                   unsigned char*, int, const int*, long, hipStream_t_);
void emb_ht_rehash(const u64*, const int*, long, u64*, int*, long,
                   hipStream_t_);
void emb_ht_lookup_admit(u64*, int*, long, const i64*, long, int*, i64*, long,
                         int*, long, int, u64, int, u64*, i64*,
                         unsigned char*, const int*, hipStream_t_);
void emb_admit_age(int*, long, int, hipStream_t_);
void emb_array_touch(unsigned char*, const i64*, long, long, long, i64*,
                     unsigned char*, const int*, hipStream_t_);
void emb_gather_init(float*, float*, long, long, const i64*,
                     const unsigned char*, const i64*, long, const i64*,
                     float*, int, float, float, float, u64, const float*,
                     const int*, hipStream_t_);
void emb_reduce_by_inverse(const i64*, const float*, long, long, float*, u64*,
                           long, hipStream_t_);
void emb_reduce_bags_by_inverse(const i64*, const float*, long, long,
                                const int*, const i64*, long, int, float*,
                                u64*, long, hipStream_t_);
void emb_pool_fwd(const float*, long, long, const i64*, long, const void*,
                  int, long, const i64*, long, int, float*, int*,
                  hipStream_t_);
void emb_pool_fwd_weighted(const float*, long, long, const i64*, long,
                           const void*, int, long, const i64*, long, int,
                           const float*, float*, int*, float*, hipStream_t_);
void emb_reduce_bags_weighted_by_inverse(const i64*, const float*, long, long,
                                         const int*, const float*,
                                         const float*, long, float*, u64*,
                                         long, hipStream_t_);
void emb_pool_wgrad(const float*, long, long, const i64*, long, const void*,
                    int, long, const float*, const int*, const float*,
                    const float*, const float*, long, int, float*,
                    hipStream_t_);
void emb_pool_lookup(const float*, long, long, const i64*, long, const i64*,
                     long, int, const float*, const u64*, const int*, long,
                     const unsigned char*, long, float*, hipStream_t_);
long emb_quant_stride(int, long);
void emb_quantize_rows(int, const float*, long, long, const i64*, void*,
                       long, hipStream_t_);
void emb_pool_lookup_q(int, const void*, long, long, const i64*, long,
                       const i64*, long, int, const float*, const u64*,
                       const int*, long, const unsigned char*, long, float*,
                       hipStream_t_);
void emb_gather_lookup_q(int, const void*, long, long, const i64*, long,
                         const u64*, const int*, long, const unsigned char*,
                         long, float*, hipStream_t_);
void emb_apply_optimizer(int, float*, float*, long, long, const i64*, long,
                         const float*, const u64*, const float*, const int*,
                         hipStream_t_);
void emb_ctr_head_fwd(const float*, const float*, const float*, const float*, long,
                      long, long, long, long, void*, float*, float*, int,
                      int, hipStream_t_);
void emb_ctr_head_bwd(const float*, const float*, const float*, const void*,
                      const float*, const float*, long, long, long, long,
                      long, float*, float*, float*, float*, int, int,
                      hipStream_t_);
int emb_ctr_head_rows_waves(long, long, long, long, long, int, int);
long emb_ctr_head_rows_bwd_grid(long, long, int);
void emb_ctr_head_fwd_rows(const float*, const float*, const float*,
                           const float*, long, long, long, long, long, void*,
                           float*, float*, int, int, int, hipStream_t_);
void emb_ctr_head_bwd_rows(const float*, const float*, const float*,
                           const void*, const float*, const float*, long,
                           long, long, long, long, float*, float*, float*,
                           float*, int, int, int, hipStream_t_);
void emb_mlp3_bias_bwd(const float*, const void*, const void*, const void*,
                       const void*, long, long, float*, void*, void*, void*,
                       void*, void*, int, int, hipStream_t_);
void emb_mlp3_wgrad(const void*, const void*, const void*, const void*,
                    const void*, const void*, long, long, long, long,
                    float*, void*, void*, void*, float*, long, hipStream_t_);
void emb_mlp3_pack(const void*, void*, long, long, long, long, int,
                   const void*, void*, long, long, long, long, int,
                   const void*, void*, long, long, long, long, int,
                   hipStream_t_);
void emb_bce_fwd(const float*, const float*, long, float*, hipStream_t_);
void emb_bce_bwd(const float*, const float*, long, const float*, float*,
                 hipStream_t_);
void emb_bucketize_pad(const i64*, long, const int*, long, long, i64*, int*,
                       int*, int*, int*, hipStream_t_);
void emb_mask_tail(i64*, float*, u64*, long, long, const int*, hipStream_t_);
void emb_mark_rows(const i64*, long, const unsigned char*, const int*,
                   const int*, int*, long, hipStream_t_);
long emb_delta_tile_rows();
long emb_delta_tiles(long);
void emb_delta_count(const int*, long, int, const int*, const unsigned char*,
                     int*, hipStream_t_);
void emb_delta_compact(const int*, long, int, const int*,
                       const unsigned char*, const int*, i64*, hipStream_t_);
void emb_delta_gather(const float*, const float*, long, long, long,
                      const i64*, long, long, const i64*, long, long, long,
                      const int*, i64*, float*, float*, hipStream_t_);
void emb_expire_flag(const int*, long, int, const int*, const unsigned char*,
                     unsigned char*, hipStream_t_);
void emb_flag_slots(const i64*, long, unsigned char*, long, hipStream_t_);
void emb_expire_count(int, const unsigned char*, long, const int*,
                      const unsigned char*, const int*, int*, hipStream_t_);
void emb_expire_counts(const int*, long, const int*, long, int*,
                       hipStream_t_);
void emb_expire_compact(int, const unsigned char*, long, const int*,
                        const unsigned char*, const int*, const int*, int*,
                        i64*, const i64*, long, long, long, hipStream_t_);
void emb_move_rows(void*, long, long, const int*, const int*, long,
                   const int*, hipStream_t_);
void emb_ht_build(u64*, int*, long, const i64*, long, const int*, int*, long,
                  hipStream_t_);
void emb_expire_array(unsigned char*, const unsigned char*, long,
                      hipStream_t_);
void emb_fault_in(const i64*, long, const int*, const u64*, const int*, long,
                  const float*, const float*, float*, float*, long, long,
                  const i64*, unsigned char*, int*, hipStream_t_);
void emb_spill_rows(const i64*, const i64*, long, const float*, const float*,
                    float*, float*, long, long, hipStream_t_);
void emb_gather_host(const i64*, long, const i64*, const u64*, const int*,
                     long, const float*, float*, long, hipStream_t_);
void emb_gather_pad(const float*, const u64*, long, const int*, long, float*,
                    hipStream_t_);
void emb_scatter_out(const float*, const i64*, long, const int*, long, float*,
                     hipStream_t_);
void emb_split_payload(const float*, long, long, const int*, float*, u64*,
                       hipStream_t_);
void emb_flat_step_scalars(float*, float, float, hipStream_t_);
void emb_flat_opt(int, void*, float*, float*, float*, void*,
                  const float*, long, int, float, float, float, float,
                  hipStream_t_);
void emb_flat_adagrad_f32(float*, float*, const float*, long, float, float,
                          hipStream_t_);
void emb_flat_adagrad_bf16(float*, float*, const void*, void*, long, float,
                           float, hipStream_t_);
void emb_cin_fwd(const float*, const float*, const void*, float*, long,
                 long, long, long, long, hipStream_t_);
void emb_cin_dw(const void*, const void*, const void*, float*, long, long,
                long, long, long, hipStream_t_);
void emb_cin_dx(const float*, const void*, const float*, const float*,
                float*, float*, long, long, long, long, long, hipStream_t_);
void emb_mlp3_fwd(const void*, long, long, const void*, const void*,
                  const void*, const void*, const void*, const void*,
                  const void*, const void*, const float*, long, long, void*,
                  void*, void*, float*, int, int, hipStream_t_);
void emb_mlp3_bwd(const float*, long, long, const void*, const void*,
                  const void*, const void*, const void*, const void*,
                  const void*, long, long, void*, void*, void*, void*,
                  float*, int, int, hipStream_t_);
void emb_mlp3_pack_frag(int, const void* const*, void* const*, const long*,
                        const long*, const long*, const long*, const long*,
                        const int*, hipStream_t_);
}

namespace {

using OptTensor = c10::optional<torch::Tensor>;

hipStream_t_ cur_stream() {
    return reinterpret_cast<hipStream_t_>(
        at::cuda::getCurrentCUDAStream().stream());
}

long next_pow2(long x) {
    long p = 16;
    while (p < x) p <<= 1;
    return p;
}

const int* u_ptr(const OptTensor& u_dev) {
    if (!u_dev.has_value()) return nullptr;
    TORCH_CHECK(u_dev->dtype() == torch::kInt32, "u_dev must be int32");
    return u_dev->data_ptr<int>();
}

#define CHECK_GPU(t) TORCH_CHECK((t).is_cuda(), #t " must be on GPU")
#define CHECK_CONT(t) TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")

// ---- unique ----------------------------------------------------------

// shared body of unique_bounded / unique_bounded_indexed: {uk, inverse,
// counter} and, when ``indexed``, {seg_off, seg_cnt, perm, long_list,
// n_long} behind them
std::vector<torch::Tensor> unique_bounded_impl(
    torch::Tensor keys, OptTensor field_offsets, bool indexed,
    bool stop_after_assign = false, OptTensor valid = c10::nullopt,
    int64_t shard_num = 1) {
    CHECK_GPU(keys); CHECK_CONT(keys);
    TORCH_CHECK(keys.dtype() == torch::kInt64);
    const i64* foff = nullptr;
    int F = 0;
    if (field_offsets.has_value() && field_offsets->numel()) {
        CHECK_GPU(*field_offsets); CHECK_CONT(*field_offsets);
        TORCH_CHECK(field_offsets->dtype() == torch::kInt64,
                    "field_offsets must be int64");
        TORCH_CHECK(keys.numel() % field_offsets->numel() == 0,
                    "keys length must be a multiple of field_offsets");
        foff = field_offsets->data_ptr<i64>();
        F = (int)field_offsets->numel();
    }
    const c10::cuda::CUDAGuard guard(keys.device());
    long n = keys.numel();
    auto opts_i64 = keys.options();
    auto opts_i32 = keys.options().dtype(torch::kInt32);
    auto opts_u8 = keys.options().dtype(torch::kUInt8);
    long cap = next_pow2(2 * n);
    auto tk = torch::empty({cap}, opts_i64);
    auto tv = torch::empty({cap}, opts_i32);
    auto slot_of = torch::empty({n}, opts_i32);
    auto is_first = torch::empty({n}, opts_u8);
    auto uk = torch::empty({n}, opts_i64);  // tail unread
    auto inverse = torch::empty({n}, opts_i64);
    auto counter = torch::empty({1}, opts_i32);
    if (!indexed) {
        emb_unique(keys.data_ptr<i64>(), n, (u64*)tk.data_ptr<i64>(),
                   tv.data_ptr<int>(), cap, slot_of.data_ptr<int>(),
                   is_first.data_ptr<uint8_t>(), uk.data_ptr<i64>(),
                   inverse.data_ptr<i64>(), counter.data_ptr<int>(), foff, F,
                   cur_stream());
        return {uk, inverse, counter};
    }
    TORCH_CHECK(n < (1L << 31), "unique_bounded_indexed: n must fit int32");
    // tcount | toff share one allocation, seg_off | seg_cnt | perm | rank
    // another; the two bump counters sit 64 bytes apart
    auto tct = torch::empty({2, cap}, opts_i32);
    auto segs = torch::empty({4, n}, opts_i32);
    long long_cap = n / (emb_seg_threshold() + 1) + 1;
    auto long_list = torch::empty({long_cap}, opts_i32);
    auto ctr = torch::empty({32}, opts_i32);
    auto seg_off = segs.select(0, 0), seg_cnt = segs.select(0, 1);
    auto perm = segs.select(0, 2), rank = segs.select(0, 3);
    auto n_long = ctr.narrow(0, 16, 1);
    if (stop_after_assign) {
        // the form k_pull_merged continues from: the scratch it resolves
        // (slot_of, tv, toff, rank) comes back beside the results, and the
        // array touch runs inside the assign kernel when ``valid`` is given
        auto slots = torch::empty({n}, opts_i64);
        auto new_mask = torch::empty({n}, opts_u8);
        unsigned char* vptr = nullptr;
        long vcap = 0;
        if (valid.has_value()) {
            CHECK_GPU(*valid); CHECK_CONT(*valid);
            TORCH_CHECK(valid->dtype() == torch::kUInt8 && shard_num >= 1,
                        "unique_bounded_assign: valid must be uint8");
            vptr = valid->data_ptr<uint8_t>();
            vcap = valid->numel();
        }
        emb_unique_indexed_assign(
            keys.data_ptr<i64>(), n, (u64*)tk.data_ptr<i64>(),
            tv.data_ptr<int>(), cap, slot_of.data_ptr<int>(),
            is_first.data_ptr<uint8_t>(), uk.data_ptr<i64>(),
            inverse.data_ptr<i64>(), counter.data_ptr<int>(), foff, F,
            tct.data_ptr<int>(), tct.data_ptr<int>() + cap,
            rank.data_ptr<int>(), seg_off.data_ptr<int>(),
            seg_cnt.data_ptr<int>(), perm.data_ptr<int>(),
            long_list.data_ptr<int>(), long_cap, ctr.data_ptr<int>(),
            n_long.data_ptr<int>(), vptr, shard_num, vcap,
            slots.data_ptr<i64>(), new_mask.data_ptr<uint8_t>(),
            cur_stream());
        return {uk, inverse, counter, seg_off, seg_cnt, perm, long_list,
                n_long, slot_of, tv, tct.select(0, 1), rank, slots, new_mask};
    }
    emb_unique_indexed(keys.data_ptr<i64>(), n, (u64*)tk.data_ptr<i64>(),
                       tv.data_ptr<int>(), cap, slot_of.data_ptr<int>(),
                       is_first.data_ptr<uint8_t>(), uk.data_ptr<i64>(),
                       inverse.data_ptr<i64>(), counter.data_ptr<int>(), foff,
                       F, tct.data_ptr<int>(), tct.data_ptr<int>() + cap,
                       rank.data_ptr<int>(), seg_off.data_ptr<int>(),
                       seg_cnt.data_ptr<int>(), perm.data_ptr<int>(),
                       long_list.data_ptr<int>(), long_cap,
                       ctr.data_ptr<int>(), n_long.data_ptr<int>(),
                       cur_stream());
    return {uk, inverse, counter, seg_off, seg_cnt, perm, long_list, n_long};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> unique_bounded(
    torch::Tensor keys, OptTensor field_offsets) {
    auto r = unique_bounded_impl(keys, field_offsets, false);
    return {r[0], r[1], r[2]};
}

// unique_bounded plus the inverted index of the batch (embops.hip,
// "segmented reduce"): uid's elements are perm[seg_off[uid] ..
// seg_off[uid] + seg_cnt[uid]); long_list[:n_long] names the uids with more
// than seg_reduce_threshold() elements. All int32, device-resident.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
unique_bounded_indexed(torch::Tensor keys, OptTensor field_offsets) {
    auto r = unique_bounded_impl(keys, field_offsets, true);
    return {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
}

// unique_bounded_indexed without its last kernel, for pull_merged: returns
// {uk, inverse, u_dev, seg_off, seg_cnt, perm, long_list, n_long, slot_of,
// tv, toff, rank, slots, new_mask}. inverse and perm are completed by
// pull_merged. With ``valid`` (array table) the assign kernel also touches
// the table: slots / new_mask are filled below u_dev and valid is updated;
// without it they come back unset, for ht_lookup's results.
std::vector<torch::Tensor> unique_bounded_assign(
    torch::Tensor keys, OptTensor field_offsets, OptTensor valid,
    int64_t shard_num) {
    return unique_bounded_impl(keys, field_offsets, true, true, valid,
                               shard_num);
}

// The rest of a bounded pull after unique_bounded_assign (and ht_lookup for
// a hash table): inverse, perm and gather + lazy init in one launch.
// ``array_cap`` > 0: array table of that many rows, the slot comes from the
// element's own key and the tail of slots / new_mask is written here;
// 0: slots [n] is read per uid. ``keys`` is the dedup's input (raw field ids
// with ``field_offsets``).
torch::Tensor pull_merged(torch::Tensor weights, torch::Tensor state,
                          torch::Tensor keys, OptTensor field_offsets,
                          torch::Tensor slot_of, torch::Tensor tv,
                          torch::Tensor toff, torch::Tensor rank,
                          torch::Tensor inverse, torch::Tensor perm,
                          torch::Tensor slots, torch::Tensor new_mask,
                          int64_t array_cap, int64_t shard_num,
                          int64_t init_cat, double p0, double p1, double p2,
                          int64_t seed, torch::Tensor state_init_row,
                          bool want_out, torch::Tensor u_dev) {
    CHECK_GPU(weights); CHECK_CONT(weights);
    CHECK_GPU(keys); CHECK_CONT(keys);
    TORCH_CHECK(weights.dtype() == torch::kFloat32 && weights.dim() == 2
                && keys.dtype() == torch::kInt64, "pull_merged dtypes");
    long n = keys.numel();
    TORCH_CHECK(n < (1L << 31), "pull_merged: n must fit int32");
    for (const auto* t : {&slot_of, &tv, &toff, &rank, &perm, &u_dev}) {
        CHECK_GPU(*t); CHECK_CONT(*t);
        TORCH_CHECK(t->dtype() == torch::kInt32,
                    "pull_merged: index tensors must be int32");
    }
    CHECK_GPU(inverse); CHECK_CONT(inverse); CHECK_GPU(slots);
    CHECK_CONT(slots); CHECK_GPU(new_mask); CHECK_CONT(new_mask);
    TORCH_CHECK(inverse.dtype() == torch::kInt64
                && slots.dtype() == torch::kInt64
                && new_mask.dtype() == torch::kUInt8, "pull_merged dtypes");
    TORCH_CHECK(slot_of.numel() == n && rank.numel() == n
                && perm.numel() == n && inverse.numel() == n
                && slots.numel() == n && new_mask.numel() == n
                && tv.numel() == toff.numel() && u_dev.numel() == 1,
                "pull_merged: scratch does not match keys");
    TORCH_CHECK(array_cap >= 0 && array_cap <= weights.size(0)
                && shard_num >= 1, "pull_merged: array_cap beyond the table");
    const i64* foff = nullptr;
    int F = 0;
    if (field_offsets.has_value() && field_offsets->numel()) {
        CHECK_GPU(*field_offsets); CHECK_CONT(*field_offsets);
        TORCH_CHECK(field_offsets->dtype() == torch::kInt64
                    && n % field_offsets->numel() == 0,
                    "pull_merged: field_offsets");
        foff = field_offsets->data_ptr<i64>();
        F = (int)field_offsets->numel();
    }
    const c10::cuda::CUDAGuard guard(weights.device());
    long dim = weights.size(1);
    long sd = state.numel() ? state.size(1) : 0;
    if (sd) {
        CHECK_GPU(state); CHECK_CONT(state);
        CHECK_GPU(state_init_row); CHECK_CONT(state_init_row);
        TORCH_CHECK(state.size(0) == weights.size(0)
                    && state_init_row.numel() >= sd,
                    "pull_merged: state does not match the table");
    }
    torch::Tensor out;
    float* out_ptr = nullptr;
    if (want_out) {
        out = torch::empty({n, dim}, weights.options());
        out_ptr = out.data_ptr<float>();
    } else {
        out = torch::empty({0}, weights.options());
    }
    if (init_cat == 1) p1 = p1 - p0;   // the span, as gather_init passes it
    emb_pull_merged(weights.data_ptr<float>(),
                    sd ? state.data_ptr<float>() : nullptr, dim, sd,
                    keys.data_ptr<i64>(), foff, F, n,
                    slot_of.data_ptr<int>(), tv.data_ptr<int>(),
                    toff.data_ptr<int>(), rank.data_ptr<int>(),
                    inverse.data_ptr<i64>(), perm.data_ptr<int>(),
                    slots.data_ptr<i64>(), new_mask.data_ptr<uint8_t>(),
                    array_cap > 0 ? 1 : 0, shard_num, array_cap, out_ptr,
                    (int)init_cat, (float)p0, (float)p1, (float)p2,
                    (u64)seed,
                    sd ? state_init_row.data_ptr<float>() : nullptr,
                    u_dev.data_ptr<int>(), cur_stream());
    return out;
}

std::tuple<torch::Tensor, torch::Tensor> unique_inverse(torch::Tensor keys) {
    auto r = unique_bounded(keys, c10::nullopt);
    long u = std::get<2>(r).item<int>();  // host sync
    return {std::get<0>(r).narrow(0, 0, u), std::get<1>(r)};
}

// ---- persistent hash table -------------------------------------------

std::tuple<torch::Tensor, torch::Tensor> ht_lookup(
    torch::Tensor tk, torch::Tensor tv, torch::Tensor keys,
    torch::Tensor nrows, torch::Tensor slot_keys, bool insert,
    OptTensor u_dev) {
    CHECK_GPU(keys); CHECK_CONT(keys);
    const c10::cuda::CUDAGuard guard(keys.device());
    long n = keys.numel();
    auto slots = torch::empty({n}, keys.options());
    auto new_mask = torch::empty({n}, keys.options().dtype(torch::kUInt8));
    if (n)
        emb_ht_lookup((u64*)tk.data_ptr<i64>(), tv.data_ptr<int>(),
                      tk.numel(), keys.data_ptr<i64>(), n,
                      nrows.data_ptr<int>(), slot_keys.data_ptr<i64>(),
                      slots.data_ptr<i64>(), new_mask.data_ptr<uint8_t>(),
                      insert ? 1 : 0, u_ptr(u_dev), slot_keys.numel(),
                      cur_stream());
    return {slots, new_mask};
}

// ---- feature admission ---------------------------------------------------
// ht_lookup(insert = true) behind a count-min filter (embops.hip, "feature
// admission"): a key that misses adds one sighting to ``sketch`` (int32
// [depth * width], width a power of two) and is inserted only when its
// estimate reaches ``min_count``; otherwise its slot is -1. ``stats`` (int64
// [2]) gains the admitted and the turned-away sightings.

void check_sketch(const torch::Tensor& sketch, int64_t depth) {
    CHECK_GPU(sketch); CHECK_CONT(sketch);
    TORCH_CHECK(sketch.dtype() == torch::kInt32, "sketch must be int32");
    TORCH_CHECK(depth >= 1 && depth <= 8, "depth must be in 1..8");
    long W = sketch.numel() / depth;
    TORCH_CHECK(W >= 1 && W * depth == sketch.numel() && (W & (W - 1)) == 0,
                "sketch must hold depth rows of a power-of-two width");
}

std::tuple<torch::Tensor, torch::Tensor> ht_lookup_admit(
    torch::Tensor tk, torch::Tensor tv, torch::Tensor keys,
    torch::Tensor nrows, torch::Tensor slot_keys, torch::Tensor sketch,
    int64_t depth, int64_t seed, int64_t min_count, torch::Tensor stats,
    OptTensor u_dev) {
    CHECK_GPU(keys); CHECK_CONT(keys);
    TORCH_CHECK(keys.dtype() == torch::kInt64);
    check_sketch(sketch, depth);
    CHECK_GPU(stats); CHECK_CONT(stats);
    TORCH_CHECK(stats.dtype() == torch::kInt64 && stats.numel() == 2,
                "stats must be int64 [2]");
    TORCH_CHECK(min_count >= 1 && min_count <= INT32_MAX,
                "min_count must be a positive int32");
    const c10::cuda::CUDAGuard guard(keys.device());
    long n = keys.numel();
    auto slots = torch::empty({n}, keys.options());
    auto new_mask = torch::empty({n}, keys.options().dtype(torch::kUInt8));
    if (n)
        emb_ht_lookup_admit((u64*)tk.data_ptr<i64>(), tv.data_ptr<int>(),
                            tk.numel(), keys.data_ptr<i64>(), n,
                            nrows.data_ptr<int>(), slot_keys.data_ptr<i64>(),
                            slot_keys.numel(), sketch.data_ptr<int>(),
                            sketch.numel() / depth, (int)depth, (u64)seed,
                            (int)min_count, (u64*)stats.data_ptr<i64>(),
                            slots.data_ptr<i64>(),
                            new_mask.data_ptr<uint8_t>(), u_ptr(u_dev),
                            cur_stream());
    return {slots, new_mask};
}

// every counter >> shift in place; shift >= 31 zeroes the sketch
void admit_age(torch::Tensor sketch, int64_t shift) {
    CHECK_GPU(sketch); CHECK_CONT(sketch);
    TORCH_CHECK(sketch.dtype() == torch::kInt32, "sketch must be int32");
    TORCH_CHECK(shift >= 0, "shift must not be negative");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(sketch.data_ptr()) % 16 == 0,
                "sketch must be 16-byte aligned");
    const c10::cuda::CUDAGuard guard(sketch.device());
    emb_admit_age(sketch.data_ptr<int>(), sketch.numel(),
                  (int)(shift > 31 ? 31 : shift), cur_stream());
}

void ht_rehash(torch::Tensor tk_old, torch::Tensor tv_old, torch::Tensor tk_new,
               torch::Tensor tv_new) {
    const c10::cuda::CUDAGuard guard(tk_old.device());
    emb_ht_rehash((u64*)tk_old.data_ptr<i64>(), tv_old.data_ptr<int>(),
                  tk_old.numel(), (u64*)tk_new.data_ptr<i64>(),
                  tv_new.data_ptr<int>(), tk_new.numel(), cur_stream());
}

// ---- array table ------------------------------------------------------

std::tuple<torch::Tensor, torch::Tensor> array_touch(
    torch::Tensor valid, torch::Tensor keys, int64_t shard_num,
    OptTensor u_dev) {
    const c10::cuda::CUDAGuard guard(valid.device());
    long n = keys.numel();
    auto slots = torch::empty({n}, keys.options());
    auto new_mask = torch::empty({n}, keys.options().dtype(torch::kUInt8));
    if (n)
        emb_array_touch(valid.data_ptr<uint8_t>(), keys.data_ptr<i64>(), n,
                        shard_num, valid.numel(), slots.data_ptr<i64>(),
                        new_mask.data_ptr<uint8_t>(), u_ptr(u_dev),
                        cur_stream());
    return {slots, new_mask};
}

// ---- gather + lazy init ----------------------------------------------

torch::Tensor gather_init(torch::Tensor weights, torch::Tensor state,
                          torch::Tensor slots, torch::Tensor new_mask,
                          torch::Tensor keys, OptTensor inverse,
                          int64_t init_cat, double p0, double p1, double p2,
                          int64_t seed, torch::Tensor state_init_row,
                          bool want_out, OptTensor u_dev) {
    CHECK_GPU(weights); CHECK_CONT(weights);
    const c10::cuda::CUDAGuard guard(weights.device());
    long n = inverse.has_value() ? inverse->numel() : keys.numel();
    long dim = weights.size(1);
    long sd = state.numel() ? state.size(1) : 0;
    torch::Tensor out;
    float* out_ptr = nullptr;
    if (want_out) {
        out = torch::empty({n, dim}, weights.options());
        out_ptr = out.data_ptr<float>();
    } else {
        out = torch::empty({0}, weights.options());
    }
    // uniform (init_cat 1): the kernel takes the span, subtracted in double
    // and rounded once as core/rng.py does, so both sides multiply by the
    // same float for any (minval, maxval)
    if (init_cat == 1) p1 = p1 - p0;
    emb_gather_init(weights.data_ptr<float>(),
                    sd ? state.data_ptr<float>() : nullptr, dim, sd,
                    slots.data_ptr<i64>(),
                    new_mask.numel() ? new_mask.data_ptr<uint8_t>() : nullptr,
                    keys.data_ptr<i64>(), n,
                    inverse.has_value() ? inverse->data_ptr<i64>() : nullptr,
                    out_ptr, (int)init_cat,
                    (float)p0, (float)p1, (float)p2, (u64)seed,
                    sd ? state_init_row.data_ptr<float>() : nullptr,
                    u_ptr(u_dev), cur_stream());
    return out;
}

// ---- reduce-by-key ----------------------------------------------------

std::tuple<torch::Tensor, torch::Tensor> reduce_by_inverse(
    torch::Tensor inverse, torch::Tensor grads, int64_t u) {
    CHECK_GPU(grads); CHECK_CONT(grads);
    TORCH_CHECK(grads.dtype() == torch::kFloat32,
                "reduce_by_inverse: grads must be float32");
    const c10::cuda::CUDAGuard guard(grads.device());
    long n = grads.size(0);
    long dim = grads.size(1);
    auto ugrads = torch::empty({u, dim}, grads.options());
    auto counts = torch::empty({u}, grads.options().dtype(torch::kInt64));
    emb_reduce_by_inverse(inverse.data_ptr<i64>(), grads.data_ptr<float>(), n,
                          dim, ugrads.data_ptr<float>(),
                          (u64*)counts.data_ptr<i64>(), u, cur_stream());
    return {ugrads, counts};
}

// Same (ugrads [n, dim], counts [n]) as reduce_by_inverse(inverse, grads, n),
// summed through the inverted index of unique_bounded_indexed: no atomics,
// and rows at and beyond *u_dev come back as zeros with count 0.
std::tuple<torch::Tensor, torch::Tensor> reduce_by_index(
    torch::Tensor seg_off, torch::Tensor seg_cnt, torch::Tensor perm,
    torch::Tensor long_list, torch::Tensor n_long, torch::Tensor grads,
    torch::Tensor u_dev) {
    CHECK_GPU(grads); CHECK_CONT(grads);
    TORCH_CHECK(grads.dtype() == torch::kFloat32 && grads.dim() == 2,
                "reduce_by_index: grads must be float32 [n, dim]");
    long n = grads.size(0);
    long dim = grads.size(1);
    TORCH_CHECK(dim <= emb_seg_max_dim(),
                "reduce_by_index: dim above the kernel's ladder");
    for (const auto* t : {&seg_off, &seg_cnt, &perm, &long_list, &n_long,
                          &u_dev}) {
        CHECK_GPU(*t); CHECK_CONT(*t);
        TORCH_CHECK(t->dtype() == torch::kInt32,
                    "reduce_by_index: index tensors must be int32");
    }
    TORCH_CHECK(seg_off.numel() == n && seg_cnt.numel() == n
                && perm.numel() == n,
                "reduce_by_index: index does not match grads");
    TORCH_CHECK(n_long.numel() == 1 && u_dev.numel() == 1);
    const c10::cuda::CUDAGuard guard(grads.device());
    auto ugrads = torch::empty({n, dim}, grads.options());
    auto counts = torch::empty({n}, grads.options().dtype(torch::kInt64));
    emb_reduce_by_index(seg_off.data_ptr<int>(), seg_cnt.data_ptr<int>(),
                        perm.data_ptr<int>(), long_list.data_ptr<int>(),
                        n_long.data_ptr<int>(), long_list.numel(),
                        grads.data_ptr<float>(), n, dim,
                        u_dev.data_ptr<int>(), ugrads.data_ptr<float>(),
                        (u64*)counts.data_ptr<i64>(), cur_stream());
    return {ugrads, counts};
}

// reduce_by_index followed by apply_optimizer on its result, as one launch:
// the per-unique sums are applied to the rows behind ``slots`` (int64 [n],
// saved from the pull) where they are formed. uids at and beyond *u_dev and
// slots < 0 are skipped.
void reduce_apply_by_index(
    int64_t opt, torch::Tensor weights, torch::Tensor state,
    torch::Tensor slots, torch::Tensor seg_off, torch::Tensor seg_cnt,
    torch::Tensor perm, torch::Tensor long_list, torch::Tensor n_long,
    torch::Tensor grads, std::vector<double> cfg, torch::Tensor u_dev) {
    CHECK_GPU(grads); CHECK_CONT(grads);
    CHECK_GPU(weights); CHECK_CONT(weights);
    CHECK_GPU(slots); CHECK_CONT(slots);
    TORCH_CHECK(grads.dtype() == torch::kFloat32 && grads.dim() == 2,
                "reduce_apply_by_index: grads must be float32 [n, dim]");
    TORCH_CHECK(weights.dtype() == torch::kFloat32 && weights.dim() == 2,
                "reduce_apply_by_index: weights must be float32 [R, dim]");
    TORCH_CHECK(opt >= 0 && opt <= 8, "reduce_apply_by_index: optimizer id");
    long n = grads.size(0);
    long dim = grads.size(1);
    TORCH_CHECK(dim == weights.size(1),
                "reduce_apply_by_index: grads do not match the table's dim");
    TORCH_CHECK(dim <= emb_seg_max_dim(),
                "reduce_apply_by_index: dim above the kernel's ladder");
    for (const auto* t : {&seg_off, &seg_cnt, &perm, &long_list, &n_long,
                          &u_dev}) {
        CHECK_GPU(*t); CHECK_CONT(*t);
        TORCH_CHECK(t->dtype() == torch::kInt32,
                    "reduce_apply_by_index: index tensors must be int32");
    }
    TORCH_CHECK(seg_off.numel() == n && seg_cnt.numel() == n
                && perm.numel() == n,
                "reduce_apply_by_index: index does not match grads");
    TORCH_CHECK(slots.dtype() == torch::kInt64 && slots.numel() == n,
                "reduce_apply_by_index: slots must be int64 [n]");
    TORCH_CHECK(n_long.numel() == 1 && u_dev.numel() == 1);
    long sd = state.numel() ? state.size(1) : 0;
    if (sd) {
        CHECK_GPU(state); CHECK_CONT(state);
        TORCH_CHECK(state.dtype() == torch::kFloat32
                    && state.size(0) == weights.size(0),
                    "reduce_apply_by_index: state must be float32 [R, sd]");
    }
    const c10::cuda::CUDAGuard guard(grads.device());
    float c[7] = {0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < cfg.size() && i < 7; ++i) c[i] = (float)cfg[i];
    emb_reduce_apply_by_index(
        (int)opt, seg_off.data_ptr<int>(), seg_cnt.data_ptr<int>(),
        perm.data_ptr<int>(), long_list.data_ptr<int>(),
        n_long.data_ptr<int>(), long_list.numel(), grads.data_ptr<float>(),
        n, dim, u_dev.data_ptr<int>(), slots.data_ptr<i64>(),
        weights.data_ptr<float>(), sd ? state.data_ptr<float>() : nullptr,
        sd, c, cur_stream());
}

// ---- multi-hot bags: pooled gather + bag-indirected reduce ------------

// rows [R, dim] f32; inverse (optional: identity) int64 [nnz]; map
// (optional) int64 or int32 [u], -1 = zero row; offsets int64 [B+1];
// mode 0 sum / 1 mean / 2 sqrtn. Returns (out [B, dim], bag_of int32
// [nnz]; empty when !want_bag_of).
std::tuple<torch::Tensor, torch::Tensor> pool_fwd(
    torch::Tensor rows, OptTensor inverse, OptTensor map,
    torch::Tensor offsets, int64_t mode, bool want_bag_of) {
    CHECK_GPU(rows); CHECK_CONT(rows);
    CHECK_GPU(offsets); CHECK_CONT(offsets);
    TORCH_CHECK(rows.dtype() == torch::kFloat32 && rows.dim() == 2,
                "pool_fwd: rows must be float32 [R, dim]");
    TORCH_CHECK(offsets.dtype() == torch::kInt64 && offsets.dim() == 1
                && offsets.numel() >= 1,
                "pool_fwd: offsets must be int64 [B+1]");
    TORCH_CHECK(mode >= 0 && mode <= 2, "pool_fwd: bad mode");
    const void* map_ptr = nullptr;
    int map_kind = 0;
    long u = 0;
    if (map.has_value()) {
        CHECK_GPU(*map); CHECK_CONT(*map);
        u = map->numel();
        if (map->dtype() == torch::kInt64) {
            map_kind = 1;
            map_ptr = map->data_ptr<i64>();
        } else {
            TORCH_CHECK(map->dtype() == torch::kInt32,
                        "pool_fwd: map must be int64 or int32");
            map_kind = 2;
            map_ptr = map->data_ptr<int>();
        }
    }
    long R = rows.size(0), dim = rows.size(1);
    long nnz = map_kind ? u : R;
    const i64* inv_ptr = nullptr;
    if (inverse.has_value()) {
        CHECK_GPU(*inverse); CHECK_CONT(*inverse);
        TORCH_CHECK(inverse->dtype() == torch::kInt64,
                    "pool_fwd: inverse must be int64");
        nnz = inverse->numel();
        inv_ptr = inverse->data_ptr<i64>();
    }
    const c10::cuda::CUDAGuard guard(rows.device());
    long B = offsets.numel() - 1;
    auto out = torch::empty({B, dim}, rows.options());
    auto bag_of = torch::empty({want_bag_of ? nnz : 0},
                               rows.options().dtype(torch::kInt32));
    emb_pool_fwd(rows.data_ptr<float>(), R, dim, inv_ptr, nnz, map_ptr,
                 map_kind, u, offsets.data_ptr<i64>(), B, (int)mode,
                 out.data_ptr<float>(),
                 want_bag_of ? bag_of.data_ptr<int>() : nullptr,
                 cur_stream());
    return {out, bag_of};
}

// Same (ugrads [u, dim], counts [u]) as reduce_by_inverse over the
// expanded gradient grad_out[bag_of[e]] * scale[bag_of[e]], without
// building it; elements with bag_of < 0 are skipped.
std::tuple<torch::Tensor, torch::Tensor> reduce_bags_by_inverse(
    torch::Tensor inverse, torch::Tensor grad_out, torch::Tensor bag_of,
    torch::Tensor offsets, int64_t mode, int64_t u) {
    CHECK_GPU(grad_out); CHECK_CONT(grad_out);
    CHECK_GPU(inverse); CHECK_CONT(inverse);
    CHECK_GPU(bag_of); CHECK_CONT(bag_of);
    CHECK_GPU(offsets); CHECK_CONT(offsets);
    TORCH_CHECK(grad_out.dtype() == torch::kFloat32 && grad_out.dim() == 2,
                "reduce_bags_by_inverse: grad_out must be float32 [B, dim]");
    TORCH_CHECK(inverse.dtype() == torch::kInt64
                && bag_of.dtype() == torch::kInt32
                && offsets.dtype() == torch::kInt64,
                "reduce_bags_by_inverse dtypes");
    TORCH_CHECK(bag_of.numel() == inverse.numel(),
                "reduce_bags_by_inverse: bag_of/inverse length mismatch");
    TORCH_CHECK(offsets.numel() == grad_out.size(0) + 1,
                "reduce_bags_by_inverse: offsets must be [B+1]");
    TORCH_CHECK(mode >= 0 && mode <= 2, "reduce_bags_by_inverse: bad mode");
    const c10::cuda::CUDAGuard guard(grad_out.device());
    long n = inverse.numel();
    long B = grad_out.size(0);
    long dim = grad_out.size(1);
    auto ugrads = torch::empty({u, dim}, grad_out.options());
    auto counts = torch::empty({u}, grad_out.options().dtype(torch::kInt64));
    emb_reduce_bags_by_inverse(inverse.data_ptr<i64>(),
                               grad_out.data_ptr<float>(), n, dim,
                               bag_of.data_ptr<int>(),
                               offsets.data_ptr<i64>(), B, (int)mode,
                               ugrads.data_ptr<float>(),
                               (u64*)counts.data_ptr<i64>(), u,
                               cur_stream());
    return {ugrads, counts};
}

// ---- per-sample weights ------------------------------------------------

// the (inverse -> map -> rows) index chain shared by the weighted pool and
// its weight gradient; nnz is the element count it implies
struct PoolChain {
    const i64* inv_ptr = nullptr;
    const void* map_ptr = nullptr;
    int map_kind = 0;
    long u = 0, nnz = 0;
};

static PoolChain pool_chain(const char* who, const torch::Tensor& rows,
                            const OptTensor& inverse, const OptTensor& map) {
    PoolChain c;
    if (map.has_value()) {
        CHECK_GPU(*map); CHECK_CONT(*map);
        c.u = map->numel();
        if (map->dtype() == torch::kInt64) {
            c.map_kind = 1;
            c.map_ptr = map->data_ptr<i64>();
        } else {
            TORCH_CHECK(map->dtype() == torch::kInt32, who,
                        ": map must be int64 or int32");
            c.map_kind = 2;
            c.map_ptr = map->data_ptr<int>();
        }
    }
    c.nnz = c.map_kind ? c.u : rows.size(0);
    if (inverse.has_value()) {
        CHECK_GPU(*inverse); CHECK_CONT(*inverse);
        TORCH_CHECK(inverse->dtype() == torch::kInt64, who,
                    ": inverse must be int64");
        c.nnz = inverse->numel();
        c.inv_ptr = inverse->data_ptr<i64>();
    }
    return c;
}

// pool_fwd with per-sample weights (float32 [nnz]): out[b] = scale_b *
// sum_j w_j * row_j, scale_b = 1 | 1/sum w | 1/sqrt(sum w^2) (0 when the
// denominator is 0). Returns (out [B, dim], bag_of int32 [nnz], bag_scale
// float32 [B]); ``out_buf`` / ``scale_buf`` (optional) are written instead
// of fresh allocations.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> pool_fwd_weighted(
    torch::Tensor rows, OptTensor inverse, OptTensor map,
    torch::Tensor offsets, torch::Tensor weights, int64_t mode,
    OptTensor out_buf, OptTensor scale_buf) {
    CHECK_GPU(rows); CHECK_CONT(rows);
    CHECK_GPU(offsets); CHECK_CONT(offsets);
    CHECK_GPU(weights); CHECK_CONT(weights);
    TORCH_CHECK(rows.dtype() == torch::kFloat32 && rows.dim() == 2
                && rows.size(1) >= 1,
                "pool_fwd_weighted: rows must be float32 [R, dim >= 1]");
    TORCH_CHECK(offsets.dtype() == torch::kInt64 && offsets.dim() == 1
                && offsets.numel() >= 1,
                "pool_fwd_weighted: offsets must be int64 [B+1]");
    TORCH_CHECK(mode >= 0 && mode <= 2, "pool_fwd_weighted: bad mode");
    PoolChain c = pool_chain("pool_fwd_weighted", rows, inverse, map);
    TORCH_CHECK(weights.dtype() == torch::kFloat32 && weights.dim() == 1
                && weights.numel() == c.nnz,
                "pool_fwd_weighted: weights must be float32 [nnz]");
    const c10::cuda::CUDAGuard guard(rows.device());
    long R = rows.size(0), dim = rows.size(1);
    long B = offsets.numel() - 1;
    // caller-provided outputs (optional) must have exactly the shapes
    // allocated here
    auto out = out_buf.has_value() ? *out_buf
                                   : torch::empty({B, dim}, rows.options());
    auto bag_scale = scale_buf.has_value()
        ? *scale_buf : torch::empty({B}, rows.options());
    CHECK_GPU(out); CHECK_CONT(out);
    CHECK_GPU(bag_scale); CHECK_CONT(bag_scale);
    TORCH_CHECK(out.dtype() == torch::kFloat32 && out.dim() == 2
                && out.size(0) == B && out.size(1) == dim,
                "pool_fwd_weighted: out must be float32 [B, dim]");
    TORCH_CHECK(bag_scale.dtype() == torch::kFloat32
                && bag_scale.dim() == 1 && bag_scale.numel() == B,
                "pool_fwd_weighted: bag_scale must be float32 [B]");
    auto bag_of = torch::empty({c.nnz}, rows.options().dtype(torch::kInt32));
    emb_pool_fwd_weighted(rows.data_ptr<float>(), R, dim, c.inv_ptr, c.nnz,
                          c.map_ptr, c.map_kind, c.u,
                          offsets.data_ptr<i64>(), B, (int)mode,
                          weights.data_ptr<float>(), out.data_ptr<float>(),
                          bag_of.data_ptr<int>(),
                          bag_scale.data_ptr<float>(), cur_stream());
    return {out, bag_of, bag_scale};
}

// reduce_bags_by_inverse with element e's factor weights[e] *
// bag_scale[bag_of[e]] (bag_scale from pool_fwd_weighted); counts do not
// depend on the weights.
std::tuple<torch::Tensor, torch::Tensor> reduce_bags_weighted_by_inverse(
    torch::Tensor inverse, torch::Tensor grad_out, torch::Tensor bag_of,
    torch::Tensor weights, torch::Tensor bag_scale, int64_t u) {
    CHECK_GPU(grad_out); CHECK_CONT(grad_out);
    CHECK_GPU(inverse); CHECK_CONT(inverse);
    CHECK_GPU(bag_of); CHECK_CONT(bag_of);
    CHECK_GPU(weights); CHECK_CONT(weights);
    CHECK_GPU(bag_scale); CHECK_CONT(bag_scale);
    TORCH_CHECK(grad_out.dtype() == torch::kFloat32 && grad_out.dim() == 2,
                "reduce_bags_weighted_by_inverse: grad_out must be float32 "
                "[B, dim]");
    TORCH_CHECK(inverse.dtype() == torch::kInt64
                && bag_of.dtype() == torch::kInt32
                && weights.dtype() == torch::kFloat32
                && bag_scale.dtype() == torch::kFloat32,
                "reduce_bags_weighted_by_inverse dtypes");
    TORCH_CHECK(bag_of.numel() == inverse.numel()
                && weights.numel() == inverse.numel(),
                "reduce_bags_weighted_by_inverse: bag_of/weights/inverse "
                "length mismatch");
    TORCH_CHECK(bag_scale.numel() == grad_out.size(0),
                "reduce_bags_weighted_by_inverse: bag_scale must be [B]");
    TORCH_CHECK(u >= 0, "reduce_bags_weighted_by_inverse: bad u");
    const c10::cuda::CUDAGuard guard(grad_out.device());
    long n = inverse.numel();
    long B = grad_out.size(0);
    long dim = grad_out.size(1);
    auto ugrads = torch::empty({u, dim}, grad_out.options());
    auto counts = torch::empty({u}, grad_out.options().dtype(torch::kInt64));
    emb_reduce_bags_weighted_by_inverse(
        inverse.data_ptr<i64>(), grad_out.data_ptr<float>(), n, dim,
        bag_of.data_ptr<int>(), weights.data_ptr<float>(),
        bag_scale.data_ptr<float>(), B, ugrads.data_ptr<float>(),
        (u64*)counts.data_ptr<i64>(), u, cur_stream());
    return {ugrads, counts};
}

// dw [nnz]: gradient of pool_fwd_weighted w.r.t. its weights, reading
// the rows through the same (inverse, map) chain; 0 for elements with
// bag_of outside [0, B).
torch::Tensor pool_wgrad(torch::Tensor rows, OptTensor inverse, OptTensor map,
                         torch::Tensor weights, torch::Tensor bag_of,
                         torch::Tensor bag_scale, torch::Tensor out,
                         torch::Tensor grad_out, int64_t mode,
                         OptTensor dw_buf) {
    CHECK_GPU(rows); CHECK_CONT(rows);
    CHECK_GPU(weights); CHECK_CONT(weights);
    CHECK_GPU(bag_of); CHECK_CONT(bag_of);
    CHECK_GPU(bag_scale); CHECK_CONT(bag_scale);
    CHECK_GPU(out); CHECK_CONT(out);
    CHECK_GPU(grad_out); CHECK_CONT(grad_out);
    TORCH_CHECK(rows.dtype() == torch::kFloat32 && rows.dim() == 2,
                "pool_wgrad: rows must be float32 [R, dim]");
    TORCH_CHECK(out.dtype() == torch::kFloat32 && out.dim() == 2
                && out.size(1) == rows.size(1)
                && grad_out.dtype() == torch::kFloat32
                && grad_out.sizes() == out.sizes(),
                "pool_wgrad: out and grad_out must be float32 [B, dim]");
    TORCH_CHECK(mode >= 0 && mode <= 2, "pool_wgrad: bad mode");
    PoolChain c = pool_chain("pool_wgrad", rows, inverse, map);
    TORCH_CHECK(weights.dtype() == torch::kFloat32
                && weights.numel() == c.nnz,
                "pool_wgrad: weights must be float32 [nnz]");
    TORCH_CHECK(bag_of.dtype() == torch::kInt32 && bag_of.numel() == c.nnz,
                "pool_wgrad: bag_of must be int32 [nnz]");
    TORCH_CHECK(bag_scale.dtype() == torch::kFloat32
                && bag_scale.numel() == out.size(0),
                "pool_wgrad: bag_scale must be float32 [B]");
    const c10::cuda::CUDAGuard guard(rows.device());
    auto dw = dw_buf.has_value() ? *dw_buf
                                 : torch::empty({c.nnz}, rows.options());
    CHECK_GPU(dw); CHECK_CONT(dw);
    TORCH_CHECK(dw.dtype() == torch::kFloat32 && dw.dim() == 1
                && dw.numel() == c.nnz,
                "pool_wgrad: dw must be float32 [nnz]");
    emb_pool_wgrad(rows.data_ptr<float>(), rows.size(0), rows.size(1),
                   c.inv_ptr, c.nnz, c.map_ptr, c.map_kind, c.u,
                   weights.data_ptr<float>(), bag_of.data_ptr<int>(),
                   bag_scale.data_ptr<float>(), out.data_ptr<float>(),
                   grad_out.data_ptr<float>(), out.size(0), (int)mode,
                   dw.data_ptr<float>(), cur_stream());
    return dw;
}

// Read-only pooled lookup: table rows [R, dim] f32, values int64 [nnz_cap]
// keys, offsets int64 [B+1], optional weights f32 [nnz_cap] -> out [B, dim]
// in one launch, the table only read. Exactly one of (tk, tv) — the hash
// table, int64 / int32 [cap], cap a power of two — or (valid uint8 [cap],
// shard_num) — the array table — names the key -> row resolution.
torch::Tensor pool_lookup(torch::Tensor rows, torch::Tensor values,
                          torch::Tensor offsets, int64_t mode,
                          OptTensor weights, OptTensor tk, OptTensor tv,
                          OptTensor valid, int64_t shard_num) {
    CHECK_GPU(rows); CHECK_CONT(rows);
    CHECK_GPU(values); CHECK_CONT(values);
    CHECK_GPU(offsets); CHECK_CONT(offsets);
    TORCH_CHECK(rows.dtype() == torch::kFloat32 && rows.dim() == 2
                && rows.size(1) >= 1,
                "pool_lookup: rows must be float32 [R, dim >= 1]");
    TORCH_CHECK(values.dtype() == torch::kInt64 && values.dim() == 1,
                "pool_lookup: values must be int64 [nnz]");
    TORCH_CHECK(offsets.dtype() == torch::kInt64 && offsets.dim() == 1
                && offsets.numel() >= 1,
                "pool_lookup: offsets must be int64 [B+1]");
    TORCH_CHECK(mode >= 0 && mode <= 2, "pool_lookup: bad mode");
    TORCH_CHECK(values.device() == rows.device()
                && offsets.device() == rows.device(),
                "pool_lookup: values and offsets must be on the table's "
                "device");
    long nnz = values.numel();
    const float* w_ptr = nullptr;
    if (weights.has_value()) {
        CHECK_GPU(*weights); CHECK_CONT(*weights);
        TORCH_CHECK(weights->dtype() == torch::kFloat32
                    && weights->dim() == 1 && weights->numel() == nnz
                    && weights->device() == rows.device(),
                    "pool_lookup: weights must be float32 [nnz]");
        w_ptr = weights->data_ptr<float>();
    }
    const bool hash = tk.has_value() || tv.has_value();
    TORCH_CHECK(hash != valid.has_value(),
                "pool_lookup: pass either (tk, tv) or (valid, shard_num)");
    const u64* tk_ptr = nullptr;
    const int* tv_ptr = nullptr;
    const uint8_t* valid_ptr = nullptr;
    long cap = 0;
    if (hash) {
        TORCH_CHECK(tk.has_value() && tv.has_value(),
                    "pool_lookup: tk and tv go together");
        CHECK_GPU(*tk); CHECK_CONT(*tk);
        CHECK_GPU(*tv); CHECK_CONT(*tv);
        cap = tk->numel();
        TORCH_CHECK(tk->dtype() == torch::kInt64
                    && tv->dtype() == torch::kInt32 && tv->numel() == cap
                    && cap >= 1 && (cap & (cap - 1)) == 0
                    && tk->device() == rows.device()
                    && tv->device() == rows.device(),
                    "pool_lookup: tk int64 / tv int32 [cap], cap a power "
                    "of two");
        tk_ptr = (const u64*)tk->data_ptr<i64>();
        tv_ptr = tv->data_ptr<int>();
    } else {
        CHECK_GPU(*valid); CHECK_CONT(*valid);
        cap = valid->numel();
        TORCH_CHECK(valid->dtype() == torch::kUInt8
                    && valid->device() == rows.device(),
                    "pool_lookup: valid must be uint8 [cap]");
        TORCH_CHECK(shard_num >= 1, "pool_lookup: shard_num must be >= 1");
        valid_ptr = valid->data_ptr<uint8_t>();
    }
    const c10::cuda::CUDAGuard guard(rows.device());
    long B = offsets.numel() - 1;
    auto out = torch::empty({B, rows.size(1)}, rows.options());
    emb_pool_lookup(rows.data_ptr<float>(), rows.size(0), rows.size(1),
                    values.data_ptr<i64>(), nnz, offsets.data_ptr<i64>(), B,
                    (int)mode, w_ptr, tk_ptr, tv_ptr, cap, valid_ptr,
                    (long)shard_num, out.data_ptr<float>(), cur_stream());
    return out;
}

// ---- quantized serving tables -----------------------------------------
// slab: uint8 [R, stride] packed rows, stride == emb_quant_stride(fmt, dim),
// fmt 0 = int8 (codes + fp32 scale + fp32 lo), 1 = fp16; rows are read and
// written as dwords, so the slab starts on a 4-byte boundary.

void check_slab(const torch::Tensor& slab, int64_t dim, int64_t fmt,
                const char* who) {
    TORCH_CHECK(slab.is_cuda() && slab.is_contiguous()
                && slab.dtype() == torch::kUInt8 && slab.dim() == 2,
                who, ": slab must be a contiguous uint8 [R, stride] GPU "
                "tensor");
    TORCH_CHECK(fmt == 0 || fmt == 1, who, ": fmt must be 0 (int8) or 1 "
                "(fp16)");
    TORCH_CHECK(dim >= 1, who, ": dim must be >= 1");
    TORCH_CHECK(slab.size(1) == emb_quant_stride((int)fmt, (long)dim), who,
                ": slab stride ", slab.size(1), " is not the stride ",
                emb_quant_stride((int)fmt, (long)dim), " of this format and "
                "dim");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(slab.data_ptr()) % 4 == 0, who,
                ": slab must be 4-byte aligned");
}

// the key -> row table of a lookup: exactly one of (tk, tv) — hash, int64 /
// int32 [cap], cap a power of two — or (valid uint8 [cap], shard_num)
struct KeyTable {
    const u64* tk = nullptr;
    const int* tv = nullptr;
    const uint8_t* valid = nullptr;
    long cap = 0;
};

KeyTable check_key_table(const OptTensor& tk, const OptTensor& tv,
                         const OptTensor& valid, int64_t shard_num,
                         const torch::Device& dev, const char* who) {
    KeyTable t;
    const bool hash = tk.has_value() || tv.has_value();
    TORCH_CHECK(hash != valid.has_value(), who,
                ": pass either (tk, tv) or (valid, shard_num)");
    if (hash) {
        TORCH_CHECK(tk.has_value() && tv.has_value(), who,
                    ": tk and tv go together");
        CHECK_GPU(*tk); CHECK_CONT(*tk);
        CHECK_GPU(*tv); CHECK_CONT(*tv);
        t.cap = tk->numel();
        TORCH_CHECK(tk->dtype() == torch::kInt64
                    && tv->dtype() == torch::kInt32 && tv->numel() == t.cap
                    && t.cap >= 1 && (t.cap & (t.cap - 1)) == 0
                    && tk->device() == dev && tv->device() == dev, who,
                    ": tk int64 / tv int32 [cap], cap a power of two, on "
                    "the slab's device");
        t.tk = (const u64*)tk->data_ptr<i64>();
        t.tv = tv->data_ptr<int>();
    } else {
        CHECK_GPU(*valid); CHECK_CONT(*valid);
        t.cap = valid->numel();
        TORCH_CHECK(valid->dtype() == torch::kUInt8
                    && valid->device() == dev, who,
                    ": valid must be uint8 [cap] on the slab's device");
        TORCH_CHECK(shard_num >= 1, who, ": shard_num must be >= 1");
        t.valid = valid->data_ptr<uint8_t>();
    }
    return t;
}

// Quantize fp32 rows w [n, dim] into rows slots[i] of the slab, in place.
// A slot < 0 or >= R is skipped. Two source rows naming one slot in one
// call is the caller's error (the two groups race on the row); callers
// deduplicate first, as QuantizedShard.import_rows does (last one wins).
// Values are not validated here (non-finite rows, fp16 overflow): that is
// the host-side check of the import.
void quantize_rows(torch::Tensor w, torch::Tensor slots, torch::Tensor slab,
                   int64_t fmt) {
    CHECK_GPU(w); CHECK_CONT(w);
    CHECK_GPU(slots); CHECK_CONT(slots);
    TORCH_CHECK(w.dtype() == torch::kFloat32 && w.dim() == 2
                && w.size(1) >= 1,
                "quantize_rows: w must be float32 [n, dim >= 1]");
    check_slab(slab, w.size(1), fmt, "quantize_rows");
    TORCH_CHECK(slots.dtype() == torch::kInt64 && slots.dim() == 1
                && slots.numel() == w.size(0),
                "quantize_rows: slots must be int64 [n]");
    TORCH_CHECK(w.device() == slab.device()
                && slots.device() == slab.device(),
                "quantize_rows: w and slots must be on the slab's device");
    const c10::cuda::CUDAGuard guard(slab.device());
    emb_quantize_rows((int)fmt, w.data_ptr<float>(), w.size(0), w.size(1),
                      slots.data_ptr<i64>(), slab.data_ptr(), slab.size(0),
                      cur_stream());
}

// pool_lookup over a packed slab: values int64 [nnz_cap] keys, offsets
// int64 [B+1], optional weights f32 [nnz_cap] -> out f32 [B, dim] in one
// launch, the table only read.
torch::Tensor pool_lookup_q(torch::Tensor slab, int64_t dim, int64_t fmt,
                            torch::Tensor values, torch::Tensor offsets,
                            int64_t mode, OptTensor weights, OptTensor tk,
                            OptTensor tv, OptTensor valid,
                            int64_t shard_num) {
    check_slab(slab, dim, fmt, "pool_lookup_q");
    CHECK_GPU(values); CHECK_CONT(values);
    CHECK_GPU(offsets); CHECK_CONT(offsets);
    TORCH_CHECK(values.dtype() == torch::kInt64 && values.dim() == 1,
                "pool_lookup_q: values must be int64 [nnz]");
    TORCH_CHECK(offsets.dtype() == torch::kInt64 && offsets.dim() == 1
                && offsets.numel() >= 1,
                "pool_lookup_q: offsets must be int64 [B+1]");
    TORCH_CHECK(mode >= 0 && mode <= 2, "pool_lookup_q: bad mode");
    TORCH_CHECK(values.device() == slab.device()
                && offsets.device() == slab.device(),
                "pool_lookup_q: values and offsets must be on the table's "
                "device");
    long nnz = values.numel();
    const float* w_ptr = nullptr;
    if (weights.has_value()) {
        CHECK_GPU(*weights); CHECK_CONT(*weights);
        TORCH_CHECK(weights->dtype() == torch::kFloat32
                    && weights->dim() == 1 && weights->numel() == nnz
                    && weights->device() == slab.device(),
                    "pool_lookup_q: weights must be float32 [nnz]");
        w_ptr = weights->data_ptr<float>();
    }
    const KeyTable t = check_key_table(tk, tv, valid, shard_num,
                                       slab.device(), "pool_lookup_q");
    const c10::cuda::CUDAGuard guard(slab.device());
    long B = offsets.numel() - 1;
    auto out = torch::empty({B, dim},
                            slab.options().dtype(torch::kFloat32));
    emb_pool_lookup_q((int)fmt, slab.data_ptr(), slab.size(0), dim,
                      values.data_ptr<i64>(), nnz, offsets.data_ptr<i64>(),
                      B, (int)mode, w_ptr, t.tk, t.tv, t.cap, t.valid,
                      (long)shard_num, out.data_ptr<float>(), cur_stream());
    return out;
}

// flat read over a packed slab: keys int64 [n] -> f32 [n, dim] in one
// launch; zeros for key -1, an absent key or an out-of-range table entry
torch::Tensor gather_lookup_q(torch::Tensor slab, int64_t dim, int64_t fmt,
                              torch::Tensor keys, OptTensor tk, OptTensor tv,
                              OptTensor valid, int64_t shard_num) {
    check_slab(slab, dim, fmt, "gather_lookup_q");
    CHECK_GPU(keys); CHECK_CONT(keys);
    TORCH_CHECK(keys.dtype() == torch::kInt64 && keys.dim() == 1
                && keys.device() == slab.device(),
                "gather_lookup_q: keys must be int64 [n] on the table's "
                "device");
    const KeyTable t = check_key_table(tk, tv, valid, shard_num,
                                       slab.device(), "gather_lookup_q");
    const c10::cuda::CUDAGuard guard(slab.device());
    long n = keys.numel();
    auto out = torch::empty({n, dim},
                            slab.options().dtype(torch::kFloat32));
    emb_gather_lookup_q((int)fmt, slab.data_ptr(), slab.size(0), dim,
                        keys.data_ptr<i64>(), n, t.tk, t.tv, t.cap, t.valid,
                        (long)shard_num, out.data_ptr<float>(),
                        cur_stream());
    return out;
}

void mask_tail(torch::Tensor keys, torch::Tensor grads, torch::Tensor counts,
               OptTensor u_dev) {
    CHECK_GPU(keys); CHECK_CONT(keys); CHECK_CONT(grads); CHECK_CONT(counts);
    TORCH_CHECK(grads.size(0) == keys.numel()
                && counts.numel() == keys.numel(), "mask_tail sizes");
    const c10::cuda::CUDAGuard guard(keys.device());
    emb_mask_tail(keys.data_ptr<i64>(), grads.data_ptr<float>(),
                  (u64*)counts.data_ptr<i64>(), keys.numel(), grads.size(1),
                  u_ptr(u_dev), cur_stream());
}

// ---- delta checkpoints --------------------------------------------------

void mark_rows(torch::Tensor slots, OptTensor mask, OptTensor u_dev,
               torch::Tensor epoch_dev, torch::Tensor row_epoch) {
    CHECK_GPU(slots); CHECK_CONT(slots);
    CHECK_GPU(epoch_dev); CHECK_GPU(row_epoch); CHECK_CONT(row_epoch);
    TORCH_CHECK(slots.dtype() == torch::kInt64, "slots must be int64");
    TORCH_CHECK(epoch_dev.dtype() == torch::kInt32 && epoch_dev.numel() == 1,
                "epoch_dev must be int32[1]");
    TORCH_CHECK(row_epoch.dtype() == torch::kInt32,
                "row_epoch must be int32");
    const unsigned char* mp = nullptr;
    if (mask.has_value()) {
        CHECK_GPU(*mask); CHECK_CONT(*mask);
        TORCH_CHECK(mask->element_size() == 1
                    && mask->numel() == slots.numel(),
                    "mask must hold one byte per slot");
        mp = static_cast<const unsigned char*>(mask->data_ptr());
    }
    if (u_dev.has_value()) CHECK_GPU(*u_dev);
    const c10::cuda::CUDAGuard guard(slots.device());
    emb_mark_rows(slots.data_ptr<i64>(), slots.numel(), mp, u_ptr(u_dev),
                  epoch_dev.data_ptr<int>(), row_epoch.data_ptr<int>(),
                  row_epoch.numel(), cur_stream());
}

// rows with row_epoch >= since that are live, in ascending order:
// (slots int64 [R], tail -1; n_dev int32 [1]). Count per tile, scan the
// tile counts, compact; nothing is read on the host.
std::tuple<torch::Tensor, torch::Tensor> select_changed(
    torch::Tensor row_epoch, int64_t since, OptTensor nrows_dev,
    OptTensor valid) {
    CHECK_GPU(row_epoch); CHECK_CONT(row_epoch);
    TORCH_CHECK(row_epoch.dtype() == torch::kInt32,
                "row_epoch must be int32");
    TORCH_CHECK(nrows_dev.has_value() != valid.has_value(),
                "select_changed takes nrows_dev (hash) or valid (array)");
    TORCH_CHECK(since >= INT32_MIN && since <= INT32_MAX, "since range");
    long R = row_epoch.numel();
    const int* np = nullptr;
    const unsigned char* vp = nullptr;
    if (nrows_dev.has_value()) {
        CHECK_GPU(*nrows_dev);
        TORCH_CHECK(nrows_dev->dtype() == torch::kInt32
                    && nrows_dev->numel() == 1, "nrows_dev must be int32[1]");
        np = nrows_dev->data_ptr<int>();
    } else {
        CHECK_GPU(*valid); CHECK_CONT(*valid);
        TORCH_CHECK(valid->element_size() == 1 && valid->numel() == R,
                    "valid must hold one byte per row");
        vp = static_cast<const unsigned char*>(valid->data_ptr());
    }
    const c10::cuda::CUDAGuard guard(row_epoch.device());
    auto i32 = row_epoch.options();
    auto slots = torch::empty({R}, i32.dtype(torch::kInt64));
    if (R == 0) return {slots, torch::zeros({1}, i32)};
    long T = emb_delta_tiles(R);
    auto counts = torch::empty({T}, i32);
    emb_delta_count(row_epoch.data_ptr<int>(), R, (int)since, np, vp,
                    counts.data_ptr<int>(), cur_stream());
    auto incl = torch::cumsum(counts, 0, torch::kInt32);
    emb_delta_compact(row_epoch.data_ptr<int>(), R, (int)since, np, vp,
                      incl.data_ptr<int>(), slots.data_ptr<i64>(),
                      cur_stream());
    return {slots, incl.slice(0, T - 1, T)};
}

// rows of slots[start, start+count) -> (keys_out, w_out, s_out); positions
// at or past *n_dev and slots outside the slab write nothing. The outputs
// may be passed in, so that one staging block serves a whole export.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> gather_rows_by_slot(
    torch::Tensor weights, torch::Tensor state, OptTensor slot_keys,
    int64_t shard_num, int64_t shard_id, torch::Tensor slots, int64_t start,
    int64_t count, torch::Tensor n_dev, OptTensor keys_out, OptTensor w_out,
    OptTensor s_out) {
    CHECK_GPU(weights); CHECK_CONT(weights); CHECK_CONT(state);
    CHECK_GPU(slots); CHECK_CONT(slots); CHECK_GPU(n_dev);
    TORCH_CHECK(weights.dim() == 2 && weights.dtype() == torch::kFloat32,
                "weights must be float32 [R, dim]");
    TORCH_CHECK(slots.dtype() == torch::kInt64, "slots must be int64");
    TORCH_CHECK(n_dev.dtype() == torch::kInt32 && n_dev.numel() == 1,
                "n_dev must be int32[1]");
    TORCH_CHECK(start >= 0 && count >= 0, "start/count must be >= 0");
    long R = weights.size(0), dim = weights.size(1);
    long sd = (state.dim() == 2 && state.numel()) ? state.size(1) : 0;
    if (sd) {
        CHECK_GPU(state);
        TORCH_CHECK(state.dtype() == torch::kFloat32 && state.size(0) >= R,
                    "state must be float32 with a row per weights row");
    }
    const i64* sk = nullptr;
    if (slot_keys.has_value()) {
        CHECK_GPU(*slot_keys); CHECK_CONT(*slot_keys);
        TORCH_CHECK(slot_keys->dtype() == torch::kInt64
                    && slot_keys->numel() >= R,
                    "slot_keys must be int64 with a key per weights row");
        sk = slot_keys->data_ptr<i64>();
    }
    const c10::cuda::CUDAGuard guard(weights.device());
    auto ko = keys_out.has_value() ? *keys_out
        : torch::zeros({count}, slots.options());
    auto wo = w_out.has_value() ? *w_out
        : torch::zeros({count, dim}, weights.options());
    auto so = s_out.has_value() ? *s_out
        : torch::zeros({count, sd}, weights.options());
    CHECK_GPU(ko); CHECK_CONT(ko); CHECK_GPU(wo); CHECK_CONT(wo);
    CHECK_CONT(so);
    TORCH_CHECK(ko.dtype() == torch::kInt64 && ko.numel() >= count,
                "keys_out must be int64 [>= count]");
    TORCH_CHECK(wo.dtype() == torch::kFloat32 && wo.dim() == 2
                && wo.size(0) >= count && wo.size(1) == dim,
                "w_out must be float32 [>= count, dim]");
    if (sd) {
        CHECK_GPU(so);
        TORCH_CHECK(so.dtype() == torch::kFloat32 && so.dim() == 2
                    && so.size(0) >= count && so.size(1) == sd,
                    "s_out must be float32 [>= count, state_dim]");
    }
    emb_delta_gather(weights.data_ptr<float>(),
                     sd ? state.data_ptr<float>() : nullptr, R, dim, sd, sk,
                     shard_num, shard_id, slots.data_ptr<i64>(),
                     slots.numel(), start, count, n_dev.data_ptr<int>(),
                     ko.data_ptr<i64>(), wo.data_ptr<float>(),
                     sd ? so.data_ptr<float>() : nullptr, cur_stream());
    return {ko, wo, so};
}

// ---- row expiry -----------------------------------------------------------
// Removal of rows in place. The caller flags the dead rows (expire_flags by
// age, flag_slots by name); remove_flagged / remove_flagged_array do the rest
// and return the removed keys in ascending old-slot order.

static void check_dead(const torch::Tensor& dead) {
    CHECK_GPU(dead); CHECK_CONT(dead);
    TORCH_CHECK(dead.dtype() == torch::kUInt8 && dead.dim() == 1,
                "dead must be uint8 [R]");
}

static const int* nrows_ptr(const torch::Tensor& nrows_dev) {
    CHECK_GPU(nrows_dev);
    TORCH_CHECK(nrows_dev.dtype() == torch::kInt32 && nrows_dev.numel() == 1,
                "nrows_dev must be int32[1]");
    return nrows_dev.data_ptr<int>();
}

// dead uint8 [R]: the live rows with row_epoch < before
torch::Tensor expire_flags(torch::Tensor row_epoch, int64_t before,
                           OptTensor nrows_dev, OptTensor valid) {
    CHECK_GPU(row_epoch); CHECK_CONT(row_epoch);
    TORCH_CHECK(row_epoch.dtype() == torch::kInt32,
                "row_epoch must be int32");
    TORCH_CHECK(nrows_dev.has_value() != valid.has_value(),
                "expire_flags takes nrows_dev (hash) or valid (array)");
    TORCH_CHECK(before >= INT32_MIN && before <= INT32_MAX, "before range");
    long R = row_epoch.numel();
    const int* np = nullptr;
    const unsigned char* vp = nullptr;
    if (nrows_dev.has_value()) {
        np = nrows_ptr(*nrows_dev);
    } else {
        CHECK_GPU(*valid); CHECK_CONT(*valid);
        TORCH_CHECK(valid->element_size() == 1 && valid->numel() == R,
                    "valid must hold one byte per row");
        vp = static_cast<const unsigned char*>(valid->data_ptr());
    }
    const c10::cuda::CUDAGuard guard(row_epoch.device());
    auto dead = torch::empty({R}, row_epoch.options().dtype(torch::kUInt8));
    emb_expire_flag(row_epoch.data_ptr<int>(), R, (int)before, np, vp,
                    dead.data_ptr<uint8_t>(), cur_stream());
    return dead;
}

// dead uint8 [rows]: 1 at the named slots (misses and duplicates allowed)
torch::Tensor flag_slots(torch::Tensor slots, int64_t rows) {
    CHECK_GPU(slots); CHECK_CONT(slots);
    TORCH_CHECK(slots.dtype() == torch::kInt64, "slots must be int64");
    TORCH_CHECK(rows >= 0, "rows must be >= 0");
    const c10::cuda::CUDAGuard guard(slots.device());
    auto dead = torch::empty({rows}, slots.options().dtype(torch::kUInt8));
    emb_flag_slots(slots.data_ptr<i64>(), slots.numel(),
                   dead.data_ptr<uint8_t>(), rows, cur_stream());
    return dead;
}

// count + scan of one compaction: the inclusive tile sums [T]
static torch::Tensor expire_scan(int mode, const torch::Tensor& dead,
                                 const int* np, const unsigned char* vp,
                                 const int* cnt) {
    long R = dead.numel();
    auto i32 = dead.options().dtype(torch::kInt32);
    auto counts = torch::empty({emb_delta_tiles(R)}, i32);
    emb_expire_count(mode, dead.data_ptr<uint8_t>(), R, np, vp, cnt,
                     counts.data_ptr<int>(), cur_stream());
    return torch::cumsum(counts, 0, torch::kInt32);
}

// Hash table: remove the flagged live rows in place. planes are the
// per-row buffers ([rows, ...] contiguous, a whole number of 32-bit words
// per row; slot_keys must be one of them); every one keeps its storage.
// Returns (removed keys int64 [m], n'). The one host read is of {m, n'}.
std::tuple<torch::Tensor, int64_t> remove_flagged(
    torch::Tensor dead, std::vector<torch::Tensor> planes,
    torch::Tensor slot_keys, torch::Tensor tk, torch::Tensor tv,
    torch::Tensor nrows_dev) {
    check_dead(dead);
    long R = dead.numel();
    CHECK_GPU(slot_keys); CHECK_CONT(slot_keys);
    TORCH_CHECK(slot_keys.dtype() == torch::kInt64 && slot_keys.numel() >= R,
                "slot_keys must be int64 with a key per flagged row");
    CHECK_GPU(tk); CHECK_CONT(tk); CHECK_GPU(tv); CHECK_CONT(tv);
    long cap = tk.numel();
    TORCH_CHECK(tk.dtype() == torch::kInt64 && tv.dtype() == torch::kInt32
                && tv.numel() == cap && cap > 0 && (cap & (cap - 1)) == 0,
                "tk/tv must be an int64/int32 table of power-of-two size");
    const int* np = nrows_ptr(nrows_dev);
    std::vector<long> wpr;
    bool has_keys = false;
    for (const auto& p : planes) {
        CHECK_GPU(p); CHECK_CONT(p);
        TORCH_CHECK(p.dim() >= 1 && p.size(0) >= R,
                    "a plane must hold a row per flagged row");
        long row_bytes = p.size(0) ? (long)(p.numel() / p.size(0))
                                         * (long)p.element_size() : 0;
        TORCH_CHECK(row_bytes % 4 == 0,
                    "a plane's rows must be whole 32-bit words");
        wpr.push_back(row_bytes / 4);
        has_keys = has_keys || p.data_ptr() == slot_keys.data_ptr();
    }
    TORCH_CHECK(has_keys, "slot_keys must be among the planes");
    const c10::cuda::CUDAGuard guard(dead.device());
    auto i32 = dead.options().dtype(torch::kInt32);
    auto i64o = dead.options().dtype(torch::kInt64);
    if (R == 0) return {torch::empty({0}, i64o), 0};
    long T = emb_delta_tiles(R);
    const uint8_t* dp = dead.data_ptr<uint8_t>();
    auto cnt = torch::empty({2}, i32);
    auto incl_d = expire_scan(0, dead, np, nullptr, nullptr);
    emb_expire_counts(incl_d.data_ptr<int>(), T, np, R, cnt.data_ptr<int>(),
                      cur_stream());
    auto host = cnt.cpu();   // the one host read: {m, n'}
    long m = host.data_ptr<int>()[0], nprime = host.data_ptr<int>()[1];
    auto keys = torch::empty({m}, i64o);
    if (m == 0) return {keys, nprime};
    // the removed keys, before any row moves
    emb_expire_compact(0, dp, R, np, nullptr, nullptr,
                       incl_d.data_ptr<int>(), nullptr, keys.data_ptr<i64>(),
                       slot_keys.data_ptr<i64>(), 1, 0, m, cur_stream());
    long h = m < nprime ? m : nprime;   // bound of the hole count
    if (h > 0) {
        auto holes = torch::empty({h}, i32);
        auto movers = torch::empty({h}, i32);
        auto incl_h = expire_scan(1, dead, np, nullptr, cnt.data_ptr<int>());
        emb_expire_compact(1, dp, R, np, nullptr, cnt.data_ptr<int>(),
                           incl_h.data_ptr<int>(), holes.data_ptr<int>(),
                           nullptr, nullptr, 1, 0, h, cur_stream());
        auto incl_m = expire_scan(2, dead, np, nullptr, cnt.data_ptr<int>());
        emb_expire_compact(2, dp, R, np, nullptr, cnt.data_ptr<int>(),
                           incl_m.data_ptr<int>(), movers.data_ptr<int>(),
                           nullptr, nullptr, 1, 0, h, cur_stream());
        const int* moves = incl_h.data_ptr<int>() + (T - 1);
        for (size_t i = 0; i < planes.size(); ++i)
            emb_move_rows(planes[i].data_ptr(), R, wpr[i],
                          holes.data_ptr<int>(), movers.data_ptr<int>(), h,
                          moves, cur_stream());
    }
    emb_ht_build((u64*)tk.data_ptr<i64>(), tv.data_ptr<int>(), cap,
                 slot_keys.data_ptr<i64>(), R, cnt.data_ptr<int>(),
                 nrows_dev.data_ptr<int>(), nprime, cur_stream());
    return {keys, nprime};
}

// Array table: clear the valid byte of the flagged live rows; returns their
// keys (slot * shard_num + shard_id, ascending). One host read (the count).
torch::Tensor remove_flagged_array(torch::Tensor dead, torch::Tensor valid,
                                   int64_t shard_num, int64_t shard_id) {
    check_dead(dead);
    long R = dead.numel();
    CHECK_GPU(valid); CHECK_CONT(valid);
    TORCH_CHECK(valid.element_size() == 1 && valid.numel() == R,
                "valid must hold one byte per row");
    const c10::cuda::CUDAGuard guard(dead.device());
    auto i64o = dead.options().dtype(torch::kInt64);
    if (R == 0) return torch::empty({0}, i64o);
    long T = emb_delta_tiles(R);
    auto vp = static_cast<unsigned char*>(valid.data_ptr());
    auto incl = expire_scan(0, dead, nullptr, vp, nullptr);
    long m = incl.slice(0, T - 1, T).item<int>();   // the one host read
    auto keys = torch::empty({m}, i64o);
    if (m == 0) return keys;
    emb_expire_compact(0, dead.data_ptr<uint8_t>(), R, nullptr, vp, nullptr,
                       incl.data_ptr<int>(), nullptr, keys.data_ptr<i64>(),
                       nullptr, shard_num, shard_id, m, cur_stream());
    emb_expire_array(vp, dead.data_ptr<uint8_t>(), R, cur_stream());
    return keys;
}

// ---- capacity tier v2 --------------------------------------------------
// Pinned host tensors are device-accessible on ROCm (hipHostMalloc-backed
// via the torch pinned allocator): the fault-in/spill kernels read/write
// them directly — only touched rows cross the host link.

#define CHECK_PINNED(t) \
    TORCH_CHECK((t).is_pinned(), #t " must be a pinned host tensor")

// Shared argument checks of the three tier bindings. Every check runs before
// the launch: a mis-sized call would read or write pinned host memory out of
// bounds.

// int64 [n] on the GPU, contiguous
static void tier_check_i64(const torch::Tensor& t, long n, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.dtype() == torch::kInt64, name, " must be int64");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(n < 0 || t.numel() == n, name, " must hold one entry per key (",
                n, "), got ", t.numel());
}

// the device-side host map: tk int64 [cap], tv int32 [cap], cap = 2^k
static void tier_check_table(const torch::Tensor& htk,
                             const torch::Tensor& htv) {
    tier_check_i64(htk, -1, "htk");
    TORCH_CHECK(htv.is_cuda() && htv.dtype() == torch::kInt32
                && htv.is_contiguous(), "htv must be a contiguous int32 GPU "
                "tensor");
    long cap = htk.numel();
    TORCH_CHECK(cap > 0 && (cap & (cap - 1)) == 0,
                "host table size must be a power of two, got ", cap);
    TORCH_CHECK(htv.numel() == cap, "htv must be as long as htk (", cap,
                "), got ", htv.numel());
}

// float32 [rows, dim] slab on the GPU, contiguous
static void tier_check_slab(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.dtype() == torch::kFloat32 && t.dim() == 2, name,
                " must be float32 [rows, width]");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// pinned float32 [rows, width] host slab, contiguous
static void tier_check_host(const torch::Tensor& t, long width,
                            const char* name) {
    TORCH_CHECK(!t.is_cuda() && t.is_pinned(), name,
                " must be a pinned host tensor");
    TORCH_CHECK(t.dtype() == torch::kFloat32 && t.dim() == 2, name,
                " must be float32 [rows, width]");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(t.size(1) == width, name, " must be ", width,
                " wide like the cache slab, got ", t.size(1));
}

// state [R, sd] beside weights [R, dim] (an empty state means sd == 0) and
// the host state slab that goes with it; returns sd
static long tier_check_state(const torch::Tensor& weights,
                             const torch::Tensor& state,
                             const OptTensor& host_s) {
    long sd = state.numel() ? state.size(1) : 0;
    if (sd) {
        tier_check_slab(state, "state");
        TORCH_CHECK(state.size(0) >= weights.size(0),
                    "state must have a row per weights row");
        TORCH_CHECK(host_s.has_value(), "state tier needs host_s");
    }
    if (sd)
        tier_check_host(*host_s, sd, "host_s");
    else if (host_s.has_value())    // never dereferenced: only its width
        TORCH_CHECK(host_s->dim() == 2 && host_s->size(1) == 0,
                    "host_s must be 0 wide for a table without state");
    return sd;
}

void fault_in(torch::Tensor keys, OptTensor u_dev, torch::Tensor htk,
              torch::Tensor htv, torch::Tensor host_w, OptTensor host_s,
              torch::Tensor weights, torch::Tensor state, torch::Tensor slots,
              torch::Tensor new_mask, torch::Tensor faulted) {
    CHECK_GPU(keys); CHECK_CONT(keys); CHECK_CONT(host_w);
    CHECK_PINNED(host_w);
    long n = keys.numel();
    tier_check_i64(keys, n, "keys");
    if (u_dev.has_value())
        TORCH_CHECK(u_dev->is_cuda() && u_dev->dtype() == torch::kInt32
                    && u_dev->numel() == 1, "u_dev must be int32[1] on GPU");
    tier_check_table(htk, htv);
    tier_check_slab(weights, "weights");
    tier_check_host(host_w, weights.size(1), "host_w");
    long sd = tier_check_state(weights, state, host_s);
    tier_check_i64(slots, n, "slots");
    TORCH_CHECK(new_mask.is_cuda() && new_mask.dtype() == torch::kUInt8
                && new_mask.is_contiguous() && new_mask.numel() == n,
                "new_mask must be a contiguous uint8 GPU tensor with one "
                "entry per key (", n, ")");
    TORCH_CHECK(faulted.is_cuda() && faulted.dtype() == torch::kInt32
                && faulted.numel() == 1, "faulted must be int32[1] on GPU");
    const c10::cuda::CUDAGuard guard(keys.device());
    emb_fault_in(keys.data_ptr<i64>(), n, u_ptr(u_dev),
                 (const u64*)htk.data_ptr<i64>(), htv.data_ptr<int>(),
                 htk.numel(), host_w.data_ptr<float>(),
                 sd ? host_s->data_ptr<float>() : nullptr,
                 weights.data_ptr<float>(),
                 sd ? state.data_ptr<float>() : nullptr, weights.size(1), sd,
                 slots.data_ptr<i64>(), new_mask.data_ptr<uint8_t>(),
                 faulted.data_ptr<int>(), cur_stream());
}

void spill_rows(torch::Tensor cache_slots, torch::Tensor host_slots,
                torch::Tensor weights, torch::Tensor state,
                torch::Tensor host_w, OptTensor host_s) {
    CHECK_GPU(cache_slots); CHECK_CONT(cache_slots); CHECK_CONT(host_slots);
    CHECK_PINNED(host_w);
    long n = cache_slots.numel();
    tier_check_i64(cache_slots, n, "cache_slots");
    tier_check_i64(host_slots, n, "host_slots");
    tier_check_slab(weights, "weights");
    tier_check_host(host_w, weights.size(1), "host_w");
    long sd = tier_check_state(weights, state, host_s);
    const c10::cuda::CUDAGuard guard(cache_slots.device());
    emb_spill_rows(cache_slots.data_ptr<i64>(), host_slots.data_ptr<i64>(),
                   n, weights.data_ptr<float>(),
                   sd ? state.data_ptr<float>() : nullptr,
                   host_w.data_ptr<float>(),
                   sd ? host_s->data_ptr<float>() : nullptr, weights.size(1),
                   sd, cur_stream());
}

void gather_host(torch::Tensor keys, torch::Tensor cache_slots,
                 torch::Tensor htk, torch::Tensor htv, torch::Tensor host_w,
                 torch::Tensor out) {
    CHECK_GPU(keys); CHECK_CONT(keys); CHECK_CONT(out);
    CHECK_PINNED(host_w);
    long n = keys.numel();
    tier_check_i64(keys, n, "keys");
    tier_check_i64(cache_slots, n, "cache_slots");
    tier_check_table(htk, htv);
    tier_check_slab(out, "out");
    TORCH_CHECK(out.size(0) == n, "out must have one row per key (", n,
                "), got ", out.size(0));
    tier_check_host(host_w, out.size(1), "host_w");
    const c10::cuda::CUDAGuard guard(keys.device());
    emb_gather_host(keys.data_ptr<i64>(), n, cache_slots.data_ptr<i64>(),
                    (const u64*)htk.data_ptr<i64>(), htv.data_ptr<int>(),
                    htk.numel(), host_w.data_ptr<float>(),
                    out.data_ptr<float>(), out.size(1), cur_stream());
}

// ---- padded all-to-all -------------------------------------------------

void bucketize_pad(torch::Tensor uk_buf, OptTensor u_dev, int64_t world,
                   int64_t cap, torch::Tensor send_keys,
                   torch::Tensor send_src, torch::Tensor pos_of,
                   torch::Tensor counts, torch::Tensor overflow) {
    CHECK_GPU(uk_buf); CHECK_CONT(uk_buf); CHECK_CONT(send_keys);
    CHECK_CONT(send_src); CHECK_CONT(pos_of);
    TORCH_CHECK(send_keys.numel() == world * cap &&
                send_src.numel() == world * cap &&
                pos_of.numel() >= uk_buf.numel() &&
                counts.numel() == world && overflow.numel() == 1,
                "bucketize_pad buffer sizes");
    TORCH_CHECK(send_src.dtype() == torch::kInt32 &&
                pos_of.dtype() == torch::kInt32 &&
                counts.dtype() == torch::kInt32 &&
                overflow.dtype() == torch::kInt32, "int32 buffers expected");
    const c10::cuda::CUDAGuard guard(uk_buf.device());
    emb_bucketize_pad(uk_buf.data_ptr<i64>(), uk_buf.numel(), u_ptr(u_dev),
                      world, cap, send_keys.data_ptr<i64>(),
                      send_src.data_ptr<int>(), pos_of.data_ptr<int>(),
                      counts.data_ptr<int>(), overflow.data_ptr<int>(),
                      cur_stream());
}

torch::Tensor gather_pad(torch::Tensor ugrads, torch::Tensor counts,
                         torch::Tensor send_src) {
    CHECK_GPU(ugrads); CHECK_CONT(ugrads); CHECK_CONT(counts);
    CHECK_CONT(send_src);
    TORCH_CHECK(ugrads.dtype() == torch::kFloat32 &&
                counts.dtype() == torch::kInt64 &&
                send_src.dtype() == torch::kInt32, "gather_pad dtypes");
    const c10::cuda::CUDAGuard guard(ugrads.device());
    long total = send_src.numel();
    long dim = ugrads.size(1);
    auto send_p = torch::empty({total, dim + 1}, ugrads.options());
    emb_gather_pad(ugrads.data_ptr<float>(), (const u64*)counts.data_ptr<i64>(),
                   dim, send_src.data_ptr<int>(), total,
                   send_p.data_ptr<float>(), cur_stream());
    return send_p;
}

torch::Tensor scatter_out(torch::Tensor rows_recv, torch::Tensor inverse,
                          torch::Tensor pos_of, int64_t n_elems) {
    CHECK_GPU(rows_recv); CHECK_CONT(rows_recv); CHECK_CONT(inverse);
    CHECK_CONT(pos_of);
    TORCH_CHECK(rows_recv.dtype() == torch::kFloat32 &&
                pos_of.dtype() == torch::kInt32, "scatter_out dtypes");
    const c10::cuda::CUDAGuard guard(rows_recv.device());
    long dim = rows_recv.size(1);
    auto out = torch::empty({n_elems, dim}, rows_recv.options());
    emb_scatter_out(rows_recv.data_ptr<float>(), inverse.data_ptr<i64>(),
                    n_elems, pos_of.data_ptr<int>(), dim,
                    out.data_ptr<float>(), cur_stream());
    return out;
}

std::tuple<torch::Tensor, torch::Tensor> split_payload(torch::Tensor g2c,
                                                       OptTensor u_dev) {
    CHECK_GPU(g2c); CHECK_CONT(g2c);
    TORCH_CHECK(g2c.dtype() == torch::kFloat32, "split_payload dtype");
    const c10::cuda::CUDAGuard guard(g2c.device());
    long u = g2c.size(0);
    long dim = g2c.size(1) - 1;
    // tail rows beyond *u_dev stay uninitialized; every consumer
    // (apply_optimizer) is u_dev-guarded and never reads them
    auto grads = torch::empty({u, dim}, g2c.options());
    auto counts = torch::empty({u}, g2c.options().dtype(torch::kInt64));
    emb_split_payload(g2c.data_ptr<float>(), u, dim, u_ptr(u_dev),
                      grads.data_ptr<float>(), (u64*)counts.data_ptr<i64>(),
                      cur_stream());
    return {grads, counts};
}

// ---- fused optimizers --------------------------------------------------

void apply_optimizer(int64_t opt, torch::Tensor weights, torch::Tensor state,
                     torch::Tensor slots, torch::Tensor grads,
                     torch::Tensor counts, std::vector<double> cfg,
                     OptTensor u_dev) {
    CHECK_GPU(weights); CHECK_CONT(weights); CHECK_CONT(grads);
    const c10::cuda::CUDAGuard guard(weights.device());
    long n = slots.numel();
    long dim = weights.size(1);
    long sd = state.numel() ? state.size(1) : 0;
    float c[7] = {0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < cfg.size() && i < 7; ++i) c[i] = (float)cfg[i];
    emb_apply_optimizer((int)opt, weights.data_ptr<float>(),
                        sd ? state.data_ptr<float>() : nullptr, dim, sd,
                        slots.data_ptr<i64>(), n, grads.data_ptr<float>(),
                        (const u64*)counts.data_ptr<i64>(), c, u_ptr(u_dev),
                        cur_stream());
}

// ---- fused CTR interaction head ---------------------------------------

// impl (ctr_head_fwd / ctr_head_bwd): 0 = the launcher's choice, the
// row-staged kernels where their LDS images fit; 1 = the per-field forward
// and the bwd_e + bwd_d pair; 2 = row-staged or an error.
#define CHECK_F32(t) \
    TORCH_CHECK((t).scalar_type() == torch::kFloat32, #t " must be float32")

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> ctr_head_fwd(
    torch::Tensor e_all, torch::Tensor dense, torch::Tensor w,
    torch::Tensor bias, bool use_fm, bool out_bf16, bool pad32, int64_t impl) {
    CHECK_GPU(e_all); CHECK_CONT(e_all); CHECK_CONT(dense); CHECK_CONT(w);
    TORCH_CHECK(impl >= 0 && impl <= 2, "ctr_head: impl must be 0, 1 or 2");
    const c10::cuda::CUDAGuard guard(e_all.device());
    long B = e_all.size(0), F = e_all.size(1), D1 = e_all.size(2);
    long dim = D1 - 1, nd = dense.size(1);
    TORCH_CHECK(D1 <= 128, "ctr_head: dim+1 must be <= 128");
    TORCH_CHECK(nd <= 32, "ctr_head: dense features must be <= 32");
    auto out_opts = e_all.options().dtype(out_bf16 ? torch::kBFloat16
                                                   : torch::kFloat32);
    long width = F * dim + nd;
    long stride = pad32 ? ((width + 31) / 32) * 32 : width;
    int S = 0;
    if (impl != 1) {
        S = emb_ctr_head_rows_waves(B, F, dim, nd, stride, out_bf16 ? 1 : 0,
                                    0);
        TORCH_CHECK(S > 0 || impl == 0, "ctr_head_fwd: impl 2, but the "
                    "row-staged kernel does not fit this shape");
    }
    if (S > 0) {
        CHECK_F32(e_all); CHECK_F32(dense); CHECK_F32(w); CHECK_F32(bias);
        CHECK_GPU(dense); CHECK_GPU(w); CHECK_GPU(bias);
        TORCH_CHECK(dense.size(0) == B && w.numel() == nd
                    && bias.numel() >= 1, "ctr_head_fwd: operand lengths");
    }
    auto deep_in = torch::empty({B, stride}, out_opts);
    auto partial = torch::empty({B}, e_all.options());
    auto s_out = torch::empty({B, dim}, e_all.options());
    CHECK_CONT(bias);
    if (S > 0)
        emb_ctr_head_fwd_rows(e_all.data_ptr<float>(),
                              dense.data_ptr<float>(), w.data_ptr<float>(),
                              bias.data_ptr<float>(), B, F, dim, nd, stride,
                              deep_in.data_ptr(), partial.data_ptr<float>(),
                              s_out.data_ptr<float>(), use_fm ? 1 : 0,
                              out_bf16 ? 1 : 0, S, cur_stream());
    else
        emb_ctr_head_fwd(e_all.data_ptr<float>(), dense.data_ptr<float>(),
                         w.data_ptr<float>(), bias.data_ptr<float>(), B, F,
                         dim, nd, stride, deep_in.data_ptr(),
                         partial.data_ptr<float>(), s_out.data_ptr<float>(),
                         use_fm ? 1 : 0, out_bf16 ? 1 : 0, cur_stream());
    return {deep_in, partial, s_out};
}

// shapes and dtypes the merged backward relies on; returns out_bf16
static bool head_bwd_check(const torch::Tensor& e_all,
                           const torch::Tensor& dense,
                           const torch::Tensor& w,
                           const torch::Tensor& d_deep_in,
                           const torch::Tensor& d_partial,
                           const torch::Tensor& s_in) {
    CHECK_GPU(e_all); CHECK_GPU(dense); CHECK_GPU(w); CHECK_GPU(d_deep_in);
    CHECK_GPU(d_partial); CHECK_GPU(s_in);
    CHECK_CONT(e_all); CHECK_CONT(dense); CHECK_CONT(w);
    CHECK_CONT(d_deep_in); CHECK_CONT(d_partial); CHECK_CONT(s_in);
    CHECK_F32(e_all); CHECK_F32(dense); CHECK_F32(w); CHECK_F32(d_partial);
    CHECK_F32(s_in);
    TORCH_CHECK(e_all.dim() == 3 && dense.dim() == 2 && d_deep_in.dim() == 2,
                "ctr_head_bwd: e_all [B,F,D1], dense [B,nd], d_deep_in "
                "[B,stride]");
    long B = e_all.size(0), F = e_all.size(1), dim = e_all.size(2) - 1;
    long nd = dense.size(1);
    bool bf = d_deep_in.scalar_type() == torch::kBFloat16;
    TORCH_CHECK(bf || d_deep_in.scalar_type() == torch::kFloat32,
                "ctr_head_bwd: d_deep_in must be bfloat16 or float32");
    TORCH_CHECK(dense.size(0) == B && w.numel() == nd
                && d_deep_in.size(0) == B
                && d_deep_in.size(1) >= F * dim + nd
                && d_partial.numel() == B && s_in.numel() == B * dim,
                "ctr_head_bwd: operand lengths");
    return bf;
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
ctr_head_bwd(torch::Tensor e_all, torch::Tensor dense, torch::Tensor w,
             torch::Tensor d_deep_in, torch::Tensor d_partial,
             torch::Tensor s_in, bool use_fm, int64_t impl) {
    CHECK_GPU(e_all); CHECK_CONT(e_all); CHECK_CONT(d_deep_in);
    TORCH_CHECK(impl >= 0 && impl <= 2, "ctr_head: impl must be 0, 1 or 2");
    const c10::cuda::CUDAGuard guard(e_all.device());
    long B = e_all.size(0), F = e_all.size(1), D1 = e_all.size(2);
    long dim = D1 - 1, nd = dense.size(1);
    long stride = d_deep_in.size(1);  // may be 32-padded
    bool out_bf16 = d_deep_in.dtype() == torch::kBFloat16;
    int S = 0;
    if (impl != 1) {
        S = emb_ctr_head_rows_waves(B, F, dim, nd, stride, out_bf16 ? 1 : 0,
                                    impl == 0 ? 2 : 1);
        TORCH_CHECK(S > 0 || impl == 0, "ctr_head_bwd: impl 2, but the "
                    "row-staged kernel does not fit this shape");
    }
    auto de_all = torch::empty_like(e_all);
    auto d_dense = torch::empty_like(dense);
    if (S > 0) {
        head_bwd_check(e_all, dense, w, d_deep_in, d_partial, s_in);
        // the merged kernel accumulates: one zero fill for both
        auto acc = torch::zeros({nd + 1}, w.options());
        auto dw = acc.narrow(0, 0, nd).view_as(w);
        auto db = acc.narrow(0, nd, 1);
        emb_ctr_head_bwd_rows(e_all.data_ptr<float>(),
                              dense.data_ptr<float>(), w.data_ptr<float>(),
                              d_deep_in.data_ptr(),
                              d_partial.data_ptr<float>(),
                              s_in.data_ptr<float>(), B, F, dim, nd, stride,
                              de_all.data_ptr<float>(),
                              d_dense.data_ptr<float>(),
                              dw.data_ptr<float>(), db.data_ptr<float>(),
                              use_fm ? 1 : 0, out_bf16 ? 1 : 0, S,
                              cur_stream());
        return {de_all, d_dense, dw, db};
    }
    // dw/db are zeroed by k_ctr_head_bwd_e before bwd_d accumulates
    auto dw = torch::empty_like(w);
    auto db = torch::empty({1}, w.options());
    if (B == 0) { dw.zero_(); db.zero_(); }
    emb_ctr_head_bwd(e_all.data_ptr<float>(), dense.data_ptr<float>(),
                     w.data_ptr<float>(), d_deep_in.data_ptr(),
                     d_partial.data_ptr<float>(),
                     s_in.data_ptr<float>(), B, F, dim, nd, stride,
                     de_all.data_ptr<float>(), d_dense.data_ptr<float>(),
                     dw.data_ptr<float>(), db.data_ptr<float>(),
                     use_fm ? 1 : 0, out_bf16 ? 1 : 0, cur_stream());
    return {de_all, d_dense, dw, db};
}

// Backward that adds dw/db into the caller's buffers (the flat optimizer's
// bound .grad views): no temporaries, no AccumulateGrad launches. A shape
// the launcher does not give to the merged kernel (impl 0 of ctr_head_bwd)
// runs the two-launch pair and adds.
std::tuple<torch::Tensor, c10::optional<torch::Tensor>>
ctr_head_bwd_acc(torch::Tensor e_all, torch::Tensor dense, torch::Tensor w,
                 torch::Tensor d_deep_in, torch::Tensor d_partial,
                 torch::Tensor s_in, bool use_fm, torch::Tensor dw_acc,
                 torch::Tensor db_acc, bool want_d_dense) {
    bool out_bf16 = head_bwd_check(e_all, dense, w, d_deep_in, d_partial,
                                   s_in);
    long B = e_all.size(0), F = e_all.size(1), dim = e_all.size(2) - 1;
    long nd = dense.size(1), stride = d_deep_in.size(1);
    CHECK_GPU(dw_acc); CHECK_GPU(db_acc); CHECK_CONT(dw_acc);
    CHECK_CONT(db_acc); CHECK_F32(dw_acc); CHECK_F32(db_acc);
    TORCH_CHECK(dw_acc.dim() == 1 && dw_acc.numel() == nd,
                "ctr_head_bwd_acc: dw_acc must be [nd]");
    TORCH_CHECK(db_acc.dim() == 1 && db_acc.numel() == 1,
                "ctr_head_bwd_acc: db_acc must be [1]");
    TORCH_CHECK(dw_acc.device() == e_all.device()
                && db_acc.device() == e_all.device(),
                "ctr_head_bwd_acc: accumulators on another device");
    const c10::cuda::CUDAGuard guard(e_all.device());
    int S = emb_ctr_head_rows_waves(B, F, dim, nd, stride, out_bf16 ? 1 : 0,
                                    2);
    if (S == 0) {
        auto r = ctr_head_bwd(e_all, dense, w, d_deep_in, d_partial, s_in,
                              use_fm, 1);
        dw_acc.add_(std::get<2>(r).reshape(-1));
        db_acc.add_(std::get<3>(r));
        if (want_d_dense) return {std::get<0>(r), std::get<1>(r)};
        return {std::get<0>(r), c10::nullopt};
    }
    auto de_all = torch::empty_like(e_all);
    c10::optional<torch::Tensor> d_dense;
    if (want_d_dense) d_dense = torch::empty_like(dense);
    emb_ctr_head_bwd_rows(e_all.data_ptr<float>(), dense.data_ptr<float>(),
                          w.data_ptr<float>(), d_deep_in.data_ptr(),
                          d_partial.data_ptr<float>(),
                          s_in.data_ptr<float>(), B, F, dim, nd, stride,
                          de_all.data_ptr<float>(),
                          want_d_dense ? d_dense->data_ptr<float>() : nullptr,
                          dw_acc.data_ptr<float>(),
                          db_acc.data_ptr<float>(), use_fm ? 1 : 0,
                          out_bf16 ? 1 : 0, S, cur_stream());
    return {de_all, d_dense};
}

// (S forward, S backward, blocks of the merged backward, launcher's choice
// for the backward); S = samples per block, 0 where the shape cannot take
// the row-staged kernel
std::tuple<int64_t, int64_t, int64_t, bool> ctr_head_rows_plan(
    int64_t B, int64_t F, int64_t dim, int64_t nd, int64_t stride,
    bool out_bf16) {
    int sf = emb_ctr_head_rows_waves(B, F, dim, nd, stride, out_bf16, 0);
    int sb = emb_ctr_head_rows_waves(B, F, dim, nd, stride, out_bf16, 1);
    int sa = emb_ctr_head_rows_waves(B, F, dim, nd, stride, out_bf16, 2);
    return {sf, sb, sb ? emb_ctr_head_rows_bwd_grid(B, nd, sb) : 0, sa > 0};
}

// ---- flat dense Adagrad -----------------------------------------------

void flat_adagrad(torch::Tensor param, torch::Tensor accum,
                  torch::Tensor grad, c10::optional<torch::Tensor> master,
                  double lr, double eps) {
    CHECK_GPU(param); CHECK_CONT(param); CHECK_CONT(accum); CHECK_CONT(grad);
    const c10::cuda::CUDAGuard guard(param.device());
    long n = param.numel();
    if (param.dtype() == torch::kFloat32) {
        emb_flat_adagrad_f32(param.data_ptr<float>(), accum.data_ptr<float>(),
                             grad.data_ptr<float>(), n, (float)lr, (float)eps,
                             cur_stream());
    } else {
        TORCH_CHECK(param.dtype() == torch::kBFloat16 && master.has_value(),
                    "bf16 flat_adagrad needs a float32 master tensor");
        emb_flat_adagrad_bf16(master->data_ptr<float>(),
                              accum.data_ptr<float>(), grad.data_ptr(),
                              param.data_ptr(), n, (float)lr, (float)eps,
                              cur_stream());
    }
}

void flat_step_scalars(torch::Tensor sc, double b1, double b2) {
    CHECK_GPU(sc); CHECK_CONT(sc);
    TORCH_CHECK(sc.numel() >= 3 && sc.dtype() == torch::kFloat32,
                "step scalars must be float32 [3]");
    const c10::cuda::CUDAGuard guard(sc.device());
    emb_flat_step_scalars(sc.data_ptr<float>(), (float)b1, (float)b2,
                          cur_stream());
}

void flat_opt(int64_t opt, torch::Tensor param, OptTensor master,
              OptTensor s1, OptTensor s2, torch::Tensor grad, OptTensor sc,
              double lr, double c0, double c1, double c2) {
    CHECK_GPU(param); CHECK_CONT(param); CHECK_CONT(grad);
    const c10::cuda::CUDAGuard guard(param.device());
    long n = param.numel();
    bool bf16 = param.dtype() == torch::kBFloat16;
    float* mp = nullptr;
    if (bf16) {
        TORCH_CHECK(master.has_value(), "bf16 flat_opt needs fp32 master");
        mp = master->data_ptr<float>();
    } else {
        TORCH_CHECK(param.dtype() == torch::kFloat32, "flat_opt dtype");
    }
    emb_flat_opt((int)opt, param.data_ptr(), mp,
                 s1.has_value() ? s1->data_ptr<float>() : nullptr,
                 s2.has_value() ? s2->data_ptr<float>() : nullptr,
                 grad.data_ptr(),
                 sc.has_value() ? sc->data_ptr<float>() : nullptr,
                 n, bf16 ? 1 : 0, (float)lr, (float)c0, (float)c1,
                 (float)c2, cur_stream());
}

// ---- fused MLP bias grads ---------------------------------------------

void mlp3_bias_bwd(torch::Tensor dout, torch::Tensor dz1, torch::Tensor dz2,
                   torch::Tensor dz3, torch::Tensor a3, torch::Tensor scratch,
                   torch::Tensor db1, torch::Tensor db2, torch::Tensor db3,
                   torch::Tensor dw4, torch::Tensor db4, bool with_dz,
                   bool with_head) {
    CHECK_GPU(dout); CHECK_CONT(dout); CHECK_CONT(dz1); CHECK_CONT(dz2);
    CHECK_CONT(dz3); CHECK_CONT(a3); CHECK_CONT(scratch);
    long M = dz1.size(0), H = dz1.size(1);
    TORCH_CHECK(dout.numel() == M && scratch.numel() >= 4 * H + 1 &&
                a3.sizes() == dz1.sizes(), "mlp3_bias_bwd shape mismatch");
    TORCH_CHECK(db1.dtype() == torch::kBFloat16 &&
                scratch.dtype() == torch::kFloat32,
                "mlp3_bias_bwd wants bf16 grads + fp32 scratch");
    TORCH_CHECK(db1.is_contiguous() && db2.is_contiguous() &&
                db3.is_contiguous() && dw4.is_contiguous() &&
                db4.is_contiguous() &&
                db1.numel() == H && db2.numel() == H && db3.numel() == H &&
                dw4.numel() == H && db4.numel() == 1, "bias grad layout");
    const c10::cuda::CUDAGuard guard(dout.device());
    emb_mlp3_bias_bwd(dout.data_ptr<float>(), dz1.data_ptr(), dz2.data_ptr(),
                      dz3.data_ptr(), a3.data_ptr(), M, H,
                      scratch.data_ptr<float>(),
                      db1.data_ptr(), db2.data_ptr(), db3.data_ptr(),
                      dw4.data_ptr(), db4.data_ptr(), with_dz ? 1 : 0,
                      with_head ? 1 : 0, cur_stream());
}

// ---- CIN implicit-GEMM -------------------------------------------------

torch::Tensor cin_fwd(torch::Tensor x0p, torch::Tensor xkp,
                      torch::Tensor wp) {
    CHECK_GPU(x0p); CHECK_CONT(x0p); CHECK_CONT(xkp); CHECK_CONT(wp);
    TORCH_CHECK(x0p.dtype() == torch::kFloat32
                && xkp.dtype() == torch::kFloat32
                && wp.dtype() == torch::kBFloat16, "cin_fwd dtypes");
    const c10::cuda::CUDAGuard guard(x0p.device());
    long N = x0p.size(0), F = x0p.size(1), H = xkp.size(1);
    long O = wp.size(0), Kp = wp.size(1);
    TORCH_CHECK(F <= 32 && H <= 128 && O >= 16 && O <= 128 && O % 16 == 0
                && Kp % 32 == 0 && Kp >= F * H && xkp.size(0) == N,
                "cin_fwd shapes");
    auto out = torch::empty({N, O}, x0p.options());
    emb_cin_fwd(x0p.data_ptr<float>(), xkp.data_ptr<float>(), wp.data_ptr(),
                out.data_ptr<float>(), N, F, H, O, Kp, cur_stream());
    return out;
}

torch::Tensor cin_dw(torch::Tensor dzt, torch::Tensor x0t,
                     torch::Tensor xkt, int64_t O, int64_t n_split) {
    CHECK_GPU(dzt); CHECK_CONT(dzt); CHECK_CONT(x0t); CHECK_CONT(xkt);
    TORCH_CHECK(dzt.dtype() == torch::kBFloat16
                && x0t.dtype() == torch::kBFloat16
                && xkt.dtype() == torch::kBFloat16, "cin_dw dtypes");
    const c10::cuda::CUDAGuard guard(dzt.device());
    long Np = dzt.size(1), F = x0t.size(0), H = xkt.size(0);
    // each wave reads a full 16-row dZt fragment: an O that is no multiple
    // of 16, or a dzt with fewer rows than O, would read past its end
    TORCH_CHECK(Np % 32 == 0 && x0t.size(1) == Np && xkt.size(1) == Np
                && F <= 32 && H <= 128 && O <= 128 && O % 16 == 0
                && dzt.size(0) == O && n_split >= 1, "cin_dw shapes");
    auto dw = torch::zeros({O, F * H},
                           dzt.options().dtype(torch::kFloat32));
    emb_cin_dw(dzt.data_ptr(), x0t.data_ptr(), xkt.data_ptr(),
               dw.data_ptr<float>(), Np, F, H, O, n_split, cur_stream());
    return dw;
}

std::tuple<torch::Tensor, torch::Tensor> cin_dx(
        torch::Tensor doutp, torch::Tensor wt, torch::Tensor x0p,
        torch::Tensor xkp) {
    CHECK_GPU(doutp); CHECK_CONT(doutp); CHECK_CONT(wt); CHECK_CONT(x0p);
    CHECK_CONT(xkp);
    TORCH_CHECK(doutp.dtype() == torch::kFloat32
                && wt.dtype() == torch::kBFloat16
                && x0p.dtype() == torch::kFloat32
                && xkp.dtype() == torch::kFloat32, "cin_dx dtypes");
    const c10::cuda::CUDAGuard guard(doutp.device());
    long N = doutp.size(0), O = doutp.size(1);
    long F = x0p.size(1), H = xkp.size(1), Op = wt.size(1);
    // k_cin_dx loads a whole 16-row Wt fragment per h-tile, so the last
    // field's partial tile reads rows up to (F-1)*H + ceil16(H) - 1; wt
    // carries zero rows up to there (padded, not bounds-checked: a check
    // in the fragment loader scalarizes the k-loop, docs/hacking.md).
    // The LDS dZ tile is 128 wide, hence Op <= 128.
    long rows = F * H > (F - 1) * H + (H + 15) / 16 * 16
                    ? F * H : (F - 1) * H + (H + 15) / 16 * 16;
    rows = (rows + 31) / 32 * 32;
    TORCH_CHECK(Op % 32 == 0 && Op <= 128 && O >= 1 && O <= Op
                && F >= 1 && F <= 32 && H <= 128
                && x0p.size(0) == N && xkp.size(0) == N
                && wt.size(0) == rows, "cin_dx shapes");
    auto dx0 = torch::empty({N, F}, x0p.options());
    auto dxk = torch::empty({N, H}, xkp.options());
    emb_cin_dx(doutp.data_ptr<float>(), wt.data_ptr(),
               x0p.data_ptr<float>(), xkp.data_ptr<float>(),
               dx0.data_ptr<float>(), dxk.data_ptr<float>(), N, F, H, O,
               Op, cur_stream());
    return {dx0, dxk};
}

void mlp3_wgrad(torch::Tensor dz1, torch::Tensor dz2, torch::Tensor dz3,
                torch::Tensor x0, torch::Tensor a1, torch::Tensor a2,
                torch::Tensor scratch, torch::Tensor dw1, torch::Tensor dw2,
                torch::Tensor dw3, OptTensor bias_scratch, long m_split) {
    // bias_scratch ([4H+1] fp32, the bias pass scratch): when given, the
    // kernel also accumulates the three dz column sums (bias grads) from
    // its LDS-staged tiles into segments 0/H/2H
    CHECK_GPU(dz1); CHECK_CONT(dz1); CHECK_CONT(dz2); CHECK_CONT(dz3);
    CHECK_CONT(x0); CHECK_CONT(a1); CHECK_CONT(a2); CHECK_CONT(scratch);
    TORCH_CHECK(dz1.dtype() == torch::kBFloat16
                && dw1.dtype() == torch::kBFloat16
                && scratch.dtype() == torch::kFloat32, "mlp3_wgrad dtypes");
    long M = dz1.size(0), H = dz1.size(1), K0p = x0.size(1);
    long K0 = dw1.size(1);
    TORCH_CHECK(M % 32 == 0, "mlp3_wgrad: M must be x32");
    // 16-byte row pieces: every operand row must start 16-byte aligned
    TORCH_CHECK(H % 8 == 0 && K0p % 8 == 0 && a1.size(1) == H
                && a2.size(1) == H, "mlp3_wgrad: H, K0p must be x8");
    for (const torch::Tensor* t : {&dz1, &dz2, &dz3, &x0, &a1, &a2})
        TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                    "mlp3_wgrad: operands must be 16-byte aligned");
    TORCH_CHECK(m_split >= 0 && m_split <= 64, "mlp3_wgrad: m_split");
    TORCH_CHECK(scratch.numel() >= H * K0p + 2 * H * H
                && dw1.size(0) == H && K0 <= K0p && dw2.numel() == H * H
                && dw3.numel() == H * H
                && dw1.is_contiguous() && dw2.is_contiguous()
                && dw3.is_contiguous(), "mlp3_wgrad shapes");
    const c10::cuda::CUDAGuard guard(dz1.device());
    float* bptr = nullptr;
    if (bias_scratch.has_value()) {
        CHECK_CONT(*bias_scratch);
        TORCH_CHECK(bias_scratch->numel() >= 3 * H
                    && bias_scratch->dtype() == torch::kFloat32,
                    "bias_scratch layout");
        bptr = bias_scratch->data_ptr<float>();
    }
    emb_mlp3_wgrad(dz1.data_ptr(), dz2.data_ptr(), dz3.data_ptr(),
                   x0.data_ptr(), a1.data_ptr(), a2.data_ptr(), M, H, K0p,
                   K0, scratch.data_ptr<float>(), dw1.data_ptr(),
                   dw2.data_ptr(), dw3.data_ptr(), bptr, m_split,
                   cur_stream());
}

void mlp3_pack(torch::Tensor s1, torch::Tensor d1, bool t1,
               torch::Tensor s2, torch::Tensor d2, bool t2,
               torch::Tensor s3, torch::Tensor d3, bool t3) {
    // one launch refreshing three padded weight copies (plain or
    // transposed); src is the [rows, cols] weight, dst the padded buffer
    torch::Tensor ss[3] = {s1, s2, s3}, dd[3] = {d1, d2, d3};
    long a[3][6];
    int tt[3] = {t1, t2, t3};
    for (int i = 0; i < 3; i++) {
        CHECK_GPU(ss[i]); CHECK_CONT(ss[i]);
        TORCH_CHECK(ss[i].dtype() == torch::kBFloat16
                    && dd[i].dtype() == torch::kBFloat16
                    && ss[i].dim() == 2 && dd[i].dim() == 2
                    && dd[i].stride(1) == 1, "mlp3_pack dtypes/shapes");
        long r = ss[i].size(0), c = ss[i].size(1);
        long dr = tt[i] ? c : r, dc = tt[i] ? r : c;
        TORCH_CHECK(dd[i].size(0) >= dr && dd[i].size(1) >= dc,
                    "mlp3_pack: dst too small");
        a[i][0] = r; a[i][1] = c;
        a[i][2] = ss[i].stride(0); a[i][3] = dd[i].stride(0);
    }
    const c10::cuda::CUDAGuard guard(s1.device());
    emb_mlp3_pack(s1.data_ptr(), d1.data_ptr(), a[0][0], a[0][1], a[0][2],
                  a[0][3], tt[0],
                  s2.data_ptr(), d2.data_ptr(), a[1][0], a[1][1], a[1][2],
                  a[1][3], tt[1],
                  s3.data_ptr(), d3.data_ptr(), a[2][0], a[2][1], a[2][2],
                  a[2][3], tt[2], cur_stream());
}

void mlp3_pack_frag(std::vector<torch::Tensor> srcs,
                    std::vector<torch::Tensor> dsts,
                    std::vector<bool> trans) {
    // one launch writing up to six fragment-major weight images (mlp.hip).
    // dst [N, Kp] gives the image's dimensions and is written in full;
    // src is the [rows, cols] weight, or its transpose when trans[i]
    const size_t n = srcs.size();
    TORCH_CHECK(n >= 1 && n <= 6 && dsts.size() == n && trans.size() == n,
                "mlp3_pack_frag: 1..6 matrices, lists of equal length");
    const void* sp[6];
    void* dp[6];
    long rows[6], cols[6], sld[6], N[6], Kp[6];
    int tt[6];
    for (size_t i = 0; i < n; i++) {
        const torch::Tensor &s = srcs[i], &d = dsts[i];
        CHECK_GPU(s); CHECK_GPU(d); CHECK_CONT(d);
        TORCH_CHECK(s.dtype() == torch::kBFloat16
                    && d.dtype() == torch::kBFloat16
                    && s.dim() == 2 && d.dim() == 2 && s.stride(1) == 1
                    && s.stride(0) >= s.size(1)
                    && s.device() == d.device(),
                    "mlp3_pack_frag dtypes/shapes");
        rows[i] = s.size(0); cols[i] = s.size(1); sld[i] = s.stride(0);
        N[i] = d.size(0); Kp[i] = d.size(1);
        tt[i] = trans[i];
        TORCH_CHECK(N[i] > 0 && N[i] % 16 == 0 && Kp[i] > 0
                    && Kp[i] % 32 == 0,
                    "mlp3_pack_frag: dst must be [x16, x32]");
        TORCH_CHECK((tt[i] ? cols[i] : rows[i]) <= N[i]
                    && (tt[i] ? rows[i] : cols[i]) <= Kp[i],
                    "mlp3_pack_frag: dst too small");
        TORCH_CHECK(N[i] * Kp[i] < (1L << 31)
                    && rows[i] * sld[i] < (1L << 31),
                    "mlp3_pack_frag: 32-bit indices");
        TORCH_CHECK((reinterpret_cast<uintptr_t>(d.data_ptr()) & 15) == 0,
                    "mlp3_pack_frag: dst must be 16-byte aligned");
        sp[i] = s.data_ptr(); dp[i] = d.data_ptr();
    }
    const c10::cuda::CUDAGuard guard(srcs[0].device());
    emb_mlp3_pack_frag((int)n, sp, dp, rows, cols, sld, N, Kp, tt,
                       cur_stream());
}

// ---- fused BCE-with-logits --------------------------------------------

torch::Tensor bce_fwd(torch::Tensor logits, torch::Tensor labels) {
    CHECK_GPU(logits); CHECK_CONT(logits); CHECK_CONT(labels);
    TORCH_CHECK(logits.dtype() == torch::kFloat32 &&
                labels.dtype() == torch::kFloat32, "bce_fwd wants fp32");
    TORCH_CHECK(logits.numel() == labels.numel(), "logits/labels mismatch");
    const c10::cuda::CUDAGuard guard(logits.device());
    auto loss = torch::empty({}, logits.options());
    emb_bce_fwd(logits.data_ptr<float>(), labels.data_ptr<float>(),
                logits.numel(), loss.data_ptr<float>(), cur_stream());
    return loss;
}

torch::Tensor bce_bwd(torch::Tensor logits, torch::Tensor labels,
                      torch::Tensor grad_out) {
    CHECK_GPU(logits); CHECK_CONT(logits); CHECK_CONT(labels);
    TORCH_CHECK(grad_out.numel() == 1, "grad_out must be scalar");
    const c10::cuda::CUDAGuard guard(logits.device());
    auto g = torch::empty_like(logits);
    emb_bce_bwd(logits.data_ptr<float>(), labels.data_ptr<float>(),
                logits.numel(), grad_out.contiguous().data_ptr<float>(),
                g.data_ptr<float>(), cur_stream());
    return g;
}

// ---- fused 3-layer MLP forward ----------------------------------------

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
mlp3_fwd(torch::Tensor x0, torch::Tensor w1, torch::Tensor b1,
         torch::Tensor w2, torch::Tensor b2, torch::Tensor w3,
         torch::Tensor b3, torch::Tensor w4, torch::Tensor b4,
         c10::optional<torch::Tensor> partial, long bm, bool frag) {
    // bm: rows per block, 0 = the launcher's choice; 16/32/64 force one
    // kernel variant (tests). frag: w1..w3 are fragment-major images
    // (mlp3_pack_frag) declared with the same shapes
    CHECK_GPU(x0); CHECK_CONT(x0);
    TORCH_CHECK(x0.dtype() == torch::kBFloat16, "mlp3_fwd: x0 must be bf16");
    const c10::cuda::CUDAGuard guard(x0.device());
    long M = x0.size(0), K0p = x0.size(1), H = w1.size(0);
    long Hp = w2.size(1);
    TORCH_CHECK(H % 16 == 0 && H <= 416, "mlp3_fwd: H must be <=416, x16");
    TORCH_CHECK(K0p % 32 == 0 && Hp % 32 == 0,
                "mlp3_fwd: padded K dims must be x32");
    TORCH_CHECK(w1.size(1) == K0p && w2.size(0) == H && w3.size(0) == H
                && w3.size(1) == Hp && w4.numel() == H);
    TORCH_CHECK(bm == 0 || bm == 16 || ((bm == 32 || bm == 64)
                                        && K0p <= 416),
                "mlp3_fwd: bm must be 0, 16, 32 or 64 (32/64: K0p <= 416)");
    if (frag) {   // an image is one linear run of H x Kp elements
        CHECK_CONT(w1); CHECK_CONT(w2); CHECK_CONT(w3);
    }
    auto a1 = torch::empty({M, H}, x0.options());
    auto a2 = torch::empty({M, H}, x0.options());
    auto a3 = torch::empty({M, H}, x0.options());
    auto out = torch::empty({M}, x0.options().dtype(torch::kFloat32));
    const float* pp = nullptr;
    if (partial.has_value()) {
        TORCH_CHECK(partial->is_contiguous() && partial->numel() == M &&
                    partial->dtype() == torch::kFloat32,
                    "mlp3_fwd: partial must be contiguous fp32 [M]");
        pp = partial->data_ptr<float>();
    }
    emb_mlp3_fwd(x0.data_ptr(), M, K0p,
                 w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                 w3.data_ptr(), b3.data_ptr(), w4.data_ptr(), b4.data_ptr(),
                 pp, H, Hp, a1.data_ptr(), a2.data_ptr(), a3.data_ptr(),
                 out.data_ptr<float>(), (int)bm, (int)frag, cur_stream());
    return {out, a1, a2, a3};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
mlp3_bwd(torch::Tensor dout, torch::Tensor a1, torch::Tensor a2,
         torch::Tensor a3, torch::Tensor w4, torch::Tensor w3t,
         torch::Tensor w2t, torch::Tensor w1t, OptTensor bias_scratch,
         long bm, bool frag) {
    // bias_scratch ([4H+1] fp32): when given, the dz3 assembly loop also
    // accumulates dw4 (dout.a3 column sums) and db4 into segments 3H/4H.
    // frag: w3t..w1t are fragment-major images (mlp3_pack_frag)
    CHECK_GPU(dout); CHECK_CONT(dout); CHECK_CONT(w3t); CHECK_CONT(w2t);
    CHECK_CONT(w1t);
    const c10::cuda::CUDAGuard guard(dout.device());
    long M = a1.size(0), H = a1.size(1), K0p = w1t.size(0);
    long Hp = w3t.size(1);
    TORCH_CHECK(Hp % 32 == 0 && w2t.size(1) == Hp && w1t.size(1) == Hp);
    TORCH_CHECK(H % 16 == 0 && H <= 416 && K0p % 16 == 0,
                "mlp3_bwd: H must be <=416, x16");
    TORCH_CHECK(bm == 0 || bm == 16 || bm == 32 || bm == 64,
                "mlp3_bwd: bm must be 0, 16, 32 or 64");
    auto dz1 = torch::empty_like(a1);
    auto dz2 = torch::empty_like(a2);
    auto dz3 = torch::empty_like(a3);
    auto dx0 = torch::empty({M, K0p}, a1.options());
    float* bptr = nullptr;
    if (bias_scratch.has_value()) {
        CHECK_CONT(*bias_scratch);
        TORCH_CHECK(bias_scratch->numel() >= 4 * H + 1
                    && bias_scratch->dtype() == torch::kFloat32,
                    "bias_scratch layout");
        bptr = bias_scratch->data_ptr<float>();
    }
    emb_mlp3_bwd(dout.data_ptr<float>(), M, K0p, a1.data_ptr(),
                 a2.data_ptr(), a3.data_ptr(), w4.data_ptr(), w3t.data_ptr(),
                 w2t.data_ptr(), w1t.data_ptr(), H, Hp, dz1.data_ptr(),
                 dz2.data_ptr(), dz3.data_ptr(), dx0.data_ptr(), bptr,
                 (int)bm, (int)frag, cur_stream());
    return {dx0, dz1, dz2, dz3};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("unique_inverse", &unique_inverse, "hash-based unique+inverse");
    m.def("unique_bounded", &unique_bounded,
          "unique+inverse without host sync (n-sized buffer + device "
          "count); optional fused per-field key offsets",
          pybind11::arg("keys"),
          pybind11::arg("field_offsets") = pybind11::none());
    m.def("ht_lookup", &ht_lookup, "hash table lookup/insert");
    m.def("ht_rehash", &ht_rehash, "hash table rehash into larger table");
    m.def("ht_lookup_admit", &ht_lookup_admit,
          "hash table lookup/insert behind a count-min admission filter",
          pybind11::arg("tk"), pybind11::arg("tv"), pybind11::arg("keys"),
          pybind11::arg("nrows"), pybind11::arg("slot_keys"),
          pybind11::arg("sketch"), pybind11::arg("depth"),
          pybind11::arg("seed"), pybind11::arg("min_count"),
          pybind11::arg("stats"), pybind11::arg("u_dev") = pybind11::none());
    m.def("admit_age", &admit_age,
          "arithmetic right shift of every admission counter, in place");
    m.def("array_touch", &array_touch,
          "array-table slot compute + valid-bitmap touch");
    m.def("gather_init", &gather_init,
          "row gather with fused lazy init (+ optional duplicate scatter)");
    m.def("reduce_by_inverse", &reduce_by_inverse,
          "grad reduce-by-key with counts (LDS-aggregated)");
    m.def("unique_bounded_indexed", &unique_bounded_indexed,
          "unique_bounded plus the batch's inverted index (seg_off, "
          "seg_cnt, perm, long_list, n_long)",
          pybind11::arg("keys"),
          pybind11::arg("field_offsets") = pybind11::none());
    m.def("unique_bounded_assign", &unique_bounded_assign,
          "unique_bounded_indexed stopped after the assign kernel (array "
          "touch inside it when valid is given); pull_merged continues",
          pybind11::arg("keys"),
          pybind11::arg("field_offsets") = pybind11::none(),
          pybind11::arg("valid") = pybind11::none(),
          pybind11::arg("shard_num") = 1);
    m.def("pull_merged", &pull_merged,
          "inverse + index filing + gather/lazy init in one launch");
    m.def("reduce_by_index", &reduce_by_index,
          "grad reduce-by-key with counts through the inverted index "
          "(segmented, no atomics)");
    m.def("reduce_apply_by_index", &reduce_apply_by_index,
          "reduce_by_index + apply_optimizer in one launch: the summed "
          "rows are applied where they are formed");
    m.def("seg_reduce_threshold", &emb_seg_threshold,
          "list length above which a uid is in long_list");
    m.def("seg_reduce_max_dim", &emb_seg_max_dim,
          "widest dim reduce_by_index covers");
    m.def("pool_fwd", &pool_fwd,
          "segment-pooled gather (sum/mean/sqrtn) over ragged bags; also "
          "emits each element's bag for the backward",
          pybind11::arg("rows"), pybind11::arg("inverse"),
          pybind11::arg("map"), pybind11::arg("offsets"),
          pybind11::arg("mode"), pybind11::arg("want_bag_of") = true);
    m.def("reduce_bags_by_inverse", &reduce_bags_by_inverse,
          "grad reduce-by-key reading the pooled [B, dim] gradient through "
          "bag_of (no [nnz, dim] expansion)");
    m.def("pool_fwd_weighted", &pool_fwd_weighted,
          "pool_fwd with per-sample weights; also emits bag_of and the "
          "per-bag combiner scale for the backward",
          pybind11::arg("rows"), pybind11::arg("inverse"),
          pybind11::arg("map"), pybind11::arg("offsets"),
          pybind11::arg("weights"), pybind11::arg("mode"),
          pybind11::arg("out") = pybind11::none(),
          pybind11::arg("bag_scale") = pybind11::none());
    m.def("reduce_bags_weighted_by_inverse",
          &reduce_bags_weighted_by_inverse,
          "bag-indirected grad reduce with the per-element factor "
          "weights[e] * bag_scale[bag_of[e]]");
    m.def("pool_wgrad", &pool_wgrad,
          "gradient of the weighted pool w.r.t. its per-sample weights",
          pybind11::arg("rows"), pybind11::arg("inverse"),
          pybind11::arg("map"), pybind11::arg("weights"),
          pybind11::arg("bag_of"), pybind11::arg("bag_scale"),
          pybind11::arg("out"), pybind11::arg("grad_out"),
          pybind11::arg("mode"), pybind11::arg("dw") = pybind11::none());
    m.def("pool_lookup", &pool_lookup,
          "read-only pooled lookup, keys -> pooled rows in one launch "
          "(hash: tk/tv; array: valid/shard_num)",
          pybind11::arg("rows"), pybind11::arg("values"),
          pybind11::arg("offsets"), pybind11::arg("mode"),
          pybind11::arg("weights") = pybind11::none(),
          pybind11::arg("tk") = pybind11::none(),
          pybind11::arg("tv") = pybind11::none(),
          pybind11::arg("valid") = pybind11::none(),
          pybind11::arg("shard_num") = 1);
    m.def("quantize_rows", &quantize_rows,
          "fp32 rows -> packed rows at the given slots of a slab (slots "
          "unique within a call)",
          pybind11::arg("w"), pybind11::arg("slots"), pybind11::arg("slab"),
          pybind11::arg("fmt"));
    m.def("pool_lookup_q", &pool_lookup_q,
          "read-only pooled lookup over a packed slab, keys -> pooled fp32 "
          "rows in one launch (hash: tk/tv; array: valid/shard_num)",
          pybind11::arg("slab"), pybind11::arg("dim"), pybind11::arg("fmt"),
          pybind11::arg("values"), pybind11::arg("offsets"),
          pybind11::arg("mode"),
          pybind11::arg("weights") = pybind11::none(),
          pybind11::arg("tk") = pybind11::none(),
          pybind11::arg("tv") = pybind11::none(),
          pybind11::arg("valid") = pybind11::none(),
          pybind11::arg("shard_num") = 1);
    m.def("gather_lookup_q", &gather_lookup_q,
          "flat read over a packed slab, keys -> fp32 rows in one launch",
          pybind11::arg("slab"), pybind11::arg("dim"), pybind11::arg("fmt"),
          pybind11::arg("keys"),
          pybind11::arg("tk") = pybind11::none(),
          pybind11::arg("tv") = pybind11::none(),
          pybind11::arg("valid") = pybind11::none(),
          pybind11::arg("shard_num") = 1);
    m.def("apply_optimizer", &apply_optimizer, "fused sparse optimizer step");
    m.def("mask_tail", &mask_tail,
          "zero the garbage tail of a bounded block (enables multi-block "
          "merge by concatenation)");
    m.def("mark_rows", &mark_rows,
          "delta checkpoints: row_epoch[slot] = *epoch_dev for the named "
          "rows (optional byte mask and device count)",
          pybind11::arg("slots"), pybind11::arg("mask") = pybind11::none(),
          pybind11::arg("u_dev") = pybind11::none(),
          pybind11::arg("epoch_dev"), pybind11::arg("row_epoch"));
    m.attr("DELTA_TILE_ROWS") = emb_delta_tile_rows();
    m.def("select_changed", &select_changed,
          "delta checkpoints: ascending slots of the live rows with "
          "row_epoch >= since -> (slots [R] with a -1 tail, n_dev int32[1])",
          pybind11::arg("row_epoch"), pybind11::arg("since"),
          pybind11::arg("nrows_dev") = pybind11::none(),
          pybind11::arg("valid") = pybind11::none());
    m.def("gather_rows_by_slot", &gather_rows_by_slot,
          "delta checkpoints: keys, weights and state of "
          "slots[start:start+count] into staging buffers",
          pybind11::arg("weights"), pybind11::arg("state"),
          pybind11::arg("slot_keys") = pybind11::none(),
          pybind11::arg("shard_num") = 1, pybind11::arg("shard_id") = 0,
          pybind11::arg("slots"), pybind11::arg("start"),
          pybind11::arg("count"), pybind11::arg("n_dev"),
          pybind11::arg("keys_out") = pybind11::none(),
          pybind11::arg("w_out") = pybind11::none(),
          pybind11::arg("s_out") = pybind11::none());
    m.def("expire_flags", &expire_flags,
          "row expiry: dead uint8 [R] = live rows with row_epoch < before",
          pybind11::arg("row_epoch"), pybind11::arg("before"),
          pybind11::arg("nrows_dev") = pybind11::none(),
          pybind11::arg("valid") = pybind11::none());
    m.def("flag_slots", &flag_slots,
          "row expiry: dead uint8 [rows] = 1 at the named slots",
          pybind11::arg("slots"), pybind11::arg("rows"));
    m.def("remove_flagged", &remove_flagged,
          "row expiry (hash table): fill the holes of the flagged rows in "
          "place over every plane and rebuild the probe table -> (removed "
          "keys in old-slot order, live rows left)",
          pybind11::arg("dead"), pybind11::arg("planes"),
          pybind11::arg("slot_keys"), pybind11::arg("tk"),
          pybind11::arg("tv"), pybind11::arg("nrows_dev"));
    m.def("remove_flagged_array", &remove_flagged_array,
          "row expiry (array table): clear the valid byte of the flagged "
          "rows -> removed keys, ascending",
          pybind11::arg("dead"), pybind11::arg("valid"),
          pybind11::arg("shard_num") = 1, pybind11::arg("shard_id") = 0);
    m.def("fault_in", &fault_in,
          "tier v2: copy host-resident rows into fresh cache slots, "
          "clearing their lazy-init mask");
    m.def("spill_rows", &spill_rows,
          "tier v2: copy cache rows into the pinned host slab");
    m.def("gather_host", &gather_host,
          "tier v2: read-only host-row gather for cache misses");
    m.def("bucketize_pad", &bucketize_pad,
          "owner-bucketize unique keys into a fixed padded [world, cap] "
          "wire block (sync-free multi-rank route)");
    m.def("gather_pad", &gather_pad,
          "gather grads+counts payload into the padded send layout");
    m.def("scatter_out", &scatter_out,
          "padded pull: wire rows -> per-element output (fused dup scatter)");
    m.def("split_payload", &split_payload,
          "split owner-reduced payload into grads + int64 counts");
    m.def("ctr_head_fwd", &ctr_head_fwd,
          "fused CTR head fwd: deep_in assembly (+cast) + FM + first-order "
          "+ dense linear",
          pybind11::arg("e_all"), pybind11::arg("dense"), pybind11::arg("w"),
          pybind11::arg("bias"), pybind11::arg("use_fm"),
          pybind11::arg("out_bf16"), pybind11::arg("pad32"),
          pybind11::arg("impl") = 0);
    m.def("ctr_head_bwd", &ctr_head_bwd, "fused CTR head backward",
          pybind11::arg("e_all"), pybind11::arg("dense"), pybind11::arg("w"),
          pybind11::arg("d_deep_in"), pybind11::arg("d_partial"),
          pybind11::arg("s"), pybind11::arg("use_fm"),
          pybind11::arg("impl") = 0);
    m.def("ctr_head_bwd_acc", &ctr_head_bwd_acc,
          "fused CTR head backward in one launch, dw/db added into the "
          "caller's buffers",
          pybind11::arg("e_all"), pybind11::arg("dense"), pybind11::arg("w"),
          pybind11::arg("d_deep_in"), pybind11::arg("d_partial"),
          pybind11::arg("s"), pybind11::arg("use_fm"),
          pybind11::arg("dw_acc"), pybind11::arg("db_acc"),
          pybind11::arg("want_d_dense") = true);
    m.def("ctr_head_rows_plan", &ctr_head_rows_plan,
          "samples per block of the row-staged head kernels for a shape");
    m.def("mlp3_bwd", &mlp3_bwd,
          "fused dgrad chain backward of the 3-layer MLP (optionally "
          "carrying the head wgrad/bias sums)",
          pybind11::arg("dout"), pybind11::arg("a1"), pybind11::arg("a2"),
          pybind11::arg("a3"), pybind11::arg("w4"), pybind11::arg("w3t"),
          pybind11::arg("w2t"), pybind11::arg("w1t"),
          pybind11::arg("bias_scratch") = pybind11::none(),
          pybind11::arg("bm") = 0, pybind11::arg("frag") = false);
    m.def("mlp3_pack", &mlp3_pack,
          "refresh three padded (or transposed) weight copies in one "
          "launch");
    m.def("mlp3_pack_frag", &mlp3_pack_frag,
          "write up to six fragment-major weight images (pads included) "
          "in one launch",
          pybind11::arg("srcs"), pybind11::arg("dsts"),
          pybind11::arg("trans"));
    m.def("mlp3_fwd", &mlp3_fwd,
          "fused 3-hidden-layer MLP forward (bf16 MFMA, bias+ReLU fused)",
          pybind11::arg("x0"), pybind11::arg("w1"), pybind11::arg("b1"),
          pybind11::arg("w2"), pybind11::arg("b2"), pybind11::arg("w3"),
          pybind11::arg("b3"), pybind11::arg("w4"), pybind11::arg("b4"),
          pybind11::arg("partial"), pybind11::arg("bm") = 0,
          pybind11::arg("frag") = false);
    m.def("mlp3_wgrad", &mlp3_wgrad,
          pybind11::arg("dz1"), pybind11::arg("dz2"), pybind11::arg("dz3"),
          pybind11::arg("x0"), pybind11::arg("a1"), pybind11::arg("a2"),
          pybind11::arg("scratch"), pybind11::arg("dw1"),
          pybind11::arg("dw2"), pybind11::arg("dw3"),
          pybind11::arg("bias_scratch") = pybind11::none(),
          pybind11::arg("m_split") = 0,
          "all three MLP weight grads in one MFMA launch (+= into bf16 "
          "grads via fp32 scratch)");
    m.def("mlp3_bias_bwd", &mlp3_bias_bwd,
          "MLP bias grads + head wgrad in one pass over the dz mirrors "
          "(with_dz=false when the fused wgrad carried the dz sums)",
          pybind11::arg("dout"), pybind11::arg("dz1"), pybind11::arg("dz2"),
          pybind11::arg("dz3"), pybind11::arg("a3"),
          pybind11::arg("scratch"), pybind11::arg("db1"),
          pybind11::arg("db2"), pybind11::arg("db3"), pybind11::arg("dw4"),
          pybind11::arg("db4"), pybind11::arg("with_dz") = true,
          pybind11::arg("with_head") = true);
    m.def("cin_fwd", &cin_fwd,
          "CIN layer forward: implicit outer-product MFMA GEMM");
    m.def("cin_dw", &cin_dw,
          "CIN weight grad: per-field split-K MFMA with on-the-fly operand");
    m.def("cin_dx", &cin_dx,
          "CIN input grads: P=W^T dZ GEMM fused with the xk/x0 contractions");
    m.def("bce_fwd", &bce_fwd, "fused BCE-with-logits forward (mean)");
    m.def("bce_bwd", &bce_bwd, "fused BCE-with-logits backward");
    m.def("flat_adagrad", &flat_adagrad,
          "fused flat-buffer Adagrad (f32, or bf16 weights + f32 master)");
    m.def("flat_opt", &flat_opt,
          "fused flat-buffer dense optimizer (0=sgd, 1=adagrad, 2=adam)");
    m.def("flat_step_scalars", &flat_step_scalars,
          "device-side step counter + Adam bias-correction factors "
          "(capture-safe)");
}
