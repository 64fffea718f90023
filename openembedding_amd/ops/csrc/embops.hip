// openembedding_amd CDNA4 (gfx950 / MI355X) kernels.
//
// GPU-resident rebuild of the reference's CPU parameter-server primitives
// (see SURVEY.md §2.8 for the mapping):
//   unique+inverse        <- client dedup, EmbeddingPullOperator.cpp:67-79
//   hash lookup/insert    <- EasyHashMap row lookup, EmbeddingTable.h:72-98
//   gather + lazy init    <- pull_weights miss path,
//                            EmbeddingOptimizerVariable.h:242-266
//   reduce-by-inverse     <- client grad pre-agg + MpscGradientReducer
//   fused sparse optimizers (9) <- EmbeddingOptimizer.h:49-390, applied once
//                            per unique key per batch with occurrence counts
//
// Design notes (MI355X):
//   - wave = 64 lanes; rows are handled by power-of-2 lane groups (G=16 for
//     dim<=32, G=64 above) so a group's row read is one coalesced segment;
//   - all tables live in HBM; probing is 1 load/probe on a splitmix64 hash
//     (load factor kept <= 0.5 by the host);
//   - lazy row init is a deterministic function of (seed, key, col, attempt)
//     via splitmix64 — bit-identical to the torch oracle in core/rng.py;
//   - compile with -ffp-contract=off so optimizer/init math matches the
//     torch float32 oracle op-for-op (no silent fma contraction).
//
// No CUDA-compat paths: this file is HIP-for-gfx950 only.

#include <hip/hip_runtime.h>
#include <cstdint>

#define DEV static __device__ __forceinline__

typedef unsigned long long u64;
typedef long long i64;

static constexpr u64 EMPTY = ~0ull;
static constexpr int BLOCK = 256;

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
static inline int grid1d(long n) {
    long g = (n + BLOCK - 1) / BLOCK;
    return (int)(g < 1 ? 1 : g);
}

// ---------------------------------------------------------------- fills
// Graph-capture-safe buffer resets. hipMemsetAsync on a capturing stream is
// NOT reliably captured into the graph on this stack (observed: scratch
// tables were cleared at capture time only, overflowed after two replays
// and the probe loops spun) — plain fill kernels capture like any launch.

template <typename T>
__global__ void k_fill(T* __restrict__ p, long n, T v) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

static inline void fill_u64(u64* p, long n, u64 v, hipStream_t s) {
    if (n) k_fill<u64><<<(int)((n + 255) / 256), 256, 0, s>>>(p, n, v);
}
static inline void fill_i32(int* p, long n, int v, hipStream_t s) {
    if (n) k_fill<int><<<(int)((n + 255) / 256), 256, 0, s>>>(p, n, v);
}
static inline void fill_u8(unsigned char* p, long n, unsigned char v,
                           hipStream_t s) {
    if (n) k_fill<unsigned char><<<(int)((n + 255) / 256), 256, 0, s>>>(p, n, v);
}
static inline void fill_f32(float* p, long n, float v, hipStream_t s) {
    if (n) k_fill<float><<<(int)((n + 255) / 256), 256, 0, s>>>(p, n, v);
}

// One launch resetting all of emb_unique's scratch (table + counter +
// is_first) — three separate fills cost ~2 extra kernel ramps per pull in
// the captured train step.
//
// IDX = true is the indexed dedup (see "inverted index" below); UIdx holds
// its scratch and outputs and is all-null for IDX = false.
struct UIdx {
    int* tcount;       // [cap] occurrences of the key in table slot s
    int* toff;         // [cap] start of that key's list in perm
    int* rank;         // [n] position of element i inside its key's list
    int* seg_off;      // [n] per uid: list start in perm
    int* seg_cnt;      // [n] per uid: list length
    int* perm;         // [n] element ids grouped by uid
    int* long_list;    // [long_cap] uids with seg_cnt > SEG_T
    int* off_counter;  // bump allocator of perm ranges
    int* n_long;       // live entries of long_list
    long long_cap;
};

template <bool IDX>
__global__ void k_unique_reset(u64* __restrict__ tk, long cap,
                               unsigned char* __restrict__ is_first, long n,
                               int* __restrict__ counter, UIdx ix) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cap) {
        tk[i] = ~0ull;   // EMPTY
        if constexpr (IDX) ix.tcount[i] = 0;
    }
    if (i < n) is_first[i] = 0;
    if (i == 0) {
        *counter = 0;
        if constexpr (IDX) { *ix.off_counter = 0; *ix.n_long = 0; }
    }
}

// Same idea for the reduce-by-key scratch (payload accumulator + counts).
__global__ void k_reduce_reset(float* __restrict__ ugrads, long ne,
                               u64* __restrict__ counts, long u) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ne) ugrads[i] = 0.0f;
    if (i < u) counts[i] = 0ull;
}

// And for the padded all-to-all send blocks (keys + src + per-peer counts).
__global__ void k_pad_reset(u64* __restrict__ send_keys,
                            int* __restrict__ send_src, long total,
                            int* __restrict__ counts, long world) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) { send_keys[i] = ~0ull; send_src[i] = -1; }
    if (i < world) counts[i] = 0;
}

// ------------------------------------------------------------------ rng

DEV u64 splitmix64(u64 z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// NOTE: core/rng.py applies the same constants with the "+C1" folded into the
// first line; both sides compute splitmix64(x) identically.

DEV u64 uniform_bits(u64 seed, u64 key, u64 col, u64 attempt) {
    u64 x = key * 0x100000ull + col + (attempt << 40);
    return splitmix64(splitmix64(x) ^ seed);
}

DEV float uniform01(u64 seed, u64 key, u64 col, u64 attempt) {
    return (float)(uniform_bits(seed, key, col, attempt) >> 40)
           * (1.0f / 16777216.0f);
}

// init categories
enum { INIT_CONSTANT = 0, INIT_UNIFORM = 1, INIT_NORMAL = 2 };

DEV float normal01(u64 seed, u64 key, u64 col, u64 attempt) {
    float u1 = uniform01(seed, key, col, 2 * attempt);
    float u2 = uniform01(seed, key, col, 2 * attempt + 1);
    float r = sqrtf(-2.0f * logf(1.0f - u1));
    return r * cosf(2.0f * 3.14159265358979323846f * u2);
}

DEV float init_value(int cat, float p0, float p1, float p2,
                     u64 seed, u64 key, u64 col) {
    // constant: p0=value; uniform: p0=minval p1=maxval-minval;
    // normal: p0=mean p1=stddev p2=truncated (one-sided rejection, reference
    // EmbeddingInitializer.h:76-81 resamples only while (w-mean)/stddev > trunc)
    if (cat == INIT_CONSTANT) return p0;
    if (cat == INIT_UNIFORM) {
        // the span arrives already rounded: the host subtracts in double
        // and rounds once, like core/rng.py. 0.7f - 0.1f here would be one
        // ulp off float(0.7 - 0.1) and break bit-identity with the oracle.
        float u = uniform01(seed, key, col, 0);
        return p0 + u * p1;
    }
    float z = normal01(seed, key, col, 0);
    if (p2 > 0.1f) {
        for (int attempt = 1; attempt < 16 && z > p2; ++attempt)
            z = normal01(seed, key, col, attempt);
    }
    return p0 + p1 * z;
}

// ------------------------------------------------------- unique + inverse
// Batch-local dedup via a scratch open-addressed table (3 passes, no spin).
//
// Contention design: CTR batches contain extremely hot keys (a vocab-3 field
// contributes batch_size copies of 3 keys), so a naive per-element CAS
// serializes thousands of atomics on one cache line (measured 24us for a
// 106k batch). An LDS pre-filter dedups per block first: one block-winner
// probes the global table and publishes the slot through LDS; hot-key global
// CAS count drops from O(batch) to O(blocks).

#define ULDS 1024  // LDS pre-filter entries (8 KiB keys + 4 KiB slots)
#define UA_ITERS 8  // elements per thread in the uid-assign kernel
#define UI_ILP 4    // parallel lookups per thread in the inverse kernel
#define SEG_T 32    // inverted index: lists longer than this are "long"

// foff/F: optional per-field key offsets fused into the read (keys is then
// the RAW [B, F] field-id layout; flat key = keys[i] + foff[i % F]) — saves
// the broadcast-add launch + 8B/elem intermediate every pull.
//
// IDX: every element also learns its rank inside its key's list. The
// block's copies of a key rank themselves with a returning LDS add on the
// key's LDS entry; after the barrier the block winner reserves the block's
// range with ONE returning global add on tcount[slot] and publishes the
// base through LDS, so a hot key costs one global atomic per block, like
// its CAS. Elements on the LDS-overflow route add 1 to tcount themselves.
template <bool IDX>
__global__ void k_unique_insert(const i64* __restrict__ keys, long n,
                                u64* __restrict__ tk, long mask,
                                int* __restrict__ slot_of,
                                unsigned char* __restrict__ is_first,
                                const i64* __restrict__ foff, int F,
                                UIdx ix) {
    __shared__ u64 lkeys[ULDS];
    __shared__ int lslot[ULDS];
    __shared__ int lcnt[IDX ? ULDS : 1];    // block's copies of the key
    __shared__ int lbase[IDX ? ULDS : 1];   // their base in the key's list
    for (int t = threadIdx.x; t < ULDS; t += blockDim.x) {
        lkeys[t] = EMPTY;
        if constexpr (IDX) lcnt[t] = 0;
    }
    __syncthreads();

    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    u64 k = 0;
    i64 kin = 0;
    if (i < n) {
        kin = keys[i];
        if (foff) kin += foff[(int)i % F];   // n < 2^31: 32-bit mod
    }
    int lh = -1;           // LDS slot of this element's key
    int lr = 0;            // IDX: rank among the block's copies / own rank
    bool lds_winner = false, lds_ok = false;
    if (i < n && (u64)kin == EMPTY) {
        // RESERVED key -1 (the scratch table's empty marker, same value the
        // reference reserves): give every occurrence the overflow-winner
        // encoding — its own unique entry, resolved to slot -1 (zeros)
        // downstream — instead of vacuously matching empty probe slots.
        is_first[i] = 1;
        slot_of[i] = -1;
    } else if (i < n) {
        k = (u64)kin;
        u64 hh = splitmix64(k);
        lh = (int)(hh & (ULDS - 1));
        for (int probes = 0; probes < 64; ++probes) {
            u64 cur = atomicCAS(&lkeys[lh], EMPTY, k);
            if (cur == EMPTY) { lds_winner = true; lds_ok = true; break; }
            if (cur == k) { lds_ok = true; break; }
            lh = (lh + 1) & (ULDS - 1);
        }
        if constexpr (IDX)
            if (lds_ok) lr = atomicAdd(&lcnt[lh], 1);
        if (lds_winner || !lds_ok) {
            // block winner (or LDS overflow): probe the global table.
            // Probes are BOUNDED by the table size: an overfull table (can
            // only happen on a host sizing bug) must never hang the GPU —
            // the overflow element becomes its own unique (slot_of
            // encoding: -1 = overflow winner, assigned directly in the
            // assign kernel; <=-2 = duplicate pointing at winner element).
            u64 h = splitmix64(k) & (u64)mask;
            long found = -1;
            for (long p = 0; p <= mask; ++p) {
                u64 cur = tk[h];
                if (cur == k) { found = (long)h; break; }
                if (cur == EMPTY) {
                    u64 prev = atomicCAS(&tk[h], EMPTY, k);
                    if (prev == EMPTY) {
                        is_first[i] = 1; found = (long)h; break;
                    }
                    if (prev == k) { found = (long)h; break; }
                }
                h = (h + 1) & (u64)mask;
            }
            if (found < 0) is_first[i] = 1;  // overflow: own unique
            slot_of[i] = found >= 0 ? (int)found : -1;
            if (lds_winner)
                lslot[lh] = found >= 0 ? (int)found : (int)(-2 - i);
            if constexpr (IDX)
                if (!lds_ok && found >= 0)
                    lr = atomicAdd(&ix.tcount[found], 1);
        }
    }
    __syncthreads();
    if (i < n && lds_ok && !lds_winner) slot_of[i] = lslot[lh];
    if constexpr (IDX) {
        if (lds_winner) {
            // a winner without a table slot (global overflow) is a list of
            // one; its block duplicates are then in no list (file header
            // of the inverted index: wrong numbers, never a bad access)
            int s = lslot[lh];
            lbase[lh] = s >= 0 ? atomicAdd(&ix.tcount[s], lcnt[lh]) : 0;
        }
        __syncthreads();
        if (i < n) ix.rank[i] = lds_ok ? lbase[lh] + lr : lr;
    }
}

//
// IDX: a first occurrence also reads its key's final count tcount[slot]
// and takes the key's range of perm from a second bump counter: the
// thread's counts are summed, a wave scan turns them into offsets and lane
// 0 reserves the wave's total beside the uid range, so the kernel still
// waits on one round of returning atomics per wave. Offsets therefore do
// not follow uid order. A first occurrence without a slot (reserved -1,
// global overflow) is a list of one and files itself in perm here.
//
// TOUCH: a first occurrence also does what k_array_touch does for its key
// (array tables): slot = key / shard_num with the same guards (key < 0 and
// slot >= cap give slot -1 and mask 0, which covers the reserved -1), reads
// and sets valid[slot] and writes slots[uid] / new_mask[uid]. The key and
// valid[slot] are loaded beside tcount, before the returning atomics, so
// the touch adds no round trip to the kernel's chain. Entries at and beyond
// *u_dev are left to the caller's next kernel (k_pull_merged), because the
// unique count is final only when this kernel has ended.
struct UTouch {
    unsigned char* valid;      // [cap] rows that are live
    long shard_num, cap;
    i64* slots;                // [n] per uid: table slot, -1 = none
    unsigned char* new_mask;   // [n] per uid: the row is new
};

DEV i64 array_slot(i64 key, long shard_num, long cap) {
    if (key < 0) return -1;     // C++ division would map -1 to slot 0
    i64 s = shard_num == 1 ? key : key / shard_num;
    return (s < 0 || s >= cap) ? -1 : s;
}

template <bool IDX, bool TOUCH = false>
__global__ void k_unique_assign(const i64* __restrict__ keys, long n,
                                const int* __restrict__ slot_of,
                                const unsigned char* __restrict__ is_first,
                                int* __restrict__ tv,
                                i64* __restrict__ unique_keys,
                                int* __restrict__ counter,
                                i64* __restrict__ inverse,
                                const i64* __restrict__ foff, int F,
                                UIdx ix, UTouch tch) {
    // UA_ITERS elements per thread with ONE returning atomic per wave:
    // ballots for all iterations are taken first (independent loads in
    // flight), their popcounts summed, a single atomicAdd reserves the uid
    // range, then uids are assigned per iteration from the running prefix.
    // (The one-atomic-per-wave version was 99% SQ_WAIT_ANY parked on the
    // dependent L2 atomic: 21.6 us/step.)
    const int lane = threadIdx.x & 63;
    const long stride = (long)gridDim.x * blockDim.x;
    long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    u64 ballots[UA_ITERS];
    int sl[IDX ? UA_ITERS : 1], c[IDX ? UA_ITERS : 1];
    i64 tkey[TOUCH ? UA_ITERS : 1], tslot[TOUCH ? UA_ITERS : 1];
    unsigned char twas[TOUCH ? UA_ITERS : 1];
    int total = 0;
    #pragma unroll
    for (int t = 0; t < UA_ITERS; ++t) {
        long i = i0 + t * stride;
        // IDX: every element's slot is read beside is_first (both
        // coalesced), so the tcount lookup does not wait for the ballots
        if constexpr (IDX) sl[t] = (i < n) ? slot_of[i] : -1;
        if constexpr (TOUCH) {
            // every element's key, coalesced beside slot_of: valid[slot]
            // is then one dependent load behind the ballots, like tcount
            tkey[t] = -1;
            if (i < n) {
                tkey[t] = keys[i];
                if (foff) tkey[t] += foff[(int)i % F];
            }
        }
        bool first = (i < n) && is_first[i];
        ballots[t] = __ballot(first);
        total += __popcll(ballots[t]);
    }
    if (!total) return;
    if constexpr (TOUCH) {
        #pragma unroll
        for (int t = 0; t < UA_ITERS; ++t)
            tslot[t] = (ballots[t] >> lane & 1ull)
                ? array_slot(tkey[t], tch.shard_num, tch.cap) : -1;
        #pragma unroll
        for (int t = 0; t < UA_ITERS; ++t)
            twas[t] = tslot[t] >= 0 ? tch.valid[tslot[t]] : 1;
    }
    int off = 0, wtot = 0;
    if constexpr (IDX) {
        int ctot = 0;
        #pragma unroll
        for (int t = 0; t < UA_ITERS; ++t) {
            c[t] = (ballots[t] >> lane & 1ull)
                       ? (sl[t] >= 0 ? ix.tcount[sl[t]] : 1) : 0;
            ctot += c[t];
        }
        int inc = ctot;   // inclusive wave scan of the per-thread totals
        #pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            int v = __shfl_up(inc, d, 64);
            if (lane >= d) inc += v;
        }
        wtot = __shfl(inc, 63, 64);
        off = inc - ctot;
    }
    int base = 0, obase = 0;
    if (lane == 0) {
        base = atomicAdd(counter, total);
        if constexpr (IDX) obase = atomicAdd(ix.off_counter, wtot);
    }
    base = __shfl(base, 0, 64);
    if constexpr (IDX) off += __shfl(obase, 0, 64);
    #pragma unroll
    for (int t = 0; t < UA_ITERS; ++t) {
        u64 b = ballots[t];
        if (b & (1ull << lane)) {
            long i = i0 + t * stride;
            int uid = base + __popcll(b & ((1ull << lane) - 1ull));
            i64 kin;
            if constexpr (TOUCH) {
                kin = tkey[t];
                tch.slots[uid] = tslot[t];
                tch.new_mask[uid] = !twas[t];
                if (tslot[t] >= 0) tch.valid[tslot[t]] = 1;
            } else {
                kin = keys[i];
                if (foff) kin += foff[(int)i % F];
            }
            unique_keys[uid] = kin;
            int s;
            if constexpr (IDX) s = sl[t]; else s = slot_of[i];
            if (s >= 0) tv[s] = uid;
            else inverse[i] = uid;  // overflow winner: direct assignment
            if constexpr (IDX) {
                ix.seg_off[uid] = off;
                ix.seg_cnt[uid] = c[t];
                if (s >= 0) ix.toff[s] = off;
                else if (off >= 0 && off < n) ix.perm[off] = (int)i;
                if (c[t] > SEG_T) {
                    int q = atomicAdd(ix.n_long, 1);
                    if (q < ix.long_cap) ix.long_list[q] = uid;
                }
                off += c[t];
            }
        }
        base += __popcll(b);
    }
}

// IDX: element i is filed at perm[toff[slot] + rank[i]].
template <bool IDX>
__global__ void k_unique_inverse(long n, const int* __restrict__ slot_of,
                                 const int* __restrict__ tv,
                                 i64* __restrict__ inverse, UIdx ix) {
    // UI_ILP independent lookups in flight per thread (2-deep load chain
    // slot_of -> tv; single-element version was latency-parked)
    const long stride = (long)gridDim.x * blockDim.x;
    long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    int s[UI_ILP];
    #pragma unroll
    for (int t = 0; t < UI_ILP; ++t) {
        long i = i0 + t * stride;
        s[t] = (i < n) ? slot_of[i] : -1;
    }
    int v[UI_ILP];
    int r[IDX ? UI_ILP : 1], o[IDX ? UI_ILP : 1];
    #pragma unroll
    for (int t = 0; t < UI_ILP; ++t) {
        v[t] = (s[t] >= 0) ? tv[s[t]] : 0;
        if constexpr (IDX) {
            o[t] = (s[t] >= 0) ? ix.toff[s[t]] : 0;
            r[t] = (s[t] >= 0) ? ix.rank[i0 + t * stride] : 0;
        }
    }
    #pragma unroll
    for (int t = 0; t < UI_ILP; ++t) {
        long i = i0 + t * stride;
        if (i >= n) continue;
        if constexpr (IDX) {
            long p = (long)o[t] + r[t];
            if (s[t] >= 0 && p >= 0 && p < n) ix.perm[p] = (int)i;
        }
        if (s[t] >= 0) inverse[i] = (i64)v[t];
        else if (s[t] <= -2) inverse[i] = inverse[-2 - s[t]];
        // s[t] == -1: overflow winner, set by the assign kernel
    }
}

// --------------------------------------------------- persistent hash table
// keys arriving here are UNIQUE within one call (callers dedup first), so a
// CAS loser on slot h can only be a different key -> keep probing; the value
// written by an insert in an earlier kernel is visible (kernel-boundary
// ordering), no spin needed.

// The probe / insert loop of one key (never EMPTY), shared by k_ht_lookup
// and the admission kernels below. Returns the slot, -1 for a miss; is_new
// is set when this call created the row.
DEV i64 ht_probe(u64* __restrict__ tk, int* __restrict__ tv, long mask,
                 u64 k, int insert, int* __restrict__ nrows,
                 i64* __restrict__ slot_keys, long row_cap,
                 unsigned char& is_new) {
    u64 h = splitmix64(k) & (u64)mask;
    i64 slot = -1;
    is_new = 0;
    // bounded probe: a full table (host sizing bug) yields slot -1 (miss)
    // instead of hanging the GPU
    for (long p = 0; p <= mask; ++p) {
        u64 cur = tk[h];
        if (cur == k) { slot = (i64)tv[h]; break; }
        if (cur == EMPTY) {
            if (!insert) { slot = -1; break; }
            u64 prev = atomicCAS(&tk[h], EMPTY, k);
            if (prev == EMPTY) {
                int s = atomicAdd(nrows, 1);
                if (s >= row_cap) {  // slab full (host sizing bug or a
                    tv[h] = -1;      // graph-captured insert): this call AND
                    slot = -1;       // every later lookup of this key must
                    break;           // see a miss — a never-written tv[h]
                }                    // here would later read as a garbage
                                     // slot index (OOB row access)
                tv[h] = s;
                slot_keys[s] = (i64)k;
                slot = s;
                is_new = 1;
                break;
            }
            if (prev == k) { slot = (i64)tv[h]; break; }
        }
        h = (h + 1) & (u64)mask;
    }
    return slot;
}

__global__ void k_ht_lookup(u64* __restrict__ tk, int* __restrict__ tv,
                            long mask, const i64* __restrict__ keys, long n,
                            int* __restrict__ nrows,
                            i64* __restrict__ slot_keys,
                            i64* __restrict__ slots,
                            unsigned char* __restrict__ new_mask,
                            int insert, const int* __restrict__ u_dev,
                            long row_cap) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (u_dev && i >= *u_dev) {
        // beyond the live unique count: write a defined miss — consumers
        // are u_dev-guarded, but a garbage slot index must never reach a
        // host-side scatter (the tier's LRU stamp faulted on exactly that)
        slots[i] = -1;
        if (new_mask) new_mask[i] = 0;
        return;
    }
    u64 k = (u64)keys[i];
    if (k == EMPTY) {
        // key -1 is the table's empty marker and therefore RESERVED —
        // exactly like the reference, which constructs every variable
        // with empty_key = -1 (EmbeddingVariable.cpp:21,38,78). Define
        // it as a miss instead of matching empty probe slots.
        slots[i] = -1;
        if (new_mask) new_mask[i] = 0;
        return;
    }
    unsigned char is_new;
    i64 slot = ht_probe(tk, tv, mask, k, insert, nrows, slot_keys, row_cap,
                        is_new);
    slots[i] = slot;
    if (new_mask) new_mask[i] = is_new;
}

// ------------------------------------------------------ feature admission
// A count-min filter in front of the insert: a key that misses the table
// earns a row only once it was seen min_count times. sketch is D rows of W
// int32 counters (W a power of two); the cell of key k in row j is
// j*W + (splitmix64(splitmix64(k) ^ (seed + j)) & (W-1)), the same function
// as ops/dispatch.py admit_cells.
//
// Two launches. k_admit_note probes read-only; a miss adds 1 to its D cells
// and leaves the marker ADMIT_PENDING. k_admit_resolve, after the kernel
// boundary, reads the D cells back with plain loads: every add of the call
// has landed, so the estimate of a key that shares a cell with another key
// of the same call does not depend on which thread ran first. One kernel
// could not give that. The adds are one dword per lane at hashed addresses,
// the slow shape for atomics; that is the sketch's nature, and a call has
// only D of them per missing key.

static constexpr i64 ADMIT_PENDING = -2;

DEV long admit_cell(u64 hk, u64 seed, int j, long W) {
    return (long)j * W + (long)(splitmix64(hk ^ (seed + (u64)j))
                                & (u64)(W - 1));
}

__global__ void k_admit_note(const u64* __restrict__ tk,
                             const int* __restrict__ tv, long mask,
                             const i64* __restrict__ keys, long n,
                             int* __restrict__ sketch, long W, int D,
                             u64 seed, i64* __restrict__ slots,
                             unsigned char* __restrict__ new_mask,
                             const int* __restrict__ u_dev) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    new_mask[i] = 0;
    if (u_dev && i >= *u_dev) { slots[i] = -1; return; }  // as k_ht_lookup
    u64 k = (u64)keys[i];
    if (k == EMPTY) { slots[i] = -1; return; }            // reserved key
    u64 h = splitmix64(k) & (u64)mask;
    for (long p = 0; p <= mask; ++p) {
        u64 cur = tk[h];
        if (cur == k) { slots[i] = (i64)tv[h]; return; }
        if (cur == EMPTY) break;
        h = (h + 1) & (u64)mask;
    }
    u64 hk = splitmix64(k);
    for (int j = 0; j < D; ++j)
        atomicAdd(&sketch[admit_cell(hk, seed, j, W)], 1);  // no return used
    slots[i] = ADMIT_PENDING;
}

// stats[0] admitted, stats[1] turned away (a sighting that got no row, the
// slab-full case included): one atomic per wave and counter
__global__ void k_admit_resolve(u64* __restrict__ tk, int* __restrict__ tv,
                                long mask, const i64* __restrict__ keys,
                                long n, const int* __restrict__ sketch,
                                long W, int D, u64 seed, int min_count,
                                int* __restrict__ nrows,
                                i64* __restrict__ slot_keys, long row_cap,
                                i64* __restrict__ slots,
                                unsigned char* __restrict__ new_mask,
                                u64* __restrict__ stats) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool pending = i < n && slots[i] == ADMIT_PENDING;
    bool admitted = false;
    if (pending) {
        u64 k = (u64)keys[i];
        u64 hk = splitmix64(k);
        int est = sketch[admit_cell(hk, seed, 0, W)];
        for (int j = 1; j < D; ++j) {
            int c = sketch[admit_cell(hk, seed, j, W)];
            est = c < est ? c : est;
        }
        i64 slot = -1;
        unsigned char is_new = 0;
        if (est >= min_count)
            slot = ht_probe(tk, tv, mask, k, 1, nrows, slot_keys, row_cap,
                            is_new);
        slots[i] = slot;
        new_mask[i] = is_new;
        admitted = slot >= 0;
    }
    u64 adm = __ballot(admitted);
    u64 away = __ballot(pending && !admitted);
    if ((threadIdx.x & 63) == 0) {
        if (adm) atomicAdd(&stats[0], (u64)__popcll(adm));
        if (away) atomicAdd(&stats[1], (u64)__popcll(away));
    }
}

// ageing: every counter >> shift (arithmetic; shift >= 31 zeroes), four
// counters per thread through 16-byte loads and stores, scalar tail
__global__ void k_admit_age(int* __restrict__ sketch, long n, int shift) {
    long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long n4 = n >> 2;
    if (q < n4) {
        int4 v = reinterpret_cast<int4*>(sketch)[q];
        if (shift >= 31) v = make_int4(0, 0, 0, 0);
        else { v.x >>= shift; v.y >>= shift; v.z >>= shift; v.w >>= shift; }
        reinterpret_cast<int4*>(sketch)[q] = v;
    }
    long t = (n4 << 2) + q;
    if (q < 3 && t < n) sketch[t] = shift >= 31 ? 0 : sketch[t] >> shift;
}

__global__ void k_ht_rehash(const u64* __restrict__ tk_old,
                            const int* __restrict__ tv_old, long cap_old,
                            u64* __restrict__ tk_new, int* __restrict__ tv_new,
                            long mask_new) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap_old) return;
    u64 k = tk_old[i];
    if (k == EMPTY) return;
    u64 h = splitmix64(k) & (u64)mask_new;
    for (long p = 0; p <= mask_new; ++p) {  // bounded (new table is larger)
        u64 prev = atomicCAS(&tk_new[h], EMPTY, k);
        if (prev == EMPTY) { tv_new[h] = tv_old[i]; return; }
        h = (h + 1) & (u64)mask_new;
    }
}

// ------------------------------------------------------ array-table touch
// keys unique within a call; computes local slots (key / shard_num, the
// reference's layout EmbeddingShardFile.h:23-25), marks rows live and
// reports which were new.

__global__ void k_array_touch(unsigned char* __restrict__ valid,
                              const i64* __restrict__ keys, long n,
                              long shard_num, long cap,
                              i64* __restrict__ slots,
                              unsigned char* __restrict__ new_mask,
                              const int* __restrict__ u_dev) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (u_dev && i >= *u_dev) { slots[i] = -1; new_mask[i] = 0; return; }
    if (keys[i] < 0) {  // invalid for a bounded vocabulary; C++ trunc
        slots[i] = -1;  // division would silently map -1 to slot 0
        new_mask[i] = 0;
        return;
    }
    i64 s = keys[i] / shard_num;
    if (s < 0 || s >= cap) s = -1;  // guarded; host validates separately
    slots[i] = s;
    if (s < 0) { new_mask[i] = 0; return; }
    unsigned char was = valid[s];
    valid[s] = 1;
    new_mask[i] = !was;
}

// -------------------------------------------------- gather + lazy row init
// One G-lane group per row; new rows are initialized in the miss path
// (weights from the deterministic initializer, optimizer state copied from
// the host-prepared state_init_row) and simultaneously returned.

// When ``inverse`` is given the kernel iterates the FULL (duplicated)
// element list and fuses the scatter-to-duplicates (the reference's client
// response scatter, EmbeddingPullOperator.cpp:229-249) into the gather: all
// duplicates of a new key recompute the same deterministic init value, so
// the racy-looking table writes are benign (same bytes).
// GI_ILP elements per G-lane group with the index chain
// (inverse -> slot -> mask/key) preloaded for all of them before any row
// copy: the one-element version was 76% SQ_WAIT_ANY (each group parked on
// its own dependent gather chain).
#define GI_ILP 4
template <int G>
__global__ void k_gather_init(float* __restrict__ weights,
                              float* __restrict__ state,
                              long dim, long sd,
                              const i64* __restrict__ slots,
                              const unsigned char* __restrict__ new_mask,
                              const i64* __restrict__ keys, long n,
                              const i64* __restrict__ inverse,
                              float* __restrict__ out,
                              int init_cat, float p0, float p1, float p2,
                              u64 seed,
                              const float* __restrict__ state_init_row,
                              const int* __restrict__ u_dev) {
    const long stride = ((long)gridDim.x * blockDim.x) / G;
    long g0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int lane = threadIdx.x % G;
    const int live = u_dev ? *u_dev : 0;

    long uid[GI_ILP];
    i64 slot[GI_ILP];
    unsigned char nm[GI_ILP];
    u64 key[GI_ILP];
    #pragma unroll
    for (int t = 0; t < GI_ILP; ++t) {
        long g = g0 + t * stride;
        bool act = g < n && !(!inverse && u_dev && g >= live);
        uid[t] = act ? (inverse ? inverse[g] : g) : -1;
    }
    #pragma unroll
    for (int t = 0; t < GI_ILP; ++t)
        slot[t] = (uid[t] >= 0) ? slots[uid[t]] : -1;
    #pragma unroll
    for (int t = 0; t < GI_ILP; ++t) {
        nm[t] = (uid[t] >= 0 && new_mask) ? new_mask[uid[t]] : 0;
        key[t] = (uid[t] >= 0 && nm[t]) ? (u64)keys[uid[t]] : 0;
    }
    #pragma unroll
    for (int t = 0; t < GI_ILP; ++t) {
        long g = g0 + t * stride;
        if (uid[t] < 0)
            continue;
        if (slot[t] < 0) {  // read-only miss: zeros out
            if (out)
                for (long j = lane; j < dim; j += G) out[g * dim + j] = 0.0f;
            continue;
        }
        float* wrow = weights + (u64)slot[t] * dim;
        if (nm[t]) {
            for (long j = lane; j < dim; j += G) {
                float v = init_value(init_cat, p0, p1, p2, seed, key[t],
                                     (u64)j);
                wrow[j] = v;
                if (out) out[g * dim + j] = v;
            }
            if (sd > 0) {
                float* srow = state + (u64)slot[t] * sd;
                for (long j = lane; j < sd; j += G)
                    srow[j] = state_init_row[j];
            }
        } else if (out) {
            for (long j = lane; j < dim; j += G)
                out[g * dim + j] = wrow[j];
        }
    }
}

// ------------------------------- inverse + index filing + gather, one launch
// k_unique_inverse and k_gather_init are one dependent chain (slot_of -> tv
// -> slots -> new_mask -> row) cut by a launch and a round trip of
// ``inverse`` through memory; k_pull_merged walks it in one kernel, after
// the dedup form that stops at k_unique_assign. A G-lane group per element,
// GI_ILP elements in flight, as k_gather_init:
//   - the group resolves slot_of[g] -> tv[s] (the uid) with the encodings of
//     k_unique_inverse: -1 = the assign kernel stored inverse[g] itself,
//     <= -2 = the duplicate of such an element, which reads the winner's;
//   - lane 0 stores inverse[g] and perm[toff[s] + rank[g]] = g: stores only,
//     nothing waits for them;
//   - the element's key is its own input (keys[g] + foff[g % F]), not
//     unique_keys[uid];
//   - the table slot is a policy. SlotArray: straight from the own key
//     (array_slot, the guards of k_array_touch), so the row load does not
//     wait for new_mask[uid] and is discarded for a new row. SlotMap: through
//     slots[uid] (hash tables, after k_ht_lookup);
//   - then k_gather_init's body: a new row is initialised by every duplicate
//     with the same deterministic bytes, state rows from state_init_row,
//     ``out`` optional, slot < 0 reads as zeros.
// A uid outside [0, min(*u_dev, n)) (only an inconsistent scratch table can
// give one) is dropped: nothing is read or written for it. SlotArray also
// writes the tail of slots / new_mask at and beyond *u_dev (-1 and 0), which
// k_array_touch defined and the touch inside k_unique_assign cannot.
struct SlotArray {
    long shard_num, cap;
    i64* slots_tail;               // [n] tail written here
    unsigned char* mask_tail;
    static constexpr bool kTail = true;
    __device__ __forceinline__ i64 of(i64 key, long) const {
        return array_slot(key, shard_num, cap);
    }
};
struct SlotMap {
    const i64* slots;              // [n] per uid
    static constexpr bool kTail = false;
    __device__ __forceinline__ i64 of(i64, long uid) const {
        return slots[uid];
    }
};

template <int G, typename Slot>
__global__ void k_pull_merged(float* __restrict__ weights,
                              float* __restrict__ state, long dim, long sd,
                              const i64* __restrict__ keys,
                              const i64* __restrict__ foff, int F, long n,
                              const int* __restrict__ slot_of,
                              const int* __restrict__ tv,
                              const int* __restrict__ toff,
                              const int* __restrict__ rank,
                              i64* __restrict__ inverse,
                              int* __restrict__ perm,
                              const unsigned char* __restrict__ new_mask,
                              Slot sp, float* __restrict__ out,
                              int init_cat, float p0, float p1, float p2,
                              u64 seed,
                              const float* __restrict__ state_init_row,
                              const int* __restrict__ u_dev) {
    const long nthreads = (long)gridDim.x * blockDim.x;
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = nthreads / G;
    const long g0 = tid / G;
    const int lane = threadIdx.x % G;
    long live = *u_dev;
    live = live < 0 ? 0 : (live > n ? n : live);
    if constexpr (Slot::kTail) {
        for (long i = live + tid; i < n; i += nthreads) {
            sp.slots_tail[i] = -1;
            sp.mask_tail[i] = 0;
        }
    }

    int s[GI_ILP];
    i64 key[GI_ILP];
    #pragma unroll
    for (int t = 0; t < GI_ILP; ++t) {
        long g = g0 + t * stride;
        s[t] = 0;
        key[t] = 0;
        if (g < n) {
            s[t] = slot_of[g];
            key[t] = keys[g];
            if (foff) key[t] += foff[(int)g % F];
        }
    }
    long uid[GI_ILP];
    int o[GI_ILP], r[GI_ILP];
    #pragma unroll
    for (int t = 0; t < GI_ILP; ++t) {
        long g = g0 + t * stride;
        uid[t] = -1;
        o[t] = 0;
        r[t] = 0;
        if (g >= n) continue;
        if (s[t] >= 0) {
            uid[t] = tv[s[t]];
            o[t] = toff[s[t]];
            r[t] = rank[g];
        } else if (s[t] == -1) {
            uid[t] = inverse[g];
        } else {
            long wnr = -2 - (long)s[t];
            uid[t] = wnr < n ? inverse[wnr] : -1;
        }
    }
    i64 slot[GI_ILP];
    unsigned char nm[GI_ILP];
    #pragma unroll
    for (int t = 0; t < GI_ILP; ++t) {
        long g = g0 + t * stride;
        if (uid[t] >= live) uid[t] = -1;
        if (uid[t] < 0) { slot[t] = -1; nm[t] = 0; continue; }
        if (lane == 0) {
            if (s[t] != -1) inverse[g] = (i64)uid[t];
            long p = (long)o[t] + r[t];
            if (s[t] >= 0 && p >= 0 && p < n) perm[p] = (int)g;
        }
        slot[t] = sp.of(key[t], uid[t]);
        nm[t] = new_mask[uid[t]];
    }
    #pragma unroll
    for (int t = 0; t < GI_ILP; ++t) {
        long g = g0 + t * stride;
        if (uid[t] < 0)
            continue;
        if (slot[t] < 0) {  // no row: zeros out
            if (out)
                for (long j = lane; j < dim; j += G) out[g * dim + j] = 0.0f;
            continue;
        }
        float* wrow = weights + (u64)slot[t] * dim;
        if (nm[t]) {
            for (long j = lane; j < dim; j += G) {
                float v = init_value(init_cat, p0, p1, p2, seed, (u64)key[t],
                                     (u64)j);
                wrow[j] = v;
                if (out) out[g * dim + j] = v;
            }
            if (sd > 0) {
                float* srow = state + (u64)slot[t] * sd;
                for (long j = lane; j < sd; j += G)
                    srow[j] = state_init_row[j];
            }
        } else if (out) {
            for (long j = lane; j < dim; j += G)
                out[g * dim + j] = wrow[j];
        }
    }
}

// ------------------------------------------------- segment-pooled gather
// Multi-hot bags (the reference's ragged sparse_read, exb.py:315-321, plus
// the sum/mean/sqrtn combiner CTR models apply on top): bag b pools the
// rows of values[offsets[b] .. offsets[b+1]). Pooling inside the gather
// means no [nnz, dim] tensor is ever written.

enum { POOL_SUM = 0, POOL_MEAN = 1, POOL_SQRTN = 2 };

// every offsets value is clamped before use: a malformed offsets tensor
// can give wrong bags but never an out-of-range read
DEV long pool_clamp(i64 v, long nnz) {
    return v < 0 ? 0 : (v > (i64)nnz ? nnz : (long)v);
}

DEV float pool_scale(int mode, long len) {
    if (len <= 0) return 0.0f;
    if (mode == POOL_MEAN) return 1.0f / (float)len;
    if (mode == POOL_SQRTN) return 1.0f / sqrtf((float)len);
    return 1.0f;
}

// combiner scale of a weighted bag from its denominator (sum of w for mean,
// sum of w^2 for sqrtn): TF's embedding_lookup_sparse with divide_no_nan
DEV float pool_wscale(int mode, float den) {
    if (mode == POOL_SUM) return 1.0f;
    if (den == 0.0f) return 0.0f;
    return mode == POOL_MEAN ? 1.0f / den : 1.0f / sqrtf(den);
}

// One G-lane group per bag, lanes over columns, PF_CF column fragments per
// lane held in registers (dim <= PF_CF*G in one pass, wider rows loop).
// The index chain (inverse -> map -> row) is resolved lane-parallel: lane l
// of the group resolves element j0+l, so G elements cost ONE pass of the
// dependent chain (two coalesced-index loads), and the next G elements'
// chain is issued before this chunk's row reads. Rows are then broadcast
// through __shfl and read PF_ILP at a time — the latency plan of
// k_gather_init, which matters most for the long bags of a long-tailed
// length distribution (one group walks its whole bag). Rows are added in
// element order with plain adds, so the result is bitwise reproducible
// (no atomics).
// ``inverse`` null = identity; ``map`` null = inverse indexes rows
// directly; a mapped row < 0 (or out of range) contributes zero.
// ``bag_of`` (optional, [nnz]) receives each element's bag, -1 for the
// tail at or beyond offsets[B] — the backward reduce reads it.
// PF_CF * PF_ILP row values are in flight per lane; the launcher trades
// column fragments for elements so narrow rows get the deeper element
// preload (a 16-element chunk of a dim <= 16 bag is ONE load latency).
//
// WEIGHTED = true is the per-sample-weight variant: lane l loads the weight
// of element j0+l beside its row index, the weight is broadcast with the
// same __shfl as the row, the row is multiplied in before the add, and the
// denominator (sum of w / sum of w^2) is accumulated in the same fixed
// element order, so the result stays bitwise reproducible. Weights at or
// beyond offsets[B] are never read. The bag's combiner scale goes to
// ``bag_scale`` [B] for the backward. WEIGHTED = false compiles to the
// plain kernel.

// row of ``rows`` that element j reads, -1 = contributes zero (j outside
// the bag, an index outside its table, or a mapped miss)
template <typename MapT>
DEV long pool_row(long j, long e, const i64* __restrict__ inverse,
                  const MapT* __restrict__ map, long nidx, long R) {
    if (j >= e) return -1;
    long uid = inverse ? (long)inverse[j] : j;
    if (uid < 0 || uid >= nidx) return -1;
    long row = map ? (long)map[uid] : uid;
    return (row >= 0 && row < R) ? row : -1;
}

// Resolver policies of pool_accumulate: element j of a bag ending at e ->
// row of ``rows``, -1 = zero row. PoolChain is the training chain above.
template <typename MapT>
struct PoolChain {
    const i64* __restrict__ inverse;
    const MapT* __restrict__ map;
    long nidx, R;
    __device__ __forceinline__ long operator()(long j, long e) const {
        return pool_row(j, e, inverse, map, nidx, R);
    }
};

// Read-only key -> row resolution inside the gather (k_pool_lookup): the
// insert == 0 probe of k_ht_lookup — same hash, EMPTY rule and probe bound,
// no CAS, nothing written. Key -1 and a tv value outside [0, R) are misses.
struct PoolHashKeys {
    const i64* __restrict__ values;
    const u64* __restrict__ tk;
    const int* __restrict__ tv;
    long mask, R;
    __device__ __forceinline__ long operator()(long j, long e) const {
        if (j >= e) return -1;
        const u64 k = (u64)values[j];
        if (k == EMPTY) return -1;
        u64 h = splitmix64(k) & (u64)mask;
        for (long p = 0; p <= mask; ++p) {
            const u64 cur = tk[h];
            if (cur == k) {
                const long row = (long)tv[h];
                return (row >= 0 && row < R) ? row : -1;
            }
            if (cur == EMPTY) return -1;
            h = (h + 1) & (u64)mask;
        }
        return -1;
    }
};

// array table: slot = key / shard_num (k_array_touch's layout), a hit only
// for 0 <= key, slot < cap and a live row
struct PoolArrayKeys {
    const i64* __restrict__ values;
    const unsigned char* __restrict__ valid;
    long shard_num, cap, R;
    __device__ __forceinline__ long operator()(long j, long e) const {
        if (j >= e) return -1;
        const i64 k = values[j];
        if (k < 0) return -1;
        const i64 slot = k / shard_num;
        if (slot >= cap || slot >= R) return -1;
        return valid[slot] ? (long)slot : -1;
    }
};

// The accumulate body shared by k_pool_fwd and k_pool_lookup: the G-lane
// group of ``lane`` pools elements [s, e) into out[b], resolving element
// rows through ``resolve``. ``bag_scale`` (WEIGHTED only) may be null.
template <int G, int PF_CF, int PF_ILP, bool WEIGHTED, typename Resolve>
DEV void pool_accumulate(const float* __restrict__ rows, long dim, long s,
                         long e, long b, int lane, int mode,
                         const float* __restrict__ weights,
                         float* __restrict__ out,
                         float* __restrict__ bag_scale,
                         const Resolve& resolve) {
    float scale = 1.0f;
    if constexpr (!WEIGHTED) scale = pool_scale(mode, e - s);
    for (long c0 = 0; c0 < dim; c0 += (long)G * PF_CF) {
        float acc[PF_CF];
        #pragma unroll
        for (int k = 0; k < PF_CF; ++k) acc[k] = 0.0f;
        long myrow = resolve(s + lane, e);
        // WEIGHTED only: this lane's element weight and the bag's
        // denominator (every column pass recomputes the same value)
        float myw = 0.0f, den = 0.0f;
        if constexpr (WEIGHTED)
            if (s + lane < e) myw = weights[s + lane];
        for (long j0 = s; j0 < e; j0 += G) {
            const long nextrow = resolve(j0 + G + lane, e);
            float nextw = 0.0f;
            if constexpr (WEIGHTED)
                if (j0 + G + lane < e) nextw = weights[j0 + G + lane];
            const int cnt = (int)((e - j0) < G ? (e - j0) : G);
            for (int t0 = 0; t0 < cnt; t0 += PF_ILP) {
                long row[PF_ILP];
                float wt[WEIGHTED ? PF_ILP : 1];
                #pragma unroll
                for (int t = 0; t < PF_ILP; ++t) {  // t0 + t < G always
                    row[t] = __shfl(myrow, t0 + t, G);
                    if constexpr (WEIGHTED) wt[t] = __shfl(myw, t0 + t, G);
                }
                float v[PF_ILP][PF_CF];
                #pragma unroll
                for (int t = 0; t < PF_ILP; ++t) {
                    #pragma unroll
                    for (int k = 0; k < PF_CF; ++k) {
                        long c = c0 + lane + (long)k * G;
                        v[t][k] = (row[t] >= 0 && c < dim)
                                      ? rows[(u64)row[t] * dim + c] : 0.0f;
                    }
                }
                #pragma unroll
                for (int t = 0; t < PF_ILP; ++t) {
                    if (t0 + t < cnt) {
                        if constexpr (WEIGHTED) {
                            #pragma unroll
                            for (int k = 0; k < PF_CF; ++k)
                                acc[k] += wt[t] * v[t][k];
                            den += (mode == POOL_SQRTN) ? wt[t] * wt[t]
                                                        : wt[t];
                        } else {
                            #pragma unroll
                            for (int k = 0; k < PF_CF; ++k) acc[k] += v[t][k];
                        }
                    }
                }
            }
            myrow = nextrow;
            if constexpr (WEIGHTED) myw = nextw;
        }
        if constexpr (WEIGHTED) {
            scale = pool_wscale(mode, den);
            if (bag_scale && c0 == 0 && lane == 0) bag_scale[b] = scale;
        }
        #pragma unroll
        for (int k = 0; k < PF_CF; ++k) {
            long c = c0 + lane + (long)k * G;
            if (c < dim) out[(u64)b * dim + c] = acc[k] * scale;
        }
    }
}

template <int G, int PF_CF, int PF_ILP, typename MapT,
          bool WEIGHTED = false>
__global__ void k_pool_fwd(const float* __restrict__ rows, long R, long dim,
                           const i64* __restrict__ inverse, long nnz,
                           const MapT* __restrict__ map, long u,
                           const i64* __restrict__ offsets, long B, int mode,
                           float* __restrict__ out,
                           int* __restrict__ bag_of,
                           const float* __restrict__ weights,
                           float* __restrict__ bag_scale) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (bag_of) {
        const long nthreads = (long)gridDim.x * blockDim.x;
        for (long j = pool_clamp(offsets[B], nnz) + tid; j < nnz;
             j += nthreads)
            bag_of[j] = -1;
    }
    const long b = tid / G;
    const int lane = threadIdx.x % G;
    if (b >= B) return;
    const long s = pool_clamp(offsets[b], nnz);
    long e = pool_clamp(offsets[b + 1], nnz);
    if (e < s) e = s;
    const long nidx = map ? u : R;   // valid range of an inverse value
    const PoolChain<MapT> resolve{inverse, map, nidx, R};
    pool_accumulate<G, PF_CF, PF_ILP, WEIGHTED>(rows, dim, s, e, b, lane,
                                                 mode, weights, out,
                                                 bag_scale, resolve);
    if (bag_of)
        for (long j = s + lane; j < e; j += G) bag_of[j] = (int)b;
}

// Read-only pooled lookup (inference / serving): values [nnz] int64 keys
// and offsets [B+1] straight to out [B, dim]. The latency plan, the scale
// (taken from offsets only, so a missed element still counts toward the
// bag length) and the element-order plain adds are k_pool_fwd's — the two
// kernels share pool_accumulate — but "resolve" is key -> row inside the
// kernel (PoolHashKeys / PoolArrayKeys): no unique, no inverse, no slots
// tensor, and the table is only read. A miss adds a zero row; an empty bag
// or one with offsets[b+1] < offsets[b] is zeros.
template <int G, int PF_CF, int PF_ILP, bool WEIGHTED, typename Resolve>
__global__ void k_pool_lookup(const float* __restrict__ rows, long dim,
                              long nnz, const i64* __restrict__ offsets,
                              long B, int mode,
                              const float* __restrict__ weights,
                              float* __restrict__ out, Resolve resolve) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long b = tid / G;
    const int lane = threadIdx.x % G;
    if (b >= B) return;
    const long s = pool_clamp(offsets[b], nnz);
    long e = pool_clamp(offsets[b + 1], nnz);
    if (e < s) e = s;
    pool_accumulate<G, PF_CF, PF_ILP, WEIGHTED>(rows, dim, s, e, b, lane,
                                                 mode, weights, out, nullptr,
                                                 resolve);
}

// ------------------------------------------------- quantized serving tables
// A read-only table stored as packed rows: a uint8 slab [R, stride] with
// stride % 4 == 0, every row a whole number of dwords (docs/kernels.md has
// the byte layout; ops/dispatch.py quantize_rows / dequantize_rows is the
// same definition in torch and the oracle of everything below).
//   QF_INT8: dim unsigned codes, zero pad to a dword, fp32 scale, fp32 lo;
//            x^ = lo + scale * (float)code (one multiply, then one add)
//   QF_FP16: dim IEEE halves, zero pad to a dword; x^ = (float)half
// All arithmetic is fp32 op for op (-ffp-contract=off, correctly rounded
// division), so a slab written here is byte-identical to the oracle's and
// a lookup is bit-identical to dequantize-then-pool on the CPU.
//
// The lookups below carry their own accumulate body instead of sharing
// pool_accumulate through a row-format policy: a lane's fragment here is a
// dword of 4 (or 2) consecutive columns with a per-row scale/lo, not one
// fp32 column, so the accumulator shape, the column index and the store
// all differ, and keeping the bodies apart leaves the fp32 instantiations
// of k_pool_fwd / k_pool_lookup untouched. What defines the result is
// shared: the resolvers, pool_clamp, pool_scale / pool_wscale, the miss and
// empty-bag rules and the element-order plain adds.

enum { QF_INT8 = 0, QF_FP16 = 1 };

template <int FMT> struct QFmt;
template <> struct QFmt<QF_INT8> {
    static constexpr int CPD = 4;    // columns per dword
    static __host__ __device__ long code_dwords(long dim) {
        return (dim + 3) / 4;
    }
    static __host__ __device__ long stride(long dim) {
        return 4 * code_dwords(dim) + 8;
    }
};
template <> struct QFmt<QF_FP16> {
    static constexpr int CPD = 2;
    static __host__ __device__ long code_dwords(long dim) {
        return (dim + 1) / 2;
    }
    static __host__ __device__ long stride(long dim) {
        return 4 * code_dwords(dim);
    }
};

DEV unsigned int q_half_bits(float x) {
    return (unsigned int)__builtin_bit_cast(unsigned short, (_Float16)x);
}
DEV float q_half_value(unsigned int bits) {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)bits);
}

// columns [CPD * d, CPD * d + CPD) of a row from its dword ``word``
template <int FMT>
DEV void q_unpack(unsigned int word, float scale, float lo,
                  float (&x)[QFmt<FMT>::CPD]) {
    if constexpr (FMT == QF_INT8) {
        #pragma unroll
        for (int i = 0; i < 4; ++i)
            x[i] = lo + scale * (float)((word >> (8 * i)) & 0xffu);
    } else {
        x[0] = q_half_value(word & 0xffffu);
        x[1] = q_half_value(word >> 16);
    }
}

// One G-lane group per source row: a shuffle min/max tree over the row
// (int8), then every lane packs whole dwords — four codes or two halves,
// pad columns as zero bytes — and lane 0 adds the scale and lo dwords.
// Source row i goes to slab row slots[i]; a slot outside [0, R) is
// skipped. Two rows of one call naming the same slot race (caller's error).
// lo is stored as min(row) + 0.0f, which turns a -0.0 minimum into +0.0:
// which zero a min over both signs returns depends on the reduction order,
// and x^ is the same for either.
template <int FMT, int G>
__global__ void k_quantize_rows(const float* __restrict__ w, long n,
                                long dim, const i64* __restrict__ slots,
                                unsigned int* __restrict__ slab, long R) {
    const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int lane = threadIdx.x % G;
    if (i >= n) return;                 // whole groups leave together
    const i64 slot = slots[i];
    if (slot < 0 || slot >= (i64)R) return;
    const float* __restrict__ src = w + (u64)i * dim;
    const long ndw = QFmt<FMT>::code_dwords(dim);
    unsigned int* __restrict__ dst =
        slab + (u64)slot * (QFmt<FMT>::stride(dim) / 4);
    float lo = 0.0f, scale = 0.0f;
    if constexpr (FMT == QF_INT8) {
        float mn = src[0], mx = src[0];
        for (long c = lane; c < dim; c += G) {
            const float v = src[c];
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
        #pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, o, G));
            mx = fmaxf(mx, __shfl_xor(mx, o, G));
        }
        lo = mn + 0.0f;
        scale = (mx - lo) / 255.0f;
        if (scale < 1.17549435e-38f) scale = 0.0f;   // FLT_MIN
    }
    for (long d = lane; d < ndw; d += G) {
        unsigned int word = 0;
        #pragma unroll
        for (int k = 0; k < QFmt<FMT>::CPD; ++k) {
            const long c = d * QFmt<FMT>::CPD + k;
            if (c >= dim) continue;
            unsigned int bits;
            if constexpr (FMT == QF_INT8) {
                float q = 0.0f;
                if (scale != 0.0f) {
                    q = rintf((src[c] - lo) / scale);
                    q = fminf(fmaxf(q, 0.0f), 255.0f);
                }
                bits = (unsigned int)q;
                word |= bits << (8 * k);
            } else {
                bits = q_half_bits(src[c]);
                word |= bits << (16 * k);
            }
        }
        dst[d] = word;
    }
    if constexpr (FMT == QF_INT8) {
        if (lane == 0) {
            dst[ndw] = __float_as_uint(scale);
            dst[ndw + 1] = __float_as_uint(lo);
        }
    }
}

// The accumulate body of k_pool_lookup_q: pool_accumulate's plan — lane l
// resolves element j0+l, the next chunk's probes are issued before this
// chunk's row reads, rows broadcast through __shfl and read PF_ILP at a
// time — over packed rows. A lane owns dword lane + k*G of a row (PF_CF of
// them), i.e. CPD consecutive columns per fragment, loaded as one dword;
// the row's scale and lo are two more dword loads per row, the same
// address in every lane. ``sdw`` is the row stride in dwords.
template <int FMT, int G, int PF_CF, int PF_ILP, bool WEIGHTED,
          typename Resolve>
DEV void pool_accumulate_q(const unsigned int* __restrict__ slab, long dim,
                           long s, long e, long b, int lane, int mode,
                           const float* __restrict__ weights,
                           float* __restrict__ out, const Resolve& resolve) {
    constexpr int CPD = QFmt<FMT>::CPD;
    const long ndw = QFmt<FMT>::code_dwords(dim);
    const long sdw = QFmt<FMT>::stride(dim) / 4;
    float scale = 1.0f;
    if constexpr (!WEIGHTED) scale = pool_scale(mode, e - s);
    for (long d0 = 0; d0 < ndw; d0 += (long)G * PF_CF) {
        float acc[PF_CF][CPD];
        #pragma unroll
        for (int k = 0; k < PF_CF; ++k)
            #pragma unroll
            for (int i = 0; i < CPD; ++i) acc[k][i] = 0.0f;
        long myrow = resolve(s + lane, e);
        float myw = 0.0f, den = 0.0f;
        if constexpr (WEIGHTED)
            if (s + lane < e) myw = weights[s + lane];
        for (long j0 = s; j0 < e; j0 += G) {
            const long nextrow = resolve(j0 + G + lane, e);
            float nextw = 0.0f;
            if constexpr (WEIGHTED)
                if (j0 + G + lane < e) nextw = weights[j0 + G + lane];
            const int cnt = (int)((e - j0) < G ? (e - j0) : G);
            for (int t0 = 0; t0 < cnt; t0 += PF_ILP) {
                long row[PF_ILP];
                float wt[WEIGHTED ? PF_ILP : 1];
                #pragma unroll
                for (int t = 0; t < PF_ILP; ++t) {  // t0 + t < G always
                    row[t] = __shfl(myrow, t0 + t, G);
                    if constexpr (WEIGHTED) wt[t] = __shfl(myw, t0 + t, G);
                }
                // Every load is unconditional, from a clamped in-range
                // address (a miss reads row 0, a lane past the row its last
                // dword; the launcher never starts this kernel with R == 0),
                // and what must not count is zeroed afterwards: word 0,
                // scale 0, lo 0 -> x^ = 0. Loads under a per-row branch
                // made the compiler wait for each row's scale / lo before
                // issuing the next row's loads (PF_ILP serial round trips
                // instead of one).
                unsigned int word[PF_ILP][PF_CF];
                float rs[PF_ILP], rl[PF_ILP];
                #pragma unroll
                for (int t = 0; t < PF_ILP; ++t) {
                    const unsigned int* __restrict__ r =
                        slab + (u64)(row[t] >= 0 ? row[t] : 0) * sdw;
                    #pragma unroll
                    for (int k = 0; k < PF_CF; ++k) {
                        const long d = d0 + lane + (long)k * G;
                        word[t][k] = r[d < ndw ? d : ndw - 1];
                    }
                    rs[t] = 0.0f;
                    rl[t] = 0.0f;
                    if constexpr (FMT == QF_INT8) {
                        rs[t] = __uint_as_float(r[ndw]);
                        rl[t] = __uint_as_float(r[ndw + 1]);
                    }
                }
                #pragma unroll
                for (int t = 0; t < PF_ILP; ++t) {
                    const bool hit = row[t] >= 0;
                    #pragma unroll
                    for (int k = 0; k < PF_CF; ++k) {
                        const long d = d0 + lane + (long)k * G;
                        word[t][k] = (hit && d < ndw) ? word[t][k] : 0u;
                    }
                    rs[t] = hit ? rs[t] : 0.0f;
                    rl[t] = hit ? rl[t] : 0.0f;
                }
                #pragma unroll
                for (int t = 0; t < PF_ILP; ++t) {
                    if (t0 + t < cnt) {
                        #pragma unroll
                        for (int k = 0; k < PF_CF; ++k) {
                            float x[CPD];
                            q_unpack<FMT>(word[t][k], rs[t], rl[t], x);
                            #pragma unroll
                            for (int i = 0; i < CPD; ++i) {
                                if constexpr (WEIGHTED)
                                    acc[k][i] += wt[t] * x[i];
                                else
                                    acc[k][i] += x[i];
                            }
                        }
                        if constexpr (WEIGHTED)
                            den += (mode == POOL_SQRTN) ? wt[t] * wt[t]
                                                        : wt[t];
                    }
                }
            }
            myrow = nextrow;
            if constexpr (WEIGHTED) myw = nextw;
        }
        if constexpr (WEIGHTED) scale = pool_wscale(mode, den);
        #pragma unroll
        for (int k = 0; k < PF_CF; ++k) {
            const long c = (d0 + lane + (long)k * G) * CPD;
            #pragma unroll
            for (int i = 0; i < CPD; ++i)
                if (c + i < dim) out[(u64)b * dim + c + i] = acc[k][i] * scale;
        }
    }
}

// Read-only pooled lookup over a packed slab: k_pool_lookup with the row
// read replaced by a dequantizing dword read. values [nnz] keys and
// offsets [B+1] -> out [B, dim] fp32, one launch, the table only read.
template <int FMT, int G, int PF_CF, int PF_ILP, bool WEIGHTED,
          typename Resolve>
__global__ void k_pool_lookup_q(const unsigned int* __restrict__ slab,
                                long dim, long nnz,
                                const i64* __restrict__ offsets, long B,
                                int mode, const float* __restrict__ weights,
                                float* __restrict__ out, Resolve resolve) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long b = tid / G;
    const int lane = threadIdx.x % G;
    if (b >= B) return;
    const long s = pool_clamp(offsets[b], nnz);
    long e = pool_clamp(offsets[b + 1], nnz);
    if (e < s) e = s;
    pool_accumulate_q<FMT, G, PF_CF, PF_ILP, WEIGHTED>(
        slab, dim, s, e, b, lane, mode, weights, out, resolve);
}

// The flat read (pull_weights): keys [n] -> out [n, dim] fp32, one G-lane
// group per key. Every lane of the group runs the same resolve (one
// address per probe across the group), then the lanes dequantize the row's
// dwords; a miss writes zeros.
template <int FMT, int G, typename Resolve>
__global__ void k_gather_lookup_q(const unsigned int* __restrict__ slab,
                                  long dim, long n, float* __restrict__ out,
                                  Resolve resolve) {
    constexpr int CPD = QFmt<FMT>::CPD;
    const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int lane = threadIdx.x % G;
    if (i >= n) return;
    const long row = resolve(i, n);
    const long ndw = QFmt<FMT>::code_dwords(dim);
    const unsigned int* __restrict__ r =
        slab + (u64)(row >= 0 ? row : 0) * (QFmt<FMT>::stride(dim) / 4);
    // unconditional loads (a miss reads row 0; never launched with R == 0),
    // zeroed afterwards, so scale / lo and the codes are one round trip
    float rs = 0.0f, rl = 0.0f;
    if constexpr (FMT == QF_INT8) {
        rs = __uint_as_float(r[ndw]);
        rl = __uint_as_float(r[ndw + 1]);
        if (row < 0) rs = rl = 0.0f;
    }
    for (long d = lane; d < ndw; d += G) {
        float x[CPD];
        const unsigned int word = r[d];
        q_unpack<FMT>(row >= 0 ? word : 0u, rs, rl, x);
        #pragma unroll
        for (int k = 0; k < CPD; ++k) {
            const long c = d * CPD + k;
            if (c < dim) out[(u64)i * dim + c] = x[k];
        }
    }
}

// -------------------------------------------------------- reduce-by-inverse
// Hot rows (small-vocab fields) make direct global atomics serialize; for
// dim <= 32 gradients+counts are pre-aggregated in an LDS hash per block
// (one global atomic per distinct uid per block), fused with the counts.

// G-lane groups, lane j covering columns j, j+G, ...: the gradient row read
// is one coalesced segment and each element costs ceil(dim/G) LDS atomics
// per lane IN PARALLEL across lanes (the previous one-thread-per-element
// version did `dim` serial LDS atomics per element with strided reads —
// 112us avg in the DeepFM profile; this shape removes both problems).
// Lane 0 of the group probes the LDS hash and broadcasts the slot.
//
// BAG = true is the pooled (multi-hot) backward: ``grads`` is then the
// [B, dim] gradient of the pooled output and element e reads row
// bag_of[e] of it, scaled by its bag's combiner scale — the [nnz, dim]
// expansion autograd would build is never materialised. Elements whose
// bag_of is outside [0, B) (the fixed-capacity tail) add neither gradient
// nor count. BAG = false compiles to the plain kernel.
//
// WEIGHTED (with BAG) is the per-sample-weight backward: element e's factor
// is w[e] * bag_scale[bag_of[e]] — the weight preloaded beside the bag, the
// scale fetched from the forward's ``bag_scale`` with the staged gradient
// fragment instead of recomputed from offsets. Counts do not depend on
// weights. The non-weighted instantiations are unchanged.

// row of the pooled gradient + scale for an element of bag ``bag``, or -1
// to skip it
DEV long reduce_src(int bag, long n, const i64* __restrict__ offsets,
                    long B, int mode, float& scale) {
    if (bag < 0 || bag >= B) return -1;
    if (mode != POOL_SUM)
        scale = pool_scale(mode, pool_clamp(offsets[bag + 1], n)
                                     - pool_clamp(offsets[bag], n));
    return bag;
}

// weighted form: the factor is w * bag_scale[bag]
DEV long reduce_src_w(int bag, long B, float w,
                      const float* __restrict__ bag_scale, float& scale) {
    if (bag < 0 || bag >= B) return -1;
    scale = w * bag_scale[bag];
    return bag;
}

template <int H, int G, int GF = 4, bool BAG = false, bool WEIGHTED = false>
__global__ void k_reduce_lds(const i64* __restrict__ inverse,
                             const float* __restrict__ grads,
                             long n, long dim,
                             float* __restrict__ ugrads,
                             u64* __restrict__ counts,
                             const int* __restrict__ bag_of,
                             const i64* __restrict__ offsets,
                             long B, int mode,
                             const float* __restrict__ weights,
                             const float* __restrict__ bag_scale) {
    static_assert(BAG || !WEIGHTED, "WEIGHTED is a sub-variant of BAG");
    extern __shared__ char smem[];
    int* luid = (int*)smem;
    int* lcnt = (int*)(smem + H * 4);
    float* lacc = (float*)(smem + H * 8);
    for (int t = threadIdx.x; t < H; t += blockDim.x) {
        luid[t] = -1;
        lcnt[t] = 0;
    }
    for (long t = threadIdx.x; t < (long)H * dim; t += blockDim.x)
        lacc[t] = 0.0f;
    __syncthreads();
    const int lane = threadIdx.x % G;
    const int group = threadIdx.x / G;
    const long base = (long)blockIdx.x * blockDim.x + group * G;
    // latency plan (PMC: 60% parked): preload every element's uid up front
    // (independent loads) and stage each element's gradient fragment one
    // iteration ahead of its LDS-accumulate, so a global load is always in
    // flight while the previous element's LDS atomics run.
    int uids[G];
    #pragma unroll
    for (int t = 0; t < G; ++t) {
        long e = base + t;
        uids[t] = (e < n) ? (int)inverse[e] : -1;
    }
    float gfrag[2][GF];  // up to GF grad values per lane (dim <= GF*G)
    const int nj = (int)((dim + G - 1) / G);
    // BAG only: every element's bag preloaded like its uid, then the row
    // of the pooled gradient (-1 = skip the element) and the combiner
    // scale of the two staged elements
    int bags[BAG ? G : 1];
    float wts[WEIGHTED ? G : 1];
    long gsrc[2] = {-1, -1};
    float gscale[2] = {1.0f, 1.0f};
    if constexpr (BAG) {
        #pragma unroll
        for (int t = 0; t < G; ++t) {
            long e = base + t;
            bags[t] = (e < n) ? bag_of[e] : -1;
            if constexpr (WEIGHTED) wts[t] = (e < n) ? weights[e] : 0.0f;
        }
        if constexpr (WEIGHTED)
            gsrc[0] = reduce_src_w(bags[0], B, wts[0], bag_scale, gscale[0]);
        else
            gsrc[0] = reduce_src(bags[0], n, offsets, B, mode, gscale[0]);
        #pragma unroll
        for (int j = 0; j < GF; ++j)
            gfrag[0][j] = (j < nj && gsrc[0] >= 0 && lane + j * G < dim)
                ? grads[(u64)gsrc[0] * dim + lane + j * G] : 0.0f;
    } else {
        #pragma unroll
        for (int j = 0; j < GF; ++j)
            gfrag[0][j] = (j < nj && base < n && lane + j * G < dim)
                              ? grads[(u64)base * dim + lane + j * G] : 0.0f;
    }
    for (int t = 0; t < G; ++t) {
        long e = base + t;
        if (e >= n) break;
        long en = base + t + 1;
        if constexpr (BAG) {
            if (t + 1 < G) {
                const int nb = (t + 1) & 1;
                if constexpr (WEIGHTED)
                    gsrc[nb] = reduce_src_w(bags[t + 1], B, wts[t + 1],
                                            bag_scale, gscale[nb]);
                else
                    gsrc[nb] = reduce_src(bags[t + 1], n, offsets, B, mode,
                                          gscale[nb]);
                #pragma unroll
                for (int j = 0; j < GF; ++j)
                    gfrag[nb][j] = (j < nj && gsrc[nb] >= 0
                                    && lane + j * G < dim)
                        ? grads[(u64)gsrc[nb] * dim + lane + j * G] : 0.0f;
            }
            if (gsrc[t & 1] < 0) continue;   // tail element: no-op
        } else if (en < n) {
            #pragma unroll
            for (int j = 0; j < GF; ++j)
                gfrag[(t + 1) & 1][j] = (j < nj && lane + j * G < dim)
                    ? grads[(u64)en * dim + lane + j * G] : 0.0f;
        }
        int uid = uids[t];
        int h = -1;
        if (lane == 0) {
            int hh = (int)(((unsigned)uid * 2654435761u) & (H - 1));
            for (int probes = 0; probes < H; ++probes) {
                int cur = atomicCAS(&luid[hh], -1, uid);
                if (cur == -1 || cur == uid) { h = hh; break; }
                hh = (hh + 1) & (H - 1);
            }
            if (h >= 0) atomicAdd(&lcnt[h], 1);
            else atomicAdd(&counts[uid], 1ull);
        }
        h = __shfl(h, (threadIdx.x & ~(G - 1)) % 64, 64);
        float* dstb = (h >= 0) ? (lacc + (u64)h * dim)
                               : (ugrads + (u64)uid * dim);
        #pragma unroll
        for (int j = 0; j < GF; ++j)
            if (j < nj && lane + j * G < dim)
                atomicAdd(&dstb[lane + j * G],
                          BAG ? gfrag[t & 1][j] * gscale[t & 1]
                              : gfrag[t & 1][j]);
    }
    __syncthreads();
    for (int h = group; h < H; h += (int)(blockDim.x / G)) {
        int uid = luid[h];
        if (uid < 0) continue;
        if (lane == 0) atomicAdd(&counts[uid], (u64)lcnt[h]);
        float* ug = ugrads + (u64)uid * dim;
        const float* acc = lacc + (u64)h * dim;
        for (long j = lane; j < dim; j += G) atomicAdd(&ug[j], acc[j]);
    }
}

template <bool BAG = false, bool WEIGHTED = false>
__global__ void k_reduce_grads(const i64* __restrict__ inverse,
                               const float* __restrict__ grads,
                               long n, long dim,
                               float* __restrict__ ugrads,
                               const int* __restrict__ bag_of,
                               const i64* __restrict__ offsets,
                               long B, int mode,
                               const float* __restrict__ weights,
                               const float* __restrict__ bag_scale) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * dim) return;
    long i = e / dim, j = e % dim;
    if (BAG) {
        float scale = 1.0f;
        long src;
        if constexpr (WEIGHTED)
            src = reduce_src_w(bag_of[i], B, weights[i], bag_scale, scale);
        else
            src = reduce_src(bag_of[i], n, offsets, B, mode, scale);
        if (src < 0) return;
        atomicAdd(&ugrads[inverse[i] * dim + j],
                  grads[(u64)src * dim + j] * scale);
    } else {
        atomicAdd(&ugrads[inverse[i] * dim + j], grads[e]);
    }
}

template <bool BAG = false>
__global__ void k_reduce_counts(const i64* __restrict__ inverse, long n,
                                u64* __restrict__ counts,
                                const int* __restrict__ bag_of, long B) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (BAG && (bag_of[i] < 0 || bag_of[i] >= B)) return;
    atomicAdd(&counts[inverse[i]], 1ull);
}

// ------------------------------------- segmented reduce (inverted index)
// The indexed dedup (k_unique_*<true>) files every element under its uid:
// uid's elements are perm[seg_off[uid] .. seg_off[uid] + seg_cnt[uid]), in
// arrival order, and long_list[0 .. *n_long) names the uids with more than
// SEG_T elements. The gradient rows are already in memory once ([n, dim],
// plain stores of the head backward), so the per-unique sums need no
// atomics, no zeroed scratch and no LDS hash: every output row and count is
// written exactly once with a plain store, rows at and beyond *u_dev as
// zeros with count 0 (what k_reduce_reset used to leave there). The sum
// order inside a list is arrival order, as it was with the atomics: not
// bitwise reproducible from run to run.
//
// One launch, two roles, chosen per block:
//   short (seg_cnt <= SEG_T): a G-lane group per uid, lanes over columns,
//     SR_ILP uids' dependent chains (seg -> perm -> row) in flight per
//     group, as k_gather_init does; the rest of a list in chunks of SR_ILP
//     rows.
//   long: a whole block per uid, a lane group per element and LR_ILP rows
//     in flight per group, so a list costs ceil(len / (block / G * LR_ILP))
//     rounds of independent loads (the next round's perm entries already
//     in flight); then a fixed-order reduction (shuffles
//     across the wave's groups, LDS across waves). The first ``long_blocks``
//     blocks walk long_list with a block stride: a static grid for capture.
//     They come first in the grid because the longest list is the kernel's
//     critical path.
// A uid is written by the role its CLAMPED count selects, so both roles
// decide from the same numbers.
//
// Guards: seg_off / seg_cnt are clamped into [0, n], every perm entry and
// every long_list entry is range-checked, *n_long and *u_dev are clamped.
// An inconsistent index (only the dedup's unreachable global-table overflow
// produces one) gives wrong sums, never an out-of-range access.
#define SR_ILP 4
#define LR_ILP 8
#define SEG_BLOCK 1024
#define SEG_LONG_BLOCKS 256
#define SEG_MAX_DIM 128   // widest rung of the launcher's ladder (G=64, CF=2)

DEV void seg_range(const int* __restrict__ seg_off,
                   const int* __restrict__ seg_cnt, long uid, long n,
                   int& off, int& cnt) {
    int o = seg_off[uid], c = seg_cnt[uid];
    o = o < 0 ? 0 : (o > n ? (int)n : o);
    c = c < 0 ? 0 : c;
    off = o;
    cnt = c > n - o ? (int)(n - o) : c;
}

template <int G, int CF>
__global__ __launch_bounds__(SEG_BLOCK)
void k_seg_reduce(const int* __restrict__ seg_off,
                  const int* __restrict__ seg_cnt,
                  const int* __restrict__ perm,
                  const int* __restrict__ long_list,
                  const int* __restrict__ n_long, long long_cap,
                  int long_blocks, const float* __restrict__ grads, long n,
                  long dim, const int* __restrict__ u_dev,
                  float* __restrict__ ugrads, u64* __restrict__ counts) {
    __shared__ float red[SEG_BLOCK / 64][G * CF];
    const int lane = threadIdx.x % G;
    long u = *u_dev;
    u = u < 0 ? 0 : (u > n ? n : u);

    if ((int)blockIdx.x < long_blocks) {
        // ---- long role
        long nl = *n_long;
        nl = nl < 0 ? 0 : (nl > long_cap ? long_cap : nl);
        const int group = threadIdx.x / G;
        constexpr int NG = SEG_BLOCK / G;
        for (long b = blockIdx.x; b < nl; b += long_blocks) {
            const int uid = long_list[b];
            int off = 0, cnt = 0;
            if (uid >= 0 && uid < u)
                seg_range(seg_off, seg_cnt, uid, n, off, cnt);
            if (cnt <= SEG_T) continue;   // block-uniform: the short role's
            float acc[CF];
            #pragma unroll
            for (int c = 0; c < CF; ++c) acc[c] = 0.0f;
            // the next round's perm entries are loaded before this round's
            // rows are consumed: a round costs one load latency, not two
            int e[LR_ILP], en[LR_ILP];
            #pragma unroll
            for (int t = 0; t < LR_ILP; ++t)
                en[t] = (group * LR_ILP + t < cnt)
                            ? perm[off + group * LR_ILP + t] : -1;
            for (long base = group * LR_ILP; base < cnt;
                 base += NG * LR_ILP) {
                #pragma unroll
                for (int t = 0; t < LR_ILP; ++t) {
                    e[t] = (en[t] < 0 || en[t] >= n) ? -1 : en[t];
                    const long nx = base + NG * LR_ILP + t;
                    en[t] = (nx < cnt) ? perm[off + nx] : -1;
                }
                float v[LR_ILP][CF];
                #pragma unroll
                for (int t = 0; t < LR_ILP; ++t)
                    #pragma unroll
                    for (int c = 0; c < CF; ++c)
                        v[t][c] = (e[t] >= 0 && lane + c * G < dim)
                            ? grads[(u64)e[t] * dim + lane + c * G] : 0.0f;
                #pragma unroll
                for (int t = 0; t < LR_ILP; ++t)
                    #pragma unroll
                    for (int c = 0; c < CF; ++c) acc[c] += v[t][c];
            }
            #pragma unroll
            for (int d = G; d < 64; d <<= 1)
                #pragma unroll
                for (int c = 0; c < CF; ++c)
                    acc[c] += __shfl_xor(acc[c], d, 64);
            if ((threadIdx.x & 63) < G) {
                #pragma unroll
                for (int c = 0; c < CF; ++c)
                    red[threadIdx.x / 64][lane + c * G] = acc[c];
            }
            __syncthreads();
            if (threadIdx.x < G * CF) {
                float s = 0.0f;
                #pragma unroll
                for (int w = 0; w < SEG_BLOCK / 64; ++w)
                    s += red[w][threadIdx.x];
                if (threadIdx.x < dim)
                    ugrads[(u64)uid * dim + threadIdx.x] = s;
            }
            if (threadIdx.x == 0) counts[uid] = (u64)cnt;
            __syncthreads();
        }
        return;
    }

    // ---- short role
    const long ngroups = (long)(gridDim.x - long_blocks) * (SEG_BLOCK / G);
    const long g0 = ((long)(blockIdx.x - long_blocks) * SEG_BLOCK
                     + threadIdx.x) / G;
    int off[SR_ILP], cnt[SR_ILP], e0[SR_ILP];
    #pragma unroll
    for (int t = 0; t < SR_ILP; ++t) {
        long uid = g0 + t * ngroups;
        off[t] = 0;
        cnt[t] = 0;
        if (uid < u) seg_range(seg_off, seg_cnt, uid, n, off[t], cnt[t]);
    }
    #pragma unroll
    for (int t = 0; t < SR_ILP; ++t) {
        e0[t] = (cnt[t] > 0 && cnt[t] <= SEG_T) ? perm[off[t]] : -1;
        if (e0[t] < 0 || e0[t] >= n) e0[t] = -1;
    }
    float acc[SR_ILP][CF];
    #pragma unroll
    for (int t = 0; t < SR_ILP; ++t)
        #pragma unroll
        for (int c = 0; c < CF; ++c)
            acc[t][c] = (e0[t] >= 0 && lane + c * G < dim)
                ? grads[(u64)e0[t] * dim + lane + c * G] : 0.0f;
    #pragma unroll
    for (int t = 0; t < SR_ILP; ++t) {
        long uid = g0 + t * ngroups;
        if (uid >= n || cnt[t] > SEG_T) continue;   // none / the long role's
        for (int k = 1; k < cnt[t]; k += SR_ILP) {
            int e[SR_ILP];
            #pragma unroll
            for (int q = 0; q < SR_ILP; ++q) {
                e[q] = (k + q < cnt[t]) ? perm[off[t] + k + q] : -1;
                if (e[q] < 0 || e[q] >= n) e[q] = -1;
            }
            float v[SR_ILP][CF];
            #pragma unroll
            for (int q = 0; q < SR_ILP; ++q)
                #pragma unroll
                for (int c = 0; c < CF; ++c)
                    v[q][c] = (e[q] >= 0 && lane + c * G < dim)
                        ? grads[(u64)e[q] * dim + lane + c * G] : 0.0f;
            #pragma unroll
            for (int q = 0; q < SR_ILP; ++q)
                #pragma unroll
                for (int c = 0; c < CF; ++c) acc[t][c] += v[q][c];
        }
        #pragma unroll
        for (int c = 0; c < CF; ++c)
            if (lane + c * G < dim)
                ugrads[(u64)uid * dim + lane + c * G] = acc[t][c];
        if (lane == 0) counts[uid] = (u64)cnt[t];
    }
}

// ------------------------------------------------- pooled weight gradient
// dw[e] = scale_b * (<g_b, r_e> - c_e * <g_b, out_b>) for element e of bag
// b = bag_of[e], with c_e = 0 (sum) | 1 (mean) | w_e * scale_b (sqrtn):
// the gradient of the weighted pool w.r.t. its per-sample weights. r_e is
// read from the table through inverse -> map exactly as pool_row does (a
// miss is a zero row), so no [nnz, dim] tensor exists on the fused route.
// One G-lane group per ELEMENT (not per bag: the longest bag does not set
// the kernel's time), lanes over columns with WG_ILP independent column
// fragments in flight; grad_out[b] and out[b] are shared by a bag's
// elements and stay cache-hot. The cross-lane sum is a fixed-order
// __shfl_xor tree and lane 0 stores with a plain store: deterministic, no
// atomics. Elements whose bag_of is outside [0, B) (the tail) store 0;
// their weights are never read.
#define WG_ILP 4
template <int G, typename MapT>
__global__ void k_pool_wgrad(const float* __restrict__ rows, long R,
                             long dim, const i64* __restrict__ inverse,
                             long nnz, const MapT* __restrict__ map, long u,
                             const float* __restrict__ weights,
                             const int* __restrict__ bag_of,
                             const float* __restrict__ bag_scale,
                             const float* __restrict__ out,
                             const float* __restrict__ grad_out, long B,
                             int mode, float* __restrict__ dw) {
    const long e = ((long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int lane = threadIdx.x % G;
    if (e >= nnz) return;               // whole group: G divides the block
    const int bag = bag_of[e];
    if (bag < 0 || bag >= B) {
        if (lane == 0) dw[e] = 0.0f;
        return;
    }
    const long nidx = map ? u : R;
    const long row = pool_row(e, nnz, inverse, map, nidx, R);
    const float scale = bag_scale[bag];
    const float* __restrict__ g = grad_out + (u64)bag * dim;
    const float* __restrict__ o = out + (u64)bag * dim;
    const float* __restrict__ r = rows + (u64)(row >= 0 ? row : 0) * dim;
    const bool need_o = mode != POOL_SUM;
    float gr = 0.0f, go = 0.0f;
    for (long c0 = lane; c0 < dim; c0 += (long)G * WG_ILP) {
        float gv[WG_ILP], rv[WG_ILP], ov[WG_ILP];
        #pragma unroll
        for (int k = 0; k < WG_ILP; ++k) {
            const long c = c0 + (long)k * G;
            const bool in = c < dim;
            gv[k] = in ? g[c] : 0.0f;
            rv[k] = (in && row >= 0) ? r[c] : 0.0f;
            ov[k] = (in && need_o) ? o[c] : 0.0f;
        }
        #pragma unroll
        for (int k = 0; k < WG_ILP; ++k) {
            gr += gv[k] * rv[k];
            go += gv[k] * ov[k];
        }
    }
    #pragma unroll
    for (int m = G / 2; m > 0; m >>= 1) {
        gr += __shfl_xor(gr, m, G);
        go += __shfl_xor(go, m, G);
    }
    if (lane == 0) {
        float cj = 0.0f;
        if (mode == POOL_MEAN) cj = 1.0f;
        else if (mode == POOL_SQRTN) cj = weights[e] * scale;
        dw[e] = need_o ? scale * (gr - cj * go) : scale * gr;
    }
}

// ------------------------------------------------------------- optimizers
// State layouts documented in core/optimizers.py; formulas are the
// reference's (EmbeddingOptimizer.h) applied per unique row. Scalar state
// (adam/adamax beta powers, test flip) is updated by lane 0 of the row's
// group and broadcast with __shfl.

enum {
    OPT_DEFAULT = 0, OPT_ADADELTA = 1, OPT_ADAGRAD = 2, OPT_ADAM = 3,
    OPT_ADAMAX = 4, OPT_FTRL = 5, OPT_RMSPROP = 6, OPT_SGD = 7, OPT_TEST = 8
};

// The formulas exist once: opt_head does the row's scalar state (lane 0 of
// the group, broadcast with __shfl; the whole G-lane group must be active)
// and opt_col updates one column from its gradient gj, which k_apply_opt
// reads from memory and k_seg_reduce_apply holds in a register. ``head`` is
// what opt_head returned (adam/adamax lr_t, test s0), ``cnt`` the row's
// occurrence count (test only).

template <int G, int OPT>
DEV float opt_head(float* s, long dim, int lane, float c0,
                   float c1, float c2) {
    if (OPT == OPT_ADAM) {
        const float lr = c0, b1 = c1, b2 = c2;
        float lr_t = 0.0f;
        if (lane == 0) {
            float b1t = s[2 * dim] * b1;
            float b2t = s[2 * dim + 1] * b2;
            s[2 * dim] = b1t;
            s[2 * dim + 1] = b2t;
            lr_t = lr * sqrtf(1.0f - b2t) / (1.0f - b1t);
        }
        return __shfl(lr_t, 0, G);
    } else if (OPT == OPT_ADAMAX) {
        const float lr = c0, b1 = c1;
        float lr_t = 0.0f;
        if (lane == 0) {
            float b1t = s[2 * dim] * b1;
            s[2 * dim] = b1t;
            lr_t = lr / (1.0f - b1t);
        }
        return __shfl(lr_t, 0, G);
    } else if (OPT == OPT_TEST) {
        const float flip = c1;
        float s0 = 0.0f;
        if (lane == 0) {
            s0 = flip - s[0];
            s[0] = s0;
        }
        return __shfl(s0, 0, G);
    }
    return 0.0f;
}

template <int OPT>
DEV void opt_col(float* w, float* s, long dim,
                 long j, float gj, float head, float cnt, float c0, float c1,
                 float c2, float c3, float c4, float c5, float c6) {
    if (OPT == OPT_DEFAULT) {
        const float lr = c0;
        w[j] -= lr * gj;
    } else if (OPT == OPT_ADADELTA) {
        const float lr = c0, rho = c1, eps = c2;
        float* accum = s;
        float* au = s + dim;
        float a = accum[j] * rho + gj * gj * (1.0f - rho);
        accum[j] = a;
        float upd = gj * sqrtf(au[j] + eps) / sqrtf(a + eps);
        au[j] = au[j] * rho + upd * upd * (1.0f - rho);
        w[j] -= lr * upd;
    } else if (OPT == OPT_ADAGRAD) {
        const float lr = c0, eps = c2;
        float* accum = s;
        float a = accum[j] + gj * gj;
        accum[j] = a;
        w[j] -= lr * gj / (sqrtf(a) + eps);
    } else if (OPT == OPT_ADAM) {
        const float b1 = c1, b2 = c2, eps = c3;
        float* m = s;
        float* v = s + dim;
        const float lr_t = head;
        float mj = m[j] * b1 + gj * (1.0f - b1);
        float vj = v[j] * b2 + gj * gj * (1.0f - b2);
        m[j] = mj; v[j] = vj;
        w[j] -= lr_t * mj / (sqrtf(vj) + eps);
    } else if (OPT == OPT_ADAMAX) {
        const float b1 = c1, b2 = c2, eps = c3;
        float* m = s;
        float* v = s + dim;
        const float lr_t = head;
        float mj = m[j] * b1 + gj * (1.0f - b1);
        float vj = fmaxf(fabsf(gj), v[j] * b2);
        m[j] = mj; v[j] = vj;
        w[j] -= lr_t * mj / (vj + eps);
    } else if (OPT == OPT_FTRL) {
        const float lr = c0, l1 = c1, l2 = c2, l2s = c3, lrp = c4, beta = c5;
        float* accum = s;
        float* linear = s + dim;
        const float adj_l2 = l2 + beta / lr / 2.0f;
        float wj = w[j];
        float gg = gj + 2.0f * l2s * wj;
        float a_old = accum[j];
        float a_new = a_old + gj * gj;
        float sigma, quad;
        if (lrp == -0.5f) {
            sigma = (sqrtf(a_new) - sqrtf(a_old)) / lr;
            quad = sqrtf(a_new) / lr + 2.0f * adj_l2;
        } else {
            float p = -lrp;
            sigma = (powf(a_new, p) - powf(a_old, p)) / lr;
            quad = powf(a_new, p) / lr + 2.0f * adj_l2;
        }
        float lin = linear[j] + gg - sigma * wj;
        linear[j] = lin;
        accum[j] = a_new;
        float l1a = fminf(fmaxf(lin, -l1), l1);
        w[j] = (l1a - lin) / quad;
    } else if (OPT == OPT_RMSPROP) {
        const float lr = c0, rho = c1, mom = c2, eps = c3;
        float* accum = s;
        float* moment = s + dim;
        float a = accum[j] * rho + gj * gj * (1.0f - rho);
        accum[j] = a;
        float mo = moment[j] * mom + lr * gj / sqrtf(a + eps);
        moment[j] = mo;
        w[j] -= mo;
    } else if (OPT == OPT_SGD) {
        const float lr = c0, mom = c1;
        const bool nesterov = c2 != 0.0f;
        float* moment = s;
        float mo = moment[j] * mom + lr * gj;
        moment[j] = mo;
        w[j] -= nesterov ? (mo * mom + lr * gj) : mo;
    } else if (OPT == OPT_TEST) {
        const float lr = c0, s0 = head;
        w[j] += lr * gj / cnt + s0;
    }
}

template <int G, int OPT>
__global__ void k_apply_opt(float* __restrict__ weights,
                            float* __restrict__ state,
                            long dim, long sd,
                            const i64* __restrict__ slots, long n,
                            const float* __restrict__ grads,
                            const u64* __restrict__ counts,
                            float c0, float c1, float c2, float c3,
                            float c4, float c5, float c6,
                            const int* __restrict__ u_dev) {
    long g = ((long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    int lane = threadIdx.x % G;
    if (g >= n) return;
    if (u_dev && g >= *u_dev) return;
    i64 slot = slots[g];
    if (slot < 0) return;
    float* w = weights + (u64)slot * dim;
    float* s = state + (u64)slot * sd;
    const float* gr = grads + (u64)g * dim;

    if (OPT == OPT_DEFAULT && c0 == 0.0f) return;   // lr 0: rows untouched
    const float head = opt_head<G, OPT>(s, dim, lane, c0, c1, c2);
    const float cnt = OPT == OPT_TEST ? (float)counts[g] : 0.0f;
    for (long j = lane; j < dim; j += G)
        opt_col<OPT>(w, s, dim, j, gr[j], head, cnt, c0, c1, c2, c3, c4, c5,
                     c6);
}

// ---------------------------------- segmented reduce + optimizer, one launch
// k_seg_reduce's two roles with the optimizer step in place of the ugrads
// and counts stores: the lane group (short role) or block (long role) that
// summed a uid's row applies it to the table row behind slots[uid], so the
// [n, dim] per-unique gradients and their counts never exist in memory and
// the commit needs no launch of its own. Same walk, same sum order, same
// guards as k_seg_reduce, and the same opt_head / opt_col as k_apply_opt:
// the table afterwards is bit for bit what the two launches leave when the
// sums do not depend on arrival order. uids at and beyond *u_dev and uids
// with slot < 0 are skipped, like k_apply_opt skips them; the count the
// ``test`` optimizer divides by is the clamped seg_cnt. Every live uid is
// applied exactly once: by the role its clamped count selects.
template <int G, int CF, int OPT>
__global__ __launch_bounds__(SEG_BLOCK)
void k_seg_reduce_apply(const int* __restrict__ seg_off,
                        const int* __restrict__ seg_cnt,
                        const int* __restrict__ perm,
                        const int* __restrict__ long_list,
                        const int* __restrict__ n_long, long long_cap,
                        int long_blocks, const float* __restrict__ grads,
                        long n, long dim, const int* __restrict__ u_dev,
                        const i64* __restrict__ slots,
                        float* __restrict__ weights,
                        float* __restrict__ state, long sd,
                        float c0, float c1, float c2, float c3, float c4,
                        float c5, float c6) {
    __shared__ float red[SEG_BLOCK / 64][G * CF];
    __shared__ float tot[G * CF];
    const int lane = threadIdx.x % G;
    long u = *u_dev;
    u = u < 0 ? 0 : (u > n ? n : u);
    if (OPT == OPT_DEFAULT && c0 == 0.0f) return;   // lr 0: rows untouched

    if ((int)blockIdx.x < long_blocks) {
        // ---- long role
        long nl = *n_long;
        nl = nl < 0 ? 0 : (nl > long_cap ? long_cap : nl);
        const int group = threadIdx.x / G;
        constexpr int NG = SEG_BLOCK / G;
        for (long b = blockIdx.x; b < nl; b += long_blocks) {
            const int uid = long_list[b];
            int off = 0, cnt = 0;
            i64 slot = -1;
            if (uid >= 0 && uid < u) {
                seg_range(seg_off, seg_cnt, uid, n, off, cnt);
                slot = slots[uid];
            }
            if (cnt <= SEG_T) continue;   // block-uniform: the short role's
            float acc[CF];
            #pragma unroll
            for (int c = 0; c < CF; ++c) acc[c] = 0.0f;
            int e[LR_ILP], en[LR_ILP];
            #pragma unroll
            for (int t = 0; t < LR_ILP; ++t)
                en[t] = (group * LR_ILP + t < cnt)
                            ? perm[off + group * LR_ILP + t] : -1;
            for (long base = group * LR_ILP; base < cnt;
                 base += NG * LR_ILP) {
                #pragma unroll
                for (int t = 0; t < LR_ILP; ++t) {
                    e[t] = (en[t] < 0 || en[t] >= n) ? -1 : en[t];
                    const long nx = base + NG * LR_ILP + t;
                    en[t] = (nx < cnt) ? perm[off + nx] : -1;
                }
                float v[LR_ILP][CF];
                #pragma unroll
                for (int t = 0; t < LR_ILP; ++t)
                    #pragma unroll
                    for (int c = 0; c < CF; ++c)
                        v[t][c] = (e[t] >= 0 && lane + c * G < dim)
                            ? grads[(u64)e[t] * dim + lane + c * G] : 0.0f;
                #pragma unroll
                for (int t = 0; t < LR_ILP; ++t)
                    #pragma unroll
                    for (int c = 0; c < CF; ++c) acc[c] += v[t][c];
            }
            #pragma unroll
            for (int d = G; d < 64; d <<= 1)
                #pragma unroll
                for (int c = 0; c < CF; ++c)
                    acc[c] += __shfl_xor(acc[c], d, 64);
            if ((threadIdx.x & 63) < G) {
                #pragma unroll
                for (int c = 0; c < CF; ++c)
                    red[threadIdx.x / 64][lane + c * G] = acc[c];
            }
            __syncthreads();
            if (threadIdx.x < G * CF) {
                float s = 0.0f;
                #pragma unroll
                for (int w = 0; w < SEG_BLOCK / 64; ++w)
                    s += red[w][threadIdx.x];
                tot[threadIdx.x] = s;
            }
            __syncthreads();
            // the block's first group applies the row (slot: block-uniform)
            if (threadIdx.x < G && slot >= 0) {
                float* w = weights + (u64)slot * dim;
                float* s = state + (u64)slot * sd;
                const float head = opt_head<G, OPT>(s, dim, lane, c0, c1, c2);
                #pragma unroll
                for (int c = 0; c < CF; ++c)
                    if (lane + c * G < dim)
                        opt_col<OPT>(w, s, dim, lane + c * G,
                                     tot[lane + c * G], head, (float)cnt, c0,
                                     c1, c2, c3, c4, c5, c6);
            }
        }
        return;
    }

    // ---- short role
    const long ngroups = (long)(gridDim.x - long_blocks) * (SEG_BLOCK / G);
    const long g0 = ((long)(blockIdx.x - long_blocks) * SEG_BLOCK
                     + threadIdx.x) / G;
    int off[SR_ILP], cnt[SR_ILP], e0[SR_ILP];
    i64 slot[SR_ILP];
    #pragma unroll
    for (int t = 0; t < SR_ILP; ++t) {
        long uid = g0 + t * ngroups;
        off[t] = 0;
        cnt[t] = 0;
        slot[t] = -1;
        if (uid < u) {
            seg_range(seg_off, seg_cnt, uid, n, off[t], cnt[t]);
            slot[t] = slots[uid];   // with the range, not behind the chain
        }
    }
    #pragma unroll
    for (int t = 0; t < SR_ILP; ++t) {
        e0[t] = (cnt[t] > 0 && cnt[t] <= SEG_T) ? perm[off[t]] : -1;
        if (e0[t] < 0 || e0[t] >= n) e0[t] = -1;
    }
    float acc[SR_ILP][CF];
    #pragma unroll
    for (int t = 0; t < SR_ILP; ++t)
        #pragma unroll
        for (int c = 0; c < CF; ++c)
            acc[t][c] = (e0[t] >= 0 && lane + c * G < dim)
                ? grads[(u64)e0[t] * dim + lane + c * G] : 0.0f;
    #pragma unroll
    for (int t = 0; t < SR_ILP; ++t) {
        long uid = g0 + t * ngroups;
        if (uid >= u || cnt[t] > SEG_T) continue;   // none / the long role's
        for (int k = 1; k < cnt[t]; k += SR_ILP) {
            int e[SR_ILP];
            #pragma unroll
            for (int q = 0; q < SR_ILP; ++q) {
                e[q] = (k + q < cnt[t]) ? perm[off[t] + k + q] : -1;
                if (e[q] < 0 || e[q] >= n) e[q] = -1;
            }
            float v[SR_ILP][CF];
            #pragma unroll
            for (int q = 0; q < SR_ILP; ++q)
                #pragma unroll
                for (int c = 0; c < CF; ++c)
                    v[q][c] = (e[q] >= 0 && lane + c * G < dim)
                        ? grads[(u64)e[q] * dim + lane + c * G] : 0.0f;
            #pragma unroll
            for (int q = 0; q < SR_ILP; ++q)
                #pragma unroll
                for (int c = 0; c < CF; ++c) acc[t][c] += v[q][c];
        }
        if (slot[t] < 0) continue;
        float* w = weights + (u64)slot[t] * dim;
        float* s = state + (u64)slot[t] * sd;
        const float head = opt_head<G, OPT>(s, dim, lane, c0, c1, c2);
        #pragma unroll
        for (int c = 0; c < CF; ++c)
            if (lane + c * G < dim)
                opt_col<OPT>(w, s, dim, lane + c * G, acc[t][c], head,
                             (float)cnt[t], c0, c1, c2, c3, c4, c5, c6);
    }
}

// ---------------------------------------------------- flat dense optimizer
// One fused elementwise pass for the flattened dense-parameter buffer:
// bf16 form keeps an fp32 master + fp32 accumulator and writes the bf16
// working weights (native-bf16 MLP: the MFMA GEMMs read bf16 weights that
// are never re-cast per step); f32 form is plain Adagrad in one kernel
// (replaces 3 torch elementwise launches).

#include <hip/hip_bf16.h>
typedef __hip_bfloat16 oebf16;

__global__ void k_flat_adagrad_f32(float* __restrict__ p,
                                   float* __restrict__ accum,
                                   const float* __restrict__ g,
                                   long n, float lr, float eps) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float gi = g[i];
    float a = accum[i] + gi * gi;
    accum[i] = a;
    p[i] -= lr * gi / (sqrtf(a) + eps);
}

__global__ void k_flat_adagrad_bf16(float* __restrict__ master,
                                    float* __restrict__ accum,
                                    const oebf16* __restrict__ g,
                                    oebf16* __restrict__ p,
                                    long n, float lr, float eps) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float gi = (float)g[i];
    float a = accum[i] + gi * gi;
    accum[i] = a;
    float m = master[i] - lr * gi / (sqrtf(a) + eps);
    master[i] = m;
    p[i] = (oebf16)m;
}

// Generic flat dense optimizers (sgd / adagrad / adam), f32 params or
// bf16 params + fp32 master. Semantics match torch.optim defaults
// (dampening 0, no weight decay / amsgrad). Adam's bias correction reads
// DEVICE scalars prepared by k_flat_step_scalars so a hipGraph-captured
// step keeps correcting (a host-side 1-beta^t would freeze at capture).

enum { FLAT_SGD = 0, FLAT_ADAGRAD = 1, FLAT_ADAM = 2 };

__global__ void k_flat_step_scalars(float* __restrict__ sc, float b1,
                                    float b2) {
    if (threadIdx.x || blockIdx.x) return;
    float t = sc[0] + 1.0f;
    sc[0] = t;
    sc[1] = 1.0f - powf(b1, t);
    sc[2] = 1.0f - powf(b2, t);
}

template <int OPT>
__device__ __forceinline__ float flat_opt_step(
        float w, float gi, float* __restrict__ s1, float* __restrict__ s2,
        long i, const float* __restrict__ sc, float lr, float c0, float c1,
        float c2) {
    if (OPT == FLAT_ADAGRAD) {
        float a = s1[i] + gi * gi;
        s1[i] = a;
        return w - lr * gi / (sqrtf(a) + c0);
    }
    if (OPT == FLAT_SGD) {
        if (c0 == 0.0f) return w - lr * gi;     // plain
        float b = c0 * s1[i] + gi;              // momentum, dampening 0
        s1[i] = b;
        float d = (c1 != 0.0f) ? gi + c0 * b : b;   // c1 = nesterov
        return w - lr * d;
    }
    // FLAT_ADAM: c0=beta1, c1=beta2, c2=eps; sc[1]=1-b1^t, sc[2]=1-b2^t
    float m = c0 * s1[i] + (1.0f - c0) * gi;
    float v = c1 * s2[i] + (1.0f - c1) * gi * gi;
    s1[i] = m;
    s2[i] = v;
    float mh = m / sc[1];
    float vh = v / sc[2];
    return w - lr * mh / (sqrtf(vh) + c2);
}

// Both variants zero the grad element after consuming it: the next
// backward's AccumulateGrad lands on a clean buffer, so the caller's
// zero_grad() is a steady-state no-op (saves one FillFunctor launch per
// dtype group per captured step).
template <int OPT>
__global__ void k_flat_opt_f32(float* __restrict__ p,
                               float* __restrict__ s1,
                               float* __restrict__ s2,
                               float* __restrict__ g,
                               const float* __restrict__ sc, long n,
                               float lr, float c0, float c1, float c2) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    p[i] = flat_opt_step<OPT>(p[i], g[i], s1, s2, i, sc, lr, c0, c1, c2);
    g[i] = 0.0f;
}

template <int OPT>
__global__ void k_flat_opt_bf16(float* __restrict__ master,
                                float* __restrict__ s1,
                                float* __restrict__ s2,
                                oebf16* __restrict__ g,
                                oebf16* __restrict__ p,
                                const float* __restrict__ sc, long n,
                                float lr, float c0, float c1, float c2) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float m = flat_opt_step<OPT>(master[i], (float)g[i], s1, s2, i, sc, lr,
                                 c0, c1, c2);
    master[i] = m;
    p[i] = (oebf16)m;
    g[i] = (oebf16)0.0f;
}

// ---- fused BCE-with-logits (mean) --------------------------------------
// torch's BCEWithLogitsLoss costs ~5 launches per step in the captured
// train graph (log_sigmoid, mean reduce, grad fill, sigmoid-sub-scale
// chain); these two kernels replace them. Same stable formulation as
// torch: max(z,0) - z*y + log1p(exp(-|z|)).

__global__ void k_bce_fwd(const float* __restrict__ z,
                          const float* __restrict__ y, long n, float inv_n,
                          float* __restrict__ loss) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    float v = 0.f;
    if (i < n) {
        float zi = z[i];
        v = (fmaxf(zi, 0.f) - zi * y[i] + log1pf(__expf(-fabsf(zi)))) * inv_n;
    }
    for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0 && v != 0.f) atomicAdd(loss, v);
}

// Single-block variant for bench-sized batches: grid-stride sum + LDS
// cross-wave reduce + ONE plain store — no pre-zero fill, no atomics
// (two launches -> one; the fill alone was ~4 us of launch/ramp).
__global__ void k_bce_fwd_1blk(const float* __restrict__ z,
                               const float* __restrict__ y, long n,
                               float inv_n, float* __restrict__ loss) {
    __shared__ float wsum[16];
    float v = 0.f;
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
        float zi = z[i];
        v += (fmaxf(zi, 0.f) - zi * y[i]
              + log1pf(__expf(-fabsf(zi)))) * inv_n;
    }
    for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += wsum[w];
        *loss = t;
    }
}

__global__ void k_bce_bwd(const float* __restrict__ z,
                          const float* __restrict__ y, long n, float inv_n,
                          const float* __restrict__ go,
                          float* __restrict__ g) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float zi = z[i];
    float s = 1.f / (1.f + __expf(-zi));
    g[i] = (s - y[i]) * inv_n * go[0];
}

// ------------------------------------------- padded all-to-all bucketize
// The sync-free multi-rank wire format: instead of exact per-peer splits
// (whose sizes need a device->host read every step), every rank ships a
// FIXED [world, cap] key block to its peers, padded with the reserved key
// -1. Padding flows through the whole owner pipeline as defined misses
// (unique: own entry per occurrence; hash/array lookup: slot -1; gather:
// zeros; optimizer: skipped), so no host knowledge is needed anywhere and
// the full multi-rank step is hipGraph-capturable. `overflow` accumulates
// keys dropped because a bucket exceeded cap; the host checks it outside
// the hot loop and raises (capacity knob OEAMD_A2A_SLACK).
// Reference analogue: EmbeddingPullOperator.cpp:67-79 shard bucketize (the
// RPC fabric let the reference send exact sizes; xGMI all-to-all prefers
// fixed shapes).

__global__ void k_bucketize_pad(const i64* __restrict__ keys, long n,
                                const int* __restrict__ u_dev, long world,
                                long cap,
                                i64* __restrict__ send_keys,
                                int* __restrict__ send_src,
                                int* __restrict__ pos_of,
                                int* __restrict__ counts,
                                int* __restrict__ overflow) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    pos_of[i] = -1;
    if (u_dev && i >= *u_dev) return;   // beyond the live unique count
    i64 k = keys[i];
    if (k < 0) return;                  // reserved key: never shipped
    long owner = (long)((u64)k % (u64)world);
    int pos = atomicAdd(&counts[owner], 1);
    if (pos >= cap) { atomicAdd(overflow, 1); return; }
    long s = owner * cap + pos;
    send_keys[s] = k;
    send_src[s] = (int)i;
    pos_of[i] = (int)s;
}

// push payload gather into the padded send layout: row = grads ‖ count
// (count as f32: counts <= batch size, exact in fp32). Padded rows are
// zero-filled; the owner drops them anyway (their keys are -1 -> slot -1).
__global__ void k_gather_pad(const float* __restrict__ ugrads,
                             const u64* __restrict__ counts, long dim,
                             const int* __restrict__ send_src, long total,
                             float* __restrict__ send_p) {
    long dimp = dim + 1;
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total * dimp) return;
    long r = e / dimp, j = e % dimp;
    int src = send_src[r];
    float v = 0.0f;
    if (src >= 0)
        v = (j < dim) ? ugrads[(u64)src * dim + j] : (float)counts[src];
    send_p[e] = v;
}

// final pull output: out[e] = returned row of e's unique (zeros for keys
// that were never shipped: reserved/overflowed). Fuses the unique->element
// duplicate scatter with the wire->unique permutation.
__global__ void k_scatter_out(const float* __restrict__ rows_recv,
                              const i64* __restrict__ inverse, long n_elems,
                              const int* __restrict__ pos_of, long dim,
                              float* __restrict__ out) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_elems * dim) return;
    long r = e / dim, j = e % dim;
    int pos = pos_of[inverse[r]];
    out[e] = (pos >= 0) ? rows_recv[(u64)pos * dim + j] : 0.0f;
}

// split the owner-side reduced payload [u, dim+1] back into grads + counts
__global__ void k_split_payload(const float* __restrict__ g2c, long u,
                                long dim, const int* __restrict__ u_dev,
                                float* __restrict__ grads,
                                u64* __restrict__ counts) {
    long dimp = dim + 1;
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= u * dimp) return;
    long r = e / dimp, j = e % dimp;
    if (u_dev && r >= *u_dev) return;
    if (j < dim) grads[(u64)r * dim + j] = g2c[e];
    else counts[r] = (u64)(g2c[e] + 0.5f);
}

// zero the garbage tail of a bounded (buffer + device-count) gradient
// block so blocks can be merged by concatenation: a commit with several
// pulls of one variable must apply the optimizer ONCE per unique key over
// the summed gradients (reference MpscGradientReducer.h:30-53 semantics),
// not once per block.
__global__ void k_mask_tail(i64* __restrict__ keys, float* __restrict__ grads,
                            u64* __restrict__ counts, long n, long dim,
                            const int* __restrict__ u_dev) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * dim) return;
    long i = e / dim, j = e % dim;
    long live = u_dev ? (long)*u_dev : n;
    if (i < live) return;
    grads[e] = 0.f;
    if (j == 0) { keys[i] = -1; counts[i] = 0; }
}

// ------------------------------------------------------- capacity tier v2
// HBM row-cache over a pinned host-DRAM backing store (the reference's
// DRAM-cache-over-PMem design, PmemEmbeddingTable.h:237-270, re-based on
// the MI355X memory hierarchy). A SECOND device-side hash table maps
// spilled keys -> host-slab slots, so the fault-in decision runs on
// device with no host key lists; pinned host memory is read/written
// directly by these kernels (zero-copy gather: only touched rows cross
// the PCIe/host link).

__device__ __forceinline__ long host_probe(const u64* __restrict__ htk,
                                           const int* __restrict__ htv,
                                           long mask, u64 k) {
    u64 h = splitmix64(k) & (u64)mask;
    for (long p = 0; p <= mask; ++p) {
        u64 cur = htk[h];
        if (cur == k) return (long)htv[h];
        if (cur == EMPTY) return -1;
        h = (h + 1) & (u64)mask;
    }
    return -1;
}

// fault-in: rows that missed the cache (new_mask=1) but live in the host
// tier are copied host->cache and their new_mask cleared, so the
// downstream gather treats them as existing rows (no lazy re-init).
// G lanes per row.
template <int G>
__global__ void k_fault_in(const i64* __restrict__ keys, long n,
                           const int* __restrict__ u_dev,
                           const u64* __restrict__ htk,
                           const int* __restrict__ htv, long hmask,
                           const float* __restrict__ host_w,
                           const float* __restrict__ host_s,
                           float* __restrict__ weights,
                           float* __restrict__ state, long dim, long sd,
                           const i64* __restrict__ slots,
                           unsigned char* __restrict__ new_mask,
                           int* __restrict__ faulted) {
    long g = ((long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    int lane = threadIdx.x % G;
    if (g >= n) return;
    if (u_dev && g >= *u_dev) return;
    if (!new_mask[g]) return;
    i64 slot = slots[g];
    if (slot < 0) return;
    u64 k = (u64)keys[g];
    if (k == EMPTY) return;
    long hs = host_probe(htk, htv, hmask, k);
    if (hs < 0) return;                       // truly new: lazy init
    float* wrow = weights + (u64)slot * dim;
    const float* hw = host_w + (u64)hs * dim;
    for (long j = lane; j < dim; j += G) wrow[j] = hw[j];
    if (sd > 0) {
        float* srow = state + (u64)slot * sd;
        const float* hsrow = host_s + (u64)hs * sd;
        for (long j = lane; j < sd; j += G) srow[j] = hsrow[j];
    }
    if (lane == 0) {
        new_mask[g] = 0;
        atomicAdd(faulted, 1);
    }
}

// spill: copy cache rows (by slot) into host-slab rows (by host slot)
template <int G>
__global__ void k_spill_rows(const i64* __restrict__ cache_slots,
                             const i64* __restrict__ host_slots, long n,
                             const float* __restrict__ weights,
                             const float* __restrict__ state,
                             float* __restrict__ host_w,
                             float* __restrict__ host_s, long dim, long sd) {
    long g = ((long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    int lane = threadIdx.x % G;
    if (g >= n) return;
    i64 cs = cache_slots[g], hs = host_slots[g];
    if (cs < 0 || hs < 0) return;
    const float* wrow = weights + (u64)cs * dim;
    float* hw = host_w + (u64)hs * dim;
    for (long j = lane; j < dim; j += G) hw[j] = wrow[j];
    if (sd > 0) {
        const float* srow = state + (u64)cs * sd;
        float* hsrow = host_s + (u64)hs * sd;
        for (long j = lane; j < sd; j += G) hsrow[j] = srow[j];
    }
}

// read-only host gather (serving/export): rows that missed the cache
// (slot -1) but exist in the host tier are read straight into `out`
template <int G>
__global__ void k_gather_host(const i64* __restrict__ keys, long n,
                              const i64* __restrict__ cache_slots,
                              const u64* __restrict__ htk,
                              const int* __restrict__ htv, long hmask,
                              const float* __restrict__ host_w,
                              float* __restrict__ out, long dim) {
    long g = ((long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    int lane = threadIdx.x % G;
    if (g >= n) return;
    if (cache_slots[g] >= 0) return;          // cache hit already gathered
    u64 k = (u64)keys[g];
    if (k == EMPTY) return;
    long hs = host_probe(htk, htv, hmask, k);
    if (hs < 0) return;                       // unknown key: stays zeros
    const float* hw = host_w + (u64)hs * dim;
    for (long j = lane; j < dim; j += G) out[(u64)g * dim + j] = hw[j];
}

// ------------------------------------------------------ delta checkpoints
// Change tracking for incremental dumps: row_epoch[slot] holds the epoch of
// the row's last write; a delta is the rows with row_epoch >= since. The
// current epoch is read THROUGH epoch_dev, so a captured step stamps the
// epoch that is current at replay, not the one frozen at capture.

// stamp: one thread per element; duplicates store the same value (benign)
__global__ void k_mark_rows(const i64* __restrict__ slots, long n,
                            const unsigned char* __restrict__ mask,
                            const int* __restrict__ u_dev,
                            const int* __restrict__ epoch_dev,
                            int* __restrict__ row_epoch, long R) {
    long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    if (u_dev && g >= *u_dev) return;
    if (mask && !mask[g]) return;
    i64 s = slots[g];
    if (s < 0 || s >= R) return;
    row_epoch[s] = *epoch_dev;
}

// Ordered stream compaction of the changed rows in three launches: per-tile
// counts, a scan of the counts (the launcher's caller), and a compaction
// that re-evaluates the predicate. No block ever waits for another. A tile
// is DT_ITEMS rounds of one block; round i covers rows
// [tile + i*BLOCK, tile + (i+1)*BLOCK), one row per thread (coalesced), so
// ascending row order is (round, wave, lane).
#define DT_ITEMS 8
#define DT_TILE (BLOCK * DT_ITEMS)
#define DT_WAVES (BLOCK / 64)

DEV bool delta_pred(const int* __restrict__ row_epoch, int since, long r,
                    long R, long live,
                    const unsigned char* __restrict__ valid) {
    if (r >= R) return false;
    if (valid ? valid[r] == 0 : r >= live) return false;
    return row_epoch[r] >= since;
}

DEV long delta_live(const int* __restrict__ nrows_dev, long R) {
    if (!nrows_dev) return R;
    long live = (long)*nrows_dev;
    return live < 0 ? 0 : (live > R ? R : live);
}

__global__ __launch_bounds__(BLOCK)
void k_delta_count(const int* __restrict__ row_epoch, long R, int since,
                   const int* __restrict__ nrows_dev,
                   const unsigned char* __restrict__ valid,
                   int* __restrict__ tile_counts) {
    __shared__ int wave_cnt[DT_WAVES];
    long live = delta_live(nrows_dev, R);
    long base = (long)blockIdx.x * DT_TILE + threadIdx.x;
    int c = 0;
#pragma unroll
    for (int i = 0; i < DT_ITEMS; ++i) {
        bool p = delta_pred(row_epoch, since, base + (long)i * BLOCK, R, live,
                            valid);
        c += __popcll(__ballot(p));
    }
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < DT_WAVES; ++w) t += wave_cnt[w];
        tile_counts[blockIdx.x] = t;
    }
}

// tile_incl: inclusive scan of tile_counts over all T tiles
__global__ __launch_bounds__(BLOCK)
void k_delta_compact(const int* __restrict__ row_epoch, long R, int since,
                     const int* __restrict__ nrows_dev,
                     const unsigned char* __restrict__ valid,
                     const int* __restrict__ tile_incl, long T,
                     i64* __restrict__ slots) {
    __shared__ int cnt[DT_ITEMS * DT_WAVES];
    __shared__ int off[DT_ITEMS * DT_WAVES];
    long live = delta_live(nrows_dev, R);
    long base = (long)blockIdx.x * DT_TILE + threadIdx.x;
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;
    bool p[DT_ITEMS];
    int rank[DT_ITEMS];
#pragma unroll
    for (int i = 0; i < DT_ITEMS; ++i) {
        p[i] = delta_pred(row_epoch, since, base + (long)i * BLOCK, R, live,
                          valid);
        u64 b = __ballot(p[i]);
        rank[i] = __popcll(b & below);
        if (lane == 0) cnt[i * DT_WAVES + wave] = __popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int j = 0; j < DT_ITEMS * DT_WAVES; ++j) {
            off[j] = run;
            run += cnt[j];
        }
    }
    __syncthreads();
    long total = (long)tile_incl[T - 1];
    long tile_base = blockIdx.x ? (long)tile_incl[blockIdx.x - 1] : 0;
#pragma unroll
    for (int i = 0; i < DT_ITEMS; ++i) {
        long r = base + (long)i * BLOCK;
        if (p[i]) {
            long pos = tile_base + off[i * DT_WAVES + wave] + rank[i];
            if (pos >= 0 && pos < R) slots[pos] = r;
        }
        // the tail of the list: position r is past every compacted entry
        if (r < R && r >= total) slots[r] = -1;
    }
}

// gather the rows of slots[start, start+count) into staging buffers; one
// G-lane group per row, keys from slot_keys (hash) or the array layout
template <int G>
__global__ void k_delta_gather(const float* __restrict__ weights,
                               const float* __restrict__ state, long R,
                               long dim, long sd,
                               const i64* __restrict__ slot_keys,
                               long shard_num, long shard_id,
                               const i64* __restrict__ slots, long nslots,
                               long start, long count,
                               const int* __restrict__ n_dev,
                               i64* __restrict__ keys_out,
                               float* __restrict__ w_out,
                               float* __restrict__ s_out) {
    long g = ((long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    int lane = threadIdx.x % G;
    if (g >= count) return;
    long pos = start + g;
    if (pos < 0 || pos >= nslots || pos >= (long)*n_dev) return;
    i64 slot = slots[pos];
    if (slot < 0 || slot >= R) return;
    if (lane == 0)
        keys_out[g] = slot_keys ? slot_keys[slot]
                                : slot * shard_num + shard_id;
    const float* wrow = weights + (u64)slot * dim;
    float* wo = w_out + (u64)g * dim;
    for (long j = lane; j < dim; j += G) wo[j] = wrow[j];
    if (sd > 0) {
        const float* srow = state + (u64)slot * sd;
        float* so = s_out + (u64)g * sd;
        for (long j = lane; j < sd; j += G) so[j] = srow[j];
    }
}

// ------------------------------------------------------------- row expiry
// Removal of rows in place (maintenance, between steps). The caller flags
// the dead rows in dead[R]; the ordered compaction above, over other
// predicates, lists the removed keys, the holes and the movers, a move kernel
// fills the holes plane by plane and the probe table is rebuilt from
// slot_keys. With n live rows of which m are dead and n' = n - m:
//   XP_DEAD   live rows that are flagged            (their keys are returned)
//   XP_HOLE   flagged rows below n'                 (destinations)
//   XP_MOVER  live rows at or above n' not flagged  (sources)
// There are as many holes as movers, and the i-th mover goes to the i-th
// hole. cnt = {m, n'} lives on the device: XP_HOLE / XP_MOVER read n' there.
// An array table (valid != null) has XP_DEAD only: nothing moves.
#define XP_DEAD 0
#define XP_HOLE 1
#define XP_MOVER 2

// dead[r] = row r is live and was last written before epoch `before`
__global__ void k_expire_flag(const int* __restrict__ row_epoch, long R,
                              int before, const int* __restrict__ nrows_dev,
                              const unsigned char* __restrict__ valid,
                              unsigned char* __restrict__ dead) {
    long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    bool live = valid ? valid[r] != 0 : r < delta_live(nrows_dev, R);
    dead[r] = (live && row_epoch[r] < before) ? 1 : 0;
}

// dead[slot] = 1 for the named rows; misses (-1) and slots outside the slab
// are skipped, duplicates store the same value (benign)
__global__ void k_flag_slots(const i64* __restrict__ slots, long n,
                             unsigned char* __restrict__ dead, long R) {
    long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    i64 s = slots[g];
    if (s < 0 || s >= R) return;
    dead[s] = 1;
}

template <int MODE>
DEV bool expire_pred(const unsigned char* __restrict__ dead, long r, long R,
                     long live, long np,
                     const unsigned char* __restrict__ valid) {
    if (r >= R) return false;
    if (valid) return MODE == XP_DEAD && valid[r] != 0 && dead[r] != 0;
    if (r >= live) return false;
    if (MODE == XP_DEAD) return dead[r] != 0;
    if (MODE == XP_HOLE) return r < np && dead[r] != 0;
    return r >= np && dead[r] == 0;
}

// k_delta_count over expire_pred
template <int MODE>
__global__ __launch_bounds__(BLOCK)
void k_expire_count(const unsigned char* __restrict__ dead, long R,
                    const int* __restrict__ nrows_dev,
                    const unsigned char* __restrict__ valid,
                    const int* __restrict__ cnt,
                    int* __restrict__ tile_counts) {
    __shared__ int wave_cnt[DT_WAVES];
    long live = delta_live(nrows_dev, R);
    long np = MODE == XP_DEAD ? 0 : (long)cnt[1];
    long base = (long)blockIdx.x * DT_TILE + threadIdx.x;
    int c = 0;
#pragma unroll
    for (int i = 0; i < DT_ITEMS; ++i) {
        bool p = expire_pred<MODE>(dead, base + (long)i * BLOCK, R, live, np,
                                   valid);
        c += __popcll(__ballot(p));
    }
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < DT_WAVES; ++w) t += wave_cnt[w];
        tile_counts[blockIdx.x] = t;
    }
}

// cnt = {m, n'} from the scanned XP_DEAD tile counts
__global__ void k_expire_counts(const int* __restrict__ tile_incl, long T,
                                const int* __restrict__ nrows_dev, long R,
                                int* __restrict__ cnt) {
    if (blockIdx.x || threadIdx.x) return;
    long m = (long)tile_incl[T - 1];
    cnt[0] = (int)m;
    cnt[1] = (int)(delta_live(nrows_dev, R) - m);
}

// k_delta_compact over expire_pred: position pos of the ordered list gets
// the row (list) and/or its key (keys_out: slot_keys[r], or the array
// layout's r * shard_num + shard_id); out_cap bounds both
template <int MODE>
__global__ __launch_bounds__(BLOCK)
void k_expire_compact(const unsigned char* __restrict__ dead, long R,
                      const int* __restrict__ nrows_dev,
                      const unsigned char* __restrict__ valid,
                      const int* __restrict__ cnt,
                      const int* __restrict__ tile_incl,
                      int* __restrict__ list, i64* __restrict__ keys_out,
                      const i64* __restrict__ slot_keys, long shard_num,
                      long shard_id, long out_cap) {
    __shared__ int wcnt[DT_ITEMS * DT_WAVES];
    __shared__ int off[DT_ITEMS * DT_WAVES];
    long live = delta_live(nrows_dev, R);
    long np = MODE == XP_DEAD ? 0 : (long)cnt[1];
    long base = (long)blockIdx.x * DT_TILE + threadIdx.x;
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;
    bool p[DT_ITEMS];
    int rank[DT_ITEMS];
#pragma unroll
    for (int i = 0; i < DT_ITEMS; ++i) {
        p[i] = expire_pred<MODE>(dead, base + (long)i * BLOCK, R, live, np,
                                 valid);
        u64 b = __ballot(p[i]);
        rank[i] = __popcll(b & below);
        if (lane == 0) wcnt[i * DT_WAVES + wave] = __popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int j = 0; j < DT_ITEMS * DT_WAVES; ++j) {
            off[j] = run;
            run += wcnt[j];
        }
    }
    __syncthreads();
    long tile_base = blockIdx.x ? (long)tile_incl[blockIdx.x - 1] : 0;
#pragma unroll
    for (int i = 0; i < DT_ITEMS; ++i) {
        if (!p[i]) continue;
        long r = base + (long)i * BLOCK;
        long pos = tile_base + off[i * DT_WAVES + wave] + rank[i];
        if (pos < 0 || pos >= out_cap) continue;
        if (list) list[pos] = (int)r;
        if (keys_out)
            keys_out[pos] = slot_keys ? slot_keys[r]
                                      : r * shard_num + shard_id;
    }
}

// Row move over one plane of 32-bit words: row movers[i] -> row holes[i] for
// i < *count_dev, one G-lane group per row, coalesced along the row. Every
// source lies in [n', n) and every destination in [0, n'): the two ranges
// are disjoint, no row is both read and written, so the parallel in-place
// move is race free in any order (the dst < src test below enforces it).
template <int G>
__global__ void k_move_rows(unsigned* __restrict__ base, long R, long wpr,
                            const int* __restrict__ holes,
                            const int* __restrict__ movers, long cap,
                            const int* __restrict__ count_dev) {
    long g = ((long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    int lane = threadIdx.x % G;
    if (g >= cap || g >= (long)*count_dev) return;
    long dst = holes[g], src = movers[g];
    if (dst < 0 || dst >= src || src >= R) return;
    const unsigned* s = base + (u64)src * wpr;
    unsigned* d = base + (u64)dst * wpr;
    for (long j = lane; j < wpr; j += G) d[j] = s[j];
}

// Probe table rebuild after a removal: tk was filled with EMPTY; one thread
// per surviving slot s < n' inserts (slot_keys[s], s) with a bounded-probe
// CAS, like k_ht_rehash. The capacity is unchanged, so the load factor only
// falls. n' comes from cnt (not from nrows_dev), and thread 0 publishes it
// to nrows_dev, which no thread of this kernel reads.
__global__ void k_ht_build(u64* __restrict__ tk, int* __restrict__ tv,
                           long mask, const i64* __restrict__ slot_keys,
                           long R, const int* __restrict__ cnt,
                           int* __restrict__ nrows_dev) {
    long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long np = (long)cnt[1];
    if (s == 0) *nrows_dev = (int)np;
    if (s >= np || s >= R) return;
    u64 k = (u64)slot_keys[s];
    if (k == EMPTY) return;
    u64 h = splitmix64(k) & (u64)mask;
    for (long p = 0; p <= mask; ++p) {
        u64 prev = atomicCAS(&tk[h], EMPTY, k);
        if (prev == EMPTY) { tv[h] = (int)s; return; }
        h = (h + 1) & (u64)mask;
    }
}

// array table: the flagged live rows stop being valid
__global__ void k_expire_array(unsigned char* __restrict__ valid,
                               const unsigned char* __restrict__ dead,
                               long R) {
    long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R && dead[r]) valid[r] = 0;
}

// ============================================================== launchers

// shared dispatch ladder of the plain and the bag-indirected reduce
template <bool BAG, bool WEIGHTED = false>
static void reduce_dispatch(const i64* inverse, const float* grads, long n,
                            long dim, float* ugrads, u64* counts, long u,
                            const int* bag_of, const i64* offsets, long B,
                            int mode, hipStream_t stream,
                            const float* weights = nullptr,
                            const float* bag_scale = nullptr) {
    {
        long ne = u * dim;
        long mx = ne > u ? ne : u;
        if (mx) k_reduce_reset<<<(int)((mx + 255) / 256), 256, 0, stream>>>(
            ugrads, ne, counts, u);
    }
    if (n == 0) return;
    int grid = cdiv(n, BLOCK);
    // H must cover the block's worst-case distinct uids (BLOCK = 256):
    // an undersized hash overflows most elements to DIRECT global atomics
    // — measured 360 us/call at dim 65 with H=64 (75% overflow) vs the
    // LDS-aggregated path's ~tens of us (profiles/bench_deepfm_dim64)
    if (dim <= 16) {
        // G=8: halves the serial per-group element chain vs G=16
        // (nj = ceil(16/8) = 2 fragments)
        const int H = 512;
        size_t smem = H * 8 + (size_t)H * dim * 4;   // <= 40 KiB
        k_reduce_lds<H, 8, 4, BAG, WEIGHTED><<<grid, BLOCK, smem, stream>>>(
            inverse, grads, n, dim, ugrads, counts, bag_of, offsets, B,
            mode, weights, bag_scale);
    } else if (dim <= 96) {
        // G=16: quarter-length serial element chain vs G=64 (each group
        // walks its G elements in order); GF=8 staging slots cover
        // ceil(96/16)=6 fragments
        const int H = 256;
        size_t smem = H * 8 + (size_t)H * dim * 4;   // <= 98 KiB
        k_reduce_lds<H, 16, 8, BAG, WEIGHTED><<<grid, BLOCK, smem, stream>>>(
            inverse, grads, n, dim, ugrads, counts, bag_of, offsets, B,
            mode, weights, bag_scale);
    } else if (dim <= 128) {
        const int H = 128;
        size_t smem = H * 8 + (size_t)H * dim * 4;   // <= 66 KiB
        k_reduce_lds<H, 64, 4, BAG, WEIGHTED><<<grid, BLOCK, smem, stream>>>(
            inverse, grads, n, dim, ugrads, counts, bag_of, offsets, B,
            mode, weights, bag_scale);
    } else {
        k_reduce_grads<BAG, WEIGHTED><<<grid1d(n * dim), BLOCK, 0, stream>>>(
            inverse, grads, n, dim, ugrads, bag_of, offsets, B, mode,
            weights, bag_scale);
        k_reduce_counts<BAG><<<grid1d(n), BLOCK, 0, stream>>>(
            inverse, n, counts, bag_of, B);
    }
}

// shared dispatch ladder of the plain and the weighted pooled gather;
// map_kind: 0 = none, 1 = int64 (table slots), 2 = int32 (padded pos_of)
template <bool WEIGHTED>
static void pool_dispatch(const float* rows, long R, long dim,
                          const i64* inverse, long nnz, const void* map,
                          int map_kind, long u, const i64* offsets, long B,
                          int mode, float* out, int* bag_of,
                          const float* weights, float* bag_scale,
                          hipStream_t stream) {
    if (B == 0 && (!bag_of || nnz == 0)) return;
#define LAUNCH_POOL(G, CF, ILP)                                             \
    do {                                                                    \
        int gg = grid1d((B > 0 ? B : 1) * G);                               \
        if (map_kind == 2)                                                  \
            k_pool_fwd<G, CF, ILP, int, WEIGHTED><<<gg, BLOCK, 0, stream>>>(\
                rows, R, dim, inverse, nnz, (const int*)map, u, offsets, B, \
                mode, out, bag_of, weights, bag_scale);                     \
        else                                                                \
            k_pool_fwd<G, CF, ILP, i64, WEIGHTED><<<gg, BLOCK, 0, stream>>>(\
                rows, R, dim, inverse, nnz,                                 \
                map_kind ? (const i64*)map : nullptr, u, offsets, B, mode,  \
                out, bag_of, weights, bag_scale);                           \
    } while (0)
    // G as in emb_gather_init (16 lanes up to dim 32, a full wave above);
    // every rung keeps 16 row values in flight per lane
    if (dim <= 16) LAUNCH_POOL(16, 1, 16);
    else if (dim <= 32) LAUNCH_POOL(16, 2, 8);
    else if (dim <= 64) LAUNCH_POOL(64, 1, 16);
    else if (dim <= 128) LAUNCH_POOL(64, 2, 8);
    else LAUNCH_POOL(64, 4, 4);   // dim > 256 loops over column passes
#undef LAUNCH_POOL
}

// the same ladder for the read-only lookup; Resolve is the key -> row policy
template <bool WEIGHTED, typename Resolve>
static void pool_lookup_dispatch(const float* rows, long dim, long nnz,
                                 const i64* offsets, long B, int mode,
                                 const float* weights, float* out,
                                 const Resolve& resolve,
                                 hipStream_t stream) {
    if (B == 0) return;
#define LAUNCH_LOOKUP(G, CF, ILP)                                           \
    k_pool_lookup<G, CF, ILP, WEIGHTED, Resolve>                            \
        <<<grid1d(B * G), BLOCK, 0, stream>>>(rows, dim, nnz, offsets, B,   \
                                              mode, weights, out, resolve)
    if (dim <= 16) LAUNCH_LOOKUP(16, 1, 16);
    else if (dim <= 32) LAUNCH_LOOKUP(16, 2, 8);
    else if (dim <= 64) LAUNCH_LOOKUP(64, 1, 16);
    else if (dim <= 128) LAUNCH_LOOKUP(64, 2, 8);
    else LAUNCH_LOOKUP(64, 4, 4);
#undef LAUNCH_LOOKUP
}

// The group ladders of the packed kernels go by a row's dword count
// (ceil(dim / 4) for int8, ceil(dim / 2) for fp16). The row-parallel
// kernels (quantize, flat gather): 4 lanes up to 4 dwords (a dim-9 int8 row
// is three), 16 up to 16, 32 up to 32, a wave above.
#define Q_ROW_LADDER(ndw, LAUNCH)                                           \
    do {                                                                    \
        if ((ndw) <= 4) LAUNCH(4);                                          \
        else if ((ndw) <= 16) LAUNCH(16);                                   \
        else if ((ndw) <= 32) LAUNCH(32);                                   \
        else LAUNCH(64);                                                    \
    } while (0)

template <int FMT>
static void quantize_dispatch(const float* w, long n, long dim,
                              const i64* slots, unsigned int* slab, long R,
                              hipStream_t stream) {
#define LAUNCH_QUANT(G)                                                     \
    k_quantize_rows<FMT, G><<<grid1d(n * G), BLOCK, 0, stream>>>(           \
        w, n, dim, slots, slab, R)
    Q_ROW_LADDER(QFmt<FMT>::code_dwords(dim), LAUNCH_QUANT);
#undef LAUNCH_QUANT
}

template <int FMT, bool WEIGHTED, typename Resolve>
static void pool_lookup_q_dispatch(const unsigned int* slab, long dim,
                                   long nnz, const i64* offsets, long B,
                                   int mode, const float* weights, float* out,
                                   const Resolve& resolve,
                                   hipStream_t stream) {
    if (B == 0) return;
#define LAUNCH_LOOKUP_Q(G, CF, ILP)                                         \
    k_pool_lookup_q<FMT, G, CF, ILP, WEIGHTED, Resolve>                     \
        <<<grid1d(B * G), BLOCK, 0, stream>>>(slab, dim, nnz, offsets, B,   \
                                              mode, weights, out, resolve)
    // The pooled lookup: 16 lanes up to 16 dwords, 32 up to 32, a wave
    // above, two fragments per lane from 65 dwords, wider rows loop. There
    // is no 4-lane rung: a group probes G keys per dependent round, and
    // a bag of 32 walked four keys at a time measured 88 us against 38 us
    // for the fp32 lookup's 16 lanes (profiles/serving_quantized.md)
    const long ndw = QFmt<FMT>::code_dwords(dim);
    if (ndw <= 16) LAUNCH_LOOKUP_Q(16, 1, 8);
    else if (ndw <= 32) LAUNCH_LOOKUP_Q(32, 1, 8);
    else if (ndw <= 64) LAUNCH_LOOKUP_Q(64, 1, 8);
    else LAUNCH_LOOKUP_Q(64, 2, 4);
#undef LAUNCH_LOOKUP_Q
}

template <int FMT, typename Resolve>
static void pool_lookup_q_fmt(const unsigned int* slab, long dim, long nnz,
                              const i64* offsets, long B, int mode,
                              const float* weights, float* out,
                              const Resolve& resolve, hipStream_t stream) {
    if (weights)
        pool_lookup_q_dispatch<FMT, true>(slab, dim, nnz, offsets, B, mode,
                                          weights, out, resolve, stream);
    else
        pool_lookup_q_dispatch<FMT, false>(slab, dim, nnz, offsets, B, mode,
                                           nullptr, out, resolve, stream);
}

template <int FMT, typename Resolve>
static void gather_lookup_q_fmt(const unsigned int* slab, long dim, long n,
                                float* out, const Resolve& resolve,
                                hipStream_t stream) {
#define LAUNCH_GATHER_Q(G)                                                  \
    k_gather_lookup_q<FMT, G, Resolve>                                      \
        <<<grid1d(n * G), BLOCK, 0, stream>>>(slab, dim, n, out, resolve)
    Q_ROW_LADDER(QFmt<FMT>::code_dwords(dim), LAUNCH_GATHER_Q);
#undef LAUNCH_GATHER_Q
}

// ``tch`` non-null is the form that stops after assign (with the array
// touch inside it when tch->valid is set): the caller's k_pull_merged
// resolves slot_of -> tv itself and files the elements.
template <bool IDX>
static void unique_launch(const i64* keys, long n, u64* tk, int* tv, long cap,
                          int* slot_of, unsigned char* is_first,
                          i64* unique_keys, i64* inverse, int* counter,
                          const i64* foff, int F, const UIdx& ix,
                          hipStream_t stream, const UTouch* tch = nullptr) {
    // fill kernel, not hipMemsetAsync: memsets issued here were NOT
    // replayed inside hipGraph captures (scratch kept stale keys across
    // replays until the probe loops hung); kernels always capture. One
    // fused launch — the three separate fills were each ~4.5 us of
    // launch/ramp in the step (profiles/step_attrib_r2.txt)
    {
        long mx = cap > n ? cap : n;
        k_unique_reset<IDX><<<(int)((mx + 255) / 256), 256, 0, stream>>>(
            tk, cap, is_first, n, counter, ix);
    }
    long mask = cap - 1;
    k_unique_insert<IDX><<<grid1d(n), BLOCK, 0, stream>>>(
        keys, n, tk, mask, slot_of, is_first, foff, F, ix);
    int ga = grid1d((n + UA_ITERS - 1) / UA_ITERS);
    int gi = grid1d((n + UI_ILP - 1) / UI_ILP);
    if (tch) {
        if (IDX && tch->valid)
            k_unique_assign<IDX, IDX><<<ga, BLOCK, 0, stream>>>(
                keys, n, slot_of, is_first, tv, unique_keys, counter,
                inverse, foff, F, ix, *tch);
        else
            k_unique_assign<IDX><<<ga, BLOCK, 0, stream>>>(
                keys, n, slot_of, is_first, tv, unique_keys, counter,
                inverse, foff, F, ix, UTouch{});
        return;
    }
    k_unique_assign<IDX><<<ga, BLOCK, 0, stream>>>(
        keys, n, slot_of, is_first, tv, unique_keys, counter, inverse, foff,
        F, ix, UTouch{});
    k_unique_inverse<IDX><<<gi, BLOCK, 0, stream>>>(n, slot_of, tv, inverse,
                                                    ix);
}

extern "C" {

void emb_unique(const i64* keys, long n, u64* tk, int* tv, long cap,
                int* slot_of, unsigned char* is_first, i64* unique_keys,
                i64* inverse, int* counter, const i64* foff, int F,
                hipStream_t stream) {
    unique_launch<false>(keys, n, tk, tv, cap, slot_of, is_first,
                         unique_keys, inverse, counter, foff, F, UIdx{},
                         stream);
}

// The same dedup, which also files every element under its uid (the
// inverted index that emb_reduce_by_index sums through). tcount/toff [cap]
// and rank [n] are scratch; long_list has long_cap >= n / (SEG_T + 1) + 1
// entries, which no batch of n elements can exceed.
void emb_unique_indexed(const i64* keys, long n, u64* tk, int* tv, long cap,
                        int* slot_of, unsigned char* is_first,
                        i64* unique_keys, i64* inverse, int* counter,
                        const i64* foff, int F, int* tcount, int* toff,
                        int* rank, int* seg_off, int* seg_cnt, int* perm,
                        int* long_list, long long_cap, int* off_counter,
                        int* n_long, hipStream_t stream) {
    UIdx ix{tcount, toff, rank, seg_off, seg_cnt, perm, long_list,
            off_counter, n_long, long_cap};
    unique_launch<true>(keys, n, tk, tv, cap, slot_of, is_first, unique_keys,
                        inverse, counter, foff, F, ix, stream);
}

// emb_unique_indexed without its last kernel, for k_pull_merged: stops
// after k_unique_assign, which also touches the array table when ``valid``
// is given (slots / new_mask [n] per uid; their tail is emb_pull_merged's).
// slot_of, tv, toff and rank are then the merged kernel's inputs; inverse
// holds only the entries the assign kernel stores itself.
void emb_unique_indexed_assign(const i64* keys, long n, u64* tk, int* tv,
                               long cap, int* slot_of,
                               unsigned char* is_first, i64* unique_keys,
                               i64* inverse, int* counter, const i64* foff,
                               int F, int* tcount, int* toff, int* rank,
                               int* seg_off, int* seg_cnt, int* perm,
                               int* long_list, long long_cap,
                               int* off_counter, int* n_long,
                               unsigned char* valid, long shard_num,
                               long table_cap, i64* slots,
                               unsigned char* new_mask, hipStream_t stream) {
    UIdx ix{tcount, toff, rank, seg_off, seg_cnt, perm, long_list,
            off_counter, n_long, long_cap};
    UTouch tch{valid, shard_num, table_cap, slots, new_mask};
    unique_launch<true>(keys, n, tk, tv, cap, slot_of, is_first, unique_keys,
                        inverse, counter, foff, F, ix, stream, &tch);
}

// The rest of the pull after emb_unique_indexed_assign (and, for hash
// tables, emb_ht_lookup): inverse, the index's perm and gather/init in one
// launch. ``array`` != 0 takes the slot from the element's own key and
// writes the tail of slots / new_mask; otherwise slots [n] is read per uid.
void emb_pull_merged(float* weights, float* state, long dim, long sd,
                     const i64* keys, const i64* foff, int F, long n,
                     const int* slot_of, const int* tv, const int* toff,
                     const int* rank, i64* inverse, int* perm, i64* slots,
                     unsigned char* new_mask, int array, long shard_num,
                     long table_cap, float* out, int init_cat, float p0,
                     float p1, float p2, u64 seed,
                     const float* state_init_row, const int* u_dev,
                     hipStream_t stream) {
    if (n == 0) return;
    long npg = (n + GI_ILP - 1) / GI_ILP;
#define LAUNCH_PM(G, SP)                                                    \
    k_pull_merged<G><<<grid1d(npg * G), BLOCK, 0, stream>>>(                \
        weights, state, dim, sd, keys, foff, F, n, slot_of, tv, toff, rank, \
        inverse, perm, new_mask, SP, out, init_cat, p0, p1, p2, seed,       \
        state_init_row, u_dev)
    if (array) {
        SlotArray sp{shard_num, table_cap, slots, new_mask};
        if (dim <= 32) LAUNCH_PM(16, sp); else LAUNCH_PM(64, sp);
    } else {
        SlotMap sp{slots};
        if (dim <= 32) LAUNCH_PM(16, sp); else LAUNCH_PM(64, sp);
    }
#undef LAUNCH_PM
}

int emb_seg_threshold() { return SEG_T; }
int emb_seg_max_dim() { return SEG_MAX_DIM; }

// Per-unique sums and counts through the inverted index: what
// emb_reduce_by_inverse gives for u = n, without its reset launch.
// dim <= SEG_MAX_DIM (the caller checks).
void emb_reduce_by_index(const int* seg_off, const int* seg_cnt,
                         const int* perm, const int* long_list,
                         const int* n_long, long long_cap,
                         const float* grads, long n, long dim,
                         const int* u_dev, float* ugrads, u64* counts,
                         hipStream_t stream) {
    if (n == 0) return;
    int lb = (int)(long_cap < SEG_LONG_BLOCKS ? long_cap : SEG_LONG_BLOCKS);
    long groups = (n + SR_ILP - 1) / SR_ILP;
#define LAUNCH_SEG(G, CF)                                                   \
    k_seg_reduce<G, CF>                                                     \
        <<<lb + cdiv(groups * G, SEG_BLOCK), SEG_BLOCK, 0, stream>>>(       \
            seg_off, seg_cnt, perm, long_list, n_long, long_cap, lb, grads, \
            n, dim, u_dev, ugrads, counts)
    // G as in emb_gather_init: 16 lanes up to dim 32, a full wave above
    if (dim <= 16) LAUNCH_SEG(16, 1);
    else if (dim <= 32) LAUNCH_SEG(16, 2);
    else if (dim <= 64) LAUNCH_SEG(64, 1);
    else LAUNCH_SEG(64, 2);
#undef LAUNCH_SEG
}

void emb_ht_lookup(u64* tk, int* tv, long cap, const i64* keys, long n,
                   int* nrows, i64* slot_keys, i64* slots,
                   unsigned char* new_mask, int insert, const int* u_dev,
                   long row_cap, hipStream_t stream) {
    k_ht_lookup<<<grid1d(n), BLOCK, 0, stream>>>(tk, tv, cap - 1, keys, n,
                                                 nrows, slot_keys, slots,
                                                 new_mask, insert, u_dev,
                                                 row_cap);
}

// slots doubles as the hand-over between the two launches (ADMIT_PENDING)
void emb_ht_lookup_admit(u64* tk, int* tv, long cap, const i64* keys, long n,
                         int* nrows, i64* slot_keys, long row_cap,
                         int* sketch, long W, int D, u64 seed, int min_count,
                         u64* stats, i64* slots, unsigned char* new_mask,
                         const int* u_dev, hipStream_t stream) {
    k_admit_note<<<grid1d(n), BLOCK, 0, stream>>>(tk, tv, cap - 1, keys, n,
                                                  sketch, W, D, seed, slots,
                                                  new_mask, u_dev);
    k_admit_resolve<<<grid1d(n), BLOCK, 0, stream>>>(
        tk, tv, cap - 1, keys, n, sketch, W, D, seed, min_count, nrows,
        slot_keys, row_cap, slots, new_mask, stats);
}

void emb_admit_age(int* sketch, long n, int shift, hipStream_t stream) {
    // one thread per four counters; the first three also take the tail
    int grid = grid1d((n >> 2) > 3 ? (n >> 2) : 3);
    if (n) k_admit_age<<<grid, BLOCK, 0, stream>>>(sketch, n, shift);
}

void emb_ht_rehash(const u64* tk_old, const int* tv_old, long cap_old,
                   u64* tk_new, int* tv_new, long cap_new,
                   hipStream_t stream) {
    fill_u64(tk_new, cap_new, EMPTY, stream);
    k_ht_rehash<<<grid1d(cap_old), BLOCK, 0, stream>>>(
        tk_old, tv_old, cap_old, tk_new, tv_new, cap_new - 1);
}

void emb_array_touch(unsigned char* valid, const i64* keys, long n,
                     long shard_num, long cap, i64* slots,
                     unsigned char* new_mask, const int* u_dev,
                     hipStream_t stream) {
    k_array_touch<<<grid1d(n), BLOCK, 0, stream>>>(valid, keys, n, shard_num,
                                                   cap, slots, new_mask,
                                                   u_dev);
}

void emb_gather_init(float* weights, float* state, long dim, long sd,
                     const i64* slots, const unsigned char* new_mask,
                     const i64* keys, long n, const i64* inverse, float* out,
                     int init_cat, float p0, float p1, float p2, u64 seed,
                     const float* state_init_row, const int* u_dev,
                     hipStream_t stream) {
    if (n == 0) return;
    long npg = (n + GI_ILP - 1) / GI_ILP;
    if (dim <= 32) {
        int gg = grid1d(npg * 16);
        k_gather_init<16><<<gg, BLOCK, 0, stream>>>(
            weights, state, dim, sd, slots, new_mask, keys, n, inverse, out,
            init_cat, p0, p1, p2, seed, state_init_row, u_dev);
    } else {
        int gg = grid1d(npg * 64);
        k_gather_init<64><<<gg, BLOCK, 0, stream>>>(
            weights, state, dim, sd, slots, new_mask, keys, n, inverse, out,
            init_cat, p0, p1, p2, seed, state_init_row, u_dev);
    }
}

void emb_reduce_by_inverse(const i64* inverse, const float* grads, long n,
                           long dim, float* ugrads, u64* counts, long u,
                           hipStream_t stream) {
    reduce_dispatch<false>(inverse, grads, n, dim, ugrads, counts, u,
                           nullptr, nullptr, 0, 0, stream);
}

// grads is the pooled [B, dim] gradient; n = number of elements (nnz)
void emb_reduce_bags_by_inverse(const i64* inverse, const float* grad_out,
                                long n, long dim, const int* bag_of,
                                const i64* offsets, long B, int mode,
                                float* ugrads, u64* counts, long u,
                                hipStream_t stream) {
    reduce_dispatch<true>(inverse, grad_out, n, dim, ugrads, counts, u,
                          bag_of, offsets, B, mode, stream);
}

// map_kind: 0 = none, 1 = int64 (table slots), 2 = int32 (padded pos_of)
void emb_pool_fwd(const float* rows, long R, long dim, const i64* inverse,
                  long nnz, const void* map, int map_kind, long u,
                  const i64* offsets, long B, int mode, float* out,
                  int* bag_of, hipStream_t stream) {
    pool_dispatch<false>(rows, R, dim, inverse, nnz, map, map_kind, u,
                         offsets, B, mode, out, bag_of, nullptr, nullptr,
                         stream);
}

// weighted pool: also writes bag_scale [B]
void emb_pool_fwd_weighted(const float* rows, long R, long dim,
                           const i64* inverse, long nnz, const void* map,
                           int map_kind, long u, const i64* offsets, long B,
                           int mode, const float* weights, float* out,
                           int* bag_of, float* bag_scale,
                           hipStream_t stream) {
    pool_dispatch<true>(rows, R, dim, inverse, nnz, map, map_kind, u,
                        offsets, B, mode, out, bag_of, weights, bag_scale,
                        stream);
}

// read-only pooled lookup, values -> out in one launch. tk != null: hash
// table (tk/tv, cap a power of two); else array table (valid [cap],
// shard_num >= 1). weights null = plain pool.
void emb_pool_lookup(const float* rows, long R, long dim, const i64* values,
                     long nnz, const i64* offsets, long B, int mode,
                     const float* weights, const u64* tk, const int* tv,
                     long cap, const unsigned char* valid, long shard_num,
                     float* out, hipStream_t stream) {
    if (tk) {
        const PoolHashKeys r{values, tk, tv, cap - 1, R};
        if (weights)
            pool_lookup_dispatch<true>(rows, dim, nnz, offsets, B, mode,
                                       weights, out, r, stream);
        else
            pool_lookup_dispatch<false>(rows, dim, nnz, offsets, B, mode,
                                        nullptr, out, r, stream);
    } else {
        const PoolArrayKeys r{values, valid, shard_num, cap, R};
        if (weights)
            pool_lookup_dispatch<true>(rows, dim, nnz, offsets, B, mode,
                                       weights, out, r, stream);
        else
            pool_lookup_dispatch<false>(rows, dim, nnz, offsets, B, mode,
                                        nullptr, out, r, stream);
    }
}

// ---- quantized serving tables
long emb_quant_stride(int fmt, long dim) {
    return fmt == QF_INT8 ? QFmt<QF_INT8>::stride(dim)
                          : QFmt<QF_FP16>::stride(dim);
}

// fp32 rows w [n, dim] -> packed rows slots[i] of slab [R, stride(fmt, dim)]
void emb_quantize_rows(int fmt, const float* w, long n, long dim,
                       const i64* slots, void* slab, long R,
                       hipStream_t stream) {
    if (n == 0) return;
    if (fmt == QF_INT8)
        quantize_dispatch<QF_INT8>(w, n, dim, slots, (unsigned int*)slab, R,
                                   stream);
    else
        quantize_dispatch<QF_FP16>(w, n, dim, slots, (unsigned int*)slab, R,
                                   stream);
}

// read-only pooled lookup over a packed slab [R, stride(fmt, dim)]; the
// table arguments are emb_pool_lookup's
void emb_pool_lookup_q(int fmt, const void* slab, long R, long dim,
                       const i64* values, long nnz, const i64* offsets,
                       long B, int mode, const float* weights, const u64* tk,
                       const int* tv, long cap, const unsigned char* valid,
                       long shard_num, float* out, hipStream_t stream) {
    if (R == 0) {   // nothing to read (the kernel reads row 0 for a miss)
        fill_f32(out, B * dim, 0.0f, stream);
        return;
    }
    const unsigned int* s = (const unsigned int*)slab;
    if (tk) {
        const PoolHashKeys r{values, tk, tv, cap - 1, R};
        if (fmt == QF_INT8)
            pool_lookup_q_fmt<QF_INT8>(s, dim, nnz, offsets, B, mode,
                                       weights, out, r, stream);
        else
            pool_lookup_q_fmt<QF_FP16>(s, dim, nnz, offsets, B, mode,
                                       weights, out, r, stream);
    } else {
        const PoolArrayKeys r{values, valid, shard_num, cap, R};
        if (fmt == QF_INT8)
            pool_lookup_q_fmt<QF_INT8>(s, dim, nnz, offsets, B, mode,
                                       weights, out, r, stream);
        else
            pool_lookup_q_fmt<QF_FP16>(s, dim, nnz, offsets, B, mode,
                                       weights, out, r, stream);
    }
}

// flat read over a packed slab: keys [n] -> out [n, dim], zeros for a miss
void emb_gather_lookup_q(int fmt, const void* slab, long R, long dim,
                         const i64* keys, long n, const u64* tk,
                         const int* tv, long cap, const unsigned char* valid,
                         long shard_num, float* out, hipStream_t stream) {
    if (n == 0) return;
    if (R == 0) {   // nothing to read (the kernel reads row 0 for a miss)
        fill_f32(out, n * dim, 0.0f, stream);
        return;
    }
    const unsigned int* s = (const unsigned int*)slab;
    if (tk) {
        const PoolHashKeys r{keys, tk, tv, cap - 1, R};
        if (fmt == QF_INT8)
            gather_lookup_q_fmt<QF_INT8>(s, dim, n, out, r, stream);
        else
            gather_lookup_q_fmt<QF_FP16>(s, dim, n, out, r, stream);
    } else {
        const PoolArrayKeys r{keys, valid, shard_num, cap, R};
        if (fmt == QF_INT8)
            gather_lookup_q_fmt<QF_INT8>(s, dim, n, out, r, stream);
        else
            gather_lookup_q_fmt<QF_FP16>(s, dim, n, out, r, stream);
    }
}

// weighted pooled backward: element e's factor is
// weights[e] * bag_scale[bag_of[e]]
void emb_reduce_bags_weighted_by_inverse(const i64* inverse,
                                         const float* grad_out, long n,
                                         long dim, const int* bag_of,
                                         const float* weights,
                                         const float* bag_scale, long B,
                                         float* ugrads, u64* counts, long u,
                                         hipStream_t stream) {
    reduce_dispatch<true, true>(inverse, grad_out, n, dim, ugrads, counts, u,
                                bag_of, nullptr, B, 0, stream, weights,
                                bag_scale);
}

// gradient of the weighted pool w.r.t. the per-sample weights, dw [nnz]
void emb_pool_wgrad(const float* rows, long R, long dim, const i64* inverse,
                    long nnz, const void* map, int map_kind, long u,
                    const float* weights, const int* bag_of,
                    const float* bag_scale, const float* out,
                    const float* grad_out, long B, int mode, float* dw,
                    hipStream_t stream) {
    if (nnz == 0) return;
#define LAUNCH_WGRAD(G)                                                     \
    do {                                                                    \
        int gg = grid1d(nnz * G);                                           \
        if (map_kind == 2)                                                  \
            k_pool_wgrad<G, int><<<gg, BLOCK, 0, stream>>>(                 \
                rows, R, dim, inverse, nnz, (const int*)map, u, weights,    \
                bag_of, bag_scale, out, grad_out, B, mode, dw);             \
        else                                                                \
            k_pool_wgrad<G, i64><<<gg, BLOCK, 0, stream>>>(                 \
                rows, R, dim, inverse, nnz,                                 \
                map_kind ? (const i64*)map : nullptr, u, weights, bag_of,   \
                bag_scale, out, grad_out, B, mode, dw);                     \
    } while (0)
    // G as on the gather ladder
    if (dim <= 32) LAUNCH_WGRAD(16);
    else LAUNCH_WGRAD(64);
#undef LAUNCH_WGRAD
}

#define LAUNCH_OPT(G, OPT)                                                  \
    k_apply_opt<G, OPT><<<grid1d(n * G), BLOCK, 0, stream>>>(               \
        weights, state, dim, sd, slots, n, grads, counts, c[0], c[1], c[2], \
        c[3], c[4], c[5], c[6], u_dev)

void emb_apply_optimizer(int opt, float* weights, float* state, long dim,
                         long sd, const i64* slots, long n,
                         const float* grads, const u64* counts,
                         const float* c, const int* u_dev,
                         hipStream_t stream) {
    if (n == 0) return;
    if (dim <= 32) {
        const int G = 16;
        switch (opt) {
            case OPT_DEFAULT: LAUNCH_OPT(16, OPT_DEFAULT); break;
            case OPT_ADADELTA: LAUNCH_OPT(16, OPT_ADADELTA); break;
            case OPT_ADAGRAD: LAUNCH_OPT(16, OPT_ADAGRAD); break;
            case OPT_ADAM: LAUNCH_OPT(16, OPT_ADAM); break;
            case OPT_ADAMAX: LAUNCH_OPT(16, OPT_ADAMAX); break;
            case OPT_FTRL: LAUNCH_OPT(16, OPT_FTRL); break;
            case OPT_RMSPROP: LAUNCH_OPT(16, OPT_RMSPROP); break;
            case OPT_SGD: LAUNCH_OPT(16, OPT_SGD); break;
            case OPT_TEST: LAUNCH_OPT(16, OPT_TEST); break;
        }
        (void)G;
    } else {
        const int G = 64;
        switch (opt) {
            case OPT_DEFAULT: LAUNCH_OPT(64, OPT_DEFAULT); break;
            case OPT_ADADELTA: LAUNCH_OPT(64, OPT_ADADELTA); break;
            case OPT_ADAGRAD: LAUNCH_OPT(64, OPT_ADAGRAD); break;
            case OPT_ADAM: LAUNCH_OPT(64, OPT_ADAM); break;
            case OPT_ADAMAX: LAUNCH_OPT(64, OPT_ADAMAX); break;
            case OPT_FTRL: LAUNCH_OPT(64, OPT_FTRL); break;
            case OPT_RMSPROP: LAUNCH_OPT(64, OPT_RMSPROP); break;
            case OPT_SGD: LAUNCH_OPT(64, OPT_SGD); break;
            case OPT_TEST: LAUNCH_OPT(64, OPT_TEST); break;
        }
        (void)G;
    }
}

// emb_reduce_by_index + emb_apply_optimizer in one launch: nothing per
// unique leaves the kernel but the table rows. dim <= SEG_MAX_DIM (the
// caller checks); an unknown ``opt`` launches nothing.
void emb_reduce_apply_by_index(int opt, const int* seg_off,
                               const int* seg_cnt, const int* perm,
                               const int* long_list, const int* n_long,
                               long long_cap, const float* grads, long n,
                               long dim, const int* u_dev, const i64* slots,
                               float* weights, float* state, long sd,
                               const float* c, hipStream_t stream) {
    if (n == 0) return;
    int lb = (int)(long_cap < SEG_LONG_BLOCKS ? long_cap : SEG_LONG_BLOCKS);
    long groups = (n + SR_ILP - 1) / SR_ILP;
#define LAUNCH_SEG_OPT(G, CF, OPT)                                          \
    k_seg_reduce_apply<G, CF, OPT>                                          \
        <<<lb + cdiv(groups * G, SEG_BLOCK), SEG_BLOCK, 0, stream>>>(       \
            seg_off, seg_cnt, perm, long_list, n_long, long_cap, lb, grads, \
            n, dim, u_dev, slots, weights, state, sd, c[0], c[1], c[2],     \
            c[3], c[4], c[5], c[6])
#define SWITCH_SEG_OPT(G, CF)                                               \
    switch (opt) {                                                          \
        case OPT_DEFAULT: LAUNCH_SEG_OPT(G, CF, OPT_DEFAULT); break;        \
        case OPT_ADADELTA: LAUNCH_SEG_OPT(G, CF, OPT_ADADELTA); break;      \
        case OPT_ADAGRAD: LAUNCH_SEG_OPT(G, CF, OPT_ADAGRAD); break;        \
        case OPT_ADAM: LAUNCH_SEG_OPT(G, CF, OPT_ADAM); break;              \
        case OPT_ADAMAX: LAUNCH_SEG_OPT(G, CF, OPT_ADAMAX); break;          \
        case OPT_FTRL: LAUNCH_SEG_OPT(G, CF, OPT_FTRL); break;              \
        case OPT_RMSPROP: LAUNCH_SEG_OPT(G, CF, OPT_RMSPROP); break;        \
        case OPT_SGD: LAUNCH_SEG_OPT(G, CF, OPT_SGD); break;                \
        case OPT_TEST: LAUNCH_SEG_OPT(G, CF, OPT_TEST); break;              \
    }
    // the rungs of emb_reduce_by_index; G is emb_apply_optimizer's too
    if (dim <= 16) { SWITCH_SEG_OPT(16, 1) }
    else if (dim <= 32) { SWITCH_SEG_OPT(16, 2) }
    else if (dim <= 64) { SWITCH_SEG_OPT(64, 1) }
    else { SWITCH_SEG_OPT(64, 2) }
#undef SWITCH_SEG_OPT
#undef LAUNCH_SEG_OPT
}

void emb_mask_tail(i64* keys, float* grads, u64* counts, long n, long dim,
                   const int* u_dev, hipStream_t stream) {
    if (n)
        k_mask_tail<<<grid1d(n * dim), BLOCK, 0, stream>>>(keys, grads,
                                                           counts, n, dim,
                                                           u_dev);
}

void emb_mark_rows(const i64* slots, long n, const unsigned char* mask,
                   const int* u_dev, const int* epoch_dev, int* row_epoch,
                   long R, hipStream_t stream) {
    if (n && R)
        k_mark_rows<<<grid1d(n), BLOCK, 0, stream>>>(slots, n, mask, u_dev,
                                                     epoch_dev, row_epoch, R);
}

long emb_delta_tile_rows() { return DT_TILE; }
long emb_delta_tiles(long R) { return (R + DT_TILE - 1) / DT_TILE; }

void emb_delta_count(const int* row_epoch, long R, int since,
                     const int* nrows_dev, const unsigned char* valid,
                     int* tile_counts, hipStream_t stream) {
    if (R)
        k_delta_count<<<(int)emb_delta_tiles(R), BLOCK, 0, stream>>>(
            row_epoch, R, since, nrows_dev, valid, tile_counts);
}

void emb_delta_compact(const int* row_epoch, long R, int since,
                       const int* nrows_dev, const unsigned char* valid,
                       const int* tile_incl, i64* slots,
                       hipStream_t stream) {
    long T = emb_delta_tiles(R);
    if (R)
        k_delta_compact<<<(int)T, BLOCK, 0, stream>>>(
            row_epoch, R, since, nrows_dev, valid, tile_incl, T, slots);
}

void emb_delta_gather(const float* weights, const float* state, long R,
                      long dim, long sd, const i64* slot_keys,
                      long shard_num, long shard_id, const i64* slots,
                      long nslots, long start, long count, const int* n_dev,
                      i64* keys_out, float* w_out, float* s_out,
                      hipStream_t stream) {
    if (count <= 0 || !R) return;
    if (dim <= 32)
        k_delta_gather<16><<<grid1d(count * 16), BLOCK, 0, stream>>>(
            weights, state, R, dim, sd, slot_keys, shard_num, shard_id,
            slots, nslots, start, count, n_dev, keys_out, w_out, s_out);
    else
        k_delta_gather<64><<<grid1d(count * 64), BLOCK, 0, stream>>>(
            weights, state, R, dim, sd, slot_keys, shard_num, shard_id,
            slots, nslots, start, count, n_dev, keys_out, w_out, s_out);
}

void emb_expire_flag(const int* row_epoch, long R, int before,
                     const int* nrows_dev, const unsigned char* valid,
                     unsigned char* dead, hipStream_t stream) {
    if (R)
        k_expire_flag<<<grid1d(R), BLOCK, 0, stream>>>(row_epoch, R, before,
                                                       nrows_dev, valid, dead);
}

void emb_flag_slots(const i64* slots, long n, unsigned char* dead, long R,
                    hipStream_t stream) {
    fill_u8(dead, R, 0, stream);
    if (n && R)
        k_flag_slots<<<grid1d(n), BLOCK, 0, stream>>>(slots, n, dead, R);
}

void emb_expire_count(int mode, const unsigned char* dead, long R,
                      const int* nrows_dev, const unsigned char* valid,
                      const int* cnt, int* tile_counts, hipStream_t stream) {
    if (!R) return;
    int T = (int)emb_delta_tiles(R);
#define LAUNCH_XP_COUNT(M)                                                   \
    k_expire_count<M><<<T, BLOCK, 0, stream>>>(dead, R, nrows_dev, valid,   \
                                               cnt, tile_counts)
    if (mode == XP_DEAD) LAUNCH_XP_COUNT(XP_DEAD);
    else if (mode == XP_HOLE) LAUNCH_XP_COUNT(XP_HOLE);
    else LAUNCH_XP_COUNT(XP_MOVER);
#undef LAUNCH_XP_COUNT
}

void emb_expire_counts(const int* tile_incl, long T, const int* nrows_dev,
                       long R, int* cnt, hipStream_t stream) {
    k_expire_counts<<<1, 64, 0, stream>>>(tile_incl, T, nrows_dev, R, cnt);
}

void emb_expire_compact(int mode, const unsigned char* dead, long R,
                        const int* nrows_dev, const unsigned char* valid,
                        const int* cnt, const int* tile_incl, int* list,
                        i64* keys_out, const i64* slot_keys, long shard_num,
                        long shard_id, long out_cap, hipStream_t stream) {
    if (!R || out_cap <= 0) return;
    int T = (int)emb_delta_tiles(R);
#define LAUNCH_XP_COMPACT(M)                                                 \
    k_expire_compact<M><<<T, BLOCK, 0, stream>>>(                           \
        dead, R, nrows_dev, valid, cnt, tile_incl, list, keys_out,          \
        slot_keys, shard_num, shard_id, out_cap)
    if (mode == XP_DEAD) LAUNCH_XP_COMPACT(XP_DEAD);
    else if (mode == XP_HOLE) LAUNCH_XP_COMPACT(XP_HOLE);
    else LAUNCH_XP_COMPACT(XP_MOVER);
#undef LAUNCH_XP_COMPACT
}

void emb_move_rows(void* base, long R, long wpr, const int* holes,
                   const int* movers, long cap, const int* count_dev,
                   hipStream_t stream) {
    if (cap <= 0 || !R || wpr <= 0) return;
    unsigned* b = static_cast<unsigned*>(base);
    if (wpr <= 2)
        k_move_rows<1><<<grid1d(cap), BLOCK, 0, stream>>>(
            b, R, wpr, holes, movers, cap, count_dev);
    else if (wpr <= 32)
        k_move_rows<16><<<grid1d(cap * 16), BLOCK, 0, stream>>>(
            b, R, wpr, holes, movers, cap, count_dev);
    else
        k_move_rows<64><<<grid1d(cap * 64), BLOCK, 0, stream>>>(
            b, R, wpr, holes, movers, cap, count_dev);
}

// rows: a host bound of n' that sizes the grid (at least one thread runs,
// to publish n')
void emb_ht_build(u64* tk, int* tv, long cap, const i64* slot_keys, long R,
                  const int* cnt, int* nrows_dev, long rows,
                  hipStream_t stream) {
    fill_u64(tk, cap, EMPTY, stream);
    k_ht_build<<<grid1d(rows > 0 ? rows : 1), BLOCK, 0, stream>>>(
        tk, tv, cap - 1, slot_keys, R, cnt, nrows_dev);
}

void emb_expire_array(unsigned char* valid, const unsigned char* dead, long R,
                      hipStream_t stream) {
    if (R)
        k_expire_array<<<grid1d(R), BLOCK, 0, stream>>>(valid, dead, R);
}

void emb_fault_in(const i64* keys, long n, const int* u_dev, const u64* htk,
                  const int* htv, long hcap, const float* host_w,
                  const float* host_s, float* weights, float* state,
                  long dim, long sd, const i64* slots,
                  unsigned char* new_mask, int* faulted,
                  hipStream_t stream) {
    if (!n) return;
    if (dim <= 32)
        k_fault_in<16><<<grid1d(n * 16), BLOCK, 0, stream>>>(
            keys, n, u_dev, htk, htv, hcap - 1, host_w, host_s, weights,
            state, dim, sd, slots, new_mask, faulted);
    else
        k_fault_in<64><<<grid1d(n * 64), BLOCK, 0, stream>>>(
            keys, n, u_dev, htk, htv, hcap - 1, host_w, host_s, weights,
            state, dim, sd, slots, new_mask, faulted);
}

void emb_spill_rows(const i64* cache_slots, const i64* host_slots, long n,
                    const float* weights, const float* state, float* host_w,
                    float* host_s, long dim, long sd, hipStream_t stream) {
    if (!n) return;
    if (dim <= 32)
        k_spill_rows<16><<<grid1d(n * 16), BLOCK, 0, stream>>>(
            cache_slots, host_slots, n, weights, state, host_w, host_s, dim,
            sd);
    else
        k_spill_rows<64><<<grid1d(n * 64), BLOCK, 0, stream>>>(
            cache_slots, host_slots, n, weights, state, host_w, host_s, dim,
            sd);
}

void emb_gather_host(const i64* keys, long n, const i64* cache_slots,
                     const u64* htk, const int* htv, long hcap,
                     const float* host_w, float* out, long dim,
                     hipStream_t stream) {
    if (!n) return;
    if (dim <= 32)
        k_gather_host<16><<<grid1d(n * 16), BLOCK, 0, stream>>>(
            keys, n, cache_slots, htk, htv, hcap - 1, host_w, out, dim);
    else
        k_gather_host<64><<<grid1d(n * 64), BLOCK, 0, stream>>>(
            keys, n, cache_slots, htk, htv, hcap - 1, host_w, out, dim);
}

void emb_bucketize_pad(const i64* keys, long n, const int* u_dev, long world,
                       long cap, i64* send_keys, int* send_src, int* pos_of,
                       int* counts, int* overflow, hipStream_t stream) {
    long total = world * cap;
    // one fused reset launch: keys EMPTY ((i64)-1), src -1, counts 0
    if (total) k_pad_reset<<<grid1d(total), BLOCK, 0, stream>>>(
        (u64*)send_keys, send_src, total, counts, world);
    // overflow intentionally NOT cleared: it accumulates across steps and
    // the host reads+clears it outside the hot loop
    if (n) k_bucketize_pad<<<grid1d(n), BLOCK, 0, stream>>>(
        keys, n, u_dev, world, cap, send_keys, send_src, pos_of, counts,
        overflow);
}

void emb_gather_pad(const float* ugrads, const u64* counts, long dim,
                    const int* send_src, long total, float* send_p,
                    hipStream_t stream) {
    if (total)
        k_gather_pad<<<grid1d(total * (dim + 1)), BLOCK, 0, stream>>>(
            ugrads, counts, dim, send_src, total, send_p);
}

void emb_scatter_out(const float* rows_recv, const i64* inverse, long n_elems,
                     const int* pos_of, long dim, float* out,
                     hipStream_t stream) {
    if (n_elems)
        k_scatter_out<<<grid1d(n_elems * dim), BLOCK, 0, stream>>>(
            rows_recv, inverse, n_elems, pos_of, dim, out);
}

void emb_split_payload(const float* g2c, long u, long dim, const int* u_dev,
                       float* grads, u64* counts, hipStream_t stream) {
    if (u)
        k_split_payload<<<grid1d(u * (dim + 1)), BLOCK, 0, stream>>>(
            g2c, u, dim, u_dev, grads, counts);
}

void emb_flat_adagrad_f32(float* p, float* accum, const float* g, long n,
                          float lr, float eps, hipStream_t stream) {
    if (n) k_flat_adagrad_f32<<<grid1d(n), BLOCK, 0, stream>>>(p, accum, g, n,
                                                               lr, eps);
}

void emb_flat_adagrad_bf16(float* master, float* accum, const void* g,
                           void* p, long n, float lr, float eps,
                           hipStream_t stream) {
    if (n) k_flat_adagrad_bf16<<<grid1d(n), BLOCK, 0, stream>>>(
        master, accum, (const oebf16*)g, (oebf16*)p, n, lr, eps);
}

void emb_flat_step_scalars(float* sc, float b1, float b2,
                           hipStream_t stream) {
    k_flat_step_scalars<<<1, 64, 0, stream>>>(sc, b1, b2);
}

#define LAUNCH_FLAT(OPT)                                                    \
    do {                                                                    \
        if (bf16)                                                           \
            k_flat_opt_bf16<OPT><<<grid1d(n), BLOCK, 0, stream>>>(          \
                master, s1, s2, (oebf16*)g, (oebf16*)p, sc, n, lr,          \
                c0, c1, c2);                                                \
        else                                                                \
            k_flat_opt_f32<OPT><<<grid1d(n), BLOCK, 0, stream>>>(          \
                (float*)p, s1, s2, (float*)g, sc, n, lr, c0, c1, c2);       \
    } while (0)

void emb_flat_opt(int opt, void* p, float* master, float* s1, float* s2,
                  void* g, const float* sc, long n, int bf16,
                  float lr, float c0, float c1, float c2,
                  hipStream_t stream) {
    if (!n) return;
    switch (opt) {
        case FLAT_SGD: LAUNCH_FLAT(FLAT_SGD); break;
        case FLAT_ADAGRAD: LAUNCH_FLAT(FLAT_ADAGRAD); break;
        case FLAT_ADAM: LAUNCH_FLAT(FLAT_ADAM); break;
    }
}

void emb_bce_fwd(const float* z, const float* y, long n, float* loss,
                 hipStream_t stream) {
    if (!n) { fill_f32(loss, 1, 0.f, stream); return; }
    if (n <= 65536) {   // one block reduces it faster than fill + atomics
        k_bce_fwd_1blk<<<1, 1024, 0, stream>>>(z, y, n, 1.f / (float)n,
                                               loss);
        return;
    }
    fill_f32(loss, 1, 0.f, stream);
    k_bce_fwd<<<grid1d(n), BLOCK, 0, stream>>>(z, y, n, 1.f / (float)n,
                                               loss);
}

void emb_bce_bwd(const float* z, const float* y, long n, const float* go,
                 float* g, hipStream_t stream) {
    int ga = grid1d(n);
    if (n) k_bce_bwd<<<ga, BLOCK, 0, stream>>>(z, y, n, 1.f / (float)n, go, g);
}

}  // extern "C"
