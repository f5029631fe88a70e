// metrics_common.h — what the metric chains on the device share (metrics.hip: logloss, AUC, GAUC; rankmetrics.hip: NDCG, MRR, HitRate):
// the order-preserving key map, the class byte, the run / group heads with their (+, max, max) scan, and the fixed-shape reduction tree.
// Everything sits in an unnamed namespace: each translation unit that includes the file gets its own copy of the kernels.
//
//   tiles        : every kernel is a streaming kernel — 256 threads, a thread owns 4 consecutive entries (16-byte accesses where the
//                  buffers allow), a block 1024 of them;
//   tree levels  : every sum runs over those fixed 1024-entry tiles in index order — 4 consecutive entries per thread, then a binary tree
//                  over the block's 256 threads in LDS — level after level until one value is left.  The tree is a function of the count
//                  alone: no result depends on scheduling.
#pragma once
#include "rat_device.h"
#include "../../include/rat_hip.h"

#include <cmath>
#ifdef RAT_EMU
#include <algorithm>
#include <numeric>
#else
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#endif

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_ITEMS = 4;                          // consecutive entries per thread
constexpr int MT_TILE = MT_THREADS * MT_ITEMS;       // entries per block: the leaf width of every reduction tree

// what a tree carries: a and b, c are summed, d is OR-ed
struct __attribute__((aligned(16))) Part {
    double a;
    int64_t b, c, d;
};
__device__ __forceinline__ Part part_zero() { return Part{0.0, 0, 0, 0}; }
__device__ __forceinline__ Part part_join(const Part& lo, const Part& hi) { return Part{lo.a + hi.a, lo.b + hi.b, lo.c + hi.c, lo.d | hi.d}; }

// per sorted row, before the scan: {negative? 1 : 0, position if a run starts here, position if a group starts here}
// after the inclusive scan: {negatives in [0, i], first row of i's run, first row of i's group}
struct __attribute__((aligned(16))) Scan3 {
    uint32_t neg, run, grp, pad;
};
struct Scan3Op {
    __host__ __device__ Scan3 operator()(const Scan3& x, const Scan3& y) const {
        return Scan3{x.neg + y.neg, x.run > y.run ? x.run : y.run, x.grp > y.grp ? x.grp : y.grp, 0u};
    }
};

// 16-byte register images for the wide stores (the same in the host emulation)
struct __attribute__((aligned(16))) Quad32 {
    uint32_t x, y, z, w;
};
struct __attribute__((aligned(16))) Pair64 {
    uint64_t x, y;
};

size_t align256(size_t v) { return (v + 255) / 256 * 256; }
int64_t tiles_of(int64_t n) { return (n + MT_TILE - 1) / MT_TILE; }
bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the block's 256 per-thread values -> their sum in thread 0, lower index on the left at every node
__device__ __forceinline__ Part block_tree(Part v) {
    __shared__ Part tree_s[MT_THREADS];
    const int t = (int)threadIdx.x;
    __syncthreads();                                 // the previous use of tree_s by this block is over
    tree_s[t] = v;
    __syncthreads();
    for (int s = MT_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) tree_s[t] = part_join(tree_s[t], tree_s[t + s]);
        __syncthreads();
    }
    return tree_s[0];
}

// order-preserving fp32 -> uint32: negative values flip every bit, the others the sign bit; -0.0 is +0.0
__device__ __forceinline__ uint32_t pred_key(float p) {
    uint32_t u = rat_fbits(p);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <class KeyT> __device__ __forceinline__ KeyT make_key(float p, int32_t g);
template <> __device__ __forceinline__ uint32_t make_key<uint32_t>(float p, int32_t) { return pred_key(p); }
template <> __device__ __forceinline__ uint64_t make_key<uint64_t>(float p, int32_t g) {
    return ((uint64_t)((uint32_t)g ^ 0x80000000u) << 32) | pred_key(p);
}
__device__ __forceinline__ bool same_group(uint32_t, uint32_t) { return true; }
__device__ __forceinline__ bool same_group(uint64_t x, uint64_t y) { return (x >> 32) == (y >> 32); }

// ---- run heads and group heads of the sorted rows -----------------------------------------------------------------------------------
template <class KeyT>
__global__ void __launch_bounds__(MT_THREADS)
heads_kernel(const KeyT* __restrict__ keys, const uint8_t* __restrict__ cls, int64_t n, Scan3* __restrict__ heads) {
    const int64_t i0 = ((int64_t)blockIdx.x * MT_THREADS + threadIdx.x) * MT_ITEMS;
    if (i0 >= n) return;
    KeyT prev = i0 > 0 ? keys[i0 - 1] : KeyT(0);
#pragma unroll
    for (int j = 0; j < MT_ITEMS; ++j) {
        const int64_t i = i0 + j;
        if (i >= n) break;
        const KeyT k = keys[i];
        const bool run = i == 0 || k != prev;
        const bool grp = i == 0 || !same_group(k, prev);
        heads[i] = Scan3{cls[i] ? 0u : 1u, run ? (uint32_t)i : 0u, grp ? (uint32_t)i : 0u, 0u};
        prev = k;
    }
}

// negatives in [0, i)
__device__ __forceinline__ uint32_t neg_before(const Scan3* __restrict__ scan, uint32_t i) { return i > 0 ? scan[i - 1].neg : 0u; }

// ---- one level of a tree: out[b] = in[1024 b .. 1024 b + 1023] in index order ------------------------------------------------------------------
__global__ void __launch_bounds__(MT_THREADS)
tree_level_kernel(const Part* __restrict__ in, int64_t count, Part* __restrict__ out) {
    const int64_t i0 = ((int64_t)blockIdx.x * MT_THREADS + threadIdx.x) * MT_ITEMS;
    Part acc = part_zero();
#pragma unroll
    for (int j = 0; j < MT_ITEMS; ++j)
        if (i0 + j < count) acc = part_join(acc, in[i0 + j]);
    const Part sum = block_tree(acc);
    if (threadIdx.x == 0) out[blockIdx.x] = sum;
}

// level_a[0 .. count) -> *root, through as many levels as it takes; level_a holds tiles(n) entries, level_b tiles(tiles(n)), count <= tiles(n)
void reduce_tree(Part* level_a, Part* level_b, int64_t count, Part* root, void* stream) {
    Part* in = level_a;
    Part* out = level_b;
    for (;;) {
        const int64_t blocks = tiles_of(count);
        Part* dst = blocks == 1 ? root : out;
        RAT_LAUNCH(tree_level_kernel, (unsigned)blocks, MT_THREADS, 0, stream, in, count, dst);
        if (blocks == 1) return;
        count = blocks;
        Part* t = in; in = out; out = t;             // level_b holds tiles(tiles(n)) entries, level_a more: every later level fits
    }
}

// keys_in / cls_in -> keys / cls, stably sorted by key; heads and their scan over the sorted rows.  temp: rocPRIM temporary storage
template <class KeyT>
int sort_heads_scan(void* temp, size_t temp_bytes, KeyT* keys_in, KeyT* keys, uint8_t* cls_in, uint8_t* cls, Scan3* heads, Scan3* scan,
                    int64_t n, void* stream, const char* what) {
    const unsigned blocks = (unsigned)tiles_of(n);
#ifdef RAT_EMU
    (void)temp;
    (void)temp_bytes;
    (void)what;
    std::vector<uint32_t> order((size_t)n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return keys_in[x] < keys_in[y]; });
    for (int64_t i = 0; i < n; ++i) {
        keys[i] = keys_in[order[(size_t)i]];
        cls[i] = cls_in[order[(size_t)i]];
    }
    RAT_LAUNCH((heads_kernel<KeyT>), blocks, MT_THREADS, 0, stream, keys, cls, n, heads);
    std::partial_sum(heads, heads + n, scan, Scan3Op());
#else
    hipStream_t s = (hipStream_t)stream;
    size_t tb = temp_bytes;
    if (rocprim::radix_sort_pairs(temp, tb, keys_in, keys, cls_in, cls, (size_t)n, 0, (unsigned)(8 * sizeof(KeyT)), s) != hipSuccess)
        return rat_fail(std::string(what) + ": radix sort failed");
    RAT_LAUNCH((heads_kernel<KeyT>), blocks, MT_THREADS, 0, stream, keys, cls, n, heads);
    tb = temp_bytes;
    if (rocprim::inclusive_scan(temp, tb, heads, scan, (size_t)n, Scan3Op(), s) != hipSuccess)
        return rat_fail(std::string(what) + ": scan failed");
#endif
    return 0;
}

}  // namespace
