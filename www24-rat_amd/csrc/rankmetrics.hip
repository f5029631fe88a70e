// rankmetrics.hip — NDCG@k, MRR@k and HitRate@k per group of an evaluation pass, on the device.
//
// The reference checked out beside this project evaluates logloss and AUC only; later FuxiCTR releases report NDCG(k=...), MRR and
// HitRate(k=...) per group beside gAUC.  Here they come out of one launch chain over the device vectors; 64 bytes per cutoff are all
// a caller has to read back.  Definitions (include/rat_hip.h: rat_eval_rank_metrics; rat_amd/metrics.py):
//
//   order   : inside a group np.argsort(-p_g, kind="stable") over the group's rows in input order — descending prediction, ties keep
//             input order, -0.0 equal to +0.0 (the order rank_requests documents).  A row's place r is 0-based.
//   counted : a group counts if it holds at least one positive (y == 1); every metric is the unweighted mean over the counted groups.
//   for a counted group with P positives and f the place of its first positive:
//             DCG@k = sum_{r < k, y_r = 1} 1 / log2(r + 2),  IDCG@k = sum_{j < min(P, k)} 1 / log2(j + 2),  NDCG@k = DCG@k / IDCG@k,
//             MRR@k = 1 / (f + 1) if f < k else 0,  HitRate@k = 1 if f < k else 0.  All arithmetic is float64.
//
// The chain (everything that reads all rows runs once per call; a cutoff costs one sweep over the keys and a few entries per group):
//   keys        : (group ^ 0x80000000) << 32 | ~pred_key(p) — ascending keys are ascending group ids and, inside a group, descending
//                 predictions — with the class as a one-byte payload; the status bits of every 1024-row tile, reduced in the block;
//   radix sort  : rocPRIM, stable (std::stable_sort under RAT_EMU): stability is what makes ties keep input order;
//   heads, scan : metrics_common.h — per sorted row {negatives so far, start of its run, start of its group};
//   terms       : per sorted row i at place r = i - group start: {1 / log2(r + 2) if the row is a positive, 1 / log2(i + 2), r if it is a
//                 positive, "a group starts here"} — no cutoff enters;
//   prefix sums : ONE inclusive scan of those entries (rocPRIM's bitwise-reproducible scan with a custom operator; a sequential scan
//                 under RAT_EMU): the first component is summed and the third minimised SEGMENTED — they restart at every group head —,
//                 the second is summed over all rows.  Row i then holds the DCG of its group's places 0 .. r, the ideal sum
//                 H(i + 1) = sum_{j <= i} 1 / log2(j + 2), and the place of the first positive among its group's places 0 .. r.
//                 Because a group's rows stand in the order of their places, DCG@k is the entry at the group's row min(k, rows) - 1 and
//                 IDCG@k is H(min(P, k)): a cutoff is two look-ups.  No group's sum is a difference of global prefix sums, there are no
//                 floating atomics, and nothing depends on scheduling;
//   cutoff      : per cutoff, at the last row of every group: the rows, the positives P and the first positive's place f from the two
//                 scans, then DCG / IDCG, 1 / (f + 1) and the hit if f < k, "a group counted" and "a group seen" -> two reduction trees;
//   finish      : one thread per cutoff writes out[i][0..7].
// All kernels written here are streaming kernels: a thread owns 4 consecutive rows and moves them with 16-byte accesses where the buffers
// allow.
#include "metrics_common.h"

namespace {

constexpr int RK_MAX_CUTOFFS = 8;
constexpr int RK_ROOTS = 1 + 2 * RK_MAX_CUTOFFS;     // {status} then per cutoff {quotient sum, counted, hits} {rr sum, groups seen}
constexpr uint32_t RK_NO_POSITIVE = 0xffffffffu;

enum { ST_NAN_PRED = 1, ST_BAD_LABEL = 2, ST_NO_POSITIVE = 16 };

// one sorted row before the scan, and the prefix at that row after it (see the chain above); head != 0: a group starts here
struct Seg {
    double dcg, ideal;
    uint32_t first, head;
};
struct SegOp {
    __host__ __device__ Seg operator()(const Seg& x, const Seg& y) const {
        const double ideal = x.ideal + y.ideal;
        if (y.head) return Seg{y.dcg, ideal, y.first, y.head};
        return Seg{x.dcg + y.dcg, ideal, x.first < y.first ? x.first : y.first, x.head};
    }
};

struct Cutoffs {
    int32_t k[RK_MAX_CUTOFFS];
};

// ---- keys, classes and the status tiles ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MT_THREADS)
rank_keys_kernel(const float* __restrict__ y_pred, const float* __restrict__ y_true, const int32_t* __restrict__ group, int64_t n, int vec,
                 uint64_t* __restrict__ keys, uint8_t* __restrict__ cls, Part* __restrict__ parts) {
    const int64_t i0 = ((int64_t)blockIdx.x * MT_THREADS + threadIdx.x) * MT_ITEMS;
    float p[MT_ITEMS], y[MT_ITEMS];
    int32_t g[MT_ITEMS];
    const bool full = i0 + MT_ITEMS <= n;
    if (full && vec) {                               // 16 bytes per lane, consecutive lanes on consecutive addresses
        const float4 pv = *reinterpret_cast<const float4*>(y_pred + i0);
        const float4 yv = *reinterpret_cast<const float4*>(y_true + i0);
        const Quad32 gv = *reinterpret_cast<const Quad32*>(group + i0);
        p[0] = pv.x; p[1] = pv.y; p[2] = pv.z; p[3] = pv.w;
        y[0] = yv.x; y[1] = yv.y; y[2] = yv.z; y[3] = yv.w;
        g[0] = (int32_t)gv.x; g[1] = (int32_t)gv.y; g[2] = (int32_t)gv.z; g[3] = (int32_t)gv.w;
    } else {
#pragma unroll
        for (int j = 0; j < MT_ITEMS; ++j) {
            const bool in = i0 + j < n;
            p[j] = in ? y_pred[i0 + j] : 0.f;
            y[j] = in ? y_true[i0 + j] : 0.f;
            g[j] = in ? group[i0 + j] : 0;
        }
    }
    Part acc = part_zero();
    uint64_t k[MT_ITEMS];
    uint32_t c4 = 0;
#pragma unroll
    for (int j = 0; j < MT_ITEMS; ++j) {
        k[j] = ((uint64_t)((uint32_t)g[j] ^ 0x80000000u) << 32) | (uint32_t)~pred_key(p[j]);
        const uint32_t pos = y[j] == 1.0f ? 1u : 0u;
        c4 |= pos << (8 * j);
        if (i0 + j < n) {
            acc.b += pos;
            acc.d |= (p[j] != p[j] ? ST_NAN_PRED : 0) | ((y[j] == 0.0f || y[j] == 1.0f) ? 0 : ST_BAD_LABEL);
        }
    }
    if (full) {
        *reinterpret_cast<Pair64*>(keys + i0) = Pair64{k[0], k[1]};
        *reinterpret_cast<Pair64*>(keys + i0 + 2) = Pair64{k[2], k[3]};
        *reinterpret_cast<uint32_t*>(cls + i0) = c4;
    } else {
#pragma unroll
        for (int j = 0; j < MT_ITEMS; ++j)
            if (i0 + j < n) {
                keys[i0 + j] = k[j];
                cls[i0 + j] = (uint8_t)((c4 >> (8 * j)) & 1u);
            }
    }
    const Part sum = block_tree(acc);
    if (threadIdx.x == 0) parts[blockIdx.x] = sum;
}

// ---- the entries of the sorted rows, before the scan --------------------------------------------------------------------------------------
// terms: 3 x 8 bytes per row {DCG term, ideal term, first | head << 32}; a thread's 4 rows are 96 contiguous bytes
__global__ void __launch_bounds__(MT_THREADS)
rank_terms_kernel(const Scan3* __restrict__ scan, const uint8_t* __restrict__ cls, int64_t n, Seg* __restrict__ terms) {
    const int64_t i0 = ((int64_t)blockIdx.x * MT_THREADS + threadIdx.x) * MT_ITEMS;
    if (i0 >= n) return;
    const bool full = i0 + MT_ITEMS <= n;
    uint32_t c4 = 0;
    if (full) {
        c4 = *reinterpret_cast<const uint32_t*>(cls + i0);
    } else {
#pragma unroll
        for (int j = 0; j < MT_ITEMS; ++j)
            if (i0 + j < n) c4 |= (uint32_t)(cls[i0 + j] & 1u) << (8 * j);
    }
    uint64_t dcg[MT_ITEMS], ideal[MT_ITEMS], tail[MT_ITEMS];
#pragma unroll
    for (int j = 0; j < MT_ITEMS; ++j) {
        const int64_t i = i0 + j;
        dcg[j] = ideal[j] = tail[j] = 0;
        if (i < n) {
            const int64_t place = i - (int64_t)scan[i].grp;
            const bool pos = (c4 >> (8 * j)) & 1u;
            dcg[j] = __builtin_bit_cast(uint64_t, pos ? 1.0 / log2((double)(place + 2)) : 0.0);
            ideal[j] = __builtin_bit_cast(uint64_t, 1.0 / log2((double)(i + 2)));
            tail[j] = (uint64_t)(pos ? (uint32_t)place : RK_NO_POSITIVE) | ((uint64_t)(place == 0 ? 1u : 0u) << 32);
        }
    }
    if (full) {
        Pair64* dst = reinterpret_cast<Pair64*>(terms + i0);
        dst[0] = Pair64{dcg[0], ideal[0]};
        dst[1] = Pair64{tail[0], dcg[1]};
        dst[2] = Pair64{ideal[1], tail[1]};
        dst[3] = Pair64{dcg[2], ideal[2]};
        dst[4] = Pair64{tail[2], dcg[3]};
        dst[5] = Pair64{ideal[3], tail[3]};
    } else {
#pragma unroll
        for (int j = 0; j < MT_ITEMS; ++j)
            if (i0 + j < n)
                terms[i0 + j] = Seg{__builtin_bit_cast(double, dcg[j]), __builtin_bit_cast(double, ideal[j]), (uint32_t)tail[j],
                                    (uint32_t)(tail[j] >> 32)};
    }
}

// ---- one cutoff: the terms of every group, at its last row; summed per tile -------------------------------------------------------------------
// first[tile] = {sum of DCG / IDCG, groups counted, hits}, second[tile] = {sum of the reciprocal ranks, groups seen}
__global__ void __launch_bounds__(MT_THREADS)
rank_cutoff_kernel(const uint64_t* __restrict__ keys, const Scan3* __restrict__ scan, const Seg* __restrict__ sums, int64_t n, int64_t k,
                   Part* __restrict__ first, Part* __restrict__ second) {
    const int64_t i0 = ((int64_t)blockIdx.x * MT_THREADS + threadIdx.x) * MT_ITEMS;
    Part acc = part_zero(), bcc = part_zero();
    uint64_t key = i0 < n ? keys[i0] : 0;
#pragma unroll
    for (int j = 0; j < MT_ITEMS; ++j) {
        const int64_t i = i0 + j;
        if (i >= n) break;
        const uint64_t next = i + 1 < n ? keys[i + 1] : 0;
        if (i + 1 == n || !same_group(next, key)) {      // the group [start, i] ends here
            const Scan3 me = scan[i];
            const int64_t start = (int64_t)me.grp;
            const int64_t rows = i + 1 - start;
            const int64_t positives = rows - ((int64_t)me.neg - (int64_t)neg_before(scan, me.grp));
            bcc.b += 1;
            if (positives > 0) {
                const int64_t f = (int64_t)sums[i].first;
                const double dcg = sums[start + (k < rows ? k : rows) - 1].dcg;         // the group's places 0 .. min(k, rows) - 1
                const double idcg = sums[(k < positives ? k : positives) - 1].ideal;    // H(min(P, k)): the row index is only a count
                acc.a += dcg / idcg;
                acc.b += 1;
                if (f < k) {
                    acc.c += 1;
                    bcc.a += 1.0 / (double)(f + 1);
                }
            }
        }
        key = next;
    }
    const Part sum = block_tree(acc);
    if (threadIdx.x == 0) first[blockIdx.x] = sum;
    const Part sum_b = block_tree(bcc);
    if (threadIdx.x == 0) second[blockIdx.x] = sum_b;
}

__global__ void rank_finish_kernel(const Part* __restrict__ roots, int m, Cutoffs cut, double* __restrict__ out) {
    const int t = (int)threadIdx.x;
    if (blockIdx.x != 0 || t >= m) return;
    const double nan = __builtin_nan("");
    const Part first = roots[1 + 2 * t], last = roots[2 + 2 * t];
    int64_t status = roots[0].d;
    const int64_t counted = first.b;
    if (counted == 0) status |= ST_NO_POSITIVE;
    const bool ok = status == 0;
    double* o = out + 8 * t;
    o[0] = ok ? first.a / (double)counted : nan;
    o[1] = ok ? last.a / (double)counted : nan;
    o[2] = ok ? (double)first.c / (double)counted : nan;
    o[3] = (double)counted;
    o[4] = (double)last.b;
    o[5] = (double)first.c;
    o[6] = (double)cut.k[t];
    o[7] = (double)status;
}

// ---- workspace ------------------------------------------------------------------------------------------------------------------------------
struct View {
    uint64_t* keys_in;       // [n]
    uint64_t* keys;          // [n], sorted
    uint8_t* cls_in;         // [n]
    uint8_t* cls;            // [n], sorted
    Scan3* heads;            // [n]
    Scan3* scan;             // [n]
    Seg* terms;              // [n]
    Seg* sums;               // [n]
    Part* level_a;           // [tiles(n)]
    Part* level_a2;          // [tiles(n)]: the second tree of a cutoff
    Part* level_b;           // [tiles(tiles(n))]
    Part* roots;             // [RK_ROOTS]
    void* temp;              // rocPRIM temporary storage
    size_t temp_bytes;
};

size_t prim_temp_bytes(int64_t n) {
#ifdef RAT_EMU
    (void)n;
    return 256;
#else
    size_t need = 0, b = 0;
    uint64_t* k8 = nullptr;
    uint8_t* c = nullptr;
    Scan3* s = nullptr;
    Seg* t = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, b, k8, k8, c, c, (size_t)n, 0, 64, (hipStream_t)0);
    need = b > need ? b : need;
    (void)rocprim::inclusive_scan(nullptr, b, s, s, (size_t)n, Scan3Op(), (hipStream_t)0);
    need = b > need ? b : need;
    (void)rocprim::deterministic_inclusive_scan(nullptr, b, t, t, (size_t)n, SegOp(), (hipStream_t)0);
    need = b > need ? b : need;
    return align256(need) + 256;
#endif
}

// the carve-up of a workspace for n rows (base == nullptr: sizes only); returns the bytes in front of the rocPRIM storage
size_t carve(void* ws, int64_t n, View& v) {
    char* base = static_cast<char*>(ws);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        void* p = base ? base + off : nullptr;
        off += align256(bytes);
        return p;
    };
    v.keys_in = static_cast<uint64_t*>(take((size_t)n * 8));
    v.keys = static_cast<uint64_t*>(take((size_t)n * 8));
    v.cls_in = static_cast<uint8_t*>(take((size_t)n));
    v.cls = static_cast<uint8_t*>(take((size_t)n));
    v.heads = static_cast<Scan3*>(take((size_t)n * sizeof(Scan3)));
    v.scan = static_cast<Scan3*>(take((size_t)n * sizeof(Scan3)));
    v.terms = static_cast<Seg*>(take((size_t)n * sizeof(Seg)));
    v.sums = static_cast<Seg*>(take((size_t)n * sizeof(Seg)));
    v.level_a = static_cast<Part*>(take((size_t)tiles_of(n) * sizeof(Part)));
    v.level_a2 = static_cast<Part*>(take((size_t)tiles_of(n) * sizeof(Part)));
    v.level_b = static_cast<Part*>(take((size_t)tiles_of(tiles_of(n)) * sizeof(Part)));
    v.roots = static_cast<Part*>(take(RK_ROOTS * sizeof(Part)));
    v.temp = base ? base + off : nullptr;
    return off;
}

}  // namespace

extern "C" size_t rat_eval_rank_metrics_workspace(int64_t n, int n_cutoffs) {
    (void)n_cutoffs;                                 // a cutoff needs no buffer of its own; the roots are laid out for the maximum
    if (n < 1) n = 1;
    if (n > 0x7fffffffLL) n = 0x7fffffffLL;
    View v{};
    return carve(nullptr, n, v) + prim_temp_bytes(n);
}

extern "C" int rat_eval_rank_metrics(const float* y_pred, const float* y_true, const int32_t* group, int64_t n, const int32_t* cutoffs,
                                     int n_cutoffs, double* out, void* workspace, size_t workspace_bytes, void* stream) {
    static_assert(sizeof(Seg) == 24, "rank_terms_kernel stores a thread's 4 rows as 6 x 16 bytes");
    RAT_REQUIRE(y_pred && y_true && group && cutoffs && out && workspace, "null pointer");
    RAT_REQUIRE(n >= 1 && n <= 0x7fffffffLL, "n must be in [1, 2^31 - 1]");
    RAT_REQUIRE(n_cutoffs >= 1 && n_cutoffs <= RK_MAX_CUTOFFS, "n_cutoffs must be in [1, 8]");
    Cutoffs cut{};
    for (int c = 0; c < n_cutoffs; ++c) {
        RAT_REQUIRE(cutoffs[c] >= 1, "a cutoff must be >= 1");
        cut.k[c] = cutoffs[c];
    }
    RAT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "workspace must be 256-byte aligned");
    RAT_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0, "out must be 8-byte aligned");
    RAT_REQUIRE(workspace_bytes >= rat_eval_rank_metrics_workspace(n, n_cutoffs), "workspace too small");
    View v{};
    v.temp_bytes = workspace_bytes - carve(workspace, n, v);
    const unsigned blocks = (unsigned)tiles_of(n);
    const int vec = al16(y_pred) && al16(y_true) && al16(group);

    // once per call: keys by (group, descending prediction), the status bits, the sort, the heads and their scan, the rows' prefix sums
    RAT_LAUNCH(rank_keys_kernel, blocks, MT_THREADS, 0, stream, y_pred, y_true, group, n, vec, v.keys_in, v.cls_in, v.level_a);
    reduce_tree(v.level_a, v.level_b, blocks, v.roots + 0, stream);
    if (sort_heads_scan<uint64_t>(v.temp, v.temp_bytes, v.keys_in, v.keys, v.cls_in, v.cls, v.heads, v.scan, n, stream,
                                  "rat_eval_rank_metrics") != 0)
        return -1;
    RAT_LAUNCH(rank_terms_kernel, blocks, MT_THREADS, 0, stream, v.scan, v.cls, n, v.terms);
#ifdef RAT_EMU
    std::partial_sum(v.terms, v.terms + n, v.sums, SegOp());
#else
    size_t tb = v.temp_bytes;
    if (rocprim::deterministic_inclusive_scan(v.temp, tb, v.terms, v.sums, (size_t)n, SegOp(), (hipStream_t)stream) != hipSuccess)
        return rat_fail("rat_eval_rank_metrics: prefix scan failed");
#endif

    // once per cutoff: every group's terms from the prefix sums
    for (int c = 0; c < n_cutoffs; ++c) {
        RAT_LAUNCH(rank_cutoff_kernel, blocks, MT_THREADS, 0, stream, v.keys, v.scan, v.sums, n, (int64_t)cut.k[c], v.level_a, v.level_a2);
        reduce_tree(v.level_a, v.level_b, blocks, v.roots + 1 + 2 * c, stream);
        reduce_tree(v.level_a2, v.level_b, blocks, v.roots + 2 + 2 * c, stream);
    }
    RAT_LAUNCH(rank_finish_kernel, 1, 64, 0, stream, v.roots, n_cutoffs, cut, out);
    return rat_check_launch("rat_eval_rank_metrics");
}
