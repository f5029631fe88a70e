// metrics.hip — logloss, AUC and per-group GAUC of an evaluation pass, on the device.
//
// The reference evaluates on the host (fuxictr/metrics.py:22-41: sklearn's log_loss with eps = 1e-7 and roc_auc_score over numpy
// copies of every prediction and label) and names GAUC without implementing it (fuxictr/metrics.py:29-39: `pass`).  Here the three
// come out of one launch chain over the device vectors; 64 bytes are all a caller has to read back.
//
//   logloss : mean of -(y log p + (1 - y) log(1 - p)) in float64, p = clip(double(pred), 1e-7, 1 - 1e-7) — rat_amd.metrics.log_loss.
//   AUC     : exact, as an integer statistic.  Over the predictions sorted ascending (-0.0 keyed as +0.0, so the two tie as they do
//             in numpy), U2 = sum over runs of equal predictions of pos_run * (2 * neg_before_run + neg_run), an int64
//             (U2 <= 2 pos neg < 2^62); AUC = U2 / (2 pos neg), ONE division in double — the same two integers
//             rat_amd.metrics.auc_score (average ranks) divides.  pos means y_true == 1.
//   GAUC    : the same statistic per group over the sort by (group id, prediction); a group counts only if it holds both classes;
//             GAUC = sum_g n_g AUC_g / sum_g n_g over the counted groups, n_g = the rows of group g — the definition later FuxiCTR
//             releases use (their metrics.py weighs every user's AUC by that user's number of samples).  A group id is only ever a
//             sort key, never an address: any int32 is legal.
//
// The chain (one "pass" for AUC with 32-bit keys; with groups a second pass with 64-bit keys for GAUC):
//   build_keys   : order-preserving fp32 -> uint32 map (+ the group id in the upper half), the class as a one-byte payload, and — in the
//                  first pass — the logloss terms, positives and status bits of every 1024-row tile, reduced in the block;
//   radix sort   : rocPRIM (a library primitive, as in sparse.hip; std::stable_sort under RAT_EMU);
//   heads        : per sorted row {negative?, own position if it starts a run, own position if it starts a group};
//   scan         : rocPRIM inclusive scan with (+, max, max) -> per row {negatives so far, start of its run, start of its group};
//   run terms    : at the last row of every run pos_run * (2 neg_before_run + neg_run), 0 elsewhere.  Without groups the terms are
//                  summed right there; with groups they are written out and an int64 inclusive scan (rocPRIM) follows, so that a
//                  group's U2 is a difference of two scan values — no atomics anywhere;
//   group terms  : at the last row of every group the quotient, weighted by the group's rows;
//   tree levels  : every sum runs over fixed 1024-entry tiles in index order — 4 consecutive entries per thread, then a binary tree over
//                  the block's 256 threads in LDS — level after level until one value is left.  The tree is a function of n alone: the
//                  results do not depend on scheduling, and everything but logloss (whose terms sit at the rows' positions) not on
//                  the order of the rows either;
//   finish       : one thread writes out[0..7].
// All kernels are streaming kernels: a thread owns 4 consecutive rows and moves them with 16-byte accesses where the buffers allow.
#include "metrics_common.h"

namespace {

constexpr int MT_ROOTS = 3;                          // {logloss terms, positives, status} {U2} {weighted quotients, rows, groups}

enum { ST_NAN_PRED = 1, ST_BAD_LABEL = 2, ST_ONE_CLASS = 4, ST_NO_GROUP = 8 };

struct AddI64 {
    __host__ __device__ int64_t operator()(int64_t x, int64_t y) const { return x + y; }
};

// ---- keys, classes and (LOSS) the logloss tiles -----------------------------------------------------------------------------------
template <class KeyT, bool LOSS>
__global__ void __launch_bounds__(MT_THREADS)
build_keys_kernel(const float* __restrict__ y_pred, const float* __restrict__ y_true, const int32_t* __restrict__ group, int64_t n,
                  int vec, KeyT* __restrict__ keys, uint8_t* __restrict__ cls, Part* __restrict__ parts) {
    const int64_t i0 = ((int64_t)blockIdx.x * MT_THREADS + threadIdx.x) * MT_ITEMS;
    float p[MT_ITEMS], y[MT_ITEMS];
    int32_t g[MT_ITEMS];
    const bool full = i0 + MT_ITEMS <= n;
    if (full && vec) {                               // 16 bytes per lane, consecutive lanes on consecutive addresses
        const float4 pv = *reinterpret_cast<const float4*>(y_pred + i0);
        const float4 yv = *reinterpret_cast<const float4*>(y_true + i0);
        p[0] = pv.x; p[1] = pv.y; p[2] = pv.z; p[3] = pv.w;
        y[0] = yv.x; y[1] = yv.y; y[2] = yv.z; y[3] = yv.w;
    } else {
#pragma unroll
        for (int j = 0; j < MT_ITEMS; ++j) {
            const bool in = i0 + j < n;
            p[j] = in ? y_pred[i0 + j] : 0.f;
            y[j] = in ? y_true[i0 + j] : 0.f;
        }
    }
#pragma unroll
    for (int j = 0; j < MT_ITEMS; ++j) g[j] = (sizeof(KeyT) == 8 && i0 + j < n) ? group[i0 + j] : 0;
    Part acc = part_zero();
    KeyT k[MT_ITEMS];
    uint32_t c4 = 0;
#pragma unroll
    for (int j = 0; j < MT_ITEMS; ++j) {
        const bool in = i0 + j < n;
        k[j] = make_key<KeyT>(p[j], g[j]);
        const uint32_t pos = y[j] == 1.0f ? 1u : 0u;
        c4 |= pos << (8 * j);
        if (LOSS && in) {
            double q = (double)p[j];
            const bool nan = q != q;
            q = q < 1e-7 ? 1e-7 : (q > 1.0 - 1e-7 ? 1.0 - 1e-7 : q);      // a NaN stays a NaN, as in np.clip
            const double yd = (double)y[j];
            acc.a += -(yd * log(q) + (1.0 - yd) * log(1.0 - q));
            acc.b += pos;
            acc.d |= (nan ? ST_NAN_PRED : 0) | ((y[j] == 0.0f || y[j] == 1.0f) ? 0 : ST_BAD_LABEL);
        }
    }
    if (full) {
        if (sizeof(KeyT) == 4) {
            *reinterpret_cast<Quad32*>(keys + i0) = Quad32{(uint32_t)k[0], (uint32_t)k[1], (uint32_t)k[2], (uint32_t)k[3]};
        } else {
            uint64_t* kp = reinterpret_cast<uint64_t*>(keys + i0);
            *reinterpret_cast<Pair64*>(kp) = Pair64{(uint64_t)k[0], (uint64_t)k[1]};
            *reinterpret_cast<Pair64*>(kp + 2) = Pair64{(uint64_t)k[2], (uint64_t)k[3]};
        }
        *reinterpret_cast<uint32_t*>(cls + i0) = c4;
    } else {
#pragma unroll
        for (int j = 0; j < MT_ITEMS; ++j)
            if (i0 + j < n) {
                keys[i0 + j] = k[j];
                cls[i0 + j] = (uint8_t)((c4 >> (8 * j)) & 1u);
            }
    }
    if (LOSS) {
        const Part sum = block_tree(acc);
        if (threadIdx.x == 0) parts[blockIdx.x] = sum;
    }
}

// ---- the term of every run, at its last row -------------------------------------------------------------------------------------------
// SUM: the terms are summed per tile (parts[tile].b); otherwise they are written to terms[i]
template <class KeyT, bool SUM>
__global__ void __launch_bounds__(MT_THREADS)
run_terms_kernel(const KeyT* __restrict__ keys, const Scan3* __restrict__ scan, int64_t n, int64_t* __restrict__ terms,
                 Part* __restrict__ parts) {
    const int64_t i0 = ((int64_t)blockIdx.x * MT_THREADS + threadIdx.x) * MT_ITEMS;
    Part acc = part_zero();
    int64_t t[MT_ITEMS];
    KeyT k = i0 < n ? keys[i0] : KeyT(0);
#pragma unroll
    for (int j = 0; j < MT_ITEMS; ++j) {
        const int64_t i = i0 + j;
        t[j] = 0;
        if (i < n) {
            const KeyT next = i + 1 < n ? keys[i + 1] : KeyT(0);
            if (i + 1 == n || next != k) {           // the run [s, i] of group [g, ...] ends here
                const Scan3 me = scan[i];
                const uint32_t before_run = neg_before(scan, me.run);
                const int64_t neg_run = (int64_t)me.neg - before_run;
                const int64_t pos_run = (i + 1 - (int64_t)me.run) - neg_run;
                const int64_t neg_before_run = (int64_t)before_run - neg_before(scan, me.grp);
                t[j] = pos_run * (2 * neg_before_run + neg_run);
            }
            k = next;
        }
        acc.b += t[j];
    }
    if (SUM) {
        const Part sum = block_tree(acc);
        if (threadIdx.x == 0) parts[blockIdx.x] = sum;
    } else if (i0 + MT_ITEMS <= n) {
        *reinterpret_cast<Pair64*>(terms + i0) = Pair64{(uint64_t)t[0], (uint64_t)t[1]};
        *reinterpret_cast<Pair64*>(terms + i0 + 2) = Pair64{(uint64_t)t[2], (uint64_t)t[3]};
    } else {
#pragma unroll
        for (int j = 0; j < MT_ITEMS; ++j)
            if (i0 + j < n) terms[i0 + j] = t[j];
    }
}

// ---- the quotient of every group that holds both classes, at its last row, weighted by its rows; summed per tile ----------------------------
__global__ void __launch_bounds__(MT_THREADS)
group_terms_kernel(const uint64_t* __restrict__ keys, const Scan3* __restrict__ scan, const int64_t* __restrict__ cum, int64_t n,
                   Part* __restrict__ parts) {
    const int64_t i0 = ((int64_t)blockIdx.x * MT_THREADS + threadIdx.x) * MT_ITEMS;
    Part acc = part_zero();
    uint64_t k = i0 < n ? keys[i0] : 0;
#pragma unroll
    for (int j = 0; j < MT_ITEMS; ++j) {
        const int64_t i = i0 + j;
        if (i >= n) break;
        const uint64_t next = i + 1 < n ? keys[i + 1] : 0;
        if (i + 1 == n || !same_group(next, k)) {
            const Scan3 me = scan[i];
            const int64_t rows = i + 1 - (int64_t)me.grp;
            const int64_t neg = (int64_t)me.neg - neg_before(scan, me.grp);
            const int64_t pos = rows - neg;
            if (pos > 0 && neg > 0) {
                const int64_t u2 = cum[i] - (me.grp > 0 ? cum[me.grp - 1] : 0);
                acc.a += (double)rows * ((double)u2 / (double)(2 * pos * neg));
                acc.b += rows;
                acc.c += 1;
            }
        }
        k = next;
    }
    const Part sum = block_tree(acc);
    if (threadIdx.x == 0) parts[blockIdx.x] = sum;
}

__global__ void finish_kernel(const Part* __restrict__ roots, int64_t n, int grouped, double* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double nan = __builtin_nan("");
    const Part loss = roots[0], all = roots[1];
    const int64_t pos = loss.b, neg = n - loss.b;
    int64_t status = loss.d;
    if (pos == 0 || neg == 0) status |= ST_ONE_CLASS;
    double groups = 0.0, rows = 0.0, gauc = nan;
    if (grouped) {
        const Part per = roots[2];
        groups = (double)per.c;
        rows = (double)per.b;
        if (per.c == 0) status |= ST_NO_GROUP;
        else gauc = per.a / (double)per.b;
    }
    const bool ranked = (status & (ST_NAN_PRED | ST_BAD_LABEL | ST_ONE_CLASS)) == 0;
    out[0] = (status & ST_NAN_PRED) ? nan : loss.a / (double)n;
    out[1] = ranked ? (double)all.b / (double)(2 * pos * neg) : nan;
    out[2] = ranked && !(status & ST_NO_GROUP) ? gauc : nan;
    out[3] = (double)pos;
    out[4] = (double)neg;
    out[5] = groups;
    out[6] = rows;
    out[7] = (double)status;
}

// ---- workspace ------------------------------------------------------------------------------------------------------------------------------
struct View {
    void* keys_in;           // KeyT [n]
    void* keys;              // KeyT [n], sorted
    uint8_t* cls_in;         // [n]
    uint8_t* cls;            // [n], sorted
    Scan3* heads;            // [n]
    Scan3* scan;             // [n]
    int64_t* terms;          // [n]  (grouped only)
    int64_t* cum;            // [n]  (grouped only)
    Part* level_a;           // [tiles(n)]
    Part* level_b;           // [tiles(tiles(n))]
    Part* roots;             // [MT_ROOTS]
    void* temp;              // rocPRIM temporary storage
    size_t temp_bytes;
};

size_t prim_temp_bytes(int64_t n, int grouped) {
#ifdef RAT_EMU
    (void)n;
    (void)grouped;
    return 256;
#else
    size_t need = 0, b = 0;
    uint32_t* k4 = nullptr;
    uint64_t* k8 = nullptr;
    uint8_t* c = nullptr;
    Scan3* s = nullptr;
    int64_t* t = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, b, k4, k4, c, c, (size_t)n, 0, 32, (hipStream_t)0);
    need = b > need ? b : need;
    (void)rocprim::inclusive_scan(nullptr, b, s, s, (size_t)n, Scan3Op(), (hipStream_t)0);
    need = b > need ? b : need;
    if (grouped) {
        (void)rocprim::radix_sort_pairs(nullptr, b, k8, k8, c, c, (size_t)n, 0, 64, (hipStream_t)0);
        need = b > need ? b : need;
        (void)rocprim::inclusive_scan(nullptr, b, t, t, (size_t)n, AddI64(), (hipStream_t)0);
        need = b > need ? b : need;
    }
    return align256(need) + 256;
#endif
}

// the carve-up of a workspace for n rows (base == nullptr: sizes only); returns the bytes in front of the rocPRIM storage
size_t carve(void* ws, int64_t n, int grouped, View& v) {
    char* base = static_cast<char*>(ws);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        void* p = base ? base + off : nullptr;
        off += align256(bytes);
        return p;
    };
    const size_t key_bytes = (size_t)n * (grouped ? 8 : 4);
    v.keys_in = take(key_bytes);
    v.keys = take(key_bytes);
    v.cls_in = static_cast<uint8_t*>(take((size_t)n));
    v.cls = static_cast<uint8_t*>(take((size_t)n));
    v.heads = static_cast<Scan3*>(take((size_t)n * sizeof(Scan3)));
    v.scan = static_cast<Scan3*>(take((size_t)n * sizeof(Scan3)));
    v.terms = v.cum = nullptr;
    if (grouped) {
        v.terms = static_cast<int64_t*>(take((size_t)n * sizeof(int64_t)));
        v.cum = static_cast<int64_t*>(take((size_t)n * sizeof(int64_t)));
    }
    v.level_a = static_cast<Part*>(take((size_t)tiles_of(n) * sizeof(Part)));
    v.level_b = static_cast<Part*>(take((size_t)tiles_of(tiles_of(n)) * sizeof(Part)));
    v.roots = static_cast<Part*>(take(MT_ROOTS * sizeof(Part)));
    v.temp = base ? base + off : nullptr;
    return off;
}

// level_a[0 .. count) -> *root, through as many levels as it takes
void reduce_levels(const View& v, int64_t count, Part* root, void* stream) { reduce_tree(v.level_a, v.level_b, count, root, stream); }

template <class KeyT>
int sort_and_scan(const View& v, int64_t n, void* stream) {
    return sort_heads_scan<KeyT>(v.temp, v.temp_bytes, static_cast<KeyT*>(v.keys_in), static_cast<KeyT*>(v.keys), v.cls_in, v.cls, v.heads,
                                 v.scan, n, stream, "rat_eval_metrics");
}

}  // namespace

extern "C" size_t rat_eval_metrics_workspace(int64_t n, int grouped) {
    if (n < 1) n = 1;
    if (n > 0x7fffffffLL) n = 0x7fffffffLL;
    View v{};
    return carve(nullptr, n, grouped != 0, v) + prim_temp_bytes(n, grouped != 0);
}

extern "C" int rat_eval_metrics(const float* y_pred, const float* y_true, const int32_t* group, int64_t n, double* out, void* workspace,
                                size_t workspace_bytes, void* stream) {
    RAT_REQUIRE(y_pred && y_true && out && workspace, "null pointer");
    RAT_REQUIRE(n >= 1 && n <= 0x7fffffffLL, "n must be in [1, 2^31 - 1]");
    const int grouped = group != nullptr;
    RAT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "workspace must be 256-byte aligned");
    RAT_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0, "out must be 8-byte aligned");
    RAT_REQUIRE(workspace_bytes >= rat_eval_metrics_workspace(n, grouped), "workspace too small");
    View v{};
    v.temp_bytes = workspace_bytes - carve(workspace, n, grouped, v);
    const unsigned blocks = (unsigned)tiles_of(n);
    const int vec = al16(y_pred) && al16(y_true);

    // pass 1: keys by prediction -> logloss, the class counts, the status bits, U2 of all rows
    RAT_LAUNCH((build_keys_kernel<uint32_t, true>), blocks, MT_THREADS, 0, stream, y_pred, y_true, group, n, vec,
               static_cast<uint32_t*>(v.keys_in), v.cls_in, v.level_a);
    reduce_levels(v, blocks, v.roots + 0, stream);
    if (sort_and_scan<uint32_t>(v, n, stream) != 0) return -1;
    RAT_LAUNCH((run_terms_kernel<uint32_t, true>), blocks, MT_THREADS, 0, stream, static_cast<const uint32_t*>(v.keys), v.scan, n,
               (int64_t*)nullptr, v.level_a);
    reduce_levels(v, blocks, v.roots + 1, stream);

    // pass 2: keys by (group, prediction) -> the weighted quotients of the groups that hold both classes
    if (grouped) {
        RAT_LAUNCH((build_keys_kernel<uint64_t, false>), blocks, MT_THREADS, 0, stream, y_pred, y_true, group, n, vec,
                   static_cast<uint64_t*>(v.keys_in), v.cls_in, (Part*)nullptr);
        if (sort_and_scan<uint64_t>(v, n, stream) != 0) return -1;
        RAT_LAUNCH((run_terms_kernel<uint64_t, false>), blocks, MT_THREADS, 0, stream, static_cast<const uint64_t*>(v.keys), v.scan, n,
                   v.terms, (Part*)nullptr);
#ifdef RAT_EMU
        std::partial_sum(v.terms, v.terms + n, v.cum);
#else
        size_t tb = v.temp_bytes;
        if (rocprim::inclusive_scan(v.temp, tb, v.terms, v.cum, (size_t)n, AddI64(), (hipStream_t)stream) != hipSuccess)
            return rat_fail("rat_eval_metrics: scan failed");
#endif
        RAT_LAUNCH(group_terms_kernel, blocks, MT_THREADS, 0, stream, static_cast<const uint64_t*>(v.keys), v.scan, v.cum, n, v.level_a);
        reduce_levels(v, blocks, v.roots + 2, stream);
    }
    RAT_LAUNCH(finish_kernel, 1, 64, 0, stream, v.roots, n, grouped, out);
    return rat_check_launch("rat_eval_metrics");
}
