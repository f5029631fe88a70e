// online.hip — the request path of the retrieval: ids of a fresh query batch -> neighbour lists, without leaving the device.
//
// The offline job (retrieval.hip, rat_bm25_topk) maps the query ids to IDF weights on the host (rat_amd/retrieval.py:
// map_data_to_idf, a numpy searchsorted per column) and gives ONE work-group a tile of four queries and the whole pool — right for
// 200 000 queries, wrong for a request of 1-64 rows, which would occupy 1-16 of the chip's 256 CUs.  Two pieces close that gap:
//
//   rat_bm25_query_prepare   map_data_to_idf on the device: a binary search per (query, column) in the pool's IDF tables (built
//                            once per pool by retrieval.idf_tables and kept in HBM), including the reference's dtype rule — if
//                            row 0 of the batch misses in a column, every weight of that column is truncated toward zero.
//   rat_bm25_topk_split      rat_bm25_topk's contract with the pool cut into `splits` contiguous row ranges: work-group
//                            (tile, range) scans its range exactly as bm25_topk_kernel scans the pool (same fp64 sums, f ascending)
//                            and leaves its K best in workspace [Q][splits][K]; a second launch merges the partial lists of a query.
//                            The order (score descending, pool index ascending) is total, and the K best of the pool are among
//                            the K best of the ranges, so the result is the single-range result bit for bit, whatever `splits`.
//
// Both scan-side merges are per WAVE (lanes exchange their list heads through a wave-private LDS tile, no work-group barrier);
// the four waves' lists of a work-group are then ranked against each other after the one barrier of the kernel.
// Nothing here allocates, synchronises or uses a floating-point atomic: the pair is captured into the serving graph (rat_amd/online.py).
#include "bm25_scan.h"
#include "pool_common.h"

namespace {

constexpr int ON_THREADS = 256;
constexpr int ON_WAVES = ON_THREADS / 64;
constexpr int ON_FMAX = 32;
constexpr int ON_KMAX = 32;
constexpr int ON_MAX_SPLITS = 4096;
// splits = 0: the rule read off tools/online_bench.py's sweep (profiles/online/online_bench.txt): with at least one query
// tile per CU the single-range kernel already fills the chip; below that, enough ranges for ON_TARGET_GROUPS work-groups (two per
// CU — what the scan kernel's 226 VGPRs let a CU hold; more ranges only add merge work), every range at least one full trip of the
// scan loop (256 lanes x 4 rows), at most ON_AUTO_MAX_SPLITS.
constexpr int64_t ON_SINGLE_TILES = 256;
constexpr int64_t ON_TARGET_GROUPS = 512;
constexpr int64_t ON_MIN_RANGE_ROWS = 1024;
constexpr int64_t ON_AUTO_MAX_SPLITS = 256;

// ---- arg-max over the 64 lanes of ONE wave, QT independent problems at once: every lane passes a candidate per problem and gets
// the wave's best back.  Two levels through a wave-private LDS tile (64 heads -> 8 group bests -> 1), double-buffered by the
// call's parity so that a call costs two wave fences and no work-group barrier.
template <int QT>
struct WaveTile {
    double hv[2][QT][64];
    int64_t hi[2][QT][64];
    double gv[2][QT][8];
    int64_t gi[2][QT][8];
};

template <int QT>
__device__ __forceinline__ void wave_best(WaveTile<QT>& w, int parity, double (&s)[QT], int64_t (&i)[QT]) {
    const int lane = rat_lane();
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        w.hv[parity][t][lane] = s[t];
        w.hi[parity][t][lane] = i[t];
    }
    RAT_WAVE_FENCE();
    const int g = lane & 7;
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        double cs = 0.0;
        int64_t ci = -1;
#pragma unroll
        for (int j = 0; j < 8; ++j) take_better(w.hv[parity][t][8 * g + j], w.hi[parity][t][8 * g + j], cs, ci);
        if (lane < 8) {
            w.gv[parity][t][g] = cs;
            w.gi[parity][t][g] = ci;
        }
    }
    RAT_WAVE_FENCE();
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        double cs = 0.0;
        int64_t ci = -1;
#pragma unroll
        for (int j = 0; j < 8; ++j) take_better(w.gv[parity][t][j], w.gi[parity][t][j], cs, ci);
        s[t] = cs;
        i[t] = ci;
    }
}

// ------------------------------------------------------------------------------------------------------------ pass 1: scan a range
struct SplitArgs {
    const int32_t* db_t;     // [F][N]
    const int32_t* qry;      // [Q][F]
    const double* idf;       // [Q][F]
    double* part_val;        // [Q][splits][K]
    int64_t* part_idx;       // [Q][splits][K]
    double* out_val;         // [Q][K]
    int64_t* out_idx;        // [Q][K]
    int64_t* out_len;        // [Q]
    int64_t N, Q;            // N: rows of the pool — POOL_DEV / POOL_RING: read from *n_dev instead, and N is not used
    int F, K, splits;
    const int64_t* n_dev;    // POOL_DEV: the pool's current row count (the header a RetrievalIndex with capacity keeps);
                             // POOL_RING: that header is two words, {row count, physical slot of the oldest live row}
    int64_t stride;          // POOL_DEV / POOL_RING: column stride of db_t (the capacity); otherwise the stride is N
    const int64_t* before;   // [Q], HORIZON only: query q sees the logical rows i < before[q]
    uint32_t exact_mask;     // EXACT only: bit f set = used column f is an exact-match column (it gates a row, it adds no weight)
    const int32_t* listing;  // EXACT only: one word, != 0 = the listing rule holds for this call (bm25_exact_list_kernel)
};

// Where the scan takes the pool's extent from.
// POOL_HOST: rat_bm25_topk_split (row count and column stride are the host argument N).  POOL_DEV: rat_bm25_topk_split_dev — the
// row count is read from device memory (clamped to [0, stride]: no row past the buffers is ever addressed) and db_t is [F][stride].
// POOL_RING: rat_bm25_topk_split_ring — db_t is a ring of `stride` slots: the header also holds `head` (clamped to [0, stride)), and
// LOGICAL row n (0 = oldest) lives in slot head + n, minus stride when that is >= stride (head + n < 2 stride, so a compare and a
// subtract).  Only the address of the one id load is physical: ranges, list entries, ties and the merge all see logical rows.
// Everything after the prologue is the same code, so the same fp64 sums in the same order and the same merge.
// (The forms, their header clamps and the ring's wrap are pool_common.h's.)

// HORIZON (rat_bm25_topk_split_before): query q's candidates are the logical rows below before[q], clamped to [0, N] on the device.
// The rows are scored as ever and a row at or past its query's horizon then scores 0 — one compare and select per (row, query) after
// the field loop — so it never enters a list; what follows (insertion, wave merge, ranking, bm25_merge_kernel) is the same code, and
// the sums, their order and the total order are those of the plain scan over the rows [0, before[q]).  Ranges are still cut over
// [0, N), and a work-group whose range lies past every horizon of its tile scans it all the same (nothing here is tuned).
// POOL_HOST with HORIZON takes the column stride from a.stride (the pool's capacity), the row count from a.N.
//
// EXACT (rat_bm25_topk_split_exact; always with HORIZON, whose list may be null here: no horizon, every query sees [0, N)): the
// used columns in a.exact_mask are exact-match columns.  In the field loop such a column adds no weight; it ANDs "row equals query
// here" into a gate, one bit per (row, query) of the trip.  After the loop a row inside the gate scores (sum + 1) — the sum over the
// remaining columns, f ascending, as rat_bm25_topk_grouped forms it — and any other row 0, before the horizon select.  A candidate
// scores at least 1, so it is positive; insertion, wave merge, ranking and bm25_merge_kernel are the same code.
template <int KMAX, int QT, int RU, int POOL, bool HORIZON, bool EXACT = false>
__global__ void __launch_bounds__(ON_THREADS) bm25_scan_split_kernel(SplitArgs a) {
    static_assert(!EXACT || (HORIZON && RU * QT <= 32), "the exact-match scan has the horizon select and one gate word per trip");
    __shared__ WaveTile<QT> tile_s[ON_WAVES];
    __shared__ double wl_v[ON_WAVES][QT][KMAX];          // the K best of every wave, ranked against each other after the barrier
    __shared__ int64_t wl_i[ON_WAVES][QT][KMAX];
    const int tid = threadIdx.x, lane = rat_lane(), wave = rat_wave();
    const int64_t ntiles = (a.Q + QT - 1) / QT;
    // the prologue keeps its own clamps (pool_view's, spelled out): through pool_view the same values compile to another
    // instruction stream in 12 of this kernel's 18 instantiations (profiles/online/shared_code_resource_usage.txt), and the scan is
    // to stay the parent's code
    int64_t N = a.N, stride = a.N;
    [[maybe_unused]] int64_t head = 0;
    if constexpr (POOL != POOL_HOST) {
        stride = a.stride;
        N = a.n_dev[0];
        N = N < 0 ? 0 : (N > stride ? stride : N);
    }
    if constexpr (POOL == POOL_RING) {
        head = a.n_dev[1];
        head = head < 0 ? 0 : (head >= stride ? stride - 1 : head);
    }
    if constexpr (HORIZON && POOL == POOL_HOST) {
        stride = a.stride;
        N = N < 0 ? 0 : (N > stride ? stride : N);
    }
    const int64_t chunk = (N + a.splits - 1) / a.splits;
    int parity = 0;
    for (int64_t item = blockIdx.x; item < ntiles * a.splits; item += gridDim.x) {
        const int64_t q0 = (item / a.splits) * QT;
        const int split = (int)(item % a.splits);
        const int64_t lo = split * chunk < N ? split * chunk : N;            // ranges past the end of the pool are empty
        const int64_t hi = lo + chunk < N ? lo + chunk : N;
        [[maybe_unused]] int64_t bef[QT];                  // HORIZON: the tile's horizons, clamped to [0, N]
        if constexpr (HORIZON) {
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                const int64_t q = q0 + t < a.Q ? q0 + t : a.Q - 1;            // wave-uniform: scalar loads
                int64_t b = N;
                if constexpr (!EXACT)
                    b = a.before[q];
                else if (a.before != nullptr)
                    b = a.before[q];
                bef[t] = b < 0 ? 0 : (b > N ? N : b);
            }
        }
        double val[QT][KMAX], kth[QT];                     // kth = score of the current K-th entry (0 while the list is not full)
        int64_t idx[QT][KMAX];
        list_init<KMAX, QT>(val, idx, kth);
        // ---- scan rows [lo, hi) the way bm25_topk_kernel scans [0, N): every lane walks its rows in increasing order and offers
        //      them to its lists (bm25_scan.h: RAT_BM25_LIST_INSERT, the same text)
        for (int64_t n0 = lo + tid; n0 < hi; n0 += (int64_t)ON_THREADS * RU) {
            double s[RU][QT];
#pragma unroll
            for (int u = 0; u < RU; ++u)
#pragma unroll
                for (int t = 0; t < QT; ++t) s[u][t] = 0.0;
            [[maybe_unused]] uint32_t gate = ~0u;          // EXACT: bit u * QT + t = row u equals query t on every exact column so far
            for (int f = 0; f < a.F; ++f) {
                int32_t id[RU];
#pragma unroll
                for (int u = 0; u < RU; ++u) {                                            // RU independent loads in flight per field
                    const int64_t n = n0 + (int64_t)u * ON_THREADS;
                    int64_t slot = n;
                    if constexpr (POOL == POOL_RING) slot = ring_wrap(n + head, stride);  // logical row -> its slot of the ring
                    id[u] = n < hi ? a.db_t[(int64_t)f * stride + slot] : -1;
                }
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    const int64_t q = q0 + t < a.Q ? q0 + t : a.Q - 1;                    // wave-uniform: scalar loads
                    const int32_t qid = a.qry[q * a.F + f];
                    if constexpr (EXACT) {
                        if ((a.exact_mask >> f) & 1u) {                                   // wave-uniform: the column gates, it adds nothing
#pragma unroll
                            for (int u = 0; u < RU; ++u) gate &= ~((uint32_t)(qid != id[u]) << (u * QT + t));
                            continue;
                        }
                    }
                    const double w = a.idf[q * a.F + f];
#pragma unroll
                    for (int u = 0; u < RU; ++u) s[u][t] += (qid == id[u] && n0 + (int64_t)u * ON_THREADS < hi) ? w : 0.0;
                }
            }
            if constexpr (EXACT) {                         // (sum + 1) inside the gate, 0 outside; a row past the range is outside
#pragma unroll
                for (int u = 0; u < RU; ++u)
#pragma unroll
                    for (int t = 0; t < QT; ++t)
                        s[u][t] = (((gate >> (u * QT + t)) & 1u) != 0 && n0 + (int64_t)u * ON_THREADS < hi) ? s[u][t] + 1.0 : 0.0;
            }
            if constexpr (HORIZON) {
#pragma unroll
                for (int u = 0; u < RU; ++u)
#pragma unroll
                    for (int t = 0; t < QT; ++t) s[u][t] = n0 + (int64_t)u * ON_THREADS < bef[t] ? s[u][t] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < RU; ++u) {                                                // rows in increasing order
                const int64_t n = n0 + (int64_t)u * ON_THREADS;
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    RAT_BM25_LIST_INSERT(KMAX, val[t], idx[t], kth[t], a.K, s[u][t], n);
                }
            }
        }
        // ---- every wave merges its 64 private lists: up to K rounds of a wave arg-max over the lists' heads, the QT queries in
        //      lock step.  Lane t * KMAX + k keeps slot (t, k) of the wave's result.  A wave none of whose lanes owns a row
        //      (wave-uniform) has nothing to merge.
        int k_end = 0;
        if (lo + (int64_t)wave * 64 < hi) {
            for (; k_end < a.K; ++k_end) {
                double hs[QT];
                int64_t hx[QT];
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    hs[t] = val[t][0];
                    hx[t] = idx[t][0];
                }
                wave_best<QT>(tile_s[wave], parity, hs, hx);
                parity ^= 1;
                bool any = false;
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    any |= hx[t] >= 0;
                    if (hx[t] >= 0 && idx[t][0] == hx[t]) list_pop<KMAX>(val[t], idx[t]);     // the winner pops its head
                    if (lane == t * KMAX + k_end) {
                        wl_v[wave][t][k_end] = hx[t] >= 0 ? hs[t] : 0.0;
                        wl_i[wave][t][k_end] = hx[t];
                    }
                }
                if (!any) {                            // every list of every query is exhausted (the same in all lanes)
                    ++k_end;
                    break;
                }
            }
        }
        if (lane < QT * KMAX && lane % KMAX >= k_end) {
            wl_v[wave][lane / KMAX][lane % KMAX] = 0.0;
            wl_i[wave][lane / KMAX][lane % KMAX] = -1;
        }
        __syncthreads();
        // ---- rank the four waves' lists against each other: entry (w, t, k) goes to slot (number of better entries), if < K
        if (tid < ON_WAVES * QT * KMAX) {
            const int w = tid / (QT * KMAX), t = (tid / KMAX) % QT, k = tid % KMAX;
            if (k < a.K && q0 + t < a.Q) {
                const double es = wl_v[w][t][k];
                const int64_t ei = wl_i[w][t][k];
                int rank = 0, total = 0;
                for (int w2 = 0; w2 < ON_WAVES; ++w2)
                    for (int k2 = 0; k2 < a.K; ++k2) {
                        const int64_t oi = wl_i[w2][t][k2];
                        total += oi >= 0 ? 1 : 0;
                        rank += (oi >= 0 && ei >= 0 && better(wl_v[w2][t][k2], oi, es, ei)) ? 1 : 0;
                    }
                const int64_t base = ((q0 + t) * a.splits + split) * a.K;
                if (ei >= 0 && rank < a.K) {
                    a.part_val[base + rank] = es;
                    a.part_idx[base + rank] = ei;
                }
                if (w == 0 && k >= total) {                                                // fewer than K candidates in this range
                    a.part_val[base + k] = 0.0;
                    a.part_idx[base + k] = -1;
                }
            }
        }
        __syncthreads();                               // the next item reuses wl_*
    }
}

// ------------------------------------------------------------------------------------------------------------ pass 2: merge
// One wave per query over its splits * K partial entries: round k picks the best entry that comes AFTER round k - 1's winner in the
// total order (indices are distinct, so "after" is strict) — no per-list state.
__global__ void __launch_bounds__(64) bm25_merge_kernel(SplitArgs a) {
    __shared__ WaveTile<1> tile_s;
    const int lane = rat_lane();
    const int64_t C = (int64_t)a.splits * a.K;
    int parity = 0;
    for (int64_t q = blockIdx.x; q < a.Q; q += gridDim.x) {
        const double* pv = a.part_val + q * C;
        const int64_t* pi = a.part_idx + q * C;
        double ps = 0.0;
        int64_t px = -1;                               // previous winner (none yet)
        int k = 0;
        for (; k < a.K; ++k) {
            double cs[1] = {0.0};
            int64_t ci[1] = {-1};
            for (int64_t c = lane; c < C; c += 64) {
                const double s = pv[c];
                const int64_t i = pi[c];
                if (i >= 0 && (px < 0 || better(ps, px, s, i))) take_better(s, i, cs[0], ci[0]);
            }
            wave_best<1>(tile_s, parity, cs, ci);
            parity ^= 1;
            if (ci[0] < 0) break;                      // nothing left (the same in all lanes)
            ps = cs[0];
            px = ci[0];
            if (lane == 0) {
                a.out_val[q * a.K + k] = ps;
                a.out_idx[q * a.K + k] = px;
            }
        }
        for (int j = k + lane; j < a.K; j += 64) {     // zero scores are dropped: index -1, value 0
            a.out_val[q * a.K + j] = 0.0;
            a.out_idx[q * a.K + j] = -1;
        }
        if (lane == 0) a.out_len[q] = k;
    }
}

// ------------------------------------------------------------------------------------------------------------ pass 3 (EXACT): listing
// The listing rule of the exact-match retrieval (rat_amd/retrieval.py: no group of the call is larger than K): a query's entries are
// its candidates in ascending logical index, each with value 1.0.  Every candidate scored >= 1 and there are at most K of them, so the
// merged list already holds them all, in score order: one wave per query gives entry k the slot (number of valid entries with a lower
// index) — the indices are distinct, the valid entries stand in front — and nothing is rescanned.  *listing == 0: nothing to do.
__global__ void __launch_bounds__(64) bm25_exact_list_kernel(SplitArgs a) {
    if (a.listing[0] == 0) return;                     // the same in every thread of the grid
    const int lane = rat_lane();
    for (int64_t q = blockIdx.x; q < a.Q; q += gridDim.x) {
        int64_t* idx = a.out_idx + q * a.K;
        const int64_t mine = lane < a.K ? idx[lane] : -1;
        int rank = 0;
        for (int j = 0; j < a.K; ++j) {
            const int64_t other = idx[j];
            rank += (other >= 0 && mine >= 0 && other < mine) ? 1 : 0;         // rank < K: at most K - 1 others
        }
        __syncthreads();                               // every entry is read before one is overwritten
        if (mine >= 0) {
            idx[rank] = mine;
            a.out_val[q * a.K + rank] = 1.0;
        }
        __syncthreads();
    }
}

int64_t auto_splits(int64_t n_qry, int64_t n_db, int topk) {
    const int64_t tiles = topk <= 8 ? (n_qry + 3) / 4 : n_qry;
    if (tiles >= ON_SINGLE_TILES) return 1;
    int64_t s = (ON_TARGET_GROUPS + tiles - 1) / tiles;
    const int64_t by_rows = n_db / ON_MIN_RANGE_ROWS;
    if (s > by_rows) s = by_rows;
    if (s > ON_AUTO_MAX_SPLITS) s = ON_AUTO_MAX_SPLITS;
    return s < 1 ? 1 : s;
}

// the three entry points of the split scan: the same two launches, the scan instantiated with the row count by value, from the device,
// or with the ring's header from the device
// EXACT: the scan with the exact-match gate, the same merge, then the listing pass
template <int POOL, bool HORIZON = false, bool EXACT = false>
int launch_split(const char* who, const int32_t* db_t, const int32_t* qry_ids, const double* qry_idf, double* out_values,
                 int64_t* out_indices, int64_t* out_lens, void* workspace, size_t workspace_bytes, int64_t n_db, const int64_t* n_dev,
                 int64_t stride, int64_t n_qry, int n_fields, int topk, int splits, void* stream, const int64_t* before = nullptr,
                 uint32_t exact_mask = 0, const int32_t* listing = nullptr) {
    const size_t need = (size_t)n_qry * (size_t)splits * (size_t)topk * (sizeof(double) + sizeof(int64_t));
    if (workspace == nullptr || workspace_bytes < need)
        return rat_fail(std::string(who) + ": workspace smaller than rat_bm25_topk_split_workspace()");
    if (((uintptr_t)workspace & 7) != 0) return rat_fail(std::string(who) + ": workspace must be 8-byte aligned");
    SplitArgs a{};
    a.db_t = db_t;
    a.qry = qry_ids;
    a.idf = qry_idf;
    a.part_val = static_cast<double*>(workspace);
    a.part_idx = reinterpret_cast<int64_t*>(a.part_val + (size_t)n_qry * splits * topk);
    a.out_val = out_values;
    a.out_idx = out_indices;
    a.out_len = out_lens;
    a.N = n_db;
    a.Q = n_qry;
    a.F = n_fields;
    a.K = topk;
    a.splits = splits;
    a.n_dev = n_dev;
    a.stride = stride;
    a.before = before;
    a.exact_mask = exact_mask;
    a.listing = listing;
    if (topk <= 8) {
        const int64_t items = (n_qry + 3) / 4 * splits;
        RAT_LAUNCH((bm25_scan_split_kernel<8, 4, 4, POOL, HORIZON, EXACT>), (unsigned)(items < 65536 ? items : 65536), ON_THREADS, 0, stream, a);
    } else {
        const int64_t items = n_qry * splits;
        RAT_LAUNCH((bm25_scan_split_kernel<32, 1, 4, POOL, HORIZON, EXACT>), (unsigned)(items < 65536 ? items : 65536), ON_THREADS, 0, stream, a);
    }
    if (rat_check_launch(who) != 0) return -1;
    RAT_LAUNCH(bm25_merge_kernel, (unsigned)(n_qry < 65536 ? n_qry : 65536), 64, 0, stream, a);
    if constexpr (EXACT) {
        if (rat_check_launch(who) != 0) return -1;
        RAT_LAUNCH(bm25_exact_list_kernel, (unsigned)(n_qry < 65536 ? n_qry : 65536), 64, 0, stream, a);
    }
    return rat_check_launch(who);
}

// ------------------------------------------------------------------------------------------------------------ query-side IDF mapping
struct PrepArgs {
    const int32_t* ids;      // [Q][row_stride]
    const int32_t* cols;     // [F]
    const int32_t* tab_ids;  // per column: sorted distinct ids, concatenated
    const double* tab_idf;   // their weights
    const int64_t* tab_off;  // [F + 1]
    int32_t* qry_ids;        // [Q][F]
    double* qry_idf;         // [Q][F]
    int64_t Q;
    int row_stride, F;
    const int64_t* first_row;  // [Q], SEG only: the batch row that opens row q's request
};

// np.searchsorted(vals, x) clipped to the last entry, then vals[pos] == x (retrieval.map_data_to_idf): -> position or -1
__device__ __forceinline__ int64_t table_find(const int32_t* vals, int64_t n, int32_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (vals[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < n && vals[lo] == x ? lo : -1;
}

// SEG: the batch holds several requests, each one query batch of the reference — the dtype rule of row q looks at the first row of
// ITS request, first_row[q] (clamped to [0, Q): a corrupt array gives a wrong weight, never an address outside `ids`)
template <bool SEG>
__global__ void __launch_bounds__(256) bm25_query_prepare_kernel(PrepArgs a) {
    const int64_t total = a.Q * a.F;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t q = e / a.F;
        const int f = (int)(e % a.F);
        const int32_t* vals = a.tab_ids + a.tab_off[f];
        const double* idf = a.tab_idf + a.tab_off[f];
        const int64_t n = a.tab_off[f + 1] - a.tab_off[f];
        const int32_t x = a.ids[q * a.row_stride + a.cols[f]];
        const int64_t pos = table_find(vals, n, x);
        double w = pos >= 0 ? idf[pos] : 0.0;
        // the reference's np.vectorize takes the column's dtype from the batch's FIRST row: a miss there makes the column int64
        int64_t first = 0;
        if constexpr (SEG) {
            first = a.first_row[q];
            first = first < 0 ? 0 : (first < a.Q ? first : a.Q - 1);
        }
        if (table_find(vals, n, a.ids[first * a.row_stride + a.cols[f]]) < 0) w = (double)(int64_t)w;
        a.qry_ids[e] = x;
        a.qry_idf[e] = w;
    }
}

}  // namespace

extern "C" int rat_bm25_query_prepare(const int32_t* ids, const int32_t* cols, const int32_t* table_ids, const double* table_idf,
                                      const int64_t* table_offsets, int32_t* qry_ids, double* qry_idf, int64_t n_qry, int row_stride,
                                      int n_fields, void* stream) {
    RAT_REQUIRE(ids && cols && table_ids && table_idf && table_offsets && qry_ids && qry_idf, "null pointer");
    RAT_REQUIRE(n_qry > 0 && n_fields > 0 && row_stride > 0, "bad dims");
    RAT_REQUIRE(n_fields <= ON_FMAX, "more than 32 retrieval columns are not supported");
    PrepArgs a{ids, cols, table_ids, table_idf, table_offsets, qry_ids, qry_idf, n_qry, row_stride, n_fields, nullptr};
    const int64_t blocks = (n_qry * n_fields + 255) / 256;
    RAT_LAUNCH(bm25_query_prepare_kernel<false>, (unsigned)(blocks < 4096 ? blocks : 4096), 256, 0, stream, a);
    return rat_check_launch("rat_bm25_query_prepare");
}

extern "C" int rat_bm25_query_prepare_seg(const int32_t* ids, const int64_t* first_row, const int32_t* cols, const int32_t* table_ids,
                                          const double* table_idf, const int64_t* table_offsets, int32_t* qry_ids, double* qry_idf,
                                          int64_t n_qry, int row_stride, int n_fields, void* stream) {
    RAT_REQUIRE(ids && first_row && cols && table_ids && table_idf && table_offsets && qry_ids && qry_idf, "null pointer");
    RAT_REQUIRE(n_qry > 0 && n_fields > 0 && row_stride > 0, "bad dims");
    RAT_REQUIRE(n_fields <= ON_FMAX, "more than 32 retrieval columns are not supported");
    PrepArgs a{ids, cols, table_ids, table_idf, table_offsets, qry_ids, qry_idf, n_qry, row_stride, n_fields, first_row};
    const int64_t blocks = (n_qry * n_fields + 255) / 256;
    RAT_LAUNCH(bm25_query_prepare_kernel<true>, (unsigned)(blocks < 4096 ? blocks : 4096), 256, 0, stream, a);
    return rat_check_launch("rat_bm25_query_prepare_seg");
}

extern "C" size_t rat_bm25_topk_split_workspace(int64_t n_qry, int topk, int splits) {
    if (n_qry <= 0 || topk <= 0 || splits < 0) return 0;
    // splits = 0: the most the library may choose for this many queries (it does not know the pool yet)
    const int64_t s = splits > 0 ? splits : auto_splits(n_qry, INT64_MAX, topk);
    return (size_t)n_qry * (size_t)s * (size_t)topk * (sizeof(double) + sizeof(int64_t));
}

extern "C" int rat_bm25_topk_split(const int32_t* db_ids_field_major, const int32_t* qry_ids, const double* qry_idf, double* out_values,
                                   int64_t* out_indices, int64_t* out_lens, void* workspace, size_t workspace_bytes, int64_t n_db,
                                   int64_t n_qry, int n_fields, int topk, int splits, void* stream) {
    RAT_REQUIRE(db_ids_field_major && qry_ids && qry_idf && out_values && out_indices && out_lens, "null pointer");
    RAT_REQUIRE(n_db > 0 && n_qry > 0 && n_fields > 0 && topk > 0, "bad dims");
    RAT_REQUIRE(n_fields <= ON_FMAX, "more than 32 retrieval columns are not supported");
    RAT_REQUIRE(topk <= ON_KMAX, "topK > 32 is not supported");
    RAT_REQUIRE(splits >= 0 && splits <= ON_MAX_SPLITS, "splits must be 0 (library's choice) or 1..4096");
    if (splits == 0) {
        splits = (int)auto_splits(n_qry, n_db, topk);
        if (splits == 1)                               // the query tiles fill the chip: the single-range kernel, no second pass
            return rat_bm25_topk(db_ids_field_major, qry_ids, qry_idf, out_values, out_indices, out_lens, n_db, n_qry, n_fields, topk,
                                 stream);
    }
    return launch_split<POOL_HOST>("rat_bm25_topk_split", db_ids_field_major, qry_ids, qry_idf, out_values, out_indices, out_lens, workspace,
                               workspace_bytes, n_db, nullptr, n_db, n_qry, n_fields, topk, splits, stream);
}

extern "C" int rat_bm25_topk_split_dev(const int32_t* db_ids_field_major, const int64_t* n_db_dev, const int32_t* qry_ids,
                                       const double* qry_idf, double* out_values, int64_t* out_indices, int64_t* out_lens,
                                       void* workspace, size_t workspace_bytes, int64_t capacity, int64_t n_qry, int n_fields, int topk,
                                       int splits, void* stream) {
    RAT_REQUIRE(db_ids_field_major && n_db_dev && qry_ids && qry_idf && out_values && out_indices && out_lens, "null pointer");
    RAT_REQUIRE(capacity > 0 && n_qry > 0 && n_fields > 0 && topk > 0, "bad dims");
    RAT_REQUIRE(n_fields <= ON_FMAX, "more than 32 retrieval columns are not supported");
    RAT_REQUIRE(topk <= ON_KMAX, "topK > 32 is not supported");
    RAT_REQUIRE(splits >= 0 && splits <= ON_MAX_SPLITS, "splits must be 0 (library's choice) or 1..4096");
    // the launch shape may not depend on the row count (a captured launch serves the pool after it has grown): the rule of
    // rat_bm25_topk_split applied to the CAPACITY; where it would hand over to the single-range kernel, one range through this one
    if (splits == 0) splits = (int)auto_splits(n_qry, capacity, topk);
    return launch_split<POOL_DEV>("rat_bm25_topk_split_dev", db_ids_field_major, qry_ids, qry_idf, out_values, out_indices, out_lens, workspace,
                              workspace_bytes, 0, n_db_dev, capacity, n_qry, n_fields, topk, splits, stream);
}

extern "C" int rat_bm25_topk_split_ring(const int32_t* db_ids_field_major, const int64_t* header_dev, const int32_t* qry_ids,
                                        const double* qry_idf, double* out_values, int64_t* out_indices, int64_t* out_lens,
                                        void* workspace, size_t workspace_bytes, int64_t capacity, int64_t n_qry, int n_fields, int topk,
                                        int splits, void* stream) {
    RAT_REQUIRE(db_ids_field_major && header_dev && qry_ids && qry_idf && out_values && out_indices && out_lens, "null pointer");
    RAT_REQUIRE(capacity > 0 && n_qry > 0 && n_fields > 0 && topk > 0, "bad dims");
    RAT_REQUIRE(n_fields <= ON_FMAX, "more than 32 retrieval columns are not supported");
    RAT_REQUIRE(topk <= ON_KMAX, "topK > 32 is not supported");
    RAT_REQUIRE(splits >= 0 && splits <= ON_MAX_SPLITS, "splits must be 0 (library's choice) or 1..4096");
    if (splits == 0) splits = (int)auto_splits(n_qry, capacity, topk);       // from the capacity, as rat_bm25_topk_split_dev
    return launch_split<POOL_RING>("rat_bm25_topk_split_ring", db_ids_field_major, qry_ids, qry_idf, out_values, out_indices, out_lens,
                                   workspace, workspace_bytes, 0, header_dev, capacity, n_qry, n_fields, topk, splits, stream);
}

// ------------------------------------------------------------------------------------------------------------ growing the pool
namespace {

struct AppendArgs {
    const int32_t* ids;      // [M][L] the new rows
    const float* labels;     // [M]
    const int32_t* cols;     // [F]
    int32_t* db_t;           // [F][capacity]
    int32_t* pool_ids;       // [capacity][L]   (nullable, with pool_labels: an index without the scorer's row store)
    float* pool_labels;      // [capacity]
    int64_t* count;          // the header: rows in the pool
    int64_t M, capacity;
    int L, F;
};

// Work items e: [0, F * M) the field-major side — e = f * M + i, so 64 consecutive lanes write 64 consecutive rows of one column
// (one 256-byte store per wave; the reads are L ints apart) — then [F * M, F * M + M * L) the row-major side, a straight copy
// (pool_ids[n + i][c] is word n * L + e), the first M of which also carry a label.  n comes from the header; a batch that would not
// fit writes nothing (the host refuses it before; this is the bound on the device).
__global__ void __launch_bounds__(256) pool_append_kernel(AppendArgs a) {
    const int64_t n = *a.count;
    if (n < 0 || n + a.M > a.capacity) return;
    const int64_t nt = (int64_t)a.F * a.M;
    const int64_t total = nt + (a.pool_ids ? a.M * a.L : 0);
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        if (e < nt) {
            const int64_t f = e / a.M, i = e % a.M;
            a.db_t[f * a.capacity + n + i] = a.ids[i * a.L + a.cols[f]];
        } else {
            const int64_t r = e - nt;
            a.pool_ids[n * a.L + r] = a.ids[r];
            if (r < a.M) a.pool_labels[n + r] = a.labels[r];
        }
    }
}

// the tail launch: the rows are in place (stream order), now they count
__global__ void __launch_bounds__(64) pool_commit_kernel(int64_t* count, int64_t M, int64_t capacity) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const int64_t n = *count;
        if (n >= 0 && n + M <= capacity) *count = n + M;
    }
}

}  // namespace

extern "C" int rat_pool_append(const int32_t* ids, const float* labels, const int32_t* cols, int32_t* db_ids_field_major,
                               int32_t* pool_ids, float* pool_labels, int64_t* n_db_dev, int64_t n_rows, int64_t capacity,
                               int row_len, int n_fields, void* stream) {
    RAT_REQUIRE(ids && cols && db_ids_field_major && n_db_dev, "null pointer");
    RAT_REQUIRE((pool_ids == nullptr) == (pool_labels == nullptr), "pool_ids and pool_labels go together");
    RAT_REQUIRE(pool_ids == nullptr || labels != nullptr, "null labels");
    RAT_REQUIRE(n_rows > 0 && capacity > 0 && n_rows <= capacity && row_len > 0 && n_fields > 0, "bad dims");
    RAT_REQUIRE(n_fields <= ON_FMAX, "more than 32 retrieval columns are not supported");
    AppendArgs a{ids, labels, cols, db_ids_field_major, pool_ids, pool_labels, n_db_dev, n_rows, capacity, row_len, n_fields};
    const int64_t blocks = (n_rows * (n_fields + (pool_ids ? row_len : 0)) + 255) / 256;
    RAT_LAUNCH(pool_append_kernel, (unsigned)(blocks < 4096 ? blocks : 4096), 256, 0, stream, a);
    if (rat_check_launch("rat_pool_append") != 0) return -1;
    RAT_LAUNCH(pool_commit_kernel, 1u, 64, 0, stream, n_db_dev, n_rows, capacity);
    return rat_check_launch("rat_pool_append");
}

// ------------------------------------------------------------------------------------------------------------ a pool that slides
// The same buffers as a ring: the header is {n, head}, logical row i lives in slot head + i (wrapped once).  A push that does not fit
// overwrites the oldest rows — they leave the window in the tail launch, after the new rows are in place.
namespace {

struct RingHeader {
    int64_t n, head;
    bool ok;
};
// the header as both launches of a push and the evict read it; a header outside its domain (never written by these kernels) stops them
__device__ __forceinline__ RingHeader ring_header(const int64_t* header, int64_t capacity) {
    RingHeader h{header[0], header[1], false};
    h.ok = h.n >= 0 && h.n <= capacity && h.head >= 0 && h.head < capacity;
    return h;
}

// pool_append_kernel's work items, every destination through the ring: row i of the batch goes to slot base + i (wrapped) with
// base = head + n (wrapped) — the slot behind the newest row, which is the oldest row's once the window is full.  64 consecutive lanes
// still write 64 consecutive slots of a column, in two pieces where the wrap falls among them; on the row-major side word r of the
// batch goes to word base * L + r of pool_ids, wrapped at capacity * L.  AppendArgs::count is the two-word header here.
__global__ void __launch_bounds__(256) pool_push_kernel(AppendArgs a) {
    const RingHeader h = ring_header(a.count, a.capacity);
    if (!h.ok || a.M > a.capacity) return;
    const int64_t base = ring_wrap(h.head + h.n, a.capacity);
    const int64_t nt = (int64_t)a.F * a.M;
    const int64_t total = nt + (a.pool_ids ? a.M * a.L : 0);
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        if (e < nt) {
            const int64_t f = e / a.M, i = e % a.M;
            a.db_t[f * a.capacity + ring_wrap(base + i, a.capacity)] = a.ids[i * a.L + a.cols[f]];
        } else {
            const int64_t r = e - nt;
            a.pool_ids[ring_wrap(base * a.L + r, a.capacity * a.L)] = a.ids[r];
            if (r < a.M) a.pool_labels[ring_wrap(base + r, a.capacity)] = a.labels[r];
        }
    }
}

// the tail launch of a push: the E = max(0, n + M - capacity) oldest rows leave, the M new ones count
__global__ void __launch_bounds__(64) pool_push_commit_kernel(int64_t* header, int64_t M, int64_t capacity) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const RingHeader h = ring_header(header, capacity);
        if (!h.ok || M > capacity) return;
        const int64_t E = h.n + M > capacity ? h.n + M - capacity : 0;
        header[1] = ring_wrap(h.head + E, capacity);
        header[0] = h.n + M - E;
    }
}

// the m oldest rows leave; the pool never becomes empty (a fresh index refuses an empty pool)
__global__ void __launch_bounds__(64) pool_evict_kernel(int64_t* header, int64_t m, int64_t capacity) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const RingHeader h = ring_header(header, capacity);
        if (!h.ok || m < 0 || m >= h.n) return;
        header[1] = ring_wrap(h.head + m, capacity);
        header[0] = h.n - m;
    }
}

}  // namespace

extern "C" int rat_pool_push(const int32_t* ids, const float* labels, const int32_t* cols, int32_t* db_ids_field_major, int32_t* pool_ids,
                             float* pool_labels, int64_t* header_dev, int64_t n_rows, int64_t capacity, int row_len, int n_fields,
                             void* stream) {
    RAT_REQUIRE(ids && cols && db_ids_field_major && header_dev, "null pointer");
    RAT_REQUIRE((pool_ids == nullptr) == (pool_labels == nullptr), "pool_ids and pool_labels go together");
    RAT_REQUIRE(pool_ids == nullptr || labels != nullptr, "null labels");
    RAT_REQUIRE(n_rows > 0 && capacity > 0 && row_len > 0 && n_fields > 0, "bad dims");
    RAT_REQUIRE(n_fields <= ON_FMAX, "more than 32 retrieval columns are not supported");
    if (n_rows > capacity) return 0;                   // more rows than the window holds: nothing is written, the header stays
    AppendArgs a{ids, labels, cols, db_ids_field_major, pool_ids, pool_labels, header_dev, n_rows, capacity, row_len, n_fields};
    const int64_t blocks = (n_rows * (n_fields + (pool_ids ? row_len : 0)) + 255) / 256;
    RAT_LAUNCH(pool_push_kernel, (unsigned)(blocks < 4096 ? blocks : 4096), 256, 0, stream, a);
    if (rat_check_launch("rat_pool_push") != 0) return -1;
    RAT_LAUNCH(pool_push_commit_kernel, 1u, 64, 0, stream, header_dev, n_rows, capacity);
    return rat_check_launch("rat_pool_push");
}

extern "C" int rat_pool_evict(int64_t* header_dev, int64_t n_rows, int64_t capacity, void* stream) {
    RAT_REQUIRE(header_dev, "null pointer");
    RAT_REQUIRE(capacity > 0, "bad dims");
    RAT_LAUNCH(pool_evict_kernel, 1u, 64, 0, stream, header_dev, n_rows, capacity);
    return rat_check_launch("rat_pool_evict");
}

// ------------------------------------------------------------------------------------------------------------ a pool that loses rows
// rat_pool_delete: the rows named by a strictly ascending list of logical indices leave the ring, the survivors close up in age order.
// Survivor j ends at logical j - #{deleted < j}: a destination is at or before its source and the ranges overlap, so the move is
// staged — per store ("plane"), launch 1 gathers the survivors of the suffix [del[0], n) into scratch in compact order, launch 2
// copies them back from logical del[0] on; stream order is the only ordering between work-groups.  Both are destination-driven:
// compact position j' takes logical row j' + k, k = the number of list entries with del[k] - k <= j' (that sequence is
// non-decreasing: a binary search).  Rows older than del[0] are not touched, head does not move, the tail launch sets n -= n_del.
namespace {

struct DeleteArgs {
    int32_t* db_t;           // [F][capacity]
    int32_t* pool_ids;       // [capacity][L]   (nullable, with pool_labels)
    float* pool_labels;      // [capacity]
    const int64_t* header;   // {n, head}
    const int64_t* del;      // [n_del] logical indices, strictly ascending
    int32_t* scratch;        // capacity * max(F, L) words (capacity * F without the row store)
    int64_t n_del, capacity;
    int L, F;
};

enum { PLANE_DB_T = 0, PLANE_IDS = 1, PLANE_LABELS = 2 };
constexpr int64_t DEL_ITEMS_PER_THREAD = 4;            // the grid is sized for this many words per thread at the full capacity

// What both launches of a plane see.  n is clamped to [0, capacity], head to [0, capacity) (pool_view) and del[0] to [0, n]:
// compact positions are [first, n - n_del) and a source is j' + k <= n - n_del - 1 + n_del, a live row whatever
// the list holds — nothing outside the buffers is addressed for any header or list content.
struct DeleteView {
    int64_t n, head, first, count;                     // count = survivors of the suffix = compact positions to move
};
__device__ __forceinline__ DeleteView delete_view(const DeleteArgs& a) {
    const PoolView pool = pool_view<POOL_RING>(a.header, 0, a.capacity);
    DeleteView v;
    v.n = pool.n;
    v.head = pool.head;
    v.first = a.del[0];
    v.first = v.first < 0 ? 0 : (v.first > v.n ? v.n : v.first);
    v.count = v.n - a.n_del - v.first;
    v.count = v.count < 0 ? 0 : v.count;
    return v;
}
// number of list entries k with del[k] - k <= j
__device__ __forceinline__ int64_t deleted_up_to(const int64_t* del, int64_t n_del, int64_t j) {
    int64_t lo = 0, hi = n_del;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (del[mid] - mid <= j)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// Work items e of a plane, as pool_push_kernel addresses the stores: db_t — e = f * count + i, 64 consecutive lanes move 64
// consecutive rows of one column (in two pieces where the wrap falls among them); pool_ids — word e = i * L + c of the compact rows;
// labels — e = i.  BACK = false: scratch[e] = store[slot of logical first + i + k]; BACK = true: store[slot of logical first + i] =
// scratch[e].
template <int PLANE, bool BACK>
__global__ void __launch_bounds__(256) pool_delete_move_kernel(DeleteArgs a) {
    const DeleteView v = delete_view(a);
    const int64_t width = PLANE == PLANE_DB_T ? a.F : (PLANE == PLANE_IDS ? a.L : 1);
    const int64_t total = v.count * width;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = PLANE == PLANE_DB_T ? e % v.count : (PLANE == PLANE_IDS ? e / a.L : e);
        const int64_t w = PLANE == PLANE_DB_T ? e / v.count : (PLANE == PLANE_IDS ? e % a.L : 0);      // column f / word c of the row
        int64_t row = v.first + i;
        if constexpr (!BACK) row += deleted_up_to(a.del, a.n_del, row);
        const int64_t slot = ring_wrap(v.head + row, a.capacity);
        if constexpr (PLANE == PLANE_LABELS) {
            float* lab = reinterpret_cast<float*>(a.scratch);
            if constexpr (BACK)
                a.pool_labels[slot] = lab[e];
            else
                lab[e] = a.pool_labels[slot];
        } else {
            int32_t* at = PLANE == PLANE_DB_T ? a.db_t + w * a.capacity + slot : a.pool_ids + slot * a.L + w;
            if constexpr (BACK)
                *at = a.scratch[e];
            else
                a.scratch[e] = *at;
        }
    }
}

// the tail launch: the survivors are in place (stream order), now the deleted rows stop counting; the pool never becomes empty
__global__ void __launch_bounds__(64) pool_delete_commit_kernel(int64_t* header, int64_t n_del, int64_t capacity) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const RingHeader h = ring_header(header, capacity);
        if (!h.ok || n_del <= 0 || n_del >= h.n) return;
        header[0] = h.n - n_del;
    }
}

template <int PLANE>
int launch_delete_plane(const DeleteArgs& a, int64_t width, void* stream) {
    const int64_t per_block = 256 * DEL_ITEMS_PER_THREAD;
    const int64_t blocks = (a.capacity * width + per_block - 1) / per_block;
    const unsigned grid = (unsigned)(blocks < 4096 ? blocks : 4096);
    RAT_LAUNCH((pool_delete_move_kernel<PLANE, false>), grid, 256, 0, stream, a);
    if (rat_check_launch("rat_pool_delete") != 0) return -1;
    RAT_LAUNCH((pool_delete_move_kernel<PLANE, true>), grid, 256, 0, stream, a);
    return rat_check_launch("rat_pool_delete");
}

}  // namespace

extern "C" int rat_pool_delete(int32_t* db_ids_field_major, int32_t* pool_ids, float* pool_labels, int64_t* header_dev,
                               const int64_t* del_dev, void* scratch, size_t scratch_bytes, int64_t n_del, int64_t capacity, int row_len,
                               int n_fields, void* stream) {
    RAT_REQUIRE(db_ids_field_major && header_dev, "null pointer");
    RAT_REQUIRE((pool_ids == nullptr) == (pool_labels == nullptr), "pool_ids and pool_labels go together");
    RAT_REQUIRE(capacity > 0 && row_len > 0 && n_fields > 0, "bad dims");
    RAT_REQUIRE(n_fields <= ON_FMAX, "more than 32 retrieval columns are not supported");
    if (n_del <= 0) return 0;                          // nothing to delete: nothing is launched
    RAT_REQUIRE(del_dev && scratch, "null pointer");
    RAT_REQUIRE(n_del <= capacity, "more deletions than the window holds rows");
    const int64_t width = pool_ids && row_len > n_fields ? row_len : n_fields;
    RAT_REQUIRE(scratch_bytes / sizeof(int32_t) / (size_t)capacity >= (size_t)width, "scratch smaller than the largest store");
    RAT_REQUIRE(((uintptr_t)scratch & 3) == 0, "scratch must be 4-byte aligned");
    DeleteArgs a{db_ids_field_major, pool_ids, pool_labels, header_dev, del_dev, static_cast<int32_t*>(scratch), n_del, capacity,
                 row_len, n_fields};
    if (launch_delete_plane<PLANE_DB_T>(a, n_fields, stream) != 0) return -1;
    if (pool_ids) {
        if (launch_delete_plane<PLANE_IDS>(a, row_len, stream) != 0) return -1;
        if (launch_delete_plane<PLANE_LABELS>(a, 1, stream) != 0) return -1;
    }
    RAT_LAUNCH(pool_delete_commit_kernel, 1u, 64, 0, stream, header_dev, n_del, capacity);
    return rat_check_launch("rat_pool_delete");
}

// ------------------------------------------------------------------------------------------------------------ a pool addressed by key
// rat_pool_find: the logical indices (ascending) of the live rows that equal one of M keys on C columns.  One kernel serves both
// stores through two strides — word (slot, c) is store[slot * row_stride + cols[c] * col_stride]: db_t has row stride 1 and column
// stride capacity (or N), a wave reads 64 consecutive rows of a column; pool_ids has row stride L and column stride 1, the C columns
// of a row share cache lines.  Three launches, kernel boundaries the only ordering between work-groups (as rat_pool_delete: nobody
// waits on a flag, and the ORDER of the output needs no atomic):
//   1  work-group g owns the logical range [g R, (g + 1) R), R = ceil(n / groups) from the row count read on the device (ranges past
//      the end are empty); a thread looks its row up in the sorted key table (binary search) and the group's match count goes to ws[g]
//   2  one work-group: exclusive offsets of the counts -> ws[groups + g], the total -> ws[2 groups] and out_count
//   3  the same ranges, the same test: a shuffle scan over the wave and the waves' sums through LDS give every match its rank inside
//      the group, and the logical index goes to out_idx[offset + rank] if that is < max_out; the grid then fills out_idx[min(total,
//      max_out) .. max_out) with -1 — so the list can be handed on whole (rat_pool_set_labels skips -1), no count read back.
// rat_pool_set_labels writes labels through the ring at such a list.
namespace {

constexpr int FIND_THREADS = 256;
constexpr int FIND_WAVES = FIND_THREADS / 64;
constexpr int FIND_MAX_COLS = 32;
constexpr int FIND_MAX_GROUPS = 4096;
// groups = 0: from the capacity only (the grid may not depend on the live count: a find queues behind pushes, evictions and
// deletions) — four trips of a work-group per range at the full capacity, at most RAT_POOL_FIND_AUTO_GROUPS ranges
constexpr int64_t FIND_AUTO_ROWS = 4 * FIND_THREADS;

struct FindArgs {
    const int32_t* store;
    int64_t row_stride, col_stride;
    const int64_t* header;   // POOL_DEV: {n}; POOL_RING: {n, head}; POOL_HOST: not read
    int64_t N, capacity;     // N: the row count of POOL_HOST; capacity: the rows (slots) the store holds
    const int32_t* cols;     // [C] positions inside the store, clamped to [0, store_cols)
    const int32_t* keys;     // [M][C] sorted lexicographically (signed), distinct
    int64_t M;
    int C, store_cols, groups;
    int64_t* out_idx;        // [max_out]
    int64_t* out_count;      // [1]
    int64_t max_out;
    int64_t* ws;             // [groups] counts, [groups] exclusive offsets, [1] total
};

__device__ __forceinline__ int64_t find_col_offset(const FindArgs& a, int c) {     // wave-uniform: scalar loads
    int64_t col = a.cols[c];
    col = col < 0 ? 0 : (col >= a.store_cols ? a.store_cols - 1 : col);
    return col * a.col_stride;
}

// Is the C-tuple of the row in `slot` one of the keys?  Lower bound of the tuple in the key table; column 0 of the row stays in a
// register and decides almost every step, the others are read (again, from cache) only where column 0 ties.  mid stays in [0, M)
// and the interval shrinks every step whatever the table holds: an unsorted table gives a wrong answer, never a wrong address.
__device__ __forceinline__ bool find_row_matches(const FindArgs& a, int64_t slot) {
    const int32_t* row = a.store + slot * a.row_stride;
    const int32_t v0 = row[find_col_offset(a, 0)];
    int64_t lo = 0, hi = a.M;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int32_t* key = a.keys + mid * a.C;
        bool less = key[0] < v0, equal = key[0] == v0;
        for (int c = 1; equal && c < a.C; ++c) {
            const int32_t v = row[find_col_offset(a, c)];
            less = key[c] < v;
            equal = key[c] == v;
        }
        if (equal) return true;
        if (less)
            lo = mid + 1;
        else
            hi = mid;
    }
    return false;
}

template <int POOL, bool WRITE>
__global__ void __launch_bounds__(FIND_THREADS) pool_find_kernel(FindArgs a) {
    __shared__ int wave_sum[FIND_WAVES];
    const int tid = threadIdx.x, lane = rat_lane(), wave = rat_wave();
    const PoolView v = pool_view<POOL>(a.header, a.N, a.capacity);
    const int64_t R = (v.n + a.groups - 1) / a.groups;
    const int64_t g = blockIdx.x;
    const int64_t lo = g * R < v.n ? g * R : v.n;                              // ranges past the end of the pool are empty
    const int64_t hi = lo + R < v.n ? lo + R : v.n;
    [[maybe_unused]] int64_t base = 0;                                         // WRITE: where the trip's first match goes
    if constexpr (WRITE) base = a.ws[a.groups + g];
    int count = 0;
    for (int64_t i0 = lo; i0 < hi; i0 += FIND_THREADS) {                       // the trip count is the same in every thread
        const int64_t i = i0 + tid;
        const int hit = i < hi && find_row_matches(a, ring_wrap(v.head + i, a.capacity)) ? 1 : 0;
        if constexpr (!WRITE) {
            count += hit;
        } else {
            int incl = hit;                                                    // matches of this wave up to and including this lane
            for (int d = 1; d < 64; d <<= 1) {
                const int below = __shfl(incl, (lane - d) & 63);
                if (lane >= d) incl += below;
            }
            if (lane == 63) wave_sum[wave] = incl;
            __syncthreads();
            int before = 0, all = 0;
            for (int w = 0; w < FIND_WAVES; ++w) {
                const int s = wave_sum[w];
                all += s;
                before += w < wave ? s : 0;
            }
            const int64_t pos = base + before + incl - hit;
            if (hit && pos < a.max_out) a.out_idx[pos] = i;
            base += all;
            __syncthreads();                                                   // the next trip reuses wave_sum
        }
    }
    if constexpr (!WRITE) {
        for (int d = 32; d > 0; d >>= 1) count += __shfl_xor(count, d);
        if (lane == 0) wave_sum[wave] = count;
        __syncthreads();
        if (tid == 0) {
            int64_t sum = 0;
            for (int w = 0; w < FIND_WAVES; ++w) sum += wave_sum[w];
            a.ws[g] = sum;
        }
    } else {
        int64_t first = a.ws[2 * (int64_t)a.groups];                           // the total; the tail behind the matches is -1
        first = first < 0 ? 0 : (first > a.max_out ? a.max_out : first);
        for (int64_t j = first + g * FIND_THREADS + tid; j < a.max_out; j += (int64_t)gridDim.x * FIND_THREADS) a.out_idx[j] = -1;
    }
}

// launch 2: thread t takes `per` consecutive counts; its offset is the sum of the threads' sums before it
__global__ void __launch_bounds__(FIND_THREADS) pool_find_offsets_kernel(int64_t* ws, int64_t* out_count, int groups) {
    __shared__ int64_t part[FIND_THREADS];
    const int tid = threadIdx.x;
    const int per = (groups + FIND_THREADS - 1) / FIND_THREADS;
    const int g0 = tid * per < groups ? tid * per : groups;
    const int g1 = g0 + per < groups ? g0 + per : groups;
    int64_t sum = 0;
    for (int g = g0; g < g1; ++g) sum += ws[g];
    part[tid] = sum;
    __syncthreads();
    int64_t before = 0;
    for (int t = 0; t < tid; ++t) before += part[t];
    for (int g = g0; g < g1; ++g) {
        ws[groups + g] = before;
        before += ws[g];
    }
    if (tid == FIND_THREADS - 1) {                                             // the last thread's running sum is the total
        ws[2 * (int64_t)groups] = before;
        out_count[0] = before;
    }
}

template <int POOL>
int launch_find(const FindArgs& a, void* stream) {
    RAT_LAUNCH((pool_find_kernel<POOL, false>), (unsigned)a.groups, FIND_THREADS, 0, stream, a);
    if (rat_check_launch("rat_pool_find") != 0) return -1;
    RAT_LAUNCH(pool_find_offsets_kernel, 1u, FIND_THREADS, 0, stream, a.ws, a.out_count, a.groups);
    if (rat_check_launch("rat_pool_find") != 0) return -1;
    RAT_LAUNCH((pool_find_kernel<POOL, true>), (unsigned)a.groups, FIND_THREADS, 0, stream, a);
    return rat_check_launch("rat_pool_find");
}

struct SetLabelsArgs {
    float* pool_labels;      // [capacity]
    const int64_t* header;
    const int64_t* indices;  // [m] logical; < 0 or >= n: skipped
    const float* labels;     // [m], or [1] with label_stride = 0
    int64_t N, capacity, m;
    int label_stride;
};

template <int POOL>
__global__ void __launch_bounds__(256) pool_set_labels_kernel(SetLabelsArgs a) {
    const PoolView v = pool_view<POOL>(a.header, a.N, a.capacity);
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < a.m; j += (int64_t)gridDim.x * 256) {
        const int64_t i = a.indices[j];
        if (i >= 0 && i < v.n) a.pool_labels[ring_wrap(v.head + i, a.capacity)] = a.labels[j * a.label_stride];
    }
}

}  // namespace

extern "C" int rat_pool_find(const int32_t* store, int64_t row_stride, int64_t col_stride, int store_cols, int pool_form,
                             const int64_t* header_dev, int64_t n_rows, int64_t capacity, const int32_t* cols, int n_cols,
                             const int32_t* keys, int64_t n_keys, int64_t* out_idx, int64_t max_out, int64_t* out_count, void* workspace,
                             size_t workspace_bytes, int groups, void* stream) {
    RAT_REQUIRE(store && cols && keys && out_count && workspace, "null pointer");
    RAT_POOL_FORM_CHECK(pool_form, header_dev, n_rows, capacity,
                        capacity > 0 && row_stride > 0 && col_stride > 0 && store_cols > 0 && n_keys > 0 && max_out >= 0);
    RAT_REQUIRE(n_cols > 0 && n_cols <= FIND_MAX_COLS, "1 to 32 key columns are supported");
    RAT_REQUIRE(max_out == 0 || out_idx, "null out_idx");
    RAT_REQUIRE(groups >= 0 && groups <= FIND_MAX_GROUPS, "groups must be 0 (library's choice) or 1..4096");
    if (groups == 0) {
        const int64_t by_rows = (capacity + FIND_AUTO_ROWS - 1) / FIND_AUTO_ROWS;
        groups = (int)(by_rows < RAT_POOL_FIND_AUTO_GROUPS ? by_rows : RAT_POOL_FIND_AUTO_GROUPS);
    }
    RAT_REQUIRE((capacity + groups - 1) / groups <= INT32_MAX, "more than 2^31 - 1 rows per range: pass more groups");
    RAT_REQUIRE(workspace_bytes / sizeof(int64_t) >= 2 * (size_t)groups + 1, "workspace smaller than 8 (2 groups + 1) bytes");
    RAT_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
    FindArgs a{store, row_stride, col_stride, header_dev, n_rows, capacity, cols, keys, n_keys, n_cols, store_cols, groups,
               out_idx, out_count, max_out, static_cast<int64_t*>(workspace)};
    return dispatch_pool(pool_form, [&](auto form) { return launch_find<decltype(form)::value>(a, stream); });
}

extern "C" int rat_pool_set_labels(float* pool_labels, int pool_form, const int64_t* header_dev, int64_t n_rows, int64_t capacity,
                                   const int64_t* indices, const float* labels, int64_t m, int label_stride, void* stream) {
    RAT_REQUIRE(pool_labels, "null pointer");
    RAT_POOL_FORM_CHECK(pool_form, header_dev, n_rows, capacity, capacity > 0);
    RAT_REQUIRE(label_stride == 0 || label_stride == 1, "label_stride must be 1 (a label per index) or 0 (one label for all)");
    if (m <= 0) return 0;                              // nothing to write: nothing is launched
    RAT_REQUIRE(indices && labels, "null pointer");
    SetLabelsArgs a{pool_labels, header_dev, indices, labels, n_rows, capacity, m, label_stride};
    const int64_t blocks = (m + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 4096 ? blocks : 4096);
    dispatch_pool(pool_form, [&](auto form) { RAT_LAUNCH(pool_set_labels_kernel<decltype(form)::value>, grid, 256, 0, stream, a); });
    return rat_check_launch("rat_pool_set_labels");
}

// ------------------------------------------------------------------------------------------------------------ a pool that looks at itself
// rat_pool_gather_rows: ids and labels of the logical rows indices[B] out of the row store, through the pool form, and every row's
// own logical index — its horizon: the rows older than it — for rat_bm25_topk_split_before, which scans with that horizon per query.
// The two are chained on a stream with nothing read back in between.
namespace {

struct GatherRowsArgs {
    const int32_t* pool_ids;     // [capacity][L]
    const float* pool_labels;    // [capacity]
    const int64_t* header;
    const int64_t* indices;      // [B] logical; < 0 or >= n: a row of zeros, label 0
    int32_t* out_ids;            // [B][L]
    float* out_labels;           // [B]
    int64_t* out_before;         // [B] indices[j] clamped to [0, n]
    int64_t N, capacity, B;
    int L;
};

// work item e = word (j, c) of out_ids: consecutive lanes copy consecutive words of a row; the lane of a row's first word also
// writes its label and its horizon
template <int POOL>
__global__ void __launch_bounds__(256) pool_gather_rows_kernel(GatherRowsArgs a) {
    const PoolView v = pool_view<POOL>(a.header, a.N, a.capacity);
    const int64_t total = a.B * a.L;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t j = e / a.L;
        const int c = (int)(e % a.L);
        const int64_t i = a.indices[j];
        const bool live = i >= 0 && i < v.n;
        const int64_t slot = live ? ring_wrap(v.head + i, a.capacity) : 0;
        a.out_ids[e] = live ? a.pool_ids[slot * a.L + c] : 0;
        if (c == 0) {
            a.out_labels[j] = live ? a.pool_labels[slot] : 0.0f;
            a.out_before[j] = i < 0 ? 0 : (i > v.n ? v.n : i);
        }
    }
}

}  // namespace

extern "C" int rat_pool_gather_rows(const int32_t* pool_ids, const float* pool_labels, int pool_form, const int64_t* header_dev,
                                    int64_t n_rows, int64_t capacity, const int64_t* indices, int32_t* out_ids, float* out_labels,
                                    int64_t* out_before, int64_t n_indices, int row_len, void* stream) {
    RAT_REQUIRE(pool_ids && pool_labels, "null pointer");
    RAT_POOL_FORM_CHECK(pool_form, header_dev, n_rows, capacity, capacity > 0 && row_len > 0);
    if (n_indices <= 0) return 0;                      // nothing to gather: nothing is launched
    RAT_REQUIRE(indices && out_ids && out_labels && out_before, "null pointer");
    GatherRowsArgs a{pool_ids, pool_labels, header_dev, indices, out_ids, out_labels, out_before, n_rows, capacity, n_indices, row_len};
    const int64_t blocks = (n_indices * row_len + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 4096 ? blocks : 4096);
    dispatch_pool(pool_form, [&](auto form) { RAT_LAUNCH(pool_gather_rows_kernel<decltype(form)::value>, grid, 256, 0, stream, a); });
    return rat_check_launch("rat_pool_gather_rows");
}

extern "C" int rat_bm25_topk_split_before(const int32_t* db_ids_field_major, int pool_form, const int64_t* header_dev, int64_t n_rows,
                                          int64_t capacity, const int32_t* qry_ids, const double* qry_idf, const int64_t* before_dev,
                                          double* out_values, int64_t* out_indices, int64_t* out_lens, void* workspace,
                                          size_t workspace_bytes, int64_t n_qry, int n_fields, int topk, int splits, void* stream) {
    RAT_REQUIRE(db_ids_field_major && qry_ids && qry_idf && before_dev && out_values && out_indices && out_lens, "null pointer");
    RAT_POOL_FORM_CHECK(pool_form, header_dev, n_rows, capacity, capacity > 0 && n_qry > 0 && n_fields > 0 && topk > 0);
    RAT_REQUIRE(n_fields <= ON_FMAX, "more than 32 retrieval columns are not supported");
    RAT_REQUIRE(topk <= ON_KMAX, "topK > 32 is not supported");
    RAT_REQUIRE(splits >= 0 && splits <= ON_MAX_SPLITS, "splits must be 0 (library's choice) or 1..4096");
    // from the capacity in every form, as rat_bm25_topk_split_dev: one range too goes through the split kernel, which has the horizon
    if (splits == 0) splits = (int)auto_splits(n_qry, capacity, topk);
    // POOL_HOST: the row count by value and no header; otherwise the header and no count
    return dispatch_pool(pool_form, [&](auto form) {
        constexpr int POOL = decltype(form)::value;
        return launch_split<POOL, true>("rat_bm25_topk_split_before", db_ids_field_major, qry_ids, qry_idf, out_values, out_indices, out_lens,
                                        workspace, workspace_bytes, POOL == POOL_HOST ? n_rows : 0, POOL == POOL_HOST ? nullptr : header_dev,
                                        capacity, n_qry, n_fields, topk, splits, stream, before_dev);
    });
}

// ------------------------------------------------------------------------------------------------------------ neighbours equal on given columns
// Exact-match retrieval on the request path (rat_amd/retrieval.py: exact_match_col_indices; the offline job numbers the groups on the
// host and hands them to rat_bm25_topk_grouped).  Here nobody numbers anything: the scan compares the query's ids on the exact columns
// with the row's ids — db_t holds every used column — and the two batch-wide rules of the offline path are decided on the device from
// the candidate counts, with nothing read back:
//   rat_bm25_exact_count   c[q] = live rows (below q's horizon) equal to query q on every exact column: work-group (query tile, range)
//                          counts its range into ws[q][range], a second launch sums a query's partials in range order — integers,
//                          one result whatever the grid
//   rat_bm25_exact_plan    first_row[q] = the first query with a candidate (what rat_bm25_query_prepare_seg takes its dtype rule
//                          from: the offline path drops candidate-less queries before it maps the weights), and the listing flag
//   rat_bm25_topk_split_exact   the gated scan, the merge and the listing pass (launch_split<POOL, true, true>)
namespace {

constexpr int EC_THREADS = 256;
constexpr int EC_WAVES = EC_THREADS / 64;
constexpr int EC_QT = 8;                               // queries per work-group: their ids on the exact columns are staged in LDS
static_assert(ON_FMAX * EC_QT <= EC_THREADS, "one thread stages one (exact column, query) id");
constexpr int EC_MAX_GROUPS = 4096;
// groups = 0: from the capacity and the number of queries only — enough ranges for EC_TARGET_GROUPS work-groups (the kernel is small:
// a CU holds many), every range at least one full trip of four waves over four rows each, at most RAT_BM25_EXACT_AUTO_GROUPS
constexpr int64_t EC_TARGET_GROUPS = 1024;
constexpr int64_t EC_MIN_RANGE_ROWS = 1024;

struct ExactCountArgs {
    const int32_t* db_t;     // [F][capacity]
    const int32_t* ids;      // [Q][row_stride] the request's encoded rows
    const int32_t* cols;     // [F] used column f -> its column of `ids`, clamped to [0, row_stride)
    const int64_t* header;
    const int64_t* before;   // [Q] or null
    int64_t* ws;             // [Q][groups]
    int64_t* counts;         // [Q]
    int64_t N, capacity, Q;
    int row_stride, F, groups;
    uint32_t mask;
};

template <int POOL>
__global__ void __launch_bounds__(EC_THREADS) bm25_exact_count_kernel(ExactCountArgs a) {
    __shared__ int wave_sum[EC_WAVES][EC_QT];
    __shared__ int32_t qid_s[ON_FMAX][EC_QT];          // the tile's ids on the exact columns, exact column e = 0 .. n_exact - 1
    __shared__ int field_s[ON_FMAX];                   // exact column e -> its used column f
    const int tid = threadIdx.x, lane = rat_lane(), wave = rat_wave();
    const PoolView v = pool_view<POOL>(a.header, a.N, a.capacity);
    int n_exact = 0;                                   // the same in every thread: the mask is a kernel argument
    for (int f = 0; f < a.F; ++f) {
        if (((a.mask >> f) & 1u) == 0) continue;
        if (tid == 0) field_s[n_exact] = f;
        ++n_exact;
    }
    const int64_t R = (v.n + a.groups - 1) / a.groups;
    const int64_t ntiles = (a.Q + EC_QT - 1) / EC_QT;
    for (int64_t item = blockIdx.x; item < ntiles * a.groups; item += gridDim.x) {
        const int64_t q0 = (item / a.groups) * EC_QT;
        const int64_t g = item % a.groups;
        const int64_t lo = g * R < v.n ? g * R : v.n;                          // ranges past the end of the pool are empty
        const int64_t hi = lo + R < v.n ? lo + R : v.n;
        int64_t bef[EC_QT];
#pragma unroll
        for (int t = 0; t < EC_QT; ++t) {
            const int64_t q = q0 + t < a.Q ? q0 + t : a.Q - 1;                 // wave-uniform: scalar loads
            const int64_t b = a.before != nullptr ? a.before[q] : v.n;
            bef[t] = b < 0 ? 0 : (b > v.n ? v.n : b);
        }
        // the tile's query ids are staged once per item: the row loop reads them from LDS (one address per wave: a broadcast)
        __syncthreads();                               // field_s is written; the previous item has read qid_s
        if (tid < n_exact * EC_QT) {
            const int e = tid / EC_QT, t = tid % EC_QT;
            const int64_t q = q0 + t < a.Q ? q0 + t : a.Q - 1;
            int col = a.cols[field_s[e]];
            col = col < 0 ? 0 : (col >= a.row_stride ? a.row_stride - 1 : col);
            qid_s[e][t] = a.ids[q * a.row_stride + col];
        }
        __syncthreads();
        int count[EC_QT];
#pragma unroll
        for (int t = 0; t < EC_QT; ++t) count[t] = 0;
        for (int64_t i = lo + tid; i < hi; i += EC_THREADS) {
            const int64_t slot = ring_wrap(v.head + i, a.capacity);
            uint32_t equal = (1u << EC_QT) - 1u;
            for (int e = 0; e < n_exact; ++e) {
                const int32_t id = a.db_t[(int64_t)field_s[e] * a.capacity + slot];
#pragma unroll
                for (int t = 0; t < EC_QT; ++t) equal &= ~((uint32_t)(qid_s[e][t] != id) << t);
            }
#pragma unroll
            for (int t = 0; t < EC_QT; ++t) count[t] += (((equal >> t) & 1u) != 0 && i < bef[t]) ? 1 : 0;
        }
#pragma unroll
        for (int t = 0; t < EC_QT; ++t) {
            int c = count[t];
            for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
            if (lane == 0) wave_sum[wave][t] = c;
        }
        __syncthreads();
        if (tid < EC_QT && q0 + tid < a.Q) {
            int64_t sum = 0;
            for (int w = 0; w < EC_WAVES; ++w) sum += wave_sum[w][tid];
            a.ws[(q0 + tid) * a.groups + g] = sum;
        }
        __syncthreads();                               // the next item reuses wave_sum
    }
}

__global__ void __launch_bounds__(256) bm25_exact_sum_kernel(const int64_t* ws, int64_t* counts, int64_t Q, int groups) {
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < Q; q += (int64_t)gridDim.x * 256) {
        int64_t sum = 0;
        for (int g = 0; g < groups; ++g) sum += ws[q * groups + g];
        counts[q] = sum;
    }
}

// one work-group: the first query with a candidate (Q when there is none) and the largest count, a minimum and a maximum through LDS.
// The counts are only compared — whatever they hold, first_row stays inside [0, Q) and the flag is 0 or 1.
__global__ void __launch_bounds__(256) bm25_exact_plan_kernel(const int64_t* counts, int64_t* first_row, int32_t* listing, int64_t Q,
                                                              int K) {
    __shared__ int64_t first_s[256];
    __shared__ int64_t most_s[256];
    const int tid = threadIdx.x;
    int64_t first = Q, most = 0;
    for (int64_t q = tid; q < Q; q += 256) {
        const int64_t c = counts[q];
        if (c > 0 && q < first) first = q;
        most = c > most ? c : most;
    }
    first_s[tid] = first;
    most_s[tid] = most;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if (tid < step) {
            first_s[tid] = first_s[tid + step] < first_s[tid] ? first_s[tid + step] : first_s[tid];
            most_s[tid] = most_s[tid + step] > most_s[tid] ? most_s[tid + step] : most_s[tid];
        }
        __syncthreads();
    }
    first = first_s[0] < Q ? first_s[0] : 0;
    for (int64_t q = tid; q < Q; q += 256) first_row[q] = first;
    if (tid == 0) listing[0] = most_s[0] <= K ? 1 : 0;
}

int64_t auto_count_groups(int64_t n_qry, int64_t capacity) {
    const int64_t tiles = (n_qry + EC_QT - 1) / EC_QT;
    int64_t g = (EC_TARGET_GROUPS + tiles - 1) / tiles;
    const int64_t by_rows = capacity / EC_MIN_RANGE_ROWS;
    if (g > by_rows) g = by_rows;
    if (g > RAT_BM25_EXACT_AUTO_GROUPS) g = RAT_BM25_EXACT_AUTO_GROUPS;
    return g < 1 ? 1 : g;
}

// the exact columns as one bit per used column: at least one, none past the used columns, and a column left to score
bool exact_mask_ok(uint32_t mask, int n_fields) {
    const uint32_t all = n_fields >= 32 ? ~0u : ((1u << n_fields) - 1u);
    return mask != 0 && (mask & ~all) == 0 && mask != all;
}

}  // namespace

extern "C" int rat_bm25_exact_count(const int32_t* db_ids_field_major, int pool_form, const int64_t* header_dev, int64_t n_rows,
                                    int64_t capacity, const int32_t* ids, const int32_t* cols, uint32_t exact_mask,
                                    const int64_t* before_dev, int64_t* out_counts, void* workspace, size_t workspace_bytes,
                                    int64_t n_qry, int row_stride, int n_fields, int groups, void* stream) {
    RAT_REQUIRE(db_ids_field_major && ids && cols && out_counts && workspace, "null pointer");
    RAT_POOL_FORM_CHECK(pool_form, header_dev, n_rows, capacity, capacity > 0 && n_qry > 0 && n_fields > 0 && row_stride > 0);
    RAT_REQUIRE(n_fields <= ON_FMAX, "more than 32 retrieval columns are not supported");
    RAT_REQUIRE(exact_mask_ok(exact_mask, n_fields), "exact_mask must name at least one used column and leave at least one to score");
    RAT_REQUIRE(groups >= 0 && groups <= EC_MAX_GROUPS, "groups must be 0 (library's choice) or 1..4096");
    if (groups == 0) groups = (int)auto_count_groups(n_qry, capacity);         // from the capacity: a captured launch keeps its shape
    RAT_REQUIRE((capacity + groups - 1) / groups <= INT32_MAX, "more than 2^31 - 1 rows per range: pass more groups");
    RAT_REQUIRE(workspace_bytes / sizeof(int64_t) / (size_t)n_qry >= (size_t)groups, "workspace smaller than 8 n_qry groups bytes");
    RAT_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
    ExactCountArgs a{db_ids_field_major, ids, cols, header_dev, before_dev, static_cast<int64_t*>(workspace), out_counts, n_rows,
                     capacity, n_qry, row_stride, n_fields, groups, exact_mask};
    const int64_t items = (n_qry + EC_QT - 1) / EC_QT * groups;
    const unsigned grid = (unsigned)(items < 65536 ? items : 65536);
    dispatch_pool(pool_form, [&](auto form) { RAT_LAUNCH(bm25_exact_count_kernel<decltype(form)::value>, grid, EC_THREADS, 0, stream, a); });
    if (rat_check_launch("rat_bm25_exact_count") != 0) return -1;
    const int64_t blocks = (n_qry + 255) / 256;
    RAT_LAUNCH(bm25_exact_sum_kernel, (unsigned)(blocks < 4096 ? blocks : 4096), 256, 0, stream, a.ws, out_counts, n_qry, groups);
    return rat_check_launch("rat_bm25_exact_count");
}

extern "C" int rat_bm25_exact_plan(const int64_t* counts, int64_t* first_row, int32_t* listing_dev, int64_t n_qry, int topk,
                                   void* stream) {
    RAT_REQUIRE(counts && first_row && listing_dev, "null pointer");
    RAT_REQUIRE(n_qry > 0 && topk > 0, "bad dims");
    RAT_LAUNCH(bm25_exact_plan_kernel, 1u, 256, 0, stream, counts, first_row, listing_dev, n_qry, topk);
    return rat_check_launch("rat_bm25_exact_plan");
}

extern "C" int rat_bm25_topk_split_exact(const int32_t* db_ids_field_major, int pool_form, const int64_t* header_dev, int64_t n_rows,
                                         int64_t capacity, const int32_t* qry_ids, const double* qry_idf, uint32_t exact_mask,
                                         const int64_t* before_dev, const int32_t* listing_dev, double* out_values,
                                         int64_t* out_indices, int64_t* out_lens, void* workspace, size_t workspace_bytes,
                                         int64_t n_qry, int n_fields, int topk, int splits, void* stream) {
    RAT_REQUIRE(db_ids_field_major && qry_ids && qry_idf && listing_dev && out_values && out_indices && out_lens, "null pointer");
    RAT_POOL_FORM_CHECK(pool_form, header_dev, n_rows, capacity, capacity > 0 && n_qry > 0 && n_fields > 0 && topk > 0);
    RAT_REQUIRE(n_fields <= ON_FMAX, "more than 32 retrieval columns are not supported");
    RAT_REQUIRE(topk <= ON_KMAX, "topK > 32 is not supported");
    RAT_REQUIRE(exact_mask_ok(exact_mask, n_fields), "exact_mask must name at least one used column and leave at least one to score");
    RAT_REQUIRE(splits >= 0 && splits <= ON_MAX_SPLITS, "splits must be 0 (library's choice) or 1..4096");
    if (splits == 0) splits = (int)auto_splits(n_qry, capacity, topk);        // from the capacity, as rat_bm25_topk_split_before
    return dispatch_pool(pool_form, [&](auto form) {                          // the count or the header, as rat_bm25_topk_split_before
        constexpr int POOL = decltype(form)::value;
        return launch_split<POOL, true, true>("rat_bm25_topk_split_exact", db_ids_field_major, qry_ids, qry_idf, out_values, out_indices,
                                              out_lens, workspace, workspace_bytes, POOL == POOL_HOST ? n_rows : 0,
                                              POOL == POOL_HOST ? nullptr : header_dev, capacity, n_qry, n_fields, topk, splits, stream,
                                              before_dev, exact_mask, listing_dev);
    });
}
