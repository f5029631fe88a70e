// postings.hip — candidate retrieval through posting lists, for requests whose rows share a context (rat_bm25_topk_postings).
//
// The rows of one request are the same context row with the columns V (vary_mask) swapped.  With the weights of V set to 0.0 a pool row
// scores a(n), the same for every row of the request; T = the K best of a() over the indexed rows is ONE ordinary scan per request
// (the caller's, rat_bm25_topk_split_before with before = n_sorted).  A pool row that equals query b in no column of V scores
// full(n) == a(n) bit for bit (+0.0 is exact), any other row full(n) >= a(n) (weights >= 0, rounding is monotone).  So the K best of b
// over the whole pool are the K best of three sets of rows, each scored in full from db_t:
//     1. the rows in the posting lists of b's ids in the columns of V     (post_ids / post_rows: per used column the indexed rows
//                                                                          [0, n_sorted) sorted by (id, row); a list is the range
//                                                                          between a lower and an upper bound)
//     2. the rows of T                                                     (ctx_indices [n_ctx][K], -1 padded; row b's list: ctx_row[b])
//     3. the tail rows [n_sorted, n) appended since the index was built.
// A row is offered once: from the list of the FIRST column of V in which it equals b, from T only when it equals b in no column of V,
// and the tail is disjoint from both (the lists and T hold rows below n_sorted only: anything else in them is skipped).
//
// One wave per query, four queries per work-group.  Lanes stride over the stream; each keeps a private list sorted under the full
// total order (score descending, index ascending: bm25_scan.h's better()).  The stream is NOT ascending in the index, so
// RAT_BM25_LIST_INSERT — right only for rows arriving in ascending order — is not used: list_offer below compares indices too.  The
// wave then takes the best of the 64 heads K times, as the split scan's per-wave merge does (wave_head: the same two-level arg-max
// through a wave-private LDS tile; online.hip keeps its own in its unnamed namespace).
//
// Scores are the scans': fp64, (db == q) ? idf : 0.0 added with f ascending over all n_fields; a row with score > 0 is a candidate.
// For ANY content of the header, n_sorted, post_rows, ctx_indices and ctx_row every address lies inside the buffers: the counts are
// clamped (n to [0, capacity], n_sorted to [0, n], ctx_row to [0, n_ctx)), a posting or context row outside [0, n_sorted) is skipped
// before it addresses db_t, and the binary searches stay inside [0, n_sorted).  Corrupt input gives a wrong answer, never a wrong address.
// No atomics, no communication between work-groups, nothing allocated or read back: one capturable launch.
#include "bm25_scan.h"
#include "pool_common.h"

namespace {

constexpr int PL_THREADS = 256;
constexpr int PL_WAVES = PL_THREADS / 64;
constexpr int PL_FMAX = 32;
constexpr int PL_KMAX = 32;

struct PostArgs {
    const int32_t* db_t;         // [F][capacity]
    const int64_t* header;       // POOL_DEV: {n}
    const int32_t* post_ids;     // [F][capacity]
    const int32_t* post_rows;    // [F][capacity]
    const int64_t* n_sorted;     // one word, any content
    const int32_t* qry;          // [Q][F]
    const double* idf;           // [Q][F]
    const int64_t* ctx_idx;      // [n_ctx][K], any content
    const int64_t* ctx_row;      // [Q], any content
    double* out_val;             // [Q][K]
    int64_t* out_idx;            // [Q][K]
    int64_t* out_len;            // [Q]
    int64_t N, capacity, n_ctx, Q;
    uint32_t vary_mask;
    int F, K;
};

// the heads of the 64 lists of one wave -> the best of them, in every lane: 64 heads -> 8 group bests -> 1 through the wave's tile,
// double-buffered by the call's parity (two wave fences a call, no work-group barrier)
struct HeadTile {
    double hv[2][64];
    int64_t hi[2][64];
    double gv[2][8];
    int64_t gi[2][8];
};

__device__ __forceinline__ void wave_head(HeadTile& w, int parity, double& s, int64_t& i) {
    const int lane = rat_lane();
    w.hv[parity][lane] = s;
    w.hi[parity][lane] = i;
    RAT_WAVE_FENCE();
    const int g = lane & 7;
    double cs = 0.0;
    int64_t ci = -1;
#pragma unroll
    for (int j = 0; j < 8; ++j) take_better(w.hv[parity][8 * g + j], w.hi[parity][8 * g + j], cs, ci);
    if (lane < 8) {
        w.gv[parity][g] = cs;
        w.gi[parity][g] = ci;
    }
    RAT_WAVE_FENCE();
    cs = 0.0;
    ci = -1;
#pragma unroll
    for (int j = 0; j < 8; ++j) take_better(w.gv[parity][j], w.gi[parity][j], cs, ci);
    s = cs;
    i = ci;
}

// Row n with score s > 0 into a list of K entries sorted under better(): rows arrive in ANY order, so the comparison is the full
// total order at every slot (an empty slot, index -1, loses to everything).  (ks, ki) mirror the K-th entry, so that the common case —
// a full list and a row that does not beat it — costs one comparison and no walk.
template <int KMAX>
__device__ __forceinline__ void list_offer(double (&val)[KMAX], int32_t (&idx)[KMAX], double& ks, int32_t& ki, int K, double s, int32_t n) {
    if (ki >= 0 && !better(s, n, ks, ki)) return;
    double cs = s;
    int32_t ci = n;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < K && ci >= 0 && (idx[k] < 0 || better(cs, ci, val[k], idx[k]))) {
            const double ts = val[k];
            const int32_t ti = idx[k];
            val[k] = cs;
            idx[k] = ci;
            cs = ts;
            ci = ti;
        }
        if (k == K - 1) {
            ks = val[k];
            ki = idx[k];
        }
    }
}

__device__ __forceinline__ int64_t clamp_pos(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }      // to [0, hi]

// first position in ids[0, n) whose id is >= x (UPPER: > x); every probe lies inside [0, n)
template <bool UPPER>
__device__ __forceinline__ int64_t bound(const int32_t* ids, int64_t n, int32_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (UPPER ? ids[mid] <= x : ids[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

template <int KMAX, int POOL>
__global__ void __launch_bounds__(PL_THREADS) bm25_postings_kernel(PostArgs a) {
    __shared__ HeadTile tile_s[PL_WAVES];
    const int lane = rat_lane(), wave = rat_wave();
    const int64_t N = pool_view<POOL>(a.header, a.N, a.capacity).n;
    const int64_t ns = clamp_pos(a.n_sorted[0], N);
    const int F = a.F, K = a.K;
    int parity = 0;
    for (int64_t q = (int64_t)blockIdx.x * PL_WAVES + wave; q < a.Q; q += (int64_t)gridDim.x * PL_WAVES) {   // wave-uniform
        const int32_t* qid = a.qry + q * F;
        const double* w = a.idf + q * F;
        double val[KMAX], ks = 0.0;
        int32_t idx[KMAX], ki = -1;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            val[k] = 0.0;
            idx[k] = -1;
        }
        // row n (inside [0, N)) in full, f ascending as the scans add; it is offered unless it equals the query in a column of `skip`
        auto offer = [&](int64_t n, uint32_t skip) {
            double s = 0.0;
            uint32_t hit = 0;
            for (int f = 0; f < F; ++f) {
                const bool eq = a.db_t[(int64_t)f * a.capacity + n] == qid[f];
                s += eq ? w[f] : 0.0;
                hit |= (uint32_t)eq << f;
            }
            if ((hit & skip) == 0 && s > 0.0) list_offer<KMAX>(val, idx, ks, ki, K, s, (int32_t)n);
        };
        // 1. the posting lists of the query's ids in the varying columns, ascending; a row belongs to the first list that holds it
        uint32_t earlier = 0;
        for (int f = 0; f < F; ++f) {
            if (((a.vary_mask >> f) & 1u) == 0) continue;                                  // the same in every thread of the grid
            const int32_t* ids = a.post_ids + (int64_t)f * a.capacity;
            const int32_t* rows = a.post_rows + (int64_t)f * a.capacity;
            const int64_t lo = bound<false>(ids, ns, qid[f]), hi = bound<true>(ids, ns, qid[f]);
            for (int64_t p = lo + lane; p < hi; p += 64) {
                const int64_t n = rows[p];
                if (n >= 0 && n < ns) offer(n, earlier);
            }
            earlier |= 1u << f;
        }
        // 2. the request's context list: what equals the query in a varying column came (or, corrupt, could have come) from a list
        const int64_t c = clamp_pos(a.ctx_row[q], a.n_ctx - 1);
        for (int j = lane; j < K; j += 64) {
            const int64_t n = a.ctx_idx[c * K + j];
            if (n >= 0 && n < ns) offer(n, a.vary_mask);
        }
        // 3. the tail
        for (int64_t n = ns + lane; n < N; n += 64) offer(n, 0u);

        // ---- the best of the 64 heads, K times; the winner pops its head
        int k = 0;
        for (; k < K; ++k) {
            double hs = val[0];
            int64_t hx = idx[0];
            wave_head(tile_s[wave], parity, hs, hx);
            parity ^= 1;
            if (hx < 0) break;                             // every list is exhausted (the same in all lanes)
            if ((int64_t)idx[0] == hx) {
#pragma unroll
                for (int j = 0; j + 1 < KMAX; ++j) {
                    val[j] = val[j + 1];
                    idx[j] = idx[j + 1];
                }
                val[KMAX - 1] = 0.0;
                idx[KMAX - 1] = -1;
            }
            if (lane == 0) {
                a.out_val[q * K + k] = hs;
                a.out_idx[q * K + k] = hx;
            }
        }
        for (int j = k + lane; j < K; j += 64) {           // zero scores are dropped: index -1, value 0
            a.out_val[q * K + j] = 0.0;
            a.out_idx[q * K + j] = -1;
        }
        if (lane == 0) a.out_len[q] = k;
    }
}

}  // namespace

extern "C" int rat_bm25_topk_postings(const int32_t* db_ids_field_major, int pool_form, const int64_t* header_dev, int64_t n_rows,
                                      int64_t capacity, const int32_t* post_ids, const int32_t* post_rows, const int64_t* n_sorted_dev,
                                      const int32_t* qry_ids, const double* qry_idf, uint32_t vary_mask, const int64_t* ctx_indices,
                                      const int64_t* ctx_row, int64_t n_ctx, double* out_values, int64_t* out_indices,
                                      int64_t* out_lens, int64_t n_qry, int n_fields, int topk, void* stream) {
    RAT_REQUIRE(db_ids_field_major && post_ids && post_rows && n_sorted_dev && qry_ids && qry_idf && ctx_indices && ctx_row &&
                    out_values && out_indices && out_lens,
                "null pointer");
    RAT_POOL_FORM_CHECK(pool_form, header_dev, n_rows, capacity,
                        capacity > 0 && capacity <= 0x7fffffffLL && n_qry > 0 && n_ctx > 0 && n_fields > 0 && topk > 0);
    RAT_REQUIRE(pool_form != POOL_RING, "a sliding window is not served: its evictions and deletions renumber the rows of the lists");
    RAT_REQUIRE(n_fields <= PL_FMAX, "more than 32 retrieval columns are not supported");
    RAT_REQUIRE(topk <= PL_KMAX, "topK > 32 is not supported");
    PostArgs a{};
    a.db_t = db_ids_field_major;
    a.header = header_dev;
    a.post_ids = post_ids;
    a.post_rows = post_rows;
    a.n_sorted = n_sorted_dev;
    a.qry = qry_ids;
    a.idf = qry_idf;
    a.ctx_idx = ctx_indices;
    a.ctx_row = ctx_row;
    a.out_val = out_values;
    a.out_idx = out_indices;
    a.out_len = out_lens;
    a.N = n_rows;
    a.capacity = capacity;
    a.n_ctx = n_ctx;
    a.Q = n_qry;
    a.vary_mask = n_fields >= 32 ? vary_mask : (vary_mask & ((1u << n_fields) - 1u));      // bits past the used columns name nothing
    a.F = n_fields;
    a.K = topk;
    const int64_t groups = (n_qry + PL_WAVES - 1) / PL_WAVES;
    const unsigned grid = (unsigned)(groups < 65536 ? groups : 65536);
    if (pool_form == POOL_HOST) {
        if (topk <= 8)
            RAT_LAUNCH((bm25_postings_kernel<8, POOL_HOST>), grid, PL_THREADS, 0, stream, a);
        else
            RAT_LAUNCH((bm25_postings_kernel<32, POOL_HOST>), grid, PL_THREADS, 0, stream, a);
    } else {
        if (topk <= 8)
            RAT_LAUNCH((bm25_postings_kernel<8, POOL_DEV>), grid, PL_THREADS, 0, stream, a);
        else
            RAT_LAUNCH((bm25_postings_kernel<32, POOL_DEV>), grid, PL_THREADS, 0, stream, a);
    }
    return rat_check_launch("rat_bm25_topk_postings");
}
