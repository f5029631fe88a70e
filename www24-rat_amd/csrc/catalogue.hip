// catalogue.hip — a request against a device-resident item catalogue: candidates as indices, and the best n of ALL of it.
//
// topn.hip ends a request whose candidates the caller spelled out as [C][W] id tuples.  Here the tuples live on the device once —
// cat int32 [M][W], item i's ids of the columns `cols` — and a candidate is an index into them.  Three kernels, on both sides of the
// unchanged request chain (rat_amd/online.py: top_items, rank_items, top_catalogue):
//
//   rat_catalogue_expand    out[b][l] = cat[i(b)][w] where l == cols[w], otherwise ctx[f(b)][l]: rat_candidates_expand (the same kernel,
//                           order_common.h's expand_kernel) with the candidate's columns read from the catalogue.  i(b) = items[b] (a list of indices), or — items == NULL,
//                           the SWEEP form — item0 + (b - f(b)): the k-th row of a request is catalogue item item0 + k.
//   rat_topn_exclude        out_y[b] = -inf where the catalogue item of row b (sweep form) is in its request's exclusion list — an
//                           ascending int32 list per request, searched by lower bound —, otherwise y[b], the same bits.
//   rat_topn_merge          a chunk's page (rat_topn_seg's outputs at the requests' head rows, position -> item0 + position) merged
//                           into the running page of every request, in place: rat_topn_seg's total order over (value, catalogue
//                           index).  A sweep visits the items in ascending order, so a running entry comes before a chunk entry of
//                           equal value; inside each page the entries already stand in that order.  Every entry gets
//                               order_key(value) (order_common.h's, as rat_topn_seg ranked by it: NaN lowest, -0.0 == +0.0) + 1, 0 for an empty slot
//                           and its place is the number of entries that come before it: 2 x 64 comparisons per lane out of LDS, ONE
//                           wave per request.  Chunk entries whose item is excluded are dropped first (looked up, not judged by value).
//                           Values are moved, never computed with.
//
// f(b) = clamp(first_row[b], 0, B - 1) as in topn.hip.  For ANY content of first_row, items, cols, the offsets, the lists, the pages and
// their lengths every address lies inside the buffers: a row, an item, a head, a length and an offset are clamped before they index
// anything, item0 is clamped to [-2^31, 2^32] (which changes no clamped item: |b - f(b)| < 2^31) so that no sum overflows, and the places
// of a merge are a permutation of 0 .. entries - 1 whatever the pages hold (ties fall to the page, then to the slot).
// No atomics, no communication between work-groups, nothing allocated or read back; every output element is written by every launch.
#include "order_common.h"

namespace {

constexpr int CT_WAVE = 64;                // rat_topn_merge: one wave per request, RAT_MAX_TOPN slots per page
static_assert(RAT_MAX_TOPN <= CT_WAVE, "a lane holds one slot of each page");

// is `item` in list[lo, hi)?  The list is ascending: lower bound, then one comparison.  lo <= hi inside the list, so every probe is;
// an unsorted list gives a wrong answer, never a wrong address
__device__ __forceinline__ bool listed(const int32_t* list, int64_t lo, int64_t hi, int64_t item) {
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)list[mid] < item)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < end && (int64_t)list[lo] == item;
}

// request r's list inside ex_items [E]: offsets clamped to [0, E] and to each other
__device__ __forceinline__ void list_of(const int64_t* ex_offsets, int64_t r, int64_t E, int64_t& lo, int64_t& hi) {
    lo = clamp_to(ex_offsets[r], 0, E);
    hi = clamp_to(ex_offsets[r + 1], lo, E);
}

struct CatExpandArgs {
    const int32_t* ctx;          // [B][L], head rows only are read
    const int32_t* cat;          // [M][W]
    const int32_t* items;        // [B] or nullptr: the sweep form
    const int32_t* cols;         // [W]
    const int64_t* first_row;    // [B], any content
    int32_t* out;                // [B][L]
    int64_t item0, B, M;
    int L, W;
    // expand_kernel's (order_common.h) source of a candidate's own columns: the catalogue row of item i(b)
    __device__ const int32_t* row(int64_t b, int64_t h) const {
        return cat + clamp_to(items != nullptr ? (int64_t)items[b] : item0 + (b - h), 0, M - 1) * W;
    }
};

struct ExcludeArgs {
    const float* y;              // [B]
    const int64_t* first_row;    // [B], any content
    const int32_t* ex_items;     // [E], per request ascending
    const int64_t* ex_offsets;   // [R + 1], any content
    float* out_y;                // [B]
    int64_t item0, rows_per_request, E, R, B;
};

__global__ void __launch_bounds__(256) topn_exclude_kernel(ExcludeArgs a) {
    for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < a.B; b += (int64_t)gridDim.x * 256) {
        const int64_t h = clamp_row(a.first_row[b], a.B);
        int64_t lo, hi;
        list_of(a.ex_offsets, clamp_to(h / a.rows_per_request, 0, a.R - 1), a.E, lo, hi);
        const uint32_t bits = listed(a.ex_items, lo, hi, a.item0 + (b - h)) ? 0xff800000u : rat_fbits(a.y[b]);
        a.out_y[b] = rat_bitsf(bits);
    }
}

struct MergeArgs {
    int32_t* run_item;           // [R][n]
    float* run_val;              // [R][n]
    int32_t* run_len;            // [R]
    const int32_t* pos;          // [B][n]   rat_topn_seg's outputs: read at the rows heads[r]
    const float* val;            // [B][n]
    const int32_t* len;          // [B]
    const int64_t* heads;        // [R], any content
    const int32_t* ex_items;     // [E] or nullptr: nothing is excluded
    const int64_t* ex_offsets;   // [R + 1], any content
    int64_t item0, E, R, B;
    int n;
};

__global__ void __launch_bounds__(CT_WAVE) topn_merge_kernel(MergeArgs a) {
    __shared__ uint32_t keys[2][CT_WAVE];                                     // [0]: the running page, [1]: the chunk's; 0 = empty slot
    const int t = threadIdx.x, n = a.n;
    const int64_t r = blockIdx.x;
    const int64_t h = clamp_row(a.heads[r], a.B);
    const int rl = (int)clamp_to(a.run_len[r], 0, n), cl = (int)clamp_to(a.len[h], 0, n);
    int32_t item[2] = {-1, -1};
    float value[2] = {0.0f, 0.0f};
    bool live[2] = {t < rl, t < cl};
    if (live[0]) {
        item[0] = a.run_item[r * n + t];
        value[0] = a.run_val[r * n + t];
    }
    if (live[1]) {
        const int64_t it = a.item0 + (int64_t)a.pos[h * n + t];
        item[1] = (int32_t)it;
        value[1] = a.val[h * n + t];
        if (a.ex_items != nullptr) {
            int64_t lo, hi;
            list_of(a.ex_offsets, r, a.E, lo, hi);
            live[1] = !listed(a.ex_items, lo, hi, it);
        }
    }
    keys[0][t] = live[0] ? order_key(value[0]) + 1u : 0u;
    keys[1][t] = live[1] ? order_key(value[1]) + 1u : 0u;
    __syncthreads();                                                          // every slot of both pages is in registers: the running page may be rewritten

    // an entry's place: the entries before it.  Larger key first; equal keys: the running page first, then the lower slot
    const uint32_t k0 = keys[0][t], k1 = keys[1][t];
    int place0 = 0, place1 = 0, kept = 0;
    for (int j = 0; j < CT_WAVE; ++j) {
        const uint32_t q0 = keys[0][j], q1 = keys[1][j];
        place0 += (q0 > k0 || (q0 == k0 && j < t)) + (q1 > k0);
        place1 += (q0 >= k1) + (q1 > k1 || (q1 == k1 && j < t));
        kept += (q0 != 0u) + (q1 != 0u);
    }
    if (live[0] && place0 < n) {
        a.run_item[r * n + place0] = item[0];
        a.run_val[r * n + place0] = value[0];
    }
    if (live[1] && place1 < n) {
        a.run_item[r * n + place1] = item[1];
        a.run_val[r * n + place1] = value[1];
    }
    const int cnt = kept < n ? kept : n;
    if (t >= cnt && t < n) {
        a.run_item[r * n + t] = -1;
        a.run_val[r * n + t] = 0.0f;
    }
    if (t == 0) a.run_len[r] = cnt;
}

// |b - f(b)| < 2^31 and a position is an int32: behind this clamp no item0 + k overflows, and no item clamped to [0, M) changes
int64_t item0_arg(int64_t item0) { return item0 < -0x80000000LL ? -0x80000000LL : (item0 > 0x100000000LL ? 0x100000000LL : item0); }

}  // namespace

extern "C" int rat_catalogue_expand(const int32_t* ctx, const int32_t* cat, const int32_t* items, int64_t item0, const int32_t* cols,
                                    const int64_t* first_row, int64_t B, int L, int W, int64_t M, int32_t* out, void* stream) {
    RAT_REQUIRE(ctx && cat && cols && first_row && out, "null pointer");
    RAT_REQUIRE(B >= 1 && B <= 0x7fffffffLL, "B must be in [1, 2^31 - 1]");
    RAT_REQUIRE(L >= 1 && L <= EXPAND_MAX_L, "L must be in [1, 8192]");
    RAT_REQUIRE(W >= 1 && W <= EXPAND_MAX_L, "W must be in [1, 8192]");
    RAT_REQUIRE(M >= 1 && M <= 0x7fffffffLL, "M must be in [1, 2^31 - 1]");
    CatExpandArgs a{ctx, cat, items, cols, first_row, out, item0_arg(item0), B, M, L, W};
    expand_launch(a, stream);
    return rat_check_launch("rat_catalogue_expand");
}

extern "C" int rat_topn_exclude(const float* y, const int64_t* first_row, int64_t item0, int64_t rows_per_request, const int32_t* ex_items,
                                const int64_t* ex_offsets, int64_t E, int64_t R, int64_t B, float* out_y, void* stream) {
    RAT_REQUIRE(y && first_row && ex_offsets && out_y && (ex_items || E == 0), "null pointer");
    RAT_REQUIRE(B >= 1 && B <= 0x7fffffffLL, "B must be in [1, 2^31 - 1]");
    RAT_REQUIRE(R >= 1 && R <= 0x7fffffffLL, "R must be in [1, 2^31 - 1]");
    RAT_REQUIRE(E >= 0, "E must be >= 0");
    RAT_REQUIRE(rows_per_request >= 1, "rows_per_request must be >= 1");
    ExcludeArgs a{y, first_row, ex_items, ex_offsets, out_y, item0_arg(item0), rows_per_request, E, R, B};
    const int64_t blocks = (B + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 4096 ? blocks : 4096);
    RAT_LAUNCH(topn_exclude_kernel, grid, 256, 0, stream, a);
    return rat_check_launch("rat_topn_exclude");
}

extern "C" int rat_topn_merge(int32_t* run_item, float* run_val, int32_t* run_len, const int32_t* pos, const float* val, const int32_t* len,
                              const int64_t* heads, int64_t item0, const int32_t* ex_items, const int64_t* ex_offsets, int64_t E,
                              int64_t R, int64_t B, int n, void* stream) {
    RAT_REQUIRE(run_item && run_val && run_len && pos && val && len && heads, "null pointer");
    RAT_REQUIRE((ex_items == nullptr || ex_offsets != nullptr) && (ex_items != nullptr || ex_offsets == nullptr || E == 0),
                "null pointer (ex_items and ex_offsets come together)");
    RAT_REQUIRE(B >= 1 && B <= 0x7fffffffLL, "B must be in [1, 2^31 - 1]");
    RAT_REQUIRE(R >= 1 && R <= 0x7fffffffLL, "R must be in [1, 2^31 - 1]");
    RAT_REQUIRE(E >= 0, "E must be >= 0");
    RAT_REQUIRE(n >= 1 && n <= RAT_MAX_TOPN, "n must be in [1, RAT_MAX_TOPN]");
    MergeArgs a{run_item, run_val, run_len, pos, val, len, heads, ex_items, ex_offsets, item0_arg(item0), E, R, B, n};
    RAT_LAUNCH(topn_merge_kernel, (unsigned)R, CT_WAVE, 0, stream, a);
    return rat_check_launch("rat_topn_merge");
}
