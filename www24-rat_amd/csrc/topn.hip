// topn.hip — the end of a request: each request's n best candidates, and the candidates' rows built from one context row, on the device.
//
// A CTR request is one user with a slate of candidate items.  The request chain (online.hip, rat_amd/online.py) leaves y_pred [B] on
// the device with first_row [B] — for every row the row that opens its request; two kernels spare the caller the host work on both
// sides of that chain:
//
//   rat_candidates_expand   out[b][l] = cand[b][w] where l == cols[w], otherwise ctx[f(b)][l]: the full rows of every candidate from
//                           ONE context row per request (held at the request's head row) and the candidates' own columns.  One
//                           launch (order_common.h's expand_kernel); the inverse of `cols` is built in LDS by every work-group, rows move as 16-byte words when the
//                           row width and the buffers allow.
//   rat_topn_seg            per request the positions (inside the request) and values of its n largest predictions, in the order
//                           np.argsort(-y_seg, kind="stable")[:n]: value descending, equal values (-0.0 and +0.0 tie) by ascending
//                           position, NaN after every number.  Every candidate gets the 64-bit key
//                               (order_common.h's order_key of y, NaN -> 0) << 32  |  0xFFFFFFFF - position
//                           — unique inside a segment — and round k takes the largest key below the key of round k - 1: n rounds of
//                           a work-group arg-max.  No floating-point arithmetic touches y, so out_val carries y's bits.
//
// f(b) = clamp(first_row[b], 0, B - 1) in both.  Row h is a head iff f(h) == h; its segment runs up to the first j > h with
// f(j) != h (or B).  For valid first_row the segments are the requests; for ANY first_row every address derived from it lies inside the
// buffers: a row index is clamped before it is used, a segment never leaves [h, B), and a position comes out of a key that was built
// from a row of the segment.
//
// A work-group owns TN_ROWS consecutive batch rows: it writes the padding of those that are no heads and ranks the segments of those
// that are, one after the other (a head's segment may reach far beyond the group's rows: it is read, never written).  The keys of a
// segment's first TN_STAGE rows are staged in LDS while its end is searched; rows beyond are re-read from y in every round.
// No atomics, no communication between work-groups, nothing allocated or read back: both kernels are captured into the serving graph.
#include "order_common.h"

namespace {

constexpr int TN_THREADS = 256;
constexpr int TN_WAVES = TN_THREADS / 64;
constexpr int TN_ROWS = 16;                // batch rows per work-group
constexpr int TN_STAGE = 1024;             // rows of a segment whose keys are kept in LDS

// the largest of the work-group's 256 keys, to every thread: shuffles inside a wave (two 32-bit halves), then one LDS word per wave
// and ONE barrier.  `turn` counts the calls of this thread (the same for all threads): the slots are double-buffered by its parity,
// a slot is rewritten two calls later, i.e. behind the barrier of the call in between, which every thread passes after its reads.
__device__ __forceinline__ uint64_t block_max(uint64_t key, uint64_t (*slots)[TN_WAVES], unsigned& turn) {
    uint32_t hi = (uint32_t)(key >> 32), lo = (uint32_t)key;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t ohi = __shfl_xor(hi, m, 64), olo = __shfl_xor(lo, m, 64);
        const bool take = ohi > hi || (ohi == hi && olo > lo);
        hi = take ? ohi : hi;
        lo = take ? olo : lo;
    }
    uint64_t* s = slots[turn++ & 1u];
    if (rat_lane() == 0) s[threadIdx.x >> 6] = ((uint64_t)hi << 32) | lo;
    __syncthreads();
    uint64_t best = s[0];
#pragma unroll
    for (int w = 1; w < TN_WAVES; ++w) best = s[w] > best ? s[w] : best;
    return best;
}

struct TopnArgs {
    const float* y;              // [B]
    const int64_t* first_row;    // [B], any content
    int32_t* out_pos;            // [B][n]
    float* out_val;              // [B][n]
    int32_t* out_len;            // [B]
    int64_t B;
    int n;
};

__global__ void __launch_bounds__(TN_THREADS) topn_seg_kernel(TopnArgs a) {
    __shared__ uint32_t keys[TN_STAGE];
    __shared__ uint64_t slots[2][TN_WAVES];
    unsigned turn = 0;
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * TN_ROWS;
    const int rows = (int)(a.B - row0 < TN_ROWS ? a.B - row0 : TN_ROWS);

    // rows that open no request: length 0 and a row of padding
    for (int e = t; e < rows * a.n; e += TN_THREADS) {
        const int64_t b = row0 + e / a.n;
        if (clamp_row(a.first_row[b], a.B) != b) {
            a.out_pos[b * a.n + e % a.n] = -1;
            a.out_val[b * a.n + e % a.n] = 0.0f;
        }
    }
    if (t < rows && clamp_row(a.first_row[row0 + t], a.B) != row0 + t) a.out_len[row0 + t] = 0;

    for (int r = 0; r < rows; ++r) {
        const int64_t h = row0 + r;
        if (clamp_row(a.first_row[h], a.B) != h) continue;                     // (the same for every thread of the work-group)

        // the segment's end, 256 rows at a time: the smallest position i whose row is past B or belongs to another request — and,
        // on the way, the keys of the first TN_STAGE rows into LDS (rows behind the end are staged too and never looked at)
        int64_t len = 0;
        for (int64_t base = 0;; base += TN_THREADS) {
            const int64_t i = base + t, j = h + i;
            const bool inside = j < a.B && (i == 0 || clamp_row(a.first_row[j], a.B) == h);
            if (j < a.B && i < TN_STAGE) keys[i] = order_key(a.y[j]);
            const uint64_t end = block_max(inside ? 0ull : ~0ull - (uint64_t)i, slots, turn);
            if (end != 0ull) {
                len = (int64_t)(~0ull - end);
                break;
            }
        }

        // round k: the largest key below the one round k - 1 took.  0 is no key (a position is below 2^31), ~0 is above every key
        // (the largest order_key is +inf's, 0xFF800000)
        const int cnt = (int)(len < a.n ? len : a.n);
        uint64_t last = ~0ull;
        for (int k = 0; k < cnt; ++k) {
            uint64_t best = 0ull;
            for (int64_t i = t; i < len; i += TN_THREADS) {
                const uint32_t o = i < TN_STAGE ? keys[i] : order_key(a.y[h + i]);
                const uint64_t key = ((uint64_t)o << 32) | (0xFFFFFFFFu - (uint32_t)i);
                if (key < last && key > best) best = key;
            }
            last = block_max(best, slots, turn);
            if (t == 0) {
                const uint32_t pos = 0xFFFFFFFFu - (uint32_t)last;
                a.out_pos[h * a.n + k] = (int32_t)pos;
                a.out_val[h * a.n + k] = a.y[h + pos];
            }
        }
        for (int k = cnt + t; k < a.n; k += TN_THREADS) {
            a.out_pos[h * a.n + k] = -1;
            a.out_val[h * a.n + k] = 0.0f;
        }
        if (t == 0) a.out_len[h] = cnt;
    }
}

struct ExpandArgs {
    const int32_t* ctx;          // [B][L], head rows only are read
    const int32_t* cand;         // [B][W]
    const int32_t* cols;         // [W]
    const int64_t* first_row;    // [B], any content
    int32_t* out;                // [B][L]
    int64_t B;
    int L, W;
    // expand_kernel's (order_common.h) source of a candidate's own columns: the caller's tuple of row b
    __device__ const int32_t* row(int64_t b, int64_t) const { return cand + b * W; }
};

}  // namespace

extern "C" int rat_topn_seg(const float* y, const int64_t* first_row, int64_t B, int n, int32_t* out_pos, float* out_val,
                            int32_t* out_len, void* stream) {
    RAT_REQUIRE(y && first_row && out_pos && out_val && out_len, "null pointer");
    RAT_REQUIRE(B >= 1 && B <= 0x7fffffffLL, "B must be in [1, 2^31 - 1]");
    RAT_REQUIRE(n >= 1 && n <= RAT_MAX_TOPN, "n must be in [1, RAT_MAX_TOPN]");
    TopnArgs a{y, first_row, out_pos, out_val, out_len, B, n};
    const unsigned grid = (unsigned)((B + TN_ROWS - 1) / TN_ROWS);
    RAT_LAUNCH(topn_seg_kernel, grid, TN_THREADS, 0, stream, a);
    return rat_check_launch("rat_topn_seg");
}

extern "C" int rat_candidates_expand(const int32_t* ctx, const int32_t* cand, const int32_t* cols, const int64_t* first_row, int64_t B,
                                     int L, int W, int32_t* out, void* stream) {
    RAT_REQUIRE(ctx && cand && cols && first_row && out, "null pointer");
    RAT_REQUIRE(B >= 1 && B <= 0x7fffffffLL, "B must be in [1, 2^31 - 1]");
    RAT_REQUIRE(L >= 1 && L <= EXPAND_MAX_L, "L must be in [1, 8192]");
    RAT_REQUIRE(W >= 1 && W <= EXPAND_MAX_L, "W must be in [1, 8192]");
    ExpandArgs a{ctx, cand, cols, first_row, out, B, L, W};
    expand_launch(a, stream);
    return rat_check_launch("rat_candidates_expand");
}
