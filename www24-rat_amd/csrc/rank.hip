// rank.hip — the end of a request, in full: every request's whole ranking on the device.
//
// rat_topn_seg (topn.hip) returns a page, n <= 64 candidates per request, in n rounds of a work-group arg-max.  A caller that needs the
// whole order — a re-ranker behind the model, rules that walk down the list, rank metrics — gets it here, from the same y_pred [B] and
// first_row [B] the request chain leaves on the device:
//
//   rat_rank_seg            per request the permutation np.argsort(-y_seg, kind="stable"), the values in that order and every row's
//                           place: rank by COUNTING.  One thread per row; the row's rank is the number of rows of its segment that come
//                           before it in topn.hip's total order — a before b iff y[a] > y[b], or neither compares greater and a < b:
//                           the rows with a larger 64-bit key
//                               (order_common.h's order_key of y, NaN -> 0, -0.0 -> +0.0's) << 32  |  0xFFFFFFFF - row
//                           — and the thread scatters its position and its value to that place.  No floating-point arithmetic touches
//                           y: out_val carries y's bits.
//
// f(b) = clamp(first_row[b], 0, B - 1), heads and segments as in topn.hip: row h is a head iff f(h) == h, its segment runs up to the
// first j > h with f(j) != h (or B), and row b is a MEMBER of segment h iff h <= b < that end.  Segments are disjoint, so every output
// element has exactly one writer: a member writes out_rank[b] and the slot h + rank of out_order / out_val (the ranks of a segment's
// members are a permutation of its positions), a row that is a member of nothing writes its own three entries of padding.  For ANY
// first_row every address lies inside the buffers: a row index is clamped before it is used, and h + rank < end <= B.
//
// A work-group owns RK_THREADS consecutive rows.  A thread whose row names a head at or before itself is a CANDIDATE; the work-group
// streams (key, f) of the rows from its lowest candidate head upwards through an LDS tile of RK_TILE rows, and every candidate walks
// its own segment in the tile — all lanes of a wave inside one segment read the same LDS word, a broadcast — counting and looking for
// the segment's end.  Heads are ordered as their segments are, so the segment of the HIGHEST candidate head ends last: the streaming
// stops at the first tile boundary at or behind that end, which every thread reads off first_row itself — no vote per tile.  A long
// segment is thereby spread over all the work-groups that hold its rows, with no communication between them, at O(segment length) LDS
// reads per row.  No atomics, nothing allocated or read back, one launch: captured into the serving graph.
#include "order_common.h"

namespace {

constexpr int RK_THREADS = 256;            // rows per work-group, one thread each
constexpr int RK_WAVES = RK_THREADS / 64;
constexpr int RK_TILE = 1024;              // rows whose (key, f) one LDS tile holds
constexpr int RK_STEP = 8;                 // tile entries a thread reads before it looks at them
constexpr uint32_t RK_NO_ROW = 0xFFFFFFFFu;   // f of a tile entry behind B (a row index is below 2^31): ends every segment

// topn.hip's 64-bit key with the ROW in the place of the position inside the segment (a row is below 2^31): unique, and inside a
// segment a before b iff key(a) > key(b) — larger value first, equal values by ascending row
__device__ __forceinline__ uint64_t row_key(float v, int64_t row) {
    return ((uint64_t)order_key(v) << 32) | (0xFFFFFFFFu - (uint32_t)row);
}

struct RankArgs {
    const float* y;              // [B]
    const int64_t* first_row;    // [B], any content
    int32_t* out_order;          // [B]
    float* out_val;              // [B]
    int32_t* out_rank;           // [B]
    int64_t B;
};

__global__ void __launch_bounds__(RK_THREADS) rank_seg_kernel(RankArgs a) {
    // entries RK_TILE .. RK_TILE + RK_STEP - 2 are never rows: a thread reads RK_STEP entries at a time from any start below RK_TILE
    __shared__ uint64_t keys[RK_TILE + RK_STEP - 1];
    __shared__ uint32_t owner[RK_TILE + RK_STEP - 1];
    __shared__ int32_t heads[2][RK_WAVES];
    const int t = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x * RK_THREADS + t;

    // the row's head, if it names one at or before itself
    int32_t h = -1;
    float v = 0.0f;
    if (b < a.B) {
        const int64_t f = clamp_row(a.first_row[b], a.B);
        if (f <= b && clamp_row(a.first_row[f], a.B) == f) h = (int32_t)f;
        v = a.y[b];
    }
    const uint64_t mine = row_key(v, b);

    // the lowest and the highest candidate head of the work-group, to every thread: shuffles, one LDS word per wave, one barrier
    int32_t lo = h < 0 ? 0x7fffffff : h, hi = h;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int32_t olo = __shfl_xor(lo, m, 64), ohi = __shfl_xor(hi, m, 64);
        lo = olo < lo ? olo : lo;
        hi = ohi > hi ? ohi : hi;
    }
    if (rat_lane() == 0) {
        heads[0][t >> 6] = lo;
        heads[1][t >> 6] = hi;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < RK_WAVES; ++w) {
        lo = heads[0][w] < lo ? heads[0][w] : lo;
        hi = heads[1][w] > hi ? heads[1][w] : hi;
    }

    int32_t rank = 0;
    int64_t end = -1;                                                          // the end of the thread's segment, once it is seen
    if (hi >= 0) {                                                             // (the same for every thread of the work-group)
        for (int64_t base = lo;; base += RK_TILE) {
            for (int i = t; i < RK_TILE + RK_STEP - 1; i += RK_THREADS) {
                const int64_t j = base + i;
                const bool row = i < RK_TILE && j < a.B;
                keys[i] = row ? row_key(a.y[j], j) : 0ull;
                owner[i] = row ? (uint32_t)clamp_row(a.first_row[j], a.B) : RK_NO_ROW;
            }
            __syncthreads();
            if (h >= 0 && end < 0 && h < base + RK_TILE) {
                // walk the segment from its head (or from the tile's first row): `at` stops at the first entry of another segment, and
                // an entry of the segment comes before the thread's own row iff its key is larger.  The reads of a step are addressed
                // by a counter, not by what the step before found, and nothing in a step branches
                int at = h > base ? (int)(h - base) : 0;
                uint32_t open = 1u;
                for (int i = at; open && i < RK_TILE; i += RK_STEP) {
                    uint64_t k[RK_STEP];
                    uint32_t o[RK_STEP];
#pragma unroll
                    for (int u = 0; u < RK_STEP; ++u) {
                        k[u] = keys[i + u];
                        o[u] = owner[i + u];
                    }
#pragma unroll
                    for (int u = 0; u < RK_STEP; ++u) {
                        // 0 / 1 in registers, not flags: flags become lane masks chained through the scalar unit, measured 1.45x slower
                        open &= (uint32_t)(o[u] == (uint32_t)h);
                        rank += (int32_t)(open & (uint32_t)(k[u] > mine));
                        at += (int)open;
                    }
                }
                if (at < RK_TILE) end = base + at;                             // (an entry behind the tile says nothing: the next tile does)
            }
            // the segment of the highest candidate head ends last: go on while the next tile starts at or before that head, or inside
            // its segment
            const int64_t next = base + RK_TILE;
            if (next >= a.B || (next > hi && clamp_row(a.first_row[next], a.B) != hi)) {
                if (end < 0) end = next < a.B ? next : a.B;                    // no end seen: the segment reaches the last tile's end
                break;
            }
            __syncthreads();                                                   // the tile is rewritten
        }
    }

    if (b < a.B) {
        if (h >= 0 && b < end) {
            a.out_rank[b] = rank;
            a.out_order[(int64_t)h + rank] = (int32_t)(b - h);
            a.out_val[(int64_t)h + rank] = v;
        } else {
            a.out_rank[b] = -1;
            a.out_order[b] = -1;
            a.out_val[b] = 0.0f;
        }
    }
}

}  // namespace

extern "C" int rat_rank_seg(const float* y, const int64_t* first_row, int64_t B, int32_t* out_order, float* out_val, int32_t* out_rank,
                            void* stream) {
    RAT_REQUIRE(y && first_row && out_order && out_val && out_rank, "null pointer");
    RAT_REQUIRE(B >= 1 && B <= 0x7fffffffLL, "B must be in [1, 2^31 - 1]");
    RankArgs a{y, first_row, out_order, out_val, out_rank, B};
    const unsigned grid = (unsigned)((B + RK_THREADS - 1) / RK_THREADS);
    RAT_LAUNCH(rank_seg_kernel, grid, RK_THREADS, 0, stream, a);
    return rat_check_launch("rat_rank_seg");
}
