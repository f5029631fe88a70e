// order_common.h — what the ends of a request share (topn.hip: rat_topn_seg, rat_candidates_expand; rank.hip: rat_rank_seg;
// catalogue.hip: rat_catalogue_expand, rat_topn_exclude, rat_topn_merge).  The contract this file owns:
//
//   the order    : order_key is THE map fp32 -> uint32 every ranking kernel orders by — ascending with the value, NaN -> 0 (below
//                  -inf, which maps to 0x007FFFFF), -0.0 -> the key of +0.0, the largest key +inf's, 0xFF800000.  rat_topn_merge
//                  merges pages rat_topn_seg ranked and rat_rank_seg's order has rat_topn_seg's as its prefix only because the three
//                  use this one function, bit for bit;
//   the rows     : f(b) = clamp_row(first_row[b], B): a row index is clamped before it addresses anything;
//   the expansion: out[b][l] = row(b)[w] where l == cols[w], otherwise ctx[f(b)][l] — one kernel and one launch rule for every source
//                  of a candidate's own columns.  The source is the args struct: its member row(b, h) names the candidate's W words.
// Everything sits in an unnamed namespace: each translation unit that includes the file gets its own copy.
#pragma once
#include "rat_device.h"
#include "../../include/rat_hip.h"

namespace {

constexpr int EXPAND_MAX_L = 8192;         // the inverse column map is L words of LDS

__device__ __forceinline__ int64_t clamp_to(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int64_t clamp_row(int64_t r, int64_t B) { return clamp_to(r, 0, B - 1); }

// fp32 -> uint32, ascending with the value: NaN -> 0 (below -inf, which maps to 0x007FFFFF), -0.0 -> the key of +0.0
__device__ __forceinline__ uint32_t order_key(float v) {
    uint32_t u = rat_fbits(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Src: ctx [B][L] (head rows only are read), cols [W], first_row [B] (any content), out [B][L], B, L, W, and row(b, h) — the W words
// of candidate b, whose request opens at row h.
// work item = one word (VEC: one 16-byte group of four) of out.  inv[l] = the w with cols[w] == l, or -1: built by every
// work-group, L + W words of traffic against the 256+ words it then writes per trip
template <bool VEC, class Src>
__global__ void __launch_bounds__(256) expand_kernel(Src a) {
    RAT_DYN_SMEM(smem);
    int32_t* inv = reinterpret_cast<int32_t*>(smem);
    for (int l = threadIdx.x; l < a.L; l += 256) inv[l] = -1;
    __syncthreads();
    for (int w = threadIdx.x; w < a.W; w += 256) {
        const int32_t c = a.cols[w];
        if (c >= 0 && c < a.L) inv[c] = w;                                      // a column outside the row is skipped
    }
    __syncthreads();
    const int per_row = VEC ? a.L / 4 : a.L;
    const int64_t total = a.B * per_row;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t b = e / per_row;
        const int l = (int)(e % per_row) * (VEC ? 4 : 1);
        const int64_t h = clamp_row(a.first_row[b], a.B);
        const int32_t* c = a.row(b, h);
        if (VEC) {
            rat_u4 v = *reinterpret_cast<const rat_u4*>(a.ctx + h * a.L + l);
            const int w0 = inv[l], w1 = inv[l + 1], w2 = inv[l + 2], w3 = inv[l + 3];
            if (w0 >= 0) v.x = (unsigned)c[w0];
            if (w1 >= 0) v.y = (unsigned)c[w1];
            if (w2 >= 0) v.z = (unsigned)c[w2];
            if (w3 >= 0) v.w = (unsigned)c[w3];
            *reinterpret_cast<rat_u4*>(a.out + b * a.L + l) = v;
        } else {
            const int w = inv[l];
            a.out[b * a.L + l] = w >= 0 ? c[w] : a.ctx[h * a.L + l];
        }
    }
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the launch of expand_kernel: 16-byte words when the row width and the buffers allow, at most 4096 work-groups, L words of LDS.
// The caller has checked B, L and W and names the launch to rat_check_launch.
template <class Src>
void expand_launch(const Src& a, void* stream) {
    const bool vec = a.L % 4 == 0 && al16(a.ctx) && al16(a.out);
    const int64_t blocks = (a.B * (vec ? a.L / 4 : a.L) + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 4096 ? blocks : 4096);
    const size_t lds = (size_t)a.L * sizeof(int32_t);
    if (vec)
        RAT_LAUNCH((expand_kernel<true, Src>), grid, 256, lds, stream, a);
    else
        RAT_LAUNCH((expand_kernel<false, Src>), grid, 256, lds, stream, a);
}

}  // namespace
