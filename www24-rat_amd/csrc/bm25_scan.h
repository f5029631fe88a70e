// bm25_scan.h — what the two BM25 scans share (retrieval.hip: bm25_topk_kernel, the whole pool per query tile; online.hip:
// bm25_scan_split_kernel, a range of it).  The contract this file owns: the total order (score descending, pool index ascending) and the
// private sorted list every lane keeps under it — its initial state, the insertion with the `placed` rule, and the pop of its head
// during the merge.  rat_bm25_topk_split promises rat_bm25_topk's result bit for bit; that holds because both scans insert and pop
// through the one text below.
//
// The scoring trips are NOT here.  The two field loops differ in what a trip reads and gates (db_grp against the exact_mask gate, the
// ring's slot, the range end `hi` against N, the column stride), and one loop for both would need a flag whose branch survives into the
// other kernel's scan: each kernel keeps its own loop, with the same fp64 sums in the same order (f ascending).
//
// Everything works on the caller's arrays in place, fully unrolled: the lists stay in registers.
#pragma once
#include "rat_device.h"

namespace {

__device__ __forceinline__ bool better(double sa, int64_t ia, double sb, int64_t ib) {   // (score desc, index asc)
    return sa > sb || (sa == sb && ia < ib);
}
// candidate (so, io) against the running best (cs, ci); an index < 0 is "no entry"
__device__ __forceinline__ void take_better(double so, int64_t io, double& cs, int64_t& ci) {
    if (io >= 0 && (ci < 0 || better(so, io, cs, ci))) {
        cs = so;
        ci = io;
    }
}

// the empty lists of a query tile; kth = score of the current K-th entry (0 while the list is not full)
template <int KMAX, int QT>
__device__ __forceinline__ void list_init(double (&val)[QT][KMAX], int64_t (&idx)[QT][KMAX], double (&kth)[QT]) {
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        kth[t] = 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            val[t][k] = 0.0;
            idx[t][k] = -1;
        }
    }
}

// Row n with score s into one list of K entries: RAT_BM25_LIST_INSERT(KMAX, val[t], idx[t], kth[t], a.K, s[u][t], n).  Every lane
// walks its rows in increasing order, so among equal scores the lower index arrives first and a later row must be STRICTLY better
// than the current K-th entry to get in.
// A macro, not a function: as a __forceinline__ function the same statements compile to another instruction stream in both scans —
// the same registers, but the compares against K merged across the insertion sites and other per-loop counts
// (profiles/online/shared_code_resource_usage.txt) — and a run of that variant against the parent was slower where a work-group scans
// the whole pool (profiles/online/shared_code_ab.txt, the function variant's column).  The text below is the one copy; expanded, it is
// the code both kernels always had.  A full statement; val, idx, kth, K, s and n are plain lvalues and are evaluated more than once.
#define RAT_BM25_LIST_INSERT(KMAX, val, idx, kth, K, s, n)                                                                       \
    do {                                                                                                                         \
        if ((s) > (kth)) {                            /* positive AND strictly better than the K-th */                          \
            double cs = (s);                                                                                                     \
            int64_t ci = (n);                                                                                                    \
            bool placed = false;      /* once the newcomer sits the rest only shifts down: a displaced entry is OLDER */        \
                                      /* (lower index) than the equal scores below it and must stay in front of them */         \
            _Pragma("unroll")                                                                                                    \
            for (int k = 0; k < (KMAX); ++k) {                                                                                   \
                if (k < (K) && (placed || cs > (val)[k])) {                                                                      \
                    placed = true;                                                                                               \
                    const double ts = (val)[k];                                                                                  \
                    const int64_t ti = (idx)[k];                                                                                 \
                    (val)[k] = cs;                                                                                               \
                    (idx)[k] = ci;                                                                                               \
                    cs = ts;                                                                                                     \
                    ci = ti;                                                                                                     \
                }                                                                                                                \
                if (k == (K) - 1) (kth) = (val)[k];                                                                              \
            }                                                                                                                    \
        }                                                                                                                        \
    } while (0)

// the merge took this list's head: the winner pops it
template <int KMAX>
__device__ __forceinline__ void list_pop(double (&val)[KMAX], int64_t (&idx)[KMAX]) {
#pragma unroll
    for (int j = 0; j + 1 < KMAX; ++j) {
        val[j] = val[j + 1];
        idx[j] = idx[j + 1];
    }
    val[KMAX - 1] = 0.0;
    idx[KMAX - 1] = -1;
}

}  // namespace
