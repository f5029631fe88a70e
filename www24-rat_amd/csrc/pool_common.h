// pool_common.h — the retrieval pool's form on the device (online.hip: the scan, find, relabel, gather, count, delete; batch.hip: the
// batch assembly).  The contract this file owns:
//
//   the forms    : POOL_HOST — the row count is a host argument, no header is read; POOL_DEV — header {n}: the count lives in device
//                  memory (a pool with reserved capacity grows under a captured launch); POOL_RING — header {n, head}: the buffers are
//                  a ring of `capacity` slots, LOGICAL row i (0 = oldest) lives in slot head + i, minus capacity when that is
//                  >= capacity (head + i < 2 capacity: a compare and a subtract).  The values are rat_hip.h's RAT_POOL_*;
//   the clamps   : a header is read through pool_view — n to [0, capacity], head to [0, capacity) — so no slot outside the buffers is
//                  addressed whatever the header holds;
//   the entry    : an entry point that takes `pool_form` refuses a bad form, a missing header and a host row count outside
//                  [0, capacity] with the same words (pool_form_check), and instantiates its kernel per form through dispatch_pool.
// Everything sits in an unnamed namespace: each translation unit that includes the file gets its own copy.
#pragma once
#include "rat_device.h"
#include "../../include/rat_hip.h"

#include <type_traits>

namespace {

enum { POOL_HOST = 0, POOL_DEV = 1, POOL_RING = 2 };
static_assert(POOL_HOST == RAT_POOL_HOST && POOL_DEV == RAT_POOL_DEV && POOL_RING == RAT_POOL_RING, "the ABI's pool_form values");

__device__ __forceinline__ int64_t ring_wrap(int64_t slot, int64_t capacity) {     // slot < 2 capacity
    return slot >= capacity ? slot - capacity : slot;
}
// the ring's head, clamped to [0, capacity)
__device__ __forceinline__ int64_t ring_head(const int64_t* header, int64_t capacity) {
    const int64_t head = header[1];
    return head < 0 ? 0 : (head >= capacity ? capacity - 1 : head);
}

// the live rows as every launch sees them: n clamped to [0, capacity] and head to [0, capacity)
struct PoolView {
    int64_t n, head;
};
template <int POOL>
__device__ __forceinline__ PoolView pool_view(const int64_t* header, int64_t n_host, int64_t capacity) {
    PoolView v{n_host, 0};
    if constexpr (POOL != POOL_HOST) v.n = header[0];
    v.n = v.n < 0 ? 0 : (v.n > capacity ? capacity : v.n);
    if constexpr (POOL == POOL_RING) v.head = ring_head(header, capacity);
    return v;
}

// The requirements every entry point with a `pool_form` argument states, in the order and the words it always stated them; `who` is
// the entry point (RAT_REQUIRE would name this function) and dims_ok its own "bad dims" condition, which stands between the header's
// check and the row count's.  Returns 0 or rat_fail(...).
int pool_form_check(const char* who, int pool_form, const int64_t* header_dev, int64_t n_rows, int64_t capacity, bool dims_ok) {
    const char* msg = nullptr;
    if (!(pool_form == POOL_HOST || pool_form == POOL_DEV || pool_form == POOL_RING))
        msg = "pool_form must be 0, 1 or 2";
    else if (!(pool_form == POOL_HOST || header_dev))
        msg = "null header";
    else if (!dims_ok)
        msg = "bad dims";
    else if (!(pool_form != POOL_HOST || (n_rows >= 0 && n_rows <= capacity)))
        msg = "n_rows outside [0, capacity]";
    return msg == nullptr ? 0 : rat_fail(std::string(who) + ": " + msg);
}
// the check as an entry point states it, in RAT_REQUIRE's place: names the entry point itself and returns -1 from it
#define RAT_POOL_FORM_CHECK(pool_form, header_dev, n_rows, capacity, dims_ok)                                          \
    do {                                                                                                               \
        if (pool_form_check(__func__, (pool_form), (header_dev), (n_rows), (capacity), (dims_ok)) != 0) return -1;     \
    } while (0)

// f(std::integral_constant<int, POOL_*>) for a checked pool_form: the one place a run-time form becomes a template argument
template <class F>
auto dispatch_pool(int pool_form, F&& f) {
    if (pool_form == POOL_HOST) return f(std::integral_constant<int, POOL_HOST>{});
    if (pool_form == POOL_DEV) return f(std::integral_constant<int, POOL_DEV>{});
    return f(std::integral_constant<int, POOL_RING>{});
}

}  // namespace
