// rocprim's device-wide primitives as the operators use them: how much scratch a call needs.  Included only by the files that
// call rocprim.  n is clamped to at least 1, and the query's return code is ignored on purpose: without a device it fails and
// leaves 0 bytes, so the *_workspace_bytes functions (and the argument checks in front of them) still work on such a machine.
#pragma once
#include "common.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace mpnhip {

// radix_sort_pairs of (Key, int) over all of the key's bits (sorting fewer bits never needs more)
template <class Key>
inline size_t sort_pairs_temp(int64_t n) {
    size_t bytes = 0;
    Key* k = nullptr;
    int* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, k, k, v, v, (size_t)(n > 0 ? n : 1), 0, (unsigned)(8 * sizeof(Key)), (hipStream_t)0);
    return bytes;
}

template <class T>
inline size_t exclusive_scan_temp(int64_t n) {
    size_t bytes = 0;
    T* p = nullptr;
    (void)rocprim::exclusive_scan(nullptr, bytes, p, p, (T)0, (size_t)(n > 0 ? n : 1), rocprim::plus<T>(), (hipStream_t)0);
    return bytes;
}

template <class T>
inline size_t inclusive_scan_temp(int64_t n) {
    size_t bytes = 0;
    T* p = nullptr;
    (void)rocprim::inclusive_scan(nullptr, bytes, p, p, (size_t)(n > 0 ? n : 1), rocprim::plus<T>(), (hipStream_t)0);
    return bytes;
}

}  // namespace mpnhip
