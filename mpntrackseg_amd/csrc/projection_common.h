// What the projectors' files share (projection.hip, exact_projection.hip): the id check, the arg-max key of the greedy rounding
// and the lock-free union-find of mpnhip_connected_components.
//
// Union-find: every edge finds both roots and links the LARGER under the smaller with a compare-and-swap, retrying from the value
// it lost to.  parent[v] <= v always holds, so there is no cycle, a walk to the root passes strictly falling ids (at most v
// steps), and the root of a component is its smallest vertex; one launch, no host loop, no flag read.
#pragma once
#include "common.h"

namespace mpnhip {

__device__ __forceinline__ bool ids_ok(int64_t r, int64_t c, int64_t N) { return r >= 0 && r < N && c >= 0 && c < N; }

// active scores are > 0.5, so their bit patterns order as unsigned integers; among equal scores the lowest edge id is largest
__device__ __forceinline__ unsigned long long pack_key(float score, int64_t e) {
    return ((unsigned long long)__float_as_uint(score) << 32) | (unsigned long long)(~(unsigned)e);
}

static __global__ void k_cc_init(int* __restrict__ parent, int64_t N) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < N) parent[v] = (int)v;
}

// every value ever stored in parent[x] is an ancestor of x and <= x, so a stale read only lengthens the walk
__device__ __forceinline__ int cc_find(int* parent, int x) {
    for (;;) {
        const int p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED);
        if (p == x) return x;
        x = p;
    }
}

// joins the components of a and b
__device__ __forceinline__ void cc_link(int* parent, int a, int b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }   // a: the larger root, goes under b
        const int old = atomicCAS(&parent[a], a, b);
        if (old == a) return;
        a = old;   // a was linked meanwhile (to something smaller): go on from there
    }
}

// root[v] = find(v); is_root (may be null) flags the roots
static __global__ void k_cc_roots(int* parent, int64_t N, int* __restrict__ root, int* __restrict__ is_root) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    const int r = cc_find(parent, (int)v);
    root[v] = r;
    if (is_root) is_root[v] = r == (int)v ? 1 : 0;
}

}  // namespace mpnhip
