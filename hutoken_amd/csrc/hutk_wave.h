// hutk_wave.h -- the primitives that the kernels of several files share: a search by one wavefront, its inclusive sum and
// maximum scans, and the scan over a workgroup of 256 threads.  Device code only; every function is inlined into its caller.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hutk {

// How many of the entries 0 .. n-1 satisfy pred, where pred(i) holds for a leading run of them and for no entry behind
// it.  One wavefront searches: each round its 64 lanes probe evenly spaced entries of the range and count the hits, so
// 2^20 entries take four dependent loads where a binary search takes twenty.  All 64 lanes must call it; all get the
// answer.  With pred(i) = x[i] < v the result is the first entry at or after v; with pred(i) = x[i] <= v the result less
// one is the last entry at or before v (-1 when there is none).
template <class Pred>
__device__ __forceinline__ int64_t wave_count_leading(int64_t n, Pred pred) {
    int64_t lo = 0, hi = n;  // entries below lo satisfy pred, those from hi on do not
    const int lane = threadIdx.x & 63;
    while (lo < hi) {
        const int64_t step = (hi - lo + 63) >> 6;
        const int64_t at = lo + lane * step;
        const int hits = __popcll(__ballot(at < hi && pred(at)));
        const int64_t top = lo + hits * step;  // the first probe that missed
        if (hits) lo += (hits - 1) * step + 1;
        hi = !hits ? lo : top < hi ? top : hi;
    }
    return lo;
}

// inclusive scan over the 64 lanes of a wavefront
template <class V>
__device__ __forceinline__ V wave_incl(V v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const V p = __shfl_up(v, off);
        if (lane >= off) v += p;
    }
    return v;
}

// inclusive maximum over the 64 lanes of a wavefront: lane i gets max(v of lanes 0 .. i)
template <class V>
__device__ __forceinline__ V wave_incl_max(V v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const V p = __shfl_up(v, off);
        if (lane >= off && p > v) v = p;
    }
    return v;
}

// exclusive scan over the 256 threads of a workgroup; total: the sum.  s_part: four values of LDS, free again after the call
template <class V>
__device__ __forceinline__ V block_excl(V v, V* s_part, V& total) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const V incl = wave_incl(v, lane);
    if (lane == 63) s_part[wave] = incl;
    __syncthreads();
    V before = incl - v;
    total = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        if (u < wave) before += s_part[u];
        total += s_part[u];
    }
    __syncthreads();
    return before;
}

}  // namespace hutk
