// Device helpers shared by the threshold-curve kernels (kernels.hip and
// mc_onepass.hip). Every kernel that buckets a probability must go through
// these exact functions: the one-pass update and the two-kernel update are
// required to agree bit for bit.
#pragma once

#include <hip/hip_runtime.h>

__device__ __forceinline__ float bf16_to_f32(unsigned short u) {
    unsigned int v = ((unsigned int)u) << 16;
    return __uint_as_float(v);
}

// bucket j = #thresholds <= p  (searchsorted right) in [0, T]
__device__ __forceinline__ int bucket_of(float p, const float* __restrict__ thr, int T) {
    int lo = 0, hi = T;  // count of thresholds <= p
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (thr[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// For (near-)uniform threshold grids (the linspace default): O(1) guess from
// the spacing, then an EXACT +-1 fixup against the actual threshold values —
// bit-identical to the binary search at ~2 LDS reads instead of log2(T).
__device__ __forceinline__ int bucket_of_uniform(float p, const float* __restrict__ thr, int T,
                                                 float t0, float inv_step) {
    int j = (int)floorf((p - t0) * inv_step) + 1;
    j = j < 0 ? 0 : (j > T ? T : j);
    while (j < T && thr[j] <= p) j++;
    while (j > 0 && thr[j - 1] > p) j--;
    return j;
}
