// Device helpers shared by the threshold-curve kernels (kernels.hip and
// mc_onepass.hip). Every kernel that buckets a probability must go through
// these exact functions: the one-pass update and the two-kernel update are
// required to agree bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include "row_fold.h"

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
    // clamp in float BEFORE the conversion: (int) of a NaN or of a value past
    // INT_MAX is undefined. fmaxf drops a NaN operand, so a NaN score starts at
    // j = 0 and stays there (both fixups compare false) — bucket 0, negative
    // at every threshold, exactly as bucket_of and `score >= thr` have it.
    float g = floorf((p - t0) * inv_step);
    g = fminf(fmaxf(g, -1.0f), (float)(T - 1));
    int j = (int)g + 1;
    while (j < T && thr[j] <= p) j++;
    while (j > 0 && thr[j - 1] > p) j--;
    return j;
}

// One (class-chunk, 256-row) tile of the ballot-merge histogram: lane = row,
// the wave walks classes [c_lo, c_hi) together, identical (bucket, label) keys
// are merged per wave and ONE atomic carries the popcount. Shared by
// k_multiclass_curve_hist (kernels.hip) and the deferred phase of
// k_onepass_tail (mc_onepass.hip), so both bin a row the same way bit for bit.
// Block of 256 threads; sthr = the T thresholds in LDS; row0 = first row of
// the tile. norm: 0 none, 1 softmax from rowmax/rowinv, 2 sigmoid (already
// resolved against the batch-global decision by the caller). skip_done: rows
// marked rowinv < 0 were binned by k_mc_onepass and are left out.
// mode 0: multiclass one-vs-rest, mode 1: multilabel.
template <typename T_>
__device__ __forceinline__ void curve_hist_tile(
    const T_* __restrict__ probs, const long long* __restrict__ target, long long B, long long C,
    const float* __restrict__ sthr, int T, long long ignore_index, int has_ignore, int mode,
    int uniform, float t0, float inv_step, long long c_lo, long long c_hi, long long row0,
    int norm, const float* __restrict__ rowmax, const float* __restrict__ rowinv, bool skip_done,
    unsigned long long* __restrict__ hist /* (C, T+1, 2) */) {
    typedef long long ll;
    const int lane = threadIdx.x & 63;
    const ll row = row0 + threadIdx.x;
    bool valid = row < B;
    ll trow = 0;
    if (mode == 0 && valid) {
        trow = target[row];
        if (has_ignore && trow == ignore_index) valid = false;
    }
    if (skip_done && valid && rowinv[row] < 0.0f) valid = false;  // done in the one-pass kernel
    const float rmax = (norm == 1 && valid) ? rowmax[row] : 0.0f;
    const float rinv = (norm == 1 && valid) ? rowinv[row] : 0.0f;
    const T_* prow = probs + (valid ? row * C : 0);
    const ll* tgt_row = target + (valid ? row * C : 0);
    // one vector load covers the whole class chunk (4 scalar 2B/4B loads were
    // the latency bottleneck at small chunks)
    float pv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const bool vec4 = (c_hi - c_lo) == 4 && ((c_lo & 3) == 0) && ((C & 3) == 0);
    if (valid && vec4) unpack(reinterpret_cast<const vec4_t<T_>*>(prow)[c_lo >> 2], pv);
    for (ll c = c_lo; c < c_hi; c++) {
        int key = -1;
        if (valid) {
            int label;
            if (mode == 0) {
                label = (trow == c) ? 1 : 0;
            } else {
                ll t = tgt_row[c];
                label = (t == 1) ? 1 : 0;
                if (has_ignore && t == ignore_index) label = -1;
            }
            if (label >= 0) {
                // selects, not pv[c - c_lo]: a runtime index would put pv in scratch
                const int k = (int)(c - c_lo);
                float p = vec4 ? (k == 0 ? pv[0] : k == 1 ? pv[1] : k == 2 ? pv[2] : pv[3])
                               : ld_f32(prow, c);
                if (norm == 1) p = expf(p - rmax) * rinv;
                else if (norm == 2) p = 1.0f / (1.0f + expf(-p));
                int j = uniform ? bucket_of_uniform(p, sthr, T, t0, inv_step)
                                : bucket_of(p, sthr, T);
                key = j * 2 + label;
            }
        }
        // wave-aggregate identical keys -> one atomic per distinct key
        unsigned long long active = __ballot(key >= 0);
        while (active) {
            int leader = __ffsll((unsigned long long)active) - 1;
            int lkey = __shfl(key, leader);
            unsigned long long same = __ballot(key == lkey) & active;
            if (lane == leader)
                atomicAdd(&hist[(unsigned long long)c * (T + 1) * 2 + lkey],
                          (unsigned long long)__popcll(same));
            active &= ~same;
        }
    }
}
