// The multilabel decision rule shared by the kernels that threshold (N, L)
// logits or probabilities. The batch is normalised with sigmoid iff any
// element lies outside [0,1]; instead of normalising, the kernels compare the
// raw value against the cut-off moved into the logit domain.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

// sigmoid(x) > thr  <=>  x > logit(thr). The expression is the one
// k_multilabel_stat (kernels.hip) evaluates, on the device, so both produce the
// same bits: -inf at thr = 0 (always positive), +inf at thr = 1 (never).
__device__ __forceinline__ float ml_logit_threshold(float thr) {
    return logf(thr / (1.0f - thr));
}

// "outside [0,1]": false for NaN, true for +-inf
__device__ __forceinline__ bool ml_outside_unit(float x) { return x < 0.0f || x > 1.0f; }

// the probability the curve bins, written as curve_hist_tile (curve_common.h)
// writes it, so the bucket is the same bit for bit
__device__ __forceinline__ float ml_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
