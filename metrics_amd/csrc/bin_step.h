// The fixed part of one fused binary step (bin_step.hip): ignore rule, cut-off
// and the addresses of every buffer the two kernels touch. Plain C, no device
// code. Python mirrors it field by field (ops/_hip.py, BinStep);
// ma_bin_step_field_names and ma_bin_step_sizeof let the loader and a test
// hold the two against each other. Every field is 8 bytes wide, so the layout
// has no padding.
//
// Native code reads a record on the host during the call and never keeps its
// address; kernels get the pointers by value. Every optional group is null / 0
// when absent.
#pragma once

// X(type, name), in declaration order
#define BIN_STEP_FIELDS(X)                                                                         \
    X(long long, ignore_index)                                                                     \
    X(long long, has_ignore)                                                                       \
    X(double, thr) /* the decision cut-off; the kernels use (float)thr */                          \
    /* count scratch [6] u64 = pos, neg among kept elements, then predicted-positive by label */  \
    /* (1, 0) under the raw and under the sigmoid cut: filled by k_bin_step, consumed and     */  \
    /* zeroed by k_bin_tail                                                                    */  \
    X(unsigned long long*, counts)                                                                 \
    /* one byte per k_bin_step block: bit 0 = saw an element outside [0,1] (ignored positions */  \
    /* included), bit 1 = saw a kept one. Overwritten every step, never zeroed                */  \
    X(unsigned char*, records)                                                                     \
    /* stat states, one element each; optional as a group */                                       \
    X(long long*, tp)                                                                              \
    X(long long*, fp)                                                                              \
    X(long long*, tn)                                                                              \
    X(long long*, fn)                                                                              \
    X(long long*, confmat) /* (2, 2) state [[tn, fp], [fn, tp]]; optional */                       \
    /* curve group, on iff T > 0: float thresholds, the uniform-grid parameters of          */    \
    /* bucket_of_uniform, the lazy (1, T+1, 2) histogram, the per-step scratch [2][T+1][2]   */    \
    /* u64 (raw, sigmoid; zero between steps) and the epoch buffer E (2 u32)                 */    \
    X(long long, T)                                                                                \
    X(const float*, thresholds)                                                                    \
    X(long long, uniform)                                                                          \
    X(double, t0)                                                                                  \
    X(double, inv_step)                                                                            \
    X(unsigned long long*, hist)                                                                   \
    X(unsigned long long*, curve_scratch)                                                          \
    X(unsigned int*, epoch_buf)

typedef struct BinStep {
#define BIN_STEP_DECLARE(type, name) type name;
    BIN_STEP_FIELDS(BIN_STEP_DECLARE)
#undef BIN_STEP_DECLARE
} BinStep;
