// The fixed part of one fused multilabel step (ml_step.hip): shape, ignore
// rule, cut-off and the addresses of every buffer the two kernels touch.
// Plain C, no device code. Python mirrors it field by field (ops/_hip.py,
// MlStep); ma_ml_step_field_names and ma_ml_step_sizeof let the loader and a
// test hold the two against each other. Every field is 8 bytes wide, so the
// layout has no padding.
//
// Native code reads a record on the host during the call and never keeps its
// address; kernels get the pointers by value. Every optional group is null / 0
// when absent.
#pragma once

// X(type, name), in declaration order
#define ML_STEP_FIELDS(X)                                                                          \
    X(long long, L)                                                                                \
    X(long long, ignore_index)                                                                     \
    X(long long, has_ignore)                                                                       \
    X(double, thr) /* the decision cut-off; the kernels use (float)thr */                          \
    /* count scratch [L][6] u64 = pos, neg, then predicted-positive by label (1, 0) under the */  \
    /* raw and under the sigmoid cut: filled by k_ml_step, consumed and zeroed by k_ml_tail    */  \
    X(unsigned long long*, counts)                                                                 \
    /* one byte per k_ml_step block: bit 0 = deferred a region, bit 1 = saw an element */         \
    /* outside [0,1]. Overwritten every step, never zeroed                              */         \
    X(unsigned char*, records)                                                                     \
    /* stat states, (L,) each; optional as a group */                                              \
    X(long long*, tp)                                                                              \
    X(long long*, fp)                                                                              \
    X(long long*, tn)                                                                              \
    X(long long*, fn)                                                                              \
    X(long long*, confmat) /* (L, 2, 2) state [[tn, fp], [fn, tp]]; optional */                    \
    /* exact-match states, one element each, and the per-row mismatch words (>= N u32, */         \
    /* bit 0 raw cut, bit 1 sigmoid cut; zero between steps); optional as a group        */         \
    X(long long*, correct)                                                                         \
    X(long long*, total)                                                                           \
    X(unsigned int*, rowbad)                                                                       \
    /* curve group, on iff T > 0: float thresholds, the uniform-grid parameters of        */      \
    /* bucket_of_uniform, the lazy (L, T+1, 2) histogram, the epoch buffer E (2 u32) and  */      \
    /* one flag byte per region (region_cap of them; zero between steps)                  */      \
    X(long long, T)                                                                                \
    X(const float*, thresholds)                                                                    \
    X(long long, uniform)                                                                          \
    X(double, t0)                                                                                  \
    X(double, inv_step)                                                                            \
    X(unsigned long long*, hist)                                                                   \
    X(unsigned int*, epoch_buf)                                                                    \
    X(unsigned char*, region_flags)                                                                \
    X(long long, region_cap)

typedef struct MlStep {
#define ML_STEP_DECLARE(type, name) type name;
    ML_STEP_FIELDS(ML_STEP_DECLARE)
#undef ML_STEP_DECLARE
} MlStep;
