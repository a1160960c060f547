// The fixed part of one fused multiclass step: shape, ignore rule and the
// addresses of every buffer the count and apply kernels touch. Plain C, no
// device code. Python mirrors it field by field (ops/_hip.py, McStep);
// ma_mc_step_field_names, ma_mc_step_sizeof and ma_mc_step_dump let the loader
// and a test hold the two against each other. Every field is 8 bytes wide, so
// the layout has no padding.
//
// Native code reads a record on the host during the call and never keeps its
// address (a plan copies it by value); kernels get the pointers by value.
// Every optional group is null / 0 when absent.
#pragma once

// X(type, name), in declaration order
#define MC_STEP_FIELDS(X)                                                                          \
    X(long long, C)                                                                                \
    X(long long, ignore_index)                                                                     \
    X(long long, has_ignore)                                                                       \
    /* count block [tp|fp|fn|valid], 3*C+1 u64: filled by the count kernels, consumed and */      \
    /* zeroed by the apply kernels                                                         */      \
    X(unsigned long long*, counts)                                                                 \
    X(unsigned long long*, confmat) /* (C, C) state, counted into directly; optional */            \
    /* stat states, (C,) each; optional as a group */                                              \
    X(long long*, tp)                                                                              \
    X(long long*, fp)                                                                              \
    X(long long*, tn)                                                                              \
    X(long long*, fn)                                                                              \
    /* exact-match states, one element each; optional as a group */                                \
    X(long long*, correct)                                                                         \
    X(long long*, total)                                                                           \
    /* softmax row statistics (B floats each) and the curve epoch buffer E (2 u32); */            \
    /* optional as a group, logits only                                              */            \
    X(float*, rowmax)                                                                              \
    X(float*, rowinv)                                                                              \
    X(unsigned int*, epoch_buf)                                                                    \
    /* top-k slot: on iff k > 0; block [tp_k|fp_k|fn_k], 3*C u64, and its four states */          \
    X(long long, k)                                                                                \
    X(unsigned long long*, topk_counts)                                                            \
    X(long long*, tp_k)                                                                            \
    X(long long*, fp_k)                                                                            \
    X(long long*, tn_k)                                                                            \
    X(long long*, fn_k)

typedef struct McStep {
#define MC_STEP_DECLARE(type, name) type name;
    MC_STEP_FIELDS(MC_STEP_DECLARE)
#undef MC_STEP_DECLARE
} McStep;
