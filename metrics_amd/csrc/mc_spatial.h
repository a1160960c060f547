// The fixed part of one fused spatial multiclass step (mc_spatial.hip): class
// count, ignore rule and the addresses of every buffer the two kernels touch.
// Plain C, no device code. Python mirrors it field by field (ops/_hip.py,
// McSpatialStep); ma_mc_spatial_step_field_names and
// ma_mc_spatial_step_sizeof let the loader and a test hold the two against each
// other. Every field is 8 bytes wide, so the layout has no padding.
//
// Native code reads a record on the host during the call and never keeps its
// address; kernels get the pointers by value. Every optional group is null / 0
// when absent.
#pragma once

// X(type, name), in declaration order
#define MC_SPATIAL_STEP_FIELDS(X)                                                                  \
    X(long long, C)                                                                                \
    X(long long, ignore_index)                                                                     \
    X(long long, has_ignore)                                                                       \
    /* count scratch [tp|fp|fn], 3*C u64: filled by k_mc_spatial_step, consumed and zeroed by */  \
    /* k_mc_spatial_tail                                                                      */  \
    X(unsigned long long*, counts)                                                                 \
    /* three u32 per k_mc_spatial_step block: valid pixels, saw a kept pixel with an element  */  \
    /* outside [0,1], deferred a tile. Overwritten every step, never zeroed                   */  \
    X(unsigned int*, records)                                                                      \
    /* stat states, (C,) each; optional as a group */                                              \
    X(long long*, tp)                                                                              \
    X(long long*, fp)                                                                              \
    X(long long*, tn)                                                                              \
    X(long long*, fn)                                                                              \
    X(long long*, confmat) /* (C, C) state, counted into directly; optional */                     \
    /* exact-match group: the two states and one u32 per sample (>= N words, zero between */      \
    /* steps); optional as a group                                                         */      \
    X(long long*, correct)                                                                         \
    X(long long*, total)                                                                           \
    X(unsigned int*, rowbad)                                                                       \
    X(long long, sample_cap) /* words of rowbad */                                                 \
    /* curve group, on iff T > 0: float thresholds, the uniform-grid parameters of           */   \
    /* bucket_of_uniform, the lazy (C, T+1, 2) histogram, the epoch buffer E (2 u32), the    */   \
    /* row statistics in row order (n, s) (>= N*S floats each) and one flag byte per tile    */   \
    /* (tile_cap of them, zero between steps)                                                */   \
    X(long long, T)                                                                                \
    X(const float*, thresholds)                                                                    \
    X(long long, uniform)                                                                          \
    X(double, t0)                                                                                  \
    X(double, inv_step)                                                                            \
    X(unsigned long long*, hist)                                                                   \
    X(unsigned int*, epoch_buf)                                                                    \
    X(float*, rowmax)                                                                              \
    X(float*, rowinv)                                                                              \
    X(long long, row_cap) /* floats behind rowmax and behind rowinv */                             \
    X(unsigned char*, tile_flags)                                                                  \
    X(long long, tile_cap)

typedef struct McSpatialStep {
#define MC_SPATIAL_STEP_DECLARE(type, name) type name;
    MC_SPATIAL_STEP_FIELDS(MC_SPATIAL_STEP_DECLARE)
#undef MC_SPATIAL_STEP_DECLARE
} McSpatialStep;
