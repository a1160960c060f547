// Per-row building blocks shared by the multiclass kernels (kernels.hip and
// mc_onepass.hip): element loads keyed on the dtype, the online-softmax and
// argmax folds with their 64-lane merges, the per-row counting, the epoch
// publish and the stat-delta epilogue. The one-pass step must equal the
// two-kernel step bit for bit; both call the softmax functions, so "same fold"
// holds by construction, and the two argmax forms (carried index / value first,
// for a row held in registers) follow one exact rule. Each kernel only picks its group width K per shape — K
// changes the rounding of rowinv, so a kernel's choice is part of its contract.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

// ---- dtype: T is float, or unsigned short holding bf16 bits ----
template <typename T>
inline constexpr bool is_bf16_v = std::is_same<T, unsigned short>::value;

// One statement with DT = float for dtype code 0 and DT = unsigned short for
// every other code, written once. LAUNCH_BY_DTYPE is the common case of it:
// KERNEL<DT> with the argument list written once.
#define FOR_DTYPE(dtype, ...)                                                                      \
    do {                                                                                           \
        if ((dtype) == 0) {                                                                        \
            typedef float DT;                                                                      \
            __VA_ARGS__;                                                                           \
        } else {                                                                                   \
            typedef unsigned short DT;                                                             \
            __VA_ARGS__;                                                                           \
        }                                                                                          \
    } while (0)
#define LAUNCH_BY_DTYPE(dtype, KERNEL, grid, block, shmem, stream, ...)                            \
    FOR_DTYPE(dtype, KERNEL<DT><<<grid, block, shmem, stream>>>(__VA_ARGS__))

__device__ __forceinline__ float bf16_to_f32(unsigned short u) {
    unsigned int v = ((unsigned int)u) << 16;
    return __uint_as_float(v);
}

template <typename T>
__device__ __forceinline__ float ld_f32(const T* __restrict__ p, long long i) {
    if constexpr (is_bf16_v<T>) return bf16_to_f32(p[i]);
    else return (float)p[i];
}

// 4 consecutive elements of T as one vector, and 8 bf16 as two (8-byte aligned)
template <typename T>
using vec4_t = typename std::conditional<is_bf16_v<T>, ushort4, float4>::type;
struct bf16x8 { ushort4 a; ushort4 b; };

__device__ __forceinline__ void unpack(const float4& u, float (&f)[4]) {
    f[0] = u.x; f[1] = u.y; f[2] = u.z; f[3] = u.w;
}
__device__ __forceinline__ void unpack(const ushort4& u, float (&f)[4]) {
    f[0] = bf16_to_f32(u.x); f[1] = bf16_to_f32(u.y);
    f[2] = bf16_to_f32(u.z); f[3] = bf16_to_f32(u.w);
}
__device__ __forceinline__ void unpack(const bf16x8& u, float (&f)[8]) {
    f[0] = bf16_to_f32(u.a.x); f[1] = bf16_to_f32(u.a.y);
    f[2] = bf16_to_f32(u.a.z); f[3] = bf16_to_f32(u.a.w);
    f[4] = bf16_to_f32(u.b.x); f[5] = bf16_to_f32(u.b.y);
    f[6] = bf16_to_f32(u.b.z); f[7] = bf16_to_f32(u.b.w);
}
// one packed 16-byte register vector: 8 bf16 or 4 fp32
template <typename T>
__device__ __forceinline__ void unpack16(const uint4& u, float (&f)[16 / sizeof(T)]) {
    if constexpr (is_bf16_v<T>) {
        f[0] = bf16_to_f32((unsigned short)(u.x & 0xffffu)); f[1] = bf16_to_f32((unsigned short)(u.x >> 16));
        f[2] = bf16_to_f32((unsigned short)(u.y & 0xffffu)); f[3] = bf16_to_f32((unsigned short)(u.y >> 16));
        f[4] = bf16_to_f32((unsigned short)(u.z & 0xffffu)); f[5] = bf16_to_f32((unsigned short)(u.z >> 16));
        f[6] = bf16_to_f32((unsigned short)(u.w & 0xffffu)); f[7] = bf16_to_f32((unsigned short)(u.w >> 16));
    } else {
        f[0] = __uint_as_float(u.x); f[1] = __uint_as_float(u.y);
        f[2] = __uint_as_float(u.z); f[3] = __uint_as_float(u.w);
    }
}

// ---- 64-lane exchanges without LDS ----
// MA_ROWFOLD_XLANE=0 builds every merge below on __shfl_down (ds_bpermute, an
// LDS round trip per step) instead: the A/B lever for profiles/README.md.
#ifndef MA_ROWFOLD_XLANE
#define MA_ROWFOLD_XLANE 1
#endif

// value of lane l + OFF for the lanes a __shfl_down tree towards lane 0 reads
// (l < OFF); the other lanes get an unspecified value. All 64 lanes must be
// active. OFF <= 8 is a DPP row shift (row_shl: lane l reads l + OFF of its
// 16-lane row), 16 and 32 are the half-row / half-wave swaps: with both
// operands the same register, the second result holds lane l + OFF for l in
// the lower half of each pair.
template <int OFF>
__device__ __forceinline__ unsigned int lane_down_u32(unsigned int x) {
#if MA_ROWFOLD_XLANE
    if constexpr (OFF == 32) {
        return __builtin_amdgcn_permlane32_swap(x, x, false, false)[1];
    } else if constexpr (OFF == 16) {
        return __builtin_amdgcn_permlane16_swap(x, x, false, false)[1];
    } else {
        static_assert(OFF >= 1 && OFF <= 8, "row shift");
        return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)x, 0x100 + OFF, 0xf, 0xf, true);
    }
#else
    return (unsigned int)__shfl_down((int)x, OFF);
#endif
}
template <int OFF>
__device__ __forceinline__ float lane_down(float x) {
    return __uint_as_float(lane_down_u32<OFF>(__float_as_uint(x)));
}

// max of a float / min of an unsigned over the 64 lanes, returned to every
// lane (wave-uniform); all 64 lanes must be active. Both are idempotent, so the butterfly may fold a lane's
// own value in twice: quad swaps, row rotates by 4 and 8 (every lane of a
// 16-lane row then holds the row's result), row_bcast15 into rows 1 and 3,
// row_bcast31 into rows 2 and 3; lane 63 holds the wave's. `old` = the value
// itself keeps the rows a broadcast does not write unchanged. NaN never wins
// the max (fmaxf drops it).
#define MA_DPP_STEP(v, ctrl, rows) __builtin_amdgcn_update_dpp((v), (v), (ctrl), (rows), 0xf, false)
__device__ __forceinline__ float wave_max_f32(float x) {
#if MA_ROWFOLD_XLANE
    auto step = [](float v, int o) { return fmaxf(v, __int_as_float(o)); };
    x = step(x, MA_DPP_STEP(__float_as_int(x), 0xb1, 0xf));   // quad_perm [1,0,3,2]
    x = step(x, MA_DPP_STEP(__float_as_int(x), 0x4e, 0xf));   // quad_perm [2,3,0,1]
    x = step(x, MA_DPP_STEP(__float_as_int(x), 0x124, 0xf));  // row_ror 4
    x = step(x, MA_DPP_STEP(__float_as_int(x), 0x128, 0xf));  // row_ror 8
    x = step(x, MA_DPP_STEP(__float_as_int(x), 0x142, 0xa));  // row_bcast15
    x = step(x, MA_DPP_STEP(__float_as_int(x), 0x143, 0xc));  // row_bcast31
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
#else
    for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_down(x, off));
    return __shfl(x, 0);
#endif
}
__device__ __forceinline__ unsigned int wave_min_u32(unsigned int x) {
#if MA_ROWFOLD_XLANE
    auto step = [](unsigned int v, int o) { return min(v, (unsigned int)o); };
    x = step(x, MA_DPP_STEP((int)x, 0xb1, 0xf));
    x = step(x, MA_DPP_STEP((int)x, 0x4e, 0xf));
    x = step(x, MA_DPP_STEP((int)x, 0x124, 0xf));
    x = step(x, MA_DPP_STEP((int)x, 0x128, 0xf));
    x = step(x, MA_DPP_STEP((int)x, 0x142, 0xa));
    x = step(x, MA_DPP_STEP((int)x, 0x143, 0xc));
    return (unsigned int)__builtin_amdgcn_readlane((int)x, 63);
#else
    for (int off = 32; off > 0; off >>= 1) x = min(x, (unsigned int)__shfl_down((int)x, off));
    return (unsigned int)__shfl((int)x, 0);
#endif
}

// ---- row groups: LPR lanes per row, 64 / LPR rows per wave ----
// A group is LPR consecutive lanes, LPR in {16, 32, 64}: a 16-lane DPP row, a
// half wave, or the wave. Every function below needs all 64 lanes active and
// never moves a value from one group into another, so the groups of a wave may
// hold unrelated rows (or none). LPR = 64 is the wave function above, with its
// wave-uniform result.
//
// max / min over the group, returned to every lane of it: the quad swaps and
// row rotates of the wave butterfly; a 32-lane group adds the swap of its two
// 16-lane rows.
template <int LPR>
__device__ __forceinline__ float group_max_f32(float x) {
    static_assert(LPR == 16 || LPR == 32 || LPR == 64, "lanes per row");
    if constexpr (LPR == 64) {
        return wave_max_f32(x);
    } else {
#if MA_ROWFOLD_XLANE
        auto step = [](float v, int o) { return fmaxf(v, __int_as_float(o)); };
        x = step(x, MA_DPP_STEP(__float_as_int(x), 0xb1, 0xf));
        x = step(x, MA_DPP_STEP(__float_as_int(x), 0x4e, 0xf));
        x = step(x, MA_DPP_STEP(__float_as_int(x), 0x124, 0xf));
        x = step(x, MA_DPP_STEP(__float_as_int(x), 0x128, 0xf));
        if constexpr (LPR == 32) {
            const auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
            x = fmaxf(__uint_as_float(p[0]), __uint_as_float(p[1]));
        }
#else
        for (int off = LPR / 2; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off));
#endif
        return x;
    }
}
template <int LPR>
__device__ __forceinline__ unsigned int group_min_u32(unsigned int x) {
    static_assert(LPR == 16 || LPR == 32 || LPR == 64, "lanes per row");
    if constexpr (LPR == 64) {
        return wave_min_u32(x);
    } else {
#if MA_ROWFOLD_XLANE
        auto step = [](unsigned int v, int o) { return min(v, (unsigned int)o); };
        x = step(x, MA_DPP_STEP((int)x, 0xb1, 0xf));
        x = step(x, MA_DPP_STEP((int)x, 0x4e, 0xf));
        x = step(x, MA_DPP_STEP((int)x, 0x124, 0xf));
        x = step(x, MA_DPP_STEP((int)x, 0x128, 0xf));
        if constexpr (LPR == 32) {
            const auto p = __builtin_amdgcn_permlane16_swap(x, x, false, false);
            x = min(p[0], p[1]);
        }
#else
        for (int off = LPR / 2; off > 0; off >>= 1) x = min(x, (unsigned int)__shfl_xor((int)x, off));
#endif
        return x;
    }
}
// value of the group's first lane, returned to every lane of the group: a row
// broadcast of lane 0 of each 16-lane row; in a 32-lane group the odd rows then
// take the even row's (the first result of the half-row swap).
template <int LPR>
__device__ __forceinline__ unsigned int group_first_u32(unsigned int x) {
    static_assert(LPR == 16 || LPR == 32 || LPR == 64, "lanes per row");
    if constexpr (LPR == 64) {
        return (unsigned int)__builtin_amdgcn_readfirstlane((int)x);
    } else {
#if MA_ROWFOLD_XLANE
        x = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)x, 0x150, 0xf, 0xf, false);  // row_newbcast:0
        if constexpr (LPR == 32) x = __builtin_amdgcn_permlane16_swap(x, x, false, false)[0];
        return x;
#else
        return (unsigned int)__shfl((int)x, 0, LPR);
#endif
    }
}
template <int LPR>
__device__ __forceinline__ float group_first(float x) {
    return __uint_as_float(group_first_u32<LPR>(__float_as_uint(x)));
}
#undef MA_DPP_STEP

// ---- online softmax: (m, s) = (running max, sum of exp(x - m)) ----
// Fold a group of K elements: group max first, then the group's sum, then the
// two-way merge into (m, s). row_out collects the "outside [0,1]" bit, taken
// from the group's extremes: some f[i] < 0 or > 1 <=> min < 0 or max > 1.
// fminf/fmaxf drop NaN and both compares are false for NaN, as the per-element
// test was (an all-NaN group leaves mn = mk = NaN: no bit). Returns the group
// maximum (NaN only for an all-NaN group).
template <int K>
__device__ __forceinline__ float softmax_fold(const float (&f)[K], float& m, float& s,
                                              unsigned int& row_out) {
    float mk = f[0], mn = f[0];
#pragma unroll
    for (int i = 1; i < K; i++) { mk = fmaxf(mk, f[i]); mn = fminf(mn, f[i]); }
    row_out |= (mn < 0.0f || mk > 1.0f) ? 1u : 0u;
    float sk = 0.0f;
#pragma unroll
    for (int i = 0; i < K; i++) sk += __expf(f[i] - mk);
    if (mk > m) { s = s * __expf(m - mk) + sk; m = mk; }
    else { s += sk * __expf(mk - m); }
    return mk;
}

// One step of the 64-lane merge, branch-free. Either order of the two-way
// merge scales by exp(smaller max - larger max); m is never NaN (the fold
// never stores one), so that is one __expf for both. fmaf spelled out: the
// two-branch form this replaces contracted to the same fused multiply-adds,
// and rowinv keeps its bits. m takes om only when om > m, so a -0.0 / +0.0
// pair keeps the sign it kept before.
__device__ __forceinline__ void softmax_merge_step(float& m, float& s, float om, float os) {
    const float e = __expf(fminf(m, om) - fmaxf(m, om));
    const bool up = om > m;
    s = up ? fmaf(s, e, os) : fmaf(os, e, s);
    m = up ? om : m;
}

// 64-lane merge, lane l with lane l + off for off = 32 ... 1; the row's (m, s)
// lands in lane 0
__device__ __forceinline__ void softmax_merge_wave(float& m, float& s) {
    softmax_merge_step(m, s, lane_down<32>(m), lane_down<32>(s));
    softmax_merge_step(m, s, lane_down<16>(m), lane_down<16>(s));
    softmax_merge_step(m, s, lane_down<8>(m), lane_down<8>(s));
    softmax_merge_step(m, s, lane_down<4>(m), lane_down<4>(s));
    softmax_merge_step(m, s, lane_down<2>(m), lane_down<2>(s));
    softmax_merge_step(m, s, lane_down<1>(m), lane_down<1>(s));
}

// The same merge for a row held by a group of LPR lanes (see "row groups").
// VIRTUAL LANES: lane l of the group stands for the lanes L = l + LPR*q,
// q < Q = 64 / LPR, of a wave that holds the row alone, and keeps one (m, s)
// pair per q, folded over exactly the vectors L + 64*k that lane L folds, in
// the same order. The tree of softmax_merge_wave pairs L with L + off: while
// off >= LPR that is the pair (q, q + off / LPR) of one lane, below it the
// same lane_down step, which never leaves a 16-lane row (lane_down<16> pairs
// the two rows of a 32-lane group). Same operands, same order, same rounding:
// m[0], s[0] of the group's first lane are bit for bit what lane 0 of the wave
// form holds. The other pairs are scratch afterwards.
template <int LPR>
__device__ __forceinline__ void softmax_merge_group(float (&m)[64 / LPR], float (&s)[64 / LPR]) {
    static_assert(LPR == 16 || LPR == 32 || LPR == 64, "lanes per row");
#pragma unroll
    for (int off = 32; off >= LPR; off >>= 1) {
#pragma unroll
        for (int q = 0; q < off / LPR; q++) softmax_merge_step(m[q], s[q], m[q + off / LPR], s[q + off / LPR]);
    }
    if constexpr (LPR == 64) softmax_merge_step(m[0], s[0], lane_down<32>(m[0]), lane_down<32>(s[0]));
    if constexpr (LPR >= 32) softmax_merge_step(m[0], s[0], lane_down<16>(m[0]), lane_down<16>(s[0]));
    softmax_merge_step(m[0], s[0], lane_down<8>(m[0]), lane_down<8>(s[0]));
    softmax_merge_step(m[0], s[0], lane_down<4>(m[0]), lane_down<4>(s[0]));
    softmax_merge_step(m[0], s[0], lane_down<2>(m[0]), lane_down<2>(s[0]));
    softmax_merge_step(m[0], s[0], lane_down<1>(m[0]), lane_down<1>(s[0]));
}

// ---- argmax, lowest index on a tie (torch.argmax); c = index of f[0] ----
template <int K, typename Idx>
__device__ __forceinline__ void argmax_fold(const float (&f)[K], Idx c, float& best,
                                            Idx& best_idx) {
#pragma unroll
    for (int i = 0; i < K; i++) {
        if (f[i] > best || (f[i] == best && c + i < best_idx)) { best = f[i]; best_idx = c + i; }
    }
}

template <typename Idx>
__device__ __forceinline__ void argmax_merge_wave(float& best, Idx& best_idx) {
    for (int off = 32; off > 0; off >>= 1) {
        float ov = __shfl_down(best, off);
        Idx oi = __shfl_down(best_idx, off);
        if (ov > best || (ov == best && oi < best_idx)) { best = ov; best_idx = oi; }
    }
}

// ---- argmax of a row held in registers: value first, index after ----
// The same rule as argmax_fold / argmax_merge_wave (largest non-NaN value,
// lowest index on a tie, 0x7fffffff when every element is NaN), for a kernel
// that still has the row when the maximum is known. During the fold a lane
// keeps only best = fmaxf(best, group max), starting at -INFINITY (an all-NaN
// group leaves it alone); rowbest = wave_max_f32(best); then
// row_argmax_index(): the lowest index this lane holds with f == rowbest
// (+0.0 and -0.0 tie, as they do under > and ==; a row of -inf matches at its
// first -inf; NaN matches nothing), and wave_min_u32 over the lanes.
// r[j] is vector lane + LPR*j of the row, lane counted inside the row's group
// (LPR = 64: the wave); vectors at or past nvec hold no data.
template <typename T, int NV, int LPR = 64>
__device__ __forceinline__ unsigned int row_argmax_index(const uint4 (&r)[NV], int lane, int nvec,
                                                         float rowbest) {
    constexpr int EPV = 16 / sizeof(T);
    unsigned int idx = 0x7fffffffu;
#pragma unroll
    for (int k = NV - 1; k >= 0; k--) {  // descending: the lowest match is written last
        const int v = lane + k * LPR;
        if (v < nvec) {
            float f[EPV];
            unpack16<T>(r[k], f);
#pragma unroll
            for (int i = EPV - 1; i >= 0; i--) idx = (f[i] == rowbest) ? (unsigned int)(v * EPV + i) : idx;
        }
    }
    return idx;
}

// ---- one row's counts (called by the lane that holds target and argmax) ----
// Bounds guard: bad labels with validate_args=False must not corrupt memory.
// Returns whether the row was valid (counted).
__device__ __forceinline__ bool count_row(long long t, long long p, long long C, bool ignored,
                                          unsigned long long* __restrict__ tp,
                                          unsigned long long* __restrict__ fp,
                                          unsigned long long* __restrict__ fn,
                                          unsigned long long* __restrict__ confmat) {
    if (ignored || t < 0 || t >= C || p < 0 || p >= C) return false;
    if (p == t) {
        atomicAdd(&tp[t], 1ULL);
    } else {
        atomicAdd(&fp[p], 1ULL);
        atomicAdd(&fn[t], 1ULL);
    }
    if (confmat) atomicAdd(&confmat[t * C + p], 1ULL);
    return true;
}

// ---- top-k slot: rank of the target's logit, and the row's second count ----
// rank = #{ j : x[j] > x[t] or (x[j] == x[t] and j < t) }, IEEE compares: a
// NaN element never counts, a NaN x[t] has rank 0, +0.0 and -0.0 tie and the
// index decides. The effective prediction of the slot is t if rank < k, else
// the argmax p (the reference's _refine_preds_oh). c = index of f[0].
template <int K, typename Idx>
__device__ __forceinline__ void rank_fold(const float (&f)[K], Idx c, float xt, Idx t,
                                          unsigned int& cnt) {
#pragma unroll
    for (int i = 0; i < K; i++) cnt += (f[i] > xt || (f[i] == xt && c + i < t)) ? 1u : 0u;
}

// 32-bit word wi (per lane, 0 <= wi < 4*NV) of the lane's row slice r[0..NV):
// registers cannot be indexed per lane, so the word comes out of a binary
// select tree over the bits of wi — one compare per bit and 4*NV - 1 selects,
// where a chain of (wi == q) tests pays a compare per word. NV a power of two.
template <int NV>
__device__ __forceinline__ unsigned int row_slice_word(const uint4 (&r)[NV], int wi) {
    static_assert((NV & (NV - 1)) == 0, "power of two");
    unsigned int w[4 * NV];
#pragma unroll
    for (int k = 0; k < NV; k++) { w[4 * k] = r[k].x; w[4 * k + 1] = r[k].y; w[4 * k + 2] = r[k].z; w[4 * k + 3] = r[k].w; }
#pragma unroll
    for (int bit = 0; (1 << bit) < 4 * NV; bit++) {
        const bool odd = ((wi >> bit) & 1) != 0;
#pragma unroll
        for (int i = 0; i < ((4 * NV) >> (bit + 1)); i++) w[i] = odd ? w[2 * i + 1] : w[2 * i];
    }
    return w[0];
}

// element e of a row held in registers by a group of LPR lanes (r[j] is vector
// lane + LPR*j of the row), returned to every lane of the group: the 32-bit
// word is picked out of the lane's registers and read from the lane that holds
// it. e must be the same in every lane of a group and inside the row; with
// LPR = 64 it is wave-uniform and the word comes over as a scalar, a narrower
// group reads it with a lane-indexed shuffle. All 64 lanes must be active. No
// memory access.
template <typename T, int NV, int LPR = 64>
__device__ __forceinline__ float row_element(const uint4 (&r)[NV], int e, int lane = 0) {
    constexpr int EPV = 16 / sizeof(T);
    const int vec = e / EPV, i = e % EPV;
    const int wi = (vec / LPR) * 4 + (is_bf16_v<T> ? (i >> 1) : i);  // word of the lane's slice
    unsigned int w = row_slice_word<NV>(r, wi);
    if constexpr (LPR == 64) w = (unsigned int)__builtin_amdgcn_readlane((int)w, vec & 63);
    else w = (unsigned int)__shfl((int)w, (lane & ~(LPR - 1)) | (vec & (LPR - 1)));
    if constexpr (is_bf16_v<T>) return __uint_as_float((i & 1) ? (w & 0xffff0000u) : (w << 16));
    else return __uint_as_float(w);
}

// sum over the 64 lanes, lane l with lane l + off for off = 32 ... 1; the sum
// lands in lane 0. All 64 lanes must be active.
__device__ __forceinline__ unsigned int wave_sum_u32(unsigned int x) {
    x += lane_down_u32<32>(x);
    x += lane_down_u32<16>(x);
    x += lane_down_u32<8>(x);
    x += lane_down_u32<4>(x);
    x += lane_down_u32<2>(x);
    x += lane_down_u32<1>(x);
    return x;
}
// the same over a group of LPR lanes: the steps that stay inside the group;
// the sum lands in the group's first lane
template <int LPR>
__device__ __forceinline__ unsigned int group_sum_u32(unsigned int x) {
    static_assert(LPR == 16 || LPR == 32 || LPR == 64, "lanes per row");
    if constexpr (LPR == 64) x += lane_down_u32<32>(x);
    if constexpr (LPR >= 32) x += lane_down_u32<16>(x);
    x += lane_down_u32<8>(x);
    x += lane_down_u32<4>(x);
    x += lane_down_u32<2>(x);
    x += lane_down_u32<1>(x);
    return x;
}

// Called next to count_row, for a row count_row accepted (so t and p are in
// range): the slot shares the top-1 `valid`.
__device__ __forceinline__ void count_row_topk(long long t, long long p, unsigned int rank, int k,
                                               unsigned long long* __restrict__ tp,
                                               unsigned long long* __restrict__ fp,
                                               unsigned long long* __restrict__ fn) {
    const long long pk = rank < (unsigned int)k ? t : p;
    if (pk == t) {
        atomicAdd(&tp[t], 1ULL);
    } else {
        atomicAdd(&fp[pk], 1ULL);
        atomicAdd(&fn[t], 1ULL);
    }
}

// ---- "some element of the batch lies outside [0,1]" ----
// wave OR of the per-thread bit, then one LDS OR per wave that saw it; the
// caller zeroes *blk_outside before and syncs the block after
__device__ __forceinline__ void or_outside_block(unsigned int outside, unsigned int* blk_outside) {
    for (int off = 32; off > 0; off >>= 1) outside |= __shfl_down(outside, off);
    if ((threadIdx.x & 63) == 0 && outside) atomicOr(blk_outside, 1u);
}

// one thread per block, after the sync: record epoch `cur` in E[0]. Poll before
// the global atomic: once any block set the epoch the rest skip — an atomicMax
// per block on one address serializes ~100ns each
__device__ __forceinline__ void publish_outside(unsigned int* __restrict__ E, unsigned int cur,
                                                unsigned int blk_outside) {
    if (E && blk_outside && E[0] != cur) atomicMax(&E[0], cur);
}

// ---- stat-delta epilogue for class i: consume and zero the three scratch
// slots [tp|fp|fn], add them to the states, tn += valid - the rest. Read and
// zeroed by the same thread. Returns the tp delta.
__device__ __forceinline__ long long apply_stat_class(
    unsigned long long* __restrict__ scratch, long long C, long long i, long long valid,
    long long* __restrict__ tp, long long* __restrict__ fp, long long* __restrict__ tn,
    long long* __restrict__ fn) {
    const long long dtp = (long long)scratch[i];
    const long long dfp = (long long)scratch[C + i];
    const long long dfn = (long long)scratch[2 * C + i];
    scratch[i] = 0;
    scratch[C + i] = 0;
    scratch[2 * C + i] = 0;
    tp[i] += dtp;
    fp[i] += dfp;
    fn[i] += dfn;
    tn[i] += valid - dtp - dfp - dfn;
    return dtp;
}
