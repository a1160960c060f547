// Per-row building blocks shared by the multiclass kernels (kernels.hip and
// mc_onepass.hip): element loads keyed on the dtype, the online-softmax and
// argmax folds with their 64-lane merges, the per-row counting, the epoch
// publish and the stat-delta epilogue. The one-pass step must equal the
// two-kernel step bit for bit; both call these functions, so "same fold" holds
// by construction. Each kernel only picks its group width K per shape — K
// changes the rounding of rowinv, so a kernel's choice is part of its contract.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

// ---- dtype: T is float, or unsigned short holding bf16 bits ----
template <typename T>
inline constexpr bool is_bf16_v = std::is_same<T, unsigned short>::value;

// KERNEL<float> for dtype code 0, KERNEL<unsigned short> for every other code,
// with the argument list written once; DT names the element type inside it.
#define LAUNCH_BY_DTYPE(dtype, KERNEL, grid, block, shmem, stream, ...)                            \
    do {                                                                                           \
        if ((dtype) == 0) {                                                                        \
            typedef float DT;                                                                      \
            KERNEL<DT><<<grid, block, shmem, stream>>>(__VA_ARGS__);                               \
        } else {                                                                                   \
            typedef unsigned short DT;                                                             \
            KERNEL<DT><<<grid, block, shmem, stream>>>(__VA_ARGS__);                               \
        }                                                                                          \
    } while (0)

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

// ---- online softmax: (m, s) = (running max, sum of exp(x - m)) ----
// Fold a group of K elements: group max first, then the group's sum, then the
// two-way merge into (m, s). row_out collects the "outside [0,1]" bit.
template <int K>
__device__ __forceinline__ void softmax_fold(const float (&f)[K], float& m, float& s,
                                             unsigned int& row_out) {
    float mk = f[0];
#pragma unroll
    for (int i = 1; i < K; i++) mk = fmaxf(mk, f[i]);
    float sk = 0.0f;
#pragma unroll
    for (int i = 0; i < K; i++) {
        row_out |= (f[i] < 0.0f || f[i] > 1.0f) ? 1u : 0u;
        sk += __expf(f[i] - mk);
    }
    if (mk > m) { s = s * __expf(m - mk) + sk; m = mk; }
    else { s += sk * __expf(mk - m); }
}

// 64-lane merge; the row's (m, s) lands in lane 0
__device__ __forceinline__ void softmax_merge_wave(float& m, float& s) {
    for (int off = 32; off > 0; off >>= 1) {
        float om = __shfl_down(m, off);
        float os = __shfl_down(s, off);
        if (om > m) { s = s * __expf(m - om) + os; m = om; }
        else { s += os * __expf(om - m); }
    }
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
