// MI355X (gfx950 / CDNA4) metric-update kernels.
//
// Design notes (see /root/repo/SURVEY.md §2.9 for the reference call sites
// each kernel replaces):
//  - every kernel is memory-bound: the rules applied are 64-wide wavefronts,
//    coalesced vectorized loads (float4 / ushort4-bf16), grid capped at
//    ~2048 blocks with grid-stride loops, per-wave shuffle reductions, and
//    integer atomics (order-independent => deterministic by construction).
//  - K1/K4 (torchmetrics functional/classification/stat_scores.py:371-449,
//    confusion_matrix.py): fused argmax + per-class tp/fp/fn (+ optional
//    full confusion matrix) in ONE pass over the (B,C) logits.
//  - K5/K2 (precision_recall_curve.py:30-251): threshold curves as a
//    bucketized histogram (binary search into sorted thresholds) — the
//    (T,2,2) confmat state is a suffix-sum of the histogram, done on device.
//  - K13 (functional/regression/*): fused elementwise-error reductions with
//    fp64 block partials reduced in a second fixed-order pass
//    (deterministic, unlike float atomics).
//  - K6/K7 (functional/detection/iou.py): all-pairs box IoU with
//    GIoU/DIoU/CIoU epilogues, boxes1 tile staged in LDS.
//
// Build: hipcc --offload-arch=gfx950 -O3 (see csrc/build.py). No CUDA
// compatibility paths; wave size is hard-coded 64.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "compute_common.h"
#include "curve_common.h"
#include "mc_step.h"

#define WAVE 64
#define CHECK(x)                                                                                   \
    do {                                                                                           \
        hipError_t _e = (x);                                                                       \
        if (_e != hipSuccess) return (int)_e;                                                      \
    } while (0)

typedef long long ll;


// ---------------------------------------------------------------------------
// K1a: fused row-argmax + multiclass stat scores from logits (B, C)
// one wave per row; tp/fp/fn per class via global atomics; optional confmat.
// Tie-break matches torch.argmax: lowest index wins.
// ---------------------------------------------------------------------------
// TOPK: the optional top-k stat slot of the fused collection step. The row's
// effective prediction for the slot is the target if its logit ranks inside
// the top k, else the argmax (row_fold.h, count_row_topk); the rank is counted
// while the row streams by, against x[t] read before the loop. A template
// parameter: without the slot this is the kernel it was before.
template <typename T, bool TOPK = false>
__global__ void __launch_bounds__(256) k_mc_stat_logits(
    const T* __restrict__ preds, const ll* __restrict__ target, ll B, ll C, ll ignore_index,
    int has_ignore, unsigned long long* __restrict__ tp, unsigned long long* __restrict__ fp,
    unsigned long long* __restrict__ fn, unsigned long long* __restrict__ confmat,
    unsigned long long* __restrict__ valid_count, ll* __restrict__ argmax_out,
    float* __restrict__ rowmax, float* __restrict__ rowinv, unsigned int* __restrict__ E,
    int topk = 0, unsigned long long* __restrict__ tp2 = nullptr,
    unsigned long long* __restrict__ fp2 = nullptr, unsigned long long* __restrict__ fn2 = nullptr) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave_in_block = threadIdx.x / WAVE;
    const int waves_per_block = blockDim.x / WAVE;
    const ll row0 = (ll)blockIdx.x * waves_per_block + wave_in_block;
    const ll row_stride = (ll)gridDim.x * waves_per_block;
    const bool want_stats = rowmax != nullptr;  // softmax row-stats piggyback
    const unsigned int cur_epoch = E ? E[1] + 1u : 0u;
    unsigned int outside = 0;
    __shared__ unsigned int block_valid;
    __shared__ unsigned int blk_outside;
    if (threadIdx.x == 0) { block_valid = 0; blk_outside = 0; }
    __syncthreads();
    unsigned int my_valid = 0;

    for (ll row = row0; row < B; row += row_stride) {
        const T* prow = preds + row * C;
        float best = -INFINITY;
        ll best_idx = 0x7fffffffffffffffLL;
        float sm_m = -3.4e38f, sm_s = 0.0f;  // online softmax (max, sumexp)
        unsigned int row_out = 0;
        // top-k slot: target and its logit before the row streams by (an
        // out-of-range target reads nothing; its row is not counted)
        ll tk = 0;
        float xt = 0.0f;
        unsigned int cnt = 0;
        if constexpr (TOPK) {
            tk = target[row];
            if (tk >= 0 && tk < C) xt = ld_f32(prow, tk);
        }
        // vectorized loads: 16B/lane for bf16 when C%8==0, else 8B/4B paths
        if (is_bf16_v<T> && (C & 7) == 0) {
            const bf16x8* pv = reinterpret_cast<const bf16x8*>(prow);
            const ll nvec = C / 8;
            for (ll v = lane; v < nvec; v += WAVE) {
                float f[8];
                unpack(pv[v], f);
                if (want_stats) softmax_fold(f, sm_m, sm_s, row_out);
                argmax_fold(f, v * 8, best, best_idx);
                if constexpr (TOPK) rank_fold(f, v * 8, xt, tk, cnt);
            }
        } else if ((C & 3) == 0) {
            const vec4_t<T>* pv = reinterpret_cast<const vec4_t<T>*>(prow);
            const ll nvec = C / 4;
            for (ll v = lane; v < nvec; v += WAVE) {
                float f[4];
                unpack(pv[v], f);
                if (want_stats) softmax_fold(f, sm_m, sm_s, row_out);
                argmax_fold(f, v * 4, best, best_idx);
                if constexpr (TOPK) rank_fold(f, v * 4, xt, tk, cnt);
            }
        } else {
            for (ll c = lane; c < C; c += WAVE) {
                const float f[1] = {ld_f32(prow, c)};
                if (want_stats) softmax_fold(f, sm_m, sm_s, row_out);
                argmax_fold(f, c, best, best_idx);
                if constexpr (TOPK) rank_fold(f, c, xt, tk, cnt);
            }
        }
        if (want_stats) {
            softmax_merge_wave(sm_m, sm_s);
            if (lane == 0) { rowmax[row] = sm_m; rowinv[row] = 1.0f / sm_s; }
        }
        argmax_merge_wave(best, best_idx);
        if constexpr (TOPK) cnt = wave_sum_u32(cnt);  // lane 0 holds the row's rank
        // the row's range bit lands in lane 0, which holds the target: an
        // ignored row takes no part in the softmax decision (reference order)
        const bool row_any_out = want_stats && __ballot(row_out != 0u) != 0ULL;
        if (lane == 0) {
            const ll t = target[row];
            const bool ignored = has_ignore && t == ignore_index;
            if (argmax_out) argmax_out[row] = best_idx;
            if (row_any_out && !ignored) outside = 1u;
            if (count_row(t, best_idx, C, ignored, tp, fp, fn, confmat)) {
                my_valid++;
                if constexpr (TOPK) count_row_topk(t, best_idx, cnt, topk, tp2, fp2, fn2);
            }
        }
    }
    // one valid-count atomic per block, not per row
    if (my_valid) atomicAdd(&block_valid, my_valid);
    or_outside_block(outside, &blk_outside);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (block_valid) atomicAdd(valid_count, (unsigned long long)block_valid);
        publish_outside(E, cur_epoch, blk_outside);
    }
}

// K1-tiny: thread-per-row variant for small C. A 64-lane wave wastes
// (64-C)/64 of its lanes when C < 64 in the wave-per-row mapping; here each
// THREAD walks one row serially (vector loads keep the per-wave footprint
// contiguous: lane i streams row i, so a wave touches 64 consecutive rows =
// full cachelines). No shuffles; per-row tail work is identical to K1.
template <typename T>
__global__ void __launch_bounds__(256) k_mc_stat_logits_tiny(
    const T* __restrict__ preds, const ll* __restrict__ target, ll B, ll C, ll ignore_index,
    int has_ignore, unsigned long long* __restrict__ tp, unsigned long long* __restrict__ fp,
    unsigned long long* __restrict__ fn, unsigned long long* __restrict__ confmat,
    unsigned long long* __restrict__ valid_count, ll* __restrict__ argmax_out,
    float* __restrict__ rowmax, float* __restrict__ rowinv, unsigned int* __restrict__ E) {
    const bool want_stats = rowmax != nullptr;
    const unsigned int cur_epoch = E ? E[1] + 1u : 0u;
    unsigned int outside = 0;
    __shared__ unsigned int block_valid;
    __shared__ unsigned int blk_outside;
    // LDS-privatized counters: with only C distinct addresses, global atomics
    // serialize badly at small C — accumulate per block, flush once
    extern __shared__ unsigned int s_cnt[];  // [tp C][fp C][fn C][confmat C*C?]
    unsigned int* s_tp = s_cnt;
    unsigned int* s_fp = s_cnt + C;
    unsigned int* s_fn = s_cnt + 2 * C;
    // confmat privatized only while C*C fits comfortably in LDS; beyond that
    // its C*C global addresses are uncontended enough anyway
    const bool priv_cm = confmat && C <= 64;
    unsigned int* s_cm = priv_cm ? s_cnt + 3 * C : nullptr;
    const ll lds_words = 3 * C + (priv_cm ? C * C : 0);
    for (ll i = threadIdx.x; i < lds_words; i += blockDim.x) s_cnt[i] = 0;
    if (threadIdx.x == 0) { block_valid = 0; blk_outside = 0; }
    __syncthreads();
    unsigned int my_valid = 0;

    for (ll row = (ll)blockIdx.x * blockDim.x + threadIdx.x; row < B;
         row += (ll)gridDim.x * blockDim.x) {
        const T* prow = preds + row * C;
        float best = -INFINITY;
        ll best_idx = 0;
        float sm_m = -3.4e38f, sm_s = 0.0f;
        unsigned int row_out = 0;
        auto fold = [&](float f, ll c) {
            if (f > best) { best = f; best_idx = c; }
            if (want_stats) {
                row_out |= (f < 0.0f || f > 1.0f) ? 1u : 0u;
                if (f > sm_m) { sm_s = sm_s * __expf(sm_m - f) + 1.0f; sm_m = f; }
                else { sm_s += __expf(f - sm_m); }
            }
        };
        if ((C & 3) == 0) {
            const vec4_t<T>* pv = reinterpret_cast<const vec4_t<T>*>(prow);
            for (ll v = 0; v < C / 4; v++) {
                float f[4];
                unpack(pv[v], f);
                fold(f[0], v * 4); fold(f[1], v * 4 + 1); fold(f[2], v * 4 + 2); fold(f[3], v * 4 + 3);
            }
        } else {
            for (ll c = 0; c < C; c++) fold(ld_f32(prow, c), c);
        }
        if (want_stats) { rowmax[row] = sm_m; rowinv[row] = 1.0f / sm_s; }
        ll t = target[row];
        ll p = best_idx;
        if (argmax_out) argmax_out[row] = p;
        // an ignored row takes no part in the softmax decision (reference order)
        outside |= (has_ignore && t == ignore_index) ? 0u : row_out;
        if (!(has_ignore && t == ignore_index) && t >= 0 && t < C && p >= 0 && p < C) {
            my_valid++;
            if (p == t) {
                atomicAdd(&s_tp[t], 1u);
            } else {
                atomicAdd(&s_fp[p], 1u);
                atomicAdd(&s_fn[t], 1u);
            }
            if (s_cm) atomicAdd(&s_cm[t * C + p], 1u);
            else if (confmat) atomicAdd(&confmat[t * C + p], 1ULL);
        }
    }
    if (my_valid) atomicAdd(&block_valid, my_valid);
    if (outside) atomicOr(&blk_outside, 1u);
    __syncthreads();
    for (ll c = threadIdx.x; c < C; c += blockDim.x) {
        if (s_tp[c]) atomicAdd(&tp[c], (unsigned long long)s_tp[c]);
        if (s_fp[c]) atomicAdd(&fp[c], (unsigned long long)s_fp[c]);
        if (s_fn[c]) atomicAdd(&fn[c], (unsigned long long)s_fn[c]);
    }
    if (s_cm) {
        for (ll i = threadIdx.x; i < C * C; i += blockDim.x)
            if (s_cm[i]) atomicAdd(&confmat[i], (unsigned long long)s_cm[i]);
    }
    if (threadIdx.x == 0) {
        if (block_valid) atomicAdd(valid_count, (unsigned long long)block_valid);
        publish_outside(E, cur_epoch, blk_outside);
    }
}

// K1b: multiclass stat scores from integer label preds (element-wise).
// use_lds=1: tp/fp/fn (and confmat when priv_cm) accumulate in LDS and flush
// once per block — global atomics over only C addresses serialize at small C.
__global__ void __launch_bounds__(256) k_mc_stat_labels(
    const ll* __restrict__ preds, const ll* __restrict__ target, ll N, ll C, ll ignore_index,
    int has_ignore, unsigned long long* __restrict__ tp, unsigned long long* __restrict__ fp,
    unsigned long long* __restrict__ fn, unsigned long long* __restrict__ confmat,
    unsigned long long* __restrict__ valid_count, int use_lds, int priv_cm) {
    extern __shared__ unsigned int s_cnt[];
    unsigned int* s_tp = use_lds ? s_cnt : nullptr;
    unsigned int* s_fp = use_lds ? s_cnt + C : nullptr;
    unsigned int* s_fn = use_lds ? s_cnt + 2 * C : nullptr;
    unsigned int* s_cm = (use_lds && priv_cm && confmat) ? s_cnt + 3 * C : nullptr;
    if (use_lds) {
        const ll lds_words = 3 * C + (s_cm ? C * C : 0);
        for (ll b = threadIdx.x; b < lds_words; b += blockDim.x) s_cnt[b] = 0;
        __syncthreads();
    }
    ll i = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    ll stride = (ll)gridDim.x * blockDim.x;
    unsigned long long local_valid = 0;
    for (; i < N; i += stride) {
        ll t = target[i];
        if (has_ignore && t == ignore_index) continue;
        ll p = preds[i];
        if (t < 0 || t >= C || p < 0 || p >= C) continue;
        local_valid++;
        if (use_lds) {
            if (p == t) {
                atomicAdd(&s_tp[t], 1u);
            } else {
                atomicAdd(&s_fp[p], 1u);
                atomicAdd(&s_fn[t], 1u);
            }
            if (s_cm) atomicAdd(&s_cm[t * C + p], 1u);
            else if (confmat) atomicAdd(&confmat[t * C + p], 1ULL);
        } else {
            if (p == t) {
                atomicAdd(&tp[t], 1ULL);
            } else {
                atomicAdd(&fp[p], 1ULL);
                atomicAdd(&fn[t], 1ULL);
            }
            if (confmat) atomicAdd(&confmat[t * C + p], 1ULL);
        }
    }
    __shared__ unsigned long long blk_valid;
    if (threadIdx.x == 0) blk_valid = 0;
    __syncthreads();
    if (local_valid) atomicAdd(&blk_valid, local_valid);
    __syncthreads();
    if (use_lds) {
        for (ll c = threadIdx.x; c < C; c += blockDim.x) {
            if (s_tp[c]) atomicAdd(&tp[c], (unsigned long long)s_tp[c]);
            if (s_fp[c]) atomicAdd(&fp[c], (unsigned long long)s_fp[c]);
            if (s_fn[c]) atomicAdd(&fn[c], (unsigned long long)s_fn[c]);
        }
        if (s_cm)
            for (ll b = threadIdx.x; b < C * C; b += blockDim.x)
                if (s_cm[b]) atomicAdd(&confmat[b], (unsigned long long)s_cm[b]);
    }
    if (threadIdx.x == 0 && blk_valid) atomicAdd(valid_count, blk_valid);
}

// ---------------------------------------------------------------------------
// K1c: LDS-privatized bincount (deterministic: integer atomics)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bincount_lds(
    const ll* __restrict__ x, ll N, ll bins, unsigned long long* __restrict__ out) {
    extern __shared__ unsigned int lbins[];
    for (ll b = threadIdx.x; b < bins; b += blockDim.x) lbins[b] = 0;
    __syncthreads();
    ll i = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    ll stride = (ll)gridDim.x * blockDim.x;
    for (; i < N; i += stride) {
        ll v = x[i];
        if (v >= 0 && v < bins) atomicAdd(&lbins[v], 1u);
    }
    __syncthreads();
    for (ll b = threadIdx.x; b < bins; b += blockDim.x) {
        unsigned int c = lbins[b];
        if (c) atomicAdd(&out[b], (unsigned long long)c);
    }
}

__global__ void __launch_bounds__(256) k_bincount_global(
    const ll* __restrict__ x, ll N, ll bins, unsigned long long* __restrict__ out) {
    ll i = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    ll stride = (ll)gridDim.x * blockDim.x;
    for (; i < N; i += stride) {
        ll v = x[i];
        if (v >= 0 && v < bins) atomicAdd(&out[v], 1ULL);
    }
}

// ---------------------------------------------------------------------------
// K4: fused binary stat scores. Counts BOTH the raw-threshold and the
// sigmoid-threshold interpretation in one pass plus an "outside [0,1]" flag,
// so the host picks the right one without a device sync (the reference's
// normalize_logits_if_needed contortion, done properly in one kernel).
// out layout: [2][4] = {raw,sig} x {tp,fp,tn,fn}; flag: 1 if any value
// outside [0,1].
// ---------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) k_binary_stat(
    const T* __restrict__ preds, const ll* __restrict__ target, ll N, float threshold,
    ll ignore_index, int has_ignore, unsigned long long* __restrict__ out,
    unsigned int* __restrict__ outside_flag) {
    ll i = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    ll stride = (ll)gridDim.x * blockDim.x;
    // thresholding sigmoid(x) > thr  <=>  x > logit(thr)
    const float logit_thr = logf(threshold / (1.0f - threshold));
    unsigned long long cnt[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    unsigned int outside = 0;
    for (; i < N; i += stride) {
        ll t = target[i];
        float p = ld_f32(preds, i);
        // the range test sees ignored elements too (reference: sigmoid iff ANY
        // element lies outside [0,1], decided before the ignore mask applies)
        outside |= (p < 0.0f || p > 1.0f) ? 1u : 0u;
        if (has_ignore && t == ignore_index) continue;
        int pr_raw = p > threshold;
        int pr_sig = p > logit_thr;
        int tt = (int)t;
        // idx: tp=0 fp=1 tn=2 fn=3
        cnt[0][pr_raw == 1 ? (tt == 1 ? 0 : 1) : (tt == 0 ? 2 : 3)]++;
        cnt[1][pr_sig == 1 ? (tt == 1 ? 0 : 1) : (tt == 0 ? 2 : 3)]++;
    }
    // wave shuffle reduce -> LDS block reduce -> ONE atomic per counter per block
    __shared__ unsigned long long blk[8];
    __shared__ unsigned int blk_outside;
    if (threadIdx.x < 8) blk[threadIdx.x] = 0;
    if (threadIdx.x == 0) blk_outside = 0;
    __syncthreads();
    for (int v = 0; v < 2; v++)
        for (int k = 0; k < 4; k++) {
            unsigned long long c = cnt[v][k];
            for (int off = WAVE / 2; off > 0; off >>= 1) c += __shfl_down(c, off);
            if ((threadIdx.x & (WAVE - 1)) == 0 && c) atomicAdd(&blk[v * 4 + k], c);
        }
    or_outside_block(outside, &blk_outside);
    __syncthreads();
    if (threadIdx.x < 8 && blk[threadIdx.x]) atomicAdd(&out[threadIdx.x], blk[threadIdx.x]);
    if (threadIdx.x == 0 && blk_outside) atomicOr(outside_flag, 1u);
}

// K4b: fused multilabel stat scores: (N, L) -> per-label [2][L][4] counters.
template <typename T>
__global__ void __launch_bounds__(256) k_multilabel_stat(
    const T* __restrict__ preds, const ll* __restrict__ target, ll N, ll L, float threshold,
    ll ignore_index, int has_ignore, unsigned long long* __restrict__ out,
    unsigned int* __restrict__ outside_flag, int use_lds) {
    // use_lds: privatize the 8L counters per block (small-L atomic contention)
    extern __shared__ unsigned int s_ml[];
    if (use_lds) {
        for (ll b = threadIdx.x; b < 8 * L; b += blockDim.x) s_ml[b] = 0;
        __syncthreads();
    }
    ll i = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    ll stride = (ll)gridDim.x * blockDim.x;
    const float logit_thr = logf(threshold / (1.0f - threshold));
    unsigned int outside = 0;
    for (; i < N * L; i += stride) {
        ll l = i % L;
        ll t = target[i];
        float p = ld_f32(preds, i);
        // the range test sees ignored elements too (reference: sigmoid iff ANY
        // element lies outside [0,1], decided before the ignore mask applies)
        outside |= (p < 0.0f || p > 1.0f) ? 1u : 0u;
        if (has_ignore && t == ignore_index) continue;
        int pr_raw = p > threshold;
        int pr_sig = p > logit_thr;
        int tt = (int)t;
        const ll j0 = (0 * L + l) * 4 + (pr_raw == 1 ? (tt == 1 ? 0 : 1) : (tt == 0 ? 2 : 3));
        const ll j1 = (1 * L + l) * 4 + (pr_sig == 1 ? (tt == 1 ? 0 : 1) : (tt == 0 ? 2 : 3));
        if (use_lds) {
            atomicAdd(&s_ml[j0], 1u);
            atomicAdd(&s_ml[j1], 1u);
        } else {
            atomicAdd(&out[j0], 1ULL);
            atomicAdd(&out[j1], 1ULL);
        }
    }
    if (use_lds) {
        __syncthreads();
        for (ll b = threadIdx.x; b < 8 * L; b += blockDim.x)
            if (s_ml[b]) atomicAdd(&out[b], (unsigned long long)s_ml[b]);
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) outside |= __shfl_down(outside, off);
    if ((threadIdx.x & (WAVE - 1)) == 0 && outside) atomicOr(outside_flag, 1u);
}

// ---------------------------------------------------------------------------
// K5/K2: threshold-curve histogram. preds are NORMALIZED probabilities.
// bucket j = #thresholds <= p  (searchsorted right) in [0, T];
// hist layout (T+1, 2): [bucket][target]. The (T,2,2) confmat state is the
// suffix-sum, computed by k_curve_suffix below.
// ---------------------------------------------------------------------------
// bucket_of / bucket_of_uniform: see curve_common.h

// detect values outside [0,1] (=> inputs are logits, normalize in-kernel).
// DEVICE-epoch protocol (hipGraph-capturable, no host state): E[1] counts
// completed curve updates (bumped by k_curve_suffix), E[0] records the epoch
// whose inputs were out-of-range. "Normalize this update" <=> E[0] == E[1]+1.
// has_ignore (binary curve only): samples whose target is ignore_index are
// removed BEFORE the range test, as in the reference; the multilabel curve
// tests every element and passes has_ignore = 0.
template <typename T_>
__global__ void __launch_bounds__(256) k_range_flag(
    const T_* __restrict__ x, ll N, const ll* __restrict__ target, ll ignore_index,
    int has_ignore, unsigned int* __restrict__ E) {
    const unsigned int cur = E[1] + 1u;  // stable: only k_curve_suffix writes E[1]
    ll i = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    ll stride = (ll)gridDim.x * blockDim.x;
    unsigned int outside = 0;
    for (; i < N; i += stride) {
        if (has_ignore && target[i] == ignore_index) continue;
        float p = ld_f32(x, i);
        outside |= (p < 0.0f || p > 1.0f) ? 1u : 0u;
    }
    __shared__ unsigned int blk_outside;
    if (threadIdx.x == 0) blk_outside = 0;
    __syncthreads();
    or_outside_block(outside, &blk_outside);
    __syncthreads();
    if (threadIdx.x == 0) publish_outside(E, cur, blk_outside);
}

// per-row max + 1/sum(exp(x - max)) for in-kernel softmax (online, one pass),
// plus the outside-[0,1] flag. Wave per row, lanes stride classes (coalesced).
template <typename T_>
__global__ void __launch_bounds__(256) k_mc_rowstats(
    const T_* __restrict__ probs, const ll* __restrict__ target, ll B, ll C, ll ignore_index,
    int has_ignore, unsigned int* __restrict__ E, float* __restrict__ rowmax,
    float* __restrict__ rowinv) {
    const unsigned int cur = E[1] + 1u;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    const int waves_per_block = blockDim.x / WAVE;
    ll row = (ll)blockIdx.x * waves_per_block + wave;
    const ll row_stride = (ll)gridDim.x * waves_per_block;
    unsigned int outside = 0;
    for (; row < B; row += row_stride) {
        const T_* prow = probs + row * C;
        // online softmax merged 8 elements at a time; 16B vector loads per
        // lane (scalar 2B loads were 3.5x slower: latency-bound)
        float m = -3.4e38f, s = 0.0f;
        // an ignored row takes no part in the range test (the reference drops
        // ignored samples before it); one wave-uniform load, only with has_ignore
        unsigned int row_out = 0;
        const bool row_ignored = has_ignore && target[row] == ignore_index;
        if (is_bf16_v<T_> && (C & 7) == 0) {
            const bf16x8* pv = reinterpret_cast<const bf16x8*>(prow);
            const ll nvec = C / 8;
            for (ll v = lane; v < nvec; v += WAVE) {
                float f[8];
                unpack(pv[v], f);
                softmax_fold(f, m, s, row_out);
            }
        } else if (!is_bf16_v<T_> && (C & 3) == 0) {
            const vec4_t<T_>* pv = reinterpret_cast<const vec4_t<T_>*>(prow);
            const ll nvec = C / 4;
            for (ll v = lane; v < nvec; v += WAVE) {
                float f[4];
                unpack(pv[v], f);
                softmax_fold(f, m, s, row_out);
            }
        } else {
            for (ll c = lane; c < C; c += WAVE) {
                const float f[1] = {ld_f32(prow, c)};
                softmax_fold(f, m, s, row_out);
            }
        }
        softmax_merge_wave(m, s);
        if (lane == 0) { rowmax[row] = m; rowinv[row] = 1.0f / s; }
        outside |= row_ignored ? 0u : row_out;
    }
    __shared__ unsigned int blk_outside2;
    if (threadIdx.x == 0) blk_outside2 = 0;
    __syncthreads();
    or_outside_block(outside, &blk_outside2);
    __syncthreads();
    if (threadIdx.x == 0) publish_outside(E, cur, blk_outside2);
}

template <typename T_>
__global__ void __launch_bounds__(256) k_binary_curve_hist(
    const T_* __restrict__ preds, const ll* __restrict__ target, ll N,
    const float* __restrict__ thresholds, int T, ll ignore_index, int has_ignore,
    int uniform, float t0, float inv_step, int norm_sigmoid, const unsigned int* __restrict__ E,
    unsigned long long* __restrict__ hist /* (T+1,2) */) {
    extern __shared__ unsigned int lhist[];  // (T+1)*2
    float* sthr = (float*)&lhist[(T + 1) * 2];
    for (int b = threadIdx.x; b < (T + 1) * 2; b += blockDim.x) lhist[b] = 0;
    for (int b = threadIdx.x; b < T; b += blockDim.x) sthr[b] = thresholds[b];
    __syncthreads();
    const bool do_sigmoid = norm_sigmoid && E && E[0] == E[1] + 1u;
    ll i = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    ll stride = (ll)gridDim.x * blockDim.x;
    for (; i < N; i += stride) {
        ll t = target[i];
        if (has_ignore && t == ignore_index) continue;
        float p = ld_f32(preds, i);
        if (do_sigmoid) p = 1.0f / (1.0f + expf(-p));
        int j = uniform ? bucket_of_uniform(p, sthr, T, t0, inv_step) : bucket_of(p, sthr, T);
        atomicAdd(&lhist[j * 2 + (t == 1 ? 1 : 0)], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < (T + 1) * 2; b += blockDim.x) {
        unsigned int c = lhist[b];
        if (c) atomicAdd(&hist[b], (unsigned long long)c);
    }
}

// multiclass one-vs-rest: probs (B, C) -> hist (C, T+1, 2), global atomics,
// coalesced row reads.
// mode 0: multiclass one-vs-rest (target (B,), label = target[row]==c)
// mode 1: multilabel (target (B,C), label = target[i])
//
// Layout: each lane owns a ROW, the wave walks the class dimension together,
// so all 64 lanes share c. Softmax-skewed probabilities pile into the same few
// buckets, so identical (bucket,label) keys are merged per wave via
// ballot/shfl and ONE atomic carries the popcount — this collapsed the
// measured 8.2M contended atomics (600us at B=8192,C=1000,T=200; probe
// csrc/probe_curve.hip) by the wave's key-multiplicity. Per-lane row reads are
// sequential in c => L1-resident after the first touch of each 64B line.
// grid: x = class chunks, y = row chunks of 256.
template <typename T_>
__global__ void __launch_bounds__(256) k_multiclass_curve_hist(
    const T_* __restrict__ probs, const ll* __restrict__ target, ll B, ll C,
    const float* __restrict__ thresholds, int T, ll ignore_index, int has_ignore, int mode,
    int uniform, float t0, float inv_step, int c_chunk,
    int norm_kind /*0 none, 1 softmax (rowstats), 2 sigmoid*/, const unsigned int* __restrict__ E,
    const float* __restrict__ rowmax, const float* __restrict__ rowinv,
    unsigned long long* __restrict__ hist /* (C, T+1, 2) */) {
    extern __shared__ float sthr2[];
    for (int b = threadIdx.x; b < T; b += blockDim.x) sthr2[b] = thresholds[b];
    __syncthreads();
    // XCD-aware chunk mapping: consecutive blockIdx.x round-robin over the 8
    // XCDs (each with its own L2), but adjacent class-chunks read 8B slices
    // of the SAME cache lines — give each XCD a contiguous band of chunks so
    // line sharing stays within one L2 instead of fetching the line 8x.
    ll bx = blockIdx.x;
    {
        const ll nx = gridDim.x;
        const ll band = nx / 8;
        // bijection on the first 8*band blocks; the tail keeps identity
        if (band > 1 && bx < 8 * band) bx = (bx % 8) * band + bx / 8;
    }
    const ll c_lo = bx * c_chunk;
    const ll c_hi = min(c_lo + (ll)c_chunk, C);
    const int norm = (norm_kind && E && E[0] == E[1] + 1u) ? norm_kind : 0;
    // the tile body is shared with the one-pass tail kernel (curve_common.h)
    curve_hist_tile<T_>(probs, target, B, C, sthr2, T, ignore_index, has_ignore, mode, uniform, t0,
                        inv_step, c_lo, c_hi, (ll)blockIdx.y * 256, norm, rowmax, rowinv,
                        /*skip_done=*/false, hist);
}

// LDS-privatized variant: each block owns a (class-chunk x T+1 x 2) uint32
// histogram in LDS, loops a row range with (8 rows x 32 classes) thread tiles
// (coalesced loads), and flushes nonzero LDS bins to global once. Wins when
// the per-wave ballot-merge variant is atomic-bound (softmax skew piles most
// of a class's mass into few buckets -> LDS same-address atomics are ~4x
// cheaper than L2, and the flush is one atomic per NONZERO bin per block).
template <typename T_>
__global__ void __launch_bounds__(256) k_multiclass_curve_hist_lds(
    const T_* __restrict__ probs, const ll* __restrict__ target, ll B, ll C,
    const float* __restrict__ thresholds, int T, ll ignore_index, int has_ignore, int mode,
    int uniform, float t0, float inv_step, int c_chunk, int rows_per_block,
    int norm_kind, const unsigned int* __restrict__ E, const float* __restrict__ rowmax,
    const float* __restrict__ rowinv, unsigned long long* __restrict__ hist /* (C, T+1, 2) */) {
    extern __shared__ unsigned int lds[];  // [c_chunk][(T+1)][2] then thresholds
    const int bins_per_class = (T + 1) * 2;
    const int lds_bins = c_chunk * bins_per_class;
    float* sthr = (float*)&lds[lds_bins];
    for (int b = threadIdx.x; b < lds_bins; b += blockDim.x) lds[b] = 0;
    for (int b = threadIdx.x; b < T; b += blockDim.x) sthr[b] = thresholds[b];
    __syncthreads();

    const ll c_lo = (ll)blockIdx.x * c_chunk;
    const ll c_hi = min(c_lo + (ll)c_chunk, C);
    const ll r_lo = (ll)blockIdx.y * rows_per_block;
    const ll r_hi = min(r_lo + (ll)rows_per_block, B);
    const int cc = threadIdx.x & 31;           // class within chunk (32-wide)
    const int rr = threadIdx.x >> 5;           // row within 8-row tile
    const ll c = c_lo + cc;
    const int norm = (norm_kind && E && E[0] == E[1] + 1u) ? norm_kind : 0;

    for (ll row = r_lo + rr; row < r_hi; row += 8) {
        ll trow = 0;
        bool rvalid = true;
        if (mode == 0) {
            trow = target[row];
            if (has_ignore && trow == ignore_index) rvalid = false;
        }
        if (rvalid && c < c_hi) {
            int label;
            if (mode == 0) {
                label = (trow == c) ? 1 : 0;
            } else {
                ll t = target[row * C + c];
                label = (t == 1) ? 1 : 0;
                if (has_ignore && t == ignore_index) label = -1;
            }
            if (label >= 0) {
                float p = ld_f32(probs, row * C + c);
                if (norm == 1) p = expf(p - rowmax[row]) * rowinv[row];
                else if (norm == 2) p = 1.0f / (1.0f + expf(-p));
                const int j = uniform ? bucket_of_uniform(p, sthr, T, t0, inv_step)
                                      : bucket_of(p, sthr, T);
                atomicAdd(&lds[cc * bins_per_class + j * 2 + label], 1u);
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < lds_bins; b += blockDim.x) {
        const unsigned int v = lds[b];
        if (v) {
            const int lc = b / bins_per_class;
            const int bin = b - lc * bins_per_class;
            const ll gc = c_lo + lc;
            if (gc < C) atomicAdd(&hist[gc * (ll)(T + 1) * 2 + bin], (unsigned long long)v);
        }
    }
}

// suffix-sum the histogram into (/onto) the running confmat state:
//   confmat[t][1][1] += sum_{j>t} hist[j][1]   (tp)
//   confmat[t][0][1] += sum_{j>t} hist[j][0]   (fp)
//   confmat[t][1][0] += pos_total - tp         (fn)
//   confmat[t][0][0] += neg_total - fp         (tn)
// one block per outer index (class or 1). The histogram is staged in LDS and
// suffix-summed there (global O(T^2) loads -> LDS): T <= 4096.
// transposed=1 writes the (T, O, 2, 2) layout (the metric state layout for
// multiclass/multilabel curves) so the accumulation happens in-place with no
// permute+copy of the 6.4MB state.
__global__ void k_curve_suffix(
    unsigned long long* __restrict__ hist /* (O, T+1, 2) */, int T, ll outer, int transposed,
    int zero_hist, unsigned int* __restrict__ E /* nullable device-epoch */,
    ll* __restrict__ confmat /* (O, T, 2, 2) or (T, O, 2, 2) */) {
    extern __shared__ unsigned long long sh[];  // (T+1) * 2
    const ll o = blockIdx.x;
    unsigned long long* h = hist + o * (ll)(T + 1) * 2;
    ll* cm = confmat + (transposed ? o * 4 : o * (ll)T * 4);
    const ll tstride = transposed ? outer * 4 : 4;
    for (int j = threadIdx.x; j < (T + 1) * 2; j += blockDim.x) sh[j] = h[j];
    __syncthreads();
    // the histogram scratch is consumed here: zero it in-flight so the next
    // update skips a separate fill kernel (buffer is reused, stream-ordered)
    if (zero_hist)
        for (int j = threadIdx.x; j < (T + 1) * 2; j += blockDim.x) h[j] = 0;
    __shared__ unsigned long long pos_total, neg_total;
    if (threadIdx.x == 0) {
        unsigned long long pt = 0, nt = 0;
        for (int j = 0; j <= T; j++) { nt += sh[j * 2 + 0]; pt += sh[j * 2 + 1]; }
        pos_total = pt; neg_total = nt;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        unsigned long long tp = 0, fp = 0;
        for (int j = t + 1; j <= T; j++) { fp += sh[j * 2 + 0]; tp += sh[j * 2 + 1]; }
        // layout [t][target][pred] (reference: bins = 2*target + pred)
        ll* c = cm + (ll)t * tstride;
        c[3] += (ll)tp;                    // [1][1] tp
        c[1] += (ll)fp;                    // [0][1] fp
        c[2] += (ll)(pos_total - tp);      // [1][0] fn
        c[0] += (ll)(neg_total - fp);      // [0][0] tn
    }
    // close this update's epoch: next curve update compares against E[1]+1
    if (E && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&E[1], 1u);
}

// tiled suffix kernel for the TRANSPOSED (T, C, 2, 2) state layout: one block
// per tile of CTILE classes; per-class suffix sums are scanned once into LDS
// and the state writes go out as contiguous (CTILE*4)-element runs per t —
// the one-class-per-block version wrote 32 KB-strided 32 B chunks (every
// write its own cache line RMW).
template <int CTILE>
__global__ void k_curve_suffix_tiled(
    unsigned long long* __restrict__ hist /* (C, T+1, 2) */, int T, ll C, int zero_hist,
    unsigned int* __restrict__ E, ll* __restrict__ confmat /* (T, C, 2, 2) */) {
    extern __shared__ unsigned long long shs[];
    unsigned long long* stage = shs;                       // CTILE * (T+1) * 2
    unsigned long long* suf = shs + CTILE * (ll)(T + 1) * 2;  // CTILE * (T+1) * 2
    const ll c0 = (ll)blockIdx.x * CTILE;
    const int ctile = (int)min((ll)CTILE, C - c0);
    // the tile body is shared with k_curve_flush_auc (compute_common.h)
    curve_suffix_tile<CTILE, false>(hist, T, C, zero_hist, 1, confmat, stage, suf, c0, ctile);
    if (E && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&E[1], 1u);
}

// Pay what a histogram in "pending b0" format still owes (mc_onepass.hip): the
// one-pass step leaves out every element of bucket b0 = bucket_of(0.0f) of the
// rows it bins from registers and keeps, per class and since the last flush,
// P[c] = binned rows whose target is c and R[c] = binned rows. Class c got one
// element per such row, label 1 for P[c] of them, so
//     hist[c][b0][1] += P[c]          - sum_j hist[c][j][1]
//     hist[c][b0][0] += (R[c] - P[c]) - sum_j hist[c][j][0]
// completes it exactly. One wave per class: lane l sums the words l, l + 64,
// ... of the class row (coalesced; 64 is even, so a lane keeps to one label),
// the lanes of a label are added up, lane 0 stores both. Plain stores: the
// kernel runs between a step and the suffix kernel, alone on the histogram.
// P and R are zeroed here: the histogram no longer owes anything.
__global__ void __launch_bounds__(256) k_curve_resolve_pending(
    unsigned long long* __restrict__ hist /* (C, T+1, 2) */, ll C, int T,
    const float* __restrict__ thresholds, unsigned long long* __restrict__ P,
    unsigned long long* __restrict__ R) {
    typedef unsigned long long ull;
    const int lane = threadIdx.x & 63;
    const ll c = (ll)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    if (c >= C) return;  // whole waves leave: c is wave-uniform
    const int row = (T + 1) * 2;
    ull* h = hist + c * (ll)row;
    ull sum = 0;
    for (int j = lane; j < row; j += 64) sum += h[j];
    for (int off = 32; off >= 2; off >>= 1) sum += __shfl_down(sum, off);
    const ull sum1 = __shfl(sum, 1);  // label 1; lane 0 holds label 0
    if (lane == 0) {
        const ull p = P[c], r = R[c];
        const int b0 = bucket_of(0.0f, thresholds, T);
        h[b0 * 2 + 0] += (r - p) - sum;
        h[b0 * 2 + 1] += p - sum1;
        P[c] = 0;
        R[c] = 0;
    }
}

// ---------------------------------------------------------------------------
// fused (C,C) confusion-matrix scalar computes: MCC + unweighted Cohen kappa +
// macro Jaccard in TWO launches. The eager torch chains emit ~25 small
// kernels (row/col sums, traces, dot products, guarded divides) per compute;
// at ~4us dispatch each that is pure launch overhead. Phase A tiles columns
// (coalesced) and emits row sums (wave-reduced, one atomic per row-tile),
// column sums and the diagonal; phase B (one block) folds the C-sized
// vectors into the three scalars and re-zeroes the row-sum scratch in-flight.
__global__ void k_confmat_moments(
    const ll* __restrict__ cm, ll C, ll rows_per_block,
    unsigned long long* __restrict__ tk /* (C), pre-zeroed */,
    unsigned long long* __restrict__ pk /* (C), pre-zeroed */,
    unsigned long long* __restrict__ diag) {
    // 2D grid: x tiles 256 columns (coalesced), y tiles rows — a column-only
    // grid is 4 blocks at C=1000 (0.4% occupancy, measured 575us); row tiling
    // brings it to the ~10us memory floor at the cost of pk atomics
    const ll c = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    const ll r_lo = (ll)blockIdx.y * rows_per_block;
    const ll r_hi = min(r_lo + rows_per_block, C);
    const int lane = threadIdx.x & (WAVE - 1);
    unsigned long long col_acc = 0;
    for (ll r = r_lo; r < r_hi; r++) {
        unsigned long long v = (c < C) ? (unsigned long long)cm[r * C + c] : 0ULL;
        col_acc += v;
        if (c == r) diag[r] = v;
        // wave-reduce this tile's contribution to row r: one atomic per wave
        unsigned long long rv = v;
        for (int off = WAVE / 2; off > 0; off >>= 1) rv += __shfl_down(rv, off);
        if (lane == 0 && rv) atomicAdd(&tk[r], rv);
    }
    if (c < C && col_acc) atomicAdd(&pk[c], col_acc);
}

__global__ void k_confmat_scalars(
    unsigned long long* __restrict__ pk, const unsigned long long* __restrict__ diag,
    unsigned long long* __restrict__ tk /* consumed + re-zeroed */, ll C,
    float zero_division, float* __restrict__ out /* [mcc, kappa, jaccard_macro] */) {
    confmat_scalars_eval(pk, diag, tk, C, zero_division, out);
}

// single-thread epoch close for the lazy-confmat path (see ma_curve_epoch_bump)
__global__ void k_epoch_bump(unsigned int* __restrict__ E) {
    if (threadIdx.x == 0) E[1] += 1u;
}

// exact-match epilogue: correct += sum(tp), total += valid — one block,
// zeroes the scratch in-flight (same valid-slot protocol as k_apply_stat_exact).
__global__ void k_exact_apply(unsigned long long* __restrict__ scratch, ll C, ll B,
                              ll* __restrict__ correct, ll* __restrict__ total) {
    __shared__ unsigned long long part[256];
    unsigned long long acc = 0;
    for (ll i = threadIdx.x; i < C; i += blockDim.x) {
        acc += scratch[i];
        scratch[i] = 0;
        scratch[C + i] = 0;
        scratch[2 * C + i] = 0;
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // reference semantics (_multiclass_exact_match_update): ignored
        // samples are forced equal, so they count as correct AND in total
        const ll valid = (ll)scratch[3 * C];
        correct[0] += (ll)part[0] + (B - valid);
        total[0] += B;
        scratch[3 * C] = 0;
    }
}

// fused stat-delta apply: given the kernel scratch [tp|fp|fn|valid] produced
// by k_mc_stat_*, add the deltas into the four metric state tensors
// (tn += valid - tp - fp - fn) and, when correct/total are given, the
// exact-match accumulation of k_exact_apply — ONE launch replaces ~8 small
// torch kernels (and the back-to-back k_exact_apply + apply pair).
// SINGLE block: every thread can read the valid slot before thread 0 zeroes
// it (post-sync), so the whole scratch is consumed and re-zeroed in one launch
// with no cross-block race and no host-side epochs — which also makes the
// launch hipGraph-capturable.
// TOPK: the same launch also applies the top-k slot's scratch [tp_k|fp_k|fn_k]
// to its four states, with the same valid.
template <bool TOPK>
__global__ void k_apply_stat_exact(
    unsigned long long* __restrict__ scratch /* 3*C + 1 */, ll C, ll B,
    ll* __restrict__ tp, ll* __restrict__ fp, ll* __restrict__ tn, ll* __restrict__ fn,
    ll* __restrict__ correct /* nullable, with total */, ll* __restrict__ total,
    unsigned int* __restrict__ E /* nullable: close the curve epoch here */,
    unsigned long long* __restrict__ scratch2 /* 3*C, TOPK only */, ll* __restrict__ tp2,
    ll* __restrict__ fp2, ll* __restrict__ tn2, ll* __restrict__ fn2) {
    if (E && threadIdx.x == 0) E[1] += 1u;
    __shared__ unsigned long long part[256];
    __shared__ unsigned long long valid_s;
    if (threadIdx.x == 0) valid_s = scratch[3 * C];
    __syncthreads();
    const ll valid = (ll)valid_s;
    if (threadIdx.x == 0) scratch[3 * C] = 0;
    unsigned long long acc = 0;
    for (ll i = threadIdx.x; i < C; i += blockDim.x) {
        acc += (unsigned long long)apply_stat_class(scratch, C, i, valid, tp, fp, tn, fn);
        if constexpr (TOPK) apply_stat_class(scratch2, C, i, valid, tp2, fp2, tn2, fn2);
    }
    if (!correct) return;  // block-uniform
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        correct[0] += (ll)part[0] + (B - valid);
        total[0] += B;
    }
}

// one-launch stat-score compute (_linear_stat_eval, compute_common.h),
// batched: one block per formula over the SAME shared (C,) stat
// states — the 9 linear stat metrics of a compute group pay ONE dispatch per
// compute generation instead of nine. params: 13 floats per formula
// (n0-3, d0-3, avg_mode, zero_w_topk, zero_division, post_a, post_b).
__global__ void k_linear_stat_multi(
    const ll* __restrict__ tp, const ll* __restrict__ fp, const ll* __restrict__ tn,
    const ll* __restrict__ fn, ll C, const float* __restrict__ params,
    float* __restrict__ outs) {
    linear_stat_eval_params(tp, fp, tn, fn, C, params + (ll)blockIdx.x * 13, outs + blockIdx.x);
}

// per-class AUROC / AveragePrecision straight from the thresholded curve
// confmat state (T, C, 2, 2) — one block per class, threads stride the
// threshold axis; replaces the ~25-launch torch chain (safe-divides, flips,
// cats, trapz) at compute time. mode 0: AUROC (trapz of tpr over fpr, flipped
// t), weights = support at the last threshold. mode 1: AP
// (-sum((r[t+1]-r[t]) * p[t]) with p_T=1, r_T=0), weights = support at t=0.
__global__ void k_curve_auc_from_confmat(
    const ll* __restrict__ confmat /* (T, C, 2, 2) */, int T, ll C, int mode,
    float* __restrict__ out /* (C,) */, float* __restrict__ weights /* (C,) nullable */) {
    const ll c = blockIdx.x;
    __shared__ double red[256];
    // integrands, slot order and tree are shared with k_curve_flush_auc
    const CurveCmGlobal cm{confmat, C, c};
    red[threadIdx.x] = curve_auc_slot_sum(cm, T, mode, (int)threadIdx.x);
    __syncthreads();
    tree256_block(red);
    if (threadIdx.x == 0) {
        out[c] = (float)red[0];
        if (weights) weights[c] = curve_auc_weight(cm, T, mode);
    }
}

// ---------------------------------------------------------------------------
// K13: fused elementwise-error reductions, deterministic fp64 two-pass.
// op: 0 = squared error, 1 = abs error, 2 = abs percentage |d|/max(|t|,eps),
//     3 = squared log error (log1p(x)-log1p(y))^2, 4 = moments
//     (n. sum_x, sum_x2, sum_y, sum_y2, sum_xy -> 6 outputs), 5 = logcosh
// partials: (num_blocks, n_out) f64; second kernel reduces in fixed order.
// ---------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) k_err_reduce_partial(
    const T* __restrict__ x, const T* __restrict__ y, ll N, int op, double eps,
    double* __restrict__ partials, int n_out) {
    __shared__ double sdata[256 * 2];  // up to 2 accumulators reduced at once per pass
    double acc[6] = {0, 0, 0, 0, 0, 0};
    ll i = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    ll stride = (ll)gridDim.x * blockDim.x;
    for (; i < N; i += stride) {
        float xf = ld_f32(x, i), yf = ld_f32(y, i);
        double xd = xf, yd = yf;
        switch (op) {
            case 0: { double d = xd - yd; acc[0] += d * d; } break;
            case 1: acc[0] += fabs(xd - yd); break;
            case 2: acc[0] += fabs(xd - yd) / fmax(fabs(yd), eps); break;
            case 3: { double d = log1p(xd) - log1p(yd); acc[0] += d * d; } break;
            case 4:
                acc[0] += xd; acc[1] += xd * xd; acc[2] += yd; acc[3] += yd * yd; acc[4] += xd * yd;
                acc[5] += 1.0;
                break;
            // log cosh d = |d| + log1p(exp(-2|d|)) - ln 2: exp never overflows
            case 5: { double d = fabs(xd - yd); acc[0] += d + log1p(exp(-2.0 * d)) - 0.6931471805599453; } break;
        }
    }
    // block tree-reduce each accumulator
    for (int a = 0; a < n_out; a++) {
        sdata[threadIdx.x] = acc[a];
        __syncthreads();
        for (int s = blockDim.x / 2; s > 0; s >>= 1) {
            if (threadIdx.x < s) sdata[threadIdx.x] += sdata[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) partials[(ll)blockIdx.x * n_out + a] = sdata[0];
        __syncthreads();
    }
}

__global__ void k_err_reduce_final(const double* __restrict__ partials, int num_blocks, int n_out,
                                   double* __restrict__ out) {
    // single block; fixed-order accumulation per output => deterministic
    for (int a = threadIdx.x; a < n_out; a += blockDim.x) {
        double s = 0;
        for (int b = 0; b < num_blocks; b++) s += partials[(ll)b * n_out + a];
        out[a] += s;
    }
}

// ---------------------------------------------------------------------------
// K6/K7: all-pairs box IoU (xyxy) with GIoU/DIoU/CIoU epilogues.
// variant: 0=iou 1=giou 2=diou 3=ciou. boxes1 tile staged in LDS.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_box_iou(
    const float* __restrict__ b1, ll N, const float* __restrict__ b2, ll M, int variant,
    float* __restrict__ out /* (N, M) */) {
    __shared__ float tile[64][4];
    // grid: (ceil(M/256), ceil(N/64))
    ll j = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    ll i0 = (ll)blockIdx.y * 64;
    ll ilim = min((ll)64, N - i0);
    for (int k = threadIdx.x; k < 64 * 4; k += blockDim.x) {
        int r = k / 4;
        if (i0 + r < N) tile[r][k % 4] = b1[(i0 + r) * 4 + (k % 4)];
    }
    __syncthreads();
    if (j >= M) return;
    float x1b = b2[j * 4 + 0], y1b = b2[j * 4 + 1], x2b = b2[j * 4 + 2], y2b = b2[j * 4 + 3];
    float area_b = (x2b - x1b) * (y2b - y1b);
    for (ll r = 0; r < ilim; r++) {
        float x1a = tile[r][0], y1a = tile[r][1], x2a = tile[r][2], y2a = tile[r][3];
        float area_a = (x2a - x1a) * (y2a - y1a);
        float ix1 = fmaxf(x1a, x1b), iy1 = fmaxf(y1a, y1b);
        float ix2 = fminf(x2a, x2b), iy2 = fminf(y2a, y2b);
        float iw = fmaxf(ix2 - ix1, 0.0f), ih = fmaxf(iy2 - iy1, 0.0f);
        float inter = iw * ih;
        float uni = area_a + area_b - inter;
        float iou = uni > 0.f ? inter / uni : 0.0f;
        float res = iou;
        if (variant >= 1) {
            float cx1 = fminf(x1a, x1b), cy1 = fminf(y1a, y1b);
            float cx2 = fmaxf(x2a, x2b), cy2 = fmaxf(y2a, y2b);
            if (variant == 1) {  // GIoU
                float carea = (cx2 - cx1) * (cy2 - cy1);
                res = carea > 0.f ? iou - (carea - uni) / carea : iou;
            } else {
                float cw = cx2 - cx1, ch = cy2 - cy1;
                float cdiag = cw * cw + ch * ch + 1e-7f;
                float dx = (x1a + x2a - x1b - x2b) * 0.5f, dy = (y1a + y2a - y1b - y2b) * 0.5f;
                float dist = dx * dx + dy * dy;
                if (variant == 2) {  // DIoU
                    res = iou - dist / cdiag;
                } else {  // CIoU
                    float wa = x2a - x1a, ha = y2a - y1a, wb = x2b - x1b, hb = y2b - y1b;
                    float v = (4.0f / (M_PI * M_PI)) *
                              powf(atanf(wb / (hb + 1e-7f)) - atanf(wa / (ha + 1e-7f)), 2.0f);
                    float alpha = v / (1.0f - iou + v + 1e-7f);
                    res = iou - dist / cdiag - alpha * v;
                }
            }
        }
        out[(i0 + r) * M + j] = res;
    }
}

// ---------------------------------------------------------------------------
// extern "C" launchers
// ---------------------------------------------------------------------------
static inline int grid_for(ll n, int block) {
    ll g = (n + block - 1) / block;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (int)g;
}

// rows per wave of k_mc_stat_logits (MA_STAT_DIV) and the largest C of the
// thread-per-row kernel (MA_STAT_SMALLC), each read once
static int mc_stat_rows_div() {
    static int rows_div = 0;
    if (rows_div == 0) {
        const char* e = getenv("MA_STAT_DIV");
        rows_div = e ? atoi(e) : 16;
        if (rows_div < 4) rows_div = 4;
    }
    return rows_div;
}
static int mc_stat_smallc() {
    static int smallc = -1;
    if (smallc < 0) {
        const char* e = getenv("MA_STAT_SMALLC");
        smallc = e ? atoi(e) : 128;
    }
    return smallc;
}

extern "C" {

// whether ma_mc_stat_logits has the top-k slot at C classes: the thread-per-row
// kernel for small C has none
int ma_mc_stat_topk_covers(ll C) { return C > mc_stat_smallc() ? 1 : 0; }

// Count pass over (B, C) logits into the record's count block (and confmat,
// row statistics, argmax_out where given). The top-k slot is on iff st->k > 0:
// the pass then also counts, per valid row, the effective prediction "target if
// it ranks inside the top k, else the argmax" into topk_counts. -103 where the
// slot is asked for but not covered, or a buffer it needs is missing.
int ma_mc_stat_logits(uintptr_t stream, const McStep* st, uintptr_t preds,
                      int dtype /*0=f32 1=bf16*/, uintptr_t target, ll B, uintptr_t argmax_out) {
    hipStream_t s = (hipStream_t)stream;
    const ll C = st->C;
    if (!st->counts) return -103;
    if (st->k != 0 && (st->k < 0 || !ma_mc_stat_topk_covers(C) || !st->topk_counts)) return -103;
#define MC_STAT_ARGS                                                                               \
    (const DT*)preds, (const ll*)target, B, C, st->ignore_index, (int)st->has_ignore, st->counts,  \
        st->counts + C, st->counts + 2 * C, st->confmat, st->counts + 3 * C, (ll*)argmax_out,      \
        st->rowmax, st->rowinv, st->epoch_buf
    // small-C: thread-per-row variant (wave-per-row wastes (64-C)/64 lanes)
    if (C <= mc_stat_smallc()) {
        int grid = grid_for(B, 256);
        if (grid > 4096) grid = 4096;
        const size_t shmem =
            (size_t)(3 * C + (st->confmat && C <= 64 ? C * C : 0)) * sizeof(unsigned int);
        LAUNCH_BY_DTYPE(dtype, k_mc_stat_logits_tiny, grid, 256, shmem, s, MC_STAT_ARGS);
        return (int)hipGetLastError();
    }
    // each wave loops several rows: more vector loads in flight per lane
    // (latency-bound otherwise; sweep tools/curve_sweep.py analogue)
    const int grid = grid_for(B, mc_stat_rows_div());
    if (st->k > 0) {
        unsigned long long* c2 = st->topk_counts;
        FOR_DTYPE(dtype, (k_mc_stat_logits<DT, true><<<grid, 256, 0, s>>>(
                             MC_STAT_ARGS, (int)st->k, c2, c2 + C, c2 + 2 * C)));
    } else {
        FOR_DTYPE(dtype, (k_mc_stat_logits<DT, false><<<grid, 256, 0, s>>>(MC_STAT_ARGS)));
    }
#undef MC_STAT_ARGS
    return (int)hipGetLastError();
}

// The same counts from integer label predictions. No row statistics, and no
// top-k slot: -103 where it is asked for, as above.
int ma_mc_stat_labels(uintptr_t stream, const McStep* st, uintptr_t preds, uintptr_t target,
                      ll N) {
    hipStream_t s = (hipStream_t)stream;
    const ll C = st->C;
    if (!st->counts || st->k != 0) return -103;
    const int use_lds = C <= 128;
    const int priv_cm = st->confmat && C <= 64;
    const size_t shmem = use_lds ? (size_t)(3 * C + (priv_cm ? C * C : 0)) * sizeof(unsigned int) : 0;
    int grid = grid_for(N, 256);
    if (grid > 4096) grid = 4096;
    k_mc_stat_labels<<<grid, 256, shmem, s>>>(
        (const ll*)preds, (const ll*)target, N, C, st->ignore_index, (int)st->has_ignore,
        st->counts, st->counts + C, st->counts + 2 * C, st->confmat, st->counts + 3 * C, use_lds,
        priv_cm);
    return (int)hipGetLastError();
}

// Apply pass, one single-block launch: consumes and zeroes the count block (and
// the top-k block) into the stat states, adds the exact-match counts of the B
// rows where correct/total are given, and closes the curve epoch (E[1] += 1)
// when close_epoch is set. A record without stat states is the stand-alone
// exact-match update; one with neither has nothing to consume, and only an
// epoch asked for is closed.
int ma_mc_stat_apply(uintptr_t stream, const McStep* st, ll B, int close_epoch) {
    hipStream_t s = (hipStream_t)stream;
    unsigned int* E = close_epoch ? st->epoch_buf : nullptr;
    if (!st->counts || (close_epoch && !E) || !st->correct != !st->total) return -103;
    if (!st->tp) {
        if (st->k != 0) return -103;
        if (st->correct)
            k_exact_apply<<<1, 256, 0, s>>>(st->counts, st->C, B, st->correct, st->total);
        if (E) k_epoch_bump<<<1, 1, 0, s>>>(E);
        return (int)hipGetLastError();
    }
    if (!st->fp || !st->tn || !st->fn) return -103;
    if (st->k > 0) {
        if (!st->topk_counts || !st->tp_k || !st->fp_k || !st->tn_k || !st->fn_k) return -103;
        k_apply_stat_exact<true><<<1, 256, 0, s>>>(st->counts, st->C, B, st->tp, st->fp, st->tn,
                                                   st->fn, st->correct, st->total, E,
                                                   st->topk_counts, st->tp_k, st->fp_k, st->tn_k,
                                                   st->fn_k);
    } else {
        k_apply_stat_exact<false><<<1, 256, 0, s>>>(st->counts, st->C, B, st->tp, st->fp, st->tn,
                                                    st->fn, st->correct, st->total, E, nullptr,
                                                    nullptr, nullptr, nullptr, nullptr);
    }
    return (int)hipGetLastError();
}

// Host only: every field of a record as u64, in declaration order, and the
// size of the record, for the layout check of the Python mirror. Returns the
// number of fields written.
int ma_mc_step_dump(const McStep* st, unsigned long long* out) {
    int n = 0;
#define MC_STEP_DUMP(type, name) out[n++] = (unsigned long long)st->name;
    MC_STEP_FIELDS(MC_STEP_DUMP)
#undef MC_STEP_DUMP
    return n;
}
int ma_mc_step_sizeof() { return (int)sizeof(McStep); }
// the field names in declaration order, each followed by a comma
const char* ma_mc_step_field_names() {
#define MC_STEP_NAME(type, name) #name ","
    return MC_STEP_FIELDS(MC_STEP_NAME);
#undef MC_STEP_NAME
}

int ma_bincount(uintptr_t stream, uintptr_t x, ll N, ll bins, uintptr_t out) {
    hipStream_t s = (hipStream_t)stream;
    if (bins * (ll)sizeof(unsigned int) <= 64 * 1024) {
        k_bincount_lds<<<grid_for(N, 256), 256, bins * sizeof(unsigned int), s>>>(
            (const ll*)x, N, bins, (unsigned long long*)out);
    } else {
        k_bincount_global<<<grid_for(N, 256), 256, 0, s>>>((const ll*)x, N, bins,
                                                           (unsigned long long*)out);
    }
    return (int)hipGetLastError();
}

int ma_binary_stat(uintptr_t stream, uintptr_t preds, int dtype, uintptr_t target, ll N,
                   float threshold, ll ignore_index, int has_ignore, uintptr_t out,
                   uintptr_t outside_flag) {
    hipStream_t s = (hipStream_t)stream;
    LAUNCH_BY_DTYPE(dtype, k_binary_stat, grid_for(N, 256), 256, 0, s, (const DT*)preds,
                    (const ll*)target, N, threshold, ignore_index, has_ignore,
                    (unsigned long long*)out, (unsigned int*)outside_flag);
    return (int)hipGetLastError();
}

int ma_multilabel_stat(uintptr_t stream, uintptr_t preds, int dtype, uintptr_t target, ll N, ll L,
                       float threshold, ll ignore_index, int has_ignore, uintptr_t out,
                       uintptr_t outside_flag) {
    hipStream_t s = (hipStream_t)stream;
    const int use_lds = L <= 512;  // 8L uint counters, <=16 KB LDS
    const size_t shmem = use_lds ? (size_t)(8 * L) * sizeof(unsigned int) : 0;
    int grid = grid_for(N * L, 256);
    if (grid > 4096) grid = 4096;
    LAUNCH_BY_DTYPE(dtype, k_multilabel_stat, grid, 256, shmem, s, (const DT*)preds,
                    (const ll*)target, N, L, threshold, ignore_index, has_ignore,
                    (unsigned long long*)out, (unsigned int*)outside_flag, use_lds);
    return (int)hipGetLastError();
}

int ma_binary_curve_hist(uintptr_t stream, uintptr_t preds, int dtype, uintptr_t target, ll N,
                         uintptr_t thresholds, int T, ll ignore_index, int has_ignore,
                         int uniform, float t0, float inv_step, int norm_sigmoid, uintptr_t flag,
                         uintptr_t hist) {
    hipStream_t s = (hipStream_t)stream;
    size_t shmem = (size_t)(T + 1) * 2 * sizeof(unsigned int) + (size_t)T * sizeof(float);
    if (shmem > 160 * 1024) return -100;  // thresholds too large for LDS path
    if (norm_sigmoid && flag)
        LAUNCH_BY_DTYPE(dtype, k_range_flag, grid_for(N, 256), 256, 0, s, (const DT*)preds, N,
                        (const ll*)target, ignore_index, has_ignore, (unsigned int*)flag);
    LAUNCH_BY_DTYPE(dtype, k_binary_curve_hist, grid_for(N, 256), 256, shmem, s, (const DT*)preds,
                    (const ll*)target, N, (const float*)thresholds, T, ignore_index, has_ignore,
                    uniform, t0, inv_step, norm_sigmoid, (const unsigned int*)flag,
                    (unsigned long long*)hist);
    return (int)hipGetLastError();
}

int ma_multiclass_curve_hist(uintptr_t stream, uintptr_t probs, int dtype, uintptr_t target, ll B,
                             ll C, uintptr_t thresholds, int T, ll ignore_index, int has_ignore,
                             int mode, int uniform, float t0, float inv_step, int norm_kind,
                             uintptr_t flag, uintptr_t rowmax, uintptr_t rowinv, int variant,
                             int c_chunk_override, int stats_ready, uintptr_t hist) {
    hipStream_t s = (hipStream_t)stream;
    size_t shmem = (size_t)T * sizeof(float);
    if (shmem > 160 * 1024) return -100;
    if (norm_kind == 1 && flag && !stats_ready) {
        // softmax stats (one fused pass also sets the out-of-range flag).
        // Fewer blocks -> each wave loops several rows -> more loads in
        // flight per lane (the kernel is latency-bound at 2 vec-loads/lane).
        static int rows_div = 0;
        if (rows_div == 0) {
            const char* e = getenv("MA_ROWSTATS_DIV");
            rows_div = e ? atoi(e) : 16;
            if (rows_div < 4) rows_div = 4;
        }
        int grid = grid_for(B, rows_div);
        LAUNCH_BY_DTYPE(dtype, k_mc_rowstats, grid, 256, 0, s, (const DT*)probs,
                        (const ll*)target, B, C, ignore_index, has_ignore && mode == 0,
                        (unsigned int*)flag, (float*)rowmax, (float*)rowinv);
    } else if (norm_kind == 2 && flag) {
        LAUNCH_BY_DTYPE(dtype, k_range_flag, grid_for(B * C, 256), 256, 0, s, (const DT*)probs,
                        B * C, (const ll*)nullptr, 0, 0, (unsigned int*)flag);
    }
    // LDS-privatized variant when the per-block histogram fits comfortably
    // the kernel maps 32 threads to the classes of a chunk: a wider chunk would
    // leave classes 32.. of every chunk unread, so an override above 32 is clamped
    const int lds_c_chunk = c_chunk_override > 0 ? (c_chunk_override < 32 ? c_chunk_override : 32) : 32;
    const size_t lds_bytes = (size_t)lds_c_chunk * (T + 1) * 2 * sizeof(unsigned int)
                             + (size_t)T * sizeof(float);
    // measured (tools/curve_sweep.py, B=8192 C=1000 T=200): ballot-merge with a
    // small class chunk (oversubscribed grid) beats the LDS variant; LDS stays
    // available behind the env knob for other shapes
    const int want_lds = variant == 1;
    if (want_lds && lds_bytes <= 160 * 1024) {
        ll c_chunks_l = (C + lds_c_chunk - 1) / lds_c_chunk;
        ll row_chunks_l = 1536 / (c_chunks_l > 0 ? c_chunks_l : 1);
        if (row_chunks_l < 1) row_chunks_l = 1;
        ll max_rc = (B + 255) / 256;
        if (row_chunks_l > max_rc) row_chunks_l = max_rc;
        int rows_per_block = (int)((B + row_chunks_l - 1) / row_chunks_l);
        dim3 gridl((unsigned)c_chunks_l, (unsigned)row_chunks_l);
        LAUNCH_BY_DTYPE(dtype, k_multiclass_curve_hist_lds, gridl, 256, lds_bytes, s,
                        (const DT*)probs, (const ll*)target, B, C, (const float*)thresholds, T,
                        ignore_index, has_ignore, mode, uniform, t0, inv_step, lds_c_chunk,
                        rows_per_block, norm_kind, (const unsigned int*)flag,
                        (const float*)rowmax, (const float*)rowinv, (unsigned long long*)hist);
        return (int)hipGetLastError();
    }
    ll row_chunks = (B + 255) / 256;
    // small class chunks oversubscribe the grid (latency hiding beats the
    // per-wave reuse of staged thresholds): sweep plateaus at ~4 for the
    // bench shape; halve further only if the grid is still tiny
    int c_chunk = c_chunk_override > 0 ? c_chunk_override : 4;
    while (c_chunk_override <= 0 && c_chunk > 1 && ((C + c_chunk - 1) / c_chunk) * row_chunks < 4096) c_chunk /= 2;
    ll c_chunks = (C + c_chunk - 1) / c_chunk;
    if (row_chunks > 65535 || c_chunks > 2147483647LL) return -101;
    dim3 grid((unsigned)c_chunks, (unsigned)row_chunks);
    LAUNCH_BY_DTYPE(dtype, k_multiclass_curve_hist, grid, 256, shmem, s, (const DT*)probs,
                    (const ll*)target, B, C, (const float*)thresholds, T, ignore_index, has_ignore,
                    mode, uniform, t0, inv_step, c_chunk, norm_kind, (const unsigned int*)flag,
                    (const float*)rowmax, (const float*)rowinv, (unsigned long long*)hist);
    return (int)hipGetLastError();
}

// Complete a (C, T+1, 2) histogram in pending-b0 format in place
// (k_curve_resolve_pending). pending = [P: C][R: C] u64, the head of the
// one-pass curve scratch; 0 = the histogram owes nothing: no launch.
int ma_curve_resolve_pending(uintptr_t stream, uintptr_t hist, ll C, int T, uintptr_t thresholds,
                             uintptr_t pending) {
    if (!pending) return 0;
    if (!hist || !thresholds || C <= 0 || T < 1) return -103;
    unsigned long long* pr = (unsigned long long*)pending;
    k_curve_resolve_pending<<<(int)((C + 3) / 4), 256, 0, (hipStream_t)stream>>>(
        (unsigned long long*)hist, C, T, (const float*)thresholds, pr, pr + C);
    return (int)hipGetLastError();
}

// pending / thresholds: see ma_curve_resolve_pending, which then runs in front
// of the suffix kernel (both 0 for a histogram that owes nothing)
int ma_curve_suffix(uintptr_t stream, uintptr_t hist, ll outer, int T, int transposed,
                    int zero_hist, uintptr_t epoch_buf, uintptr_t confmat, uintptr_t pending,
                    uintptr_t thresholds) {
    hipStream_t s = (hipStream_t)stream;
    if (pending) {
        const int rc = ma_curve_resolve_pending(stream, hist, outer, T, thresholds, pending);
        if (rc != 0) return rc;
    }
    if (transposed) {
        static int ctile_sel = 0;
        if (ctile_sel == 0) {
            const char* e = getenv("MA_SUFFIX_CTILE");
            ctile_sel = e ? atoi(e) : 4;  // one wave per class in the scan phase
        }
        const int CT = ctile_sel;
        size_t shmem_t = (size_t)2 * CT * (T + 1) * 2 * sizeof(unsigned long long);
        if (CT >= 2 && shmem_t <= 160 * 1024) {
            int grid = (int)((outer + CT - 1) / CT);
            if (CT == 2)
                k_curve_suffix_tiled<2><<<grid, 256, shmem_t, s>>>(
                    (unsigned long long*)hist, T, outer, zero_hist, (unsigned int*)epoch_buf, (ll*)confmat);
            else if (CT == 4)
                k_curve_suffix_tiled<4><<<grid, 256, shmem_t, s>>>(
                    (unsigned long long*)hist, T, outer, zero_hist, (unsigned int*)epoch_buf, (ll*)confmat);
            else
                k_curve_suffix_tiled<8><<<grid, 256, shmem_t, s>>>(
                    (unsigned long long*)hist, T, outer, zero_hist, (unsigned int*)epoch_buf, (ll*)confmat);
            return (int)hipGetLastError();
        }
    }
    // k_curve_suffix also holds two static __shared__ u64 totals
    size_t shmem = (size_t)(T + 1) * 2 * sizeof(unsigned long long);
    if (shmem + 2 * sizeof(unsigned long long) > 160 * 1024) return -100;
    k_curve_suffix<<<(int)outer, 256, shmem, s>>>((unsigned long long*)hist, T, outer, transposed,
                                                  zero_hist, (unsigned int*)epoch_buf,
                                                  (ll*)confmat);
    return (int)hipGetLastError();
}

// close a curve update's device epoch WITHOUT the suffix pass: used by the
// lazy-confmat path, where histograms accumulate across updates and the
// suffix/confmat materialization is deferred to compute()/state access.
int ma_linear_stat_multi(uintptr_t stream, uintptr_t tp, uintptr_t fp, uintptr_t tn,
                         uintptr_t fn, ll C, int n_formulas, uintptr_t params, uintptr_t outs) {
    hipStream_t s = (hipStream_t)stream;
    k_linear_stat_multi<<<n_formulas, 256, 0, s>>>((const ll*)tp, (const ll*)fp, (const ll*)tn,
                                                   (const ll*)fn, C, (const float*)params,
                                                   (float*)outs);
    return (int)hipGetLastError();
}

// phase A of the confmat scalars alone (also launched by the collection
// compute plan, mc_compute.hip): row sums, column sums, diagonal into the
// pre-zeroed 3C u64 scratch [tk | pk | diag]
int ma_confmat_moments(uintptr_t stream, uintptr_t cm, ll C, uintptr_t scratch /* 3C u64 */) {
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* tk = (unsigned long long*)scratch;
    unsigned long long* pk = tk + C;
    unsigned long long* diag = pk + C;
    const int gx = (int)((C + 255) / 256);
    // enough row tiles to fill the chip (>=1024 blocks), bounded by C
    ll row_tiles = (1024 + gx - 1) / gx;
    if (row_tiles > C) row_tiles = C;
    const ll rows_per_block = (C + row_tiles - 1) / row_tiles;
    row_tiles = (C + rows_per_block - 1) / rows_per_block;
    dim3 grid((unsigned)gx, (unsigned)row_tiles);
    k_confmat_moments<<<grid, 256, 0, s>>>((const ll*)cm, C, rows_per_block, tk, pk, diag);
    return (int)hipGetLastError();
}

int ma_confmat_scalars(uintptr_t stream, uintptr_t cm, ll C, uintptr_t scratch /* 3C u64 */,
                       float zero_division, uintptr_t out /* 3 f32 */) {
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* tk = (unsigned long long*)scratch;
    unsigned long long* pk = tk + C;
    unsigned long long* diag = pk + C;
    const int rc = ma_confmat_moments(stream, cm, C, scratch);
    if (rc != 0) return rc;
    k_confmat_scalars<<<1, 256, 0, s>>>(pk, diag, tk, C, zero_division, (float*)out);
    return (int)hipGetLastError();
}

int ma_curve_epoch_bump(uintptr_t stream, uintptr_t epoch_buf) {
    hipStream_t s = (hipStream_t)stream;
    k_epoch_bump<<<1, 1, 0, s>>>((unsigned int*)epoch_buf);
    return (int)hipGetLastError();
}

int ma_curve_auc_from_confmat(uintptr_t stream, uintptr_t confmat, int T, ll C, int mode,
                               uintptr_t out, uintptr_t weights) {
    hipStream_t s = (hipStream_t)stream;
    k_curve_auc_from_confmat<<<(unsigned)C, 256, 0, s>>>((const ll*)confmat, T, C, mode,
                                                         (float*)out, (float*)weights);
    return (int)hipGetLastError();
}

int ma_err_reduce(uintptr_t stream, uintptr_t x, uintptr_t y, int dtype, ll N, int op, double eps,
                  uintptr_t partials, int num_blocks, int n_out, uintptr_t out) {
    hipStream_t s = (hipStream_t)stream;
    LAUNCH_BY_DTYPE(dtype, k_err_reduce_partial, num_blocks, 256, 0, s, (const DT*)x,
                    (const DT*)y, N, op, eps, (double*)partials, n_out);
    k_err_reduce_final<<<1, 64, 0, s>>>((const double*)partials, num_blocks, n_out, (double*)out);
    return (int)hipGetLastError();
}

int ma_box_iou(uintptr_t stream, uintptr_t b1, ll N, uintptr_t b2, ll M, int variant,
               uintptr_t out) {
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)((M + 255) / 256), (unsigned)((N + 63) / 64));
    k_box_iou<<<grid, 256, 0, s>>>((const float*)b1, N, (const float*)b2, M, variant, (float*)out);
    return (int)hipGetLastError();
}

}  // extern "C"
