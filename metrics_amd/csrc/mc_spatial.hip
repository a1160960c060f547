// Fused update of a multiclass collection fed (N, C, *spatial) predictions
// (gfx950): ONE pass over the contiguous (N, C, S) logits / probabilities
// (S = product of the spatial dims) and the (N, S) int64 targets feeds the
// stat-scores, confusion-matrix, exact-match and threshold-curve group leaders.
// Two launches per step, k_mc_spatial_step and k_mc_spatial_tail; record:
// mc_spatial.h. Nothing is transposed: the stand-alone paths first write a
// (N*S, C) copy of the predictions, this one reads them where they lie.
//
// SEMANTICS (taken from the stand-alone paths, the oracles of the tests). A
// PIXEL is one (n, s); its COLUMN the C values preds[n, :, s]; its row index,
// for the row statistics, n*S + s.
//  - argmax: the fold of k_mc_stat_logits_tiny, `f > best` from best = -inf,
//    index 0: largest non-NaN value, lowest index on a tie, 0 when every
//    element is NaN (docs/PARITY.md);
//  - online softmax: the recurrence of k_mc_stat_logits_tiny over the classes
//    in index order, rowmax = m, rowinv = 1 / s;
//  - a pixel is COUNTED iff its target is not ignored and 0 <= t < C
//    (count_row), and KEPT iff its target is not ignored;
//  - exact match: a kept pixel with argmax != t, an out-of-range target
//    included, marks its sample; an ignored pixel never does;
//  - curve: softmax iff any kept pixel holds an element outside [0,1] (NaN is
//    not outside, +-inf is), a batch-global decision; every kept pixel is
//    binned for every class c with label t == c, p = x or
//    __expf(x - rowmax) * rowinv, through bucket_of / bucket_of_uniform.
//
// LAYOUT. Consecutive pixels of one class are consecutive in memory, so a lane
// OWNS V consecutive pixels of one image (V = 8 bf16 or 4 fp32: one 16-byte
// load per class) and walks c = 0 .. C-1 with stride S. The 64 lanes of a wave
// read 1 KiB of consecutive addresses per class, and a pixel's fold needs no
// cross-lane step. The vector path needs S % V == 0 and a 16-byte aligned
// base; otherwise a lane owns one pixel (sp_tile<.., 1>) and does the same
// work through the same fold and binning functions. A wave TILE is 64 * V (or
// 64) pixels of one image; tiles never straddle two images (the last tile of
// an image is partly empty), and the waves of the grid stride over the tiles.
//
// One pass over a tile yields
//  - the counts. While the (C, C) matrix fits into LDS next to the rest it is
//    the only thing counted per pixel, one LDS atomic; the block derives
//    tp / fp / fn [3][C] from it at its end (diagonal, column and row sums).
//    Beyond that tp / fp / fn are counted in LDS and the matrix with global
//    atomics onto the state, as the tiny kernel does. Either way the block
//    flushes [3][C] once, one global atomic per non-zero word, into the count
//    scratch, and a matrix kept in LDS onto the confmat state;
//  - the sample's mismatch word: one atomicOr per wave tile at most;
//  - rowmax / rowinv of every pixel, stored in row order;
//  - CURVE, under the certainty rule of the other steps: a wave that has seen
//    a kept pixel with an element outside [0,1], in this tile or an earlier
//    one, knows the decision is "softmax" and bins the tile now, into the
//    block's private LDS histogram [C][T+1][2] u32. The column is read a
//    second time for that (see docs/ARCHITECTURE.md for where that read is
//    expected to hit). A tile with kept pixels seen before its wave is certain
//    is DEFERRED: one flag byte, nothing binned. The block flushes its
//    histogram once, one global atomic per non-zero bin, into the leader's
//    lazy (C, T+1, 2) histogram.
// The block ends with one record {valid, outside, deferred}; no atomic touches
// a single global flag word.
//
// k_mc_spatial_tail runs behind it. Every block reduces the `grid` records.
// Block 0: one thread per class applies tp/fp/fn and tn += valid - the rest
// and zeroes the scratch; thread 0 adds total += N and closes the curve epoch,
// E[1] += 1 (E[0] is never written, so E[0] <= E[1] keeps holding for the
// stand-alone producers). The first blocks stride the N samples: correct +=
// samples whose mismatch word is 0, the word zeroed (one atomic per block onto
// `correct`). If any tile was deferred, the waves of all blocks stride the
// tile flags; a flagged tile is binned under the batch-global decision with
// the same function sp_bin and the stored row statistics, into a block-private
// LDS histogram flushed like the step's, and its flag is cleared.
//
// There is no spin, ticket or grid-wide wait. Nothing one block of a launch
// writes is read by another block of that launch; blocks only meet in atomic
// adds / ORs onto histogram, state, scratch and mismatch words. Every scratch
// slot, mismatch word and tile flag is read and zeroed by the one tail thread
// (wave) that owns it; records are never zeroed, the tail reads only `grid`.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "curve_common.h"
#include "mc_spatial.h"
#include "row_fold.h"

typedef long long ll;
typedef unsigned long long ull;

#define SP_BLOCK 1024     // threads of both kernels: 16 waves, one block per CU at the LDS gate
#define SP_WAVES (SP_BLOCK / 64)
#define SP_GRID_MAX 256   // blocks of k_mc_spatial_step = records; one per CU
#define SP_TAIL_GRID 256
#define SP_ROW_BLOCKS 64  // tail blocks that count samples: atomics onto `correct`
#define SP_MAX_C 256      // class cap: the LDS count block [3][C] u32
// LDS of a workgroup on gfx950, and what the kernels keep statically (block
// record and reduction words, rounded up); MC_SPATIAL_LDS_* in ops/_hip.py
// are the same two numbers
#define SP_LDS_BYTES (160 * 1024)
#define SP_LDS_STATIC 128

// everything both kernels need, by value
struct SpArgs {
    const void* preds;
    const ll* target;
    ll N, S, tpi, n_tiles;  // tpi = tiles per image
    int C, has_ignore, vec, cm_lds, thr_lds, grid;
    ll ignore_index;
    ull* counts;
    unsigned int* records;
    ll *tp, *fp, *tn, *fn, *confmat, *correct, *total;
    unsigned int* rowbad;
    int T, uniform;
    float t0, inv_step;
    const float* thresholds;
    ull* hist;
    unsigned int* E;
    float *rowmax, *rowinv;
    unsigned char* flags;
};

// one pixel's fold state: argmax and online softmax, classes in index order
struct SpPix {
    float best;
    int idx;
    float m, s;
    unsigned int out;
};

__device__ __forceinline__ void sp_fold(SpPix& p, float f, int c) {
    if (f > p.best) { p.best = f; p.idx = c; }
    p.out |= (f < 0.0f || f > 1.0f) ? 1u : 0u;
    if (f > p.m) { p.s = p.s * __expf(p.m - f) + 1.0f; p.m = f; }
    else { p.s += __expf(f - p.m); }
}

// h[key] += 1 for every lane with key >= 0; all 64 lanes call. The lanes that
// share the key of the first such lane go in one atomic carrying their count
// (a dominant class or bucket would otherwise serialise the wave on one LDS
// word), the others add on their own.
__device__ __forceinline__ void sp_lds_count(unsigned int* __restrict__ h, int key, int lane) {
    const ull act = __ballot(key >= 0);
    if (act == 0ULL) return;
    const int lead = __ffsll(act) - 1;
    const int k0 = __shfl(key, lead);
    const ull same = __ballot(key == k0);
    if (lane == lead) atomicAdd(&h[k0], (unsigned int)__popcll(same));
    else if (key >= 0 && key != k0) atomicAdd(&h[key], 1u);
}

// K consecutive elements of class c of a lane's pixels; col = &preds[n, 0, s0]
template <typename T_, int K>
__device__ __forceinline__ void sp_load(const T_* __restrict__ col, ll off, float (&f)[K]) {
    if constexpr (K == 1) f[0] = ld_f32(col, off);
    else unpack16<T_>(*reinterpret_cast<const uint4*>(col + off), f);
}

// Bin the kept pixels of one tile (bit k of `live`: pixel k of this lane) for
// every class into the histogram h [C][T+1][2] u32 in LDS. All 64 lanes call;
// a lane without data has in = false. softmax: p = __expf(x - rm) * ri.
template <typename T_, int K>
__device__ __forceinline__ void sp_bin(
    const T_* __restrict__ col, ll S, int C, bool in, const ll (&t)[K], unsigned int live,
    bool softmax, const float (&rm)[K], const float (&ri)[K], unsigned int* __restrict__ h,
    const float* __restrict__ sthr, int T, int uniform, float t0, float inv_step, int lane) {
    const int bins = (T + 1) * 2;
    for (int c = 0; c < C; c++) {
        float f[K];
#pragma unroll
        for (int k = 0; k < K; k++) f[k] = 0.0f;
        if (in && live) sp_load<T_, K>(col, (ll)c * S, f);
#pragma unroll
        for (int k = 0; k < K; k++) {
            int key = -1;
            if ((live >> k) & 1u) {
                const float p = softmax ? __expf(f[k] - rm[k]) * ri[k] : f[k];
                const int j = uniform ? bucket_of_uniform(p, sthr, T, t0, inv_step) : bucket_of(p, sthr, T);
                key = c * bins + j * 2 + (t[k] == (ll)c ? 1 : 0);
            }
            sp_lds_count(h, key, lane);
        }
    }
}

// where a lane's K pixels of `tile` lie
struct SpPos {
    ll n, s0, row0;
    bool in;
};
template <int K>
__device__ __forceinline__ SpPos sp_pos(const SpArgs& a, ll tile, int lane) {
    SpPos p;
    p.n = tile / a.tpi;
    p.s0 = (tile - p.n * a.tpi) * (64 * K) + (ll)lane * K;
    p.in = p.s0 < a.S;  // K > 1: S % K == 0, so all K pixels or none
    p.row0 = p.n * a.S + (p.in ? p.s0 : 0);
    return p;
}

// what a wave carries through its tiles
struct SpWave {
    unsigned int valid;
    bool certain, any_out, any_def;  // wave-uniform
};

template <typename T_, bool CURVE, int K>
__device__ __forceinline__ void sp_tile(
    const SpArgs& a, ll tile, int lane, unsigned int* __restrict__ s_cnt, unsigned int* __restrict__ s_cm,
    unsigned int* __restrict__ s_hist, const float* __restrict__ sthr, SpWave& w) {
    const int C = a.C;
    const SpPos pos = sp_pos<K>(a, tile, lane);
    const T_* col = (const T_*)a.preds + pos.n * (ll)C * a.S + (pos.in ? pos.s0 : 0);
    ll t[K];
    SpPix px[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        t[k] = pos.in ? a.target[pos.row0 + k] : 0;
        px[k] = {-INFINITY, 0, -3.4e38f, 0.0f, 0u};
    }
    if (pos.in) {
#pragma unroll 4
        for (int c = 0; c < C; c++) {
            float f[K];
            sp_load<T_, K>(col, (ll)c * a.S, f);
#pragma unroll
            for (int k = 0; k < K; k++) sp_fold(px[k], f[k], c);
        }
    }
    unsigned int live = 0;
    bool kept_out = false, bad = false;
    float rm[K], ri[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const bool lv = pos.in && !(a.has_ignore && t[k] == a.ignore_index);
        const bool ok = lv && t[k] >= 0 && t[k] < (ll)C;
        const int tt = ok ? (int)t[k] : 0, p = px[k].idx;
        live |= lv ? (1u << k) : 0u;
        kept_out = kept_out || (lv && px[k].out != 0u);
        bad = bad || (lv && !(ok && p == tt));
        w.valid += ok ? 1u : 0u;
        if (s_cm) {
            sp_lds_count(s_cm, ok ? tt * C + p : -1, lane);
        } else {
            sp_lds_count(s_cnt, ok && p == tt ? tt : -1, lane);
            sp_lds_count(s_cnt, ok && p != tt ? C + p : -1, lane);
            sp_lds_count(s_cnt, ok && p != tt ? 2 * C + tt : -1, lane);
            if (a.confmat && ok) atomicAdd((ull*)&a.confmat[tt * C + p], 1ULL);
        }
        rm[k] = px[k].m;
        ri[k] = 1.0f / px[k].s;
        if constexpr (CURVE) {
            if (pos.in) {
                a.rowmax[pos.row0 + k] = rm[k];
                a.rowinv[pos.row0 + k] = ri[k];
            }
        }
    }
    if (a.rowbad && __ballot(bad) != 0ULL && lane == 0) atomicOr(&a.rowbad[pos.n], 1u);
    if constexpr (CURVE) {
        const bool tile_out = __ballot(kept_out) != 0ULL;
        w.any_out = w.any_out || tile_out;
        w.certain = w.certain || tile_out;
        if (__ballot(live != 0u) != 0ULL) {
            if (w.certain) {
                sp_bin<T_, K>(col, a.S, C, pos.in, t, live, true, rm, ri, s_hist, sthr, a.T, a.uniform, a.t0,
                              a.inv_step, lane);
            } else {
                if (lane == 0) a.flags[tile] = 1;
                w.any_def = true;
            }
        }
    }
}

// dynamic LDS of both kernels, u32 words: [3*C counts][C*C matrix, cm_lds]
// [C*(T+1)*2 histogram, CURVE][T thresholds, thr_lds]
template <typename T_, bool CURVE>
__global__ void __launch_bounds__(SP_BLOCK) k_mc_spatial_step(const SpArgs a) {
    extern __shared__ unsigned int s_dyn[];
    __shared__ unsigned int s_rec[3];  // valid, outside, deferred

    constexpr int V = 16 / sizeof(T_);
    const int C = a.C;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int hist_words = CURVE ? C * (a.T + 1) * 2 : 0;
    unsigned int* s_cnt = s_dyn;
    unsigned int* s_cm = a.cm_lds ? s_dyn + 3 * C : nullptr;
    unsigned int* s_hist = s_dyn + 3 * C + (a.cm_lds ? C * C : 0);
    float* s_thr = (float*)(s_hist + hist_words);

    const int zero_words = 3 * C + (a.cm_lds ? C * C : 0) + hist_words;
    for (int i = threadIdx.x; i < zero_words; i += blockDim.x) s_dyn[i] = 0;
    if constexpr (CURVE) {
        if (a.thr_lds)
            for (int i = threadIdx.x; i < a.T; i += blockDim.x) s_thr[i] = a.thresholds[i];
    }
    if (threadIdx.x < 3) s_rec[threadIdx.x] = 0;
    __syncthreads();

    SpWave w = {0u, false, false, false};
    const ll stride = (ll)gridDim.x * SP_WAVES;
    for (ll tile = (ll)blockIdx.x * SP_WAVES + wave; tile < a.n_tiles; tile += stride) {
        // the branches differ only in the address space of the thresholds
        if (a.vec) {
            if (a.thr_lds) sp_tile<T_, CURVE, V>(a, tile, lane, s_cnt, s_cm, s_hist, s_thr, w);
            else sp_tile<T_, CURVE, V>(a, tile, lane, s_cnt, s_cm, s_hist, a.thresholds, w);
        } else {
            if (a.thr_lds) sp_tile<T_, CURVE, 1>(a, tile, lane, s_cnt, s_cm, s_hist, s_thr, w);
            else sp_tile<T_, CURVE, 1>(a, tile, lane, s_cnt, s_cm, s_hist, a.thresholds, w);
        }
    }

    const unsigned int wv = wave_sum_u32(w.valid);
    if (lane == 0) {
        if (wv) atomicAdd(&s_rec[0], wv);
        if (w.any_out) atomicOr(&s_rec[1], 1u);
        if (w.any_def) atomicOr(&s_rec[2], 1u);
    }
    __syncthreads();
    if (s_cm) {
        // tp = diagonal, fp = column sum - tp, fn = row sum - tp
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            unsigned int rs = 0, cs = 0;
            for (int j = 0; j < C; j++) { rs += s_cm[c * C + j]; cs += s_cm[j * C + c]; }
            const unsigned int d = s_cm[c * C + c];
            s_cnt[c] = d;
            s_cnt[C + c] = cs - d;
            s_cnt[2 * C + c] = rs - d;
        }
        __syncthreads();
        if (a.confmat) {
            for (int i = threadIdx.x; i < C * C; i += blockDim.x) {
                const unsigned int v = s_cm[i];
                if (v) atomicAdd((ull*)&a.confmat[i], (ull)v);
            }
        }
    }
    if (a.tp) {
        for (int i = threadIdx.x; i < 3 * C; i += blockDim.x) {
            const unsigned int v = s_cnt[i];
            if (v) atomicAdd(&a.counts[i], (ull)v);
        }
    }
    if constexpr (CURVE) {
        for (int i = threadIdx.x; i < hist_words; i += blockDim.x) {
            const unsigned int v = s_hist[i];
            if (v) atomicAdd(&a.hist[i], (ull)v);
        }
    }
    if (threadIdx.x < 3) a.records[3 * blockIdx.x + threadIdx.x] = s_rec[threadIdx.x];
}

// one deferred tile in the tail: targets and row statistics are read back
template <typename T_, int K>
__device__ __forceinline__ void sp_tail_tile(const SpArgs& a, ll tile, int lane, bool softmax,
                                             unsigned int* __restrict__ s_hist,
                                             const float* __restrict__ sthr) {
    const SpPos pos = sp_pos<K>(a, tile, lane);
    const T_* col = (const T_*)a.preds + pos.n * (ll)a.C * a.S + (pos.in ? pos.s0 : 0);
    ll t[K];
    float rm[K], ri[K];
    unsigned int live = 0;
#pragma unroll
    for (int k = 0; k < K; k++) {
        t[k] = pos.in ? a.target[pos.row0 + k] : 0;
        const bool lv = pos.in && !(a.has_ignore && t[k] == a.ignore_index);
        live |= lv ? (1u << k) : 0u;
        rm[k] = (softmax && pos.in) ? a.rowmax[pos.row0 + k] : 0.0f;
        ri[k] = (softmax && pos.in) ? a.rowinv[pos.row0 + k] : 0.0f;
    }
    sp_bin<T_, K>(col, a.S, a.C, pos.in, t, live, softmax, rm, ri, s_hist, sthr, a.T, a.uniform, a.t0,
                  a.inv_step, lane);
}

// dynamic LDS (CURVE): [C*(T+1)*2 histogram][T thresholds, thr_lds]
template <typename T_, bool CURVE>
__global__ void __launch_bounds__(SP_BLOCK) k_mc_spatial_tail(const SpArgs a, int row_blocks) {
    extern __shared__ unsigned int s_dyn[];
    __shared__ ull s_valid;
    __shared__ unsigned int s_fl[2];  // outside, deferred
    __shared__ unsigned int s_good;

    constexpr int V = 16 / sizeof(T_);
    const int C = a.C;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;

    // ---- (a) the batch: valid pixels and the two decisions ----
    if (threadIdx.x == 0) { s_valid = 0; s_fl[0] = 0; s_fl[1] = 0; s_good = 0; }
    __syncthreads();
    for (int i = threadIdx.x; i < a.grid; i += blockDim.x) {
        const unsigned int v = a.records[3 * i], o = a.records[3 * i + 1], d = a.records[3 * i + 2];
        if (v) atomicAdd(&s_valid, (ull)v);
        if (o) atomicOr(&s_fl[0], 1u);
        if (d) atomicOr(&s_fl[1], 1u);
    }
    __syncthreads();
    const ll valid = (ll)s_valid;
    const bool outside = s_fl[0] != 0u, deferred = s_fl[1] != 0u;

    // ---- (b) block 0: the stat states, total, the epoch ----
    if (blockIdx.x == 0) {
        if (a.tp)
            for (int c = threadIdx.x; c < C; c += blockDim.x)
                apply_stat_class(a.counts, C, c, valid, a.tp, a.fp, a.tn, a.fn);
        if (threadIdx.x == 0) {
            if (a.total) a.total[0] += a.N;
            if (CURVE && a.E) a.E[1] += 1u;
        }
    }

    // ---- (c) exact match: samples without a mismatch ----
    if (a.rowbad && (int)blockIdx.x < row_blocks) {
        unsigned int good = 0;
        for (ll r = (ll)blockIdx.x * blockDim.x + threadIdx.x; r < a.N; r += (ll)row_blocks * blockDim.x) {
            const unsigned int wd = a.rowbad[r];
            if (wd) a.rowbad[r] = 0;
            good += wd ? 0u : 1u;
        }
        good = wave_sum_u32(good);
        if (lane == 0 && good) atomicAdd(&s_good, good);
        __syncthreads();
        if (threadIdx.x == 0 && s_good) atomicAdd((ull*)a.correct, (ull)s_good);
    }

    // ---- (d) the deferred tiles, under the batch-global decision ----
    if constexpr (CURVE) {
        if (!deferred) return;  // block-uniform
        const int hist_words = C * (a.T + 1) * 2;
        unsigned int* s_hist = s_dyn;
        float* s_thr = (float*)(s_hist + hist_words);
        for (int i = threadIdx.x; i < hist_words; i += blockDim.x) s_hist[i] = 0;
        if (a.thr_lds)
            for (int i = threadIdx.x; i < a.T; i += blockDim.x) s_thr[i] = a.thresholds[i];
        __syncthreads();
        const ll stride = (ll)gridDim.x * SP_WAVES;
        for (ll tile = (ll)blockIdx.x * SP_WAVES + wave; tile < a.n_tiles; tile += stride) {
            if (a.flags[tile] == 0) continue;  // wave-uniform
            if (a.vec) {
                if (a.thr_lds) sp_tail_tile<T_, V>(a, tile, lane, outside, s_hist, s_thr);
                else sp_tail_tile<T_, V>(a, tile, lane, outside, s_hist, a.thresholds);
            } else {
                if (a.thr_lds) sp_tail_tile<T_, 1>(a, tile, lane, outside, s_hist, s_thr);
                else sp_tail_tile<T_, 1>(a, tile, lane, outside, s_hist, a.thresholds);
            }
            if (lane == 0) a.flags[tile] = 0;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < hist_words; i += blockDim.x) {
            const unsigned int v = s_hist[i];
            if (v) atomicAdd(&a.hist[i], (ull)v);
        }
    }
}

// ---- host: the layout of a step, a function of the shape, dtype, T and base ----
struct SpLayout {
    int V, vec, tile_px, grid, tgrid, row_blocks, cm_lds, thr_lds;
    ll tpi, n_tiles, flag_cap;
    size_t lds, tail_lds;
};

// false: shape not covered. T = 0: no curve leader. misalign = bytes of the
// preds address past a 16-byte boundary.
static bool sp_layout(ll N, ll C, ll S, int dtype, ll T, unsigned int misalign, SpLayout* o) {
    if (dtype != 0 && dtype != 1) return false;
    if (N < 0 || S < 0 || C < 1 || C > SP_MAX_C || T < 0 || T > (1 << 20)) return false;
    if (N > 0 && S > 0 && (S >= (1LL << 31) || N >= (1LL << 31) / S)) return false;  // N*S < 2^31
    const int esize = dtype == 0 ? 4 : 2;
    if (misalign % esize) return false;
    const size_t counts = 12 * (size_t)C, hist = T > 0 ? 8 * (size_t)C * (size_t)(T + 1) : 0;
    // the curve gate: counts + histogram + static (MC_SPATIAL_* in ops/_hip.py)
    if (counts + hist + SP_LDS_STATIC > SP_LDS_BYTES) return false;
    size_t lds = counts + hist;
    o->thr_lds = T > 0 && lds + 4 * (size_t)T + SP_LDS_STATIC <= SP_LDS_BYTES;
    if (o->thr_lds) lds += 4 * (size_t)T;
    o->cm_lds = lds + 4 * (size_t)C * C + SP_LDS_STATIC <= SP_LDS_BYTES;
    if (o->cm_lds) lds += 4 * (size_t)C * C;
    o->lds = lds;
    o->tail_lds = T > 0 ? hist + (o->thr_lds ? 4 * (size_t)T : 0) : 0;
    o->V = 16 / esize;
    o->vec = misalign == 0 && S % o->V == 0;
    o->tile_px = o->vec ? 64 * o->V : 64;
    o->tpi = (S + o->tile_px - 1) / o->tile_px;
    o->n_tiles = N * o->tpi;
    o->flag_cap = N * ((S + 63) / 64);  // the element-per-lane path has the most tiles
    ll grid = (o->n_tiles + SP_WAVES - 1) / SP_WAVES;
    if (grid > SP_GRID_MAX) grid = SP_GRID_MAX;
    o->grid = (int)grid;  // 0: nothing to read, the tail alone
    ll tg = T > 0 ? grid : (N + SP_BLOCK - 1) / SP_BLOCK;
    if (tg > (T > 0 ? SP_TAIL_GRID : SP_ROW_BLOCKS)) tg = T > 0 ? SP_TAIL_GRID : SP_ROW_BLOCKS;
    if (tg < 1) tg = 1;
    o->tgrid = (int)tg;
    o->row_blocks = tg < SP_ROW_BLOCKS ? (int)tg : SP_ROW_BLOCKS;
    return true;
}

template <typename T_, bool CURVE>
static int sp_launch(hipStream_t s, const SpArgs& a, const SpLayout& lay) {
    if (a.grid > 0) {
        k_mc_spatial_step<T_, CURVE><<<a.grid, SP_BLOCK, lay.lds, s>>>(a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    k_mc_spatial_tail<T_, CURVE><<<lay.tgrid, SP_BLOCK, lay.tail_lds, s>>>(a, lay.row_blocks);
    return (int)hipGetLastError();
}

extern "C" {

int ma_mc_spatial_step_sizeof() { return (int)sizeof(McSpatialStep); }
// the field names in declaration order, each followed by a comma
const char* ma_mc_spatial_step_field_names() {
#define MC_SPATIAL_STEP_NAME(type, name) #name ","
    return MC_SPATIAL_STEP_FIELDS(MC_SPATIAL_STEP_NAME);
#undef MC_SPATIAL_STEP_NAME
}

// Host only: what a step over (N, C, S) predictions of `dtype` (0 = f32,
// 1 = bf16) with T thresholds (0: no curve leader) needs, for a 16-byte
// aligned `preds`. out = {pixels per lane of the vector path, 1 if this shape
// takes the vector path, pixels per wave tile, threads per block, blocks of
// k_mc_spatial_step, blocks of k_mc_spatial_tail, dynamic LDS bytes of the
// step, 1 if the (C, C) matrix is kept in LDS, 1 if the thresholds are, wave
// tiles, tile flag bytes to provide (the worst case over both paths), record
// words to provide}. -103: shape not covered.
int ma_mc_spatial_layout(ll N, ll C, ll S, int dtype, int T, ll* out) {
    SpLayout lay;
    if (!sp_layout(N, C, S, dtype, T, 0, &lay)) return -103;
    out[0] = lay.V;
    out[1] = lay.vec;
    out[2] = lay.tile_px;
    out[3] = SP_BLOCK;
    out[4] = lay.grid;
    out[5] = lay.tgrid;
    out[6] = (ll)lay.lds;
    out[7] = lay.cm_lds;
    out[8] = lay.thr_lds;
    out[9] = lay.n_tiles;
    out[10] = lay.flag_cap;
    out[11] = 3 * SP_GRID_MAX;
    return 0;
}

// the class cap and the two numbers of the curve gate, for the loader to hold
// against the Python constants
int ma_mc_spatial_max_classes() { return SP_MAX_C; }
int ma_mc_spatial_lds_bytes() { return SP_LDS_BYTES; }
int ma_mc_spatial_lds_static() { return SP_LDS_STATIC; }

// The whole spatial step on one stream in two launches (N == 0 or S == 0: the
// tail alone). The record is read here, on the host; the kernels get its
// pointers by value. -103 for a shape, dtype, class count or address the
// kernels do not cover, a missing buffer or one too small; nothing is launched
// then.
int ma_mc_spatial_step(uintptr_t stream, const McSpatialStep* st, uintptr_t preds, int dtype /*0=f32 1=bf16*/,
                       uintptr_t target, ll N, ll S) {
    if (dtype != 0 && dtype != 1) return -103;
    if (!st->counts || !st->records) return -103;
    if (N > 0 && S > 0 && (!preds || !target)) return -103;
    if (target % sizeof(ll)) return -103;
    // every group is whole or absent
    if (!st->tp != !st->fp || !st->tp != !st->tn || !st->tp != !st->fn) return -103;
    if (!st->correct != !st->total || !st->correct != !st->rowbad) return -103;
    if (st->rowbad && st->sample_cap < N) return -103;
    const bool curve = st->T > 0;
    if (curve && (!st->thresholds || !st->hist || !st->epoch_buf || !st->rowmax || !st->rowinv || !st->tile_flags))
        return -103;
    SpLayout lay;
    if (!sp_layout(N, st->C, S, dtype, st->T, (unsigned int)(preds & 15), &lay)) return -103;
    if (curve && (st->row_cap < N * S || st->tile_cap < lay.n_tiles)) return -103;
    SpArgs a;
    a.preds = (const void*)preds;
    a.target = (const ll*)target;
    a.N = N; a.S = S; a.tpi = lay.tpi; a.n_tiles = lay.n_tiles;
    a.C = (int)st->C; a.has_ignore = (int)st->has_ignore; a.vec = lay.vec;
    a.cm_lds = lay.cm_lds; a.thr_lds = lay.thr_lds; a.grid = lay.grid;
    a.ignore_index = st->ignore_index;
    a.counts = st->counts; a.records = st->records;
    a.tp = st->tp; a.fp = st->fp; a.tn = st->tn; a.fn = st->fn; a.confmat = st->confmat;
    a.correct = st->correct; a.total = st->total; a.rowbad = st->rowbad;
    a.T = (int)st->T; a.uniform = (int)st->uniform;
    a.t0 = (float)st->t0; a.inv_step = (float)st->inv_step;
    a.thresholds = st->thresholds; a.hist = st->hist; a.E = st->epoch_buf;
    a.rowmax = st->rowmax; a.rowinv = st->rowinv; a.flags = st->tile_flags;
    hipStream_t s = (hipStream_t)stream;
    int rc = 0;
    if (curve) FOR_DTYPE(dtype, rc = sp_launch<DT, true>(s, a, lay));
    else FOR_DTYPE(dtype, rc = sp_launch<DT, false>(s, a, lay));
    return rc;
}

}  // extern "C"
