// Fused update of a binary collection (gfx950): ONE pass over the flat
// logits / probabilities and the flat int64 targets feeds the stat-scores,
// confusion-matrix and threshold-curve group leaders. Two launches per step,
// k_bin_step and k_bin_tail; record: bin_step.h.
//
// SEMANTICS (taken from the stand-alone paths, which a fused collection must
// equal bit for bit). The three groups do NOT share one normalisation
// decision:
//  - stat scores: sigmoid iff ANY element, ignored positions included, lies
//    outside [0,1] (k_binary_stat)                                 -> outside_all
//  - confusion matrix and curve: sigmoid iff any element whose target is NOT
//    ignored lies outside [0,1] (_binary_confusion_matrix_format drops the
//    ignored elements first; k_range_flag with has_ignore)        -> outside_kept
// NaN is not outside, +-inf is (ml_outside_unit). The prediction is x > thr
// without and x > logit(thr) with normalisation (ml_rule.h), an element whose
// target is ignore_index counts in nothing, the label is t == 1. The curve
// bins p = x or 1/(1+expf(-x)) with bucket_of / bucket_of_uniform, as
// k_binary_curve_hist does. Targets outside {0, 1, ignore_index} are outside
// the contract: they count as label 0.
//
// LAYOUT. The input is a flat stream of N elements. A scalar HEAD (the
// elements in front of the first 16-byte boundary of `preds`, at most 7) and a
// scalar TAIL (what is left behind the last whole vector) are taken by the
// first lanes of block 0; the BODY between them is read in 16-byte vectors:
// 8 bf16 or 4 fp32 predictions per load, and 2 int64 targets per load (the
// target vector is only 8-byte aligned in general: a head of odd length, or a
// slice such as buf[1:], shifts it by one element). One UNIT is BIN_EPT = 16
// elements per thread of a block (256, 512 or 1024 threads, by the size of the
// batch: bin_layout), vectors strided over the threads so that the lanes of a
// load read consecutive addresses; blocks grid-stride over the units.
//
// One pass over a unit yields
//  - six counters in registers across all units of the thread: pos, neg among
//    kept elements, and predicted-positive by label under the raw and under the
//    sigmoid cut. They meet once per block in LDS and leave it with one global
//    atomic per non-zero counter into the count scratch [6];
//  - the two outside bits;
//  - DUAL BINNING (curve): the block holds the histogram [T+1][2] u32 twice,
//    under the raw and under the sigmoid interpretation, and every kept
//    element is binned into both. CERTAINTY: once a wave has seen a kept
//    element outside [0,1], in this vector or an earlier one, the decision of
//    the curve is known to be "sigmoid" and the wave stops binning raw; the raw
//    histogram is never chosen for such a batch, so what it lacks does not
//    matter. Logits pay one binning per element, probabilities two; nothing
//    is deferred and nothing is read twice. The block flushes its non-zero
//    bins with global atomics into the per-step curve scratch [2][T+1][2],
//    not into the leader's histogram.
// The block ends with one record byte (outside_all, outside_kept); no atomic
// touches a single global flag word.
//
// k_bin_tail runs behind it. Every block ORs the `grid` record bytes. Thread 0
// of block 0 picks the raw or sigmoid counters by outside_all for tp/fp/tn/fn
// and by outside_kept for confmat = [[tn, fp], [fn, tp]], zeroes the six
// scratch slots and closes the curve epoch, E[1] += 1 (E[0] is never written,
// so E[0] <= E[1] keeps holding for the stand-alone producers). Threads
// striding the (T+1)*2 bins add the scratch histogram chosen by outside_kept
// into the leader's lazy (1, T+1, 2) histogram and zero both scratch copies.
//
// There is no spin, ticket or grid-wide wait. Nothing one block of a launch
// writes is read by another block of that launch; blocks only meet in atomic
// adds onto scratch words. Every scratch word is read and zeroed by the one
// thread that owns it; records are never zeroed, the tail reads only `grid` of
// them.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "bin_step.h"
#include "curve_common.h"
#include "ml_rule.h"
#include "row_fold.h"

typedef long long ll;
typedef unsigned long long ull;

#define BIN_BLOCK_MAX 1024  // threads of k_bin_step: 256, 512 or 1024 (bin_layout)
#define BIN_BLOCK_MIN 256
#define BIN_EPT 16          // elements per thread and unit
#define BIN_THREADS 262144  // threads of a full grid: 4 waves per SIMD of 256 CUs
#define BIN_MIN_UNITS 128    // a wider block needs at least this many units
#define BIN_TAIL_BLOCK 256
#define BIN_GRID_MAX 2048  // record bytes = cap of the k_bin_step grid
#define BIN_TAIL_GRID 32
// LDS of a workgroup on gfx950, and what k_bin_step keeps statically (block
// counters [6] u32 and one word, rounded up); BIN_STEP_MAX_T in ops/_hip.py is
// derived from the same two numbers
#define BIN_LDS_BYTES (160 * 1024)
#define BIN_LDS_STATIC 256
// per-wave histogram copies are used while the block's LDS stays below this,
// so that four blocks still share a CU
#define BIN_LDS_COPIES_MAX (40 * 1024)

// two consecutive targets; 8-byte aligned only (see LAYOUT)
struct __attribute__((aligned(8))) bin_ll2 { ll a, b; };

// what a thread carries through its units
struct BinAcc {
    unsigned int pos, neg, rp, rn, sp, sn;
    bool out_all, out_kept;  // per lane
    bool certain;            // wave-uniform, sticky
};

// K elements of one lane (`in` false: the lane holds none; x = 0 and t = 0
// stand in, never outside). The ballot needs every lane of the wave here.
template <bool CURVE, int K>
__device__ __forceinline__ void bin_take(
    const float (&x)[K], const ll (&t)[K], bool in, ll ignore_index, int has_ignore, float thr,
    float lthr, BinAcc& a, unsigned int* __restrict__ h_raw, unsigned int* __restrict__ h_sig,
    const float* __restrict__ sthr, int T, int uniform, float t0, float inv_step) {
    unsigned int live = 0;
    bool kept_out = false;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const bool out = in && ml_outside_unit(x[k]);
        const bool lv = in && !(has_ignore && t[k] == ignore_index);
        const bool lb = t[k] == 1;
        const bool pr = x[k] > thr;
        const bool ps = x[k] > lthr;
        // the stat range test sees ignored elements too
        a.out_all |= out;
        kept_out |= out && lv;
        live |= lv ? (1u << k) : 0u;
        a.pos += (lv && lb) ? 1u : 0u;
        a.neg += (lv && !lb) ? 1u : 0u;
        a.rp += (lv && pr && lb) ? 1u : 0u;
        a.rn += (lv && pr && !lb) ? 1u : 0u;
        a.sp += (lv && ps && lb) ? 1u : 0u;
        a.sn += (lv && ps && !lb) ? 1u : 0u;
    }
    a.out_kept |= kept_out;
    if constexpr (CURVE) {
        a.certain = a.certain || __ballot(kept_out) != 0ULL;
#pragma unroll
        for (int k = 0; k < K; k++) {
            if ((live >> k) & 1u) {
                const int lab = t[k] == 1 ? 1 : 0;
                const float p = ml_sigmoid(x[k]);
                const int j = uniform ? bucket_of_uniform(p, sthr, T, t0, inv_step)
                                      : bucket_of(p, sthr, T);
                atomicAdd(&h_sig[j * 2 + lab], 1u);
                if (!a.certain) {
                    const int jr = uniform ? bucket_of_uniform(x[k], sthr, T, t0, inv_step)
                                           : bucket_of(x[k], sthr, T);
                    atomicAdd(&h_raw[jr * 2 + lab], 1u);
                }
            }
        }
    }
}

template <typename T_, bool CURVE>
__global__ void __launch_bounds__(BIN_BLOCK_MAX) k_bin_step(
    const T_* __restrict__ preds, const ll* __restrict__ target, ll N, ll head, ll nvec,
    ll n_units, ll ignore_index, int has_ignore, float thr, ull* __restrict__ counts,
    const float* __restrict__ thresholds, int T, int uniform, float t0, float inv_step, int ncopy,
    ull* __restrict__ curve_scratch /* [2][T+1][2] */, unsigned char* __restrict__ records) {
    extern __shared__ unsigned int s_dyn[];  // CURVE: hist [ncopy][2][T+1][2] u32, then T thresholds
    __shared__ unsigned int s_cnt[6];
    __shared__ unsigned int s_flags;

    constexpr int EPV = 16 / sizeof(T_);  // elements per vector
    constexpr int NV = BIN_EPT / EPV;     // vectors per thread and unit
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int bins = (T + 1) * 2;
    float* sthr = (float*)(s_dyn + (CURVE ? ncopy * 2 * bins : 0));
    unsigned int* h_raw = s_dyn + (CURVE ? (wave % ncopy) * 2 * bins : 0);
    unsigned int* h_sig = h_raw + bins;

    if constexpr (CURVE) {
        for (int i = threadIdx.x; i < ncopy * 2 * bins; i += blockDim.x) s_dyn[i] = 0;
        for (int i = threadIdx.x; i < T; i += blockDim.x) sthr[i] = thresholds[i];
    }
    if (threadIdx.x < 6) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_flags = 0;
    __syncthreads();

    const float lthr = ml_logit_threshold(thr);
    BinAcc a = {0, 0, 0, 0, 0, 0, false, false, false};

    // ---- scalar head and tail: the first lanes of block 0 ----
    if (blockIdx.x == 0 && wave == 0) {
        const ll body_end = head + nvec * EPV;
        const ll ns = head + (N - body_end);  // < 2 * EPV <= 64
        const bool in = lane < ns;
        const ll e = lane < head ? (ll)lane : body_end + (lane - head);
        const float x[1] = {in ? ld_f32(preds, e) : 0.0f};
        const ll t[1] = {in ? target[e] : 0};
        bin_take<CURVE, 1>(x, t, in, ignore_index, has_ignore, thr, lthr, a, h_raw, h_sig, sthr, T,
                           uniform, t0, inv_step);
    }

    // ---- the body, one unit per pass ----
    const uint4* pv = reinterpret_cast<const uint4*>(preds + head);
    const ll* tb = target + head;
    for (ll unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        uint4 raw[NV];
        ll t[NV][EPV];
        bool in[NV];
#pragma unroll
        for (int v = 0; v < NV; v++) {
            const ll gv = unit * (ll)(blockDim.x * NV) + v * blockDim.x + threadIdx.x;
            in[v] = gv < nvec;
            raw[v] = make_uint4(0, 0, 0, 0);
            const bin_ll2* tv = reinterpret_cast<const bin_ll2*>(tb + (in[v] ? gv : 0) * EPV);
            if (in[v]) raw[v] = pv[gv];
#pragma unroll
            for (int k = 0; k < EPV / 2; k++) {
                bin_ll2 w = {0, 0};
                if (in[v]) w = tv[k];
                t[v][2 * k] = w.a;
                t[v][2 * k + 1] = w.b;
            }
        }
#pragma unroll
        for (int v = 0; v < NV; v++) {
            float x[EPV];
            unpack16<T_>(raw[v], x);
            bin_take<CURVE, EPV>(x, t[v], in[v], ignore_index, has_ignore, thr, lthr, a, h_raw, h_sig,
                                 sthr, T, uniform, t0, inv_step);
        }
    }

    // the block's counts meet in LDS; nothing here touches a shared global word
    const unsigned int w_pos = wave_sum_u32(a.pos), w_neg = wave_sum_u32(a.neg);
    const unsigned int w_rp = wave_sum_u32(a.rp), w_rn = wave_sum_u32(a.rn);
    const unsigned int w_sp = wave_sum_u32(a.sp), w_sn = wave_sum_u32(a.sn);
    const unsigned int wave_flags = (__ballot(a.out_all) != 0ULL ? 1u : 0u) | (__ballot(a.out_kept) != 0ULL ? 2u : 0u);
    if (lane == 0) {
        if (w_pos) atomicAdd(&s_cnt[0], w_pos);
        if (w_neg) atomicAdd(&s_cnt[1], w_neg);
        if (w_rp) atomicAdd(&s_cnt[2], w_rp);
        if (w_rn) atomicAdd(&s_cnt[3], w_rn);
        if (w_sp) atomicAdd(&s_cnt[4], w_sp);
        if (w_sn) atomicAdd(&s_cnt[5], w_sn);
        if (wave_flags) atomicOr(&s_flags, wave_flags);
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const unsigned int v = s_cnt[threadIdx.x];
        if (v) atomicAdd(&counts[threadIdx.x], (ull)v);
    }
    if constexpr (CURVE) {
        for (int i = threadIdx.x; i < 2 * bins; i += blockDim.x) {
            unsigned int v = 0;
            for (int c = 0; c < ncopy; c++) v += s_dyn[c * 2 * bins + i];
            if (v) atomicAdd(&curve_scratch[i], (ull)v);
        }
    }
    if (threadIdx.x == 0) records[blockIdx.x] = (unsigned char)s_flags;
}

template <bool CURVE>
__global__ void __launch_bounds__(BIN_TAIL_BLOCK) k_bin_tail(
    const unsigned char* __restrict__ records, int grid /* blocks k_bin_step ran with */,
    ull* __restrict__ counts, ll* __restrict__ tp, ll* __restrict__ fp, ll* __restrict__ tn,
    ll* __restrict__ fn, ll* __restrict__ confmat, unsigned int* __restrict__ E, int T,
    ull* __restrict__ hist /* (1, T+1, 2) */, ull* __restrict__ curve_scratch) {
    __shared__ unsigned int s_fl;
    const int lane = threadIdx.x & 63;

    // ---- (a) the two batch-global decisions ----
    if (threadIdx.x == 0) s_fl = 0;
    unsigned int fl = 0;
    for (int i = threadIdx.x; i < grid; i += blockDim.x) fl |= records[i];
    const unsigned int wave_fl = (__ballot(fl & 1u) != 0ULL ? 1u : 0u) | (__ballot(fl & 2u) != 0ULL ? 2u : 0u);
    __syncthreads();
    if (lane == 0 && wave_fl) atomicOr(&s_fl, wave_fl);
    __syncthreads();
    const bool outside_all = (s_fl & 1u) != 0;   // stat: any element outside [0,1]
    const bool outside_kept = (s_fl & 2u) != 0;  // confmat, curve: any kept element

    // ---- (b) one thread: pick, apply, zero ----
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const ll pos = (ll)counts[0], neg = (ll)counts[1];
        const ll rp = (ll)counts[2], rn = (ll)counts[3], sp = (ll)counts[4], sn = (ll)counts[5];
#pragma unroll
        for (int q = 0; q < 6; q++) counts[q] = 0;
        if (tp) {
            const ll pp = outside_all ? sp : rp;  // predicted positive, label 1
            const ll pn = outside_all ? sn : rn;  // predicted positive, label 0
            tp[0] += pp;
            fp[0] += pn;
            tn[0] += neg - pn;
            fn[0] += pos - pp;
        }
        if (confmat) {
            const ll pp = outside_kept ? sp : rp;
            const ll pn = outside_kept ? sn : rn;
            confmat[0] += neg - pn;
            confmat[1] += pn;
            confmat[2] += pos - pp;
            confmat[3] += pp;
        }
        if (E) E[1] += 1u;
    }

    // ---- (c) the chosen histogram of this step into the leader's ----
    if constexpr (CURVE) {
        const int bins = (T + 1) * 2;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < bins; i += gridDim.x * blockDim.x) {
            const ull r = curve_scratch[i], s = curve_scratch[bins + i];
            const ull v = outside_kept ? s : r;
            if (r) curve_scratch[i] = 0;
            if (s) curve_scratch[bins + i] = 0;
            if (v) hist[i] += v;
        }
    }
}

// ---- host: the layout of a step, a function of N, dtype, T and the head ----
struct BinLayout {
    ll head, nvec, n_units;
    int threads, grid, tgrid, ncopy;
    size_t lds;  // dynamic LDS of k_bin_step
};

static size_t bin_hist_lds(int ncopy, int T) {
    return (size_t)ncopy * 2 * (T + 1) * 2 * sizeof(unsigned int) + (size_t)T * sizeof(float);
}

static int bin_env(const char* name, int lo, int hi, int dflt) {
    const char* e = getenv(name);
    if (!e) return dflt;
    const int v = atoi(e);
    return v < lo || v > hi ? dflt : v;
}

// false: shape not covered. T = 0: no curve leader. misalign = bytes of the
// preds address past a 16-byte boundary.
static bool bin_layout(ll N, int dtype, int T, unsigned int misalign, BinLayout* o) {
    if (N < 0 || N >= (1LL << 31) || T < 0 || (dtype != 0 && dtype != 1)) return false;
    const int esize = dtype == 0 ? 4 : 2;
    if (misalign % esize) return false;
    const int epv = 16 / esize;
    if (T > 0 && bin_hist_lds(1, T) + BIN_LDS_STATIC > BIN_LDS_BYTES) return false;
    ll head = ((16 - misalign) & 15) / esize;
    if (head > N) head = N;
    o->head = head;
    o->nvec = (N - head) / epv;
    // sweep knobs (profiles/README.md): the block count, the block size, and
    // the histogram variant: 0 one pair of histograms per block, 1 one pair
    // per wave
    static int want_env = -1, threads_env = -1, variant_env = -1;
    if (want_env < 0) {
        want_env = bin_env("MA_BIN_STEP_BLOCKS", 1, BIN_GRID_MAX, 0);
        threads_env = bin_env("MA_BIN_STEP_THREADS", BIN_BLOCK_MIN, BIN_BLOCK_MAX, 0);
        if (threads_env != 256 && threads_env != 512 && threads_env != 1024) threads_env = 0;
        variant_env = bin_env("MA_BIN_STEP_VARIANT", 0, 1, 0);
    }
    // the widest block with which BIN_MIN_UNITS blocks still get a unit each:
    // every block flushes its histogram with one global atomic per non-zero
    // bin, all blocks onto the same (T+1)*2 words, so fewer and wider blocks pay
    // less for it (measured: profiles/README.md)
    int threads = BIN_BLOCK_MAX;
    while (threads > BIN_BLOCK_MIN && o->nvec * epv < (ll)BIN_MIN_UNITS * threads * BIN_EPT) threads >>= 1;
    if (threads_env) threads = threads_env;
    o->threads = threads;
    const ll vec_per_unit = (ll)threads * BIN_EPT / epv;
    o->n_units = (o->nvec + vec_per_unit - 1) / vec_per_unit;
    const ll want = want_env ? want_env : BIN_THREADS / threads;
    ll grid = o->n_units < want ? o->n_units : want;
    if (grid < 1) grid = 1;  // the scalar head and tail
    o->grid = N > 0 ? (int)grid : 0;
    const int waves = threads / 64;
    o->ncopy = 1;
    if (T > 0 && variant_env == 1 && bin_hist_lds(waves, T) + BIN_LDS_STATIC <= BIN_LDS_COPIES_MAX)
        o->ncopy = waves;
    o->lds = T > 0 ? bin_hist_lds(o->ncopy, T) : 0;
    ll tg = T > 0 ? ((ll)(T + 1) * 2 + BIN_TAIL_BLOCK - 1) / BIN_TAIL_BLOCK : 1;
    if (tg > BIN_TAIL_GRID) tg = BIN_TAIL_GRID;
    o->tgrid = (int)tg;
    return true;
}

template <typename T_, bool CURVE>
static int bin_step_launch(hipStream_t s, const BinStep& st, const BinLayout& lay, const void* preds,
                           const ll* target, ll N) {
    const int T = (int)st.T;
    if (N > 0) {
        k_bin_step<T_, CURVE><<<lay.grid, lay.threads, lay.lds, s>>>(
            (const T_*)preds, target, N, lay.head, lay.nvec, lay.n_units, st.ignore_index,
            (int)st.has_ignore, (float)st.thr, st.counts, st.thresholds, T, (int)st.uniform,
            (float)st.t0, (float)st.inv_step, lay.ncopy, st.curve_scratch, st.records);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    k_bin_tail<CURVE><<<lay.tgrid, BIN_TAIL_BLOCK, 0, s>>>(
        st.records, lay.grid, st.counts, st.tp, st.fp, st.tn, st.fn, st.confmat,
        CURVE ? st.epoch_buf : nullptr, T, st.hist, st.curve_scratch);
    return (int)hipGetLastError();
}

extern "C" {

int ma_bin_step_sizeof() { return (int)sizeof(BinStep); }
// the field names in declaration order, each followed by a comma
const char* ma_bin_step_field_names() {
#define BIN_STEP_NAME(type, name) #name ","
    return BIN_STEP_FIELDS(BIN_STEP_NAME);
#undef BIN_STEP_NAME
}

// Host only: what a step over N elements of `dtype` (0 = f32, 1 = bf16) with T
// thresholds (0: no curve leader) needs, for a 16-byte aligned `preds`.
// out = {record bytes, elements per unit, elements per vector, blocks of
// k_bin_step, blocks of k_bin_tail, dynamic LDS bytes, histogram copies per
// block}. -103: shape not covered.
int ma_bin_step_layout(ll N, int dtype, int T, ll* out) {
    BinLayout lay;
    if (!bin_layout(N, dtype, T, 0, &lay)) return -103;
    out[0] = BIN_GRID_MAX;
    out[1] = (ll)lay.threads * BIN_EPT;
    out[2] = dtype == 0 ? 4 : 8;
    out[3] = lay.grid;
    out[4] = lay.tgrid;
    out[5] = (ll)lay.lds;
    out[6] = lay.ncopy;
    return 0;
}

// The whole binary step on one stream in two launches (N == 0: the tail
// alone). The record is read here, on the host; the kernels get its pointers
// by value. -103 for a shape or dtype the kernels do not cover, a missing
// buffer or an address that is no multiple of the element size; nothing is
// launched then.
int ma_bin_step(uintptr_t stream, const BinStep* st, uintptr_t preds, int dtype /*0=f32 1=bf16*/,
                uintptr_t target, ll N) {
    if (dtype != 0 && dtype != 1) return -103;
    if (!st->counts || !st->records || (N > 0 && (!preds || !target))) return -103;
    if (target % sizeof(ll)) return -103;
    // the stat group is whole or absent
    if (!st->tp != !st->fp || !st->tp != !st->tn || !st->tp != !st->fn) return -103;
    const bool curve = st->T > 0;
    if (st->T < 0 || st->T > (1 << 20)) return -103;
    if (curve && (!st->thresholds || !st->hist || !st->curve_scratch || !st->epoch_buf)) return -103;
    BinLayout lay;
    if (!bin_layout(N, dtype, (int)st->T, (unsigned int)(preds & 15), &lay)) return -103;
    hipStream_t s = (hipStream_t)stream;
    int rc = 0;
    if (curve) FOR_DTYPE(dtype, rc = bin_step_launch<DT, true>(s, *st, lay, (const void*)preds, (const ll*)target, N));
    else FOR_DTYPE(dtype, rc = bin_step_launch<DT, false>(s, *st, lay, (const void*)preds, (const ll*)target, N));
    return rc;
}

}  // extern "C"
