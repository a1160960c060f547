// Fused update of a multilabel collection (gfx950): ONE pass over the (N, L)
// logits / probabilities and the (N, L) int64 targets feeds the stat-scores,
// confusion-matrix, exact-match and threshold-curve group leaders. Two
// launches per step, k_ml_step and k_ml_tail; record: ml_step.h.
//
// SEMANTICS (taken from the stand-alone kernels, which a fused collection must
// equal bit for bit): the batch is normalised with sigmoid iff ANY element,
// ignored positions included, lies outside [0,1] (NaN is not outside). The
// prediction is x > thr without and x > logit(thr) with normalisation
// (ml_rule.h), an element whose target is ignore_index counts in nothing, the
// label is t == 1. Targets outside {0, 1, ignore_index} are outside the
// contract. EXACT MATCH follows MultilabelExactMatch.update as it stands (and
// the reference library): a row is correct iff every element has pred ==
// target, and an ignored element compares unequal to every prediction, so a
// row with an ignored element is never correct. The curve bins p = x or 1/(1+expf(-x)) with bucket_of /
// bucket_of_uniform, as curve_hist_tile does.
//
// LAYOUT. lane = label: a wave covers a chunk of CW = 16, 32 or 64 consecutive
// labels and 64/CW consecutive rows per load, so the lanes of a load read
// consecutive addresses of each row (8 B per lane of targets, 2 or 4 B of
// predictions) and a lane's label never changes. CW is the widest chunk that
// pads L by at most an eighth (L = 1000: 64, L = 80 and 14: 16). One REGION is
// ML_U = 8 such loads of one wave: ML_U * 64/CW rows of one chunk, held in
// registers. A block (16 waves) owns one chunk for its lifetime; its waves
// stride over the chunk's regions.
//
// One pass over a region yields
//  - six counters per label in registers across all regions of the thread:
//    pos, neg, and predicted-positive by label under the raw and under the
//    sigmoid cut. They meet once per block in LDS and leave it with one global
//    atomic per non-zero counter into the count scratch [L][6];
//  - per row the mismatch bits of this chunk (raw, sigmoid), by ballot; a row
//    with a mismatch ORs them into its word of `rowbad`;
//  - the region's outside-[0,1] bit;
//  - CERTAINTY RULE (curve): once a wave has seen an outside element, in this
//    region or an earlier one, the batch-global decision is known to be
//    "sigmoid" and the region is binned from registers into the block's
//    LDS-private histogram [CW][T+1][2] u32, flushed once per block with one
//    global atomic per non-zero bin. A region with every element in [0,1],
//    seen before its wave is certain, is DEFERRED: one flag byte, no binning.
//    Logits defer practically nothing, probabilities everything.
// The block ends with one record byte (deferred, outside); no atomic touches a
// single global word.
//
// k_ml_tail runs behind it. Every block ORs the `grid` record bytes and so
// knows the decision and whether regions wait. One thread per label picks the
// raw or sigmoid counters, adds them to tp/fp/tn/fn and confmat[l] =
// [[tn, fp], [fn, tp]] and zeroes its scratch slots; threads striding the rows
// count the rows whose chosen mismatch bit is clear and zero `rowbad` (one
// atomic per block onto `correct`, from at most 64 blocks); block 0 adds
// total += N and closes the curve epoch, E[1] += 1 (E[0] is never written, so
// E[0] <= E[1] keeps holding for the stand-alone producers). If nothing was
// deferred the rest returns; otherwise the waves stride over the flagged
// regions, bin them under the batch-global decision with global atomics and
// clear the flags.
//
// There is no spin, ticket or grid-wide wait. Nothing one block of a launch
// writes is read by another block of that launch; blocks only meet in atomic
// adds / ORs onto histogram, scratch and rowbad words. Every scratch slot,
// rowbad word and region flag is read and zeroed by the one thread that owns
// it; records are never zeroed, the tail reads only `grid` of them.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "curve_common.h"
#include "ml_rule.h"
#include "ml_step.h"
#include "row_fold.h"

typedef long long ll;
typedef unsigned long long ull;

#define ML_U 8            // loads per lane and region
#define ML_BLOCK 1024     // threads of k_ml_step: 16 waves share one LDS histogram
#define ML_TAIL_BLOCK 256
#define ML_GRID_MAX 1024  // record bytes = cap of the k_ml_step grid
#define ML_ROW_BLOCKS 64  // tail blocks that count rows: atomics onto `correct`
#define ML_TAIL_GRID 1024
// LDS of a workgroup on gfx950, and what k_ml_step keeps statically (block
// counters [64][6] u32 and two words, rounded up); ML_STEP_MAX_T in ops/_hip.py
// is derived from the same two numbers
#define ML_LDS_BYTES (160 * 1024)
#define ML_LDS_STATIC 2048

// One region in registers: ML_U loads of this lane's label. x = 0 and t = 0
// stand in where the lane has no element (label >= L or row >= N); such a lane
// is never outside, and `ok` keeps it out of every count.
template <typename T_>
__device__ __forceinline__ void ml_load_region(
    const T_* __restrict__ preds, const ll* __restrict__ target, ll N, ll L, ll label, bool lab_ok,
    ll row0, int rw, float (&x)[ML_U], ll (&t)[ML_U], unsigned int& ok) {
    ok = 0;
#pragma unroll
    for (int u = 0; u < ML_U; u++) {
        const ll row = row0 + (ll)u * rw;
        const bool in = lab_ok && row < N;
        const ll idx = in ? row * L + label : 0;
        t[u] = in ? target[idx] : 0;
        x[u] = in ? ld_f32(preds, idx) : 0.0f;
        ok |= in ? (1u << u) : 0u;
    }
}

template <typename T_, bool CURVE>
__global__ void __launch_bounds__(ML_BLOCK) k_ml_step(
    const T_* __restrict__ preds, const ll* __restrict__ target, ll N, ll L, ll ignore_index,
    int has_ignore, float thr, int cw_shift, int n_chunks, ll n_rg, ull* __restrict__ counts,
    unsigned int* __restrict__ rowbad /* nullable */, const float* __restrict__ thresholds, int T,
    int uniform, float t0, float inv_step, ull* __restrict__ hist /* (L, T+1, 2) */,
    unsigned char* __restrict__ region_flags, unsigned char* __restrict__ records) {
    extern __shared__ unsigned int s_dyn[];  // CURVE: hist [CW][T+1][2] u32, then T thresholds
    __shared__ unsigned int s_cnt[64 * 6];
    __shared__ unsigned int s_flags;

    const int CW = 1 << cw_shift;
    const int rw = 64 >> cw_shift;  // rows per load of a wave
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wpb = blockDim.x >> 6;
    const int lc = lane & (CW - 1);  // label within the chunk
    const int rsub = lane >> cw_shift;
    const int chunk = blockIdx.x % n_chunks;  // the grid is a multiple of n_chunks
    const ll rb = blockIdx.x / n_chunks;
    const ll nrb = gridDim.x / n_chunks;
    const ll label = (ll)chunk * CW + lc;
    const bool lab_ok = label < L;
    const int hist_words = CW * (T + 1) * 2;
    unsigned int* s_hist = s_dyn;
    float* sthr = (float*)(s_dyn + hist_words);

    if constexpr (CURVE) {
        for (int i = threadIdx.x; i < hist_words; i += blockDim.x) s_hist[i] = 0;
        for (int i = threadIdx.x; i < T; i += blockDim.x) sthr[i] = thresholds[i];
    }
    for (int i = threadIdx.x; i < 64 * 6; i += blockDim.x) s_cnt[i] = 0;
    if (threadIdx.x == 0) s_flags = 0;
    __syncthreads();

    const float lthr = ml_logit_threshold(thr);
    // the row segment of this lane inside a 64-lane ballot
    const ull seg = cw_shift == 6 ? ~0ULL : (((1ULL << CW) - 1ULL) << (rsub * CW));
    unsigned int c_pos = 0, c_neg = 0, c_rp = 0, c_rn = 0, c_sp = 0, c_sn = 0;
    bool certain = false;  // wave-uniform, sticky
    unsigned int wave_flags = 0;

    for (ll rg = rb * wpb + wave; rg < n_rg; rg += nrb * wpb) {
        const ll row0 = rg * (ll)(rw * ML_U) + rsub;
        float x[ML_U];
        ll t[ML_U];
        unsigned int ok;
        ml_load_region<T_>(preds, target, N, L, label, lab_ok, row0, rw, x, t, ok);

        unsigned int live = 0, lab = 0;
        bool out = false;
#pragma unroll
        for (int u = 0; u < ML_U; u++) {
            const bool in = (ok >> u) & 1u;
            // the range test sees ignored elements too
            out |= ml_outside_unit(x[u]);
            const bool lv = in && !(has_ignore && t[u] == ignore_index);
            const bool lb = t[u] == 1;
            const bool pr = x[u] > thr;
            const bool ps = x[u] > lthr;
            live |= lv ? (1u << u) : 0u;
            lab |= lb ? (1u << u) : 0u;
            c_pos += (lv && lb) ? 1u : 0u;
            c_neg += (lv && !lb) ? 1u : 0u;
            c_rp += (lv && pr && lb) ? 1u : 0u;
            c_rn += (lv && pr && !lb) ? 1u : 0u;
            c_sp += (lv && ps && lb) ? 1u : 0u;
            c_sn += (lv && ps && !lb) ? 1u : 0u;
            // exact match: does this row mismatch anywhere in this chunk. An
            // ignored element never matches (see the head of this file)
            const ull bad_r = __ballot(in && (!lv || pr != lb)) & seg;
            const ull bad_s = __ballot(in && (!lv || ps != lb)) & seg;
            const unsigned int bits = (bad_r ? 1u : 0u) | (bad_s ? 2u : 0u);
            if (rowbad && lc == 0 && in && bits) atomicOr(&rowbad[row0 + (ll)u * rw], bits);
        }
        const bool region_out = __ballot(out) != 0ULL;
        if (region_out) wave_flags |= 2u;
        if constexpr (CURVE) {
            certain = certain || region_out;
            if (certain) {
#pragma unroll
                for (int u = 0; u < ML_U; u++) {
                    if ((live >> u) & 1u) {
                        const float p = ml_sigmoid(x[u]);
                        const int j = uniform ? bucket_of_uniform(p, sthr, T, t0, inv_step)
                                              : bucket_of(p, sthr, T);
                        atomicAdd(&s_hist[(lc * (T + 1) + j) * 2 + ((lab >> u) & 1u)], 1u);
                    }
                }
            } else {
                if (lane == 0) region_flags[(ll)chunk * n_rg + rg] = 1;
                wave_flags |= 1u;
            }
        }
    }

    // the block's counts meet in LDS; nothing here touches a shared global word
    if (c_pos) atomicAdd(&s_cnt[lc * 6 + 0], c_pos);
    if (c_neg) atomicAdd(&s_cnt[lc * 6 + 1], c_neg);
    if (c_rp) atomicAdd(&s_cnt[lc * 6 + 2], c_rp);
    if (c_rn) atomicAdd(&s_cnt[lc * 6 + 3], c_rn);
    if (c_sp) atomicAdd(&s_cnt[lc * 6 + 4], c_sp);
    if (c_sn) atomicAdd(&s_cnt[lc * 6 + 5], c_sn);
    if (lane == 0 && wave_flags) atomicOr(&s_flags, wave_flags);
    __syncthreads();
    for (int i = threadIdx.x; i < CW * 6; i += blockDim.x) {
        const unsigned int v = s_cnt[i];
        const ll l = (ll)chunk * CW + i / 6;
        if (v && l < L) atomicAdd(&counts[l * 6 + i % 6], (ull)v);
    }
    if constexpr (CURVE) {
        const int per_label = (T + 1) * 2;
        for (int i = threadIdx.x; i < hist_words; i += blockDim.x) {
            const unsigned int v = s_hist[i];
            if (v) {  // only labels < L were binned
                const ll l = (ll)chunk * CW + i / per_label;
                atomicAdd(&hist[(ull)l * per_label + i % per_label], (ull)v);
            }
        }
    }
    if (threadIdx.x == 0) records[blockIdx.x] = (unsigned char)s_flags;
}

template <typename T_, bool CURVE>
__global__ void __launch_bounds__(ML_TAIL_BLOCK) k_ml_tail(
    const unsigned char* __restrict__ records, int grid /* blocks k_ml_step ran with */,
    ull* __restrict__ counts, ll L, ll N, ll* __restrict__ tp, ll* __restrict__ fp,
    ll* __restrict__ tn, ll* __restrict__ fn, ll* __restrict__ confmat, ll* __restrict__ correct,
    ll* __restrict__ total, unsigned int* __restrict__ rowbad, int row_blocks,
    unsigned int* __restrict__ E, const T_* __restrict__ preds, const ll* __restrict__ target,
    ll ignore_index, int has_ignore, const float* __restrict__ thresholds, int T, int uniform,
    float t0, float inv_step, ull* __restrict__ hist, unsigned char* __restrict__ region_flags,
    int cw_shift, int n_chunks, ll n_rg) {
    extern __shared__ float sthr_t[];
    __shared__ unsigned int s_fl, s_good;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // ---- (a) the batch-global decision ----
    if (threadIdx.x == 0) { s_fl = 0; s_good = 0; }
    unsigned int fl = 0;
    for (int i = threadIdx.x; i < grid; i += blockDim.x) fl |= records[i];
    if constexpr (CURVE)
        for (int i = threadIdx.x; i < T; i += blockDim.x) sthr_t[i] = thresholds[i];
    const unsigned int wave_fl = (__ballot(fl & 1u) != 0ULL ? 1u : 0u) | (__ballot(fl & 2u) != 0ULL ? 2u : 0u);
    __syncthreads();
    if (lane == 0 && wave_fl) atomicOr(&s_fl, wave_fl);
    __syncthreads();
    const bool deferred = (s_fl & 1u) != 0;
    const bool outside = (s_fl & 2u) != 0;  // sigmoid iff any element lay outside [0,1]

    // ---- (b) one thread per label: pick, apply, zero ----
    const ll i = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < L) {
        ull* c = counts + i * 6;
        const ll pos = (ll)c[0], neg = (ll)c[1];
        const ll pp = (ll)(outside ? c[4] : c[2]);  // predicted positive, label 1
        const ll pn = (ll)(outside ? c[5] : c[3]);  // predicted positive, label 0
#pragma unroll
        for (int q = 0; q < 6; q++) c[q] = 0;
        const ll dtp = pp, dfp = pn, dtn = neg - pn, dfn = pos - pp;
        if (tp) {
            tp[i] += dtp;
            fp[i] += dfp;
            tn[i] += dtn;
            fn[i] += dfn;
        }
        if (confmat) {
            confmat[i * 4 + 0] += dtn;
            confmat[i * 4 + 1] += dfp;
            confmat[i * 4 + 2] += dfn;
            confmat[i * 4 + 3] += dtp;
        }
    }

    // ---- (c) rows without a mismatch under the chosen cut ----
    if (rowbad && (int)blockIdx.x < row_blocks) {
        const unsigned int bit = outside ? 2u : 1u;
        unsigned int good = 0;
        for (ll r = (ll)blockIdx.x * blockDim.x + threadIdx.x; r < N; r += (ll)row_blocks * blockDim.x) {
            const unsigned int w = rowbad[r];
            if (w) rowbad[r] = 0;
            good += (w & bit) ? 0u : 1u;
        }
        for (int off = 32; off > 0; off >>= 1) good += __shfl_down(good, off);
        if (lane == 0 && good) atomicAdd(&s_good, good);
        __syncthreads();
        if (threadIdx.x == 0 && s_good) atomicAdd((ull*)correct, (ull)s_good);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (total) total[0] += N;
        if (E) E[1] += 1u;
    }

    // ---- (d) the deferred regions ----
    if constexpr (CURVE) {
        if (!deferred) return;
        const int CW = 1 << cw_shift;
        const int rw = 64 >> cw_shift;
        const int lc = lane & (CW - 1);
        const int rsub = lane >> cw_shift;
        const ll nregions = (ll)n_chunks * n_rg;
        const int wpb = blockDim.x >> 6;
        for (ll r = (ll)blockIdx.x * wpb + wave; r < nregions; r += (ll)gridDim.x * wpb) {
            if (__builtin_amdgcn_readfirstlane((int)region_flags[r]) == 0) continue;
            const ll chunk = r / n_rg, rg = r % n_rg;
            const ll label = chunk * CW + lc;
            float x[ML_U];
            ll t[ML_U];
            unsigned int ok;
            ml_load_region<T_>(preds, target, N, L, label, label < L, rg * (ll)(rw * ML_U) + rsub,
                               rw, x, t, ok);
#pragma unroll
            for (int u = 0; u < ML_U; u++) {
                if (((ok >> u) & 1u) && !(has_ignore && t[u] == ignore_index)) {
                    const float p = outside ? ml_sigmoid(x[u]) : x[u];
                    const int j = uniform ? bucket_of_uniform(p, sthr_t, T, t0, inv_step)
                                          : bucket_of(p, sthr_t, T);
                    atomicAdd(&hist[((ull)label * (T + 1) + j) * 2 + (t[u] == 1 ? 1 : 0)], 1ULL);
                }
            }
            if (lane == 0) region_flags[r] = 0;
        }
    }
}

// ---- host: the layout of a step, a function of L, N and T alone ----
struct MlLayout {
    int cw_shift, n_chunks, grid, tgrid, row_blocks;
    ll n_rg, nregions;
    size_t lds;  // dynamic LDS of k_ml_step
};

static size_t ml_hist_lds(int cw_shift, int T) {
    return (size_t)(1 << cw_shift) * (T + 1) * 2 * sizeof(unsigned int) + (size_t)T * sizeof(float);
}

// false: shape not covered. T = 0: no curve leader.
static bool ml_layout(ll L, ll N, int T, MlLayout* o) {
    if (L < 1 || N < 0 || N >= (1LL << 31) || T < 0) return false;
    // the widest chunk that pads L by at most an eighth, else the narrowest
    int s = 4;
    for (int c = 6; c > 4; c--) {
        const ll cw = 1LL << c;
        const ll pad = (L + cw - 1) / cw * cw;
        if ((pad - L) * 8 <= L) { s = c; break; }
    }
    // ... that still leaves room for the block's histogram
    while (T > 0 && s > 4 && ml_hist_lds(s, T) + ML_LDS_STATIC > ML_LDS_BYTES) s--;
    const size_t lds = T > 0 ? ml_hist_lds(s, T) : 0;
    if (lds + ML_LDS_STATIC > ML_LDS_BYTES) return false;
    const ll cw = 1LL << s;
    const ll n_chunks = (L + cw - 1) / cw;
    if (n_chunks > ML_GRID_MAX) return false;
    const ll rows_per_region = (64 >> s) * ML_U;
    const ll n_rg = (N + rows_per_region - 1) / rows_per_region;
    // one block per CU while the histogram takes most of a CU's LDS, else two;
    // sweep knob MA_ML_STEP_BLOCKS (profiles/README.md)
    static int want_env = -1;
    if (want_env < 0) {
        const char* e = getenv("MA_ML_STEP_BLOCKS");
        want_env = e ? atoi(e) : 0;
        if (want_env < 0 || want_env > ML_GRID_MAX) want_env = 0;
    }
    const ll want = want_env ? want_env : lds + ML_LDS_STATIC > ML_LDS_BYTES / 2 ? 256 : 512;
    ll rb = (n_rg + ML_BLOCK / 64 - 1) / (ML_BLOCK / 64);
    ll cap = want / n_chunks;
    if (cap < 1) cap = 1;
    if (rb > cap) rb = cap;
    if (rb < 1) rb = 1;
    o->cw_shift = s;
    o->n_chunks = (int)n_chunks;
    o->n_rg = n_rg;
    o->nregions = n_chunks * n_rg;
    o->grid = N > 0 ? (int)(n_chunks * rb) : 0;
    o->lds = lds;
    ll row_blocks = (N + 8 * ML_TAIL_BLOCK - 1) / (8 * ML_TAIL_BLOCK);
    if (row_blocks > ML_ROW_BLOCKS) row_blocks = ML_ROW_BLOCKS;
    o->row_blocks = (int)row_blocks;
    ll tg = (L + ML_TAIL_BLOCK - 1) / ML_TAIL_BLOCK;
    if (tg < row_blocks) tg = row_blocks;
    if (T > 0) {  // blocks for the deferred regions, one region per wave and pass
        ll dg = (o->nregions + ML_TAIL_BLOCK / 64 - 1) / (ML_TAIL_BLOCK / 64);
        if (dg > ML_TAIL_GRID) dg = ML_TAIL_GRID;
        if (tg < dg) tg = dg;
    }
    o->tgrid = (int)tg;
    return true;
}

template <typename T_, bool CURVE>
static int ml_step_launch(hipStream_t s, const MlStep& st, const MlLayout& lay, const void* preds,
                          const ll* target, ll N) {
    const int T = (int)st.T;
    if (N > 0) {
        k_ml_step<T_, CURVE><<<lay.grid, ML_BLOCK, lay.lds, s>>>(
            (const T_*)preds, target, N, st.L, st.ignore_index, (int)st.has_ignore, (float)st.thr,
            lay.cw_shift, lay.n_chunks, lay.n_rg, st.counts, st.rowbad, st.thresholds, T,
            (int)st.uniform, (float)st.t0, (float)st.inv_step, st.hist, st.region_flags,
            st.records);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    k_ml_tail<T_, CURVE><<<lay.tgrid, ML_TAIL_BLOCK, (size_t)T * sizeof(float), s>>>(
        st.records, lay.grid, st.counts, st.L, N, st.tp, st.fp, st.tn, st.fn, st.confmat,
        st.correct, st.total, st.rowbad, lay.row_blocks, CURVE ? st.epoch_buf : nullptr,
        (const T_*)preds, target, st.ignore_index, (int)st.has_ignore, st.thresholds, T,
        (int)st.uniform, (float)st.t0, (float)st.inv_step, st.hist, st.region_flags, lay.cw_shift,
        lay.n_chunks, lay.n_rg);
    return (int)hipGetLastError();
}

extern "C" {

int ma_ml_step_sizeof() { return (int)sizeof(MlStep); }
// the field names in declaration order, each followed by a comma
const char* ma_ml_step_field_names() {
#define ML_STEP_NAME(type, name) #name ","
    return ML_STEP_FIELDS(ML_STEP_NAME);
#undef ML_STEP_NAME
}

// Host only: what a step over (N, L) with T thresholds (0: no curve leader)
// needs. out = {region flag bytes, record bytes, chunk width, rows per region,
// blocks of k_ml_step, blocks of k_ml_tail}. -103: shape not covered.
int ma_ml_step_layout(ll L, ll N, int T, ll* out) {
    MlLayout lay;
    if (!ml_layout(L, N, T, &lay)) return -103;
    out[0] = T > 0 ? lay.nregions : 0;
    out[1] = ML_GRID_MAX;
    out[2] = 1LL << lay.cw_shift;
    out[3] = (64 >> lay.cw_shift) * ML_U;
    out[4] = lay.grid;
    out[5] = lay.tgrid;
    return 0;
}

// The whole multilabel step on one stream in two launches (N == 0: the tail
// alone). The record is read here, on the host; the kernels get its pointers
// by value. -103 for a shape or dtype the kernels do not cover or a missing
// buffer; nothing is launched then.
int ma_ml_step(uintptr_t stream, const MlStep* st, uintptr_t preds, int dtype /*0=f32 1=bf16*/,
               uintptr_t target, ll N) {
    if (dtype != 0 && dtype != 1) return -103;
    if (!st->counts || !st->records || (N > 0 && (!preds || !target))) return -103;
    // groups are whole or absent
    if (!st->tp != !st->fp || !st->tp != !st->tn || !st->tp != !st->fn) return -103;
    if (!st->correct != !st->total || !st->correct != !st->rowbad) return -103;
    const bool curve = st->T > 0;
    if (st->T < 0 || st->T > (1 << 20)) return -103;
    if (curve && (!st->thresholds || !st->hist || !st->epoch_buf || !st->region_flags)) return -103;
    MlLayout lay;
    if (!ml_layout(st->L, N, (int)st->T, &lay)) return -103;
    if (curve && lay.nregions > st->region_cap) return -103;
    hipStream_t s = (hipStream_t)stream;
    int rc = 0;
    if (curve) FOR_DTYPE(dtype, rc = ml_step_launch<DT, true>(s, *st, lay, (const void*)preds, (const ll*)target, N));
    else FOR_DTYPE(dtype, rc = ml_step_launch<DT, false>(s, *st, lay, (const void*)preds, (const ll*)target, N));
    return rc;
}

}  // extern "C"
