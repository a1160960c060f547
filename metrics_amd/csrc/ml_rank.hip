// Multilabel ranking measures (gfx950): coverage error, label ranking average
// precision (LRAP) and ranking loss of one batch in ONE pass over the (N, L)
// scores and the int64 targets. Two launches per call, k_ml_rank and
// k_ml_rank_tail; nothing returns to the host.
//
// INPUT. `preds` holds the ALREADY NORMALISED scores (fp32 or bf16): the caller
// runs the package's range test and sigmoid in the input dtype, so the kernel
// sees exactly the ties the torch path sees (bf16 sigmoid ties heavily, fp32
// sigmoid saturates to 1.0). An element whose target equals ignore_index is not
// relevant and takes the score -inf: below every real score, equal to every
// other ignored element. Relevant: target == 1 and not ignored.
//
// PER ROW, with s the scores, R the relevant labels, n = |R|:
//  coverage  L if the row holds an ignored element (the torch path writes
//            -4L into the ignored slot, which becomes the row minimum and so
//            "covers" every label: reproduced on purpose, docs/PARITY.md);
//            else #{k : s_k >= min_{j in R} s_j} if n > 0; else 0.
//  LRAP      (1/n) sum_{j in R} #{k in R : s_k >= s_j} / #{k : s_k >= s_j} if
//            0 < n < L, else 1.
//  loss      rows with 0 < n < L are valid;
//            inv_j = #{k : s_k < s_j} + #{k < j : s_k == s_j}, the position
//            under a stable ascending sort, taken as L - inv_j =
//            #{k : s_k >= s_j} - #{k < j : s_k == s_j};
//            value (sum_{j in R} (L - inv_j) - n(n+1)/2) / (n (L - n)).
// Every comparison is an IEEE float compare: one with a NaN is false. What a
// row with a NaN score yields is unspecified; it never faults.
//
// MAPPING. A block is 4 waves. Up to RANK_WAVE_L labels a wave owns a row (4
// rows per block and pass); above it the whole block owns one row. The row is
// staged in LDS as fp32 (padded to a multiple of 4 with NaN, which no compare
// counts) followed by the u16 indices of its relevant labels, compacted in
// index order (wave prefix sums of the per-lane counts, the waves of a block
// row chained through LDS): 6 bytes per label. Rows are read with 16-byte
// vector loads where L and the two addresses allow it, else element by element.
// Then every lane takes ONE relevant label j and walks the row in LDS (all
// lanes read the same float4: a broadcast), counting s_k >= s_j and the ties in
// front of j; a second walk over the compacted indices counts the relevant
// s_k >= s_j. n x L compares per row, none for an irrelevant label.
//
// REDUCTION, in a fixed order. All counts are exact integers; a row's quotient
// is formed in fp64. Lanes meet in an xor butterfly (both partners add the same
// two numbers), the waves of a block row and the row slots of a block are added
// in index order, a block adds its rows in the order it visits them and writes
// four fp64 partials (coverage, LRAP, loss, valid rows) into its slab entry.
// k_ml_rank_tail (one wave) adds the entries, lane l taking l, l + 64, ... in
// order and then the same butterfly, and applies them to the fp32 states in
// place: state = (float)((double)state + delta); total += N, and for the loss
// total += 1 with the measure unchanged when no row of the batch was valid
// (the torch path's `return 0.0, 1`, decided here). No floating atomics: the
// same call gives the same bits every time.
//
// All LDS is dynamic: RANK_LDS_STATIC bytes of block scratch in front, then the
// row slices, each a multiple of 16 bytes, so float4 reads stay aligned.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "row_fold.h"

typedef long long ll;
typedef unsigned long long ull;

#define RANK_BLOCK 256
#define RANK_WAVES 4
#define RANK_WAVE_L 1024   // the last L of the wave-per-row mapping
#define RANK_GRID_MAX 2048  // slab entries = cap of the k_ml_rank grid
// LDS of a workgroup on gfx950, the block scratch in front of the row slices,
// and the bytes a label takes in a slice (fp32 score + u16 index);
// ML_RANK_MAX_L in ops/_hip.py is derived from the same three numbers
#define RANK_LDS_BYTES (160 * 1024)
#define RANK_LDS_STATIC 256
#define RANK_LABEL_BYTES 6
#define RANK_MAX_L ((RANK_LDS_BYTES - RANK_LDS_STATIC) / RANK_LABEL_BYTES / 4 * 4)  // 27264

#define RANK_WANT_COVERAGE 1
#define RANK_WANT_LRAP 2
#define RANK_WANT_LOSS 4

// two consecutive targets of a vector load
struct __attribute__((aligned(16))) rank_ll2 { ll a, b; };

// block scratch at the front of the dynamic LDS (<= RANK_LDS_STATIC bytes)
struct RankScratch {
    double red[RANK_WAVES][4];
    int cnt[RANK_WAVES];
    float mn[RANK_WAVES];
};
static_assert(sizeof(RankScratch) <= RANK_LDS_STATIC, "block scratch");

// sums over the WPR waves that hold a row, returned to every lane. Exact for
// the integer counts (< 2^53); the order is fixed: butterfly, then wave order.
template <int WPR>
__device__ __forceinline__ void rank_group_sum4(double (&v)[4], RankScratch* sc, int wave, int lane) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] += __shfl_xor(v[q], off);
    }
    if constexpr (WPR > 1) {
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 4; q++) sc->red[wave][q] = v[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; q++) {
            double a = sc->red[0][q];
            for (int w = 1; w < WPR; w++) a += sc->red[w][q];
            v[q] = a;
        }
        __syncthreads();
    }
}

template <int WPR>
__device__ __forceinline__ float rank_group_min(float v, RankScratch* sc, int wave, int lane) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
    if constexpr (WPR > 1) {
        if (lane == 0) sc->mn[wave] = v;
        __syncthreads();
        v = sc->mn[0];
        for (int w = 1; w < WPR; w++) v = fminf(v, sc->mn[w]);
        __syncthreads();
    }
    return v;
}

// one relevant label j with score sj against the whole staged row (Lp a
// multiple of 4, padded with NaN): ge = #{k : s_k >= sj}, eqb = #{k < j :
// s_k == sj}. Every lane reads the same address.
template <bool EQB>
__device__ __forceinline__ void rank_count_row(const float* __restrict__ s, int Lp, float sj, int j,
                                               unsigned int& ge, unsigned int& eqb) {
    for (int k = 0; k < Lp; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(s + k);
        ge += (v.x >= sj ? 1u : 0u) + (v.y >= sj ? 1u : 0u) + (v.z >= sj ? 1u : 0u) + (v.w >= sj ? 1u : 0u);
        if constexpr (EQB) {
            eqb += ((v.x == sj && k < j) ? 1u : 0u) + ((v.y == sj && k + 1 < j) ? 1u : 0u) +
                   ((v.z == sj && k + 2 < j) ? 1u : 0u) + ((v.w == sj && k + 3 < j) ? 1u : 0u);
        }
    }
}

// EPV: elements per thread and load, 1 or the 16-byte vector of T
template <typename T_, int WPR, int EPV>
__global__ void __launch_bounds__(RANK_BLOCK) k_ml_rank(
    const T_* __restrict__ preds, const ll* __restrict__ target, ll N, int L, ll ignore_index,
    int has_ignore, int want, ll n_groups, int slice_bytes, double* __restrict__ slab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    RankScratch* sc = reinterpret_cast<RankScratch*>(s_dyn);

    constexpr int RPB = RANK_WAVES / WPR;  // rows per block and pass
    constexpr int G = WPR * 64;            // threads per row
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int slot = wave / WPR;  // the row of the pass this wave works on
    const int wr = wave % WPR;    // this wave among the waves of the row
    const int t = wr * 64 + lane;
    const int Lp = (L + 3) & ~3;
    float* s = reinterpret_cast<float*>(s_dyn + RANK_LDS_STATIC + (size_t)slot * slice_bytes);
    unsigned short* ridx = reinterpret_cast<unsigned short*>(s + Lp);
    const int n_iter = (L + G * EPV - 1) / (G * EPV);

    // the sums of the rows this row slot has seen; every lane holds the same
    double acc_cov = 0.0, acc_lrap = 0.0, acc_loss = 0.0, acc_valid = 0.0;

    for (ll g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const ll row = g * RPB + slot;
        const bool live = row < N;
        const T_* prow = preds + (live ? row : 0) * (ll)L;
        const ll* trow = target + (live ? row : 0) * (ll)L;

        // ---- stage the row: scores, and the relevant indices in index order ----
        int n = 0;  // relevant labels so far; the same in every lane of the row
        float rmin = INFINITY;
        bool any_ign = false;
        for (int it = 0; it < n_iter; it++) {
            const int k0 = (it * G + t) * EPV;
            const bool in = live && k0 < L;  // EPV > 1: L is a multiple of EPV
            float x[EPV];
            ll tg[EPV];
            if constexpr (EPV == 1) {
                x[0] = in ? ld_f32(prow, k0) : 0.0f;
                tg[0] = in ? trow[k0] : 0;
            } else {
                uint4 raw = make_uint4(0, 0, 0, 0);
                if (in) raw = *reinterpret_cast<const uint4*>(prow + k0);
                unpack16<T_>(raw, x);
#pragma unroll
                for (int e = 0; e < EPV; e += 2) {
                    rank_ll2 w = {0, 0};
                    if (in) w = *reinterpret_cast<const rank_ll2*>(trow + k0 + e);
                    tg[e] = w.a;
                    tg[e + 1] = w.b;
                }
            }
            unsigned int relmask = 0;
#pragma unroll
            for (int e = 0; e < EPV; e++) {
                const bool ign = has_ignore && tg[e] == ignore_index;
                const bool rel = in && !ign && tg[e] == 1;
                const float v = ign ? -INFINITY : x[e];
                if (in) s[k0 + e] = v;
                any_ign |= in && ign;
                rmin = rel ? fminf(rmin, v) : rmin;
                relmask |= rel ? (1u << e) : 0u;
            }
            const int c = __popc(relmask);
            int incl = c;  // inclusive prefix over the lanes of the wave
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_up(incl, off);
                incl += lane >= off ? o : 0;
            }
            int before = 0, all = __shfl(incl, 63);
            if constexpr (WPR > 1) {
                if (lane == 0) sc->cnt[wave] = all;
                __syncthreads();
                all = 0;
                for (int w = 0; w < WPR; w++) {
                    const int o = sc->cnt[w];
                    before += w < wr ? o : 0;
                    all += o;
                }
                __syncthreads();
            }
            int pos = n + before + incl - c;
#pragma unroll
            for (int e = 0; e < EPV; e++) {
                if ((relmask >> e) & 1u) ridx[pos++] = (unsigned short)(k0 + e);
            }
            n += all;
        }
        if (live && t < Lp - L) s[L + t] = NAN;
        __syncthreads();

        // ---- coverage ----
        double r[4] = {0.0, any_ign ? 1.0 : 0.0, 0.0, 0.0};  // covered, ignored, LRAP sum, loss sum
        if (want & RANK_WANT_COVERAGE) {
            const float m = rank_group_min<WPR>(rmin, sc, wave, lane);
            unsigned int cov = 0;
            if (live) {
                for (int k = t; k < L; k += G) cov += s[k] >= m ? 1u : 0u;
            }
            r[0] = (double)cov;
        }

        // ---- one relevant label per lane against the row ----
        const bool ranked = live && n > 0 && n < L;
        if (ranked && (want & (RANK_WANT_LRAP | RANK_WANT_LOSS))) {
            double lr = 0.0;
            ull ls = 0;
            for (int p0 = 0; p0 < n; p0 += G) {
                const int p = p0 + t;
                const bool act = p < n;
                const int j = act ? (int)ridx[p] : 0;
                const float sj = act ? s[j] : NAN;  // NaN: an idle lane counts nothing
                unsigned int ge = 0, eqb = 0, ger = 0;
                if (want & RANK_WANT_LOSS) rank_count_row<true>(s, Lp, sj, j, ge, eqb);
                else rank_count_row<false>(s, Lp, sj, j, ge, eqb);
                if (want & RANK_WANT_LRAP) {
#pragma unroll 8
                    for (int q = 0; q < n; q++) ger += s[ridx[q]] >= sj ? 1u : 0u;
                }
                if (act) {
                    lr += (double)ger / (double)ge;
                    ls += (ull)(ge - eqb);
                }
            }
            r[2] = lr;
            r[3] = (double)ls;
        }
        rank_group_sum4<WPR>(r, sc, wave, lane);

        if (live) {
            const double dn = (double)n, dL = (double)L;
            acc_cov += r[1] > 0.0 ? dL : (n > 0 ? r[0] : 0.0);
            acc_lrap += ranked ? r[2] / dn : 1.0;
            if (ranked) {
                acc_loss += (r[3] - 0.5 * dn * (dn + 1.0)) / (dn * (dL - dn));
                acc_valid += 1.0;
            }
        }
        __syncthreads();  // the slices are written again by the next pass
    }

    // ---- the block's four partials, row slots in order ----
    if (wr == 0 && lane == 0) {
        sc->red[slot][0] = acc_cov;
        sc->red[slot][1] = acc_lrap;
        sc->red[slot][2] = acc_loss;
        sc->red[slot][3] = acc_valid;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double a = sc->red[0][threadIdx.x];
        for (int q = 1; q < RPB; q++) a += sc->red[q][threadIdx.x];
        slab[(ll)blockIdx.x * 4 + threadIdx.x] = a;
    }
}

// one wave: the slab entries in a fixed order, then the states in place
__global__ void __launch_bounds__(64) k_ml_rank_tail(
    const double* __restrict__ slab, int grid /* blocks k_ml_rank ran with */, ll N, int want,
    float* __restrict__ cov_measure, float* __restrict__ cov_total, float* __restrict__ lrap_measure,
    float* __restrict__ lrap_total, float* __restrict__ loss_measure, float* __restrict__ loss_total) {
    const int lane = threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = lane; b < grid; b += 64) {
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] += slab[(ll)b * 4 + q];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] += __shfl_xor(v[q], off);
    }
    if (lane != 0) return;
    const double dN = (double)N;
    if (want & RANK_WANT_COVERAGE) {
        cov_measure[0] = (float)((double)cov_measure[0] + v[0]);
        cov_total[0] = (float)((double)cov_total[0] + dN);
    }
    if (want & RANK_WANT_LRAP) {
        lrap_measure[0] = (float)((double)lrap_measure[0] + v[1]);
        lrap_total[0] = (float)((double)lrap_total[0] + dN);
    }
    if (want & RANK_WANT_LOSS) {
        if (v[3] > 0.0) {
            loss_measure[0] = (float)((double)loss_measure[0] + v[2]);
            loss_total[0] = (float)((double)loss_total[0] + dN);
        } else {
            loss_total[0] = (float)((double)loss_total[0] + 1.0);  // no valid row: measure unchanged
        }
    }
}

// ---- host: the layout of a call, a function of N and L ----
struct RankLayout {
    int wpr, grid, slice_bytes;
    ll n_groups;
    size_t lds;
};

static bool rank_layout(ll N, ll L, RankLayout* o) {
    if (N < 1 || N >= (1LL << 40) || L < 1 || L > RANK_MAX_L) return false;
    o->wpr = L <= RANK_WAVE_L ? 1 : RANK_WAVES;
    const int rpb = RANK_WAVES / o->wpr;
    const ll lp = (L + 3) & ~3LL;
    o->slice_bytes = (int)((lp * RANK_LABEL_BYTES + 15) & ~15LL);
    o->lds = RANK_LDS_STATIC + (size_t)rpb * o->slice_bytes;
    if (o->lds > RANK_LDS_BYTES) return false;
    o->n_groups = (N + rpb - 1) / rpb;
    o->grid = (int)(o->n_groups < RANK_GRID_MAX ? o->n_groups : RANK_GRID_MAX);
    return true;
}

template <typename T_, int WPR>
static void rank_launch(hipStream_t s, const RankLayout& lay, bool vec, const void* preds, const ll* target,
                        ll N, int L, ll ignore_index, int has_ignore, int want, double* slab) {
    constexpr int EPV = 16 / sizeof(T_);
    if (vec)
        k_ml_rank<T_, WPR, EPV><<<lay.grid, RANK_BLOCK, lay.lds, s>>>(
            (const T_*)preds, target, N, L, ignore_index, has_ignore, want, lay.n_groups, lay.slice_bytes, slab);
    else
        k_ml_rank<T_, WPR, 1><<<lay.grid, RANK_BLOCK, lay.lds, s>>>(
            (const T_*)preds, target, N, L, ignore_index, has_ignore, want, lay.n_groups, lay.slice_bytes, slab);
}

extern "C" {

// Host only: what a call over (N, L) needs. out = {waves per row, rows per
// block and pass, blocks of k_ml_rank, dynamic LDS bytes, slab entries (of four
// fp64 each), the last L of the wave-per-row mapping, the largest L covered}.
// -103: shape not covered.
int ma_ml_rank_layout(ll N, ll L, ll* out) {
    out[4] = RANK_GRID_MAX;
    out[5] = RANK_WAVE_L;
    out[6] = RANK_MAX_L;
    RankLayout lay;
    if (!rank_layout(N, L, &lay)) return -103;
    out[0] = lay.wpr;
    out[1] = RANK_WAVES / lay.wpr;
    out[2] = lay.grid;
    out[3] = (ll)lay.lds;
    return 0;
}

// The ranking sums of one batch, added into the fp32 states the `want` mask
// (1 coverage, 2 LRAP, 4 loss) names; the others may be null. `slab` holds
// RANK_GRID_MAX * 4 fp64. Two launches on one stream. -103 for a shape or dtype
// the kernels do not cover, a missing buffer or a misaligned address; nothing
// is launched then.
int ma_ml_rank(uintptr_t stream, uintptr_t preds, int dtype /*0=f32 1=bf16*/, uintptr_t target, ll N, ll L,
               ll ignore_index, int has_ignore, int want, uintptr_t slab, uintptr_t cov_measure,
               uintptr_t cov_total, uintptr_t lrap_measure, uintptr_t lrap_total, uintptr_t loss_measure,
               uintptr_t loss_total) {
    if (dtype != 0 && dtype != 1) return -103;
    if (want < 1 || want > 7 || !preds || !target || !slab || slab % sizeof(double)) return -103;
    if ((want & RANK_WANT_COVERAGE) && (!cov_measure || !cov_total)) return -103;
    if ((want & RANK_WANT_LRAP) && (!lrap_measure || !lrap_total)) return -103;
    if ((want & RANK_WANT_LOSS) && (!loss_measure || !loss_total)) return -103;
    const int esize = dtype == 0 ? 4 : 2;
    if (preds % esize || target % sizeof(ll)) return -103;
    RankLayout lay;
    if (!rank_layout(N, L, &lay)) return -103;
    const bool vec = L % (16 / esize) == 0 && preds % 16 == 0 && target % 16 == 0;
    hipStream_t s = (hipStream_t)stream;
    if (lay.wpr == 1)
        FOR_DTYPE(dtype, rank_launch<DT, 1>(s, lay, vec, (const void*)preds, (const ll*)target, N, (int)L,
                                            ignore_index, has_ignore, want, (double*)slab));
    else
        FOR_DTYPE(dtype, rank_launch<DT, RANK_WAVES>(s, lay, vec, (const void*)preds, (const ll*)target, N, (int)L,
                                                     ignore_index, has_ignore, want, (double*)slab));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    k_ml_rank_tail<<<1, 64, 0, s>>>((const double*)slab, lay.grid, N, want, (float*)cov_measure,
                                    (float*)cov_total, (float*)lrap_measure, (float*)lrap_total,
                                    (float*)loss_measure, (float*)loss_total);
    return (int)hipGetLastError();
}

}  // extern "C"
