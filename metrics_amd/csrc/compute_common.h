// Device code shared by the stand-alone compute kernels (kernels.hip) and the
// collection compute plan (mc_compute.hip). The plan's kernels must return
// what the stand-alone kernels return bit for bit, so both call these
// functions: the same fp32 terms, converted to double, summed in the same
// slots and paired in the same tree.
#pragma once

#include <hip/hip_runtime.h>

// ---------------------------------------------------------------------------
// Curve flush: one tile of CTILE classes of the TRANSPOSED (T, C, 2, 2) state.
//   confmat[t][1][1] += sum_{j>t} hist[j][1]   (tp)
//   confmat[t][0][1] += sum_{j>t} hist[j][0]   (fp)
//   confmat[t][1][0] += pos_total - tp         (fn)
//   confmat[t][0][0] += neg_total - fp         (tn)
// stage / suf: CTILE * (T+1) * 2 u64 of LDS each. The histogram of the tile
// is staged (and zeroed in memory when zero_hist), suffix-scanned one wave per
// class, and the state goes out as contiguous (CTILE*4)-element runs per t,
// one thread per (t, class) cell.
// flush == 0: nothing to add; histogram and state are only read.
// KEEP: the cell's four new state values stay in LDS for curve_kept():
// [0][*] over the cell's own stage slot, [1][*] over its own suf slot. Those
// two slots are read by this thread alone (the totals live in suf slot T,
// which no t < T owns), so the overwrite needs no barrier before it; the
// caller synchronises before reading the kept values.
// Block of 256 threads; ends without a barrier.
template <int CTILE, bool KEEP>
__device__ __forceinline__ void curve_suffix_tile(
    unsigned long long* __restrict__ hist /* (C, T+1, 2) */, int T, long long C, int zero_hist,
    int flush, long long* __restrict__ confmat /* (T, C, 2, 2) */,
    unsigned long long* __restrict__ stage, unsigned long long* __restrict__ suf, long long c0,
    int ctile) {
    typedef long long ll;
    typedef unsigned long long ull;
    const int W = 64;
    const int row = (T + 1) * 2;
    if (flush) {
        for (int i = threadIdx.x; i < ctile * row; i += blockDim.x) {
            const int lc = i / row;
            const int rem = i - lc * row;
            stage[lc * row + rem] = hist[(c0 + lc) * (ll)row + rem];
            if (zero_hist) hist[(c0 + lc) * (ll)row + rem] = 0;
        }
        __syncthreads();
        // wave-parallel per-class suffix scan: lane partials over T/64 chunks,
        // cross-lane exclusive suffix via shfl, then a short serial tail per
        // chunk — serial depth drops from O(T) to O(T/64)+log2(64)
        const int lane = threadIdx.x & (W - 1);
        const int wv = threadIdx.x / W;
        const int nwaves = blockDim.x / W;
        const int chunk = (T + 1 + W - 1) / W;
        for (int lc = wv; lc < ctile; lc += nwaves) {
            const ull* h = stage + lc * row;
            ull* sf = suf + lc * row;
            const int j0 = lane * chunk;
            const int j1 = min(j0 + chunk, T + 1);
            ull pf = 0, pt = 0;
            for (int j = j0; j < j1; j++) { pf += h[j * 2 + 0]; pt += h[j * 2 + 1]; }
            ull sfp = pf, stp = pt;  // inclusive suffix over lanes >= l
            for (int off = 1; off < W; off <<= 1) {
                ull of = __shfl_down(sfp, off);
                ull ot = __shfl_down(stp, off);
                if (lane + off < W) { sfp += of; stp += ot; }
            }
            ull run_f = sfp - pf;  // exclusive: sum over lanes > l
            ull run_t = stp - pt;
            for (int j = j1 - 1; j >= j0; j--) {
                // position j holds the sum over (j, T]; j == T is never read
                // as a suffix and takes the totals below
                if (j < T) { sf[j * 2 + 0] = run_f; sf[j * 2 + 1] = run_t; }
                run_f += h[j * 2 + 0];
                run_t += h[j * 2 + 1];
            }
            // lane 0's inclusive suffix is the grand total: neg / pos totals
            const ull tot_f = __shfl(sfp, 0);
            const ull tot_t = __shfl(stp, 0);
            if (lane == 0) { sf[T * 2 + 0] = tot_f; sf[T * 2 + 1] = tot_t; }
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < T * ctile; i += blockDim.x) {
        const int t = i / ctile;
        const int lc = i - t * ctile;
        ull* sf = suf + lc * row;
        ull* h = stage + lc * row;
        ll* g = confmat + ((ll)t * C + (c0 + lc)) * 4;
        ll v0 = g[0], v1 = g[1], v2 = g[2], v3 = g[3];
        if (flush) {
            const ull neg_total = sf[T * 2 + 0];
            const ull pos_total = sf[T * 2 + 1];
            const ull fp_s = sf[t * 2 + 0];
            const ull tp_s = sf[t * 2 + 1];
            v0 += (ll)(neg_total - fp_s);  // tn
            v1 += (ll)fp_s;                // fp
            v2 += (ll)(pos_total - tp_s);  // fn
            v3 += (ll)tp_s;                // tp
            g[0] = v0; g[1] = v1; g[2] = v2; g[3] = v3;
        }
        if (KEEP) {
            h[t * 2 + 0] = (ull)v0; h[t * 2 + 1] = (ull)v1;
            sf[t * 2 + 0] = (ull)v2; sf[t * 2 + 1] = (ull)v3;
        }
    }
}

// State readers for the AUC code below: cm(t, i, j) = confmat[t][class][i][j]
// as float. One class of the (T, C, 2, 2) state in memory ...
struct CurveCmGlobal {
    const long long* confmat;
    long long C, c;
    __device__ __forceinline__ float operator()(int t, int i, int j) const {
        return (float)confmat[(((long long)t * C + c) * 2 + i) * 2 + j];
    }
};
// ... or one class of a tile that curve_suffix_tile<., true> kept in LDS
// (stage, suf already offset to the class).
struct CurveCmKept {
    const unsigned long long* stage;
    const unsigned long long* suf;
    __device__ __forceinline__ float operator()(int t, int i, int j) const {
        return (float)(long long)(i == 0 ? stage[t * 2 + j] : suf[t * 2 + j]);
    }
};

__device__ __forceinline__ float curve_sdiv(float n, float d) { return d != 0.0f ? n / d : 0.0f; }

// Per-class AUROC (mode 0: trapz of tpr over fpr, flipped t) / AP (mode 1:
// -sum((r[t+1]-r[t]) * p[t]) with p_T = 1, r_T = 0) as 256 slot sums: slot s
// adds the fp32 terms t = s, s + 256, ... in that order, each converted to
// double, and the slots are then paired by tree256_*.
template <typename CM>
__device__ __forceinline__ double curve_auc_slot_sum(const CM& cm, int T, int mode, int slot) {
    double acc = 0.0;
    if (mode == 0) {
        for (int t = slot; t < T - 1; t += 256) {
            const float tp0 = cm(t, 1, 1), fn0 = cm(t, 1, 0), fp0 = cm(t, 0, 1), tn0 = cm(t, 0, 0);
            const float tp1 = cm(t + 1, 1, 1), fn1 = cm(t + 1, 1, 0), fp1 = cm(t + 1, 0, 1),
                        tn1 = cm(t + 1, 0, 0);
            const float tpr0 = curve_sdiv(tp0, tp0 + fn0), tpr1 = curve_sdiv(tp1, tp1 + fn1);
            const float fpr0 = curve_sdiv(fp0, fp0 + tn0), fpr1 = curve_sdiv(fp1, fp1 + tn1);
            acc += (double)((fpr0 - fpr1) * 0.5f * (tpr0 + tpr1));
        }
    } else {
        for (int t = slot; t < T; t += 256) {
            const float tp0 = cm(t, 1, 1), fn0 = cm(t, 1, 0), fp0 = cm(t, 0, 1);
            const float p0 = curve_sdiv(tp0, tp0 + fp0);
            const float r0 = curve_sdiv(tp0, tp0 + fn0);
            float r1;
            if (t + 1 < T) {
                const float tp1 = cm(t + 1, 1, 1), fn1 = cm(t + 1, 1, 0);
                r1 = curve_sdiv(tp1, tp1 + fn1);
            } else {
                r1 = 0.0f;  // appended endpoint (recall_T = 0)
            }
            acc += (double)(-(r1 - r0) * p0);
        }
    }
    return acc;
}

// support weights: AUROC at the last threshold, AP at t = 0
template <typename CM>
__device__ __forceinline__ float curve_auc_weight(const CM& cm, int T, int mode) {
    const int tw = mode == 0 ? T - 1 : 0;
    return cm(tw, 1, 1) + cm(tw, 1, 0);
}

// The 256-slot double tree: level off = 128, 64, ..., 1 adds slot s + off into
// slot s for s < off; slot 0 is the sum. Two carriers of the same pairing:
// a block of 256 threads with one slot each in LDS (ends with red[0] valid for
// every thread) ...
__device__ __forceinline__ void tree256_block(double* red) {
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
}
// ... or one wave whose lane l holds slots l, l + 64, l + 128, l + 192: the
// levels 128 and 64 stay inside the lane, the rest go lane to lane. IEEE
// addition commutes, so each pair gives the same double either way. Lane 0
// returns the sum.
__device__ __forceinline__ double tree256_wave(double a0, double a1, double a2, double a3) {
    a0 += a2;  // off 128: slots [0, 128) += [128, 256)
    a1 += a3;
    a0 += a1;  // off 64
    for (int off = 32; off > 0; off >>= 1) a0 += __shfl_down(a0, off);
    return a0;
}

// ---------------------------------------------------------------------------
// one-launch stat-score compute: every precision/recall/accuracy/F-beta/
// specificity/NPV/hamming reduction is post(safe_div(n.s, d.s)) with linear
// coefficients over (tp,fp,tn,fn), then micro / macro / weighted averaging —
// ONE block replaces the ~15-launch torch chain per metric at compute time.
// avg_mode: 0 macro, 1 weighted, 2 micro. Matches _adjust_weights_safe_divide
// bit-for-bit: per-class (w*s)/W summed (not sum(w*s)/W). Block of 256.
__device__ inline void _linear_stat_eval(
    const long long* __restrict__ tp, const long long* __restrict__ fp,
    const long long* __restrict__ tn, const long long* __restrict__ fn, long long C, float n0,
    float n1, float n2, float n3, float d0, float d1, float d2, float d3, int avg_mode,
    int zero_w_topk, float zero_division, float post_a, float post_b, float* __restrict__ out) {
    typedef long long ll;
    __shared__ double red[256];
    // pass 1: total weight W (macro/weighted) or nothing (micro)
    double wsum = 0.0;
    if (avg_mode != 2) {
        for (ll i = threadIdx.x; i < C; i += blockDim.x) {
            const float vtp = (float)tp[i], vfp = (float)fp[i], vfn = (float)fn[i];
            if (avg_mode == 1) {
                wsum += (double)(vtp + vfn);
            } else {
                const float empty = zero_w_topk ? (vtp + vfn) : (vtp + vfp + vfn);
                wsum += (empty == 0.0f) ? 0.0 : 1.0;
            }
        }
    }
    red[threadIdx.x] = wsum;
    __syncthreads();
    tree256_block(red);
    const float W = (float)red[0];
    __syncthreads();

    // pass 2: sum of per-class contributions, matching torch's
    // _safe_divide(w*s, W).sum() element order: each term is (w*s)/W in f32
    double a = 0.0, b = 0.0;
    for (ll i = threadIdx.x; i < C; i += blockDim.x) {
        const float vtp = (float)tp[i], vfp = (float)fp[i], vtn = (float)tn[i], vfn = (float)fn[i];
        const float num = n0 * vtp + n1 * vfp + n2 * vtn + n3 * vfn;
        const float den = d0 * vtp + d1 * vfp + d2 * vtn + d3 * vfn;
        if (avg_mode == 2) {
            a += (double)num;
            b += (double)den;
        } else {
            const float s = post_a * (den != 0.0f ? num / den : zero_division) + post_b;
            float w;
            if (avg_mode == 1) {
                w = vtp + vfn;
            } else {
                const float empty = zero_w_topk ? (vtp + vfn) : (vtp + vfp + vfn);
                w = (empty == 0.0f) ? 0.0f : 1.0f;
            }
            a += (double)(W != 0.0f ? (w * s) / W : 0.0f);
        }
    }
    red[threadIdx.x] = a;
    __syncthreads();
    tree256_block(red);
    if (avg_mode == 2) {
        __shared__ double redb[256];
        redb[threadIdx.x] = b;
        __syncthreads();
        tree256_block(redb);
        if (threadIdx.x == 0) {
            const float fa = (float)red[0], fb = (float)redb[0];
            out[0] = post_a * (fb != 0.0f ? fa / fb : zero_division) + post_b;
        }
    } else if (threadIdx.x == 0) {
        out[0] = (float)red[0];
    }
}

// params: 13 floats per formula (n0-3, d0-3, avg_mode, zero_w_topk,
// zero_division, post_a, post_b)
__device__ __forceinline__ void linear_stat_eval_params(
    const long long* __restrict__ tp, const long long* __restrict__ fp,
    const long long* __restrict__ tn, const long long* __restrict__ fn, long long C,
    const float* __restrict__ P, float* __restrict__ out) {
    _linear_stat_eval(tp, fp, tn, fn, C, P[0], P[1], P[2], P[3], P[4], P[5], P[6], P[7],
                      (int)P[8], (int)P[9], P[10], P[11], P[12], out);
}

// (C,C) confusion-matrix scalars, phase B: one block of 256 folds the C-sized
// row sums / column sums / diagonal that k_confmat_moments left into
// [mcc, kappa, jaccard_macro] and re-zeroes the row- and column-sum scratch.
__device__ inline void confmat_scalars_eval(
    unsigned long long* __restrict__ pk, const unsigned long long* __restrict__ diag,
    unsigned long long* __restrict__ tk /* consumed + re-zeroed */, long long C,
    float zero_division, float* __restrict__ out /* [mcc, kappa, jaccard_macro] */) {
    typedef long long ll;
    __shared__ double sh[6][256];
    double s_tot = 0, s_tr = 0, s_tkpk = 0, s_tk2 = 0, s_pk2 = 0;
    double j_sum = 0, j_cnt = 0;
    for (ll i = threadIdx.x; i < C; i += blockDim.x) {
        const double t = (double)tk[i];
        const double p = (double)pk[i];
        const double d = (double)diag[i];
        tk[i] = 0;  // scratch consumed: zero for the next call
        pk[i] = 0;
        s_tot += t;
        s_tr += d;
        s_tkpk += t * p;
        s_tk2 += t * t;
        s_pk2 += p * p;
        const double den = t + p - d;
        if (t + p > 0) {
            j_cnt += 1.0;
            j_sum += den > 0 ? d / den : (double)zero_division;
        }
    }
    sh[0][threadIdx.x] = s_tot; sh[1][threadIdx.x] = s_tr; sh[2][threadIdx.x] = s_tkpk;
    sh[3][threadIdx.x] = s_tk2; sh[4][threadIdx.x] = s_pk2; sh[5][threadIdx.x] = j_sum;
    __shared__ double shc[256];
    shc[threadIdx.x] = j_cnt;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) {
            for (int q = 0; q < 6; q++) sh[q][threadIdx.x] += sh[q][threadIdx.x + off];
            shc[threadIdx.x] += shc[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // float32 to match the torch reference chains bit-closely
        const float s = (float)sh[0][0], c = (float)sh[1][0];
        const float tkpk = (float)sh[2][0], tk2 = (float)sh[3][0], pk2 = (float)sh[4][0];
        const float cov = c * s - tkpk;
        const float den = (s * s - pk2) * (s * s - tk2);
        out[0] = den == 0.0f ? 0.0f : cov / sqrtf(fmaxf(den, 1.1754944e-38f));
        const float po_n = s - c;            // sum(w*cm),  w = 1 - I
        const float pe_n = s - tkpk / s;     // sum(w*E)
        out[1] = 1.0f - po_n / pe_n;         // 0/0 -> nan, x/0 -> inf: torch parity
        out[2] = shc[0] > 0 ? (float)(sh[5][0] / shc[0]) : zero_division;
    }
}
