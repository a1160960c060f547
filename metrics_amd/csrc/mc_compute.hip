// Collection compute() in one native call: what the 16-metric multiclass
// collection launches at compute time, behind one plan.
//
// A MetricCollection.compute() used to enter one Python wrapper per metric,
// each with its own cache lookup, output allocation and launch: about twenty
// launches for ~85 us of kernels inside a ~290 us call (profiles/README.md,
// "Collection compute plan"). One step of the plan makes at most three, and
// one more in front of them when the histogram is in pending-b0 format
// (k_curve_resolve_pending, kernels.hip):
//
//   1. k_curve_flush_auc<CTILE>   lazy curve flush (histogram -> (T, C, 2, 2)
//                                 state) and, from the tile still in LDS,
//                                 per-class AUROC / AP and their support
//                                 weights: the 6.4 MB state is written once
//                                 and not read back
//   2. k_confmat_moments          (kernels.hip, unchanged) row / column sums
//                                 and diagonal of the (C, C) confusion matrix
//   3. k_collection_scalars       block b < n_formulas: linear stat formula b;
//                                 then one block for mcc / kappa / jaccard,
//                                 one for exact match
//
// Every device function that produces a value is shared with the stand-alone
// kernels (compute_common.h), so the plan returns the same bits.
//
// Exposed C API (ctypes, see ops/_hip.py):
//   ma_compute_plan_create(C, T, tp, fp, tn, fn, confmat, cm_scratch, correct,
//                          total, hist, curve_state, epoch_buf, params,
//                          n_formulas, zero_division, auc_stride, &handle)
//   ma_compute_plan_step(handle, stream, flags, out, auc_out, pending, thresholds)
//   ma_compute_plan_destroy(handle)

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "compute_common.h"

typedef long long ll;
typedef unsigned long long ull;

// kernels.hip
extern "C" int ma_confmat_moments(uintptr_t stream, uintptr_t cm, ll C, uintptr_t scratch);
extern "C" int ma_curve_suffix(uintptr_t stream, uintptr_t hist, ll outer, int T, int transposed,
                               int zero_hist, uintptr_t epoch_buf, uintptr_t confmat,
                               uintptr_t pending, uintptr_t thresholds);
extern "C" int ma_curve_resolve_pending(uintptr_t stream, uintptr_t hist, ll C, int T,
                                        uintptr_t thresholds, uintptr_t pending);
extern "C" int ma_curve_auc_from_confmat(uintptr_t stream, uintptr_t confmat, int T, ll C,
                                         int mode, uintptr_t out, uintptr_t weights);

#define MA_COMPUTE_FLUSH 1  // step flag: the curve histogram holds updates to flush

// Curve flush + both AUC modes for a tile of CTILE classes. Dynamic LDS as
// k_curve_suffix_tiled: 2 * CTILE * (T+1) * 2 u64, nothing else.
// flush == 0 ("nothing to flush"): the state is only read, histogram and
// epoch word are not touched.
// auc_out: [auroc | auroc weights | ap | ap weights], each auc_stride floats.
template <int CTILE>
__global__ void __launch_bounds__(256) k_curve_flush_auc(
    ull* __restrict__ hist /* (C, T+1, 2) */, int T, ll C, int flush,
    unsigned int* __restrict__ E /* nullable */, ll* __restrict__ confmat /* (T, C, 2, 2) */,
    float* __restrict__ auc_out, ll auc_stride) {
    extern __shared__ ull shs[];
    ull* stage = shs;
    ull* suf = shs + CTILE * (ll)(T + 1) * 2;
    const ll c0 = (ll)blockIdx.x * CTILE;
    const int ctile = (int)min((ll)CTILE, C - c0);
    curve_suffix_tile<CTILE, true>(hist, T, C, 1, flush, confmat, stage, suf, c0, ctile);
    // close the epoch where k_curve_suffix_tiled does
    if (flush && E && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&E[1], 1u);
    __syncthreads();
    // one wave per (class, mode): lane l carries slots l, l+64, l+128, l+192
    // of the 256-slot sum
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    for (int task = wv; task < ctile * 2; task += 4) {
        const int lc = task >> 1;
        const int mode = task & 1;
        const CurveCmKept cm{stage + lc * (T + 1) * 2, suf + lc * (T + 1) * 2};
        const double a0 = curve_auc_slot_sum(cm, T, mode, lane);
        const double a1 = curve_auc_slot_sum(cm, T, mode, lane + 64);
        const double a2 = curve_auc_slot_sum(cm, T, mode, lane + 128);
        const double a3 = curve_auc_slot_sum(cm, T, mode, lane + 192);
        const double sum = tree256_wave(a0, a1, a2, a3);
        if (lane == 0) {
            float* o = auc_out + (ll)mode * 2 * auc_stride;
            o[c0 + lc] = (float)sum;
            o[auc_stride + c0 + lc] = curve_auc_weight(cm, T, mode);
        }
    }
}

// All scalar results of a collection in one launch; the block index selects
// the work. out: [linear 0..n-1 | mcc, kappa, jaccard | exact].
__global__ void __launch_bounds__(256) k_collection_scalars(
    const ll* __restrict__ tp, const ll* __restrict__ fp, const ll* __restrict__ tn,
    const ll* __restrict__ fn, ll C, const float* __restrict__ params, int n_formulas,
    ull* __restrict__ cm_scratch /* 3C: tk | pk | diag, nullable */, float zero_division,
    const ll* __restrict__ correct /* nullable, with total */, const ll* __restrict__ total,
    float* __restrict__ out) {
    const int b = blockIdx.x;
    if (b < n_formulas) {
        linear_stat_eval_params(tp, fp, tn, fn, C, params + (ll)b * 13, out + b);
        return;
    }
    if (cm_scratch && b == n_formulas) {
        confmat_scalars_eval(cm_scratch + C, cm_scratch + 2 * C, cm_scratch, C, zero_division,
                             out + n_formulas);
        return;
    }
    // exact match = _safe_divide(correct, total): int64 -> fp32, one IEEE divide
    if (threadIdx.x == 0) {
        const float c = (float)correct[0], t = (float)total[0];
        out[n_formulas + 3] = t != 0.0f ? c / t : 0.0f;
    }
}

// Everything that stays the same between computes. The caller owns the memory
// behind the addresses and keeps it alive as long as the plan. Any group may
// be absent: tp == 0 (no stat leader, n_formulas == 0), confmat == 0, correct
// == 0, curve_state == 0. hist may be 0 while nothing was ever there to flush.
struct ComputePlan {
    ll C, auc_stride;
    int T, n_formulas, ctile;
    size_t curve_lds;  // 0: T too large for the fused kernel, use the old ones
    float zero_division;
    ll *tp, *fp, *tn, *fn, *confmat, *correct, *total, *curve_state;
    ull *cm_scratch, *hist;
    unsigned int* epoch_buf;
    const float* params;
};

static int compute_ctile() {
    static int sel = 0;
    if (sel == 0) {
        const char* e = getenv("MA_SUFFIX_CTILE");  // same knob as ma_curve_suffix
        sel = e ? atoi(e) : 4;
        if (sel != 2 && sel != 8) sel = 4;
    }
    return sel;
}

static int compute_step(const ComputePlan& p, hipStream_t s, int flags, float* out,
                        float* auc_out, uintptr_t pending, uintptr_t thresholds) {
    const int flush = (flags & MA_COMPUTE_FLUSH) ? 1 : 0;
    if (pending && !(flush && p.curve_state)) return -103;  // owed counts are paid by a flush only
    if (p.curve_state) {
        if (!auc_out || (flush && !p.hist)) return -103;
        if (pending) {
            const int rc = ma_curve_resolve_pending((uintptr_t)s, (uintptr_t)p.hist, p.C, p.T,
                                                    thresholds, pending);
            if (rc != 0) return rc;
        }
        if (p.curve_lds) {
            const int grid = (int)((p.C + p.ctile - 1) / p.ctile);
            if (p.ctile == 2)
                k_curve_flush_auc<2><<<grid, 256, p.curve_lds, s>>>(
                    p.hist, p.T, p.C, flush, p.epoch_buf, p.curve_state, auc_out, p.auc_stride);
            else if (p.ctile == 4)
                k_curve_flush_auc<4><<<grid, 256, p.curve_lds, s>>>(
                    p.hist, p.T, p.C, flush, p.epoch_buf, p.curve_state, auc_out, p.auc_stride);
            else
                k_curve_flush_auc<8><<<grid, 256, p.curve_lds, s>>>(
                    p.hist, p.T, p.C, flush, p.epoch_buf, p.curve_state, auc_out, p.auc_stride);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return (int)e;
        } else {
            // T beyond the tiled kernel's LDS: the existing kernels, one after
            // the other, inside this call
            int rc = 0;
            if (flush)
                rc = ma_curve_suffix((uintptr_t)s, (uintptr_t)p.hist, p.C, p.T, 1, 1,
                                     (uintptr_t)p.epoch_buf, (uintptr_t)p.curve_state, 0, 0);
            for (int mode = 0; mode < 2 && rc == 0; mode++)
                rc = ma_curve_auc_from_confmat(
                    (uintptr_t)s, (uintptr_t)p.curve_state, p.T, p.C, mode,
                    (uintptr_t)(auc_out + (ll)mode * 2 * p.auc_stride),
                    (uintptr_t)(auc_out + ((ll)mode * 2 + 1) * p.auc_stride));
            if (rc != 0) return rc;
        }
    }
    if (p.confmat) {
        const int rc = ma_confmat_moments((uintptr_t)s, (uintptr_t)p.confmat, p.C,
                                          (uintptr_t)p.cm_scratch);
        if (rc != 0) return rc;
    }
    const int nblocks = p.n_formulas + (p.confmat ? 1 : 0) + (p.correct ? 1 : 0);
    if (nblocks > 0) {
        if (!out) return -103;
        k_collection_scalars<<<nblocks, 256, 0, s>>>(
            p.tp, p.fp, p.tn, p.fn, p.C, p.params, p.n_formulas,
            p.confmat ? p.cm_scratch : nullptr, p.zero_division, p.correct, p.total, out);
    }
    return (int)hipGetLastError();
}

extern "C" {

// cm_scratch: 3*C u64, zero before the first step (every step re-zeroes what
// it used). params: n_formulas * 13 floats on the device. auc_stride >= C.
// -103 for a missing buffer of a group that is present; *handle is written
// only on success.
int ma_compute_plan_create(ll C, int T, uintptr_t tp, uintptr_t fp, uintptr_t tn, uintptr_t fn,
                           uintptr_t confmat, uintptr_t cm_scratch, uintptr_t correct,
                           uintptr_t total, uintptr_t hist, uintptr_t curve_state,
                           uintptr_t epoch_buf, uintptr_t params, int n_formulas,
                           float zero_division, ll auc_stride, unsigned long long* handle) {
    if (C <= 0 || n_formulas < 0) return -103;
    if (n_formulas > 0 && !(tp && fp && tn && fn && params)) return -103;
    if (confmat && !cm_scratch) return -103;
    if ((correct != 0) != (total != 0)) return -103;
    if (curve_state && (T < 1 || auc_stride < C)) return -103;
    ComputePlan* p = new ComputePlan;
    p->C = C; p->T = T; p->n_formulas = n_formulas; p->auc_stride = auc_stride;
    p->zero_division = zero_division;
    p->tp = (ll*)tp; p->fp = (ll*)fp; p->tn = (ll*)tn; p->fn = (ll*)fn;
    p->confmat = (ll*)confmat; p->cm_scratch = (ull*)cm_scratch;
    p->correct = (ll*)correct; p->total = (ll*)total;
    p->hist = (ull*)hist; p->curve_state = (ll*)curve_state;
    p->epoch_buf = (unsigned int*)epoch_buf; p->params = (const float*)params;
    p->ctile = compute_ctile();
    // the LDS of ma_curve_suffix's tiled kernel for the same T, and its bound
    const size_t lds = (size_t)2 * p->ctile * (T + 1) * 2 * sizeof(ull);
    p->curve_lds = (curve_state && lds <= 160 * 1024) ? lds : 0;
    *handle = (unsigned long long)(uintptr_t)p;
    return 0;
}

// pending / thresholds: the curve histogram is in pending-b0 format (see
// ma_curve_resolve_pending); both 0 otherwise. Only with MA_COMPUTE_FLUSH.
int ma_compute_plan_step(uintptr_t handle, uintptr_t stream, int flags, uintptr_t out,
                         uintptr_t auc_out, uintptr_t pending, uintptr_t thresholds) {
    if (!handle) return -103;
    return compute_step(*(const ComputePlan*)handle, (hipStream_t)stream, flags, (float*)out,
                        (float*)auc_out, pending, thresholds);
}

void ma_compute_plan_destroy(uintptr_t handle) { delete (ComputePlan*)handle; }

}  // extern "C"
