// Collection compute() in one native call: what the 16-metric multiclass
// collection launches at compute time, behind one plan.
//
// A MetricCollection.compute() used to enter one Python wrapper per metric,
// each with its own cache lookup, output allocation and launch: about twenty
// launches for ~85 us of kernels inside a ~290 us call (profiles/README.md,
// "Collection compute plan"). One step of the plan makes two:
//
//   1. k_compute_passes<CTILE>    one grid, the role of a block fixed by its
//                                 index (block-uniform, no ticket, no spin, no
//                                 grid-wide wait; neither role reads what the
//                                 other writes):
//        blocks [0, ceil(C/CTILE))  curve role: lazy curve flush (histogram ->
//                                 (T, C, 2, 2) state) and, from the tile still
//                                 in LDS, per-class AUROC / AP and their support
//                                 weights: the 6.4 MB state is written once and
//                                 not read back. A histogram in pending-b0
//                                 format (mc_onepass.hip) is completed in the
//                                 staged tile, not by a pass in front.
//        the blocks after them    confusion-matrix role: ONE pass over the
//                                 (C, C) matrix gives row sums, column sums,
//                                 the diagonal and, when asked for, the copy
//                                 that MulticlassConfusionMatrix returns
//   2. k_collection_scalars       block b < n_formulas: linear stat formula b;
//                                 then one block for mcc / kappa / jaccard,
//                                 one for exact match. The only consumer of
//                                 the moments, and the next launch on the stream.
//
// A plan without a curve group or without a confusion-matrix group launches
// k_compute_passes with the one role present. Where T is too large for the
// tiled curve kernel (curve_lds == 0) the stand-alone curve kernels run in
// front, as before.
//
// Every device function that produces a value is shared with the stand-alone
// kernels (compute_common.h), so the plan returns the same bits.
//
// Exposed C API (ctypes, see ops/_hip.py):
//   ma_compute_plan_create(C, T, tp, fp, tn, fn, confmat, cm_scratch, correct,
//                          total, hist, curve_state, epoch_buf, params,
//                          n_formulas, zero_division, auc_stride, &handle)
//   ma_compute_plan_step(handle, stream, flags, out, auc_out, pending,
//                        thresholds, cm_copy)
//   ma_compute_plan_launches(handle, flags, pending)      host only
//   ma_compute_plan_destroy(handle)
//   ma_confmat_moments_copy(stream, cm, C, scratch, copy) the second role alone

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "compute_common.h"

typedef long long ll;
typedef unsigned long long ull;

// kernels.hip
extern "C" int ma_curve_suffix(uintptr_t stream, uintptr_t hist, ll outer, int T, int transposed,
                               int zero_hist, uintptr_t epoch_buf, uintptr_t confmat,
                               uintptr_t pending, uintptr_t thresholds);
extern "C" int ma_curve_auc_from_confmat(uintptr_t stream, uintptr_t confmat, int T, ll C,
                                         int mode, uintptr_t out, uintptr_t weights);

#define MA_COMPUTE_FLUSH 1  // step flag: the curve histogram holds updates to flush

// Curve role: flush + both AUC modes for a tile of CTILE classes. Dynamic LDS
// as k_curve_suffix_tiled: 2 * CTILE * (T+1) * 2 u64, nothing else.
// flush == 0 ("nothing to flush"): the state is only read, histogram and
// epoch word are not touched.
// auc_out: [auroc | auroc weights | ap | ap weights], each auc_stride floats.
struct CurveRole {
    ull* hist;  // (C, T+1, 2)
    int T, flush;
    ll C;
    unsigned int* E;  // nullable
    ll* confmat;      // (T, C, 2, 2)
    float* auc_out;
    ll auc_stride;
    ull* pending;  // nullable: [P: C][R: C], see curve_suffix_tile
    const float* thresholds;
};

template <int CTILE>
__device__ __forceinline__ void curve_flush_auc_block(const CurveRole& a, int block) {
    extern __shared__ ull shs[];
    const int T = a.T;
    ull* stage = shs;
    ull* suf = shs + CTILE * (ll)(T + 1) * 2;
    const ll c0 = (ll)block * CTILE;
    const int ctile = (int)min((ll)CTILE, a.C - c0);
    curve_suffix_tile<CTILE, true>(a.hist, T, a.C, 1, a.flush, a.confmat, stage, suf, c0, ctile,
                                   a.pending, a.thresholds);
    // close the epoch where k_curve_suffix_tiled does
    if (a.flush && a.E && block == 0 && threadIdx.x == 0) atomicAdd(&a.E[1], 1u);
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
            float* o = a.auc_out + (ll)mode * 2 * a.auc_stride;
            o[c0 + lc] = (float)sum;
            o[a.auc_stride + c0 + lc] = curve_auc_weight(cm, T, mode);
        }
    }
}

// Confusion-matrix role: block `block` of col_tiles * row_tiles takes
// CM_COLS columns x rows_per_block rows of the (C, C) matrix, two adjacent
// columns per thread, and reads each of its words once. Row sums and column
// sums are added into the pre-zeroed tk / pk (integer sums: the order is
// free), the diagonal is stored, and copy (nullable) receives the words as
// read. With C even and both matrices 16-byte aligned a thread moves its pair
// in one 16-byte access.
#define CM_COLS 512
#define CM_ROWS 8
struct ConfmatRole {
    const ll* cm;  // (C, C)
    ll C, rows_per_block;
    int col_tiles;
    ull *tk, *pk, *diag;
    ll* copy;  // nullable
};

__device__ __forceinline__ void confmat_pass_block(const ConfmatRole& a, int block) {
    const ll C = a.C;
    const int bx = block % a.col_tiles;
    const int by = block / a.col_tiles;
    const ll c = (ll)bx * CM_COLS + 2 * (ll)threadIdx.x;
    const ll r_lo = (ll)by * a.rows_per_block;
    const ll r_hi = min(r_lo + a.rows_per_block, C);
    const int lane = threadIdx.x & 63;
    const bool vec = ((C & 1) == 0) && ((((uintptr_t)a.cm | (uintptr_t)a.copy) & 15) == 0);
    const bool in0 = c < C, in1 = c + 1 < C;
    ull col0 = 0, col1 = 0;
    // CM_ROWS rows at a time: their loads are issued together, ahead of the
    // wave reductions, which would otherwise put one load latency on each row
    for (ll r0 = r_lo; r0 < r_hi; r0 += CM_ROWS) {
        ull v0[CM_ROWS], v1[CM_ROWS];
#pragma unroll
        for (int k = 0; k < CM_ROWS; k++) {
            const ll r = r0 + k;
            const ll at = r * C + c;
            v0[k] = 0; v1[k] = 0;
            if (r < r_hi) {
                if (vec) {
                    if (in0) {  // C even: the pair is inside together
                        const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(a.cm + at);
                        v0[k] = v.x; v1[k] = v.y;
                    }
                } else {
                    if (in0) v0[k] = (ull)a.cm[at];
                    if (in1) v1[k] = (ull)a.cm[at + 1];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < CM_ROWS; k++) {
            const ll r = r0 + k;
            const ll at = r * C + c;
            if (r < r_hi) {  // block-uniform
                if (a.copy) {
                    if (vec) {
                        if (in0) *reinterpret_cast<ulonglong2*>(a.copy + at) = make_ulonglong2(v0[k], v1[k]);
                    } else {
                        if (in0) a.copy[at] = (ll)v0[k];
                        if (in1) a.copy[at + 1] = (ll)v1[k];
                    }
                }
                col0 += v0[k];
                col1 += v1[k];
                if (in0 && c == r) a.diag[r] = v0[k];
                if (in1 && c + 1 == r) a.diag[r] = v1[k];
                // this wave's share of row r: one atomic per wave
                ull rv = v0[k] + v1[k];
                for (int off = 32; off > 0; off >>= 1) rv += __shfl_down(rv, off);
                if (lane == 0 && rv) atomicAdd(&a.tk[r], rv);
            }
        }
    }
    if (in0 && col0) atomicAdd(&a.pk[c], col0);
    if (in1 && col1) atomicAdd(&a.pk[c + 1], col1);
}

// Both roles in one grid: blocks [0, curve_blocks) the curve role, the rest
// the confusion-matrix role; either count may be 0. Dynamic LDS is the curve
// tile's (0 without curve blocks).
template <int CTILE>
__global__ void __launch_bounds__(256) k_compute_passes(CurveRole curve, int curve_blocks,
                                                        ConfmatRole cmr) {
    if ((int)blockIdx.x < curve_blocks)
        curve_flush_auc_block<CTILE>(curve, (int)blockIdx.x);
    else
        confmat_pass_block(cmr, (int)blockIdx.x - curve_blocks);
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

// The (col_tiles, row_tiles, rows_per_block) of the confusion-matrix role.
// About 64 row tiles: every block adds its column sums into pk with one
// atomic per column, so their number is row_tiles * C, and the blocks are
// still enough to stream the matrix next to the curve role.
static void confmat_tiles(ll C, int* col_tiles, ll* row_tiles, ll* rows_per_block) {
    *col_tiles = (int)((C + CM_COLS - 1) / CM_COLS);
    ll rt = C < 64 ? C : 64;
    *rows_per_block = (C + rt - 1) / rt;
    *row_tiles = (C + *rows_per_block - 1) / *rows_per_block;
}

// One launch of k_compute_passes; either role may be absent (curve_blocks ==
// 0 / cm == nullptr), not both.
static int launch_passes(hipStream_t s, int ctile, size_t lds, const CurveRole& curve,
                         int curve_blocks, const ll* cm, ll C, ull* cm_scratch, ll* cm_copy) {
    ConfmatRole r = {};
    ll cm_blocks = 0;
    if (cm) {
        ll row_tiles;
        confmat_tiles(C, &r.col_tiles, &row_tiles, &r.rows_per_block);
        r.cm = cm; r.C = C; r.copy = cm_copy;
        r.tk = cm_scratch; r.pk = cm_scratch + C; r.diag = cm_scratch + 2 * C;
        cm_blocks = (ll)r.col_tiles * row_tiles;
    }
    const ll grid = curve_blocks + cm_blocks;
    if (grid <= 0 || grid > 2147483647LL) return -101;
    if (ctile == 2)
        k_compute_passes<2><<<(unsigned)grid, 256, lds, s>>>(curve, curve_blocks, r);
    else if (ctile == 4)
        k_compute_passes<4><<<(unsigned)grid, 256, lds, s>>>(curve, curve_blocks, r);
    else
        k_compute_passes<8><<<(unsigned)grid, 256, lds, s>>>(curve, curve_blocks, r);
    return (int)hipGetLastError();
}

// dry: nothing is launched and no buffer is looked at beyond being there or
// not; *launches is what the same call makes otherwise.
static int compute_step(const ComputePlan& p, hipStream_t s, int flags, float* out,
                        float* auc_out, uintptr_t pending, uintptr_t thresholds, ll* cm_copy,
                        bool dry, int* launches) {
    const int flush = (flags & MA_COMPUTE_FLUSH) ? 1 : 0;
    int n = 0;
    if (pending && !(flush && p.curve_state)) return -103;  // owed counts are paid by a flush only
    if (pending && !thresholds) return -103;
    if (cm_copy && !p.confmat) return -103;
    CurveRole curve = {};
    int curve_blocks = 0;
    if (p.curve_state) {
        if (!dry && (!auc_out || (flush && !p.hist))) return -103;
        if (p.curve_lds) {
            curve.hist = p.hist; curve.T = p.T; curve.flush = flush; curve.C = p.C;
            curve.E = p.epoch_buf; curve.confmat = p.curve_state; curve.auc_out = auc_out;
            curve.auc_stride = p.auc_stride;
            curve.pending = (ull*)pending; curve.thresholds = (const float*)thresholds;
            curve_blocks = (int)((p.C + p.ctile - 1) / p.ctile);
        } else {
            // T beyond the tiled kernel's LDS: the existing kernels, one after
            // the other, inside this call (the resolve kernel in front of
            // them for a pending histogram)
            n += (pending ? 1 : 0) + flush + 2;
            int rc = 0;
            if (flush && !dry)
                rc = ma_curve_suffix((uintptr_t)s, (uintptr_t)p.hist, p.C, p.T, 1, 1,
                                     (uintptr_t)p.epoch_buf, (uintptr_t)p.curve_state, pending,
                                     thresholds);
            for (int mode = 0; mode < 2 && rc == 0 && !dry; mode++)
                rc = ma_curve_auc_from_confmat(
                    (uintptr_t)s, (uintptr_t)p.curve_state, p.T, p.C, mode,
                    (uintptr_t)(auc_out + (ll)mode * 2 * p.auc_stride),
                    (uintptr_t)(auc_out + ((ll)mode * 2 + 1) * p.auc_stride));
            if (rc != 0) return rc;
        }
    }
    if (curve_blocks > 0 || p.confmat) {
        n += 1;
        if (!dry) {
            const int rc = launch_passes(s, p.ctile, curve_blocks > 0 ? p.curve_lds : 0, curve,
                                         curve_blocks, p.confmat, p.C, p.cm_scratch, cm_copy);
            if (rc != 0) return rc;
        }
    }
    const int nblocks = p.n_formulas + (p.confmat ? 1 : 0) + (p.correct ? 1 : 0);
    if (nblocks > 0) {
        n += 1;
        if (!dry) {
            if (!out) return -103;
            k_collection_scalars<<<nblocks, 256, 0, s>>>(
                p.tp, p.fp, p.tn, p.fn, p.C, p.params, p.n_formulas,
                p.confmat ? p.cm_scratch : nullptr, p.zero_division, p.correct, p.total, out);
        }
    }
    if (launches) *launches = n;
    return dry ? 0 : (int)hipGetLastError();
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
// cm_copy: 0, or C * C int64 that receive a copy of the confusion matrix.
int ma_compute_plan_step(uintptr_t handle, uintptr_t stream, int flags, uintptr_t out,
                         uintptr_t auc_out, uintptr_t pending, uintptr_t thresholds,
                         uintptr_t cm_copy) {
    if (!handle) return -103;
    return compute_step(*(const ComputePlan*)handle, (hipStream_t)stream, flags, (float*)out,
                        (float*)auc_out, pending, thresholds, (ll*)cm_copy, false, nullptr);
}

// Host only: the number of kernel launches ma_compute_plan_step makes for
// these flags, with (pending != 0) or without a histogram in pending format.
// Negative: the error the step would return before launching anything.
int ma_compute_plan_launches(uintptr_t handle, int flags, int pending) {
    if (!handle) return -103;
    int n = 0;
    const int rc = compute_step(*(const ComputePlan*)handle, nullptr, flags, nullptr, nullptr,
                                pending ? 1 : 0, pending ? 1 : 0, nullptr, true, &n);
    return rc != 0 ? (rc < 0 ? rc : -rc) : n;
}

// The confusion-matrix role alone: row sums, column sums and diagonal of the
// (C, C) int64 matrix into the pre-zeroed 3C u64 scratch [tk | pk | diag], as
// ma_confmat_moments leaves them, and a copy of the matrix into `copy`
// (nullable), in one pass.
int ma_confmat_moments_copy(uintptr_t stream, uintptr_t cm, ll C, uintptr_t scratch,
                            uintptr_t copy) {
    if (!cm || !scratch || C <= 0) return -103;
    return launch_passes((hipStream_t)stream, 4, 0, CurveRole{}, 0, (const ll*)cm, C,
                         (ull*)scratch, (ll*)copy);
}

void ma_compute_plan_destroy(uintptr_t handle) { delete (ComputePlan*)handle; }

}  // extern "C"
