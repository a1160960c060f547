// Language-model negative log likelihood (gfx950): the two sums behind
// Perplexity, total = sum over kept rows of logsumexp(x) - x[target] and the
// number of kept rows, in ONE pass over (B, T, V) logits. Two launches per
// call, a row kernel and k_lm_nll_tail; nothing returns to the host.
//
// INPUT. `preds` is fp32, bf16 or fp16 (dtype code 0 / 1 / 2; the third code
// exists for this kernel only) with unit stride along V and arbitrary batch
// and sequence strides, in elements; `target` is int64 with arbitrary strides.
// A view such as logits[:, :-1] / labels[:, 1:] is read in place. Every row
// offset is formed in 64 bits.
//
// PER ROW r = (b, t): the target is read first. A row whose target equals
// ignore_index is skipped before any of its logits is loaded (the test is
// wave-uniform in the wave and block mappings). A kept row streams once through
// the online-softmax pair (m, s) in fp32, m the running maximum and s the sum
// of exp(x - m); x[target] is one plain load in front of the stream. The row's
// value (double)m + log((double)s) - (double)x[target] and every sum across
// rows are fp64. A kept row whose target lies outside [0, V) is never
// dereferenced at x[target]: it adds NaN to the total and 1 to the count.
//
// NON-FINITE VALUES follow the arithmetic. m starts at -FLT_MAX, so it is
// never -inf: a -inf element adds exp(-inf) = 0, a row of only -inf ends with
// s = 0 and the value -FLT_MAX + log(0) - (-inf) = NaN. A +inf element makes
// the new maximum +inf and its own term exp(inf - inf) = NaN. A NaN element
// never becomes the maximum (fmaxf drops it) and its term is NaN. x[target] =
// -inf among finite values gives +inf.
//
// THREE MAPPINGS, picked by lm_layout() from (rows, V):
//  1 group   V <= LM_G32_V: a row is owned by 16 (V <= LM_G16_V) or 32 lanes,
//            4 or 2 rows per wave; the lanes keep the virtual-lane pairs of
//            row_fold.h and meet in softmax_merge_group.
//  2 wave    a wave streams the row with 16-byte nontemporal loads, LM_DEPTH
//            loads per lane in flight before the first fold (the kernel has no
//            atomics, so the wave's in-order counter waits only for loads).
//            The elements in front of the first 16-byte boundary and behind
//            the last whole vector (at most 7 + 7) are read one per lane
//            through the same fold, so any 2-byte aligned base, any V and odd
//            row strides are served.
//  3 block   rows < LM_BLOCK_ROWS (fewer rows than the chip has SIMDs) and
//            V > LM_BLOCK_V: the LM_ROW_WAVES waves of a block interleave over
//            the row's vectors; their pairs meet in LDS and are merged in wave
//            order by wave 0.
//
// REDUCTION, in a fixed order, no floating atomics. A wave adds the fp64
// values of its kept rows in row order (the group mapping collects a pass's
// rows from the groups' first lanes in group order). The waves of a block meet
// in LDS and are added in wave order; the block stores {fp64 total, u64 count}
// into its slab entry. The grid is a function of the shape (and of the
// MA_LM_NLL_GRID cap), so the same call gives the same bits every time.
// k_lm_nll_tail (one lane) adds the entries in index order and either writes
// [total, count] as two fp64, or applies them to the fp32 states as the torch
// update does: total += (float)(total rounded to the dtype of preds),
// count += (float)n.

#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "row_fold.h"

typedef long long ll;
typedef unsigned long long ull;
typedef unsigned int lm_u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 lm_f16x2 __attribute__((ext_vector_type(2)));

#define LM_BLOCK 256        // mappings 1 and 2: 4 independent waves
#define LM_WAVES 4
#define LM_ROW_WAVES 16     // mapping 3: the waves that share a row
#define LM_G16_V 128        // the last V a 16-lane group owns
#define LM_G32_V 512        // the last V of the group mapping
#define LM_BLOCK_ROWS 1024  // mapping 3 below this many rows: 256 CUs x 4 SIMDs
#define LM_BLOCK_V 8192     // and above this V
#define LM_MAX_V (1 << 24)  // vector indices inside a row stay in 32 bits
#define LM_GRID_MAX 1024    // slab entries = cap of the row kernels' grid
#define LM_DEPTH_DEFAULT 4  // 16-byte loads per lane in flight; MA_LM_NLL_DEPTH = 4 or 8

struct LmArgs {
    const void* preds;
    const ll* target;
    ll rows, T;            // rows = B * T, row r = (r / T, r % T)
    ll ps0, ps1, ts0, ts1; // strides in elements
    ll ignore_index;
    ll n_groups;           // grid-stride tasks: groups of rows-per-block rows
    int V, has_ignore;
    double* slab;
};

// T is float, unsigned short (bf16 bits) or _Float16
template <typename T_>
__device__ __forceinline__ void lm_unpack(const lm_u32x4& u, float (&f)[16 / sizeof(T_)]) {
    if constexpr (sizeof(T_) == 4) {
#pragma unroll
        for (int i = 0; i < 4; i++) f[i] = __uint_as_float(u[i]);
    } else if constexpr (is_bf16_v<T_>) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            f[2 * i] = __uint_as_float(u[i] << 16);
            f[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const unsigned int w = u[i];  // a copy: a bit cast of the vector element itself reads word 0
            f[2 * i] = (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu));
            f[2 * i + 1] = (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
        }
    }
}

// a vector of -inf: what a lane past the row's end folds
template <typename T_>
__device__ __forceinline__ lm_u32x4 lm_neg_inf() {
    const unsigned int w = sizeof(T_) == 4 ? 0xff800000u : (is_bf16_v<T_> ? 0xff80ff80u : 0xfc00fc00u);
    return lm_u32x4{w, w, w, w};
}

// fold K elements into (m, s): the new maximum first, then every term against
// it, then the old sum rescaled once. m is finite or +inf, never -inf or NaN.
template <int K>
__device__ __forceinline__ void lm_fold(const float (&f)[K], float& m, float& s) {
    float mk = f[0];
#pragma unroll
    for (int i = 1; i < K; i++) mk = fmaxf(mk, f[i]);
    const float mn = fmaxf(m, mk);
    float sk = 0.0f;
#pragma unroll
    for (int i = 0; i < K; i++) sk += __expf(f[i] - mn);
    s = fmaf(s, __expf(m - mn), sk);
    m = mn;
}

// the same over DEPTH packed vectors, one partial sum per vector
template <typename T_, int DEPTH>
__device__ __forceinline__ void lm_fold_vectors(const lm_u32x4 (&raw)[DEPTH], float& m, float& s) {
    constexpr int EPV = 16 / sizeof(T_);
    float f[DEPTH][EPV];
    float mk = -INFINITY;
#pragma unroll
    for (int d = 0; d < DEPTH; d++) {
        lm_unpack<T_>(raw[d], f[d]);
#pragma unroll
        for (int i = 0; i < EPV; i++) mk = fmaxf(mk, f[d][i]);
    }
    const float mn = fmaxf(m, mk);
    float sk = 0.0f;
#pragma unroll
    for (int d = 0; d < DEPTH; d++) {
        float sd = 0.0f;
#pragma unroll
        for (int i = 0; i < EPV; i++) sd += __expf(f[d][i] - mn);
        sk += sd;
    }
    s = fmaf(s, __expf(m - mn), sk);
    m = mn;
}

__device__ __forceinline__ double lm_row_value(bool target_ok, float m, float s, float xt) {
    return target_ok ? (double)m + log((double)s) - (double)xt : (double)NAN;
}

// the block's {total, count}: waves in order. acc / cnt are read from lane 0.
template <int NWAVES>
__device__ __forceinline__ void lm_store_block(double acc, ull cnt, int wave, int lane, double* sh_acc,
                                               ull* sh_cnt, double* __restrict__ slab) {
    if (lane == 0) {
        sh_acc[wave] = acc;
        sh_cnt[wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = sh_acc[0];
        ull c = sh_cnt[0];
        for (int w = 1; w < NWAVES; w++) {
            a += sh_acc[w];
            c += sh_cnt[w];
        }
        slab[2 * (ll)blockIdx.x] = a;
        reinterpret_cast<ull*>(slab)[2 * (ll)blockIdx.x + 1] = c;
    }
}

// ---- mapping 1: LPR lanes per row ----
template <typename T_, int LPR>
__global__ void __launch_bounds__(LM_BLOCK) k_lm_nll_group(const LmArgs a) {
    __shared__ double sh_acc[LM_WAVES];
    __shared__ ull sh_cnt[LM_WAVES];
    constexpr int Q = 64 / LPR;  // rows per wave, and virtual lanes per lane
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int g = lane / LPR, l = lane % LPR;
    const T_* __restrict__ preds = static_cast<const T_*>(a.preds);
    const int V = a.V;
    double acc = 0.0;  // lane 0: the wave's kept rows so far, in row order
    ull cnt = 0;

    for (ll grp = blockIdx.x; grp < a.n_groups; grp += gridDim.x) {
        const ll row = (grp * LM_WAVES + wave) * Q + g;
        const bool inr = row < a.rows;
        const ll b = inr ? row / a.T : 0, t = inr ? row % a.T : 0;
        const ll tg = inr ? a.target[b * a.ts0 + t * a.ts1] : 0;
        const bool kept = inr && !(a.has_ignore && tg == a.ignore_index);
        if (!__any(kept)) continue;  // wave-uniform: nothing of these rows is read
        const bool ok = kept && tg >= 0 && tg < V;
        const T_* __restrict__ p = preds + (b * a.ps0 + t * a.ps1);
        const float xt = ok ? ld_f32(p, tg) : 0.0f;

        // virtual lane q of lane l folds the elements l + LPR*q + 64*k
        float m[Q], s[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) { m[q] = -FLT_MAX; s[q] = 0.0f; }
        for (int base = 0; base < V; base += 256) {
#pragma unroll
            for (int q = 0; q < Q; q++) {
                float f[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int e = base + j * 64 + q * LPR + l;
                    f[j] = (kept && e < V) ? ld_f32(p, e) : -INFINITY;
                }
                lm_fold<4>(f, m[q], s[q]);
            }
        }
        softmax_merge_group<LPR>(m, s);  // all 64 lanes; the group's first lane holds the row
        const double v = (l == 0 && kept) ? lm_row_value(ok, m[0], s[0], xt) : 0.0;
#pragma unroll
        for (int gg = 0; gg < Q; gg++) {
            const double vg = __shfl(v, gg * LPR);
            const int kg = __shfl((int)kept, gg * LPR);
            if (kg) { acc += vg; cnt++; }
        }
    }
    lm_store_block<LM_WAVES>(acc, cnt, wave, lane, sh_acc, sh_cnt, a.slab);
}

// ---- mappings 2 and 3: NW waves stream a row (1: each wave of the block its own) ----
template <typename T_, int NW, int DEPTH>
__global__ void __launch_bounds__(NW == 1 ? LM_BLOCK : 64 * NW) k_lm_nll_stream(const LmArgs a) {
    constexpr int NWAVES = NW == 1 ? LM_WAVES : NW;  // waves of the block
    constexpr int EPV = 16 / sizeof(T_);
    constexpr int STRIDE = 64 * NW;  // vectors one trip of the row's waves covers
    __shared__ double sh_acc[NWAVES];
    __shared__ ull sh_cnt[NWAVES];
    __shared__ float sh_m[NWAVES], sh_s[NWAVES];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const T_* __restrict__ preds = static_cast<const T_*>(a.preds);
    const int V = a.V;
    double acc = 0.0;
    ull cnt = 0;

    for (ll grp = blockIdx.x; grp < a.n_groups; grp += gridDim.x) {
        const ll row = NW == 1 ? grp * LM_WAVES + wave : grp;
        if (row >= a.rows) continue;
        const ll b = row / a.T, t = row % a.T;
        const ll tg = a.target[b * a.ts0 + t * a.ts1];
        if (a.has_ignore && tg == a.ignore_index) continue;  // uniform over the row's waves: no load
        const bool ok = tg >= 0 && tg < V;
        const T_* __restrict__ p = preds + (b * a.ps0 + t * a.ps1);
        const float xt = ok ? ld_f32(p, tg) : 0.0f;

        // [0, head) up to the first 16-byte boundary, nvec whole vectors, tail
        int head = (int)(((16u - (unsigned int)((uintptr_t)p & 15u)) & 15u) / sizeof(T_));
        head = head < V ? head : V;
        const int nvec = (V - head) / EPV;
        const int tail = V - head - nvec * EPV;
        const lm_u32x4* __restrict__ pv = reinterpret_cast<const lm_u32x4*>(p + head);

        float m = -FLT_MAX, s = 0.0f;
        if (NW == 1 || wave == 0) {  // the peeled elements, one per lane (head + tail < 2 * EPV)
            const int i = lane < head ? lane : head + nvec * EPV + (lane - head);
            const float f[1] = {lane < head + tail ? ld_f32(p, i) : -INFINITY};
            lm_fold<1>(f, m, s);
        }
        for (int v0 = NW == 1 ? 0 : wave * 64; v0 < nvec; v0 += STRIDE * DEPTH) {
            lm_u32x4 raw[DEPTH];
            if (v0 + STRIDE * (DEPTH - 1) + 64 <= nvec) {  // wave-uniform: every lane of every load is inside
#pragma unroll
                for (int d = 0; d < DEPTH; d++) raw[d] = __builtin_nontemporal_load(pv + (v0 + d * STRIDE + lane));
            } else {
#pragma unroll
                for (int d = 0; d < DEPTH; d++) {
                    const int v = v0 + d * STRIDE + lane;
                    raw[d] = v < nvec ? __builtin_nontemporal_load(pv + v) : lm_neg_inf<T_>();
                }
            }
            lm_fold_vectors<T_, DEPTH>(raw, m, s);
        }
        softmax_merge_wave(m, s);  // lane 0 holds the wave's pair
        if constexpr (NW > 1) {
            if (lane == 0) { sh_m[wave] = m; sh_s[wave] = s; }
            __syncthreads();
            if (wave == 0) {
                for (int w = 1; w < NW; w++) softmax_merge_step(m, s, sh_m[w], sh_s[w]);
            }
            __syncthreads();  // the pairs are written again for the next row
        }
        if (lane == 0 && (NW == 1 || wave == 0)) {
            acc += lm_row_value(ok, m, s, xt);
            cnt++;
        }
    }
    lm_store_block<NWAVES>(acc, cnt, wave, lane, sh_acc, sh_cnt, a.slab);
}

// one lane: the slab entries in index order, then the sums or the states
__global__ void __launch_bounds__(64) k_lm_nll_tail(const double* __restrict__ slab, int grid, int dtype,
                                                    float* __restrict__ total, float* __restrict__ count,
                                                    double* __restrict__ sums) {
    if (threadIdx.x != 0) return;
    double t = 0.0;
    ull n = 0;
#pragma unroll 8
    for (int b = 0; b < grid; b++) {
        t += slab[2 * b];
        n += reinterpret_cast<const ull*>(slab)[2 * b + 1];
    }
    if (sums) {
        sums[0] = t;
        sums[1] = (double)n;
        return;
    }
    float r = (float)t;  // torch's .to(preds.dtype) from fp64 goes through fp32 as well
    if (dtype == 1) {
        unsigned int u = __float_as_uint(r);
        if (r == r) u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;  // round to nearest even; NaN stays NaN
        r = __uint_as_float(u);
    } else if (dtype == 2) {
        r = (float)(_Float16)r;
    }
    total[0] += r;
    count[0] += (float)n;
}

// ---- host: the layout of a call, a function of rows and V ----
struct LmLayout {
    int mapping, lpr, rpw, rpb, grid;
    ll n_groups;
};

// Cap of the row kernels' grid, knob MA_LM_NLL_GRID, read at every call and
// clamped to the slab: a small cap makes every block wrap with few rows.
static int lm_grid_cap() {
    const char* e = getenv("MA_LM_NLL_GRID");
    int cap = e ? atoi(e) : LM_GRID_MAX;
    if (cap < 1) cap = 1;
    return cap > LM_GRID_MAX ? LM_GRID_MAX : cap;
}

static int lm_depth() {
    const char* e = getenv("MA_LM_NLL_DEPTH");
    const int d = e ? atoi(e) : LM_DEPTH_DEFAULT;
    return d == 8 ? 8 : 4;
}

static bool lm_layout(ll rows, ll V, int dtype, LmLayout* o) {
    if (dtype < 0 || dtype > 2 || rows < 1 || rows >= (1LL << 40) || V < 1 || V > LM_MAX_V) return false;
    if (V <= LM_G32_V) {
        o->mapping = 1;
        o->lpr = V <= LM_G16_V ? 16 : 32;
        o->rpw = 64 / o->lpr;
        o->rpb = LM_WAVES * o->rpw;
    } else if (rows < LM_BLOCK_ROWS && V > LM_BLOCK_V) {
        o->mapping = 3;
        o->lpr = 64;
        o->rpw = 1;
        o->rpb = 1;
    } else {
        o->mapping = 2;
        o->lpr = 64;
        o->rpw = 1;
        o->rpb = LM_WAVES;
    }
    o->n_groups = (rows + o->rpb - 1) / o->rpb;
    const int cap = lm_grid_cap();
    o->grid = (int)(o->n_groups < cap ? o->n_groups : cap);
    return true;
}

template <typename T_>
static void lm_launch(hipStream_t s, const LmLayout& lay, const LmArgs& a) {
    if (lay.mapping == 1) {
        if (lay.lpr == 16) k_lm_nll_group<T_, 16><<<lay.grid, LM_BLOCK, 0, s>>>(a);
        else k_lm_nll_group<T_, 32><<<lay.grid, LM_BLOCK, 0, s>>>(a);
    } else if (lay.mapping == 2) {
        if (lm_depth() == 8) k_lm_nll_stream<T_, 1, 8><<<lay.grid, LM_BLOCK, 0, s>>>(a);
        else k_lm_nll_stream<T_, 1, 4><<<lay.grid, LM_BLOCK, 0, s>>>(a);
    } else {
        if (lm_depth() == 8) k_lm_nll_stream<T_, LM_ROW_WAVES, 8><<<lay.grid, 64 * LM_ROW_WAVES, 0, s>>>(a);
        else k_lm_nll_stream<T_, LM_ROW_WAVES, 4><<<lay.grid, 64 * LM_ROW_WAVES, 0, s>>>(a);
    }
}

extern "C" {

// Host only: what a call over `rows` rows of V elements does. out = {mapping
// (1 group, 2 wave, 3 block), lanes per row, rows per wave, rows per block and
// pass, blocks of the row kernel, slab entries (of 16 bytes each), the last V
// of the group mapping, the last V of the wave mapping at this row count, the
// largest V covered, the row count from which the block mapping is off}. The
// constants are written for any arguments. -103: shape or dtype not covered.
int ma_lm_nll_layout(ll rows, ll V, int dtype, ll* out) {
    out[5] = LM_GRID_MAX;
    out[6] = LM_G32_V;
    out[7] = rows < LM_BLOCK_ROWS ? LM_BLOCK_V : LM_MAX_V;
    out[8] = LM_MAX_V;
    out[9] = LM_BLOCK_ROWS;
    LmLayout lay;
    if (!lm_layout(rows, V, dtype, &lay)) return -103;
    out[0] = lay.mapping;
    out[1] = lay.lpr;
    out[2] = lay.rpw;
    out[3] = lay.rpb;
    out[4] = lay.grid;
    return 0;
}

// The NLL sums of one (B, T, V) batch. With `sums` set, [total, count] are
// written there as two fp64; otherwise they are added into the one-element
// fp32 states `total` and `count`, the total rounded to the dtype of preds
// first. Strides in elements; `slab` holds LM_GRID_MAX entries of 16 bytes.
// Two launches on one stream. -103 for a shape or dtype the kernels do not
// cover, a missing buffer or a misaligned address; nothing is launched then.
int ma_lm_nll(uintptr_t stream, uintptr_t preds, int dtype /*0=f32 1=bf16 2=f16*/, uintptr_t target, ll B, ll T,
              ll V, ll ps0, ll ps1, ll ts0, ll ts1, ll ignore_index, int has_ignore, uintptr_t slab,
              uintptr_t total, uintptr_t count, uintptr_t sums) {
    if (dtype < 0 || dtype > 2 || B < 1 || T < 1 || B >= (1LL << 40) || T >= (1LL << 40)) return -103;
    if (!preds || !target || !slab || slab % 16 || (!sums && (!total || !count))) return -103;
    if (ps0 < 0 || ps1 < 0 || ts0 < 0 || ts1 < 0) return -103;
    const int esize = dtype == 0 ? 4 : 2;
    if (preds % esize || target % sizeof(ll) || sums % sizeof(double) || total % 4 || count % 4) return -103;
    LmLayout lay;
    if (!lm_layout(B * T, V, dtype, &lay)) return -103;
    LmArgs a;
    a.preds = (const void*)preds;
    a.target = (const ll*)target;
    a.rows = B * T;
    a.T = T;
    a.ps0 = ps0; a.ps1 = ps1; a.ts0 = ts0; a.ts1 = ts1;
    a.ignore_index = ignore_index;
    a.n_groups = lay.n_groups;
    a.V = (int)V;
    a.has_ignore = has_ignore;
    a.slab = (double*)slab;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == 0) lm_launch<float>(s, lay, a);
    else if (dtype == 1) lm_launch<unsigned short>(s, lay, a);
    else lm_launch<_Float16>(s, lay, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    k_lm_nll_tail<<<1, 64, 0, s>>>((const double*)slab, lay.grid, dtype, (float*)total, (float*)count,
                                   (double*)sums);
    return (int)hipGetLastError();
}

}  // extern "C"
