// One-pass update for the fused multiclass collection plan (gfx950).
//
// The two-kernel path reads the (B, C) logits twice: k_mc_stat_logits (argmax,
// tp/fp/fn/confmat, online-softmax row stats, out-of-range epoch flag) and
// then k_multiclass_curve_hist, which has to wait for a kernel boundary
// because "softmax iff ANY element of the batch lies outside [0,1]" is a
// batch-global decision. Here a wave owns a row (or 64 / LPR rows, see ROW
// GROUPS in front of the kernel) and keeps the whole row in registers (16 B
// per lane per vector, NV vectors per lane), so the row is read from HBM once:
//
//  phase A  what k_mc_stat_logits does: both call softmax_fold /
//           softmax_merge_wave (softmax_merge_group here: the same tree
//           for a row held by fewer lanes) and count_row of row_fold.h (8-wide groups for
//           bf16, 4-wide for fp32), so rowmax/rowinv are bit-identical to the
//           two-kernel path by construction. The argmax is taken by value
//           first and index after (wave_max_f32, row_argmax_index,
//           wave_min_u32), which the register-held row allows; the streaming
//           kernel carries (value, index) through argmax_fold /
//           argmax_merge_wave. Both implement one exact rule — largest
//           non-NaN value, lowest index on a tie — so the counts agree by
//           specification (tests/unittests/gpu/test_row_argmax_edges.py).
//           TOP-K SLOT (template parameter TOPK, optional): a second stat
//           group whose effective prediction is the target if its logit ranks
//           inside the top k, else the argmax. Only the rank is missing: x[t]
//           comes out of the registers that hold the row (row_element), one
//           compare-and-count over the unpacked values and one wave sum give
//           it, lane 0 counts into a second scratch next to count_row, the
//           tail applies that scratch with the same valid.
//  phase B  CERTAINTY RULE: if this row itself holds an element outside
//           [0,1], the batch-global answer is already known to be "softmax",
//           and the row is binned from registers right away. A row with every
//           element in [0,1] cannot know the answer; it is DEFERRED to the
//           tail kernel, which runs behind this one and bins exactly those
//           rows. There is no grid-wide barrier anywhere.
//
// TWO LAUNCHES PER STEP. k_mc_onepass ends with ONE 16-byte record per block
// (valid, binned, deferred + the block's "outside" bit, correct) instead of
// atomics on single global words: 1024 blocks finishing together on three
// words serialise, plus one flag byte (deferred a row / outside).
// k_onepass_tail reads them across the kernel boundary; every one of its
// blocks ORs all flag bytes and so knows whether rows wait and the softmax
// decision on its own, the blocks with an epilogue slice also sum the records
// for the batch-global counts — no epoch flag, no ticket, no wait. Its first ceil(C/256) blocks each apply a class slice of
// the epilogue, block 0 also the scalars and the epoch bump, and when rows
// were deferred all blocks grid-stride over the (class-chunk, 256-row) tiles
// of the deferred pass (curve_hist_tile, shared with kernels.hip).
//
// PENDING-b0 HISTOGRAM: after softmax almost every element of a row falls into
// one bucket b0 = bucket_of(+0.0f). Those elements issue no atomic at all, and
// nothing counts them per step either: the histogram is lazy (nobody reads it
// between two flushes), so between flushes it may lack exactly the b0 elements
// of the rows k_mc_onepass binned from registers. Two per-class u64 vectors in
// the curve scratch, cumulative since the last flush, carry what is missing:
//     P[c]  non-ignored rows binned so far (either kernel) whose target is c
//     R[c]  non-ignored rows binned so far (the same number in every slot;
//           per class so that no word is shared between blocks)
// Every such row adds one element to class c, label 1 if its target is c, so at
// any kernel boundary after a step
//     P[c]          - sum_j hist[c][j][1]   is still owed to hist[c][b0][1]
//     (R[c] - P[c]) - sum_j hist[c][j][0]   is still owed to hist[c][b0][0]
// exact integer identities (class total minus what is there). The flush
// (k_curve_resolve_pending in kernels.hip, in front of the suffix kernel) pays
// both and zeroes P and R, so the flushed histogram equals the two-kernel
// result bit for bit. Per step this leaves one atomic per element outside b0
// and one per row, where a per-step complement needed a second per element.
// P is not tp + fn of the stat scratch: count_row rejects a row whose argmax is
// out of range (an all-NaN row), yet that row is binned.
//
// A done row (binned or ignored) is marked rowinv[row] = -rinv; a true rinv is
// always > 0, so the sign is free. A rinv that is not > 0 (NaN, 0) is marked
// -1: the tail only tests the sign of a done row.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "curve_common.h"
#include "mc_step.h"
#include "row_fold.h"

#define WAVE 64

typedef long long ll;
typedef unsigned long long ull;

// curve scratch layout (u64): [P: C][R: C][records: 2 x GRID_MAX][flags: GRID_MAX / 8]
// P and R: see PENDING-b0 above; zeroed by the flush, never by a step.
// records: one uint4 per k_mc_onepass block, {valid, binned, deferred | outside
// << 31, correct}. Never zeroed: every launched block overwrites its own record
// every step and the tail kernel reads exactly `grid` of them. The region
// starts 16*C bytes into the 16-byte aligned scratch, so it is 16-byte aligned.
#define ONEPASS_GRID_MAX 1024  // records the scratch holds = cap of MA_ONEPASS_GRID
#define ONEPASS_REC_OFF(C) (2 * (C))
// flags: one byte per k_mc_onepass block behind the records, bit 0 = the block
// deferred a row, bit 1 = its "outside" bit: all a tail block without an
// epilogue slice needs, 1 KB instead of the 16 KB of records. Overwritten every
// step like the records; the tail reads exactly `grid` of them.
#define ONEPASS_FLAG_OFF(C) (ONEPASS_REC_OFF(C) + 2 * ONEPASS_GRID_MAX)
#define ONEPASS_CS_WORDS(C) (ONEPASS_FLAG_OFF(C) + ONEPASS_GRID_MAX / 8)
#define ONEPASS_TAIL_GRID_DEFAULT 4096  // blocks of k_onepass_tail, see onepass_step
// defaults of the row-group mapping and the grid cap, see onepass_lpr / onepass_grid_cap
// (sweep in profiles/README.md, "Row groups": more rows per wave save vector
// instructions but no time, the prefetch with twice the tasks per wave does)
#define ONEPASS_LPR_DEFAULT(nv) 64
#define ONEPASS_GRID_DEFAULT(prefetch) ((prefetch) ? 512 : 1024)
// the second row buffer of the prefetch costs 4 registers per vector: only for
// slices of up to 4 vectors per lane, 2 with the top-k slot (nothing may spill)
#define ONEPASS_PF_MAX_NVL 4
#define ONEPASS_PREFETCH_DEFAULT 1

// TOPK: the optional top-k stat slot (second scratch tp2|fp2|fn2, see
// count_row_topk). A template parameter, so the instantiation without the slot
// is the kernel it was before the slot existed.
//
// ROW GROUPS (template parameter LPR, lanes per row, 16 / 32 / 64): a row of
// NV <= 2 vectors per lane is too short for a wave — the merges, the two
// reductions, the first-lane section and every binning round cost the same
// for 64 lanes as for 16. So a wave owns G = 64 / LPR consecutive rows at
// once, one per group of LPR lanes (a 16-lane DPP row, a half wave, or the
// wave: LPR = 64 is the one-row-per-wave kernel). Lane l of group g holds the
// vectors l + LPR*j, j < NV*G, of row row0 + g. rowmax / rowinv keep their
// bits through the virtual-lane order of softmax_merge_group (row_fold.h);
// max, min, OR and the integer sums do not depend on the order. What was
// wave-uniform per row (target, row statistics, argmax, ignored / certain /
// bin_now, the rank) is per group now, i.e. a vector register; the cross-lane
// steps never leave a group, and a group whose row lies past B holds zeros,
// counts nothing, stores nothing and bins nothing while its lanes still take
// part in every step.
// Launch bounds = the waves per SIMD the grid really produces: at most 1024
// blocks of 4 waves on 256 CUs, i.e. 4, which leaves 128 registers. NV = 8
// needs more than 128 (3 waves), and so does the top-k slot on top of an
// 8-vector slice (2). No instantiation needs scratch; without the top-k slot
// none spills a scalar either, four with it spill 4-6 scalars to lanes
// (profiles/README.md, "Row groups").
#define ONEPASS_WAVES(NV, TOPK, LPR) ((NV) > 4 ? 3 : ((TOPK) && (NV) * (WAVE / (LPR)) == 8) ? 2 : 4)
//
// PREFETCH (template parameter PF): loads, stores and atomics of a wave share
// one in-order counter, so a wait for the next task's row is also a wait for
// every histogram atomic issued before it, and those take microseconds when
// the whole chip issues them. With PF the next task's row and target are
// requested into a second register buffer BEFORE phase A of the current one,
// and the wave waits for them once, behind phase A and in front of its own
// atomics: by then the previous task's atomics have had a whole phase A to
// drain, and the ones it issues next are waited for by nobody until the next
// task's phase A is done.
template <typename T_, int NV, bool TOPK, int LPR, bool PF>
__global__ void __launch_bounds__(256, ONEPASS_WAVES(NV, TOPK, LPR)) k_mc_onepass(
    const uint4* __restrict__ preds, const ll* __restrict__ target, ll B, ll C, ll ignore_index,
    int has_ignore, ull* __restrict__ counts /* [tp|fp|fn]: 3*C */,
    ull* __restrict__ confmat, float* __restrict__ rowmax, float* __restrict__ rowinv,
    const float* __restrict__ thresholds, int T, int uniform, float t0, float inv_step,
    ull* __restrict__ hist /* (C, T+1, 2) */,
    ull* __restrict__ cs /* curve scratch [P|R|records|flags]: P cumulative, one record and flag per block */,
    int topk, ull* __restrict__ counts2 /* [tp2|fp2|fn2]: 3*C, TOPK only */) {
    constexpr int EPV = 16 / sizeof(T_);  // elements per 16-byte vector
    constexpr int G = WAVE / LPR;         // rows per wave = virtual lanes per lane
    constexpr int NVL = NV * G;           // vectors per lane
    static_assert(NVL <= 8, "the row slice of a lane is at most 8 vectors (32 registers, 64 todo bits)");
    extern __shared__ float sthr[];
    __shared__ unsigned int block_valid, blk_outside, blk_binned, blk_deferred, blk_correct;

    const int lane = threadIdx.x & (WAVE - 1);
    const int l = lane & (LPR - 1);                // lane inside the group
    const int g = LPR == WAVE ? 0 : lane / LPR;    // group = row of the wave's task
    // wave-uniform by construction; tell the compiler, so the row index and
    // everything derived from it live in scalar registers
    const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int waves_per_block = blockDim.x / WAVE;
    const ll row_stride = (ll)gridDim.x * waves_per_block * G;
    const int nvec = (int)(C / EPV);  // C <= 4096 here: 32-bit class indices
    unsigned int outside = 0;
    unsigned int my_valid = 0, my_binned = 0, my_deferred = 0, my_correct = 0;

    // the group's whole row, packed, in registers: vector j of this lane is
    // pv[l + LPR*j]; a group past B holds zeros
    uint4 r[NVL];
    uint4 rn[PF ? NVL : 1];  // PF: the next task's row
    ll t_next = 0;           // PF: and its target
    auto load_row = [&](uint4* dst, ll row) {
        const bool live = LPR == WAVE || row < B;
        const uint4* pv = preds + row * (ll)nvec;
#pragma unroll
        for (int j = 0; j < NVL; j++) {
            const int v = l + j * LPR;
            dst[j] = (live && v < nvec) ? pv[v] : make_uint4(0u, 0u, 0u, 0u);
        }
    };
    auto load_target = [&](ll row) { return (LPR == WAVE || row < B) ? target[row] : 0; };
    // the first rows' loads are in flight while the block stages the thresholds
    ll row0 = ((ll)blockIdx.x * waves_per_block + wave_in_block) * G;  // first row of the wave's task
    if (row0 < B) {
        load_row(r, row0 + g);
        if constexpr (PF) t_next = load_target(row0 + g);
    }
    for (int b = threadIdx.x; b < T; b += blockDim.x) sthr[b] = thresholds[b];
    if (threadIdx.x == 0) { block_valid = 0; blk_outside = 0; blk_binned = 0; blk_deferred = 0; blk_correct = 0; }
    __syncthreads();
    const int b0 = bucket_of(0.0f, sthr, T);
    const float hi0 = b0 < T ? sthr[b0] : INFINITY;  // bucket b0 is [thr[b0-1], thr[b0])
    // PF: the first row is waited for here, so that inside the loop nothing of
    // the current row is ever pending and the only wait is the explicit one
    if constexpr (PF) __builtin_amdgcn_s_waitcnt(0x0F70);

    while (row0 < B) {
        const ll row = row0 + g;
        const bool live = LPR == WAVE || row < B;
        ll t;
        if constexpr (PF) {
            t = t_next;
            if (row0 + row_stride < B) {
                load_row(rn, row0 + row_stride + g);
                t_next = load_target(row0 + row_stride + g);
            }
        } else {
            t = live ? target[row] : 0;
        }

        // ---- phase A: the folds of k_mc_stat_logits (row_fold.h) ----
        // The row stays in registers, so the argmax index need not ride
        // through the fold: the fold keeps the lane's largest value (not the
        // softmax m, which starts at -3.4e38 rather than -inf), the index is
        // looked up once the row's maximum is known. One (max, sumexp) pair
        // per virtual lane q; vector j = q + G*k is vector L + 64*k of virtual
        // lane L = l + LPR*q, folded for k = 0, 1, ... as that lane would.
        float best = -INFINITY;
        float sm_m[G], sm_s[G];  // online softmax (max, sumexp)
#pragma unroll
        for (int q = 0; q < G; q++) { sm_m[q] = -3.4e38f; sm_s[q] = 0.0f; }
        unsigned int row_out = 0;
#pragma unroll
        for (int k = 0; k < NV; k++) {
#pragma unroll
            for (int q = 0; q < G; q++) {
                const int v = l + (q + G * k) * LPR;
                if (v < nvec) {
                    float f[EPV];
                    unpack16<T_>(r[q + G * k], f);
                    best = fmaxf(best, softmax_fold(f, sm_m[q], sm_s[q], row_out));
                }
            }
        }
        // an ignored row takes no part in the softmax decision (the reference
        // drops ignored samples before the range test); t is already loaded
        const bool ignored = live && has_ignore && t == ignore_index;
        if (ignored || !live) row_out = 0u;
        outside |= row_out;
        softmax_merge_group<LPR>(sm_m, sm_s);
        const float rowbest = group_max_f32<LPR>(best);
        const unsigned int best_idx =
            group_min_u32<LPR>(row_argmax_index<T_, NVL, LPR>(r, l, nvec, rowbest));  // 0x7fffffff: all NaN
        // the group's first lane holds the row's (max, sumexp); every lane of
        // the group needs them for phase B. All 64 lanes are active here.
        const float rmax = group_first<LPR>(sm_m[0]);
        const float rsum = group_first<LPR>(sm_s[0]);
        const float rinv = 1.0f / rsum;
        // this row alone proves "softmax": the group's slice of the ballot
        const ull any_out = __ballot(row_out != 0u);
        bool certain;
        if constexpr (LPR == WAVE) certain = any_out != 0ULL;
        else certain = ((any_out >> (g * LPR)) & ((1ULL << LPR) - 1ULL)) != 0ULL;
        const bool bin_now = certain && !ignored && live;
        // ---- top-k slot: rank of x[t] among the row, from the registers ----
        // Needed only for a valid row whose argmax is not the target (a == t
        // means rank 0); the count is skipped when no group of the wave needs
        // it, and a group that does not need it sees rank 0, which gives the
        // same counts.
        unsigned int rank = 0;
        if constexpr (TOPK) {
            const bool need = live && !ignored && t >= 0 && t < C && best_idx < (unsigned int)C && (ll)best_idx != t;
            if (__ballot(need) != 0ULL) {
                const int te = need ? (int)t : 0;
                const float xt = row_element<T_, NVL, LPR>(r, te, lane);
                unsigned int cnt = 0;
#pragma unroll
                for (int j = 0; j < NVL; j++) {
                    const int v = l + j * LPR;
                    if (v < nvec) {
                        float f[EPV];
                        unpack16<T_>(r[j], f);
                        rank_fold(f, v * EPV, xt, te, cnt);
                    }
                }
                cnt = group_sum_u32<LPR>(need ? cnt : 0u);  // the group's first lane holds the row's rank
                rank = need ? cnt : 0u;
            }
        }
        // PF: the one wait of the task (vmcnt(0) alone), see PREFETCH above
        if constexpr (PF) __builtin_amdgcn_s_waitcnt(0x0F70);
        if (l == 0 && live) {
            const ll p = (ll)best_idx;
            if (count_row(t, p, C, ignored, counts, counts + C, counts + 2 * C, confmat)) {
                my_valid++;
                if (p == t) my_correct++;
                if constexpr (TOPK) count_row_topk(t, p, rank, topk, counts2, counts2 + C, counts2 + 2 * C);
            }
            rowmax[row] = rmax;
            // the done mark must compare < 0 whatever rinv is: a row with a NaN
            // next to an element outside [0,1] has rinv = NaN, an infinite sum
            // gives 0, and the tail would bin such a row a second time
            rowinv[row] = (bin_now || ignored) ? (rinv > 0.0f ? -rinv : -1.0f) : rinv;
            if (bin_now) {
                my_binned++;
                if (t >= 0 && t < C) atomicAdd(&cs[t], 1ULL);  // P[t]
            } else if (!ignored) {
                my_deferred++;
            }
        }

        // ---- phase B: bin from registers; bucket b0 stays pending until the flush ----
        // bit j*EPV+i: element i of vector j needs the full path; 32 bits hold
        // it for a slice of up to 32 elements. A lane whose row is not binned
        // now keeps an empty queue.
        typedef typename std::conditional<(EPV * NVL <= 32), unsigned int, ull>::type todo_t;
        todo_t todo = 0;
        // out-of-range targets bin with every label 0, like the two-kernel path
        const int tc = (t >= 0 && t < C) ? (int)t : -1;
        if (bin_now) {
            // EXACT pre-filter in the logit domain. p = expf(d) * rinv with
            // d = x - rmax; bucket(p) == b0 <=> thr[b0-1] <= p < thr[b0].
            // The left half always holds (thr[b0-1] <= 0 <= p). For the right
            // half: d < log(hi0 * sumexp) - 1e-3 gives exp(d) * rinv <
            // hi0 * e^-1e-3, and the rounding of logf, expf and the product
            // (a few 1e-7 relative, 1e-5 absolute on the log) is far inside
            // the 1e-3 margin — such an element is certainly in b0 and costs
            // a subtract and a compare. Everything else, NaN included (the
            // compare is false), goes through expf and bucket_of unchanged.
            // The filter only has to be SAFE (an element it lets through is
            // binned exactly all the same), so the subtract is hoisted out of
            // the element loop: x < xcut with xcut = fl(rmax + dcut) lowered
            // by 2^-22 |rmax|. fl() is off by at most 2^-24 (|rmax| + |dcut|):
            // the |rmax| share is covered by the lowering (four times as
            // large, its own rounding included), the |dcut| share (|dcut| <
            // 100: below 1e-5) by the 1e-3 margin. rmax = +inf or a NaN sum
            // make xcut NaN: every compare false, every element takes the
            // full path.
            const float dcut = logf(hi0 * rsum) - 1e-3f;
            const float xcut = (rmax + dcut) - fabsf(rmax) * 2.4e-7f;
#pragma unroll
            for (int j = 0; j < NVL; j++) {
                if (l + j * LPR < nvec) {
                    float f[EPV];
                    unpack16<T_>(r[j], f);
#pragma unroll
                    for (int i = 0; i < EPV; i++)
                        todo |= (f[i] < xcut) ? (todo_t)0 : ((todo_t)1 << (j * EPV + i));
                }
            }
        }
        // compacted: every lane pops one pending element per round, so a wave
        // task costs max-over-lanes(popcount) rounds for all its rows together
        while (__ballot(todo != 0) != 0ULL) {
            if (todo != 0) {
                int e;
                if constexpr (sizeof(todo_t) == 4) e = __ffs((int)todo) - 1;
                else e = __ffsll((ull)todo) - 1;
                todo &= todo - 1;
                const int wi = is_bf16_v<T_> ? (e >> 1) : e;  // 32-bit word of the row slice
                const unsigned int w = row_slice_word<NVL>(r, wi);
                const float x = is_bf16_v<T_> ? __uint_as_float((e & 1) ? (w & 0xffff0000u) : (w << 16))
                                        : __uint_as_float(w);
                const int j = e / EPV, i = e % EPV;
                const int c = (l + j * LPR) * EPV + i;
                const float p = expf(x - rmax) * rinv;
                const int b = uniform ? bucket_of_uniform(p, sthr, T, t0, inv_step)
                                      : bucket_of(p, sthr, T);
                if (b != b0) {
                    const int label = (tc == c) ? 1 : 0;
                    atomicAdd(&hist[(ull)c * (T + 1) * 2 + b * 2 + label], 1ULL);
                }
            }
        }
        row0 += row_stride;
        if constexpr (PF) {
#pragma unroll
            for (int j = 0; j < NVL; j++) r[j] = rn[j];
        } else {
            if (row0 < B) load_row(r, row0 + g);  // r is dead here: same registers
        }
    }
    // the block's counts meet in LDS; nothing here touches a shared global word
    if (my_valid) atomicAdd(&block_valid, my_valid);
    if (my_binned) atomicAdd(&blk_binned, my_binned);
    if (my_deferred) atomicAdd(&blk_deferred, my_deferred);
    if (my_correct) atomicAdd(&blk_correct, my_correct);
    or_outside_block(outside, &blk_outside);
    __syncthreads();
    if (threadIdx.x == 0) {
        // one 16-byte store; a block holds < 2^31 rows, so bit 31 is free
        uint4* records = (uint4*)(cs + ONEPASS_REC_OFF(C));
        unsigned char* flags = (unsigned char*)(cs + ONEPASS_FLAG_OFF(C));
        records[blockIdx.x] = make_uint4(block_valid, blk_binned,
                                         blk_deferred | (blk_outside << 31), blk_correct);
        flags[blockIdx.x] = (unsigned char)((blk_deferred ? 1u : 0u) | (blk_outside ? 2u : 0u));
    }
}

// Tail of the one-pass step, the second and last launch. Every block:
//  (a) ORs the `grid` per-block flag bytes of k_mc_onepass (<= 1 KB, L2) and
//      so knows whether any row was deferred and the softmax decision. Only
//      the first ceil(C/256) blocks, which own an epilogue slice, also sum the
//      16-byte records (<= 16 KB) for valid / binned / correct: with 4096
//      blocks that is 4 MB of L2 reads per step in place of 64 MB;
//  (b) applies the epilogue for class blockIdx.x*256 + threadIdx.x, if there
//      is one: k_apply_stat_exact's stat deltas, and R[class] += the step's
//      binned + deferred rows (a plain add: the thread is the only writer of
//      its slot). Each slot of the stat scratches is read and zeroed by the
//      same thread. No histogram word is touched here. Block 0 also applies
//      the exact-match scalars and closes the device epoch — at once, since no
//      block of this kernel reads E: the softmax decision is `outside`;
//  (c) returns if nothing was deferred (every logits input), else grid-strides
//      over the (class-chunk, 256-row) tiles of the deferred pass. A deferred
//      row adds all its elements, b0 included; the chunk-0 tile of each row
//      tile adds 1 to P[target] for every row the tiles bin (the tile's own
//      condition), so each such row is counted exactly once.
// Nothing written by one block is read by another; there is no ticket, spin
// or grid-wide wait.
template <typename T_, bool TOPK>
__global__ void __launch_bounds__(256) k_onepass_tail(
    const uint4* __restrict__ records, const unsigned char* __restrict__ flags,
    int grid /* blocks k_mc_onepass ran with */,
    ull* __restrict__ scratch /* 3*C + 1 */, ll C, ll B, ll* __restrict__ tp, ll* __restrict__ fp,
    ll* __restrict__ tn, ll* __restrict__ fn, ll* __restrict__ correct /* nullable */,
    ll* __restrict__ total, unsigned int* __restrict__ E, ull* __restrict__ cs /* [P: C][R: C] */,
    const float* __restrict__ thresholds, int T, ull* __restrict__ hist /* (C, T+1, 2) */,
    const T_* __restrict__ probs, const ll* __restrict__ target, ll ignore_index, int has_ignore,
    int uniform, float t0, float inv_step, int c_chunk, const float* __restrict__ rowmax,
    const float* __restrict__ rowinv, ull* __restrict__ scratch2 /* 3*C, TOPK only */,
    ll* __restrict__ tp2, ll* __restrict__ fp2, ll* __restrict__ tn2, ll* __restrict__ fn2) {
    extern __shared__ float sthr_t[];  // a global-memory binary search is ~8 dependent misses
    __shared__ unsigned int wsum[256 / WAVE][5];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    // block-uniform: this block owns classes blockIdx.x*256 ... (block 0 always does)
    const bool has_slice = (ll)blockIdx.x * blockDim.x < C;

    // ---- (a) the batch-global flags; the counts where the epilogue needs them ----
    unsigned int fl = 0;
    for (int i = threadIdx.x; i < grid; i += blockDim.x) fl |= flags[i];
    // r_rows: rows this step bins, here or in k_mc_onepass (B < 2^31: no overflow)
    unsigned int r_valid = 0, r_rows = 0, r_correct = 0;
    if (has_slice) {
        for (int i = threadIdx.x; i < grid; i += blockDim.x) {
            const uint4 r = records[i];
            r_valid += r.x;
            r_rows += r.y + (r.z & 0x7fffffffu);
            r_correct += r.w;
        }
    }
    for (int b = threadIdx.x; b < T; b += blockDim.x) sthr_t[b] = thresholds[b];
    if (has_slice) {
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            r_valid += __shfl_down(r_valid, off);
            r_rows += __shfl_down(r_rows, off);
            r_correct += __shfl_down(r_correct, off);
        }
    }
    const unsigned int wave_fl = (__ballot(fl & 1u) != 0ULL ? 1u : 0u) | (__ballot(fl & 2u) != 0ULL ? 2u : 0u);
    if (lane == 0) {
        wsum[wave][0] = r_valid; wsum[wave][1] = r_rows; wsum[wave][2] = r_correct;
        wsum[wave][3] = wave_fl;
    }
    __syncthreads();
    ll valid = 0, rows = 0;
    unsigned int ncorrect = 0, all_fl = 0;
#pragma unroll
    for (int w = 0; w < 256 / WAVE; w++) {
        valid += wsum[w][0]; rows += wsum[w][1]; ncorrect += wsum[w][2]; all_fl |= wsum[w][3];
    }
    const bool deferred = (all_fl & 1u) != 0;  // some row waits for this kernel
    const unsigned int outside = all_fl >> 1;

    // ---- (b) epilogue for one class ----
    const ll i = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < C) {
        apply_stat_class(scratch, C, i, valid, tp, fp, tn, fn);
        // the top-k slot: the same valid, its own scratch and states
        if constexpr (TOPK) apply_stat_class(scratch2, C, i, valid, tp2, fp2, tn2, fn2);
        if (rows) cs[C + i] += (ull)rows;  // R[i]
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (correct) {
            correct[0] += (ll)ncorrect + (B - valid);  // Σ dtp == the records' correct count
            total[0] += B;
        }
        E[1] += 1u;
    }

    // ---- (c) the deferred rows ----
    if (!deferred) return;
    const int norm = outside ? 1 : 0;  // softmax iff any element of the batch lay outside [0,1]
    // Tile t -> (class chunk, row tile). Blocks go round-robin over the 8 XCDs
    // (each with its own L2) and adjacent class chunks read slices of the SAME
    // cache lines, so XCD x = t % 8 (the grid is a multiple of 8) keeps to a
    // contiguous band of chunks, as k_multiclass_curve_hist does; the
    // c_chunks % 8 leftover chunks come last.
    const ll c_chunks = (C + c_chunk - 1) / c_chunk;
    const ll row_chunks = (B + 255) / 256;
    const ll band = c_chunks / 8;
    const ll rem = c_chunks - band * 8;
    const ll nmain = band * 8 * row_chunks;
    const ll ntiles = c_chunks * row_chunks;
    for (ll t = blockIdx.x; t < ntiles; t += gridDim.x) {
        ll chunk, ry;
        if (t < nmain) {
            const ll u = t >> 3;
            chunk = (t & 7) * band + u % band;
            ry = u / band;
        } else {
            const ll u = t - nmain;
            chunk = band * 8 + u % rem;
            ry = u / rem;
        }
        const ll c_lo = chunk * c_chunk;
        const ll c_hi = min(c_lo + (ll)c_chunk, C);
        curve_hist_tile<T_>(probs, target, B, C, sthr_t, T, ignore_index, has_ignore, /*mode=*/0,
                            uniform, t0, inv_step, c_lo, c_hi, ry * 256, norm, rowmax, rowinv,
                            /*skip_done=*/true, hist);
        // P[target] of the rows the tiles of this row tile bin, under
        // curve_hist_tile's own condition (in range, not ignored, not marked
        // done). Every (chunk, row tile) pair is walked exactly once, so the
        // chunk-0 tile counts each of its 256 rows once; asking every tile
        // whether its chunk holds the target re-read target and rowinv for
        // each of the C/c_chunk chunks (measured: +2 us on all-deferred input)
        if (chunk == 0) {
            const ll prow = ry * 256 + threadIdx.x;
            if (prow < B) {
                const ll pt = target[prow];
                if (pt >= 0 && pt < C && !(has_ignore && pt == ignore_index) &&
                    !(rowinv[prow] < 0.0f))
                    atomicAdd(&cs[pt], 1ULL);
            }
        }
    }
}

extern "C" {

// NV (16-byte vectors per lane of a 64-lane row) the one-pass kernel would
// use, 0 = unsupported shape (caller keeps the two-kernel path). NV in
// {1,2,4,8}: bf16 C <= 1024 and fp32 C <= 512 are NV <= 2. Registers per
// instantiation: profiles/README.md, none with scratch.
int ma_mc_onepass_nv(int dtype /*0=f32 1=bf16*/, ll C, int T) {
    if (C <= 128 || T < 1 || (size_t)T * sizeof(float) > 48 * 1024) return 0;
    const int epv = dtype == 1 ? 8 : 4;
    if (dtype != 0 && dtype != 1) return 0;
    if (C % epv) return 0;
    const ll per_lane = (C / epv + WAVE - 1) / WAVE;
    if (per_lane > 8) return 0;
    int nv = 1;
    while (nv < per_lane) nv *= 2;
    return nv;
}

// u64 words of the curve scratch for C classes (records region included)
int ma_mc_onepass_scratch_words(ll C) { return (int)ONEPASS_CS_WORDS(C); }

static int onepass_lpr(int nv);
// lanes per row a plan created now would run with (MA_ONEPASS_LPR included),
// 0 = unsupported shape
int ma_mc_onepass_lpr(int dtype, ll C, int T) {
    const int nv = ma_mc_onepass_nv(dtype, C, T);
    return nv ? onepass_lpr(nv) : 0;
}

// Lanes per row (LPR) for a kernel of NV vectors per 64-lane row: a lane holds
// NV * 64 / LPR vectors, at most 8, so NV <= 2 may use 16, 32 or 64, NV = 4
// 32 or 64, NV = 8 only 64. Default (sweep in profiles/README.md, "Row
// groups"): one row per wave. Sweep knob MA_ONEPASS_LPR, read whenever a plan
// is created; a value the shape does not support is raised to the next one it
// does.
static int onepass_lpr(int nv) {
    const int min_lpr = nv <= 2 ? 16 : nv <= 4 ? 32 : 64;
    int lpr = ONEPASS_LPR_DEFAULT(nv);
    const char* e = getenv("MA_ONEPASS_LPR");
    if (e) {
        const int v = atoi(e);
        if (v == 16 || v == 32 || v == 64) lpr = v;
    }
    return lpr < min_lpr ? min_lpr : lpr;
}

// Cap of the k_mc_onepass grid, sweep knob MA_ONEPASS_GRID, read whenever a
// plan is created and clamped to the records the scratch holds. A wave task is
// 64 / LPR consecutive rows, a block 4 waves. Measured at B=8192 C=1000 with
// one row per task: 2048 blocks — every row resident at once — run the load,
// fold and binning phases chip-wide in lock step (53 us/step); with 512-1024
// blocks each wave takes several tasks, the waves drift apart and the phases
// overlap (45 us). The prefetch variant wants more tasks per wave still: 512
// blocks (profiles/README.md, "Row groups").
static int onepass_grid_cap(int prefetch) {
    const char* e = getenv("MA_ONEPASS_GRID");
    int gcap = e ? atoi(e) : ONEPASS_GRID_DEFAULT(prefetch);
    if (gcap < 64) gcap = 64;
    if (gcap > ONEPASS_GRID_MAX) gcap = ONEPASS_GRID_MAX;
    return gcap;
}
// blocks of k_mc_onepass for B rows
static int onepass_grid(ll B, int lpr, int gcap) {
    const ll tasks = (B + WAVE / lpr - 1) / (WAVE / lpr);
    ll g = (tasks + 3) / 4;
    if (g > gcap) g = gcap;
    return (int)g;
}

// cap of the tail grid, sweep knob MA_ONEPASS_TAIL_GRID (see onepass_step)
static int onepass_tail_cap() {
    static int tcap = 0;
    if (tcap == 0) {
        const char* e = getenv("MA_ONEPASS_TAIL_GRID");
        tcap = e ? atoi(e) : ONEPASS_TAIL_GRID_DEFAULT;
        if (tcap < 8) tcap = 8;
        if (tcap > 65536) tcap = 65536;
    }
    return tcap;
}

}  // extern "C"

// Everything of a step that stays the same from one step to the next: the
// step record (mc_step.h), copied by value, plus the curve leader's part. The
// caller owns the memory behind the addresses and keeps it alive as long as
// the plan.
struct OnepassPlan {
    McStep st;
    int dtype, nv, T, uniform;
    int lpr, gcap, prefetch;  // lanes per row, grid cap, prefetch: fixed when the plan is created
    float t0, inv_step;
    ull *hist, *cscratch;
    const float* thresholds;
};

template <typename T_, int NV, bool TOPK, int LPR, bool PF>
static void onepass_launch_main(const OnepassPlan& p, hipStream_t s, int grid, const void* preds,
                                const ll* target, ll B) {
    const McStep& st = p.st;
    ull* sc = st.counts;
    ull* sc2 = TOPK ? st.topk_counts : nullptr;
    k_mc_onepass<T_, NV, TOPK, LPR, PF><<<grid, 256, (size_t)p.T * sizeof(float), s>>>(
        (const uint4*)preds, target, B, st.C, st.ignore_index, (int)st.has_ignore, sc, st.confmat,
        st.rowmax, st.rowinv, p.thresholds, p.T, p.uniform, p.t0, p.inv_step, p.hist, p.cscratch,
        (int)st.k, sc2);
}
template <typename T_, bool TOPK>
static void onepass_launch_nv(const OnepassPlan& p, hipStream_t s, int grid, const void* preds,
                              const ll* target, ll B) {
    // (NV, LPR) pairs as onepass_lpr() hands them out
#define ONEPASS_CASE(NV_, LPR_)                                                                    \
    if (p.nv == NV_ && p.lpr == LPR_) {                                                            \
        if constexpr (NV_ * (WAVE / LPR_) <= (TOPK ? ONEPASS_PF_MAX_NVL / 2 : ONEPASS_PF_MAX_NVL)) { \
            if (p.prefetch)                                                                        \
                return onepass_launch_main<T_, NV_, TOPK, LPR_, true>(p, s, grid, preds, target, B); \
        }                                                                                          \
        return onepass_launch_main<T_, NV_, TOPK, LPR_, false>(p, s, grid, preds, target, B);      \
    }
    ONEPASS_CASE(1, 16); ONEPASS_CASE(1, 32); ONEPASS_CASE(1, 64);
    ONEPASS_CASE(2, 16); ONEPASS_CASE(2, 32); ONEPASS_CASE(2, 64);
    ONEPASS_CASE(4, 32); ONEPASS_CASE(4, 64);
    ONEPASS_CASE(8, 64);
#undef ONEPASS_CASE
}
template <typename T_, bool TOPK>
static void onepass_launch_tail(const OnepassPlan& p, hipStream_t s, int tgrid, int grid,
                                const void* preds, const ll* target, ll B, int c_chunk,
                                const uint4* records, const unsigned char* flags) {
    const McStep& st = p.st;
    k_onepass_tail<T_, TOPK><<<tgrid, 256, (size_t)p.T * sizeof(float), s>>>(
        records, flags, grid, st.counts, st.C, B, st.tp, st.fp, st.tn, st.fn, st.correct, st.total,
        st.epoch_buf, p.cscratch, p.thresholds, p.T, p.hist, (const T_*)preds, target,
        st.ignore_index, (int)st.has_ignore, p.uniform, p.t0, p.inv_step, c_chunk,
        (const float*)st.rowmax, (const float*)st.rowinv, st.topk_counts, st.tp_k, st.fp_k,
        st.tn_k, st.fn_k);
}
// the dtype and slot dispatch of both kernels, written once
template <bool TOPK>
static void onepass_launch_main_dt(const OnepassPlan& p, hipStream_t s, int grid, const void* preds,
                                   const ll* target, ll B) {
    if (p.dtype == 0) onepass_launch_nv<float, TOPK>(p, s, grid, preds, target, B);
    else onepass_launch_nv<unsigned short, TOPK>(p, s, grid, preds, target, B);
}
template <bool TOPK>
static void onepass_launch_tail_dt(const OnepassPlan& p, hipStream_t s, int tgrid, int grid,
                                   const void* preds, const ll* target, ll B, int c_chunk,
                                   const uint4* records, const unsigned char* flags) {
    if (p.dtype == 0) onepass_launch_tail<float, TOPK>(p, s, tgrid, grid, preds, target, B, c_chunk, records, flags);
    else onepass_launch_tail<unsigned short, TOPK>(p, s, tgrid, grid, preds, target, B, c_chunk, records, flags);
}

// The whole fused-collection step on one stream in two launches: one-pass
// kernel, tail kernel (B == 0: the tail alone, which then is the epilogue).
static int onepass_step(const OnepassPlan& p, hipStream_t s, uintptr_t preds, uintptr_t target,
                        ll B) {
    if (preds & 15) return -103;
    if (B < 0 || B >= (1LL << 31)) return -101;  // u32 counts in the records
    const ll C = p.st.C;
    uint4* records = (uint4*)(p.cscratch + ONEPASS_REC_OFF(C));
    unsigned char* flags = (unsigned char*)(p.cscratch + ONEPASS_FLAG_OFF(C));
    const int grid = B > 0 ? onepass_grid(B, p.lpr, p.gcap) : 0;
    if (B > 0) {
        if (p.st.k > 0) onepass_launch_main_dt<true>(p, s, grid, (const void*)preds, (const ll*)target, B);
        else onepass_launch_main_dt<false>(p, s, grid, (const void*)preds, (const ll*)target, B);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    // Tail grid: a function of B and C alone (nothing only the device knows).
    // The first ceil(C/256) blocks carry the epilogue; the rest exist for the
    // deferred tiles and, with logit inputs, sum the records and leave. Class
    // chunks as in the two-kernel path: 4 classes, halved while the tile count
    // stays small. Sweep knob MA_ONEPASS_TAIL_GRID (profiles/README.md): 2048
    // blocks fill every CU, but the deferred tiles differ in cost (atomics),
    // and with a static walk the slowest block sets the time; twice as many
    // blocks as fit lets the dispatcher balance them (torch.rand inputs 361 us
    // at 2048, 347 at 4000, the three-launch step 347-348) for 2.5 us of the
    // logits loop.
    const int tcap = onepass_tail_cap();
    const ll row_chunks = (B + 255) / 256;
    int c_chunk = 4;
    while (c_chunk > 1 && ((C + c_chunk - 1) / c_chunk) * row_chunks < 4096) c_chunk /= 2;
    const ll ntiles = ((C + c_chunk - 1) / c_chunk) * row_chunks;
    ll tg = ntiles < tcap ? ntiles : tcap;
    const ll eblocks = (C + 255) / 256;
    if (tg < eblocks) tg = eblocks;
    const int tgrid = (int)((tg + 7) / 8 * 8);  // multiple of 8: block % 8 is the XCD
    if (p.st.k > 0) onepass_launch_tail_dt<true>(p, s, tgrid, grid, (const void*)preds, (const ll*)target, B, c_chunk, records, flags);
    else onepass_launch_tail_dt<false>(p, s, tgrid, grid, (const void*)preds, (const ll*)target, B, c_chunk, records, flags);
    return (int)hipGetLastError();
}

extern "C" {

// Step plan: create once per set of states, step every update (stream, preds,
// target and B are all that changes), destroy when the states are replaced.
// -103 for a shape the kernel does not cover or a missing / misaligned buffer;
// *handle is written only on success. Of the record the plan needs the count
// block (its valid slot is not used here), the stat states, the row statistics
// and the epoch buffer; confmat, correct/total and the top-k slot (k > 0: every
// step also counts and applies it) are optional. cscratch = curve scratch
// [P|R|records|flags] (ma_mc_onepass_scratch_words(C) u64). P and R are zero
// before the first step and grow until the flush zeroes them again
// (k_curve_resolve_pending); records and flags need no zeroing. While P or R
// is nonzero, hist is in pending format and must go through that flush before
// anything else reads or adds to it.
int ma_onepass_plan_create(const McStep* st, int dtype, uintptr_t thresholds, int T, int uniform,
                           float t0, float inv_step, uintptr_t hist, uintptr_t cscratch,
                           unsigned long long* handle) {
    const int nv = ma_mc_onepass_nv(dtype, st->C, T);
    if (nv == 0 || (cscratch & 15) || !cscratch || !hist || !thresholds || !st->counts ||
        !st->tp || !st->fp || !st->tn || !st->fn || !st->rowmax || !st->rowinv || !st->epoch_buf ||
        !st->correct != !st->total || st->k < 0)
        return -103;
    if (st->k > 0 && (!st->topk_counts || !st->tp_k || !st->fp_k || !st->tn_k || !st->fn_k))
        return -103;
    const int lpr = onepass_lpr(nv);
    // sweep knob MA_ONEPASS_PREFETCH, see PREFETCH in front of k_mc_onepass; the
    // variant exists where the second row buffer fits (onepass_launch_nv)
    const char* pf = getenv("MA_ONEPASS_PREFETCH");
    const int prefetch = (pf ? atoi(pf) != 0 : ONEPASS_PREFETCH_DEFAULT) &&
                         nv * (WAVE / lpr) <= (st->k > 0 ? ONEPASS_PF_MAX_NVL / 2 : ONEPASS_PF_MAX_NVL);
    *handle = (unsigned long long)(uintptr_t) new OnepassPlan{
        *st, dtype, nv, T, uniform, lpr, onepass_grid_cap(prefetch), prefetch,
        t0, inv_step, (ull*)hist,
        (ull*)cscratch, (const float*)thresholds};
    return 0;
}

int ma_onepass_plan_step(uintptr_t handle, uintptr_t stream, uintptr_t preds, uintptr_t target,
                         ll B) {
    if (!handle) return -103;
    return onepass_step(*(const OnepassPlan*)handle, (hipStream_t)stream, preds, target, B);
}

void ma_onepass_plan_destroy(uintptr_t handle) { delete (OnepassPlan*)handle; }

}  // extern "C"
