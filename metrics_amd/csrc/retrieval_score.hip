// Retrieval metrics (gfx950): every query of one compute() scored in ONE
// segmented pass, no per-query loop and no host sync. ma_retrieval_scores runs
// on the caller's stream:
//
//  1. k_retr_keys      composite keys (index << 32) | descending score bits (the
//                      key of k_retrieval_keys in clf_curve.hip), the target as
//                      fp32, and the header reset. One 64-bit rocPRIM radix
//                      pass sorts the keys with the TARGET as the value: the
//                      target rides the sort, so nothing is gathered through a
//                      permutation afterwards and preds is never read again
//                      (the score comes back out of the sorted key).
//  2. k_retr_flags + rocPRIM inclusive scan + k_retr_heads: the start offset of
//                      every query, and the query count G, on the device.
//  3. NDCG only: a second key-only sort of (index << 32) | descending TARGET
//                      bits; position i of it holds the i-th largest target of
//                      the same query (graded, float or integer).
//  4. k_retrieval_score  the per-query records (retrieval_score.h), below.
//  5. k_retrieval_tail   records -> fp32 score per query, empty_target_action,
//                      and mean / min / max in fp64 to one scalar.
//
// k_retrieval_score. Every query has ONE owner, so every floating sum has a
// fixed order and a call gives the same bits every time.
//  GROUP MAPPING (first launch). A power-of-two group of W lanes (8, 16, 32,
//   64) owns a query and walks it in chunks of W, one element per lane. W is
//   the smallest of these >= the mean query length n / G, read on the device.
//   Groups take queries grid-stride and skip those longer than RETR_BLOCK_MIN.
//   In a chunk the positives at or before a lane are a ballot of "target > 0",
//   shifted and masked to the group, and a popcount of the lanes up to it; the
//   carries between chunks (positives and negatives so far, first positive
//   rank, positives and negatives in front of the open tie group) are
//   group-uniform registers.
//  BLOCK MAPPING (second launch of the same template, same start list). A
//   block of RETR_BLOCK_WAVES waves owns a query longer than RETR_BLOCK_MIN;
//   wave w takes chunk w of every RETR_BLOCK_WAVES * 64 elements. The waves
//   put their chunk totals into LDS, every wave folds those of the waves in
//   front of it into its carry-in (the prefix fix-up), and all of them advance
//   the block carry by the same sums.
//  AUROC is the integer Mann-Whitney count over the first k_eff ranks,
//   U = 2 * #(positive above negative) + #(tied positive/negative pairs), so
//   AUROC = U / (2 P N). Each pair is counted at its LATER element, which only
//   looks backwards: a negative at rank r adds (positives in front of its tie
//   group) + (positives up to r), a positive adds (negatives of its tie group
//   up to r). A tie group starts where the float score differs from the one
//   before (a float compare of the scores recovered from the keys: -0.0 and
//   +0.0 tie although their keys differ); the heads of a chunk are a ballot
//   too, so a group that straddles chunks, waves or the k_eff cut needs only
//   the two carried counts.
//  fp64 sums (tsum, AP numerator, DCG, IDCG): per lane over the chunks in rank
//   order, lanes in an xor butterfly, waves of a block in index order.
//  PR-curve mode: the owner also writes row g of cum_rel[G, max_k], the
//   positives up to each rank, continued with the total past the query's end;
//   consecutive lanes write consecutive k.
//
// NaN scores sort wherever their bits fall and tie with nothing; what they
// yield is unspecified. Nothing here is captured into a graph in any test.

#include <cstring>  // memset, needed by rocprim's texture_cache_iterator header

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "retrieval_score.h"

typedef long long ll;
typedef unsigned long long ull;

#define OK(x)                                      \
    do {                                           \
        hipError_t err_ = (x);                     \
        if (err_ != hipSuccess) return (int)err_;  \
    } while (0)

#define RETR_BLOCK 256          // threads of a block of the group mapping
#define RETR_BLOCK_WAVES 16     // waves of a block of the block mapping
// A query longer than this goes to the block mapping. A wave walks 64 elements
// per step, so at 2048 it has spent 32 dependent steps on one query while the
// lanes of a whole block could have shared them; the block pays two barriers
// per 1024 elements for that, which a shorter query does not earn back. The
// value is reasoned, not swept (docs/ROADMAP.md).
#define RETR_BLOCK_MIN 2048
#define RETR_GRID_MAX 2048

#define RETR_WANT_AP 1
#define RETR_WANT_NDCG 2
#define RETR_WANT_AUROC 4
#define RETR_WANT_RPREC 8
#define RETR_WANT_CURVE 16

enum { M_MAP, M_MRR, M_PRECISION, M_RECALL, M_HIT_RATE, M_FALL_OUT, M_NDCG, M_RPREC, M_AUROC, M_CURVE, M_COUNT };
enum { HDR_G, HDR_MAX_COUNT, HDR_MIN_COUNT, HDR_EMPTY, HDR_KEPT, HDR_TICKET };

// descending-order-preserving bits of a float and back
__device__ __forceinline__ unsigned int retr_desc_bits(float x) {
    unsigned int b = __float_as_uint(x);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ~b;
}
__device__ __forceinline__ float retr_from_key(ull key) {
    unsigned int b = ~(unsigned int)key;
    b = (b & 0x80000000u) ? (b & 0x7fffffffu) : ~b;
    return __uint_as_float(b);
}
__device__ __forceinline__ ull retr_low_mask(int n) {  // the n lowest bits, 0 <= n <= 64
    return n >= 64 ? ~0ull : ((1ull << n) - 1ull);
}

template <typename TT>
__global__ void __launch_bounds__(256) k_retr_keys(
    const ll* __restrict__ idx, const float* __restrict__ preds, const TT* __restrict__ target, ll n,
    ull* __restrict__ keys, float* __restrict__ tv, ull* __restrict__ ideal_keys, int* __restrict__ hdr) {
    const ll i = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        hdr[HDR_G] = 0;
        hdr[HDR_MAX_COUNT] = 0;
        hdr[HDR_MIN_COUNT] = INT_MAX;
        hdr[HDR_EMPTY] = 0;
        hdr[HDR_KEPT] = 0;
        hdr[HDR_TICKET] = 0;
    }
    if (i >= n) return;
    const ull hi = (ull)(unsigned int)idx[i] << 32;
    const float t = (float)target[i];
    keys[i] = hi | (ull)retr_desc_bits(preds[i]);
    tv[i] = t;
    if (ideal_keys) ideal_keys[i] = hi | (ull)retr_desc_bits(t);
}

__global__ void __launch_bounds__(256) k_retr_flags(const ull* __restrict__ keys, ll n, int* __restrict__ flags) {
    const ll i = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flags[i] = (i == 0 || (keys[i] >> 32) != (keys[i - 1] >> 32)) ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_retr_heads(
    const int* __restrict__ flags, const int* __restrict__ scan, ll n, int* __restrict__ starts,
    int* __restrict__ hdr) {
    const ll i = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int g1 = scan[i];  // 1-based query of element i, <= i + 1
    if (flags[i]) starts[g1 - 1] = (int)i;
    if (i == n - 1) {
        hdr[HDR_G] = g1;
        starts[g1] = (int)n;
    }
}

// largest and smallest query (PR-curve mode asks for them before it sizes cum_rel)
__global__ void __launch_bounds__(256) k_retr_extent(const int* __restrict__ starts, int* __restrict__ hdr) {
    const int G = hdr[HDR_G];
    int mx = 0, mn = INT_MAX;
    for (ll g = (ll)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (ll)gridDim.x * blockDim.x) {
        const int c = starts[g + 1] - starts[g];
        mx = max(mx, c);
        mn = min(mn, c);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mx = max(mx, __shfl_xor(mx, off));
        mn = min(mn, __shfl_xor(mn, off));
    }
    if ((threadIdx.x & 63) == 0 && mx > 0) {
        atomicMax(&hdr[HDR_MAX_COUNT], mx);
        atomicMin(&hdr[HDR_MIN_COUNT], mn);
    }
}

struct RetrArgs {
    const ull* keys;    // sorted (index, score desc)
    const float* tv;    // targets in that order
    const ull* ideal;   // sorted (index, target desc), NDCG only
    const int* starts;  // G + 1 offsets
    const int* hdr;
    RetrRecord* rec;
    int* cum_rel;  // [G, max_k], curve mode only
    ll n;
    int top_k;  // 0: None
    int max_k;
    int want;
};

// what a wave of the block mapping tells the others about its chunk
struct RetrChunk {
    int cp, cn;    // positives, negatives
    int first;     // rank of its first positive, -1
    int has_head;  // a tie group starts in it
    int hp, hn;    // positives, negatives in front of its LAST head
};

struct RetrShared {
    RetrChunk chunk[RETR_BLOCK_WAVES];
    double dsum[RETR_BLOCK_WAVES][4];
    ll usum[RETR_BLOCK_WAVES];
    int isum[RETR_BLOCK_WAVES][4];
};

// One query [start, start + count) by its owner: WAVES == 1, a group of W lanes
// (lane l of it, at bit `shift` of the wave); WAVES > 1, a block of WAVES waves
// of W == 64 lanes. The control flow is uniform over the owner.
template <int W, int WAVES>
__device__ __forceinline__ void retr_query(const RetrArgs& a, ll g, int start, int count, int l, int shift,
                                           int wave, RetrShared* sh) {
    constexpr int STRIDE = W * WAVES;
    const ull gmask = retr_low_mask(W);
    const ull upto = retr_low_mask(l + 1);  // the lanes of the group up to and including this one
    const int want = a.want;
    const int k_eff = a.top_k > 0 ? min(a.top_k, count) : count;
    const int n_it = (count + STRIDE - 1) / STRIDE;
    const ll i0 = (ll)start;

    int npos_total = 0;
    if (want & RETR_WANT_RPREC) {  // the first npos ranks need npos first
        for (int it = 0; it < n_it; it++) {
            const int r = it * STRIDE + wave * W + l;
            const bool pos = r < count && a.tv[i0 + r] > 0.0f;
            npos_total += __popcll((__ballot(pos) >> shift) & gmask);
        }
        if constexpr (WAVES > 1) {
            if (l == 0) sh->isum[wave][0] = npos_total;
            __syncthreads();
            npos_total = 0;
            for (int w = 0; w < WAVES; w++) npos_total += sh->isum[w][0];
            __syncthreads();
        }
    }

    // carries, uniform over the owner
    int P = 0, Nn = 0, first = -1, gp = 0, gn = 0;
    // sums of this wave (integers) and of this lane (the rest)
    int hits_k = 0, neg_k = 0, hits_r = 0;
    ull u = 0;
    double tsum = 0.0, ap = 0.0, dcg = 0.0, idcg = 0.0;

    for (int it = 0; it < n_it; it++) {
        const int base = it * STRIDE + wave * W;
        const int r = base + l;
        const bool valid = r < count;
        const float t = valid ? a.tv[i0 + r] : 0.0f;
        const bool pos = valid && t > 0.0f;
        const bool neg = valid && t == 0.0f;
        const ull mpos = (__ballot(pos) >> shift) & gmask;
        const ull mneg = (__ballot(neg) >> shift) & gmask;
        ull mhead = 0;
        if (want & RETR_WANT_AUROC) {
            bool head = false;
            if (valid) head = r == 0 || retr_from_key(a.keys[i0 + r - 1]) != retr_from_key(a.keys[i0 + r]);
            mhead = (__ballot(head) >> shift) & gmask;
        }
        const int cp = __popcll(mpos), cn = __popcll(mneg);
        const int lf = mpos ? base + __builtin_ctzll(mpos) : -1;
        const int hl = mhead ? 63 - __builtin_clzll(mhead) : -1;
        const int hp = hl >= 0 ? __popcll(mpos & retr_low_mask(hl)) : 0;
        const int hn = hl >= 0 ? __popcll(mneg & retr_low_mask(hl)) : 0;

        // carry-in of this chunk, and the carry moved past the whole stride
        int Pin = P, Nin = Nn, gpin = gp, gnin = gn;
        if constexpr (WAVES > 1) {
            if (l == 0) sh->chunk[wave] = RetrChunk{cp, cn, lf, hl >= 0, hp, hn};
            __syncthreads();
            for (int w = 0; w < WAVES; w++) {
                const RetrChunk c = sh->chunk[w];
                if (w == wave) {
                    Pin = P;
                    Nin = Nn;
                    gpin = gp;
                    gnin = gn;
                }
                if (c.has_head) {
                    gp = P + c.hp;
                    gn = Nn + c.hn;
                }
                if (first < 0) first = c.first;
                P += c.cp;
                Nn += c.cn;
            }
            __syncthreads();
        } else {
            if (hl >= 0) {
                gp = P + hp;
                gn = Nn + hn;
            }
            if (first < 0) first = lf;
            P += cp;
            Nn += cn;
        }

        const ull ink = retr_low_mask(min(max(k_eff - base, 0), W));
        hits_k += __popcll(mpos & ink);
        neg_k += __popcll(mneg & ink);
        if (want & RETR_WANT_RPREC) hits_r += __popcll(mpos & retr_low_mask(min(max(npos_total - base, 0), W)));

        const bool in_k = r < k_eff;
        const int cum = Pin + __popcll(mpos & upto);  // positives at ranks <= r
        tsum += (double)t;
        if ((want & RETR_WANT_AP) && pos && in_k) ap += (double)cum / (double)(r + 1);
        if ((want & RETR_WANT_NDCG) && in_k) {
            const double disc = log2((double)(r + 2));
            dcg += (double)t / disc;
            idcg += (double)retr_from_key(a.ideal[i0 + r]) / disc;
        }
        if ((want & RETR_WANT_AUROC) && in_k) {
            const ull hb = mhead & upto;
            int cpb = gpin, cnb = gnin;  // positives, negatives in front of this lane's tie group
            if (hb) {
                const ull bm = retr_low_mask(63 - __builtin_clzll(hb));
                cpb = Pin + __popcll(mpos & bm);
                cnb = Nin + __popcll(mneg & bm);
            }
            if (neg) u += (ull)cpb + (ull)cum;
            else if (pos) u += (ull)(Nin + __popcll(mneg & upto) - cnb);
        }
        if ((want & RETR_WANT_CURVE) && valid && r < a.max_k) a.cum_rel[g * a.max_k + r] = cum;
    }
    if (want & RETR_WANT_CURVE) {
        for (int k = count + wave * W + l; k < a.max_k; k += STRIDE) a.cum_rel[g * a.max_k + k] = P;
    }

    // ---- fold: lanes in a butterfly, then the waves in index order ----
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) {
        tsum += __shfl_xor(tsum, off);
        ap += __shfl_xor(ap, off);
        dcg += __shfl_xor(dcg, off);
        idcg += __shfl_xor(idcg, off);
        u += (ull)__shfl_xor((ll)u, off);
    }
    if constexpr (WAVES > 1) {
        if (l == 0) {
            sh->dsum[wave][0] = tsum;
            sh->dsum[wave][1] = ap;
            sh->dsum[wave][2] = dcg;
            sh->dsum[wave][3] = idcg;
            sh->usum[wave] = (ll)u;
            sh->isum[wave][0] = hits_k;
            sh->isum[wave][1] = neg_k;
            sh->isum[wave][2] = hits_r;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            tsum = ap = dcg = idcg = 0.0;
            u = 0;
            hits_k = neg_k = hits_r = 0;
            for (int w = 0; w < WAVES; w++) {
                tsum += sh->dsum[w][0];
                ap += sh->dsum[w][1];
                dcg += sh->dsum[w][2];
                idcg += sh->dsum[w][3];
                u += (ull)sh->usum[w];
                hits_k += sh->isum[w][0];
                neg_k += sh->isum[w][1];
                hits_r += sh->isum[w][2];
            }
        }
    }
    if (wave == 0 && l == 0) {
        RetrRecord rec;
        rec.count = count;
        rec.npos = P;
        rec.nneg = Nn;
        rec.hits_k = hits_k;
        rec.neg_hits_k = neg_k;
        rec.first_pos = first;
        rec.hits_r = hits_r;
        rec.pad = 0;
        rec.u = (ll)u;
        rec.tsum = tsum;
        rec.ap = ap;
        rec.dcg = dcg;
        rec.idcg = idcg;
        a.rec[g] = rec;
    }
    if constexpr (WAVES > 1) __syncthreads();  // the LDS is written again by the next query
}

template <int W>
__device__ __forceinline__ void retr_groups(const RetrArgs& a, int G) {
    const int lane = threadIdx.x & 63;
    const int l = lane & (W - 1);
    const int shift = lane & ~(W - 1);
    const ll n_groups = (ll)gridDim.x * blockDim.x / W;
    for (ll g = ((ll)blockIdx.x * blockDim.x + threadIdx.x) / W; g < G; g += n_groups) {
        const int start = a.starts[g];
        const int count = a.starts[g + 1] - start;
        if (count > RETR_BLOCK_MIN) continue;  // the block launch owns it
        retr_query<W, 1>(a, g, start, count, l, shift, 0, nullptr);
    }
}

// WAVES == 1: the group mapping; WAVES == RETR_BLOCK_WAVES: the block mapping
template <int WAVES>
__global__ void __launch_bounds__(WAVES == 1 ? RETR_BLOCK : WAVES * 64) k_retrieval_score(RetrArgs a) {
    const int G = a.hdr[HDR_G];
    if (G < 1) return;
    if constexpr (WAVES == 1) {
        const ll mean = a.n / G;  // G >= 1: n >= 1
        if (mean <= 8) retr_groups<8>(a, G);
        else if (mean <= 16) retr_groups<16>(a, G);
        else if (mean <= 32) retr_groups<32>(a, G);
        else retr_groups<64>(a, G);
    } else {
        __shared__ RetrShared sh;
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int lane = threadIdx.x & 63;
        for (ll g = blockIdx.x; g < G; g += gridDim.x) {
            const int start = a.starts[g];
            const int count = a.starts[g + 1] - start;
            if (count <= RETR_BLOCK_MIN) continue;
            retr_query<64, WAVES>(a, g, start, count, lane, 0, wave, &sh);
        }
    }
}

// Records -> scores. The formulas are those of the torch path's
// _batched_scores, formed in fp64 and rounded once. A thread takes queries
// gtid, gtid + threads, ... in order; lanes meet in a butterfly, the waves of a
// block and then the blocks are added in index order by the last block to
// finish (an integer ticket), so the scalar has a fixed order too.
__global__ void __launch_bounds__(256) k_retrieval_tail(
    const RetrRecord* __restrict__ rec, int* __restrict__ hdr, int metric, int top_k, int adaptive_k,
    int action /*0 neg 1 pos 2 skip 3 leave*/, int agg /*0 mean 1 min 2 max 3 none*/,
    float* __restrict__ scores, unsigned char* __restrict__ empty, double* __restrict__ slab,
    float* __restrict__ out) {
    __shared__ double red[4][RETR_SLAB_DOUBLES];
    __shared__ int last;
    const int G = hdr[HDR_G];
    double sum = 0.0, mn = INFINITY, mx = -INFINITY, kept = 0.0, n_empty = 0.0;
    for (ll g = (ll)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (ll)gridDim.x * blockDim.x) {
        const RetrRecord r = rec[g];
        const int k_eff = top_k > 0 ? min(top_k, r.count) : r.count;
        double s = 0.0;
        bool is_empty = r.tsum == 0.0;
        switch (metric) {
            case M_MAP: s = r.hits_k > 0 ? r.ap / (double)r.hits_k : 0.0; break;
            case M_MRR: s = (r.first_pos >= 0 && r.first_pos < k_eff) ? 1.0 / (double)(r.first_pos + 1) : 0.0; break;
            case M_PRECISION:
                s = (double)r.hits_k / (double)(top_k <= 0 ? r.count : (adaptive_k ? k_eff : top_k));
                break;
            case M_RECALL: s = (double)r.hits_k / (double)max(r.npos, 1); break;
            case M_HIT_RATE: s = r.hits_k > 0 ? 1.0 : 0.0; break;
            case M_FALL_OUT:
                s = (double)r.neg_hits_k / (double)max(r.nneg, 1);
                is_empty = r.nneg == 0;
                break;
            case M_NDCG: s = r.idcg > 0.0 ? r.dcg / r.idcg : 0.0; break;
            case M_RPREC: s = (double)r.hits_r / (double)max(r.npos, 1); break;
            case M_AUROC:
                s = (r.hits_k > 0 && r.neg_hits_k > 0)
                        ? (double)r.u / (2.0 * (double)r.hits_k * (double)r.neg_hits_k) : 0.0;
                break;
            default: s = (double)r.npos; break;  // M_CURVE: what recall divides by
        }
        bool keep = true;
        if (is_empty) {
            n_empty += 1.0;
            if (action == 0) s = 0.0;
            else if (action == 1) s = 1.0;
            else if (action == 2) keep = false;
        }
        scores[g] = (float)s;
        empty[g] = is_empty ? 1 : 0;
        if (keep) {
            sum += s;
            mn = fmin(mn, s);
            mx = fmax(mx, s);
            kept += 1.0;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off);
        mn = fmin(mn, __shfl_xor(mn, off));
        mx = fmax(mx, __shfl_xor(mx, off));
        kept += __shfl_xor(kept, off);
        n_empty += __shfl_xor(n_empty, off);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        red[wave][0] = sum;
        red[wave][1] = mn;
        red[wave][2] = mx;
        red[wave][3] = kept;
        red[wave][4] = n_empty;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) {
            sum += red[w][0];
            mn = fmin(mn, red[w][1]);
            mx = fmax(mx, red[w][2]);
            kept += red[w][3];
            n_empty += red[w][4];
        }
        double* e = slab + (ll)blockIdx.x * RETR_SLAB_DOUBLES;
        e[0] = sum;
        e[1] = mn;
        e[2] = mx;
        e[3] = kept;
        e[4] = n_empty;
        __threadfence();
        last = atomicAdd(&hdr[HDR_TICKET], 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!last || wave != 0) return;
    __threadfence();
    sum = 0.0, mn = INFINITY, mx = -INFINITY, kept = 0.0, n_empty = 0.0;
    for (int b = lane; b < (int)gridDim.x; b += 64) {
        const volatile double* e = slab + (ll)b * RETR_SLAB_DOUBLES;
        sum += e[0];
        mn = fmin(mn, e[1]);
        mx = fmax(mx, e[2]);
        kept += e[3];
        n_empty += e[4];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off);
        mn = fmin(mn, __shfl_xor(mn, off));
        mx = fmax(mx, __shfl_xor(mx, off));
        kept += __shfl_xor(kept, off);
        n_empty += __shfl_xor(n_empty, off);
    }
    if (lane != 0) return;
    double v = 0.0;  // no query left
    if (kept > 0.0) v = agg == 0 ? sum / kept : (agg == 1 ? mn : mx);
    if (agg != 3) out[0] = (float)v;
    hdr[HDR_EMPTY] = (int)n_empty;
    hdr[HDR_KEPT] = (int)kept;
    hdr[HDR_TICKET] = 0;
}

// ---- host ----
static int retr_rocprim_tmp(ll n, size_t* out) {
    size_t s_pairs = 0, s_keys = 0, s_scan = 0;
    OK(rocprim::radix_sort_pairs((void*)nullptr, s_pairs, (const ull*)nullptr, (ull*)nullptr,
                                 (const float*)nullptr, (float*)nullptr, (size_t)n));
    OK(rocprim::radix_sort_keys((void*)nullptr, s_keys, (const ull*)nullptr, (ull*)nullptr, (size_t)n));
    OK(rocprim::inclusive_scan((void*)nullptr, s_scan, (const int*)nullptr, (int*)nullptr, (size_t)n,
                               rocprim::plus<int>()));
    size_t m = s_pairs > s_keys ? s_pairs : s_keys;
    *out = m > s_scan ? m : s_scan;
    return 0;
}

static inline int retr_grid(ll n, ll per_block, int cap) {
    const ll g = (n + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

extern "C" {

// Host only: what a call over n elements needs. out = {scratch bytes, offset of
// the records, bytes of a record, the longest query of the group mapping
// (RETR_BLOCK_MIN), blocks of the group launch, blocks of the block launch (0:
// not launched), blocks of the tail}. -103: n not covered.
int ma_retrieval_scores_layout(ll n, int ndcg, ll* out) {
    out[2] = (ll)sizeof(RetrRecord);
    out[3] = RETR_BLOCK_MIN;
    if (n < 1 || n > 0x7ffffffeLL) return -103;
    size_t tmp = 0;
    int rc = retr_rocprim_tmp(n, &tmp);
    if (rc) return rc;
    RetrScratch sc;
    if (!retr_carve(n, ndcg, tmp, &sc)) return -103;
    out[0] = (ll)sc.total;
    out[1] = (ll)sc.records;
    out[4] = retr_grid(n, RETR_BLOCK, RETR_GRID_MAX);
    out[5] = n > RETR_BLOCK_MIN ? retr_grid(n, RETR_BLOCK_MIN + 1, 1024) : 0;
    out[6] = retr_grid(n, RETR_BLOCK, RETR_TAIL_GRID_MAX);
    return 0;
}

// One scoring call. phases: 1 = keys, sort, query heads (and the extent of the
// queries when `want` has the curve bit); 2 = records and tail; 3 = both. A
// call with phase 2 alone continues the phase-1 call before it on the same
// scratch (the PR curve reads G and the largest query in between).
// target_dtype 0 fp32, 1 int64. top_k 0 = None. `scores` and `empty` hold n
// entries, `out` one float, cum_rel G * max_k ints in curve mode.
// -103: arguments the kernels do not cover; nothing is launched then.
int ma_retrieval_scores(uintptr_t stream, uintptr_t idx, uintptr_t preds, uintptr_t target, int target_dtype,
                        ll n, int top_k, int max_k, int want, int metric, int adaptive_k, int action, int agg,
                        int phases, uintptr_t scratch, ull scratch_bytes, uintptr_t cum_rel, uintptr_t scores,
                        uintptr_t empty, uintptr_t out) {
    if (n < 1 || n > 0x7ffffffeLL || !scratch || scratch % 256) return -103;
    if (phases < 1 || phases > 3 || want < 0 || want > 31 || metric < 0 || metric >= M_COUNT) return -103;
    if (top_k < 0 || action < 0 || action > 3 || agg < 0 || agg > 3) return -103;
    if ((phases & 1) && (!idx || !preds || !target || idx % 8 || preds % 4 || (target_dtype != 0 && target_dtype != 1) ||
                         target % (target_dtype ? 8 : 4)))
        return -103;
    if ((phases & 2) && (!scores || !empty || !out || scores % 4 || out % 4)) return -103;
    if ((phases & 2) && (want & RETR_WANT_CURVE) && (!cum_rel || cum_rel % 4 || max_k < 1)) return -103;
    const int ndcg = (want & RETR_WANT_NDCG) ? 1 : 0;
    size_t tmp_bytes = 0;
    int rc = retr_rocprim_tmp(n, &tmp_bytes);
    if (rc) return rc;
    RetrScratch sc;
    if (!retr_carve(n, ndcg, tmp_bytes, &sc) || sc.total > scratch_bytes) return -103;

    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)scratch;
    int* hdr = (int*)(base + sc.hdr);
    ull* keys_a = (ull*)(base + sc.keys_a);
    ull* keys_b = (ull*)(base + sc.keys_b);
    ull* keys_c = ndcg ? (ull*)(base + sc.keys_c) : nullptr;
    float* tv_a = (float*)(base + sc.tv_a);
    float* tv_b = (float*)(base + sc.tv_b);
    int* starts = (int*)(base + sc.starts);
    int* flags = (int*)(base + sc.flags);
    int* scan = (int*)(base + sc.scan);
    void* tmp = (void*)(base + sc.tmp);
    const int egrid = (int)((n + 255) / 256);  // one thread per element: n < 2^31

    if (phases & 1) {
        if (target_dtype == 0)
            k_retr_keys<float><<<egrid, 256, 0, s>>>((const ll*)idx, (const float*)preds, (const float*)target, n,
                                                     keys_a, tv_a, keys_c, hdr);
        else
            k_retr_keys<ll><<<egrid, 256, 0, s>>>((const ll*)idx, (const float*)preds, (const ll*)target, n,
                                                  keys_a, tv_a, keys_c, hdr);
        OK(hipGetLastError());
        size_t b = tmp_bytes;
        OK(rocprim::radix_sort_pairs(tmp, b, keys_a, keys_b, tv_a, tv_b, (size_t)n, 0, 64, s));
        if (ndcg) {
            b = tmp_bytes;
            OK(rocprim::radix_sort_keys(tmp, b, keys_c, keys_a, (size_t)n, 0, 64, s));  // keys_a: ideal order
        }
        k_retr_flags<<<egrid, 256, 0, s>>>(keys_b, n, flags);
        OK(hipGetLastError());
        b = tmp_bytes;
        OK(rocprim::inclusive_scan(tmp, b, flags, scan, (size_t)n, rocprim::plus<int>(), s));
        k_retr_heads<<<egrid, 256, 0, s>>>(flags, scan, n, starts, hdr);
        OK(hipGetLastError());
        if (want & RETR_WANT_CURVE) {
            k_retr_extent<<<retr_grid(n, RETR_BLOCK, RETR_TAIL_GRID_MAX), 256, 0, s>>>(starts, hdr);
            OK(hipGetLastError());
        }
    }
    if (phases & 2) {
        RetrArgs a;
        a.keys = keys_b;
        a.tv = tv_b;
        a.ideal = ndcg ? (const ull*)(base + sc.ideal) : nullptr;
        a.starts = starts;
        a.hdr = hdr;
        a.rec = (RetrRecord*)(base + sc.records);
        a.cum_rel = (int*)cum_rel;
        a.n = n;
        a.top_k = top_k;
        a.max_k = max_k;
        a.want = want;
        k_retrieval_score<1><<<retr_grid(n, RETR_BLOCK, RETR_GRID_MAX), RETR_BLOCK, 0, s>>>(a);
        OK(hipGetLastError());
        if (n > RETR_BLOCK_MIN) {
            k_retrieval_score<RETR_BLOCK_WAVES>
                <<<retr_grid(n, RETR_BLOCK_MIN + 1, 1024), RETR_BLOCK_WAVES * 64, 0, s>>>(a);
            OK(hipGetLastError());
        }
        k_retrieval_tail<<<retr_grid(n, RETR_BLOCK, RETR_TAIL_GRID_MAX), 256, 0, s>>>(
            a.rec, hdr, metric, top_k, adaptive_k, action, agg, (float*)scores, (unsigned char*)empty,
            (double*)(base + sc.slab), (float*)out);
        OK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
