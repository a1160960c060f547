// Kendall rank correlation (gfx950): the pair counts of every column of one
// call by Knight's algorithm as a counting merge sort, on the caller's stream
// with no host sync. ma_kendall runs, column after column on the same scratch:
//
//  1. k_kd_keys   column d of preds (x) and target (y), fp32 / bf16 / fp16 read
//     with row stride D, each mapped to an order-preserving uint32 (the sign
//     flip; -0.0 becomes +0.0 first, so the two tie as they do in a float
//     compare; denormals stay distinct, +-inf are ordinary values) and packed
//     as (ux << 32) | uy. A NaN in either sets the column's flag word.
//  2. one rocPRIM radix sort of the 64-bit keys: the low words are then y in
//     (x, then y) ascending order, the order Knight's algorithm counts in.
//  3. k_kd_runs   tie statistics of a sorted array, templated on the key view:
//     the x runs (high word), the (x, y) runs (whole key) and, after the merge
//     sort, the y runs. A block owns the runs whose head lies in its tile of
//     KD_RUN_TILE keys in LDS; the end of a run is an upper-bound search in the
//     tile, continued in the global array for the one run that leaves the tile.
//     Per run of length t: t(t-1)/2 and the run count as exact integers (one
//     atomic per block each), t(t-1)(t-2) and t(t-1)(2t+5) in fp64 as per-block
//     partials that the tail sums in a fixed order.
//  4. k_kd_tile   a block of KD_TILE_BLOCK threads stages KD_TILE y-keys in LDS.
//     Each wave first ranks its chunks of 64 keys by brute force in registers:
//     lane l holds key l, a loop broadcasts lane j to all, and a lane counts the
//     keys that sort before its own (its position) and the earlier keys that are
//     strictly greater (its inversions). Then rank-merge levels of width 64,
//     128, ... KD_TILE / 2 ping-pong between two LDS buffers: every key
//     binary-searches its sibling run, left keys for "strictly less", right keys
//     for "less or equal" (a stable merge position), and each right key adds
//     |left| - upper_bound to the inversions. A short last tile is padded with
//     the largest word, which stays behind every key and inverts with nothing.
//     The block writes its sorted tile and adds its count to the column's 64-bit
//     counter with one atomic (an integer: the order does not matter).
//  5. k_kd_merge  one launch per width KD_TILE, 2 KD_TILE, ... < n, ping-ponging
//     two global buffers (both halves of the spent sort input). A block takes a
//     chunk of KD_CHUNK consecutive keys of one run; two binary searches with
//     the chunk's first and last key bound the part of the sibling run the chunk
//     interleaves with. Up to KD_STAGE words of it are staged in LDS and
//     searched there, a longer part is searched in global memory. Keys scatter
//     to their merged position; right keys count as in the tile phase, in 64
//     bits. A run without a sibling (odd run count, short last run) has an empty
//     sibling and lands where it was.
//  6. k_kd_tail   one block per column: the fp64 partials in a fixed order, then
//     the record: con = n(n-1)/2 - xtie - ytie + xytie - dis, tau by variant
//     a / b / c and the tie-corrected t-value, in fp64 and in the order of
//     operations of functional/regression/kendall.py; tau also as fp32 into the
//     output. A set NaN flag makes tau and the t-value NaN.
//
// No matrix instructions: the work is compares and integer adds. Launches per
// column: 6 + those of the radix sort + ceil(log2(n / KD_TILE)).

#include <cstring>  // memset, needed by rocprim's texture_cache_iterator header

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <math.h>
#include <stdint.h>

typedef long long ll;
typedef unsigned long long ull;

#define OK(x)                                      \
    do {                                           \
        hipError_t err_ = (x);                     \
        if (err_ != hipSuccess) return (int)err_;  \
    } while (0)

#define KD_TILE 4096         // y-keys a tile block sorts in LDS (two 16 KiB buffers)
#define KD_TILE_BLOCK 1024   // its threads: four keys each
#define KD_CHUNK 1024        // keys of one run a merge block takes (divides KD_TILE)
#define KD_MERGE_BLOCK 256
#define KD_STAGE 4096        // words of the sibling run a merge block stages in LDS
#define KD_RUN_TILE 2048     // keys per block of the run statistics
#define KD_RUN_BLOCK 256
// 32-bit positions would allow 2^31 - 1; the scratch (two 8-byte key buffers
// and the sort's own, about 24 bytes per element) is 6 GiB at this n.
#define KD_MAX_N (1LL << 28)
#define KD_MAX_D 65536

// the record of a column, 8-byte words
enum {
    KD_CON, KD_DIS, KD_XTIE, KD_YTIE, KD_XYTIE, KD_UX, KD_UY,  // int64
    KD_P1X, KD_P2X, KD_P1Y, KD_P2Y, KD_TAU, KD_TVAL,            // fp64
    KD_LDS_CHUNKS, KD_GLOBAL_CHUNKS, KD_NAN,                    // int64: merge chunks by route, the NaN flag
    KD_REC_WORDS
};

enum { KD_VIEW_X, KD_VIEW_XY, KD_VIEW_Y };

// ------------------------------------------------------------------ key build
__device__ __forceinline__ float kd_f32(float v) { return v; }
__device__ __forceinline__ float kd_f32(_Float16 v) { return (float)v; }
__device__ __forceinline__ float kd_f32(uint16_t v) { return __uint_as_float((unsigned int)v << 16); }  // bf16

__device__ __forceinline__ unsigned int kd_order(float v, bool& nan) {
    unsigned int b = __float_as_uint(v);
    if ((b & 0x7fffffffu) > 0x7f800000u) nan = true;
    if ((b << 1) == 0u) b = 0u;  // -0.0 == +0.0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ void __launch_bounds__(256) k_kd_init(ull* __restrict__ rec, ll words) {
    const ll i = (ll)blockIdx.x * 256 + threadIdx.x;
    if (i < words) rec[i] = 0ull;
}

template <typename T>
__global__ void __launch_bounds__(256) k_kd_keys(
    const T* __restrict__ x, const T* __restrict__ y, ll n, ll D, ll d, ull* __restrict__ keys,
    ull* __restrict__ rec) {
    const ll i = (ll)blockIdx.x * 256 + threadIdx.x;
    bool nan = false;
    if (i < n) {
        const unsigned int ux = kd_order(kd_f32(x[i * D + d]), nan);
        const unsigned int uy = kd_order(kd_f32(y[i * D + d]), nan);
        keys[i] = ((ull)ux << 32) | uy;
    }
    if (__any(nan) && (threadIdx.x & 63) == 0) atomicOr(&rec[KD_NAN], 1ull);
}

// ------------------------------------------------------------- block reductions
// Sums over a block in a fixed order: xor butterfly in a wave, waves in index
// order. Valid in thread 0. `red` holds one word per wave.
template <typename V, int WAVES>
__device__ __forceinline__ V kd_block_sum(V v, V* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();  // red may still be read from the sum before
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        v = red[0];
#pragma unroll
        for (int w = 1; w < WAVES; w++) v += red[w];
    }
    return v;
}

// ------------------------------------------------------------- run statistics
template <int VIEW>
__device__ __forceinline__ ull kd_view(const void* a, ll i) {
    if (VIEW == KD_VIEW_X) return ((const ull*)a)[i] >> 32;
    if (VIEW == KD_VIEW_XY) return ((const ull*)a)[i];
    return ((const unsigned int*)a)[i];
}

// pairs: the column's sum of t(t-1)/2; runs (may be null): its run count;
// p1 / p2 (may be null): one fp64 partial per block.
template <int VIEW>
__global__ void __launch_bounds__(KD_RUN_BLOCK) k_kd_runs(
    const void* __restrict__ a, ll n, ull* __restrict__ pairs, ull* __restrict__ runs, double* __restrict__ p1,
    double* __restrict__ p2) {
    __shared__ ull tile[KD_RUN_TILE];
    __shared__ ll red_i[KD_RUN_BLOCK / 64];
    __shared__ double red_d[KD_RUN_BLOCK / 64];
    const int tid = threadIdx.x;
    const ll t0 = (ll)blockIdx.x * KD_RUN_TILE;
    const int len = (int)min((ll)KD_RUN_TILE, n - t0);  // >= 1: the grid covers n exactly
    for (int j = tid; j < len; j += KD_RUN_BLOCK) tile[j] = kd_view<VIEW>(a, t0 + j);
    __syncthreads();

    ll s_pairs = 0, s_runs = 0;
    double s_p1 = 0.0, s_p2 = 0.0;
    for (int j = tid; j < len; j += KD_RUN_BLOCK) {
        const ull key = tile[j];
        const bool head = j ? tile[j - 1] != key : (t0 == 0 || kd_view<VIEW>(a, t0 - 1) != key);
        if (!head) continue;
        s_runs++;
        if (j + 1 < len && tile[j + 1] != key) continue;  // a run of one: all four terms are zero
        int lo = j + 1, hi = len;  // the first index of the tile past the run
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (tile[mid] == key) lo = mid + 1;
            else hi = mid;
        }
        ll end = t0 + lo;
        if (lo == len && t0 + len < n) {  // the run leaves the tile: at most one per block
            ll glo = t0 + len, ghi = n;
            while (glo < ghi) {
                const ll mid = glo + ((ghi - glo) >> 1);
                if (kd_view<VIEW>(a, mid) == key) glo = mid + 1;
                else ghi = mid;
            }
            end = glo;
        }
        const ll t = end - (t0 + j);
        s_pairs += t * (t - 1) / 2;
        const double td = (double)t, tt = td * (td - 1.0);
        s_p1 += tt * (td - 2.0);
        s_p2 += tt * (2.0 * td + 5.0);
    }
    s_pairs = kd_block_sum<ll, KD_RUN_BLOCK / 64>(s_pairs, red_i);
    s_runs = kd_block_sum<ll, KD_RUN_BLOCK / 64>(s_runs, red_i);
    if (tid == 0) {
        if (s_pairs) atomicAdd(pairs, (ull)s_pairs);
        if (runs && s_runs) atomicAdd(runs, (ull)s_runs);
    }
    if (p1) {
        s_p1 = kd_block_sum<double, KD_RUN_BLOCK / 64>(s_p1, red_d);
        s_p2 = kd_block_sum<double, KD_RUN_BLOCK / 64>(s_p2, red_d);
        if (tid == 0) {
            p1[blockIdx.x] = s_p1;
            p2[blockIdx.x] = s_p2;
        }
    }
}

// ----------------------------------------------------------------- tile phase
// How many of the `len` sorted words of `a` are below `key` (le: or equal to it).
template <typename P>
__device__ __forceinline__ int kd_below(P a, int len, unsigned int key, bool le) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const unsigned int v = a[mid];
        if (v < key || (le && v == key)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(KD_TILE_BLOCK) k_kd_tile(
    const ull* __restrict__ keys, ll n, unsigned int* __restrict__ out, ull* __restrict__ dis) {
    __shared__ unsigned int buf[2][KD_TILE];
    __shared__ ll red[KD_TILE_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ll t0 = (ll)blockIdx.x * KD_TILE;
    const int len = (int)min((ll)KD_TILE, n - t0);
    constexpr int PER = KD_TILE / KD_TILE_BLOCK;  // keys per thread, chunks of 64 per wave
    unsigned int inv = 0;  // at most PER * (63 + KD_TILE / 2 * levels): far below 2^32

#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int c0 = (wave * PER + q) * 64;
        const unsigned int key = c0 + lane < len ? (unsigned int)keys[t0 + c0 + lane] : 0xffffffffu;
        int rank = 0;
        for (int j = 0; j < 64; j++) {
            const unsigned int o = (unsigned int)__shfl((int)key, j);
            rank += (o < key) || (o == key && j < lane);
            inv += (j < lane) && (o > key);
        }
        buf[0][c0 + rank] = key;
    }
    __syncthreads();

    int cur = 0;
    for (int w = 64; w < KD_TILE; w <<= 1) {
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const int p = q * KD_TILE_BLOCK + tid;
            const unsigned int key = buf[cur][p];
            const int base = p & ~(2 * w - 1), idx = p & (w - 1);
            const bool right = (p & w) != 0;
            const int cnt = kd_below(&buf[cur][base + (right ? 0 : w)], w, key, right);
            if (right) inv += (unsigned int)(w - cnt);
            buf[cur ^ 1][base + idx + cnt] = key;
        }
        __syncthreads();
        cur ^= 1;
    }
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int p = q * KD_TILE_BLOCK + tid;
        if (p < len) out[t0 + p] = buf[cur][p];
    }
    const ll total = kd_block_sum<ll, KD_TILE_BLOCK / 64>((ll)inv, red);
    if (tid == 0 && total) atomicAdd(dis, (ull)total);
}

// ---------------------------------------------------------- global merge levels
// src: sorted runs of width w (the last may be short); dst: runs of width 2w.
__global__ void __launch_bounds__(KD_MERGE_BLOCK) k_kd_merge(
    const unsigned int* __restrict__ src, unsigned int* __restrict__ dst, ll n, ll w, ull* __restrict__ rec) {
    __shared__ unsigned int stage[KD_STAGE];
    __shared__ ll red[KD_MERGE_BLOCK / 64];
    const int tid = threadIdx.x;
    const ll c0 = (ll)blockIdx.x * KD_CHUNK;
    const int clen = (int)min((ll)KD_CHUNK, n - c0);  // >= 1; w is a multiple of KD_CHUNK: one run
    const ll r = c0 / w, run0 = r * w, base = (r & ~1LL) * w;
    const bool right = (r & 1) != 0;
    const ll sib0 = (r ^ 1) * w;
    const int slen = sib0 < n ? (int)min(w, n - sib0) : 0;  // 0: a left run without a sibling
    const unsigned int* __restrict__ sib = src + (sib0 < n ? sib0 : 0);

    int lo = 0, hi = 0;  // the sibling keys outside [lo, hi) sort before / after the whole chunk
    if (slen) {
        lo = kd_below(sib, slen, src[c0], right);
        hi = kd_below(sib, slen, src[c0 + clen - 1], right);
    }
    const int m = hi - lo;
    const bool in_lds = m <= KD_STAGE;  // block-uniform
    if (in_lds) {
        for (int j = tid; j < m; j += KD_MERGE_BLOCK) stage[j] = sib[lo + j];
        __syncthreads();
    }
    ll inv = 0;  // a right key adds up to w: 64 bits from here on
    for (int j = tid; j < clen; j += KD_MERGE_BLOCK) {
        const unsigned int key = src[c0 + j];
        const int cnt = lo + (in_lds ? kd_below(stage, m, key, right) : kd_below(sib + lo, m, key, right));
        if (right) inv += slen - cnt;
        dst[base + (c0 + j - run0) + cnt] = key;
    }
    inv = kd_block_sum<ll, KD_MERGE_BLOCK / 64>(inv, red);
    if (tid == 0) {
        if (inv) atomicAdd(&rec[KD_DIS], (ull)inv);
        if (slen) atomicAdd(&rec[in_lds ? KD_LDS_CHUNKS : KD_GLOBAL_CHUNKS], 1ull);
    }
}

// ------------------------------------------------------------------------ tail
// One block per launch (one column). part: p1x | p2x | p1y | p2y, nb each.
__global__ void __launch_bounds__(256) k_kd_tail(
    ull* __restrict__ rec, const double* __restrict__ part, ll nb, ll n, int variant, float* __restrict__ tau_out) {
    __shared__ double red[4];
    double p[4];
    for (int k = 0; k < 4; k++) {
        double s = 0.0;
        for (ll i = threadIdx.x; i < nb; i += 256) s += part[k * nb + i];
        p[k] = kd_block_sum<double, 4>(s, red);
    }
    if (threadIdx.x != 0) return;
    const double nd = (double)n;
    const double n0 = (double)(n * (n - 1)) / 2.0;  // n <= 2^28: the product is exact
    const ll dis_i = (ll)rec[KD_DIS], xt_i = (ll)rec[KD_XTIE], yt_i = (ll)rec[KD_YTIE], xyt_i = (ll)rec[KD_XYTIE];
    const ll con_i = n * (n - 1) / 2 - xt_i - yt_i + xyt_i - dis_i;
    const double con = (double)con_i, dis = (double)dis_i, xtie = (double)xt_i, ytie = (double)yt_i;
    const double cmd = con - dis;
    double tau;
    if (variant == 0) tau = cmd / (con + dis);
    else if (variant == 1) tau = cmd / sqrt((n0 - xtie) * (n0 - ytie));
    else {
        const double m = (double)min((ll)rec[KD_UX], (ll)rec[KD_UY]);
        tau = 2.0 * cmd / (nd * nd * (m - 1.0) / m);
    }
    const double base = nd * (nd - 1.0) * (2.0 * nd + 5.0);
    double tval;
    if (variant == 0) tval = 3.0 * cmd / sqrt(base / 2.0);
    else {
        const double mm = nd * (nd - 1.0);
        double denom = (base - p[1] - p[3]) / 18.0;
        denom += (2.0 * xtie * ytie) / mm;
        denom += n != 2 ? p[0] * p[2] / (9.0 * mm * (nd - 2.0)) : (double)NAN;  // n == 2: 0 / 0 in the reference
        tval = (denom == denom && denom > 0.0) ? cmd / sqrt(denom) : (double)NAN;
    }
    if (rec[KD_NAN]) tau = tval = (double)NAN;
    double* recd = (double*)rec;
    rec[KD_CON] = (ull)con_i;
    recd[KD_P1X] = p[0];
    recd[KD_P2X] = p[1];
    recd[KD_P1Y] = p[2];
    recd[KD_P2Y] = p[3];
    recd[KD_TAU] = tau;
    recd[KD_TVAL] = tval;
    tau_out[0] = (float)tau;
}

// ------------------------------------------------------------------------ host
struct KdScratch {
    size_t keys_a, keys_b, part, tmp, total;
    ll run_blocks;
};

static inline size_t kd_up(size_t v) { return (v + 255) & ~(size_t)255; }

static int kd_carve(ll n, KdScratch* sc, size_t* tmp_bytes) {
    *tmp_bytes = 0;
    OK(rocprim::radix_sort_keys((void*)nullptr, *tmp_bytes, (const ull*)nullptr, (ull*)nullptr, (size_t)n));
    sc->run_blocks = (n + KD_RUN_TILE - 1) / KD_RUN_TILE;
    sc->keys_a = 0;  // the sort input; afterwards the two y buffers of n words each
    sc->keys_b = kd_up(sc->keys_a + (size_t)n * 8);
    sc->part = kd_up(sc->keys_b + (size_t)n * 8);
    sc->tmp = kd_up(sc->part + (size_t)sc->run_blocks * 4 * 8);
    sc->total = kd_up(sc->tmp + *tmp_bytes);
    return 0;
}

static inline bool kd_covers(ll n, ll D) { return n >= 2 && n <= KD_MAX_N && D >= 1 && D <= KD_MAX_D; }

template <typename T>
static void kd_keys_launch(hipStream_t s, uintptr_t x, uintptr_t y, ll n, ll D, ll d, ull* keys, ull* rec) {
    k_kd_keys<T><<<(int)((n + 255) / 256), 256, 0, s>>>((const T*)x, (const T*)y, n, D, d, keys, rec);
}

extern "C" {

// Host only. out = {KD_TILE, KD_MAX_N, KD_STAGE, KD_CHUNK, 8-byte words of a
// column's record, scratch bytes, tile blocks, global merge levels}; the last
// three only where (n, D) is covered. -103: not covered.
int ma_kendall_layout(ll n, ll D, ll* out) {
    out[0] = KD_TILE;
    out[1] = KD_MAX_N;
    out[2] = KD_STAGE;
    out[3] = KD_CHUNK;
    out[4] = KD_REC_WORDS;
    out[5] = out[6] = out[7] = 0;
    if (!kd_covers(n, D)) return -103;
    KdScratch sc;
    size_t tmp_bytes;
    int rc = kd_carve(n, &sc, &tmp_bytes);
    if (rc) return rc;
    out[5] = (ll)sc.total;
    out[6] = (n + KD_TILE - 1) / KD_TILE;
    for (ll w = KD_TILE; w < n; w <<= 1) out[7]++;
    return 0;
}

// preds / target: (n, D) contiguous, dtype 0 fp32, 1 bf16, 2 fp16. variant 0 a,
// 1 b, 2 c. record: D * KD_REC_WORDS 8-byte words, tau: D floats; neither needs
// to be cleared. -103: arguments the kernels do not cover; nothing is launched.
int ma_kendall(uintptr_t stream, uintptr_t preds, uintptr_t target, int dtype, ll n, ll D, int variant,
               uintptr_t scratch, ull scratch_bytes, uintptr_t record, uintptr_t tau) {
    if (!kd_covers(n, D) || dtype < 0 || dtype > 2 || variant < 0 || variant > 2) return -103;
    const int esize = dtype == 0 ? 4 : 2;
    if (!preds || !target || preds % esize || target % esize) return -103;
    if (!scratch || scratch % 256 || !record || record % 8 || !tau || tau % 4) return -103;
    KdScratch sc;
    size_t tmp_bytes;
    int rc = kd_carve(n, &sc, &tmp_bytes);
    if (rc) return rc;
    if (sc.total > scratch_bytes) return -103;

    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)scratch;
    ull* keys_a = (ull*)(base + sc.keys_a);
    ull* keys_b = (ull*)(base + sc.keys_b);
    unsigned int* ybuf[2] = {(unsigned int*)keys_a, (unsigned int*)keys_a + n};
    double* part = (double*)(base + sc.part);
    void* tmp = (void*)(base + sc.tmp);
    const ll nb = sc.run_blocks;
    const int run_grid = (int)nb, tile_grid = (int)((n + KD_TILE - 1) / KD_TILE);
    const int merge_grid = (int)((n + KD_CHUNK - 1) / KD_CHUNK);

    const ll words = D * KD_REC_WORDS;
    k_kd_init<<<(int)((words + 255) / 256), 256, 0, s>>>((ull*)record, words);
    OK(hipGetLastError());
    for (ll d = 0; d < D; d++) {
        ull* rec = (ull*)record + d * KD_REC_WORDS;
        if (dtype == 0) kd_keys_launch<float>(s, preds, target, n, D, d, keys_a, rec);
        else if (dtype == 1) kd_keys_launch<uint16_t>(s, preds, target, n, D, d, keys_a, rec);
        else kd_keys_launch<_Float16>(s, preds, target, n, D, d, keys_a, rec);
        OK(hipGetLastError());
        size_t b = tmp_bytes;
        OK(rocprim::radix_sort_keys(tmp, b, keys_a, keys_b, (size_t)n, 0, 64, s));
        k_kd_runs<KD_VIEW_X><<<run_grid, KD_RUN_BLOCK, 0, s>>>(keys_b, n, rec + KD_XTIE, rec + KD_UX, part, part + nb);
        OK(hipGetLastError());
        k_kd_runs<KD_VIEW_XY><<<run_grid, KD_RUN_BLOCK, 0, s>>>(keys_b, n, rec + KD_XYTIE, nullptr, nullptr, nullptr);
        OK(hipGetLastError());
        k_kd_tile<<<tile_grid, KD_TILE_BLOCK, 0, s>>>(keys_b, n, ybuf[0], rec + KD_DIS);
        OK(hipGetLastError());
        int cur = 0;
        for (ll w = KD_TILE; w < n; w <<= 1) {
            k_kd_merge<<<merge_grid, KD_MERGE_BLOCK, 0, s>>>(ybuf[cur], ybuf[cur ^ 1], n, w, rec);
            OK(hipGetLastError());
            cur ^= 1;
        }
        k_kd_runs<KD_VIEW_Y><<<run_grid, KD_RUN_BLOCK, 0, s>>>(ybuf[cur], n, rec + KD_YTIE, rec + KD_UY, part + 2 * nb,
                                                              part + 3 * nb);
        OK(hipGetLastError());
        k_kd_tail<<<1, 256, 0, s>>>(rec, part, nb, n, variant, (float*)tau + d);
        OK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
