// Spearman rank correlation (gfx950): every column of one call through one
// pipeline on the caller's stream, with no host sync and no stored permutation.
// Average ranks are half-integers, so with a = 2 rank_x - (n + 1) and b the same
// for y the three sums the coefficient needs, Sab, Saa and Sbb, are exact
// integers. ma_spearman runs, over all n * D elements at once:
//
//  1. k_sp_keys   x and y, fp32 / bf16 / fp16 read in memory order, each mapped
//     to an order-preserving uint32 (the sign flip; -0.0 becomes +0.0 first, so
//     the two tie; denormals stay distinct, +-inf are ordinary values; every NaN
//     becomes SP_NAN_WORD, above order(+inf)). Pair: key (d << 32) | ux, value
//     uy. A NaN sets the column's flag word.
//  2. sort 1      rocPRIM radix_sort_pairs (double-buffer form) over the bits
//     [0, 32 + bits(D - 1)): column d then lies in [d n, (d + 1) n), x ascending.
//  3. k_sp_rank<A>  a block stages SP_TILE sorted keys in LDS. A wave takes the
//     ballot of key[j] != key[j - 1]; for a lane the first position f of its run
//     is the highest set bit at or below it, the last position l one before the
//     lowest set bit above it. A run that leaves the wave's 64 keys takes its end
//     from a per-chunk carry (first and last head of every chunk of 64, resolved
//     for all chunks by one ballot in wave 0). The two runs that can leave the
//     tile, to the left and to the right, cost one binary search each in global
//     memory, bounded by the column. SP_NAN_WORD is always a head, so NaNs rank
//     last, never tie and (the sort is stable) keep index order. With f, l
//     0-based in the column, a = f + l + 1 - n. Writes the pair of the second
//     sort: key (d << 32) | uy, value a + n - 1; counts the x runs.
//  4. sort 2      the same sort; the x rank rides along as the value.
//  5. k_sp_rank<B>  the same run machinery on the y keys gives b; a comes from
//     the value. Sab, Saa, Sbb and the y runs per block.
//  6. k_sp_tail   one block (a wave where a column has few slots) per column:
//     adds the column's slots, converts to fp64 (hi * 2^64 + lo on the
//     magnitude, then the sign) and applies the formula of
//     _spearman_corrcoef_compute in its order; rho as fp32 into the output, the
//     record next to it.
//
// Two mappings of steps 3 and 5, chosen on the host from n alone:
//  - column tiles (n >= SP_TILE): ceil(n / SP_TILE) blocks per column, tiles
//    aligned to the column start (a 1-D grid, column-major: D may be 65536,
//    above the limit of grid.y). The sums reach n^3 = 2^84: a thread holds int64
//    (SP_PER products below 2^56 each), the block reduces in __int128, xor
//    butterfly in a wave and the waves in index order. One slot per block.
//  - packed columns (n < SP_TILE): a block takes floor(SP_TILE / n) whole
//    columns; heads at the column starts come from the keys' high words. Sums
//    stay below SP_TILE^3: int64 LDS atomics per column (a wave that lies in
//    one column folds first and sends one atomic per sum). One slot per column.
// No global atomics on the sums anywhere; integer adds make every order give
// the same bits.
//
// No matrix instructions: the work is compares and integer adds.

#include <cstring>  // memset, needed by rocprim's texture_cache_iterator header

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <math.h>
#include <stdint.h>

typedef long long ll;
typedef unsigned long long ull;
typedef __int128 i128;

#define OK(x)                                      \
    do {                                           \
        hipError_t err_ = (x);                     \
        if (err_ != hipSuccess) return (int)err_;  \
    } while (0)

// 2048 keys are 16 KiB of LDS: the two global searches a block may need are
// spread over 2048 elements, several blocks still share a CU, and a thread's
// eight head masks stay in registers. 256 threads give each wave 8 ballots.
// Reasoned, not swept (docs/ROADMAP.md).
#define SP_TILE 2048
#define SP_BLOCK 256
#define SP_PER (SP_TILE / SP_BLOCK)
#define SP_CHUNKS (SP_TILE / 64)  // <= 64: one ballot of wave 0 resolves the carries
#define SP_WAVES (SP_BLOCK / 64)
#define SP_PACK_MAX (SP_TILE / 2)  // columns of a packed block (n >= 2)
// Positions and biased ranks are 32-bit, which would allow 2^31 - 1; the scratch
// (two 8-byte key buffers, two 4-byte value buffers, about as much again for
// the sort's own) is about 24 bytes per element: 6 GiB at this count.
#define SP_MAX_ELEMS (1LL << 28)
#define SP_MAX_D 65536
#define SP_NAN_WORD 0xffffffffu  // order(+inf) is 0xff800000
#define SP_SLOT_WORDS 8          // Sab, Saa, Sbb as (lo, hi), x runs, y runs

// the record of a column, 8-byte words
enum { SP_SAB_LO, SP_SAB_HI, SP_SAA_LO, SP_SAA_HI, SP_SBB_LO, SP_SBB_HI, SP_RUNS_X, SP_RUNS_Y, SP_RHO, SP_NAN, SP_REC_WORDS };

enum { SP_MODE_A, SP_MODE_B };

// ------------------------------------------------------------------ key build
__device__ __forceinline__ float sp_f32(float v) { return v; }
__device__ __forceinline__ float sp_f32(_Float16 v) { return (float)v; }
__device__ __forceinline__ float sp_f32(uint16_t v) { return __uint_as_float((unsigned int)v << 16); }  // bf16

__device__ __forceinline__ unsigned int sp_order(float v, bool& nan) {
    unsigned int b = __float_as_uint(v);
    if ((b & 0x7fffffffu) > 0x7f800000u) {
        nan = true;
        return SP_NAN_WORD;
    }
    if ((b << 1) == 0u) b = 0u;  // -0.0 == +0.0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ void __launch_bounds__(256) k_sp_init(unsigned int* __restrict__ flags, int D) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < D) flags[i] = 0u;
}

template <typename T>
__global__ void __launch_bounds__(256) k_sp_keys(
    const T* __restrict__ x, const T* __restrict__ y, ll total, int D, ull* __restrict__ keys,
    unsigned int* __restrict__ vals, unsigned int* __restrict__ flags) {
    const ll e = (ll)blockIdx.x * 256 + threadIdx.x;  // element (i, d) at i * D + d
    if (e >= total) return;
    const unsigned int d = (unsigned int)e % (unsigned int)D;  // total <= SP_MAX_ELEMS: 32 bits hold e
    bool nan = false;
    const unsigned int ux = sp_order(sp_f32(x[e]), nan);
    const unsigned int uy = sp_order(sp_f32(y[e]), nan);
    keys[e] = ((ull)d << 32) | ux;
    vals[e] = uy;
    if (nan) atomicOr(&flags[d], 1u);
}

// ------------------------------------------------------------------ reductions
__device__ __forceinline__ i128 sp_i128(ull lo, ull hi) { return (i128)(((unsigned __int128)hi << 64) | lo); }

template <typename V>
__device__ __forceinline__ V sp_wave_sum(V v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ i128 sp_wave_sum(i128 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const ull lo = __shfl_xor((ull)v, off);
        const ull hi = __shfl_xor((ull)(v >> 64), off);
        v += sp_i128(lo, hi);
    }
    return v;
}

// ------------------------------------------------------------------- rank pass
// keys / vals: the sorted pairs. Mode A writes out_keys / out_vals and word
// SP_RUNS_X of its slots, mode B the six sum words and SP_RUNS_Y. Tiled: block
// d * tiles + t owns tile t of column d, slot = block. Packed: block g owns the
// columns [g * G, min(D, (g + 1) * G)), slot = column.
template <int MODE, bool PACKED>
__global__ void __launch_bounds__(SP_BLOCK) k_sp_rank(
    const ull* __restrict__ keys, const unsigned int* __restrict__ vals, int n, int D, int G, int tiles,
    ull* __restrict__ out_keys, unsigned int* __restrict__ out_vals, ull* __restrict__ part) {
    __shared__ ull tile[SP_TILE];
    __shared__ int s_fh[SP_CHUNKS], s_lh[SP_CHUNKS];      // first / last head of a chunk of 64 (tile index), -1: none
    __shared__ int s_prev[SP_CHUNKS], s_next[SP_CHUNKS];  // the run start before / the head after a chunk
    __shared__ int s_edge[2];                             // the same for the whole tile
    __shared__ ll s_sum[PACKED ? 3 * SP_PACK_MAX : 1];
    __shared__ unsigned int s_cnt[PACKED ? SP_PACK_MAX : 1];
    __shared__ ull s_red[SP_WAVES][SP_SLOT_WORDS];
    const int tid = threadIdx.x, lane = tid & 63;

    // positions are relative to the column start (tiled) or to the block's first column (packed)
    int c0 = 0, len, cols = 1;
    ll g0;
    if (PACKED) {
        const int d0 = blockIdx.x * G;
        cols = min(G, D - d0);
        len = cols * n;
        g0 = (ll)d0 * n;
        for (int j = tid; j < cols; j += SP_BLOCK) {
            s_cnt[j] = 0u;
            if (MODE == SP_MODE_B) s_sum[3 * j] = s_sum[3 * j + 1] = s_sum[3 * j + 2] = 0;
        }
    } else {
        const int d = blockIdx.x / tiles;
        c0 = (blockIdx.x - d * tiles) * SP_TILE;
        len = min(SP_TILE, n - c0);
        g0 = (ll)d * n + c0;
    }
#pragma unroll
    for (int q = 0; q < SP_PER; q++) {
        const int j = q * SP_BLOCK + tid;
        if (j < len) tile[j] = keys[g0 + j];
    }

    // the two runs that may leave the tile: one search each, inside the column
    bool head0 = true;
    if (PACKED) {
        if (tid == 0) {
            s_edge[0] = 0;
            s_edge[1] = len;
        }
    } else {
        const ll col0 = g0 - c0;
        if (tid == 0) {
            int left = c0;
            const ull k = keys[g0];
            if (c0 > 0 && (unsigned int)k != SP_NAN_WORD && keys[g0 - 1] == k) {
                ll lo = col0, hi = g0 - 1;  // the first key equal to k: every key here is <= k
                while (lo < hi) {
                    const ll mid = lo + ((hi - lo) >> 1);
                    if (keys[mid] < k) lo = mid + 1;
                    else hi = mid;
                }
                left = (int)(lo - col0);
            }
            s_edge[0] = left;
            head0 = left == c0;
        }
        if (tid == 64) {
            int right = c0 + len;
            if (right < n) {  // then len == SP_TILE and keys[g0 + len] is in the column
                const ull k = keys[g0 + len - 1];
                if ((unsigned int)k != SP_NAN_WORD && keys[g0 + len] == k) {
                    ll lo = g0 + len + 1, hi = col0 + n;  // the first key past the run
                    while (lo < hi) {
                        const ll mid = lo + ((hi - lo) >> 1);
                        if (keys[mid] == k) lo = mid + 1;
                        else hi = mid;
                    }
                    right = (int)(lo - col0);
                }
            }
            s_edge[1] = right;
        }
    }
    __syncthreads();

    // head flags: a ballot per chunk of 64 keys; the padding behind a short tile is all heads
    ull masks[SP_PER];
#pragma unroll
    for (int q = 0; q < SP_PER; q++) {
        const int j = q * SP_BLOCK + tid;
        bool head = true;
        if (j < len) {
            const ull k = tile[j];
            head = j ? (tile[j - 1] != k || (unsigned int)k == SP_NAN_WORD) : head0;
        }
        const ull m = __ballot(head);
        masks[q] = m;
        if (lane == 0) {
            s_fh[j >> 6] = m ? j + __builtin_ctzll(m) : -1;
            s_lh[j >> 6] = m ? j + 63 - __builtin_clzll(m) : -1;
        }
    }
    __syncthreads();
    if (tid < 64) {  // the carries of all chunks at once
        const bool has = tid < SP_CHUNKS && s_fh[tid] >= 0;
        const ull bm = __ballot(has);
        if (tid < SP_CHUNKS) {
            const ull le = (2ull << tid) - 1ull;  // the bits at or below tid
            const ull below = bm & (le >> 1), above = bm & ~le;
            s_prev[tid] = below ? c0 + s_lh[63 - __builtin_clzll(below)] : s_edge[0];
            s_next[tid] = above ? c0 + s_fh[__builtin_ctzll(above)] : s_edge[1];
        }
    }
    __syncthreads();

    ll sab = 0, saa = 0, sbb = 0;  // a thread's SP_PER products, each below 2^56
    unsigned int heads = 0;
#pragma unroll
    for (int q = 0; q < SP_PER; q++) {
        const int j = q * SP_BLOCK + tid, jw = j - lane;
        if (jw >= len) break;  // wave-uniform
        const bool valid = j < len;
        const ull m = masks[q];
        const ull le = (2ull << lane) - 1ull;
        const ull below = m & le, above = m & ~le;
        const int f = below ? c0 + jw + 63 - __builtin_clzll(below) : s_prev[j >> 6];
        const int l = (above ? c0 + jw + __builtin_ctzll(above) : s_next[j >> 6]) - 1;
        const int col = PACKED ? (valid ? j / n : 0) : 0;
        const int r = f + l + 1 - n - 2 * col * n;  // 2 rank - (n + 1)
        const bool head = valid && ((m >> lane) & 1ull);
        ll pab = 0, paa = 0, pbb = 0;
        if (MODE == SP_MODE_A) {
            if (valid) {
                out_keys[g0 + j] = (tile[j] & 0xffffffff00000000ull) | vals[g0 + j];
                out_vals[g0 + j] = (unsigned int)(r + n - 1);
            }
        } else if (valid) {
            const ll a = (ll)vals[g0 + j] - (n - 1), b = r;
            pab = a * b;
            paa = a * a;
            pbb = b * b;
        }
        if (PACKED) {
            const int first = jw / n, last = min(jw + 63, len - 1) / n;
            if (first == last) {  // the wave lies in one column: fold, then one atomic per sum
                const unsigned int hc = (unsigned int)__popcll(__ballot(head));
                if (MODE == SP_MODE_B) {
                    pab = sp_wave_sum(pab);
                    paa = sp_wave_sum(paa);
                    pbb = sp_wave_sum(pbb);
                }
                if (lane == 0) {
                    atomicAdd(&s_cnt[first], hc);
                    if (MODE == SP_MODE_B) {
                        atomicAdd((ull*)&s_sum[3 * first], (ull)pab);
                        atomicAdd((ull*)&s_sum[3 * first + 1], (ull)paa);
                        atomicAdd((ull*)&s_sum[3 * first + 2], (ull)pbb);
                    }
                }
            } else if (valid) {
                if (head) atomicAdd(&s_cnt[col], 1u);
                if (MODE == SP_MODE_B) {
                    atomicAdd((ull*)&s_sum[3 * col], (ull)pab);
                    atomicAdd((ull*)&s_sum[3 * col + 1], (ull)paa);
                    atomicAdd((ull*)&s_sum[3 * col + 2], (ull)pbb);
                }
            }
        } else {
            heads += head;
            sab += pab;
            saa += paa;
            sbb += pbb;
        }
    }

    if (PACKED) {
        __syncthreads();
        const int d0 = blockIdx.x * G;
        for (int j = tid; j < cols; j += SP_BLOCK) {
            ull* slot = part + (ll)(d0 + j) * SP_SLOT_WORDS;
            if (MODE == SP_MODE_A) slot[SP_RUNS_X] = s_cnt[j];
            else {
                slot[SP_RUNS_Y] = s_cnt[j];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const ll v = s_sum[3 * j + k];
                    slot[2 * k] = (ull)v;
                    slot[2 * k + 1] = (ull)(v >> 63);  // sign extension
                }
            }
        }
    } else {
        const unsigned int hc = sp_wave_sum(heads);
        i128 w[3] = {(i128)sab, (i128)saa, (i128)sbb};
        if (MODE == SP_MODE_B) {
#pragma unroll
            for (int k = 0; k < 3; k++) w[k] = sp_wave_sum(w[k]);
        }
        if (lane == 0) {
            s_red[tid >> 6][6] = hc;
            if (MODE == SP_MODE_B) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    s_red[tid >> 6][2 * k] = (ull)w[k];
                    s_red[tid >> 6][2 * k + 1] = (ull)(w[k] >> 64);
                }
            }
        }
        __syncthreads();
        if (tid == 0) {
            ull* slot = part + (ll)blockIdx.x * SP_SLOT_WORDS;
            ull runs = 0;
            for (int v = 0; v < SP_WAVES; v++) runs += s_red[v][6];
            slot[MODE == SP_MODE_A ? SP_RUNS_X : SP_RUNS_Y] = runs;
            if (MODE == SP_MODE_B) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    i128 s = 0;
                    for (int v = 0; v < SP_WAVES; v++) s += sp_i128(s_red[v][2 * k], s_red[v][2 * k + 1]);
                    slot[2 * k] = (ull)s;
                    slot[2 * k + 1] = (ull)(s >> 64);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------ tail
// One block of 64 or 256 threads per column; nb slots per column. The sums are
// integers: the order they are added in does not change a bit.
__global__ void __launch_bounds__(256) k_sp_tail(
    const ull* __restrict__ part, int nb, int n, const unsigned int* __restrict__ flags, ull* __restrict__ record,
    float* __restrict__ rho_out) {
    __shared__ ull s_red[4][SP_SLOT_WORDS];
    const int tid = threadIdx.x, d = blockIdx.x, waves = blockDim.x >> 6;
    const ull* p = part + (ll)d * nb * SP_SLOT_WORDS;
    i128 s[3] = {0, 0, 0};
    ull rx = 0, ry = 0;
    for (int i = tid; i < nb; i += blockDim.x) {
        const ull* slot = p + (ll)i * SP_SLOT_WORDS;
#pragma unroll
        for (int k = 0; k < 3; k++) s[k] += sp_i128(slot[2 * k], slot[2 * k + 1]);
        rx += slot[SP_RUNS_X];
        ry += slot[SP_RUNS_Y];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) s[k] = sp_wave_sum(s[k]);
    rx = sp_wave_sum(rx);
    ry = sp_wave_sum(ry);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            s_red[tid >> 6][2 * k] = (ull)s[k];
            s_red[tid >> 6][2 * k + 1] = (ull)(s[k] >> 64);
        }
        s_red[tid >> 6][6] = rx;
        s_red[tid >> 6][7] = ry;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int v = 1; v < waves; v++) {
#pragma unroll
        for (int k = 0; k < 3; k++) s[k] += sp_i128(s_red[v][2 * k], s_red[v][2 * k + 1]);
        rx += s_red[v][6];
        ry += s_red[v][7];
    }
    double f[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        // hi * 2^64 + lo on the magnitude: on the two's complement words of a small negative sum, lo is close
        // to 2^64 and its conversion alone would round away up to 2^10. Here hi < 2^53 is exact, lo errs by
        // 2^-53 relative and the sum rounds once more.
        const bool neg = s[k] < 0;
        const unsigned __int128 mag = neg ? -(unsigned __int128)s[k] : (unsigned __int128)s[k];
        const double v = (double)(ull)(mag >> 64) * 18446744073709551616.0 + (double)(ull)mag;
        f[k] = neg ? -v : v;
    }
    const double m = 4.0 * (double)n;
    const double cov = f[0] / m, sx = sqrt(f[1] / m), sy = sqrt(f[2] / m);
    double rho = cov / (sx * sy + 1e-6);
    rho = fmin(fmax(rho, -1.0), 1.0);
    ull* rec = record + (ll)d * SP_REC_WORDS;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        rec[2 * k] = (ull)s[k];
        rec[2 * k + 1] = (ull)(s[k] >> 64);
    }
    rec[SP_RUNS_X] = rx;
    rec[SP_RUNS_Y] = ry;
    ((double*)rec)[SP_RHO] = rho;
    rec[SP_NAN] = flags[d];
    rho_out[d] = (float)rho;
}

// ------------------------------------------------------------------------ host
struct SpPlan {
    bool packed;
    int G, tiles, nb;  // columns per packed block, tiles per column, slots per column
    ll blocks;         // of a rank pass
    unsigned int end_bit;
    size_t keys[2], vals[2], part, flags, tmp, tmp_bytes, total;
};

static inline size_t sp_up(size_t v) { return (v + 255) & ~(size_t)255; }

static inline bool sp_covers(ll n, ll D) {
    return n >= 2 && D >= 1 && D <= SP_MAX_D && n <= SP_MAX_ELEMS && n * D <= SP_MAX_ELEMS;
}

static int sp_plan(ll n, ll D, SpPlan* pl) {
    const ll total = n * D;
    pl->packed = n < SP_TILE;
    pl->G = pl->packed ? (int)(SP_TILE / n) : 1;
    pl->tiles = pl->packed ? 1 : (int)((n + SP_TILE - 1) / SP_TILE);
    pl->nb = pl->tiles;
    pl->blocks = pl->packed ? (D + pl->G - 1) / pl->G : D * pl->tiles;
    pl->end_bit = 32;
    while (pl->end_bit < 64 && ((D - 1) >> (pl->end_bit - 32))) pl->end_bit++;  // D = 1 sorts 32 bits only
    rocprim::double_buffer<ull> k((ull*)nullptr, (ull*)nullptr);
    rocprim::double_buffer<unsigned int> v((unsigned int*)nullptr, (unsigned int*)nullptr);
    pl->tmp_bytes = 0;
    OK(rocprim::radix_sort_pairs((void*)nullptr, pl->tmp_bytes, k, v, (size_t)total, 0u, pl->end_bit));
    pl->keys[0] = 0;
    pl->keys[1] = sp_up(pl->keys[0] + (size_t)total * 8);
    pl->vals[0] = sp_up(pl->keys[1] + (size_t)total * 8);
    pl->vals[1] = sp_up(pl->vals[0] + (size_t)total * 4);
    pl->part = sp_up(pl->vals[1] + (size_t)total * 4);
    pl->flags = sp_up(pl->part + (size_t)D * pl->nb * SP_SLOT_WORDS * 8);
    pl->tmp = sp_up(pl->flags + (size_t)D * 4);
    pl->total = sp_up(pl->tmp + pl->tmp_bytes);
    return 0;
}

template <typename T>
static void sp_keys_launch(hipStream_t s, uintptr_t x, uintptr_t y, ll total, int D, ull* keys, unsigned int* vals,
                           unsigned int* flags) {
    k_sp_keys<T><<<(int)((total + 255) / 256), 256, 0, s>>>((const T*)x, (const T*)y, total, D, keys, vals, flags);
}

template <int MODE>
static void sp_rank_launch(hipStream_t s, const SpPlan& pl, const ull* keys, const unsigned int* vals, int n, int D,
                           ull* out_keys, unsigned int* out_vals, ull* part) {
    if (pl.packed)
        k_sp_rank<MODE, true><<<(int)pl.blocks, SP_BLOCK, 0, s>>>(keys, vals, n, D, pl.G, pl.tiles, out_keys, out_vals, part);
    else
        k_sp_rank<MODE, false><<<(int)pl.blocks, SP_BLOCK, 0, s>>>(keys, vals, n, D, pl.G, pl.tiles, out_keys, out_vals, part);
}

extern "C" {

// Host only. out = {SP_TILE, SP_MAX_ELEMS, SP_MAX_D, 8-byte words of a column's
// record, scratch bytes, 1 for the packed mapping, blocks of a rank pass, slots
// per column}; the last four only where (n, D) is covered. -103: not covered.
int ma_spearman_layout(ll n, ll D, ll* out) {
    out[0] = SP_TILE;
    out[1] = SP_MAX_ELEMS;
    out[2] = SP_MAX_D;
    out[3] = SP_REC_WORDS;
    out[4] = out[5] = out[6] = out[7] = 0;
    if (!sp_covers(n, D)) return -103;
    SpPlan pl;
    int rc = sp_plan(n, D, &pl);
    if (rc) return rc;
    out[4] = (ll)pl.total;
    out[5] = pl.packed;
    out[6] = pl.blocks;
    out[7] = pl.nb;
    return 0;
}

// preds / target: (n, D) contiguous, dtype 0 fp32, 1 bf16, 2 fp16. record:
// D * SP_REC_WORDS 8-byte words, rho: D floats; neither needs to be cleared.
// -103: arguments the kernels do not cover; nothing is launched.
int ma_spearman(uintptr_t stream, uintptr_t preds, uintptr_t target, int dtype, ll n, ll D, uintptr_t scratch,
                ull scratch_bytes, uintptr_t record, uintptr_t rho) {
    if (!sp_covers(n, D) || dtype < 0 || dtype > 2) return -103;
    const int esize = dtype == 0 ? 4 : 2;
    if (!preds || !target || preds % esize || target % esize) return -103;
    if (!scratch || scratch % 256 || !record || record % 8 || !rho || rho % 4) return -103;
    SpPlan pl;
    int rc = sp_plan(n, D, &pl);
    if (rc) return rc;
    if (pl.total > scratch_bytes) return -103;

    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)scratch;
    const ll total = n * D;
    rocprim::double_buffer<ull> keys((ull*)(base + pl.keys[0]), (ull*)(base + pl.keys[1]));
    rocprim::double_buffer<unsigned int> vals((unsigned int*)(base + pl.vals[0]), (unsigned int*)(base + pl.vals[1]));
    ull* part = (ull*)(base + pl.part);
    unsigned int* flags = (unsigned int*)(base + pl.flags);
    void* tmp = (void*)(base + pl.tmp);
    const int ni = (int)n, Di = (int)D;

    k_sp_init<<<(Di + 255) / 256, 256, 0, s>>>(flags, Di);
    OK(hipGetLastError());
    if (dtype == 0) sp_keys_launch<float>(s, preds, target, total, Di, keys.current(), vals.current(), flags);
    else if (dtype == 1) sp_keys_launch<uint16_t>(s, preds, target, total, Di, keys.current(), vals.current(), flags);
    else sp_keys_launch<_Float16>(s, preds, target, total, Di, keys.current(), vals.current(), flags);
    OK(hipGetLastError());
    size_t b = pl.tmp_bytes;
    OK(rocprim::radix_sort_pairs(tmp, b, keys, vals, (size_t)total, 0u, pl.end_bit, s));
    // the spent buffers take the pairs of the second sort, position by position
    sp_rank_launch<SP_MODE_A>(s, pl, keys.current(), vals.current(), ni, Di, keys.alternate(), vals.alternate(), part);
    OK(hipGetLastError());
    keys.swap();
    vals.swap();
    b = pl.tmp_bytes;
    OK(rocprim::radix_sort_pairs(tmp, b, keys, vals, (size_t)total, 0u, pl.end_bit, s));
    sp_rank_launch<SP_MODE_B>(s, pl, keys.current(), vals.current(), ni, Di, nullptr, nullptr, part);
    OK(hipGetLastError());
    k_sp_tail<<<Di, pl.nb > 64 ? 256 : 64, 0, s>>>(part, pl.nb, ni, flags, (ull*)record, (float*)rho);
    OK(hipGetLastError());
    return 0;
}

}  // extern "C"
