// Hausdorff distance between segmentation boundaries (gfx950): every
// (sample, class) plane of one call in two kernels and ONE host sync, with no
// one-hot tensor, no per-plane loop and no dense distance matrix.
//
//  1. k_hd_edges  the edge pass, run twice per tensor: first it COUNTS the edge
//     pixels of every (tensor, n, c) plane and flags a non-binary one-hot value
//     or a label outside [0, C); the host reads counts and flags back (the one
//     sync), sizes the edge buffer exactly and lays out a segment per listed
//     plane; the second run WRITES the edge pixels as packed (y << 16 | x) words
//     into those segments.
//       A wave owns a strip of HD_EDGE_COLS columns by HD_EDGE_ROWS rows. Lane l
//     reads column x0 + l - 1, so lanes 0 and 63 are the halo and left / right
//     neighbours are lane shuffles; the wave walks down its rows with the row
//     above, the row itself and the row below in registers, so every element is
//     loaded once per strip (64/62 * 18/16 of the tensor in all). A pixel is an
//     edge pixel if it belongs to the class and one of its four neighbours does
//     not or lies outside the image. For index inputs a pixel can only be an
//     edge pixel of its own label, so one walk over the labels serves all C
//     planes; the lanes of a row are grouped by label with a ballot per label
//     present. The edge lanes of a group take ONE cursor step (an atomic add of
//     their popcount by the first of them) and place themselves by the popcount
//     of the lanes below. The order inside a segment is whatever the atomics
//     give; max and min do not depend on it.
//  2. k_hd_dist   a block per work item (plane, direction, tile of HD_A_TILE
//     points of A). A lane keeps HD_PTS points of A and their running minima in
//     registers and the block streams B through LDS in tiles of HD_B_TILE
//     words; every lane reads the same LDS words (a broadcast) four at a time.
//     With unit spacing the running value is the exact integer dy^2 + dx^2 (or
//     max / sum of |dy|, |dx|) in 32 bits: one packed 16-bit subtract and one
//     two-element 16-bit dot product where the target has them. Any other
//     spacing takes the fp32 form of the same loop, rounded like the torch
//     chain (two products, two squares, one add, none fused). The sqrt comes
//     after the min and after the max: it is monotone and correctly rounded, so
//     the result is that of sqrt-then-min.
//       Before each B tile a wave reads the plane's current maximum; when all
//     its running minima are at or below it, its points cannot raise the result
//     and it stops computing (it still helps to load tiles until the whole block
//     is done). A stale read only delays that. The block folds its maxima and
//     merges them into the plane's cell with an atomic max on the bit pattern
//     of an unsigned integer or a non-negative float: order-independent, so a
//     call gives the same bits every time. Both directions of the undirected
//     distance share the cell.
//  3. k_hd_tail   cell -> fp32: the sqrt, inf for a plane with one empty side.
//
// No matrix instructions: the inner dimension of the pair product is 2
// (docs/MFMA.md). Nothing here is captured into a graph: the sync rules it out.

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

typedef long long ll;
typedef unsigned long long ull;

#define OK(x)                                      \
    do {                                           \
        hipError_t err_ = (x);                     \
        if (err_ != hipSuccess) return (int)err_;  \
    } while (0)

#define HD_BLOCK 256
#define HD_WAVES (HD_BLOCK / 64)
#define HD_PTS 4                       // points of A per lane
#define HD_A_TILE (HD_BLOCK * HD_PTS)  // points of A per block
#define HD_B_TILE 4096                 // words of B per LDS tile (16 KiB)
#define HD_EDGE_COLS 62                // columns a wave owns (64 lanes less the halo)
#define HD_EDGE_ROWS 16                // rows a wave walks
#define HD_MAX_DIM 32768               // 16-bit packing, 32-bit squared distance
#define HD_ITEM_WORDS 5                // a_off, a_cnt, b_off, b_cnt, cell

#define HD_FLAG_NOT_BINARY 1
#define HD_FLAG_LABEL_RANGE 2

enum { HD_EUCLIDEAN, HD_CHESSBOARD, HD_TAXICAB };

typedef short hd_short2 __attribute__((ext_vector_type(2)));

#if defined(__HIP_DEVICE_COMPILE__) && defined(__has_builtin)
#if __has_builtin(__builtin_amdgcn_sdot2) && (defined(__gfx950__) || defined(__gfx942__) || defined(__gfx90a__))
#define HD_HAVE_DOT2 1
#endif
#endif

// ------------------------------------------------------------------ edge pass
// What a pixel is to the pass: for index inputs its label (-1 outside the
// image, -2 out of range), for one-hot inputs 1 / 0 (0 outside the image).
template <typename T, bool ONEHOT>
__device__ __forceinline__ int hd_classify(T raw, int C, int& bad) {
    const ll v = (ll)raw;
    if (ONEHOT) {
        if (v != 0 && v != 1) bad |= HD_FLAG_NOT_BINARY;
        return v == 1 ? 1 : 0;
    }
    if (v < 0 || v >= C) {
        bad |= HD_FLAG_LABEL_RANGE;
        return -2;
    }
    return (int)v;
}

// x: (images, H, W); index inputs have N images and C planes each, one-hot
// inputs N * C images of one plane. counts / base / cursor are indexed by
// plane = n * C + c. WRITE false: counts and flag. WRITE true: the packed
// pixels of every plane with base[plane] >= 0.
template <typename T, bool ONEHOT, bool WRITE>
__global__ void __launch_bounds__(HD_BLOCK) k_hd_edges(
    const T* __restrict__ x, ll images, int C, int H, int W, int tiles_x, int tiles_y, ll n_strips,
    int* __restrict__ counts, int* __restrict__ flag, const ll* __restrict__ base,
    unsigned int* __restrict__ cursor, unsigned int* __restrict__ edges) {
    const int lane = threadIdx.x & 63;
    const ll strip = (ll)blockIdx.x * HD_WAVES + (threadIdx.x >> 6);
    if (strip >= n_strips) return;  // wave-uniform; the kernel has no barrier
    const int tx = (int)(strip % tiles_x);
    const int ty = (int)((strip / tiles_x) % tiles_y);
    const ll img = strip / ((ll)tiles_x * tiles_y);
    const int xx = tx * HD_EDGE_COLS + lane - 1;
    const int y0 = ty * HD_EDGE_ROWS;
    const bool col_ok = xx >= 0 && xx < W;
    const bool inner = lane >= 1 && lane <= HD_EDGE_COLS && xx < W;
    const int OUTSIDE = ONEHOT ? 0 : -1;
    const T* __restrict__ plane = x + img * (ll)H * W;
    const ull below = lane ? (~0ull >> (64 - lane)) : 0ull;  // the lanes under this one

    int bad = 0;
    int acc = 0;  // one-hot count of the strip
    int up = (col_ok && y0 > 0) ? hd_classify<T, ONEHOT>(plane[(ll)(y0 - 1) * W + xx], C, bad) : OUTSIDE;
    int cur = col_ok ? hd_classify<T, ONEHOT>(plane[(ll)y0 * W + xx], C, bad) : OUTSIDE;
    const int y_end = min(y0 + HD_EDGE_ROWS, H);
    for (int y = y0; y < y_end; y++) {
        const int dn = (col_ok && y + 1 < H) ? hd_classify<T, ONEHOT>(plane[(ll)(y + 1) * W + xx], C, bad) : OUTSIDE;
        const int left = __shfl_up(cur, 1);
        const int right = __shfl_down(cur, 1);
        const bool member = ONEHOT ? cur == 1 : cur >= 0;
        const bool e = inner && member && (up != cur || dn != cur || left != cur || right != cur);
        ull rem = __ballot(e);
        while (rem) {  // one turn per class with an edge pixel in this row
            const int leader = __builtin_ctzll(rem);
            const int c = ONEHOT ? 0 : __shfl(cur, leader);
            const ull m = ONEHOT ? rem : __ballot(e && cur == c);
            const ll p = ONEHOT ? img : img * C + c;
            const int cnt = __popcll(m);
            if (!WRITE) {
                if (ONEHOT) acc += cnt;
                else if (lane == leader) atomicAdd(&counts[p], cnt);
            } else {
                const ll b = base[p];
                if (b >= 0) {
                    unsigned int s = 0;
                    if (lane == leader) s = atomicAdd(&cursor[p], (unsigned int)cnt);
                    s = __shfl(s, leader);
                    if ((m >> lane) & 1ull)
                        edges[b + s + __popcll(m & below)] = ((unsigned int)y << 16) | (unsigned int)xx;
                }
            }
            rem &= ~m;
        }
        up = cur;
        cur = dn;
    }
    if (!WRITE) {
        if (ONEHOT && lane == 0 && acc) atomicAdd(&counts[img], acc);
        if (__any(bad)) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) bad |= __shfl_xor(bad, off);
            if (lane == 0) atomicOr(flag, bad);
        }
    }
}

// ------------------------------------------------------------ distance kernel
template <bool F32>
struct HdVal {
    typedef unsigned int type;
};
template <>
struct HdVal<true> {
    typedef float type;
};

// the value of one (a, b) pair; a and b are packed (y << 16 | x) words
template <int METRIC, bool F32>
__device__ __forceinline__ typename HdVal<F32>::type hd_pair(unsigned int a, unsigned int b, float s0, float s1) {
    if constexpr (!F32 && METRIC == HD_EUCLIDEAN) {
#ifdef HD_HAVE_DOT2
        // both halves differ by less than 2^15 and 2 * 32767^2 < 2^31
        const hd_short2 d = __builtin_bit_cast(hd_short2, a) - __builtin_bit_cast(hd_short2, b);
        return (unsigned int)__builtin_amdgcn_sdot2(d, d, 0, false);
#else
        const int dx = (int)(a & 0xffffu) - (int)(b & 0xffffu);
        const int dy = (int)(a >> 16) - (int)(b >> 16);
        return (unsigned int)(__mul24(dx, dx) + __mul24(dy, dy));
#endif
    } else {
        const int dx = abs((int)(a & 0xffffu) - (int)(b & 0xffffu));
        const int dy = abs((int)(a >> 16) - (int)(b >> 16));
        if constexpr (!F32) {
            return (unsigned int)(METRIC == HD_CHESSBOARD ? max(dy, dx) : dy + dx);
        } else {
            const float fy = __fmul_rn(s0, (float)dy), fx = __fmul_rn(s1, (float)dx);
            if constexpr (METRIC == HD_EUCLIDEAN) return __fadd_rn(__fmul_rn(fy, fy), __fmul_rn(fx, fx));
            else if constexpr (METRIC == HD_CHESSBOARD) return fmaxf(fy, fx);
            else return __fadd_rn(fy, fx);
        }
    }
}

template <bool F32>
__device__ __forceinline__ unsigned int hd_bits(typename HdVal<F32>::type v) {
    if constexpr (F32) return __float_as_uint(v);  // non-negative: the bits order like the values
    else return v;
}

template <int METRIC, bool F32>
__global__ void __launch_bounds__(HD_BLOCK) k_hd_dist(
    const ll* __restrict__ items, const unsigned int* __restrict__ edges, unsigned int* __restrict__ cells,
    float s0, float s1) {
    typedef typename HdVal<F32>::type V;
    __shared__ __attribute__((aligned(16))) unsigned int btile[HD_B_TILE];
    __shared__ unsigned int red[HD_WAVES];
    const ll* it = items + (ll)blockIdx.x * HD_ITEM_WORDS;
    const unsigned int* __restrict__ A = edges + it[0];
    const int a_cnt = (int)it[1];  // 1 .. HD_A_TILE
    const unsigned int* __restrict__ B = edges + it[2];
    const ll b_cnt = it[3];  // >= 1
    unsigned int* cell = cells + it[4];
    const int tid = threadIdx.x;

    unsigned int a[HD_PTS];
    V m[HD_PTS];
#pragma unroll
    for (int q = 0; q < HD_PTS; q++) {
        const int i = q * HD_BLOCK + tid;
        const bool valid = i < a_cnt;
        a[q] = valid ? A[i] : 0u;
        if constexpr (F32) m[q] = valid ? INFINITY : 0.0f;  // an absent point never raises the maximum
        else m[q] = valid ? 0xffffffffu : 0u;
    }

    bool done = false;
    for (ll t0 = 0; t0 < b_cnt; t0 += HD_B_TILE) {
        const int n = (int)min((ll)HD_B_TILE, b_cnt - t0);
        const int n4 = (n + 3) & ~3;  // padded with copies of the tile's first point
        if (t0) __syncthreads();      // the tile before is consumed
        for (int j = tid; j < n4; j += HD_BLOCK) btile[j] = B[t0 + (j < n ? j : 0)];
        if (!done) {
            const unsigned int now = __atomic_load_n(cell, __ATOMIC_RELAXED);
            bool under = true;
#pragma unroll
            for (int q = 0; q < HD_PTS; q++) under = under && hd_bits<F32>(m[q]) <= now;
            done = __all(under);
        }
        if (__syncthreads_and(done)) break;
        if (done) continue;
        for (int j = 0; j < n4; j += 4) {
            const uint4 w = *reinterpret_cast<const uint4*>(&btile[j]);
            const unsigned int bw[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int u = 0; u < 4; u++) {
#pragma unroll
                for (int q = 0; q < HD_PTS; q++) {
                    const V d = hd_pair<METRIC, F32>(a[q], bw[u], s0, s1);
                    m[q] = d < m[q] ? d : m[q];
                }
            }
        }
    }

    unsigned int mx = 0;
#pragma unroll
    for (int q = 0; q < HD_PTS; q++) mx = max(mx, hd_bits<F32>(m[q]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned int)__shfl_xor((int)mx, off));
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < HD_WAVES; w++) mx = max(mx, red[w]);
        atomicMax(cell, mx);
    }
}

__global__ void __launch_bounds__(256) k_hd_tail(
    const ll* __restrict__ half_empty, const unsigned int* __restrict__ cells, ll K, int metric, int f32,
    float* __restrict__ out) {
    const ll k = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    float v;
    if (half_empty[k]) v = INFINITY;
    else if (f32) v = metric == HD_EUCLIDEAN ? sqrtf(__uint_as_float(cells[k])) : __uint_as_float(cells[k]);
    else v = metric == HD_EUCLIDEAN ? (float)sqrt((double)cells[k]) : (float)cells[k];
    out[k] = v;
}

// ----------------------------------------------------------------------- host
struct HdGeom {
    int tiles_x, tiles_y;
    ll images, n_strips, planes;
    int grid;
};

static bool hd_geom(int onehot, ll N, ll C, ll H, ll W, HdGeom* g) {
    if (N < 1 || C < 1 || H < 1 || W < 1 || H > HD_MAX_DIM || W > HD_MAX_DIM) return false;
    if (N * C > 0x1fffffffLL) return false;  // 4 * planes + 1 ints of header
    g->planes = N * C;
    g->images = onehot ? N * C : N;
    g->tiles_x = (int)((W + HD_EDGE_COLS - 1) / HD_EDGE_COLS);
    g->tiles_y = (int)((H + HD_EDGE_ROWS - 1) / HD_EDGE_ROWS);
    g->n_strips = g->images * g->tiles_x * g->tiles_y;
    const ll grid = (g->n_strips + HD_WAVES - 1) / HD_WAVES;
    if (grid > 0x7fffffffLL) return false;
    g->grid = (int)grid;
    return true;
}

template <typename T, bool ONEHOT>
static int hd_edges_launch(hipStream_t s, const HdGeom& g, bool write, uintptr_t x, int C, int H, int W,
                           int* counts, int* flag, const ll* base, unsigned int* cursor, unsigned int* edges) {
    if (write)
        k_hd_edges<T, ONEHOT, true><<<g.grid, HD_BLOCK, 0, s>>>(
            (const T*)x, g.images, C, H, W, g.tiles_x, g.tiles_y, g.n_strips, counts, flag, base, cursor, edges);
    else
        k_hd_edges<T, ONEHOT, false><<<g.grid, HD_BLOCK, 0, s>>>(
            (const T*)x, g.images, C, H, W, g.tiles_x, g.tiles_y, g.n_strips, counts, flag, base, cursor, edges);
    return (int)hipGetLastError();
}

// dtype 0 uint8 / bool, 1 int8, 2 int16, 3 int32, 4 int64
static int hd_edges(hipStream_t s, bool write, uintptr_t x, int onehot, int dtype, ll N, int C, int H, int W,
                    int* counts, int* flag, const ll* base, unsigned int* cursor, unsigned int* edges) {
    HdGeom g;
    if (!hd_geom(onehot, N, C, H, W, &g)) return -103;
#define HD_CASE(code, T)                                                                                       \
    case code:                                                                                                 \
        return onehot ? hd_edges_launch<T, true>(s, g, write, x, C, H, W, counts, flag, base, cursor, edges)   \
                      : hd_edges_launch<T, false>(s, g, write, x, C, H, W, counts, flag, base, cursor, edges);
    switch (dtype) {
        HD_CASE(0, uint8_t)
        HD_CASE(1, int8_t)
        HD_CASE(2, int16_t)
        HD_CASE(3, int32_t)
        HD_CASE(4, int64_t)
    }
#undef HD_CASE
    return -103;
}

static bool hd_tensor_ok(uintptr_t x, int onehot, int dtype) {
    static const int size[5] = {1, 1, 2, 4, 8};
    return x && (onehot == 0 || onehot == 1) && dtype >= 0 && dtype <= 4 && x % size[dtype] == 0;
}

template <int METRIC>
static void hd_dist_launch(hipStream_t s, int f32, ll n_items, const ll* items, const unsigned int* edges,
                           unsigned int* cells, float s0, float s1) {
    if (f32) k_hd_dist<METRIC, true><<<(int)n_items, HD_BLOCK, 0, s>>>(items, edges, cells, s0, s1);
    else k_hd_dist<METRIC, false><<<(int)n_items, HD_BLOCK, 0, s>>>(items, edges, cells, s0, s1);
}

extern "C" {

// Host only. out = {points of A per block, words of B per LDS tile, largest H
// or W covered, header ints (flag, 2 * planes counts, 2 * planes cursors),
// edge-pass blocks of an index tensor, of a one-hot tensor}. -103: not covered.
int ma_hausdorff_layout(ll N, ll C, ll H, ll W, ll* out) {
    out[0] = HD_A_TILE;
    out[1] = HD_B_TILE;
    out[2] = HD_MAX_DIM;
    HdGeom gi, go;
    if (!hd_geom(0, N, C, H, W, &gi) || !hd_geom(1, N, C, H, W, &go)) return -103;
    out[3] = 1 + 4 * gi.planes;
    out[4] = gi.grid;
    out[5] = go.grid;
    return 0;
}

// Phase 1: counts and flags. hdr is the zeroed header: [0] flags, then the edge
// counts of preds [planes], of target [planes], then as many cursors.
int ma_hausdorff_count(uintptr_t stream, uintptr_t preds, int p_onehot, int p_dtype, uintptr_t target, int t_onehot,
                       int t_dtype, ll N, ll C, ll H, ll W, uintptr_t hdr) {
    HdGeom g;
    if (!hd_geom(0, N, C, H, W, &g) || !hdr || hdr % 4) return -103;
    if (!hd_tensor_ok(preds, p_onehot, p_dtype) || !hd_tensor_ok(target, t_onehot, t_dtype)) return -103;
    hipStream_t s = (hipStream_t)stream;
    int* h = (int*)hdr;
    int rc = hd_edges(s, false, preds, p_onehot, p_dtype, N, (int)C, (int)H, (int)W, h + 1, h, nullptr, nullptr,
                      nullptr);
    if (rc) return rc;
    return hd_edges(s, false, target, t_onehot, t_dtype, N, (int)C, (int)H, (int)W, h + 1 + g.planes, h, nullptr,
                    nullptr, nullptr);
}

// Phase 2, after the host has read the header. table (int64): the segment
// start of every (tensor, plane) in `edges`, -1 for a plane that is not listed
// [2 * planes]; one word per listed plane, non-zero where exactly one side is
// empty [K]; the work items, HD_ITEM_WORDS each [n_items]. cells: K zeroed
// words. out: K floats. metric 0 euclidean, 1 chessboard, 2 taxicab; f32 0:
// unit spacing, integer arithmetic.
int ma_hausdorff_run(uintptr_t stream, uintptr_t preds, int p_onehot, int p_dtype, uintptr_t target, int t_onehot,
                     int t_dtype, ll N, ll C, ll H, ll W, uintptr_t hdr, uintptr_t table, ll K, ll n_items,
                     uintptr_t edges, int metric, int f32, float s0, float s1, uintptr_t cells, uintptr_t out) {
    HdGeom g;
    if (!hd_geom(0, N, C, H, W, &g) || !hdr || hdr % 4 || !table || table % 8 || !edges || edges % 4) return -103;
    if (!hd_tensor_ok(preds, p_onehot, p_dtype) || !hd_tensor_ok(target, t_onehot, t_dtype)) return -103;
    if (K < 1 || K > g.planes || n_items < 0 || n_items > 0x7fffffffLL || metric < 0 || metric > 2) return -103;
    if (!cells || cells % 4 || !out || out % 4) return -103;
    hipStream_t s = (hipStream_t)stream;
    int* h = (int*)hdr;
    const ll* base = (const ll*)table;
    unsigned int* cursor = (unsigned int*)(h + 1 + 2 * g.planes);
    int rc = hd_edges(s, true, preds, p_onehot, p_dtype, N, (int)C, (int)H, (int)W, nullptr, nullptr, base, cursor,
                      (unsigned int*)edges);
    if (rc) return rc;
    rc = hd_edges(s, true, target, t_onehot, t_dtype, N, (int)C, (int)H, (int)W, nullptr, nullptr, base + g.planes,
                  cursor + g.planes, (unsigned int*)edges);
    if (rc) return rc;
    const ll* half_empty = base + 2 * g.planes;
    const ll* items = half_empty + K;
    if (n_items) {
        if (metric == HD_EUCLIDEAN)
            hd_dist_launch<HD_EUCLIDEAN>(s, f32, n_items, items, (const unsigned int*)edges, (unsigned int*)cells, s0, s1);
        else if (metric == HD_CHESSBOARD)
            hd_dist_launch<HD_CHESSBOARD>(s, f32, n_items, items, (const unsigned int*)edges, (unsigned int*)cells, s0, s1);
        else
            hd_dist_launch<HD_TAXICAB>(s, f32, n_items, items, (const unsigned int*)edges, (unsigned int*)cells, s0, s1);
        OK(hipGetLastError());
    }
    k_hd_tail<<<(int)((K + 255) / 256), 256, 0, s>>>(half_empty, (const unsigned int*)cells, K, metric, f32,
                                                      (float*)out);
    OK(hipGetLastError());
    return 0;
}

}  // extern "C"
