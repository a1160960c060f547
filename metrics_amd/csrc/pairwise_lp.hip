// Pairwise L_p distances (gfx950): pairwise_manhattan_distance and
// pairwise_minkowski_distance,
//     out[i, j] = (sum_k |x[i, k] - y[j, k]|^p)^(1/p),   x (N, D), y (M, D),
// without the (N, M, D) temporaries of the torch chain: the inputs are read
// O((N + M) * D) times a tile side, the result is written once, and with a
// reduction no (N, M) matrix exists at all. |a - b|^p is not bilinear, so this
// is no GEMM and has no use for matrix instructions (docs/MFMA.md): the work is
// two or three fp32 vector instructions per (i, j, k).
//
//  1. k_pairwise_lp  a block of LP_BLOCK = 256 lanes owns an LP_TN x LP_TM =
//     128 x 128 output tile, a lane an 8 x 8 micro-tile of fp32 accumulators
//     that stay in registers over the whole D loop: rows ty*4..+3 and
//     64+ty*4..+3, columns tx*4..+3 and 64+tx*4..+3 (tx = lane % 16, ty =
//     lane / 16), so that the eight row values and the eight column values of
//     one k are two 16-byte LDS reads each. Within a wave the row reads hit 4
//     addresses (broadcast) and the column reads 16 consecutive 16-byte words:
//     no bank conflict.
//       D is walked in chunks of LP_KC = 16. A chunk of the tile's x rows and y
//     rows is staged in LDS k-major, [k][row]: a lane fetches 8 consecutive k
//     of one row (row = lane % 128, k half = lane / 128) with 16-byte loads
//     where the row stride and the base allow it (fp32: D % 4 == 0, 16-bit:
//     D % 8 == 0, base 16-byte aligned), scalar loads otherwise, converts to
//     fp32 and writes the 8 values transposed; the lanes of a wave write 64
//     consecutive words of one k: no bank conflict either. The D tail and the
//     rows beyond N / M are staged as zeros on both sides, |0 - 0|^p = 0 for
//     every p > 0. Two LDS buffers: chunk c + 1 is fetched into registers
//     before chunk c is consumed and written to the other buffer after, one
//     barrier per chunk.
//       The inner loop is chosen at compile time by exponent class: p = 1 sub,
//     add |d|; p = 2 sub, fma; p = 3 sub, mul, fma; p = 4 sub, mul, fma; any
//     other p > 0 powf(|d|, p). fp32, ascending k, one accumulator per element.
//       Epilogue: root (none, sqrtf, cbrtf, sqrtf twice, fp64 pow), 0 on i == j if
//     asked, ONE rounding to the input dtype, then either the tile is stored
//     (64-bit offsets, 4 elements per store where M % 4 == 0), or, for "sum" /
//     "mean", the ROUNDED elements of the valid columns are folded in fp64: a
//     lane its 8 columns in a fixed order, then one lane per row the 16 lane
//     sums through LDS in ascending order. The block writes one fp32 partial per
//     (column tile, row). No float atomics: repeats give the same bits.
//  2. k_pairwise_lp_rows  a lane per row adds the partials of the row in
//     ascending tile order in fp64, divides by M for "mean" and writes (N,) in
//     the input dtype.
//
// Capture into a graph is untested.

#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <stdint.h>

typedef long long ll;

#define OK(x)                                      \
    do {                                           \
        hipError_t err_ = (x);                     \
        if (err_ != hipSuccess) return (int)err_;  \
    } while (0)

#define LP_TN 128      // rows of x of a block's tile
#define LP_TM 128      // rows of y (columns of the output) of a block's tile
#define LP_KC 16       // k of a staged chunk
#define LP_BLOCK 256
#define LP_ROWS_BLOCK 256  // rows of a block of k_pairwise_lp_rows

static_assert(LP_TN == 128 && LP_TM == 128 && LP_BLOCK == 256 && LP_KC == 16,
              "the lane mapping below is written for a 128 x 128 tile, 256 lanes and 8 k per lane and side");

enum { LP_F32, LP_BF16, LP_F16 };          // dtype codes of the entry
enum { LP_NONE, LP_SUM, LP_MEAN };         // reduction codes of the entry
enum { LP_POW, LP_P1, LP_P2, LP_P3, LP_P4 };  // exponent classes

struct LpBf16 {
    uint16_t v;
};

__device__ inline float lp_f32(float v) { return v; }
__device__ inline float lp_f32(_Float16 v) { return (float)v; }
__device__ inline float lp_f32(LpBf16 v) { return __uint_as_float((uint32_t)v.v << 16); }

// one rounding to nearest even, as torch's .to(dtype)
__device__ inline void lp_round(float f, float* o) { *o = f; }
__device__ inline void lp_round(float f, _Float16* o) { *o = (_Float16)f; }
__device__ inline void lp_round(float f, LpBf16* o) {
    uint32_t u = __float_as_uint(f);
    if (f != f) {
        o->v = 0x7fc0;
        return;
    }
    u += 0x7fffu + ((u >> 16) & 1u);
    o->v = (uint16_t)(u >> 16);
}

// 8 consecutive k of one row from k0 on as fp32; zeros beyond `rows` and D.
// vec: every row starts 16-byte aligned, and D is a multiple of a 16-byte
// vector's elements (k0 is a multiple of 8), so a vector lies inside D or outside.
template <typename T>
__device__ inline void lp_fetch(const T* __restrict__ base, ll rows, ll D, ll row, ll k0, bool vec, float (&r)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) r[q] = 0.f;
    if (row >= rows || k0 >= D) return;
    const T* p = base + row * D + k0;
    if (vec) {
        alignas(16) T tmp[8];
        if constexpr (sizeof(T) == 4) {
            *(uint4*)tmp = *(const uint4*)p;
            if (k0 + 4 < D) *(uint4*)(tmp + 4) = *(const uint4*)(p + 4);
            else *(uint4*)(tmp + 4) = make_uint4(0, 0, 0, 0);
        } else {
            *(uint4*)tmp = *(const uint4*)p;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) r[q] = lp_f32(tmp[q]);
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (k0 + q < D) r[q] = lp_f32(p[q]);
    }
}

template <int PC>
__device__ inline float lp_term(float d, float acc, float p) {
    if constexpr (PC == LP_P1) return acc + fabsf(d);
    else if constexpr (PC == LP_P2) return fmaf(d, d, acc);
    else if constexpr (PC == LP_P3) {
        const float a = fabsf(d);
        return fmaf(a * a, a, acc);
    } else if constexpr (PC == LP_P4) {
        const float d2 = d * d;
        return fmaf(d2, d2, acc);
    } else return acc + powf(fabsf(d), p);
}

// the generic root runs once per element: fp64 keeps it at one rounding
template <int PC>
__device__ inline float lp_root(float acc, double inv_p) {
    if constexpr (PC == LP_P1) return acc;
    else if constexpr (PC == LP_P2) return sqrtf(acc);
    else if constexpr (PC == LP_P3) return cbrtf(acc);
    else if constexpr (PC == LP_P4) return sqrtf(sqrtf(acc));
    else return (float)pow((double)acc, inv_p);
}

template <typename T, int PC>
__global__ __launch_bounds__(LP_BLOCK) void k_pairwise_lp(const T* __restrict__ x, const T* __restrict__ y, ll N, ll M,
                                                          ll D, int tiles_n, float p, double inv_p, int zero_diag,
                                                          int reduce, int vec_x, int vec_y, T* __restrict__ out,
                                                          float* __restrict__ partial) {
    // [buffer][x | y][k][row]; the reduction's fold reuses it as [16][LP_TN] fp64
    __shared__ alignas(16) float lds[2][2][LP_KC][LP_TN];
    static_assert(sizeof(lds) >= 16 * LP_TN * sizeof(double), "the fold must fit the staging buffers");

    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int tn = blockIdx.x % tiles_n, tm = blockIdx.x / tiles_n;
    const ll r0 = (ll)tn * LP_TN, c0 = (ll)tm * LP_TM;
    const int lrow = tid & (LP_TN - 1), lk = (tid >> 7) * 8;  // what this lane stages

    float acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;

    float rx[8], ry[8];
    lp_fetch(x, N, D, r0 + lrow, lk, vec_x, rx);
    lp_fetch(y, M, D, c0 + lrow, lk, vec_y, ry);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        lds[0][0][lk + q][lrow] = rx[q];
        lds[0][1][lk + q][lrow] = ry[q];
    }
    __syncthreads();

    const ll chunks = (D + LP_KC - 1) / LP_KC;
    for (ll c = 0; c < chunks; ++c) {
        const int cur = (int)(c & 1);
        const bool more = c + 1 < chunks;
        if (more) {
            lp_fetch(x, N, D, r0 + lrow, (c + 1) * LP_KC + lk, vec_x, rx);
            lp_fetch(y, M, D, c0 + lrow, (c + 1) * LP_KC + lk, vec_y, ry);
        }
        // powf is some hundred instructions: its loop body holds one k
        constexpr int unroll_k = PC == LP_POW ? 1 : 4;
#pragma unroll unroll_k
        for (int k = 0; k < LP_KC; ++k) {
            const float4 a0 = *(const float4*)&lds[cur][0][k][ty * 4];
            const float4 a1 = *(const float4*)&lds[cur][0][k][64 + ty * 4];
            const float4 b0 = *(const float4*)&lds[cur][1][k][tx * 4];
            const float4 b1 = *(const float4*)&lds[cur][1][k][64 + tx * 4];
            const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] = lp_term<PC>(a[i] - b[j], acc[i][j], p);
        }
        if (more) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                lds[cur ^ 1][0][lk + q][lrow] = rx[q];
                lds[cur ^ 1][1][lk + q][lrow] = ry[q];
            }
        }
        __syncthreads();  // the other buffer is full, and this one is free for chunk c + 2
    }

    double* fold = (double*)&lds[0][0][0][0];  // [tx][row of the tile]; every lane is past the last barrier
    const bool vec_out = (M & 3) == 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int li = (i < 4 ? 0 : 64) + ty * 4 + (i & 3);
        const ll gi = r0 + li;
        alignas(16) T o[8];
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const ll gj = c0 + (j < 4 ? 0 : 64) + tx * 4 + (j & 3);
            float v = lp_root<PC>(acc[i][j], inv_p);
            if (zero_diag && gi == gj) v = 0.f;
            lp_round(v, &o[j]);
            if (reduce && gj < M) s += (double)lp_f32(o[j]);
        }
        if (reduce) {
            fold[tx * LP_TN + li] = s;
        } else if (gi < N) {
            T* orow = out + (size_t)gi * (size_t)M;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const ll gj = c0 + h * 64 + tx * 4;
                if (vec_out) {  // M % 4 == 0: the four columns lie inside M or outside, and the store is aligned
                    if (gj < M) {
                        if constexpr (sizeof(T) == 4) *(uint4*)(orow + gj) = *(const uint4*)&o[h * 4];
                        else *(uint2*)(orow + gj) = *(const uint2*)&o[h * 4];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (gj + j < M) orow[gj + j] = o[h * 4 + j];
                }
            }
        }
    }
    if (reduce) {
        __syncthreads();
        if (tid < LP_TN && r0 + tid < N) {
            double s = 0.0;
#pragma unroll
            for (int t = 0; t < 16; ++t) s += fold[t * LP_TN + tid];
            partial[(size_t)tm * (size_t)N + (size_t)(r0 + tid)] = (float)s;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(LP_ROWS_BLOCK) void k_pairwise_lp_rows(const float* __restrict__ partial, ll N, int tiles_m,
                                                                   ll divide_by, T* __restrict__ out) {
    const ll r = (ll)blockIdx.x * LP_ROWS_BLOCK + threadIdx.x;
    if (r >= N) return;
    double s = 0.0;
    for (int t = 0; t < tiles_m; ++t) s += (double)partial[(size_t)t * (size_t)N + (size_t)r];
    lp_round((float)(s / (double)divide_by), &out[r]);
}

struct LpGeom {
    ll tiles_n, tiles_m, grid, partial_floats;
};

// false: a call the kernels do not cover
static bool lp_geom(ll N, ll M, ll D, LpGeom* g) {
    if (N <= 0 || M <= 0 || D <= 0) return false;
    g->tiles_n = (N + LP_TN - 1) / LP_TN;
    g->tiles_m = (M + LP_TM - 1) / LP_TM;
    if (g->tiles_n > INT_MAX || g->tiles_m > INT_MAX || g->tiles_n > INT_MAX / g->tiles_m) return false;
    if ((N + LP_ROWS_BLOCK - 1) / LP_ROWS_BLOCK > INT_MAX) return false;
    g->grid = g->tiles_n * g->tiles_m;
    g->partial_floats = N * g->tiles_m;
    return true;
}

template <typename T, int PC>
static void lp_launch(hipStream_t s, const LpGeom& g, uintptr_t x, uintptr_t y, ll N, ll M, ll D, double p, int zero_diag,
                      int reduction, uintptr_t out, float* partial) {
    const int per_vec = 16 / (int)sizeof(T);
    const int vec_x = x % 16 == 0 && D % per_vec == 0, vec_y = y % 16 == 0 && D % per_vec == 0;
    k_pairwise_lp<T, PC><<<(unsigned)g.grid, LP_BLOCK, 0, s>>>((const T*)x, (const T*)y, N, M, D, (int)g.tiles_n, (float)p,
                                                              1.0 / p, zero_diag, reduction != LP_NONE, vec_x,
                                                              vec_y, (T*)out, partial);
    if (reduction != LP_NONE)
        k_pairwise_lp_rows<T><<<(unsigned)((N + LP_ROWS_BLOCK - 1) / LP_ROWS_BLOCK), LP_ROWS_BLOCK, 0, s>>>(
            partial, N, (int)g.tiles_m, reduction == LP_MEAN ? M : 1, (T*)out);
}

template <typename T>
static void lp_by_exponent(hipStream_t s, const LpGeom& g, uintptr_t x, uintptr_t y, ll N, ll M, ll D, double p,
                           int zero_diag, int reduction, uintptr_t out, float* partial) {
    if (p == 1.0) lp_launch<T, LP_P1>(s, g, x, y, N, M, D, p, zero_diag, reduction, out, partial);
    else if (p == 2.0) lp_launch<T, LP_P2>(s, g, x, y, N, M, D, p, zero_diag, reduction, out, partial);
    else if (p == 3.0) lp_launch<T, LP_P3>(s, g, x, y, N, M, D, p, zero_diag, reduction, out, partial);
    else if (p == 4.0) lp_launch<T, LP_P4>(s, g, x, y, N, M, D, p, zero_diag, reduction, out, partial);
    else lp_launch<T, LP_POW>(s, g, x, y, N, M, D, p, zero_diag, reduction, out, partial);
}

extern "C" {

// Host only. out = {LP_TN, LP_TM, LP_KC, LP_BLOCK, and for this call: row tiles,
// column tiles, blocks, bytes of LDS of a block, fp32 words of the partial
// buffer a reduced call needs}. -103: not covered (the first four are still
// written).
int ma_pairwise_lp_layout(ll N, ll M, ll D, ll* out) {
    out[0] = LP_TN;
    out[1] = LP_TM;
    out[2] = LP_KC;
    out[3] = LP_BLOCK;
    LpGeom g;
    if (!lp_geom(N, M, D, &g)) return -103;
    out[4] = g.tiles_n;
    out[5] = g.tiles_m;
    out[6] = g.grid;
    out[7] = 2 * 2 * LP_KC * LP_TN * (ll)sizeof(float);
    out[8] = g.partial_floats;
    return 0;
}

// x: contiguous (N, D), y: contiguous (M, D), both of `dtype` (0 fp32, 1 bf16,
// 2 fp16); x == y is fine. reduction 0: out is (N, M); 1 sum / 2 mean: out is
// (N,) and `partial` holds the layout's fp32 words. out is of `dtype`. On
// `stream`, no host sync. -103: arguments the kernels do not cover; nothing is
// launched.
int ma_pairwise_lp(uintptr_t stream, uintptr_t x, uintptr_t y, int dtype, ll N, ll M, ll D, double p, int zero_diag,
                   int reduction, uintptr_t out, uintptr_t partial) {
    LpGeom g;
    if (!lp_geom(N, M, D, &g)) return -103;
    if (!(p > 0.0) || !isfinite(p) || dtype < LP_F32 || dtype > LP_F16) return -103;
    if (reduction < LP_NONE || reduction > LP_MEAN) return -103;
    const int bytes = dtype == LP_F32 ? 4 : 2;
    if (!x || x % bytes || !y || y % bytes || !out || out % bytes) return -103;
    if ((reduction == LP_NONE && M % 4 == 0 && out % 16) || (reduction != LP_NONE && (!partial || partial % 4))) return -103;
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)partial;
    const int zd = zero_diag != 0;
    if (dtype == LP_F32) lp_by_exponent<float>(s, g, x, y, N, M, D, p, zd, reduction, out, part);
    else if (dtype == LP_BF16) lp_by_exponent<LpBf16>(s, g, x, y, N, M, D, p, zd, reduction, out, part);
    else lp_by_exponent<_Float16>(s, g, x, y, N, M, D, p, zd, reduction, out, part);
    OK(hipGetLastError());
    return 0;
}

}  // extern "C"
