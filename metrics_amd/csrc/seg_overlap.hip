// Segmentation overlap counts (gfx950): the three integers per (sample, class)
// that MeanIoU, DiceScore and GeneralizedDiceScore are made of,
//     intersection[n, c] = sum_s p * t,  pred_sum[n, c] = sum_s p,  target_sum[n, c] = sum_s t,
// in ONE pass over the inputs as they are: no one-hot tensor, no product
// tensor, no host sync. Each side is a label map (N, S) in uint8 / int32 /
// int64 or one-hot planes (N, C, S) in bool / uint8 / int64; S is the product
// of the spatial dimensions. The result is added onto a zeroed (3, N, C) int64
// record. All arithmetic is integer and order-independent: a call gives the
// same bits every time.
//
//  1. k_so_labels  label map x label map. A WORKER owns a run of one sample
//     and never straddles samples; its counters are 3 * C 32-bit words in LDS
//     (so a run stays below 2^31 elements). Two mappings share the kernel body:
//       chunk mapping  a block of SO_BLOCK lanes per SO_CHUNK elements of a
//                      sample;
//       wave mapping   a wave per sample with the counters in the wave's slice
//                      of LDS, SO_WAVES samples per block, no block barrier:
//                      for S <= SO_SMALL_S, where a block would run one
//                      half-empty iteration, two barriers and a flush.
//     A lane takes SO_SLOTS = 16 elements of each side per iteration in 16-byte
//     loads (8 loads of 2 int64, 4 of 4 int32, 1 of 16 uint8; with two dtypes
//     the wider side sets the vector and the narrower side loads as many
//     elements), all issued before the first is counted. A sample starts where
//     n * S puts it, so a run has a scalar head up to the first 16-byte
//     boundary and a scalar tail; where the two sides cannot be aligned
//     together the whole run is scalar. Nothing outside the run is read.
//       Counting is merged per wave, because labels are spatially coherent: 64
//     lanes on one LDS word would serialise. A merge takes the label of the
//     first lane still waiting (a lane read), ballots the lanes that hold it,
//     and that one lane adds the popcount. At most SO_ROUNDS rounds; lanes left
//     after that hold noisy labels and add 1 each with a plain LDS atomic.
//     Three merges per slot: pred labels, target labels, and the lanes where
//     both agree. A label outside [0, C) is counted nowhere.
//       A worker flushes its non-zero counters with 64-bit global atomics onto
//     the sample's row and zeroes them for its next run (the grid is capped at
//     SO_MAX_GRID blocks and strides over the work).
//  2. k_so_planes  a side of planes against planes or against a label map
//     (t = (label == c), the map re-read once per class, mostly from L2). A
//     block per (plane, chunk of SO_CHUNK), three running sums per lane, a wave
//     shuffle fold, one LDS step across the waves and one 64-bit atomic triple
//     per block. Two byte planes take 16-byte loads as four words: bool x bool
//     by popcounts of p & t, p, t; anything with uint8 by the packed 8-bit dot
//     product against the other side and against 0x01010101, which sums values
//     other than 0 / 1 exactly. The 32-bit partial sums live for one iteration
//     (4 dot products, at most 4 * 4 * 255 * 255 < 2^32) and are folded into
//     64 bits at once. Every other pair multiplies and adds in 64 bits.
//
// No matrix instructions: the work is counting and byte dot products of length
// 4 (docs/MFMA.md). Capture into a graph is untested.

#include <hip/hip_runtime.h>

#include <stdint.h>

typedef long long ll;
typedef unsigned long long ull;

#define OK(x)                                      \
    do {                                           \
        hipError_t err_ = (x);                     \
        if (err_ != hipSuccess) return (int)err_;  \
    } while (0)

#define SO_BLOCK 256
#define SO_WAVES (SO_BLOCK / 64)
#define SO_SLOTS 16        // elements of each side a lane takes per iteration
#define SO_CHUNK 8192      // elements of a block's run: two full iterations
#define SO_SMALL_S 4096    // largest S of the wave mapping: four iterations of a wave
#define SO_ROUNDS 4        // merge rounds before the plain-atomic fall-through
// 3 * C counters for each of the SO_WAVES waves of the wave mapping within the
// 64 KiB of LDS a block has without opting in: C <= 1365; the power of two below.
#define SO_MAX_C 1024
#define SO_MAX_GRID 16384  // blocks; the work beyond is strided over

enum { SO_BOOL, SO_U8, SO_I32, SO_I64 };  // dtype codes of the entry
enum { SO_MAP_CHUNK, SO_MAP_WAVE, SO_MAP_PLANES };

#if defined(__HIP_DEVICE_COMPILE__) && defined(__has_builtin)
#if __has_builtin(__builtin_amdgcn_udot4)
#define SO_HAVE_DOT4 1
#endif
#endif

// V elements loaded as one: 16 bytes for the wider side of a pair
template <typename T, int V>
struct alignas(sizeof(T) * V) SoVec {
    T v[V];
};

template <typename A, typename B>
struct SoPair {
    static constexpr int WIDE = sizeof(A) > sizeof(B) ? (int)sizeof(A) : (int)sizeof(B);
    static constexpr int VEC = 16 / WIDE;       // elements per load
    static constexpr int U = SO_SLOTS / VEC;    // loads of each side in flight per lane
};

// The run [c0, c0 + len) of both sides as a scalar head, nvec vectors and a
// scalar rest. The head ends where BOTH sides reach a vector boundary; if they
// never do together, the head is the whole run.
struct SoRun {
    int head, nvec, rest;
};

template <typename TP, typename TT>
__device__ __forceinline__ SoRun so_run(const TP* ps, const TT* ts, int len) {
    constexpr int VEC = SoPair<TP, TT>::VEC;
    const int mp = (int)(((uintptr_t)ps / sizeof(TP)) % VEC), mt = (int)(((uintptr_t)ts / sizeof(TT)) % VEC);
    SoRun r;
    r.head = mp == mt ? min(len, (VEC - mp) % VEC) : len;
    r.nvec = (len - r.head) / VEC;
    r.rest = len - r.head - r.nvec * VEC;
    return r;
}

template <bool WAVE>
__device__ __forceinline__ void so_sync() {
    if (WAVE) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    else __syncthreads();
}

// ------------------------------------------------------------ label x label
template <typename T>
__device__ __forceinline__ int so_label(T raw, int C) {
    const ll v = (ll)raw;
    return (v >= 0 && v < C) ? (int)v : -1;
}

// Every lane with `on` adds 1 to cnt[label], merged per wave. Called by all 64
// lanes of a wave together.
__device__ __forceinline__ void so_merge(unsigned int* cnt, int label, bool on, int lane) {
    ull waiting = __ballot(on);
#pragma unroll 1
    for (int r = 0; r < SO_ROUNDS && waiting; ++r) {
        const int first = __ffsll(waiting) - 1;
        const int l = __builtin_amdgcn_readlane(label, first);
        const ull same = __ballot(on && label == l);
        if (lane == first) atomicAdd(&cnt[l], (unsigned int)__popcll(same));
        on = on && label != l;
        waiting &= ~same;
    }
    if (on) atomicAdd(&cnt[label], 1u);
}

// cnt: [intersection | pred_sum | target_sum], C words each; -1 is "no label"
__device__ __forceinline__ void so_count(unsigned int* cnt, int C, int lp, int lt, int lane) {
    so_merge(cnt + C, lp, lp >= 0, lane);
    so_merge(cnt + 2 * C, lt, lt >= 0, lane);
    so_merge(cnt, lp, lp >= 0 && lp == lt, lane);
}

// p, t: (N, S) label maps. n_work: N * chunks (chunk mapping) or N (wave
// mapping). out: (3, N, C), added onto.
template <typename TP, typename TT, bool WAVE>
__global__ void __launch_bounds__(SO_BLOCK) k_so_labels(const TP* __restrict__ p, const TT* __restrict__ t, ll N, int C,
                                                        ll S, ll chunks, ll n_work, ull* out) {
    extern __shared__ unsigned int so_lds[];
    constexpr int W = WAVE ? 64 : SO_BLOCK;  // lanes of a worker
    constexpr int VEC = SoPair<TP, TT>::VEC, U = SoPair<TP, TT>::U;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wl = WAVE ? lane : (int)threadIdx.x;
    unsigned int* cnt = so_lds + (WAVE ? wave * 3 * C : 0);
    for (int i = wl; i < 3 * C; i += W) cnt[i] = 0;
    so_sync<WAVE>();

    const ll workers = (ll)gridDim.x * (WAVE ? SO_WAVES : 1);
    for (ll w = WAVE ? (ll)blockIdx.x * SO_WAVES + wave : (ll)blockIdx.x; w < n_work; w += workers) {
        const ll n = WAVE ? w : w / chunks;
        const ll c0 = WAVE ? 0 : (w % chunks) * SO_CHUNK;
        const int len = (int)min((ll)(WAVE ? SO_SMALL_S : SO_CHUNK), S - c0);
        const TP* ps = p + n * S + c0;
        const TT* ts = t + n * S + c0;
        const SoRun run = so_run(ps, ts, len);

        const SoVec<TP, VEC>* pv = (const SoVec<TP, VEC>*)(ps + run.head);
        const SoVec<TT, VEC>* tv = (const SoVec<TT, VEC>*)(ts + run.head);
        for (int v0 = 0; v0 < run.nvec; v0 += W * U) {
            SoVec<TP, VEC> a[U];
            SoVec<TT, VEC> b[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int v = v0 + u * W + wl;
                ok[u] = v < run.nvec;
                if (ok[u]) {
                    a[u] = pv[v];
                    b[u] = tv[v];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < VEC; ++j)
                    so_count(cnt, C, ok[u] ? so_label(a[u].v[j], C) : -1, ok[u] ? so_label(b[u].v[j], C) : -1, lane);
        }
        const int loose = run.head + run.rest;  // head, then the rest behind the vectors
        for (int b0 = 0; b0 < loose; b0 += W) {
            const int i = b0 + wl;
            int lp = -1, lt = -1;
            if (i < loose) {
                const int e = i < run.head ? i : i + run.nvec * VEC;
                lp = so_label(ps[e], C);
                lt = so_label(ts[e], C);
            }
            so_count(cnt, C, lp, lt, lane);
        }
        so_sync<WAVE>();
        for (int i = wl; i < 3 * C; i += W) {
            const unsigned int v = cnt[i];
            if (v) {
                atomicAdd(out + ((ll)(i / C) * N + n) * C + i % C, (ull)v);
                cnt[i] = 0;
            }
        }
        so_sync<WAVE>();
    }
}

// ---------------------------------------------------- planes x planes / labels
template <typename T, bool PLANES>
__device__ __forceinline__ ll so_value(T raw, int c) {
    return PLANES ? (ll)raw : (ll)((ll)raw == (ll)c);
}

__device__ __forceinline__ unsigned int so_dot4(unsigned int a, unsigned int b, unsigned int acc) {
#ifdef SO_HAVE_DOT4
    return __builtin_amdgcn_udot4(a, b, acc, false);
#else
    for (int k = 0; k < 32; k += 8) acc += ((a >> k) & 0xffu) * ((b >> k) & 0xffu);
    return acc;
#endif
}

// A side is planes (N, C, S) or a label map (N, S). n_work: N * C * chunks.
// BITS: both sides are bool planes (bytes of 0 / 1). out as above.
template <typename TP, bool PPL, typename TT, bool TPL, bool BITS>
__global__ void __launch_bounds__(SO_BLOCK) k_so_planes(const TP* __restrict__ p, const TT* __restrict__ t, ll N, int C,
                                                        ll S, ll chunks, ll n_work, ull* out) {
    __shared__ ull red[3][SO_WAVES];
    constexpr int VEC = SoPair<TP, TT>::VEC, U = SoPair<TP, TT>::U;
    constexpr bool BYTES = PPL && TPL && sizeof(TP) == 1 && sizeof(TT) == 1;  // VEC 16, U 1
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (ll w = blockIdx.x; w < n_work; w += gridDim.x) {
        const ll plane = w / chunks, c0 = (w % chunks) * SO_CHUNK;
        const ll n = plane / C;
        const int c = (int)(plane % C);
        const int len = (int)min((ll)SO_CHUNK, S - c0);
        const TP* ps = p + (PPL ? plane : n) * S + c0;
        const TT* ts = t + (TPL ? plane : n) * S + c0;
        const SoRun run = so_run(ps, ts, len);
        ull inter = 0, psum = 0, tsum = 0;

        const SoVec<TP, VEC>* pv = (const SoVec<TP, VEC>*)(ps + run.head);
        const SoVec<TT, VEC>* tv = (const SoVec<TT, VEC>*)(ts + run.head);
        for (int v0 = 0; v0 < run.nvec; v0 += SO_BLOCK * U) {
            SoVec<TP, VEC> a[U];
            SoVec<TT, VEC> b[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int v = v0 + u * SO_BLOCK + (int)threadIdx.x;
                ok[u] = v < run.nvec;
                if (ok[u]) {
                    a[u] = pv[v];
                    b[u] = tv[v];
                }
            }
            if (BYTES) {
                if (ok[0]) {
                    unsigned int x[4], y[4], i32 = 0, p32 = 0, t32 = 0;
                    __builtin_memcpy(x, &a[0], 16);
                    __builtin_memcpy(y, &b[0], 16);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (BITS) {
                            i32 += __popc(x[k] & y[k]);
                            p32 += __popc(x[k]);
                            t32 += __popc(y[k]);
                        } else {
                            i32 = so_dot4(x[k], y[k], i32);
                            p32 = so_dot4(x[k], 0x01010101u, p32);
                            t32 = so_dot4(y[k], 0x01010101u, t32);
                        }
                    }
                    inter += i32;
                    psum += p32;
                    tsum += t32;
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (!ok[u]) continue;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        const ll x = so_value<TP, PPL>(a[u].v[j], c), y = so_value<TT, TPL>(b[u].v[j], c);
                        inter += (ull)(x * y);
                        psum += (ull)x;
                        tsum += (ull)y;
                    }
                }
            }
        }
        const int loose = run.head + run.rest;
        for (int i = threadIdx.x; i < loose; i += SO_BLOCK) {
            const int e = i < run.head ? i : i + run.nvec * VEC;
            const ll x = so_value<TP, PPL>(ps[e], c), y = so_value<TT, TPL>(ts[e], c);
            inter += (ull)(x * y);
            psum += (ull)x;
            tsum += (ull)y;
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            inter += __shfl_down(inter, d);
            psum += __shfl_down(psum, d);
            tsum += __shfl_down(tsum, d);
        }
        if (lane == 0) {
            red[0][wave] = inter;
            red[1][wave] = psum;
            red[2][wave] = tsum;
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            ull v = 0;
            for (int k = 0; k < SO_WAVES; ++k) v += red[threadIdx.x][k];
            if (v) atomicAdd(out + ((ll)threadIdx.x * N + n) * C + c, v);
        }
        __syncthreads();
    }
}

// ----------------------------------------------------------------------- host
struct SoGeom {
    int mapping, grid;
    ll chunks, n_work, lds;
};

static bool so_geom(ll N, ll C, ll S, int p_planes, int t_planes, SoGeom* g) {
    if (N < 1 || C < 1 || S < 1 || C > SO_MAX_C) return false;
    if (N > (1LL << 40) || S > (1LL << 46)) return false;  // N * C * chunks stays far inside 64 bits
    g->chunks = (S + SO_CHUNK - 1) / SO_CHUNK;
    ll blocks;
    if (p_planes || t_planes) {
        g->mapping = SO_MAP_PLANES;
        g->n_work = N * C * g->chunks;
        blocks = g->n_work;
        g->lds = 0;
    } else if (S <= SO_SMALL_S) {
        g->mapping = SO_MAP_WAVE;
        g->n_work = N;
        blocks = (N + SO_WAVES - 1) / SO_WAVES;
        g->lds = (ll)SO_WAVES * 3 * C * 4;
    } else {
        g->mapping = SO_MAP_CHUNK;
        g->n_work = N * g->chunks;
        blocks = g->n_work;
        g->lds = 3 * C * 4;
    }
    g->grid = (int)(blocks < SO_MAX_GRID ? blocks : SO_MAX_GRID);
    return true;
}

template <typename TP, typename TT>
static void so_labels_launch(hipStream_t s, const SoGeom& g, uintptr_t p, uintptr_t t, ll N, int C, ll S, ull* out) {
    if (g.mapping == SO_MAP_WAVE)
        k_so_labels<TP, TT, true><<<g.grid, SO_BLOCK, (size_t)g.lds, s>>>((const TP*)p, (const TT*)t, N, C, S, g.chunks,
                                                                          g.n_work, out);
    else
        k_so_labels<TP, TT, false><<<g.grid, SO_BLOCK, (size_t)g.lds, s>>>((const TP*)p, (const TT*)t, N, C, S, g.chunks,
                                                                           g.n_work, out);
}

template <typename TP, bool PPL, typename TT, bool TPL>
static void so_planes_launch(hipStream_t s, const SoGeom& g, bool bits, uintptr_t p, uintptr_t t, ll N, int C, ll S,
                             ull* out) {
    constexpr bool CAN_BITS = PPL && TPL && sizeof(TP) == 1 && sizeof(TT) == 1;
    if (bits)
        k_so_planes<TP, PPL, TT, TPL, CAN_BITS><<<g.grid, SO_BLOCK, 0, s>>>((const TP*)p, (const TT*)t, N, C, S,
                                                                              g.chunks, g.n_work, out);
    else
        k_so_planes<TP, PPL, TT, TPL, false><<<g.grid, SO_BLOCK, 0, s>>>((const TP*)p, (const TT*)t, N, C, S, g.chunks,
                                                                         g.n_work, out);
}

// a side as the kernels see it: 0 / 1 / 2 for 1- / 4- / 8-byte elements; -1 for
// a dtype the form does not take (labels: uint8, int32, int64; planes: bool,
// uint8, int64)
static int so_width(int planes, int dtype) {
    if (planes) return dtype == SO_BOOL || dtype == SO_U8 ? 0 : dtype == SO_I64 ? 2 : -1;
    return dtype == SO_U8 ? 0 : dtype == SO_I32 ? 1 : dtype == SO_I64 ? 2 : -1;
}

// the second side of a pair whose first side is (TP, PPL)
template <typename TP, bool PPL>
static bool so_second(hipStream_t s, const SoGeom& g, bool bits, int t_planes, int wt, uintptr_t p, uintptr_t t, ll N,
                      int C, ll S, ull* out) {
    if (!PPL && !t_planes) {
        if constexpr (!PPL) {
        if (wt == 0) so_labels_launch<TP, uint8_t>(s, g, p, t, N, C, S, out);
        else if (wt == 1) so_labels_launch<TP, int32_t>(s, g, p, t, N, C, S, out);
        else so_labels_launch<TP, int64_t>(s, g, p, t, N, C, S, out);
        }
        return true;
    }
    if (t_planes) {
        if (wt == 0) so_planes_launch<TP, PPL, uint8_t, true>(s, g, bits, p, t, N, C, S, out);
        else if (wt == 2) so_planes_launch<TP, PPL, int64_t, true>(s, g, bits, p, t, N, C, S, out);
        else return false;
        return true;
    }
    if constexpr (PPL) {  // planes against a label map
        if (wt == 0) so_planes_launch<TP, PPL, uint8_t, false>(s, g, false, p, t, N, C, S, out);
        else if (wt == 1) so_planes_launch<TP, PPL, int32_t, false>(s, g, false, p, t, N, C, S, out);
        else so_planes_launch<TP, PPL, int64_t, false>(s, g, false, p, t, N, C, S, out);
        return true;
    }
    return false;
}

extern "C" {

// Host only. out = {largest C, elements of a chunk, largest S of the wave
// mapping, merge rounds, samples of a block in the wave mapping, blocks the grid
// is capped at, and for this call: mapping (0 chunk, 1 wave, 2 planes), blocks,
// bytes of dynamic LDS}. -103: not covered (the first six are still written).
int ma_seg_overlap_layout(ll N, ll C, ll S, int p_planes, int t_planes, ll* out) {
    out[0] = SO_MAX_C;
    out[1] = SO_CHUNK;
    out[2] = SO_SMALL_S;
    out[3] = SO_ROUNDS;
    out[4] = SO_WAVES;
    out[5] = SO_MAX_GRID;
    SoGeom g;
    if (!so_geom(N, C, S, p_planes, t_planes, &g)) return -103;
    out[6] = g.mapping;
    out[7] = g.grid;
    out[8] = g.lds;
    return 0;
}

// preds / target: contiguous (N, S) label maps (planes 0) or (N, C, S) planes
// (planes 1); dtype 0 bool, 1 uint8, 2 int32, 3 int64. out: the zeroed
// (3, N, C) int64 record [intersection | pred_sum | target_sum]. On `stream`,
// no host sync. -103: arguments the kernels do not cover; nothing is launched.
int ma_seg_overlap(uintptr_t stream, uintptr_t preds, int p_planes, int p_dtype, uintptr_t target, int t_planes,
                   int t_dtype, ll N, ll C, ll S, uintptr_t out) {
    static const int bytes[3] = {1, 4, 8};
    SoGeom g;
    if ((p_planes != 0 && p_planes != 1) || (t_planes != 0 && t_planes != 1)) return -103;
    if (!so_geom(N, C, S, p_planes, t_planes, &g)) return -103;
    const int wp = so_width(p_planes, p_dtype), wt = so_width(t_planes, t_dtype);
    if (wp < 0 || wt < 0 || !preds || preds % bytes[wp] || !target || target % bytes[wt] || !out || out % 8) return -103;
    hipStream_t s = (hipStream_t)stream;
    const bool bits = p_planes && t_planes && p_dtype == SO_BOOL && t_dtype == SO_BOOL;
    ull* o = (ull*)out;
    bool done;
    if (p_planes) {
        if (wp == 0) done = so_second<uint8_t, true>(s, g, bits, t_planes, wt, preds, target, N, (int)C, S, o);
        else done = so_second<int64_t, true>(s, g, bits, t_planes, wt, preds, target, N, (int)C, S, o);
    } else {
        if (wp == 0) done = so_second<uint8_t, false>(s, g, bits, t_planes, wt, preds, target, N, (int)C, S, o);
        else if (wp == 1) done = so_second<int32_t, false>(s, g, bits, t_planes, wt, preds, target, N, (int)C, S, o);
        else done = so_second<int64_t, false>(s, g, bits, t_planes, wt, preds, target, N, (int)C, S, o);
    }
    if (!done) return -103;
    OK(hipGetLastError());
    return 0;
}

}  // extern "C"
