// K8 — fused windowed-image kernels for gfx950 (CDNA4).
//
// k_ssim2d_fused: the whole 2D SSIM map in ONE kernel. The torch/MIOpen
// formulation (reference functional/image/ssim.py:128-186) runs
// pad -> cat(5B) -> grouped conv -> ~8 elementwise kernels, round-tripping
// >10 full tensors through HBM. Here each workgroup loads one (TS x TS)
// output tile's input patch (reflect indexing, no materialized pad) into
// LDS, separably row-filters the five products [p, t, p2, t2, pt] in LDS,
// column-filters + evaluates the SSIM formula in registers, and reduces
// per-image sums straight into fp64 accumulators: HBM traffic = read the
// two inputs once, write B doubles.
//
// k_binary_erosion2d: windowed erosion with an arbitrary small structuring
// element (replaces the unfold path in functional/segmentation/utils.py:55
// which materializes (N,C,H,W,k^2) windows).

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <cstdint>

using ll = long long;

#define TS 32           // output tile edge
#define NTHREADS 256

__device__ __forceinline__ int reflect_idx(int i, int n) {
    // torch F.pad mode="reflect": -1 -> 1, n -> n-2 (requires pad < n)
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    // A tile that reaches past a small image (n < TS) asks for patch cells more
    // than the pad beyond the edge: 2n - 2 - i is negative there (n = 12,
    // radius 5: down to -14). No output inside the image reads such a cell, but
    // the load must stay inside the plane.
    return min(max(i, 0), n - 1);
}

template <typename T>
__global__ void __launch_bounds__(NTHREADS) k_ssim2d_fused(
    const T* __restrict__ preds, const T* __restrict__ target,
    int B, int C, int H, int W,
    const float* __restrict__ wh, int rh,   // column (vertical) weights, radius
    const float* __restrict__ ww, int rw,   // row (horizontal) weights, radius
    float c1_in, float c2_in, const float* __restrict__ dr_ptr, float k1, float k2,
    int want_cs, int crop_h, int crop_w,
    double* __restrict__ sum_sim,   // (B,)
    double* __restrict__ sum_cs) {  // (B,) or null
    extern __shared__ float lds[];
    const int patch_w = TS + 2 * rw;
    const int patch_h = TS + 2 * rh;
    float* sp = lds;                         // patch preds  (patch_h x patch_w)
    float* st = sp + patch_h * patch_w;      // patch target
    float* filt = st + patch_h * patch_w;    // 5 x (patch_h x TS) row-filtered

    const int plane = blockIdx.z;            // b * C + c
    const int b = plane / C;
    const ll plane_off = (ll)plane * H * W;
    const int x0 = blockIdx.x * TS;          // tile origin in the output map
    const int y0 = blockIdx.y * TS;

    float c1 = c1_in, c2 = c2_in;
    if (dr_ptr) {
        const float dr = *dr_ptr;
        c1 = (k1 * dr) * (k1 * dr);
        c2 = (k2 * dr) * (k2 * dr);
    }

    // ---- load the input patch with reflect indexing
    for (int i = threadIdx.x; i < patch_h * patch_w; i += NTHREADS) {
        const int py = i / patch_w;
        const int px = i - py * patch_w;
        const int gy = reflect_idx(y0 + py - rh, H);
        const int gx = reflect_idx(x0 + px - rw, W);
        const ll g = plane_off + (ll)gy * W + gx;
        sp[i] = (float)preds[g];
        st[i] = (float)target[g];
    }
    __syncthreads();

    // ---- phase 1: horizontal filter of the 5 products into filt
    const int row_elems = patch_h * TS;
    for (int i = threadIdx.x; i < row_elems; i += NTHREADS) {
        const int py = i / TS;
        const int cx = i - py * TS;          // output-tile column
        float ap = 0.f, at = 0.f, app = 0.f, att = 0.f, apt = 0.f;
        const float* rowp = sp + py * patch_w + cx;
        const float* rowt = st + py * patch_w + cx;
        for (int dx = 0; dx <= 2 * rw; ++dx) {
            const float w = ww[dx];
            const float vp = rowp[dx];
            const float vt = rowt[dx];
            ap += w * vp;
            at += w * vt;
            app += w * vp * vp;
            att += w * vt * vt;
            apt += w * vp * vt;
        }
        filt[0 * row_elems + i] = ap;
        filt[1 * row_elems + i] = at;
        filt[2 * row_elems + i] = app;
        filt[3 * row_elems + i] = att;
        filt[4 * row_elems + i] = apt;
    }
    __syncthreads();

    // ---- phase 2: vertical filter + SSIM formula + tile reduction
    double acc_sim = 0.0, acc_cs = 0.0;
    for (int i = threadIdx.x; i < TS * TS; i += NTHREADS) {
        const int ty = i / TS;
        const int tx = i - ty * TS;
        const int gy = y0 + ty;
        const int gx = x0 + tx;
        if (gy >= H || gx >= W) continue;
        float mu_p = 0.f, mu_t = 0.f, m_pp = 0.f, m_tt = 0.f, m_pt = 0.f;
        for (int dy = 0; dy <= 2 * rh; ++dy) {
            const float w = wh[dy];
            const int r = (ty + dy) * TS + tx;
            mu_p += w * filt[0 * row_elems + r];
            mu_t += w * filt[1 * row_elems + r];
            m_pp += w * filt[2 * row_elems + r];
            m_tt += w * filt[3 * row_elems + r];
            m_pt += w * filt[4 * row_elems + r];
        }
        // rounded products, never contracted into the subtractions: an fma would
        // subtract the exact mu^2 from the rounded moment and leave that moment's
        // rounding error as variance (a 1-pixel window has variance 0, and gets
        // exactly 0 only this way). __fmul_rn is a plain product here and would
        // be contracted all the same, so contraction is off for this block.
        float mu_p2, mu_t2, mu_pt, s_p, s_t, s_pt;
        {
#pragma clang fp contract(off)
            mu_p2 = mu_p * mu_p;
            mu_t2 = mu_t * mu_t;
            mu_pt = mu_p * mu_t;
            s_p = fmaxf(m_pp - mu_p2, 0.f);
            s_t = fmaxf(m_tt - mu_t2, 0.f);
            s_pt = m_pt - mu_pt;
        }
        const float upper = 2.f * s_pt + c2;
        const float lower = s_p + s_t + c2;
        const float ssim = ((2.f * mu_pt + c1) * upper) / ((mu_p2 + mu_t2 + c1) * lower);
        acc_sim += (double)ssim;
        if (want_cs && gy >= crop_h && gy < H - crop_h && gx >= crop_w && gx < W - crop_w)
            acc_cs += (double)(upper / lower);
    }

    // wave-level then LDS reduction of the two accumulators
    __shared__ double red[NTHREADS / 64 * 2];
    for (int off = 32; off > 0; off >>= 1) {
        acc_sim += __shfl_down(acc_sim, off);
        acc_cs += __shfl_down(acc_cs, off);
    }
    const int wave = threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0) {
        red[wave * 2] = acc_sim;
        red[wave * 2 + 1] = acc_cs;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0, cs = 0.0;
        for (int wv = 0; wv < NTHREADS / 64; ++wv) {
            s += red[wv * 2];
            cs += red[wv * 2 + 1];
        }
        atomicAdd(&sum_sim[b], s);
        if (want_cs) atomicAdd(&sum_cs[b], cs);
    }
}

extern "C" int ma_ssim2d_fused(
    uint64_t stream_u, uint64_t preds_u, uint64_t target_u, int dtype_code,
    ll B, ll C, ll H, ll W,
    uint64_t wh_u, int rh, uint64_t ww_u, int rw,
    float c1, float c2, uint64_t dr_ptr_u, float k1, float k2,
    int want_cs, int crop_h, int crop_w,
    uint64_t sum_sim_u, uint64_t sum_cs_u) {
    hipStream_t stream = (hipStream_t)stream_u;
    // grid.y and grid.z hold at most 65535 blocks: more planes (or tile rows)
    // than that take the torch path, like a window past the LDS tile
    if (B * C > 65535 || (H + TS - 1) / TS > 65535) return 9001;
    dim3 grid((W + TS - 1) / TS, (H + TS - 1) / TS, B * C);
    const int patch_w = TS + 2 * rw;
    const int patch_h = TS + 2 * rh;
    const size_t lds = (size_t)(2 * patch_h * patch_w + 5 * patch_h * TS) * sizeof(float);
    if (lds > 64 * 1024) return 9001;  // caller falls back to the torch path
    if (dtype_code == 0)
        hipLaunchKernelGGL(k_ssim2d_fused<float>, grid, dim3(NTHREADS), lds, stream,
                           (const float*)preds_u, (const float*)target_u, (int)B, (int)C, (int)H,
                           (int)W, (const float*)wh_u, rh, (const float*)ww_u, rw, c1, c2,
                           (const float*)dr_ptr_u, k1, k2, want_cs, crop_h, crop_w,
                           (double*)sum_sim_u, (double*)sum_cs_u);
    else
        hipLaunchKernelGGL(k_ssim2d_fused<__hip_bfloat16>, grid, dim3(NTHREADS), lds, stream,
                           (const __hip_bfloat16*)preds_u, (const __hip_bfloat16*)target_u, (int)B,
                           (int)C, (int)H, (int)W, (const float*)wh_u, rh, (const float*)ww_u, rw,
                           c1, c2, (const float*)dr_ptr_u, k1, k2, want_cs, crop_h, crop_w,
                           (double*)sum_sim_u, (double*)sum_cs_u);
    return (int)hipGetLastError();
}

// --------------------------------------------------------------- erosion

__global__ void __launch_bounds__(256) k_binary_erosion2d(
    const unsigned char* __restrict__ img, int N, int C, int H, int W,
    const int* __restrict__ strel, int kh, int kw, int oy, int ox,
    int border_value, unsigned char* __restrict__ out) {
    const ll total = (ll)N * C * H * W;
    ll i = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % W);
    const int y = (int)((i / W) % H);
    const ll plane = i / ((ll)H * W);
    const unsigned char* p = img + plane * H * W;
    // replicate the reference formula min(window - strel) + 1 exactly,
    // including its all-zero-structure corner (result can be 2)
    int mn = 2;
    for (int dy = 0; dy < kh; ++dy) {
        const int yy = y + dy - oy;
        for (int dx = 0; dx < kw; ++dx) {
            const int xx = x + dx - ox;
            const int inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W);
            const int v = inside ? (int)p[(ll)yy * W + xx] : border_value;
            const int d = v - strel[dy * kw + dx];
            if (d < mn) mn = d;
        }
    }
    out[i] = (unsigned char)(mn + 1);
}

extern "C" int ma_binary_erosion2d(
    uint64_t stream_u, uint64_t img_u, ll N, ll C, ll H, ll W,
    uint64_t strel_u, int kh, int kw, int oy, int ox, int border_value, uint64_t out_u) {
    hipStream_t stream = (hipStream_t)stream_u;
    const ll total = N * C * H * W;
    const ll grid = (total + 255) / 256;
    hipLaunchKernelGGL(k_binary_erosion2d, dim3(grid), dim3(256), 0, stream,
                       (const unsigned char*)img_u, (int)N, (int)C, (int)H, (int)W,
                       (const int*)strel_u, kh, kw, oy, ox, border_value,
                       (unsigned char*)out_u);
    return (int)hipGetLastError();
}
