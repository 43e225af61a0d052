// Single-input squeeze-and-excitation scaling (model_utils.py:36-51: x * sigmoid(fc(gap(x)))) — the fusion point of the
// one-modality networks (model_one_modality.py:165-187), which have no second tensor to blend.  The axpby_* kernels of
// pointwise.hip always read two maps; these read one:
//   forward      out = g[n,c] * x                               1 read + 1 write of the map
//   backward     dg[n,c] = sum_hw gout * x                      2 reads            (one workgroup per plane, fixed order)
//                dx = g * gout + ds[n,c] * cscale               1 read + 1 write   (ds: the squeeze's gradient, cscale = 1/HW)
// and, at the stem, the same three passes fused with the 3x3 / stride 2 max-pool that follows: the full-resolution scaled
// map is never written (forward) nor its gradient (backward).  The squeeze is gap2_kernel<V, false, false> and the
// excitation dynmm_se1_coeff_* (gate_se.hip, next to the MLP helpers it shares with the two-input fusion).
// Element-wise passes: grid (plane, chunk of kChunk elements), 16-byte accesses when HW % 4 == 0 and the pointers allow;
// every lane requests its U accesses of a chunk before it consumes the first (gap2_kernel's shape).
#include "common.h"
#include "vec.h"
#include "pool.h"

namespace dynmm {

constexpr int kU = 4;      // accesses in flight per lane

template <int V>
__global__ void __launch_bounds__(256) se1_scale_fwd_kernel(const float* x, const float* __restrict__ g, float* out,
                                                            int HW) {
    // (x / out carry no __restrict__: inference scales in place, out == x; a lane writes only what it has read)
    const size_t base = (size_t)blockIdx.x * HW;
    const float fg = g[blockIdx.x];
    const int end = min(HW, (int)(blockIdx.y + 1) * kChunk);
    int i = blockIdx.y * kChunk + threadIdx.x * V;
    for (; i + (kU - 1) * 256 * V < end; i += kU * 256 * V) {
        float v[kU][V];
#pragma unroll
        for (int u = 0; u < kU; ++u) vload<V>(x + base + i + u * 256 * V, v[u]);
#pragma unroll
        for (int u = 0; u < kU; ++u) {
#pragma unroll
            for (int j = 0; j < V; ++j) v[u][j] = fg * v[u][j];            // explicit: se1_scale_pool_fwd_kernel repeats it
            vstore<V>(out + base + i + u * 256 * V, v[u]);
        }
    }
    for (; i < end; i += 256 * V) {
        float v[V];
        vload<V>(x + base + i, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = fg * v[j];
        vstore<V>(out + base + i, v);
    }
}

template <int V>
__global__ void __launch_bounds__(256) se1_scale_bwd_reduce_kernel(const float* __restrict__ gout,
                                                                   const float* __restrict__ x, float* __restrict__ dg,
                                                                   int HW) {
    __shared__ float red[4];
    const size_t base = (size_t)blockIdx.x * HW;
    float acc = 0.f;
    int i = threadIdx.x * V;
    for (; i + (kU - 1) * 256 * V < HW; i += kU * 256 * V) {
        float gv[kU][V], xv[kU][V];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            vload<V>(gout + base + i + u * 256 * V, gv[u]);
            vload<V>(x + base + i + u * 256 * V, xv[u]);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
#pragma unroll
            for (int j = 0; j < V; ++j) acc += gv[u][j] * xv[u][j];
    }
    for (; i < HW; i += 256 * V) {
        float gv[V], xv[V];
        vload<V>(gout + base + i, gv);
        vload<V>(x + base + i, xv);
#pragma unroll
        for (int j = 0; j < V; ++j) acc += gv[j] * xv[j];
    }
    const float t = block_reduce_sum_256<float>(acc, red);     // wave shuffle, then LDS: a fixed order
    if (threadIdx.x == 0) dg[blockIdx.x] = t;
}

template <int V>
__global__ void __launch_bounds__(256) se1_scale_bwd_apply_kernel(const float* gout, const float* __restrict__ g,
                                                                  const float* __restrict__ ds, float cscale, float* dx,
                                                                  int HW) {
    // (gout / dx without __restrict__, like the forward: with it the compiler pairs element k of one 16-byte access with element
    //  k of the next in packed FMAs and stores the results as 40 single dwords per trip — 77.1 us at 32 x 64 x 120 x 160 against
    //  49.7 for the forward's identical traffic; without it the pairs are neighbours and the stores stay 16 bytes wide: 53.9 us,
    //  profiles/one_modality.md)
    const size_t base = (size_t)blockIdx.x * HW;
    const float fg = g[blockIdx.x];
    const float off = ds ? ds[blockIdx.x] * cscale : 0.f;
    const int end = min(HW, (int)(blockIdx.y + 1) * kChunk);
    int i = blockIdx.y * kChunk + threadIdx.x * V;
    for (; i + (kU - 1) * 256 * V < end; i += kU * 256 * V) {
        float v[kU][V];
#pragma unroll
        for (int u = 0; u < kU; ++u) vload<V>(gout + base + i + u * 256 * V, v[u]);
#pragma unroll
        for (int u = 0; u < kU; ++u) {
#pragma unroll
            for (int j = 0; j < V; ++j) v[u][j] = fmaf(fg, v[u][j], off);
            vstore<V>(dx + base + i + u * 256 * V, v[u]);
        }
    }
    for (; i < end; i += 256 * V) {
        float v[V];
        vload<V>(gout + base + i, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = fmaf(fg, v[j], off);
        vstore<V>(dx + base + i, v);
    }
}

// ------------------------------------------------------------------------------------------------
// Stem: y = max_pool_3x3_s2(g * x).  Even H, W % 8 == 0 (pool_fusable).  maxpool_fwd4_kernel's thread shape — 4 pooled pixels of
// one row = input columns 8t-1 .. 8t+7 — with the product formed in registers by se1_scale_fwd_kernel's expression, so values
// and arg-max codes are those of the two kernels run one after the other, tap by tap in row-major window order.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) se1_scale_pool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                 float* __restrict__ y, signed char* __restrict__ idx,
                                                                 int H, int W, int Ho, int Wo) {
    const size_t plane = blockIdx.x;
    const float* xp = x + plane * (size_t)H * W;
    const float fg = g[plane];
    const int Wq = Wo / 4, nq = Ho * Wq;
    const int beg = blockIdx.y * (kChunk / 4), end = min(nq, beg + kChunk / 4);
    for (int q = beg + threadIdx.x; q < end; q += 256) {
        const int oh = q / Wq, t = q - oh * Wq;
        // the three input rows of the window are requested before the first is compared (row -1 of the first pooled row: the
        // clamped address is loaded and its taps skipped below)
        float4 a[3], b[3];
        float left[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int ih = max(2 * oh - 1 + r, 0);                 // < H always (H even)
            const float* row = xp + (size_t)ih * W + 8 * t;
            a[r] = *reinterpret_cast<const float4*>(row);
            b[r] = *reinterpret_cast<const float4*>(row + 4);
            left[r] = t > 0 ? row[-1] : 0.f;
        }
        float best[4];
        int bi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { best[j] = -INFINITY; bi[j] = -1; }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            if (2 * oh - 1 + r < 0) continue;
            float v[9] = {left[r], a[r].x, a[r].y, a[r].z, a[r].w, b[r].x, b[r].y, b[r].z, b[r].w};
#pragma unroll
            for (int k = 0; k < 9; ++k) v[k] = fg * v[k];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int sx = 0; sx < 3; ++sx) {
                    if (j == 0 && sx == 0 && t == 0) continue;          // input column -1
                    pool_update(best[j], bi[j], v[2 * j + sx], r * 3 + sx);
                }
        }
        const size_t o = plane * (size_t)Ho * Wo + (size_t)oh * Wo + 4 * t;
        *reinterpret_cast<float4*>(y + o) = make_float4(best[0], best[1], best[2], best[3]);
        *reinterpret_cast<unsigned*>(idx + o) = (unsigned)(bi[0] & 0xff) | ((unsigned)(bi[1] & 0xff) << 8) |
                                                ((unsigned)(bi[2] & 0xff) << 16) | ((unsigned)(bi[3] & 0xff) << 24);
    }
}

// dg[plane] = sum_p gy[p] * x[argmax(p)], gathered block by block: the gradient of the (never written) scaled map at the
// 2 x 8 input pixels of a thread comes from pool_bwd_block, is multiplied with x there and summed in a fixed order.
__global__ void __launch_bounds__(256) se1_scale_pool_bwd_reduce_kernel(const float* __restrict__ gy,
                                                                        const signed char* __restrict__ idx,
                                                                        const float* __restrict__ x,
                                                                        float* __restrict__ dg, int H, int W, int Ho,
                                                                        int Wo) {
    __shared__ float red[4];
    const size_t plane = blockIdx.x;
    const float* gp = gy + plane * (size_t)Ho * Wo;
    const signed char* ip = idx + plane * (size_t)Ho * Wo;
    const float* xp = x + plane * (size_t)H * W;
    const int Wq = Wo / 4, nq = Ho * Wq;
    float acc = 0.f;
    for (int q = threadIdx.x; q < nq; q += 256) {
        const int a = q / Wq, t = q - a * Wq;
        const size_t o = (size_t)(2 * a) * W + 8 * t;
        const float4 x00 = *reinterpret_cast<const float4*>(xp + o), x01 = *reinterpret_cast<const float4*>(xp + o + 4);
        const float4 x10 = *reinterpret_cast<const float4*>(xp + o + W), x11 = *reinterpret_cast<const float4*>(xp + o + W + 4);
        float top[8], bot[8];
        pool_bwd_block(gp, ip, a, t, Ho, Wo, top, bot);
        acc += top[0] * x00.x + top[1] * x00.y + top[2] * x00.z + top[3] * x00.w;
        acc += top[4] * x01.x + top[5] * x01.y + top[6] * x01.z + top[7] * x01.w;
        acc += bot[0] * x10.x + bot[1] * x10.y + bot[2] * x10.z + bot[3] * x10.w;
        acc += bot[4] * x11.x + bot[5] * x11.y + bot[6] * x11.z + bot[7] * x11.w;
    }
    const float tsum = block_reduce_sum_256<float>(acc, red);
    if (threadIdx.x == 0) dg[plane] = tsum;
}

// dx = g * max_pool_backward(gy, idx) + ds * cscale   (gather form: every input pixel is written once, no atomics)
__global__ void __launch_bounds__(256) se1_scale_pool_bwd_apply_kernel(const float* __restrict__ gy,
                                                                       const signed char* __restrict__ idx,
                                                                       const float* __restrict__ g,
                                                                       const float* __restrict__ ds, float cscale,
                                                                       float* __restrict__ dx, int H, int W, int Ho,
                                                                       int Wo) {
    const size_t plane = blockIdx.x;
    const size_t po = plane * (size_t)Ho * Wo;
    const float fg = g[plane];
    const float off = ds ? ds[plane] * cscale : 0.f;
    float* dp = dx + plane * (size_t)H * W;
    const int Wq = Wo / 4, nq = Ho * Wq;
    const int beg = blockIdx.y * (kChunk / 4), end = min(nq, beg + kChunk / 4);
    for (int q = beg + threadIdx.x; q < end; q += 256) {
        const int a = q / Wq, t = q - a * Wq;
        float top[8], bot[8];
        pool_bwd_block(gy + po, idx + po, a, t, Ho, Wo, top, bot);
        float* r0 = dp + (size_t)(2 * a) * W + 8 * t;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<float4*>(r0 + 4 * h) = make_float4(fmaf(fg, top[4 * h], off), fmaf(fg, top[4 * h + 1], off),
                                                                 fmaf(fg, top[4 * h + 2], off), fmaf(fg, top[4 * h + 3], off));
            *reinterpret_cast<float4*>(r0 + W + 4 * h) = make_float4(fmaf(fg, bot[4 * h], off), fmaf(fg, bot[4 * h + 1], off),
                                                                     fmaf(fg, bot[4 * h + 2], off), fmaf(fg, bot[4 * h + 3], off));
        }
    }
}

}  // namespace dynmm

using namespace dynmm;
#define ST ((hipStream_t)stream)

extern "C" int dynmm_se1_scale_fwd(const float* x, const float* g, float* out, int NC, int HW, void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other users of the runtime
    if (!x || !g || !out || NC <= 0 || HW <= 0) return DYNMM_EINVAL;
    dim3 grid(NC, plane_chunks(HW, kChunk));
    if (can_vec4(HW, {x, out}))
        hipLaunchKernelGGL(se1_scale_fwd_kernel<4>, grid, dim3(256), 0, ST, x, g, out, HW);
    else
        hipLaunchKernelGGL(se1_scale_fwd_kernel<1>, grid, dim3(256), 0, ST, x, g, out, HW);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_se1_scale_bwd_reduce(const float* gout, const float* x, float* dg, int NC, int HW, void* stream) {
    (void)hipGetLastError();
    if (!gout || !x || !dg || NC <= 0 || HW <= 0) return DYNMM_EINVAL;
    if (can_vec4(HW, {gout, x}))
        hipLaunchKernelGGL(se1_scale_bwd_reduce_kernel<4>, dim3(NC), dim3(256), 0, ST, gout, x, dg, HW);
    else
        hipLaunchKernelGGL(se1_scale_bwd_reduce_kernel<1>, dim3(NC), dim3(256), 0, ST, gout, x, dg, HW);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_se1_scale_bwd_apply(const float* gout, const float* g, const float* ds, float cscale, float* dx,
                                         int NC, int HW, void* stream) {
    (void)hipGetLastError();
    if (!gout || !g || !dx || NC <= 0 || HW <= 0) return DYNMM_EINVAL;
    dim3 grid(NC, plane_chunks(HW, kChunk));
    if (can_vec4(HW, {gout, dx}))
        hipLaunchKernelGGL(se1_scale_bwd_apply_kernel<4>, grid, dim3(256), 0, ST, gout, g, ds, cscale, dx, HW);
    else
        hipLaunchKernelGGL(se1_scale_bwd_apply_kernel<1>, grid, dim3(256), 0, ST, gout, g, ds, cscale, dx, HW);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_se1_scale_pool_supported(int H, int W) { return (H > 0 && W > 0 && H % 2 == 0 && W % 8 == 0) ? 1 : 0; }

extern "C" int dynmm_se1_scale_pool_fwd(const float* x, const float* g, float* y, signed char* idx, int NC, int H, int W,
                                        void* stream) {
    (void)hipGetLastError();
    if (!x || !g || !y || !idx || NC <= 0 || H <= 0 || W <= 0) return DYNMM_EINVAL;
    const int Ho = H / 2, Wo = W / 2;
    if (!pool_fusable(H, W, Ho, Wo, {x, y}, {idx})) return DYNMM_EUNSUPPORTED;
    hipLaunchKernelGGL(se1_scale_pool_fwd_kernel, dim3(NC, plane_chunks(Ho * Wo, kChunk)), dim3(256), 0, ST, x, g, y, idx,
                       H, W, Ho, Wo);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_se1_scale_pool_bwd_reduce(const float* gy, const signed char* idx, const float* x, float* dg, int NC,
                                               int H, int W, void* stream) {
    (void)hipGetLastError();
    if (!gy || !idx || !x || !dg || NC <= 0 || H <= 0 || W <= 0) return DYNMM_EINVAL;
    const int Ho = H / 2, Wo = W / 2;
    if (!pool_fusable(H, W, Ho, Wo, {gy, x}, {idx})) return DYNMM_EUNSUPPORTED;
    hipLaunchKernelGGL(se1_scale_pool_bwd_reduce_kernel, dim3(NC), dim3(256), 0, ST, gy, idx, x, dg, H, W, Ho, Wo);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_se1_scale_pool_bwd_apply(const float* gy, const signed char* idx, const float* g, const float* ds,
                                              float cscale, float* dx, int NC, int H, int W, void* stream) {
    (void)hipGetLastError();
    if (!gy || !idx || !g || !dx || NC <= 0 || H <= 0 || W <= 0) return DYNMM_EINVAL;
    const int Ho = H / 2, Wo = W / 2;
    if (!pool_fusable(H, W, Ho, Wo, {gy, dx}, {idx})) return DYNMM_EUNSUPPORTED;
    hipLaunchKernelGGL(se1_scale_pool_bwd_apply_kernel, dim3(NC, plane_chunks(Ho * Wo, kChunk)), dim3(256), 0, ST, gy, idx,
                       g, ds, cscale, dx, H, W, Ho, Wo);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}
