// Shared device/host helpers for the gfx950 kernels of libdynmm_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "dynmm_hip.h"

// These kernels are written for one target: 160 KB of LDS per workgroup (mha_bwd_kernel<32,false> alone declares 66 KB),
// global_load_lds_dwordx4, the gfx950 MFMA set.  Fail at compile time, not at the first launch, on anything else.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libdynmm_hip is gfx950 (MI355X) code: build with --offload-arch=gfx950"
#endif

#define DYNMM_LAUNCH_CHECK()                                   \
    do {                                                       \
        hipError_t e__ = hipGetLastError();                    \
        if (e__ != hipSuccess) return -(1000 + (int)e__);      \
    } while (0)

#define DYNMM_HIP_TRY(expr)                                    \
    do {                                                       \
        hipError_t e__ = (expr);                               \
        if (e__ != hipSuccess) return -(1000 + (int)e__);      \
    } while (0)

namespace dynmm {

constexpr int kWave = 64;      // CDNA wavefront
constexpr int kNumXCD = 8;     // MI355X: 8 XCDs, each with a private L2

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline size_t ceil_div_sz(size_t a, size_t b) { return (a + b - 1) / b; }

// Workgroups are dispatched round-robin over the 8 XCDs (block b -> XCD b % 8).  Remap so that
// consecutive *logical* tile ids land on the same XCD and share its L2 (bijective for any nblk).
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int xcd = bid % kNumXCD;
    const int local = bid / kNumXCD;
    const int q = nblk / kNumXCD, r = nblk % kNumXCD;
    const int start = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return start + local;
}

template <typename T>
__device__ __forceinline__ T wave_reduce_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// Sum over a 256-thread block; result valid in thread 0.  `smem` must hold >= 4 T's.
template <typename T>
__device__ __forceinline__ T block_reduce_sum_256(T v, T* smem) {
    v = wave_reduce_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) smem[wave] = v;
    __syncthreads();
    T r = T(0);
    if (threadIdx.x == 0) r = smem[0] + smem[1] + smem[2] + smem[3];
    return r;
}

__device__ __forceinline__ float row16_sum(float v) {            // sum over the lane's row of 16 lanes, in every lane of it
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));      // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));      // quad_perm [2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, true));     // row_half_mirror
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, true));     // row_mirror
    return v;
}

// r[0 .. N-1] = p[0 .. N-1] in the widest units N allows (the attention kernels' LDS rows: one address for every lane, a
// broadcast); p: aligned to the widest unit used
template <int N>
__device__ __forceinline__ void row_ld(const float* __restrict__ p, float r[N]) {
    if constexpr (N % 4 == 0) {
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            const float4 t = reinterpret_cast<const float4*>(p)[q];
            r[4 * q] = t.x; r[4 * q + 1] = t.y; r[4 * q + 2] = t.z; r[4 * q + 3] = t.w;
        }
    } else if constexpr (N % 2 == 0) {
#pragma unroll
        for (int q = 0; q < N / 2; ++q) {
            const float2 t = reinterpret_cast<const float2*>(p)[q];
            r[2 * q] = t.x; r[2 * q + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int q = 0; q < N; ++q) r[q] = p[q];
    }
}

// Swish z * sigmoid(z) and Hswish z * relu6(z + 3) / 6 (model_utils.py:100-115), in the reference's order of operations.
// (z -> -inf: expf(-z) = +inf, the quotient is -0: finite, no NaN.)
__device__ __forceinline__ float sigmoid_f(float v) { return 1.f / (1.f + expf(-v)); }
__device__ __forceinline__ float swish_fwd(float v) { return v / (1.f + expf(-v)); }
__device__ __forceinline__ float hswish_fwd(float v) { return v * fminf(fmaxf(v + 3.f, 0.f), 6.f) / 6.f; }

__device__ __forceinline__ float act_fwd(float v, int act) {
    if (act == DYNMM_ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == DYNMM_ACT_TANH) return tanhf(v);
    if (act == DYNMM_ACT_SWISH) return swish_fwd(v);
    if (act == DYNMM_ACT_HSWISH) return hswish_fwd(v);
    return v;
}

// derivative of the activation at the PRE-activation z: the only form Swish and Hswish have (neither is invertible — minima
// near -1.28 and at -1.5).  Hswish follows torch's autograd at the kinks: hardtanh's gradient mask is strict, so the middle
// segment is -3 < z < 3 — at exactly z = 3 the derivative is 1, at exactly z = -3 it is 0.
__device__ __forceinline__ float act_grad_pre(float z, int act) {
    if (act == DYNMM_ACT_RELU) return z > 0.f ? 1.f : 0.f;
    if (act == DYNMM_ACT_TANH) { const float t = tanhf(z); return 1.f - t * t; }
    if (act == DYNMM_ACT_SWISH) {
        const float s = 1.f / (1.f + expf(-z));
        return s * (1.f + z * (1.f - s));
    }
    if (act == DYNMM_ACT_HSWISH) return z <= -3.f ? 0.f : (z < 3.f ? (2.f * z + 3.f) / 6.f : 1.f);
    return 1.f;
}

// derivative of the activation expressed through its OUTPUT y (ReLU: y>0, tanh: 1-y^2), so the
// backward never needs the pre-activation tensor (SURVEY.md §7 "shared in-place ReLU").  ReLU and tanh ONLY: the entry points
// that use it refuse the smooth codes (act_is_smooth), whose backward goes through act_grad_pre.
__device__ __forceinline__ float act_bwd(float g, float y, int act) {
    if (act == DYNMM_ACT_RELU) return y > 0.f ? g : 0.f;
    if (act == DYNMM_ACT_TANH) return g * (1.f - y * y);
    return g;
}

static inline bool act_is_smooth(int act) { return act == DYNMM_ACT_SWISH || act == DYNMM_ACT_HSWISH; }
static inline bool act_is_known(int act) { return act >= DYNMM_ACT_NONE && act <= DYNMM_ACT_HSWISH; }

// eval.py:117-141 for ONE output pixel (oh, ow): the bilinear resize (align_corners=False, scales sh = H / Ho, sw = W / Wo) of
// the C logit planes xn [C,H,W] and the first-maximum arg-max over classes (v > best from -inf, as torch.argmax).  The one
// home of this arithmetic: eval_confusion_kernel (loss_opt.hip) counts its result, argmax_resize_kernel (segment.hip) keeps it.
__device__ __forceinline__ int resize_argmax_px(const float* __restrict__ xn, int C, int H, int W, float sh, float sw, int oh,
                                                int ow) {
    float fy = sh * ((float)oh + 0.5f) - 0.5f, fx = sw * ((float)ow + 0.5f) - 0.5f;
    fy = fy < 0.f ? 0.f : fy;
    fx = fx < 0.f ? 0.f : fx;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
    const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    float best = -INFINITY;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
        const float* pc = xn + (size_t)c * H * W;
        const float v = ly0 * (lx0 * pc[y0 * W + x0] + lx1 * pc[y0 * W + x1]) +
                        ly1 * (lx0 * pc[y1 * W + x0] + lx1 * pc[y1 * W + x1]);
        if (v > best) { best = v; arg = c; }       // first maximum, as torch.argmax
    }
    return arg;
}

// out[i] = sum_s slabs[s][i] (+ an optional second region) in a fixed order: the deterministic tail of every
// split reduction in the library (conv_igemm.hip).
void launch_reduce_slabs(const float* slabs, float* out, int n, int nslabs, hipStream_t st,
                         const float* slabs2 = nullptr, float* out2 = nullptr, int n2 = 0);

}  // namespace dynmm
