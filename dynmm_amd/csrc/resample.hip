// The decoder's other resampling modes (src/models/model.py:360-410, context_modules.py:70-131):
//   * x2 up-sampling 'nearest' / 'bilinear' (align_corners=False), with the decoder's skip add fused;
//   * 'learned-3x3': nearest x2, ReplicationPad2d(1), depthwise 3x3 — the replicate-border sibling of pointwise.hip's
//     learned-3x3-zeropad kernels (those stay as they are);
//   * the bilinear resize of a pyramid-pooling branch from its (h, w) bin grid into a channel slice of the concat.
//
// Every x2 mode is the same 2x2 stencil on the INPUT with clamped neighbours.  With R(u) = clamp(floor(u / 2), 0, H-1) the
// replicate-padded nearest map reads x[R(oh + r - 1)] for tap r, so output row 2i reads rows {i-1: w0, i: w1+w2} and row 2i+1
// reads {i: w0+w1, i+1: w2} with i-1 / i+1 CLAMPED (the zero-pad kernels drop them instead).  Bilinear x2 with
// align_corners=False is exactly this stencil with w = [1,2,1] (x) [1,2,1] / 16 and no bias: ATen's source index
// 0.5 * (2i + 0.5) - 0.5 = i - 0.25 gives {i-1: 1/4, i: 3/4} (clamped to x[0] at i = 0 by the `src < 0 -> 0` rule), and
// i + 0.25 gives {i: 3/4, i+1: 1/4} (the `h1 = h0 + (h0 < in-1)` rule clamps i+1 at the last row).  Nearest x2 reads
// x[oh >> 1] (ATen's floor(dst * 0.5)).
//
// Backward passes are gathers (one lane per input pixel pair / per bin-grid element): no atomics, a fixed summation order.
#include "common.h"
#include "vec.h"

namespace dynmm {

#define ST ((hipStream_t)stream)

namespace {

constexpr int kRsChunk = 8192;
enum { kUpNearest = DYNMM_UP_NEAREST, kUpBilinear = DYNMM_UP_BILINEAR, kUpLearned = 2 };

// v where keep, +0.0 otherwise (a bit mask on the loaded value, so the load itself stays unconditional)
__device__ __forceinline__ float rs_keep(float v, bool keep) { return __int_as_float(__float_as_int(v) & -(int)keep); }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the 3x3 taps of a mode: the learned weights of channel c, or the bilinear-equivalent [1,2,1]x[1,2,1]/16
template <int MODE>
__device__ __forceinline__ void load_taps(float (&k)[9], const float* __restrict__ wgt, int c) {
    if constexpr (MODE == kUpLearned) {
#pragma unroll
        for (int j = 0; j < 9; ++j) k[j] = wgt[c * 9 + j];
    } else {
        constexpr float t[3] = {0.25f, 0.5f, 0.25f};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int q = 0; q < 3; ++q) k[r * 3 + q] = t[r] * t[q];
    }
}

// ------------------------------------------------------------------------------------------------
// x2 forward.  One lane owns input pixels (i, j0), (i, j0+1) = a 2x4 output patch; its 3x4 input neighbourhood is
// loaded on clamped coordinates (replicate borders).  grid (N*C, chunks of the plane)
// ------------------------------------------------------------------------------------------------
template <int MODE>
__global__ void __launch_bounds__(256) up2x_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wgt,
                                                       const float* __restrict__ bias, const float* __restrict__ skip,
                                                       float* __restrict__ y, int C, int H, int W) {
    const size_t plane = blockIdx.x;
    const int c = (int)(plane % C);
    const int W2 = 2 * W;
    const float* xp = x + plane * H * W;
    float* yp = y + plane * 4 * H * W;
    const float* sp = skip ? skip + plane * 4 * H * W : nullptr;
    // rc[a_row][which_row][a_col][which_col]: a = 0 (even output) {prev: w0, this: w1+w2}; a = 1 (odd) {this: w0+w1, next: w2}
    float rc[2][2][2][2];
    float b = 0.f;
    if constexpr (MODE != kUpNearest) {
        float k[9];
        load_taps<MODE>(k, wgt, c);
        if constexpr (MODE == kUpLearned) b = bias ? bias[c] : 0.f;
#pragma unroll
        for (int ar = 0; ar < 2; ++ar)
#pragma unroll
            for (int wr = 0; wr < 2; ++wr)
#pragma unroll
                for (int ac = 0; ac < 2; ++ac)
#pragma unroll
                    for (int wc = 0; wc < 2; ++wc) {
                        float s = 0.f;
#pragma unroll
                        for (int r = 0; r < 3; ++r) {
                            const bool rin = ar == 0 ? (wr == 0 ? r == 0 : r >= 1) : (wr == 0 ? r <= 1 : r == 2);
                            if (!rin) continue;
#pragma unroll
                            for (int q = 0; q < 3; ++q) {
                                const bool qin = ac == 0 ? (wc == 0 ? q == 0 : q >= 1) : (wc == 0 ? q <= 1 : q == 2);
                                if (qin) s += k[r * 3 + q];
                            }
                        }
                        rc[ar][wr][ac][wc] = s;
                    }
    }
    const int Wh = (W + 1) / 2;
    const int items = H * Wh;
    const int beg = blockIdx.y * (kRsChunk / 8), end = min(items, beg + kRsChunk / 8);
    for (int it = beg + threadIdx.x; it < end; it += 256) {
        const int i = it / Wh, j0 = (it - i * Wh) * 2;
        const bool two = j0 + 1 < W;
        float v[3][4];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            if (MODE == kUpNearest && r != 1) continue;
            const float* row = xp + (size_t)clampi(i + r - 1, 0, H - 1) * W;
#pragma unroll
            for (int q = 0; q < 4; ++q) v[r][q] = row[clampi(j0 + q - 1, 0, W - 1)];
        }
#pragma unroll
        for (int ar = 0; ar < 2; ++ar) {
            float o[4];
#pragma unroll
            for (int pc = 0; pc < 2; ++pc)
#pragma unroll
                for (int ac = 0; ac < 2; ++ac) {
                    if constexpr (MODE == kUpNearest) {
                        o[pc * 2 + ac] = v[1][pc + 1];
                    } else {
                        const int r0 = ar, c0 = pc + ac;
                        o[pc * 2 + ac] = b + rc[ar][0][ac][0] * v[r0][c0] + rc[ar][0][ac][1] * v[r0][c0 + 1] +
                                         rc[ar][1][ac][0] * v[r0 + 1][c0] + rc[ar][1][ac][1] * v[r0 + 1][c0 + 1];
                    }
                }
            const size_t off = (size_t)(2 * i + ar) * W2 + 2 * j0;
            if (two && (W2 % 4 == 0)) {
                if (sp) {
                    const float4 sk = *reinterpret_cast<const float4*>(sp + off);
                    o[0] += sk.x; o[1] += sk.y; o[2] += sk.z; o[3] += sk.w;
                }
                *reinterpret_cast<float4*>(yp + off) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
                const int nout = two ? 4 : 2;
                for (int q = 0; q < nout; ++q) yp[off + q] = o[q] + (sp ? sp[off + q] : 0.f);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// x2 input gradient.  dx[i][j] = sum_{a,b in 0..3} e[a][b] * g[2i+a-1][2j+b-1] (rows / cols outside the map add zero).
// The tap sets seen from input row i: a=0 {w2}, a=1 {w1,w2} + {w0 if i = 0}, a=2 {w0,w1} + {w2 if i = H-1}, a=3 {w0}
// (the clamped neighbour of a border row is the row itself); same along columns.  One lane owns input pixels (i, j0),
// (i, j0+1): a 4x6 patch of g, per row two 8-byte loads and two edge scalars, all on clamped coordinates.
// ------------------------------------------------------------------------------------------------
template <int MODE>
__global__ void __launch_bounds__(256) up2x_bwd_dx_kernel(const float* __restrict__ g, const float* __restrict__ wgt,
                                                          float* __restrict__ dx, int C, int H, int W) {
    const size_t plane = blockIdx.x;
    const int c = (int)(plane % C);
    const int H2 = 2 * H, W2 = 2 * W;
    const float* gp = g + plane * H2 * W2;
    float* dp = dx + plane * H * W;
    float k[9];
    if constexpr (MODE != kUpNearest) load_taps<MODE>(k, wgt, c);
    const int Wh = (W + 1) / 2;
    const int items = H * Wh;
    const int beg = blockIdx.y * (kRsChunk / 2), end = min(items, beg + kRsChunk / 2);
    for (int it = beg + threadIdx.x; it < end; it += 256) {
        const int i = it / Wh, j0 = (it - i * Wh) * 2;
        const bool two = j0 + 1 < W;
        float s0 = 0.f, s1 = 0.f;
        if constexpr (MODE == kUpNearest) {
            // dx = the 2x2 block of g over the pixel: rows 2i, 2i+1, cols 2j .. 2j+1
            const int cm = min(2 * j0 + 2, W2 - 2);
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const float* row = gp + (size_t)(2 * i + a) * W2;
                const float2 m0 = *reinterpret_cast<const float2*>(row + 2 * j0);
                const float2 m1 = *reinterpret_cast<const float2*>(row + cm);
                s0 += m0.x + m0.y;
                s1 += m1.x + m1.y;
            }
        } else {
            float4 m[4];     // cols 2j0 .. 2j0+3 as two 8-byte halves (the row pitch 2W is only 8-byte aligned for odd W)
            float lft[4], rgt[4];
            const int cm = min(2 * j0 + 2, W2 - 2);
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const float* row = gp + (size_t)clampi(2 * i + a - 1, 0, H2 - 1) * W2;
                const float2 h0 = *reinterpret_cast<const float2*>(row + 2 * j0);
                const float2 h1 = *reinterpret_cast<const float2*>(row + cm);
                m[a] = make_float4(h0.x, h0.y, h1.x, h1.y);
                lft[a] = row[max(2 * j0 - 1, 0)];
                rgt[a] = row[min(2 * j0 + 4, W2 - 1)];
            }
            // row-reduced taps wr[a][q] = sum_{r in R(a)} k[r][q]
            const bool top = i == 0, bot = i == H - 1;
            float wr[4][3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                wr[0][q] = k[6 + q];
                wr[1][q] = k[3 + q] + k[6 + q] + (top ? k[q] : 0.f);
                wr[2][q] = k[q] + k[3 + q] + (bot ? k[6 + q] : 0.f);
                wr[3][q] = k[q];
            }
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int j = j0 + p;
                const bool lb = j == 0, rb = j >= W - 1;
                float s = 0.f;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const int oh = 2 * i + a - 1;
                    const bool rok = oh >= 0 && oh < H2;
                    // the 4 columns 2j-1 .. 2j+2 of this pixel
                    const float c0 = p == 0 ? lft[a] : m[a].y;
                    const float c1 = p == 0 ? m[a].x : m[a].z;
                    const float c2 = p == 0 ? m[a].y : m[a].w;
                    const float c3 = p == 0 ? m[a].z : rgt[a];
                    const float e0 = wr[a][2];
                    const float e1 = wr[a][1] + wr[a][2] + (lb ? wr[a][0] : 0.f);
                    const float e2 = wr[a][0] + wr[a][1] + (rb ? wr[a][2] : 0.f);
                    const float e3 = wr[a][0];
                    s += e0 * rs_keep(c0, rok && !lb) + e1 * rs_keep(c1, rok) + e2 * rs_keep(c2, rok) +
                         e3 * rs_keep(c3, rok && !rb);
                }
                if (p == 0) s0 = s; else s1 = s;
            }
        }
        float* o = dp + (size_t)i * W + j0;
        if (two && (W % 2 == 0)) {
            *reinterpret_cast<float2*>(o) = make_float2(s0, s1);
        } else {
            o[0] = s0;
            if (two) o[1] = s1;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// learned-3x3 (replicate) filter / bias gradient: part_w[split][c][r][s] = sum g * U_pad, part_b[split][c] = sum g.
// grid (C, splits over n), splits summed in a fixed order by launch_reduce_slabs.  U_pad(uy, ux) = x[R(uy)][R(ux)].
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) up2x_rep_bwd_w_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                             float* __restrict__ dw, float* __restrict__ db, int N, int C,
                                                             int H, int W) {
    __shared__ float red[4];
    const int c = blockIdx.x, S = gridDim.y;
    const int H2 = 2 * H, W2 = 2 * W;
    const bool vec = (W2 % 4 == 0);
    float acc[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) acc[j] = 0.f;
    for (int n = blockIdx.y; n < N; n += S) {
        const float* gp = g + ((size_t)n * C + c) * H2 * W2;
        const float* xp = x + ((size_t)n * C + c) * H * W;
        if (vec) {
            const int Wq = W2 / 4, items = H2 * Wq;
            for (int it = threadIdx.x; it < items; it += 256) {
                const int oh = it / Wq, ow0 = (it - oh * Wq) * 4;
                const float4 gq = *reinterpret_cast<const float4*>(gp + (size_t)oh * W2 + ow0);
                const float gv[4] = {gq.x, gq.y, gq.z, gq.w};
                acc[9] += (gv[0] + gv[1]) + (gv[2] + gv[3]);
                const int jb = ow0 / 2;     // outputs ow0..ow0+3 see input cols R(ow0-1) = max(jb-1, 0) .. R(ow0+4) = min(jb+2, W-1)
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float* row = xp + (size_t)(clampi(oh + r - 1, 0, H2 - 1) >> 1) * W;
                    const float xm = row[max(jb - 1, 0)];
                    const float x0 = row[jb], x1 = row[jb + 1];
                    const float xpv = row[min(jb + 2, W - 1)];
                    acc[r * 3 + 0] += gv[0] * xm + gv[1] * x0 + gv[2] * x0 + gv[3] * x1;
                    acc[r * 3 + 1] += gv[0] * x0 + gv[1] * x0 + gv[2] * x1 + gv[3] * x1;
                    acc[r * 3 + 2] += gv[0] * x0 + gv[1] * x1 + gv[2] * x1 + gv[3] * xpv;
                }
            }
        } else {
            for (int i = threadIdx.x; i < H2 * W2; i += 256) {
                const int oh = i / W2, ow = i - oh * W2;
                const float gv = gp[i];
                acc[9] += gv;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float* row = xp + (size_t)(clampi(oh + r - 1, 0, H2 - 1) >> 1) * W;
#pragma unroll
                    for (int s = 0; s < 3; ++s) acc[r * 3 + s] += gv * row[clampi(ow + s - 1, 0, W2 - 1) >> 1];
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        const float t = block_reduce_sum_256<float>(acc[j], red);
        if (threadIdx.x == 0) {
            if (j < 9) dw[((size_t)blockIdx.y * C + c) * 9 + j] = t;
            else if (db) db[(size_t)blockIdx.y * C + c] = t;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// bilinear resize (align_corners=False) of y[N,C,h,w] into channels [c_off, c_off+C) of out[N,Ctot,H,W]:
// ATen's area_pixel_compute_source_index (scale = (float)in / out, src = scale * (dst + 0.5) - 0.5, negative -> 0),
// i0 = (int)src, i1 = i0 + (i0 < in-1), l1 = src - i0, l0 = 1 - l1.
// ------------------------------------------------------------------------------------------------
struct LinSrc {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ LinSrc lin_src(int dst, int in, int out) {
    const float scale = (float)in / (float)out;
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    LinSrc r;
    r.i0 = min((int)s, in - 1);
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    r.l1 = fminf(fmaxf(s - (float)r.i0, 0.f), 1.f);
    r.l0 = 1.f - r.l1;
    return r;
}

// one lane = 4 consecutive outputs of a row (16-byte store when the row pitch allows)
__global__ void __launch_bounds__(256) bilinear_into_fwd_kernel(const float* __restrict__ y, float* __restrict__ out, int C,
                                                                int h, int w, int Ctot, int c_off, int H, int W, int items,
                                                                int vec) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= items) return;
    const int Wq = (W + 3) / 4;
    const int x0 = (t % Wq) * 4, yy = (t / Wq) % H, c = (t / (Wq * H)) % C, n = t / (Wq * H * C);
    const float* yp = y + ((size_t)n * C + c) * h * w;
    float* op = out + (((size_t)n * Ctot + c_off + c) * H + yy) * W;
    const LinSrc sy = lin_src(yy, h, H);
    const float* r0 = yp + (size_t)sy.i0 * w;
    const float* r1 = yp + (size_t)sy.i1 * w;
    float o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const LinSrc sx = lin_src(min(x0 + q, W - 1), w, W);
        const float a = r0[sx.i0], b = r0[sx.i1], cc = r1[sx.i0], d = r1[sx.i1];
        o[q] = sy.l0 * (sx.l0 * a + sx.l1 * b) + sy.l1 * (sx.l0 * cc + sx.l1 * d);
    }
    if (vec) {
        *reinterpret_cast<float4*>(op + x0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (x0 + q < W) op[x0 + q] = o[q];
    }
}

// Backward: dy[p][q] = sum over the output pixels that read (p, q) of g * wy * wx.  The rows whose i0 or i1 is p form one
// contiguous range (both are monotone in the destination index), so do the columns; L lanes share one element, walk that
// rectangle L at a time (coalesced) and meet in a fixed xor-butterfly — nearest_into_bwd_kernel's scheme.
__device__ __forceinline__ float lin_weight(const LinSrc& s, int p) {
    return (s.i0 == p ? s.l0 : 0.f) + (s.i1 == p ? s.l1 : 0.f);
}

template <int L>
__global__ void __launch_bounds__(256) bilinear_into_bwd_kernel(const float* __restrict__ g, float* __restrict__ dy, int N,
                                                                int C, int h, int w, int Ctot, int c_off, int H, int W) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int i = t / L, l = t % L;
    const bool live = i < N * C * h * w;
    const int ii = live ? i : 0;
    const int q = ii % w, p = (ii / w) % h, c = (ii / (w * h)) % C, n = ii / (w * h * C);
    const float* gp = g + ((size_t)n * Ctot + c_off + c) * H * W;
    int y0 = H, y1 = 0, x0 = W, x1 = 0;
    for (int yy = 0; yy < H; ++yy) {
        const LinSrc s = lin_src(yy, h, H);
        if (s.i0 == p || s.i1 == p) { y0 = min(y0, yy); y1 = yy + 1; }
    }
    for (int x = 0; x < W; ++x) {
        const LinSrc s = lin_src(x, w, W);
        if (s.i0 == q || s.i1 == q) { x0 = min(x0, x); x1 = x + 1; }
    }
    const int rw = max(x1 - x0, 0), cnt = rw * max(y1 - y0, 0);
    float acc = 0.f;
    for (int e = l; e < cnt; e += L) {
        const int r = e / rw, yy = y0 + r, x = x0 + (e - r * rw);
        acc += gp[(size_t)yy * W + x] * (lin_weight(lin_src(yy, h, H), p) * lin_weight(lin_src(x, w, W), q));
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, L);
    if (live && l == 0) dy[i] = acc;
}

int up_w_splits(int N, int C) {
    int S = 2048 / C;
    if (S < 1) S = 1;
    if (S > N) S = N;
    return S;
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" int dynmm_upsample2x_fwd(const float* x, const float* skip, float* y, int N, int C, int H, int W, int mode,
                                    void* stream) {
    (void)hipGetLastError();   // drop stale errors left by other users of the runtime
    if (!x || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0) return DYNMM_EINVAL;
    if (!aligned16(y) || (skip && !aligned16(skip))) return DYNMM_EUNSUPPORTED;
    dim3 grid(N * C, ceil_div(H * ((W + 1) / 2), kRsChunk / 8));
    if (mode == DYNMM_UP_NEAREST)
        hipLaunchKernelGGL(up2x_fwd_kernel<kUpNearest>, grid, dim3(256), 0, ST, x, nullptr, nullptr, skip, y, C, H, W);
    else if (mode == DYNMM_UP_BILINEAR)
        hipLaunchKernelGGL(up2x_fwd_kernel<kUpBilinear>, grid, dim3(256), 0, ST, x, nullptr, nullptr, skip, y, C, H, W);
    else
        return DYNMM_EINVAL;
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_upsample2x_bwd(const float* g, float* dx, int N, int C, int H, int W, int mode, void* stream) {
    (void)hipGetLastError();
    if (!g || !dx || N <= 0 || C <= 0 || H <= 0 || W <= 0) return DYNMM_EINVAL;
    if (!aligned8(g) || !aligned8(dx)) return DYNMM_EUNSUPPORTED;
    dim3 grid(N * C, ceil_div(H * ((W + 1) / 2), kRsChunk / 2));
    if (mode == DYNMM_UP_NEAREST)
        hipLaunchKernelGGL(up2x_bwd_dx_kernel<kUpNearest>, grid, dim3(256), 0, ST, g, nullptr, dx, C, H, W);
    else if (mode == DYNMM_UP_BILINEAR)
        hipLaunchKernelGGL(up2x_bwd_dx_kernel<kUpBilinear>, grid, dim3(256), 0, ST, g, nullptr, dx, C, H, W);
    else
        return DYNMM_EINVAL;
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_upsample2x_dw3x3_rep_fwd(const float* x, const float* w, const float* b, const float* skip, float* y,
                                              int N, int C, int H, int W, void* stream) {
    (void)hipGetLastError();
    if (!x || !w || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0) return DYNMM_EINVAL;
    if (!aligned16(y) || (skip && !aligned16(skip))) return DYNMM_EUNSUPPORTED;
    dim3 grid(N * C, ceil_div(H * ((W + 1) / 2), kRsChunk / 8));
    hipLaunchKernelGGL(up2x_fwd_kernel<kUpLearned>, grid, dim3(256), 0, ST, x, w, b, skip, y, C, H, W);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_upsample2x_dw3x3_rep_bwd(const float* g, const float* x, const float* w, float* dx, float* dw,
                                              float* db, float* workspace, int N, int C, int H, int W, void* stream) {
    (void)hipGetLastError();
    if (!g || !w || N <= 0 || C <= 0 || H <= 0 || W <= 0) return DYNMM_EINVAL;
    if (dx) {
        if (!aligned8(g) || !aligned8(dx)) return DYNMM_EUNSUPPORTED;
        dim3 grid(N * C, ceil_div(H * ((W + 1) / 2), kRsChunk / 2));
        hipLaunchKernelGGL(up2x_bwd_dx_kernel<kUpLearned>, grid, dim3(256), 0, ST, g, w, dx, C, H, W);
        DYNMM_LAUNCH_CHECK();
    }
    if (dw) {
        if (!x || ((2 * W) % 4 == 0 && !aligned16(g))) return DYNMM_EINVAL;
        const int S = up_w_splits(N, C);   // the workspace layout of dynmm_upsample2x_dw3x3_bwd_workspace_bytes
        if (S == 1) {
            hipLaunchKernelGGL(up2x_rep_bwd_w_kernel, dim3(C, 1), dim3(256), 0, ST, g, x, dw, db, N, C, H, W);
            DYNMM_LAUNCH_CHECK();
        } else {
            if (!workspace) return DYNMM_EWORKSPACE;
            float* pw = workspace, *pb = workspace + (size_t)S * C * 9;
            hipLaunchKernelGGL(up2x_rep_bwd_w_kernel, dim3(C, S), dim3(256), 0, ST, g, x, pw, db ? pb : nullptr, N, C, H, W);
            DYNMM_LAUNCH_CHECK();
            launch_reduce_slabs(pw, dw, C * 9, S, ST, db ? pb : nullptr, db, db ? C : 0);
            DYNMM_LAUNCH_CHECK();
        }
    }
    return DYNMM_OK;
}

extern "C" int dynmm_bilinear_into_fwd(const float* y, float* out, int N, int C, int h, int w, int Ctot, int c_off, int H,
                                       int W, void* stream) {
    (void)hipGetLastError();
    if (!y || !out || N <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return DYNMM_EINVAL;
    if (c_off < 0 || c_off + C > Ctot) return DYNMM_EINVAL;
    const int items = N * C * H * ((W + 3) / 4);
    const int vec = (W % 4 == 0) && aligned16(out);
    hipLaunchKernelGGL(bilinear_into_fwd_kernel, dim3(ceil_div(items, 256)), dim3(256), 0, ST, y, out, C, h, w, Ctot, c_off,
                       H, W, items, vec);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_bilinear_into_bwd(const float* g_out, float* dy, int N, int C, int h, int w, int Ctot, int c_off, int H,
                                       int W, void* stream) {
    (void)hipGetLastError();
    if (!g_out || !dy || N <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return DYNMM_EINVAL;
    if (c_off < 0 || c_off + C > Ctot) return DYNMM_EINVAL;
    // lanes per element: a power of two near a quarter of the rectangle it collects from
    const int area = (ceil_div(H, h) + 2) * (ceil_div(W, w) + 2);
    const int nout = N * C * h * w;
#define DYNMM_BIB(L) hipLaunchKernelGGL(bilinear_into_bwd_kernel<L>, dim3(ceil_div_sz((size_t)nout * L, 256)), dim3(256), 0, ST, \
                                        g_out, dy, N, C, h, w, Ctot, c_off, H, W)
    if (area < 8) DYNMM_BIB(1);
    else if (area < 32) DYNMM_BIB(4);
    else if (area < 128) DYNMM_BIB(16);
    else DYNMM_BIB(64);
#undef DYNMM_BIB
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

}  // namespace dynmm
