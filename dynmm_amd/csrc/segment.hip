// Label maps at inference: the arg-max over classes kept as a uint8 image instead of logits.
//
// tail_argmax_kernel is the inference tail of the decoder as ONE kernel: the two learned 2x up-samplings (model.py:404-410,
// C <= 64 channels, H x W -> 4H x 4W) and the arg-max over channels.  Unfused, this tail writes the half-resolution map and
// the full-resolution logits and reads both back (2.0 GB per batch of 16 at 480x640); fused it reads the
// quarter-resolution map once and writes one byte per output pixel.
//
// Stencil cascade.  One learned up-sampling is nearest-2x followed by a depthwise 3x3, which collapses to a 2x2 window of
// its INPUT with pre-summed taps (up2_taps.h; tail.hip has the derivation): output row R reads input rows
// floor((R-1)/2) and floor((R-1)/2) + 1 with the tap sums of parity R & 1.  Applied twice: u = up1(x) on the 2H x 2W grid,
// y = up2(u) on the 4H x 4W grid.  The channels are independent, so a workgroup streams them and keeps only a running
// (best, arg) per output pixel.
//
// Border rule.  'learned-3x3-zeropad' (border 0): each conv pads its own nearest-2x map with zeros.  For stage 1 that is "x
// outside the image reads 0"; for stage 2 it is "u outside the 2H x 2W grid reads 0" — the VALUE 0, not b1 and not up1
// evaluated outside the image — so b1 reaches a border logit through fewer of w2's taps than an interior one.
// 'learned-3x3' (border 1) replicates: both stages clamp their index.  With x staged at clamped addresses, up1 evaluated one
// step outside the grid has the clamped row's inputs under tap sums that add up to the same total, so the natural
// evaluation IS the clamped value (up to the order of the fp32 additions of the taps).
#include "common.h"
#include "up2_taps.h"
#include "vec.h"

namespace dynmm {

// Work decomposition.  A workgroup of 256 lanes owns kSR x kSC = 8 x 32 pixels of x of one image = 32 x 128 output pixels;
// lane (ty, tx) = (tid >> 5, tid & 31) owns x pixel (ti0 + ty, tj0 + tx) and its 4 x 4 outputs.  Per channel:
//   x tile  (kSR + 2) x (kSC + 2): rows ti0 - 1 .., cols tj0 - 1 ..            (halo 1)
//   u tile  (2 kSR + 2) x (2 kSC + 2): u rows 2 ti0 - 1 .., cols 2 tj0 - 1 ..   (halo 1 on the u grid)
// u tile entry (lr, lc) has parity ((lr + 1) & 1, (lc + 1) & 1) and the x-tile window at (lr >> 1, lc >> 1); so the 2 x 2
// "cell" (a, b) = entries (2a.., 2b..) shares ONE x window at (a, b) and has all four parities at compile-time positions:
// (kSR + 1) x (kSC + 1) = 297 cells, one per lane plus 41 for the first wave.
// The lane's 16 outputs read the 4 x 4 u patch at (2 ty, 2 tx): output (a, b) has parity (a & 1, b & 1) and the window at
// patch ((a + 1) >> 1, (b + 1) >> 1).
// Staging as up2ce_fwd_kernel: kSCH channels at a time; the global loads of chunk k + 1 (unconditional, clamped addresses,
// value selected afterwards) are issued before the arithmetic of chunk k and land in the other x buffer after it.
constexpr int kSR = 8, kSC = 32, kSCH = 4;
constexpr int kXP = kSC + 2;                        // x tile pitch
constexpr int kXT = (kSR + 2) * kXP;                // 340 floats per channel
constexpr int kXLoads = (kXT + 255) / 256;          // 2
constexpr int kUP = 2 * kSC + 2;                    // u tile pitch (even: the 2-float accesses stay 8-byte aligned)
constexpr int kUT = (2 * kSR + 2) * kUP;            // 1188 floats per channel
constexpr int kCells = (kSR + 1) * (kSC + 1);       // 297
constexpr int kOutRowBytes = 4 * kSC;               // 128 output pixels per tile row
static_assert(kSR * kSC == 256, "one x pixel per lane");
static_assert(kCells <= 256 + 64, "the second round of cells fits the first wave");
static_assert(4 * kSR * kOutRowBytes <= (int)sizeof(float) * kSCH * kUT, "the output tile aliases the u tiles");

__global__ void __launch_bounds__(256) tail_argmax_kernel(const float* __restrict__ x, const float* __restrict__ w1,
                                                          const float* __restrict__ b1, const float* __restrict__ w2,
                                                          const float* __restrict__ b2, unsigned char* __restrict__ pred,
                                                          int N, int C, int H, int W, int zeropad, int vec16) {
    __shared__ __attribute__((aligned(16))) float coef1[kTailMaxC][kCoefLd];
    __shared__ __attribute__((aligned(16))) float coef2[kTailMaxC][kCoefLd];
    __shared__ __attribute__((aligned(16))) float xt[2][kSCH * kXT];
    __shared__ __attribute__((aligned(16))) float ut[kSCH * kUT];
    tail_build_coef(w1, b1, coef1, C);
    tail_build_coef(w2, b2, coef2, C);

    const int tw = (W + kSC - 1) / kSC, th = (H + kSR - 1) / kSR;
    int blk = blockIdx.x;
    const int n = blk / (th * tw);
    blk -= n * th * tw;
    const int ti0 = (blk / tw) * kSR, tj0 = (blk - (blk / tw) * tw) * kSC;
    const int tid = threadIdx.x, ty = tid >> 5, tx = tid & 31;
    const int HW = H * W;
    const bool zp = zeropad != 0;

    // staging geometry: element e of the x tile
    int gofs[kXLoads];
    bool gin[kXLoads], gzero[kXLoads];
#pragma unroll
    for (int k = 0; k < kXLoads; ++k) {
        const int e = k * 256 + tid;
        const int r = e / kXP, q = e - r * kXP;
        const int ii = ti0 - 1 + r, jj = tj0 - 1 + q;
        gin[k] = e < kXT;
        gzero[k] = zp && !(ii >= 0 && ii < H && jj >= 0 && jj < W);
        gofs[k] = min(max(ii, 0), H - 1) * W + min(max(jj, 0), W - 1);
    }
    // stage-1 geometry: the lane's cells (the second one exists for the first 41 lanes only)
    int cell_x[2], cell_u[2];
    bool uz[2][2][2];                               // uz: the entry lies outside the 2H x 2W grid and zero padding is on
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int e = k * 256 + tid;
        const int ee = e < kCells ? e : 0;
        const int a = ee / (kSC + 1), b = ee - a * (kSC + 1);
        cell_x[k] = a * kXP + b;
        cell_u[k] = 2 * a * kUP + 2 * b;
#pragma unroll
        for (int dr = 0; dr < 2; ++dr)
#pragma unroll
            for (int dc = 0; dc < 2; ++dc) {
                const int p = 2 * ti0 - 1 + 2 * a + dr, q = 2 * tj0 - 1 + 2 * b + dc;
                uz[k][dr][dc] = zp && !(p >= 0 && p < 2 * H && q >= 0 && q < 2 * W);
            }
    }
    const int ncell = tid < kCells - 256 ? 2 : 1;   // 2 in the first wave only
    const int pofs = 2 * ty * kUP + 2 * tx;         // the lane's u patch

    float best[16];
    int arg[16];
#pragma unroll
    for (int o = 0; o < 16; ++o) {
        best[o] = -INFINITY;
        arg[o] = 0;
    }

    const float* xn = x + (size_t)n * C * HW;
    float st[kSCH][kXLoads];
    auto stage_load = [&](int c0) {
#pragma unroll
        for (int s = 0; s < kSCH; ++s) {
            const float* xc = xn + (size_t)min(c0 + s, C - 1) * HW;
#pragma unroll
            for (int k = 0; k < kXLoads; ++k) st[s][k] = xc[gofs[k]];
        }
    };
    auto stage_store = [&](float* __restrict__ buf) {
#pragma unroll
        for (int s = 0; s < kSCH; ++s)
#pragma unroll
            for (int k = 0; k < kXLoads; ++k)
                if (gin[k]) buf[s * kXT + k * 256 + tid] = gzero[k] ? 0.f : st[s][k];
    };
    stage_load(0);
    stage_store(xt[0]);
    __syncthreads();
    for (int c0 = 0, kb = 0; c0 < C; c0 += kSCH, kb ^= 1) {
        const bool more = c0 + kSCH < C;
        if (more) stage_load(c0 + kSCH);            // in flight during this chunk's arithmetic
        const int nch = min(kSCH, C - c0);
        // stage 1: the u tiles of the chunk's channels
        for (int sl = 0; sl < nch; ++sl) {
            const float* cf = coef1[c0 + sl];
            const float* xs = xt[kb] + sl * kXT;
            float* us = ut + sl * kUT;
            for (int k = 0; k < ncell; ++k) {
                const float* xw = xs + cell_x[k];
                const float v00 = xw[0], v01 = xw[1], v10 = xw[kXP], v11 = xw[kXP + 1];
#pragma unroll
                for (int dr = 0; dr < 2; ++dr) {
                    float2 o;
#pragma unroll
                    for (int dc = 0; dc < 2; ++dc) {
                        const int ar = 1 - dr, ac = 1 - dc;         // entry (2a + dr, 2b + dc): parity (lr + 1) & 1
                        float u = cf[16] + cf[tail_ci(ar, 0, ac, 0)] * v00 + cf[tail_ci(ar, 0, ac, 1)] * v01 +
                                  cf[tail_ci(ar, 1, ac, 0)] * v10 + cf[tail_ci(ar, 1, ac, 1)] * v11;
                        u = uz[k][dr][dc] ? 0.f : u;
                        if (dc == 0) o.x = u;
                        else o.y = u;
                    }
                    *reinterpret_cast<float2*>(us + cell_u[k] + dr * kUP) = o;
                }
            }
        }
        __syncthreads();
        // stage 2: the lane's 16 outputs of each channel against the running maximum
        for (int sl = 0; sl < nch; ++sl) {
            const int c = c0 + sl;
            const float* cf = coef2[c];
            const float* up = ut + sl * kUT + pofs;
            float u[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float2 lo = *reinterpret_cast<const float2*>(up + r * kUP);
                const float2 hi = *reinterpret_cast<const float2*>(up + r * kUP + 2);
                u[r][0] = lo.x;
                u[r][1] = lo.y;
                u[r][2] = hi.x;
                u[r][3] = hi.y;
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int ar = a & 1, ac = b & 1, r0 = (a + 1) >> 1, q0 = (b + 1) >> 1, o = a * 4 + b;
                    const float v = cf[16] + cf[tail_ci(ar, 0, ac, 0)] * u[r0][q0] + cf[tail_ci(ar, 0, ac, 1)] * u[r0][q0 + 1] +
                                    cf[tail_ci(ar, 1, ac, 0)] * u[r0 + 1][q0] + cf[tail_ci(ar, 1, ac, 1)] * u[r0 + 1][q0 + 1];
                    const bool gt = v > best[o];                    // first maximum, as torch.argmax
                    best[o] = gt ? v : best[o];
                    arg[o] = gt ? c : arg[o];
                }
        }
        if (more) stage_store(xt[kb ^ 1]);
        __syncthreads();
    }
    // the tile's labels through LDS (the u tiles are dead after the last barrier): one 16-byte store per lane
    unsigned* ot = reinterpret_cast<unsigned*>(ut);
#pragma unroll
    for (int a = 0; a < 4; ++a)
        ot[(4 * ty + a) * kSC + tx] = (unsigned)arg[a * 4] | ((unsigned)arg[a * 4 + 1] << 8) |
                                      ((unsigned)arg[a * 4 + 2] << 16) | ((unsigned)arg[a * 4 + 3] << 24);
    __syncthreads();
    const int H4 = 4 * H, W4 = 4 * W;
    const int orow = tid >> 3, og = tid & 7;                        // 32 rows x 8 groups of 16 pixels
    const int R = 4 * ti0 + orow, Q = 4 * tj0 + 16 * og;
    if (R < H4 && Q < W4) {
        const uint4 v = *reinterpret_cast<const uint4*>(ot + orow * kSC + 4 * og);
        unsigned char* dst = pred + ((size_t)n * H4 + R) * W4 + Q;
        if (vec16) *reinterpret_cast<uint4*>(dst) = v;              // W % 4 == 0: the group is whole and 16-byte aligned
        else {
            unsigned* d4 = reinterpret_cast<unsigned*>(dst);        // W4 is a multiple of 4: whole, aligned dwords
            d4[0] = v.x;
            if (Q + 4 < W4) d4[1] = v.y;
            if (Q + 8 < W4) d4[2] = v.z;
            if (Q + 12 < W4) d4[3] = v.w;
        }
    }
}

// arg-max over channels of the bilinear resize of the logits: eval_confusion_kernel's pixel (common.h) with the label kept.
// A lane owns 4 consecutive pixels of an image's Ho*Wo plane and stores them as one dword where the plane allows it.
__global__ void __launch_bounds__(256) argmax_resize_kernel(const float* __restrict__ x, unsigned char* __restrict__ pred,
                                                            int C, int H, int W, int Ho, int Wo, int vec4) {
    const int n = blockIdx.y;
    const float* xn = x + (size_t)n * C * H * W;
    unsigned char* pn = pred + (size_t)n * Ho * Wo;
    const float sh = (float)H / (float)Ho, sw = (float)W / (float)Wo;
    const int P = Ho * Wo;
    for (int p0 = (blockIdx.x * 256 + threadIdx.x) * 4; p0 < P; p0 += gridDim.x * 1024) {
        unsigned packed = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = min(p0 + j, P - 1);
            const int oh = p / Wo, ow = p - oh * Wo;
            packed |= (unsigned)resize_argmax_px(xn, C, H, W, sh, sw, oh, ow) << (8 * j);
        }
        if (vec4) *reinterpret_cast<unsigned*>(pn + p0) = packed;   // P % 4 == 0: the group is whole and aligned
        else
            for (int j = 0; j < 4 && p0 + j < P; ++j) pn[p0 + j] = (unsigned char)(packed >> (8 * j));
    }
}

// cm[(label-1)*C + pred] += 1: a histogram per workgroup in LDS (32-bit counts: a workgroup sees far fewer than 2^32 pixels),
// flushed with 64-bit vector atomics on its non-zero cells.  Integer adds: exact and independent of scheduling.
constexpr int kCmMaxC = 64;
constexpr size_t kCmPixelsPerBlock = 1u << 14;        // a multiple of 16: every workgroup starts on a 16-byte group
__global__ void __launch_bounds__(256) label_confusion_kernel(const unsigned char* __restrict__ pred,
                                                              const unsigned char* __restrict__ label,
                                                              unsigned long long* __restrict__ cm, size_t n, int C,
                                                              int vec16) {
    __shared__ unsigned hist[kCmMaxC * kCmMaxC];
    for (int e = threadIdx.x; e < C * C; e += 256) hist[e] = 0u;
    __syncthreads();
    const size_t beg = (size_t)blockIdx.x * kCmPixelsPerBlock;
    const size_t end = beg + kCmPixelsPerBlock < n ? beg + kCmPixelsPerBlock : n;
    auto count = [&](unsigned pr, unsigned lb) {
        if (lb >= 1u && lb <= (unsigned)C && pr < (unsigned)C) atomicAdd(&hist[(lb - 1u) * C + pr], 1u);
    };
    size_t done = beg;
    if (vec16) {                                                    // both maps 16-byte aligned; beg is a multiple of 16
        const size_t groups = (end - beg) / 16;
        for (size_t gi = threadIdx.x; gi < groups; gi += 256) {
            const uint4 pv = *reinterpret_cast<const uint4*>(pred + beg + gi * 16);
            const uint4 lv = *reinterpret_cast<const uint4*>(label + beg + gi * 16);
            const unsigned pw[4] = {pv.x, pv.y, pv.z, pv.w}, lw[4] = {lv.x, lv.y, lv.z, lv.w};
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) count((pw[q] >> (8 * j)) & 0xffu, (lw[q] >> (8 * j)) & 0xffu);
        }
        done = beg + groups * 16;
    }
    for (size_t i = done + threadIdx.x; i < end; i += 256) count(pred[i], label[i]);
    __syncthreads();
    for (int e = threadIdx.x; e < C * C; e += 256) {
        const unsigned v = hist[e];
        if (v) atomicAdd(&cm[e], (unsigned long long)v);
    }
}

}  // namespace dynmm

using namespace dynmm;

extern "C" int dynmm_tail_argmax(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                                 unsigned char* pred, int N, int C, int H, int W, int border, void* stream) {
    (void)hipGetLastError();
    if (!x || !w1 || !w2 || !pred || N <= 0 || C <= 0 || H <= 0 || W <= 0 || border < 0 || border > 1) return DYNMM_EINVAL;
    if (C > kTailMaxC) return DYNMM_EUNSUPPORTED;
    if ((size_t)H * W > 0x7fffffffu / 16) return DYNMM_EUNSUPPORTED;        // 32-bit offsets inside a plane, both grids
    const size_t blocks = (size_t)N * ceil_div(H, kSR) * ceil_div(W, kSC);
    if (blocks > 0x7fffffffu) return DYNMM_EUNSUPPORTED;
    const int vec16 = (W % 4 == 0 && aligned16(pred)) ? 1 : 0;
    if (!vec16 && (reinterpret_cast<uintptr_t>(pred) & 3u)) return DYNMM_EUNSUPPORTED;
    hipLaunchKernelGGL(tail_argmax_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, w1, b1, w2, b2,
                       pred, N, C, H, W, border == 0 ? 1 : 0, vec16);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_argmax_resize(const float* logits, unsigned char* pred, int N, int C, int H, int W, int Ho, int Wo,
                                   void* stream) {
    (void)hipGetLastError();
    if (!logits || !pred || N <= 0 || C <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return DYNMM_EINVAL;
    if (C > kTailMaxC || N > 65535) return DYNMM_EUNSUPPORTED;
    if ((size_t)H * W > 0x7fffffffu || (size_t)Ho * Wo > 0x7fffffffu - 4096u * 1024u) return DYNMM_EUNSUPPORTED;
    const int P = Ho * Wo;
    const int vec4 = (P % 4 == 0 && (reinterpret_cast<uintptr_t>(pred) & 3u) == 0) ? 1 : 0;
    int bx = ceil_div(P, 1024);
    if (bx > 2048) bx = 2048;
    hipLaunchKernelGGL(argmax_resize_kernel, dim3(bx, N), dim3(256), 0, (hipStream_t)stream, logits, pred, C, H, W, Ho, Wo,
                       vec4);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_label_confusion(const unsigned char* pred, const unsigned char* label, long long* cm, size_t n_pixels,
                                     int C, void* stream) {
    (void)hipGetLastError();
    if (!pred || !label || !cm || C <= 0) return DYNMM_EINVAL;
    if (C > kCmMaxC) return DYNMM_EUNSUPPORTED;
    if (n_pixels == 0) return DYNMM_OK;
    const size_t blocks = ceil_div_sz(n_pixels, kCmPixelsPerBlock);
    if (blocks > 0x7fffffffu) return DYNMM_EUNSUPPORTED;
    const int vec16 = (aligned16(pred) && aligned16(label)) ? 1 : 0;
    hipLaunchKernelGGL(label_confusion_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pred, label,
                       reinterpret_cast<unsigned long long*>(cm), n_pixels, C, vec16);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}
