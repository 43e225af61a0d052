// NYUv2 input pipeline on the device (FusionDynMM/src/preprocessing.py): one launch turns a batch of decoded samples held in
// device memory (uint8 HWC RGB, 16-bit depth, uint8 labels; dynmm_amd/data.py NYUv2) into the network's inputs.
//
// Train (get_preprocessor(phase='train')), per output pixel, mapped back to the stored sample:
//   RandomRescale   cv2.resize to th x tw: INTER_LINEAR on the uint8 image, INTER_NEAREST on depth and label
//   RandomCrop      an height x width window at (ci, cj) — or, when th <= height or tw <= width, a SECOND cv2.resize of
//                   the rescaled sample to height x width (Rescale; mode 1)
//   RandomHSV       matplotlib rgb_to_hsv on 0..255 values (float32), h, s scaled and clipped to [0, 1] (hue clipped, not
//                   wrapped), v shifted and clipped to [0, 255], hsv_to_rgb, no rounding
//   RandomFlip      x -> width - 1 - x
//   Normalize       image / 255 then ImageNet mean / std; depth (d - mean) / std, raw-depth zeros kept at 0
//   MultiScaleLabel cv2 INTER_NEAREST of the augmented label to (h // r, w // r), r = 8, 16, 32
// Test (phase='test'): Rescale to height x width when the stored size differs (mode 1 with th x tw = the stored size), then
// Normalize; no HSV, no flip.
//
// cv2 restated (imgproc/resize.cpp, the generic 8U path):
//   INTER_LINEAR  fx = (float)((d + 0.5) * scale - 0.5), scale = 1 / (out / in) in double; sx = floor(fx), fx -= sx; columns
//                 clamp to the edge with fx = 0, rows clamp their index only; 11-bit weights round((1 - f) * 2048),
//                 round(f * 2048); a row pass in int, then the vertical pass as its SIMD form computes it:
//                 (((H0 >> 4) * b0 >> 16) + ((H1 >> 4) * b1 >> 16) + 2) >> 2
//   INTER_NEAREST sx = min(floor(x * (1 / (out / in))), in - 1) in double
// The float arithmetic is kept in the order and precision numpy uses (no contraction into FMAs), so labels and depth are
// bit-exact and the image differs only where a value sits on a rounding boundary (tests/nyu_aug_oracle.py).
//
// One thread writes 4 consecutive x of one row: three float4 image stores, one float4 depth store, one 4-byte label store.
// Every load is unconditional on an address clamped into the stored sample.
//
// Two entries share the per-pixel code: dynmm_rgbd_aug over a dense [S, H0, W0] store (NYUv2: one size per split) and
// dynmm_rgbd_aug_ragged over flat stores with a per-image {offset, H0, W0} table (SUNRGB-D: four cameras, four sizes, mixed
// within a batch; 64-bit offsets, a split is about 2e9 pixels).
#include "common.h"

#pragma clang fp contract(off)

namespace dynmm {

// per-sample parameter row (int32 [N, 8], dynmm_amd/data.py AUG_FIELDS): stored index, stage-1 size, mode (0 = crop,
// 1 = second resize to height x width), crop offsets, flip
struct AugParams {
    int src, th, tw, mode, ci, cj, flip, pad;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// cv2 INTER_NEAREST source index of output index d (n_in -> n_out)
__device__ __forceinline__ int nn_index(int d, int n_in, int n_out) {
    const double ifx = 1.0 / ((double)n_out / (double)n_in);
    return clampi((int)floor((double)d * ifx), 0, n_in - 1);
}

struct Lin {
    int i0, i1, w0, w1;
};

// cv2 INTER_LINEAR taps and 11-bit weights of output index d; `col`: the column rule (edge taps get weight 0), else the row rule
__device__ __forceinline__ Lin lin_coef(int d, int n_in, int n_out, bool col) {
    const double scale = 1.0 / ((double)n_out / (double)n_in);
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int i = (int)floorf(f);
    f -= (float)i;
    Lin c;
    if (col) {
        if (i < 0) f = 0.f, i = 0;
        if (i >= n_in - 1) f = 0.f, i = n_in - 1;
    }
    c.i0 = clampi(i, 0, n_in - 1);
    c.i1 = clampi(i + 1, 0, n_in - 1);
    c.w0 = (int)rintf((1.f - f) * 2048.f);
    c.w1 = (int)rintf(f * 2048.f);
    return c;
}

__device__ __forceinline__ int lin_combine(int h0, int h1, int b0, int b1) {
    const int v = ((((h0 >> 4) * b0) >> 16) + (((h1 >> 4) * b1) >> 16) + 2) >> 2;
    return clampi(v, 0, 255);
}

// the uint8 RGB of the stage-1 image (stored H0 x W0 resized to th x tw) at (y1, x1)
__device__ __forceinline__ void stage1_rgb(const unsigned char* __restrict__ img, int H0, int W0, int th, int tw, int y1,
                                           int x1, int (&rgb)[3]) {
    if (th == H0 && tw == W0) {                    // the resize is the identity: read the stored pixel
        const unsigned char* p = img + ((size_t)clampi(y1, 0, H0 - 1) * W0 + clampi(x1, 0, W0 - 1)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = p[c];
        return;
    }
    const Lin cy = lin_coef(y1, H0, th, false), cx = lin_coef(x1, W0, tw, true);
    const unsigned char* r0 = img + (size_t)cy.i0 * W0 * 3;
    const unsigned char* r1 = img + (size_t)cy.i1 * W0 * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int h0 = r0[cx.i0 * 3 + c] * cx.w0 + r0[cx.i1 * 3 + c] * cx.w1;
        const int h1 = r1[cx.i0 * 3 + c] * cx.w0 + r1[cx.i1 * 3 + c] * cx.w1;
        rgb[c] = lin_combine(h0, h1, cy.w0, cy.w1);
    }
}

// matplotlib.colors rgb_to_hsv -> scale / shift / clip -> hsv_to_rgb, as RandomHSV calls them on 0..255 values (float32;
// hsv_to_rgb's f, q, t are float64 there: h * 6 minus an int64 array)
__device__ __forceinline__ void hsv_jitter(const int (&in)[3], float hf, float sf, float vf, float (&out)[3]) {
    const float r = (float)in[0], g = (float)in[1], b = (float)in[2];
    const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
    const float delta = mx - mn;
    const float s = mx > 0.f ? delta / mx : 0.f;
    float h = 0.f;
    if (delta > 0.f) {                               // later matches overwrite earlier ones: blue, then green, then red
        if (b == mx) h = 4.f + (r - g) / delta;
        else if (g == mx) h = 2.f + (b - r) / delta;
        else h = (g - b) / delta;
    }
    h = h / 6.f;
    h = fmodf(h, 1.f);                               // numpy's % 1.0: the remainder takes the divisor's sign
    if (h < 0.f) h += 1.f;
    h = fminf(fmaxf(h * hf, 0.f), 1.f);
    const float s2 = fminf(fmaxf(s * sf, 0.f), 1.f);
    const float v = fminf(fmaxf(mx + vf, 0.f), 255.f);
    const float h6 = h * 6.f;
    const int i = (int)h6;
    const double f = (double)h6 - (double)i;
    const float p = v * (1.f - s2);
    const float q = (float)((double)v * (1.0 - (double)s2 * f));
    const float t = (float)((double)v * (1.0 - (double)s2 * (1.0 - f)));
    float o0, o1, o2;
    switch (i % 6) {
        case 0: o0 = v, o1 = t, o2 = p; break;
        case 1: o0 = q, o1 = v, o2 = p; break;
        case 2: o0 = p, o1 = v, o2 = t; break;
        case 3: o0 = p, o1 = q, o2 = v; break;
        case 4: o0 = t, o1 = p, o2 = v; break;
        default: o0 = v, o1 = p, o2 = q; break;
    }
    if (s2 == 0.f) o0 = o1 = o2 = v;
    out[0] = o0, out[1] = o1, out[2] = o2;
}

// the stored (row, column) that augmented pixel (y, xs) (before the flip) takes its depth and label from
__device__ __forceinline__ void nearest_src(const AugParams& P, int H0, int W0, int H, int W, int y, int xs, int& sy, int& sx) {
    int y1, x1;
    if (P.mode == 0) {
        y1 = y + P.ci, x1 = xs + P.cj;
    } else {
        y1 = nn_index(y, P.th, H), x1 = nn_index(xs, P.tw, W);
    }
    sy = nn_index(clampi(y1, 0, P.th - 1), H0, P.th);
    sx = nn_index(clampi(x1, 0, P.tw - 1), W0, P.tw);
}

__device__ __forceinline__ AugParams load_params(const int* __restrict__ params, int n, int S) {
    const int4 a = reinterpret_cast<const int4*>(params)[2 * n];
    const int4 b = reinterpret_cast<const int4*>(params)[2 * n + 1];
    AugParams P;
    P.src = clampi(a.x, 0, S - 1);
    P.th = a.y < 1 ? 1 : a.y;
    P.tw = a.z < 1 ? 1 : a.z;
    P.mode = a.w;
    P.ci = b.x, P.cj = b.y, P.flip = b.z, P.pad = 0;
    return P;
}

// one pixel of the label pyramid: element t of the concatenated label_down[8] / [16] / [32] of the batch, from the stored
// label map `lab` (H0 x W0) of sample n = element / (Hd * Wd); `pick` maps n to that sample's parameters and label map
template <typename Pick>
__device__ __forceinline__ void aug_pyramid_pixel(int t, int N, int H, int W, unsigned char* __restrict__ down8,
                                                  unsigned char* __restrict__ down16, unsigned char* __restrict__ down32,
                                                  Pick pick) {
    unsigned char* dst = nullptr;
    int r = 8;
    for (int k = 0; k < 3; ++k, r *= 2) {
        const int cnt = N * (H / r) * (W / r);
        if (t < cnt) {
            dst = k == 0 ? down8 : (k == 1 ? down16 : down32);
            break;
        }
        t -= cnt;
    }
    if (dst == nullptr) return;
    const int Hd = H / r, Wd = W / r;
    const int n = t / (Hd * Wd), rem = t % (Hd * Wd), dy = rem / Wd, dx = rem % Wd;
    AugParams P;
    const unsigned char* lab;
    int H0, W0;
    pick(n, P, lab, H0, W0);
    const int ya = nn_index(dy, H, Hd), xa = nn_index(dx, W, Wd);
    int sy, sx;
    nearest_src(P, H0, W0, H, W, ya, P.flip ? W - 1 - xa : xa, sy, sx);
    dst[t] = lab[(size_t)sy * W0 + sx];
}

// 4 consecutive x of row y of output sample n from one stored sample (img / dep / lab, H0 x W0): three float4 image stores,
// one float4 depth store, one 4-byte label store
__device__ __forceinline__ void aug_quad(const unsigned char* __restrict__ img, const unsigned short* __restrict__ dep,
                                         const unsigned char* __restrict__ lab, int H0, int W0, const AugParams& P,
                                         const float* __restrict__ hsv, int n, int y, int x0, int H, int W, float depth_mean,
                                         float depth_std, int raw_depth, float* __restrict__ image,
                                         float* __restrict__ depth_out, unsigned char* __restrict__ label_out) {
    float hf = 1.f, sf = 1.f, vf = 0.f;
    if (hsv) hf = hsv[4 * n], sf = hsv[4 * n + 1], vf = hsv[4 * n + 2];
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};

    float im[3][4], dv[4];
    unsigned char lv[4];
    // the second resize's rows are the same for the 4 pixels
    Lin cy2 = {0, 0, 0, 0};
    if (P.mode != 0) cy2 = lin_coef(y, P.th, H, false);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + k;
        const int xs = P.flip ? W - 1 - x : x;
        int px[3];
        if (P.mode == 0) {
            stage1_rgb(img, H0, W0, P.th, P.tw, y + P.ci, xs + P.cj, px);
        } else {
            const Lin cx2 = lin_coef(xs, P.tw, W, true);
            int a[3], b[3], c[3], d[3];
            stage1_rgb(img, H0, W0, P.th, P.tw, cy2.i0, cx2.i0, a);
            stage1_rgb(img, H0, W0, P.th, P.tw, cy2.i0, cx2.i1, b);
            stage1_rgb(img, H0, W0, P.th, P.tw, cy2.i1, cx2.i0, c);
            stage1_rgb(img, H0, W0, P.th, P.tw, cy2.i1, cx2.i1, d);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                px[ch] = lin_combine(a[ch] * cx2.w0 + b[ch] * cx2.w1, c[ch] * cx2.w0 + d[ch] * cx2.w1, cy2.w0, cy2.w1);
        }
        float v[3];
        if (hsv) {
            hsv_jitter(px, hf, sf, vf, v);
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[ch] = (float)px[ch];
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) im[ch][k] = (v[ch] / 255.f - mean[ch]) / stdv[ch];
        int sy, sx;
        nearest_src(P, H0, W0, H, W, y, xs, sy, sx);
        const unsigned short d = dep[(size_t)sy * W0 + sx];
        const float df = ((float)d - depth_mean) / depth_std;
        dv[k] = (raw_depth && d == 0) ? 0.f : df;
        lv[k] = lab[(size_t)sy * W0 + sx];
    }
    const size_t plane = (size_t)H * W, o = (size_t)y * W + x0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        *reinterpret_cast<float4*>(image + ((size_t)n * 3 + ch) * plane + o) = make_float4(im[ch][0], im[ch][1], im[ch][2], im[ch][3]);
    *reinterpret_cast<float4*>(depth_out + (size_t)n * plane + o) = make_float4(dv[0], dv[1], dv[2], dv[3]);
    *reinterpret_cast<uchar4*>(label_out + (size_t)n * plane + o) = make_uchar4(lv[0], lv[1], lv[2], lv[3]);
}

// 5 waves per SIMD = at most 96 VGPRs, what this kernel has always fitted in without scratch (through the shared functions
// the allocator otherwise lands on 97, one wave less)
__global__ void __launch_bounds__(256, 5) rgbd_aug_kernel(
    const unsigned char* __restrict__ rgb, const unsigned short* __restrict__ depth, const unsigned char* __restrict__ label,
    int S, int H0, int W0, const int* __restrict__ params, const float* __restrict__ hsv, int N, int H, int W,
    float depth_mean, float depth_std, int raw_depth, float* __restrict__ image, float* __restrict__ depth_out,
    unsigned char* __restrict__ label_out, unsigned char* __restrict__ down8, unsigned char* __restrict__ down16,
    unsigned char* __restrict__ down32, int main_blocks) {
    const size_t plane0 = (size_t)H0 * W0;
    if ((int)blockIdx.x >= main_blocks) {
        // label pyramid: one thread per pixel of label_down[8] / [16] / [32]
        aug_pyramid_pixel(((int)blockIdx.x - main_blocks) * 256 + (int)threadIdx.x, N, H, W, down8, down16, down32,
                          [&](int n, AugParams& P, const unsigned char*& lab, int& h0, int& w0) {
                              P = load_params(params, n, S);
                              lab = label + P.src * plane0, h0 = H0, w0 = W0;
                          });
        return;
    }
    const int W4 = W >> 2;
    const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (q >= N * H * W4) return;
    const int n = q / (H * W4), rem = q % (H * W4), y = rem / W4, x0 = (rem % W4) * 4;
    const AugParams P = load_params(params, n, S);
    aug_quad(rgb + P.src * plane0 * 3, depth + P.src * plane0, label + P.src * plane0, H0, W0, P, hsv, n, y, x0, H, W,
             depth_mean, depth_std, raw_depth, image, depth_out, label_out);
}

// One stored image of a ragged store (flat rgb / depth / label arrays of `total` pixels): geom row {pixel offset, H0, W0, 0}
// (int64 [S, 4]), read with two 16-byte loads.  The size is clamped into [1, 65535] (1 x 1 when it exceeds the store) and the
// image into [0, total), so every address derived from it stays inside the stores whatever the table holds.
struct RaggedImage {
    long long off;
    int H0, W0;
};

__device__ __forceinline__ RaggedImage load_geom(const long long* __restrict__ geom, int src, long long total) {
    const longlong2 a = reinterpret_cast<const longlong2*>(geom)[2 * (size_t)src];
    const longlong2 b = reinterpret_cast<const longlong2*>(geom)[2 * (size_t)src + 1];
    long long h0 = a.y < 1 ? 1 : (a.y > 65535 ? 65535 : a.y), w0 = b.x < 1 ? 1 : (b.x > 65535 ? 65535 : b.x);
    if (h0 * w0 > total) h0 = w0 = 1;
    RaggedImage g;
    g.H0 = (int)h0, g.W0 = (int)w0;
    const long long last = total - h0 * w0;
    g.off = a.x < 0 ? 0 : (a.x > last ? last : a.x);
    return g;
}

// 101 VGPRs, 4 waves per SIMD, no scratch: the 64-bit offset and the per-lane H0 / W0 cost five registers over the uniform
// kernel, and capping it at 96 spills four of them
__global__ void __launch_bounds__(256) rgbd_aug_ragged_kernel(
    const unsigned char* __restrict__ rgb, const unsigned short* __restrict__ depth, const unsigned char* __restrict__ label,
    const long long* __restrict__ geom, long long total, int S, const int* __restrict__ params, const float* __restrict__ hsv,
    int N, int H, int W, float depth_mean, float depth_std, int raw_depth, float* __restrict__ image,
    float* __restrict__ depth_out, unsigned char* __restrict__ label_out, unsigned char* __restrict__ down8,
    unsigned char* __restrict__ down16, unsigned char* __restrict__ down32, int main_blocks) {
    if ((int)blockIdx.x >= main_blocks) {
        aug_pyramid_pixel(((int)blockIdx.x - main_blocks) * 256 + (int)threadIdx.x, N, H, W, down8, down16, down32,
                          [&](int n, AugParams& P, const unsigned char*& lab, int& h0, int& w0) {
                              P = load_params(params, n, S);
                              const RaggedImage g = load_geom(geom, P.src, total);
                              lab = label + g.off, h0 = g.H0, w0 = g.W0;
                          });
        return;
    }
    const int W4 = W >> 2;
    const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (q >= N * H * W4) return;
    const int n = q / (H * W4), rem = q % (H * W4), y = rem / W4, x0 = (rem % W4) * 4;
    const AugParams P = load_params(params, n, S);
    const RaggedImage g = load_geom(geom, P.src, total);
    aug_quad(rgb + g.off * 3, depth + g.off, label + g.off, g.H0, g.W0, P, hsv, n, y, x0, H, W, depth_mean, depth_std,
             raw_depth, image, depth_out, label_out);
}

}  // namespace dynmm

using namespace dynmm;

extern "C" int dynmm_rgbd_aug(const unsigned char* rgb, const unsigned short* depth, const unsigned char* label, int S, int H0,
                              int W0, const int* params, const float* hsv, int N, int H, int W, float depth_mean,
                              float depth_std, int raw_depth, float* image, float* depth_out, unsigned char* label_out,
                              unsigned char* down8, unsigned char* down16, unsigned char* down32, void* stream) {
    (void)hipGetLastError();
    if (!rgb || !depth || !label || !params || !image || !depth_out || !label_out || S < 1 || H0 < 1 || W0 < 1 || N < 1 ||
        H < 1 || W < 1)
        return DYNMM_EINVAL;
    if ((down8 || down16 || down32) && !(down8 && down16 && down32)) return DYNMM_EINVAL;
    // 4 consecutive x per thread, float4 / uchar4 stores; int4 parameter rows
    if (W % 4 != 0 || ((uintptr_t)image & 15u) || ((uintptr_t)depth_out & 15u) || ((uintptr_t)label_out & 3u) ||
        ((uintptr_t)params & 15u))
        return DYNMM_EUNSUPPORTED;
    const long long quads = (long long)N * H * (W / 4);
    long long down = 0;
    if (down8)
        for (int r = 8; r <= 32; r *= 2) down += (long long)N * (H / r) * (W / r);
    if (quads + down > (long long)INT32_MAX - 256) return DYNMM_EUNSUPPORTED;
    const int main_blocks = (int)((quads + 255) / 256), down_blocks = (int)((down + 255) / 256);
    hipLaunchKernelGGL(rgbd_aug_kernel, dim3(main_blocks + down_blocks), dim3(256), 0, (hipStream_t)stream, rgb, depth, label,
                       S, H0, W0, params, hsv, N, H, W, depth_mean, depth_std, raw_depth, image, depth_out, label_out, down8,
                       down16, down32, main_blocks);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_rgbd_aug_ragged(const unsigned char* rgb, const unsigned short* depth, const unsigned char* label,
                                     const long long* geom, long long total, int S, const int* params, const float* hsv, int N,
                                     int H, int W, float depth_mean, float depth_std, int raw_depth, float* image,
                                     float* depth_out, unsigned char* label_out, unsigned char* down8, unsigned char* down16,
                                     unsigned char* down32, void* stream) {
    (void)hipGetLastError();
    if (!rgb || !depth || !label || !geom || !params || !image || !depth_out || !label_out || total < 1 || S < 1 || N < 1 ||
        H < 1 || W < 1)
        return DYNMM_EINVAL;
    if ((down8 || down16 || down32) && !(down8 && down16 && down32)) return DYNMM_EINVAL;
    // as dynmm_rgbd_aug, plus the 16-byte loads of the geom rows
    if (W % 4 != 0 || ((uintptr_t)image & 15u) || ((uintptr_t)depth_out & 15u) || ((uintptr_t)label_out & 3u) ||
        ((uintptr_t)params & 15u) || ((uintptr_t)geom & 15u))
        return DYNMM_EUNSUPPORTED;
    const long long quads = (long long)N * H * (W / 4);
    long long down = 0;
    if (down8)
        for (int r = 8; r <= 32; r *= 2) down += (long long)N * (H / r) * (W / r);
    if (quads + down > (long long)INT32_MAX - 256) return DYNMM_EUNSUPPORTED;
    const int main_blocks = (int)((quads + 255) / 256), down_blocks = (int)((down + 255) / 256);
    hipLaunchKernelGGL(rgbd_aug_ragged_kernel, dim3(main_blocks + down_blocks), dim3(256), 0, (hipStream_t)stream, rgb, depth,
                       label, geom, total, S, params, hsv, N, H, W, depth_mean, depth_std, raw_depth, image, depth_out,
                       label_out, down8, down16, down32, main_blocks);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}
