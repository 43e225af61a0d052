// What the 3x3 / stride 2 / pad 1 max-pool kernels and the passes fused with them share (pointwise.hip: max-pool, stem fusion
// + pools; se_scale.hip: single-input SE scale + pool): the plane chunking of the element-wise passes, the tie rule, and the
// gather form of the pool's backward from the arg-max codes (code = r * 3 + s of the winning tap, row-major in the window).
#pragma once
#include <initializer_list>
#include "common.h"

namespace dynmm {

static inline int plane_chunks(int HW, int chunk) { return (HW + chunk - 1) / chunk; }
constexpr int kChunk = 8192;

// first maximum in row-major window order wins (strict >), NaN propagates
__device__ __forceinline__ void pool_update(float& best, int& bi, float val, int code) {
    if (bi < 0 || val > best || val != val) { best = val; bi = code; }
}

// Backward: a thread owns input rows 2a, 2a+1 x columns 8t .. 8t+7 = four 2x2 blocks; the block at pooled position
// (a, m) collects from the windows (a, m), (a, m+1), (a+1, m), (a+1, m+1) by their arg-max code:
//   (2a, 2m): code 4 of w(a,m)            (2a,   2m+1): 5 of w(a,m), 3 of w(a,m+1)
//   (2a+1, 2m): 7 of w(a,m), 1 of w(a+1,m)    (2a+1, 2m+1): 8 of w(a,m), 6 of w(a,m+1), 2 of w(a+1,m), 0 of w(a+1,m+1)
// i.e. 2 pooled rows x 5 pooled columns of (gradient, code), fetched as one 16-byte + one scalar load each.
// gradient of the 2 x 8 input pixels (rows 2a, 2a+1; columns 8t .. 8t+7) of one plane from the pooled gradient gp and
// the arg-max codes ip: top[] = row 2a, bot[] = row 2a+1
__device__ __forceinline__ void pool_bwd_block(const float* __restrict__ gp, const signed char* __restrict__ ip, int a,
                                               int t, int Ho, int Wo, float (&top)[8], float (&bot)[8]) {
    float gv[2][5];
    int cd[2][5];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const bool rok = a + rr < Ho;
        const size_t o = (size_t)(rok ? a + rr : a) * Wo + 4 * t;
        const float4 g4 = *reinterpret_cast<const float4*>(gp + o);
        const unsigned c4 = *reinterpret_cast<const unsigned*>(ip + o);
        const bool cok = 4 * t + 4 < Wo;
        const float g5 = cok ? gp[o + 4] : 0.f;
        const int c5 = cok ? (int)ip[o + 4] : -1;
        gv[rr][0] = g4.x; gv[rr][1] = g4.y; gv[rr][2] = g4.z; gv[rr][3] = g4.w; gv[rr][4] = g5;
#pragma unroll
        for (int j = 0; j < 4; ++j) cd[rr][j] = rok ? (int)(signed char)((c4 >> (8 * j)) & 0xffu) : -1;
        cd[rr][4] = rok ? c5 : -1;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const float g00 = gv[0][m], g01 = gv[0][m + 1], g10 = gv[1][m], g11 = gv[1][m + 1];
        const int c00 = cd[0][m], c01 = cd[0][m + 1], c10 = cd[1][m], c11 = cd[1][m + 1];
        top[2 * m] = c00 == 4 ? g00 : 0.f;
        top[2 * m + 1] = (c00 == 5 ? g00 : 0.f) + (c01 == 3 ? g01 : 0.f);
        bot[2 * m] = (c00 == 7 ? g00 : 0.f) + (c10 == 1 ? g10 : 0.f);
        bot[2 * m + 1] = ((c00 == 8 ? g00 : 0.f) + (c01 == 6 ? g01 : 0.f)) + ((c10 == 2 ? g10 : 0.f) + (c11 == 0 ? g11 : 0.f));
    }
}

// the fused pool kernels' geometry: even H, W % 8 == 0, 16-byte aligned maps, 4-byte aligned code planes
static inline bool pool_fusable(int H, int W, int Ho, int Wo, std::initializer_list<const void*> p16,
                                std::initializer_list<const void*> p4) {
    if (H % 2 != 0 || W % 8 != 0 || Ho != H / 2 || Wo != W / 2) return false;
    for (const void* p : p16) if (reinterpret_cast<uintptr_t>(p) & 15u) return false;
    for (const void* p : p4) if (reinterpret_cast<uintptr_t>(p) & 3u) return false;
    return true;
}

}  // namespace dynmm
