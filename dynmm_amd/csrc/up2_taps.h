// The pre-summed taps of the learned 2x up-sampling (model.py:404-410), shared by the kernels that fuse it with what follows:
// the training tail (tail.hip: up-sampling + cross entropy) and the inference tail (segment.hip: two up-samplings + arg-max).
// Nearest-2x followed by a 3x3 collapses to a 2x2 window of the INPUT (tail.hip has the derivation).
#pragma once
#include "common.h"

namespace dynmm {

constexpr int kTailMaxC = 64;
constexpr int kCoefLd = 20;       // 16 pre-summed taps + bias, rows padded to 16 bytes (ds_read_b128 broadcasts)

// coef[c][tail_ci(ar, wr, ac, wc)] (16 per channel) + bias: built once per workgroup in LDS.  The two column parities of a tap
// sit next to each other, ac = 1 first: frame outputs 2k (ac = 1) and 2k + 1 (ac = 0) read the SAME 2x2 input window, so their
// logits and their contributions to dx are ONE packed operation each (v_pk_fma_f32: two fp32 FMAs per lane and issue slot) with
// an 8-byte LDS read of the coefficient pair (round 6; the backward is bound by its vector issue slots).
__device__ __forceinline__ constexpr int tail_ci(int ar, int wr, int ac, int wc) { return ((ar * 2 + wr) * 2 + wc) * 2 + (1 - ac); }
__device__ __forceinline__ void tail_build_coef(const float* __restrict__ wgt, const float* __restrict__ bias,
                                                float (*coef)[kCoefLd], int C) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float k[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) k[j] = wgt[c * 9 + j];
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
                        coef[c][tail_ci(ar, wr, ac, wc)] = s;
                    }
        coef[c][16] = bias ? bias[c] : 0.f;
    }
    __syncthreads();
}

}  // namespace dynmm
