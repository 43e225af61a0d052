// Objective of ONE expert trained on its own (modality-level DynMM, Step I: imdb_uni.py / imdb_mm.py / affect_uni.py /
// affect_mm.py): no gate, no regulariser, so nothing of the mixture heads (ml_head / moe_head) applies.
//   kind 0  BCEWithLogitsLoss():  l = max(x, 0) - x y + log1p(exp(-|x|))      (torch's stable form)
//           d l / d x = sigmoid(x) - y = (1 - y) sigmoid(x) - y sigmoid(-x)     (no cancellation for y in {0, 1})
//   kind 1  L1Loss():             l = |x - y|,  d l / d x = sign(x - y)          (0 at a tie, as torch)
// loss = mean over the B*C elements, d_out = dl/dx / (B*C).  One workgroup: each thread sums its elements in index order in
// double, the 256 sums meet in a fixed tree — the same bits on every run, no atomics.
#include "common.h"

using namespace dynmm;

namespace {

__global__ void __launch_bounds__(256) head_loss_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                        int n, int kind, float* __restrict__ loss,
                                                        float* __restrict__ d_out, double* __restrict__ loss_acc,
                                                        int rows) {
    __shared__ double red[4];
    const float fn = (float)n;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float x = out[i], y = target[i];
        float l, g;
        if (kind == DYNMM_LOSS_BCE_LOGITS) {
            const float e = expf(-fabsf(x));                     // in (0, 1]: never overflows
            const float r = 1.f / (1.f + e);
            const float sp = x >= 0.f ? r : e * r;               // sigmoid(x)
            const float sn = x >= 0.f ? e * r : r;               // sigmoid(-x)
            l = fmaxf(x, 0.f) - x * y + log1pf(e);
            g = (1.f - y) * sp - y * sn;
        } else {
            const float d = x - y;
            l = fabsf(d);
            g = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        }
        s += (double)l;
        if (d_out) d_out[i] = g / fn;
    }
    const double t = block_reduce_sum_256<double>(s, red);
    if (threadIdx.x == 0) {
        const double mean = t / (double)n;
        loss[0] = (float)mean;
        // Supervised_Learning.train's `totalloss += loss * len(batch)`: in stream order, one thread, so deterministic
        if (loss_acc) loss_acc[0] += (double)(float)mean * (double)rows;
    }
}

}  // namespace

extern "C" int dynmm_head_loss(const float* out, const float* target, int B, int C, int kind, float* loss, float* d_out,
                               double* loss_acc, void* stream) {
    (void)hipGetLastError();
    if (!out || !target || !loss || B < 1 || C < 1 || (long long)B * C > (1LL << 30) ||
        (kind != DYNMM_LOSS_BCE_LOGITS && kind != DYNMM_LOSS_L1))
        return DYNMM_EINVAL;
    hipLaunchKernelGGL(head_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, out, target, B * C, kind, loss, d_out,
                       loss_acc, B);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}
