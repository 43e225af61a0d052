// Modality-level DynMM on CMU-MOSEI features (ModalityDynMM/affect/affect_dyn.py): the evaluation protocol of
// Supervised_Learning.single_test, task "posneg-classification" (training_structures/Supervised_Learning.py:252-347), and the
// validation loss of Supervised_Learning.train (:160-185), accumulated on the device over an evaluation pass.
//   * 2x2 counts of (out[:, 0] >= 0, y >= 0): the reference's `i[0] >= 0` / `true[i] >= 0` rule (>=, not >; a NaN output
//     counts as negative, as the comparison does in Python);
//   * its loss accumulator `totalloss += criterion(out, y) * len(batch)` in fp64.  With single_test's
//     L1Loss(reduction='sum') (affect_dyn.py:228,233) a batch adds B * sum|out - y| (the sum is multiplied by the batch size
//     once more: the reported "Loss" is that quirk divided by N); with train's validation objective (mean L1 + lossw *
//     the gate regulariser) it adds (sum|out - y| / B + lossw * aux) * B.
// One workgroup per launch, fixed-order reductions: no atomics, the same result on every run.  The launches of a pass are
// ordered by their stream, so the accumulation needs no host synchronisation per batch.
#include "common.h"

namespace dynmm {

__global__ void __launch_bounds__(256) posneg_counts_kernel(const float* __restrict__ out, int out_stride,
                                                            const float* __restrict__ y, int B, const float* __restrict__ aux,
                                                            double lossw, int form, long long* __restrict__ counts,
                                                            double* __restrict__ loss_acc) {
    __shared__ double dred[4];
    __shared__ int ired[4];
    int c[4] = {0, 0, 0, 0};
    double s = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float o = out[(size_t)b * out_stride];
        const float t = y[b];
        const int k = 2 * (o >= 0.f ? 1 : 0) + (t >= 0.f ? 1 : 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] += k == j ? 1 : 0;
        s += fabs((double)o - (double)t);
    }
    int tot[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) tot[j] = block_reduce_sum_256<int>(c[j], ired);
    const double sum = block_reduce_sum_256<double>(s, dred);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) counts[j] += tot[j];
        if (loss_acc) {
            const double nb = (double)B;
            loss_acc[0] += form == 0 ? nb * sum : (sum / nb + lossw * (aux ? (double)aux[0] : 0.0)) * nb;
        }
    }
}

}  // namespace dynmm

using namespace dynmm;

extern "C" int dynmm_posneg_counts(const float* out, int out_stride, const float* y, int B, const float* aux, double lossw,
                                   int form, long long* counts, double* loss_acc, void* stream) {
    (void)hipGetLastError();
    if (!out || !y || !counts || B < 1 || out_stride < 1 || (form != 0 && form != 1)) return DYNMM_EINVAL;
    hipLaunchKernelGGL(posneg_counts_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, out, out_stride, y, B, aux, lossw,
                       form, counts, loss_acc);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}
