// Modality-level DynMM on MM-IMDB features (ModalityDynMM/multimedia/imdb_dyn.py): the pieces of the experts and of the
// multilabel mixture head that are not GEMMs.  Every Linear runs on the 1x1 MFMA convolution (ops_seq.linear_bdt); this file adds
//   * MultiBench's Maxout -> BatchNorm1d -> Dropout as ONE kernel over the GEMM output z [B, 2m] (output [B, m]), forward and
//     backward; with MAXOUT = false the same kernel is the input BatchNorm1d (op0) of MaxOut_MLP,
//   * the multilabel mixture head: DiffSoftmax gate over K experts' [B, C] logits, blend, BCEWithLogitsLoss, gate
//     regulariser and the backward seeds, one launch; and the blend's own backward for arbitrary upstream gradients,
//   * per-class TP / FP / FN counts and the BCE sum of evaluation batches, accumulated on the device,
//   * the hard-gate partition: stable index lists of the samples each expert receives.
// Everything here is small and latency-bound next to the 4096 -> 2048 GEMM of the image encoder.
#include "common.h"
#include "dropout.h"

namespace dynmm {

// ---------------------------------------------------------------------------------------------------------------
// Maxout -> BatchNorm1d -> Dropout.  One workgroup owns 64 whole columns (lane = column, the 4 waves split the rows), so the
// batch statistics are reduced inside it in a fixed order: no atomics, deterministic.  Training: batch mean and biased
// variance over B normalise, the running statistics take momentum-weighted mean and UNBIASED variance (torch), and block 0
// advances num_batches_tracked.  Eval: running statistics.  mean / rstd of the normalisation are saved for the backward,
// which recomputes v = max(z[2j], z[2j+1]) (ties: the first column, as max(-1)) and regenerates the dropout decisions
// (flat index b * m + j of the [B, m] output).
// ---------------------------------------------------------------------------------------------------------------
constexpr int kMoCols = 64;

template <bool MAXOUT>
__device__ __forceinline__ float mo_load(const float* __restrict__ z, int b, int j, int M) {
    if (MAXOUT) {
        const float2 v = *reinterpret_cast<const float2*>(z + (size_t)b * 2 * M + 2 * j);
        return v.y > v.x ? v.y : v.x;
    }
    return z[(size_t)b * M + j];
}

// column sums of the four waves' partials: sh[w][lane] -> every lane of the workgroup receives its column's total
__device__ __forceinline__ float mo_colsum(float v, float (*sh)[kMoCols]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    sh[w][lane] = v;
    __syncthreads();
    return (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
}

template <bool MAXOUT>
__global__ void __launch_bounds__(256) mo_bn_fwd_kernel(const float* __restrict__ z, float* __restrict__ y,
                                                        float* __restrict__ save_mean, float* __restrict__ save_rstd,
                                                        float* __restrict__ run_mean, float* __restrict__ run_var,
                                                        long long* __restrict__ nbt, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int B, int M, float eps,
                                                        float momentum, int train, const DropSpec spec) {
    __shared__ float sh[4][kMoCols];
    const DropState ds(spec);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = blockIdx.x * kMoCols + lane;
    const bool on = j < M;
    float mean, rstd;
    if (train) {
        float s = 0.f;
        if (on)
            for (int b = w; b < B; b += 4) s += mo_load<MAXOUT>(z, b, j, M);
        mean = mo_colsum(s, sh) / (float)B;
        float q = 0.f;
        if (on)
            for (int b = w; b < B; b += 4) {
                const float d = mo_load<MAXOUT>(z, b, j, M) - mean;
                q += d * d;
            }
        const float var = mo_colsum(q, sh) / (float)B;
        rstd = 1.f / sqrtf(var + eps);
        if (on && w == 0) {
            if (run_mean) run_mean[j] = (1.f - momentum) * run_mean[j] + momentum * mean;
            if (run_var) run_var[j] = (1.f - momentum) * run_var[j] + momentum * (var * (float)B / (float)(B - 1));
        }
        if (nbt && blockIdx.x == 0 && threadIdx.x == 0) nbt[0] += 1;
    } else {
        mean = on ? run_mean[j] : 0.f;
        rstd = on ? 1.f / sqrtf(run_var[j] + eps) : 1.f;
    }
    if (!on) return;
    if (w == 0) {
        save_mean[j] = mean;
        save_rstd[j] = rstd;
    }
    const float g = gamma[j] * rstd, sft = beta[j] - mean * g;
    for (int b = w; b < B; b += 4) {
        const float v = mo_load<MAXOUT>(z, b, j, M) * g + sft;
        y[(size_t)b * M + j] = train ? v * ds((size_t)b * M + j) : v;
    }
}

// dy' = dy * keep; dgamma = sum dy' xhat, dbeta = sum dy' (written straight into the parameters' gradients);
// dv = gamma rstd (dy' - [train] (dbeta + xhat dgamma) / B), routed to the winning column of the pair (0 to the other).
template <bool MAXOUT>
__global__ void __launch_bounds__(256) mo_bn_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ z,
                                                        const float* __restrict__ mean_, const float* __restrict__ rstd_,
                                                        const float* __restrict__ gamma, float* __restrict__ dz,
                                                        float* __restrict__ dgamma, float* __restrict__ dbeta, int B, int M,
                                                        int train, const DropSpec spec) {
    __shared__ float sh[4][kMoCols];
    const DropState ds(spec);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = blockIdx.x * kMoCols + lane;
    const bool on = j < M;
    const float mean = on ? mean_[j] : 0.f, rstd = on ? rstd_[j] : 1.f;
    float sg = 0.f, sgx = 0.f;
    if (on)
        for (int b = w; b < B; b += 4) {
            const size_t o = (size_t)b * M + j;
            const float g = train ? dy[o] * ds(o) : dy[o];
            sg += g;
            sgx += g * (mo_load<MAXOUT>(z, b, j, M) - mean) * rstd;
        }
    sg = mo_colsum(sg, sh);
    sgx = mo_colsum(sgx, sh);
    if (!on) return;
    if (w == 0) {
        if (dgamma) dgamma[j] = sgx;
        if (dbeta) dbeta[j] = sg;
    }
    if (!dz) return;
    const float gr = gamma[j] * rstd;
    const float cg = train ? sg / (float)B : 0.f, cx = train ? sgx / (float)B : 0.f;
    for (int b = w; b < B; b += 4) {
        const size_t o = (size_t)b * M + j;
        const float g = train ? dy[o] * ds(o) : dy[o];
        if (MAXOUT) {
            const float2 zz = *reinterpret_cast<const float2*>(z + (size_t)b * 2 * M + 2 * j);
            const bool second = zz.y > zz.x;
            const float xh = ((second ? zz.y : zz.x) - mean) * rstd;
            const float dv = gr * (g - cg - xh * cx);
            *reinterpret_cast<float2*>(dz + (size_t)b * 2 * M + 2 * j) = second ? make_float2(0.f, dv) : make_float2(dv, 0.f);
        } else {
            const float xh = (z[o] - mean) * rstd;
            dz[o] = gr * (g - cg - xh * cx);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Multilabel mixture head (imdb_dyn.py:95-104 + Supervised_Learning.train with BCEWithLogitsLoss, one workgroup; a lane per
// sample):
//   w = DiffSoftmax(logits / temp, hard) ; out[b, c] = sum_k w[b, k] pred_k[b, c] ; aux = mean_b w[b, K-1]
//   loss = mean_{b,c} BCEWithLogits(out, y) (torch's stable form) ; total = loss + reg * aux
// Seeds of d total: d_pred_k = w_k (sigmoid(out) - y) / (B C) ; d_logits through the soft path (straight-through).
// ---------------------------------------------------------------------------------------------------------------
struct MlPreds { const float* p[4]; };
struct MlGrads { float* p[4]; };

__device__ __forceinline__ float bce_logits(float x, float y) {
    return fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
}
__device__ __forceinline__ float sigmoid_stable(float x) {
    if (x >= 0.f) return 1.f / (1.f + expf(-x));
    const float e = expf(x);
    return e / (1.f + e);
}

// softmax of logits[b] / temp -> z, the gate weights -> w (hard: one-hot of the first maximum, straight-through value)
__device__ __forceinline__ void ml_gate(const float* __restrict__ logits, int b, int K, float temp, int hard, float z[4],
                                        float w[4]) {
    float mx = -INFINITY;
    for (int k = 0; k < K; ++k) { z[k] = logits[(size_t)b * K + k] / temp; mx = fmaxf(mx, z[k]); }
    float den = 0.f;
    for (int k = 0; k < K; ++k) { z[k] = expf(z[k] - mx); den += z[k]; }
    int arg = 0;
    float best = -1.f;
    for (int k = 0; k < K; ++k) {
        z[k] /= den;
        if (z[k] > best) { best = z[k]; arg = k; }
    }
    for (int k = 0; k < K; ++k) w[k] = hard ? ((k == arg ? 1.f : 0.f) - z[k]) + z[k] : z[k];
}

__global__ void __launch_bounds__(256) ml_head_kernel(const float* __restrict__ logits, MlPreds P, int K, int C,
                                                      const float* __restrict__ target, float temp, int hard, float reg,
                                                      float* __restrict__ out, float* __restrict__ weight,
                                                      float* __restrict__ scalars /* loss, aux, total */, MlGrads dP,
                                                      float* __restrict__ d_logits, int B) {
    __shared__ float red[4];
    float ls = 0.f, aux = 0.f;
    const float invB = 1.f / (float)B, invBC = 1.f / ((float)B * (float)C);
    for (int b = threadIdx.x; b < B; b += 256) {
        float z[4], w[4], dw[4] = {0.f, 0.f, 0.f, 0.f};
        ml_gate(logits, b, K, temp, hard, z, w);
        for (int k = 0; k < K; ++k) weight[(size_t)b * K + k] = w[k];
        aux += w[K - 1];
        for (int c = 0; c < C; ++c) {
            const size_t o = (size_t)b * C + c;
            float v = 0.f;
            for (int k = 0; k < K; ++k) v += w[k] * P.p[k][o];
            out[o] = v;
            if (target) {
                const float y = target[o];
                ls += bce_logits(v, y);
                const float g = (sigmoid_stable(v) - y) * invBC;
                for (int k = 0; k < K; ++k) {
                    if (dP.p[k]) dP.p[k][o] = w[k] * g;
                    dw[k] += P.p[k][o] * g;
                }
            }
        }
        if (target && d_logits) {
            dw[K - 1] += reg * invB;
            float dot = 0.f;
            for (int k = 0; k < K; ++k) dot += z[k] * dw[k];
            for (int k = 0; k < K; ++k) d_logits[(size_t)b * K + k] = z[k] * (dw[k] - dot) / temp;
        }
    }
    const float tl = block_reduce_sum_256<float>(ls, red);
    const float ta = block_reduce_sum_256<float>(aux, red);
    if (threadIdx.x == 0) {
        const float loss = target ? tl * invBC : 0.f;
        scalars[0] = loss;
        scalars[1] = ta * invB;
        scalars[2] = loss + reg * ta * invB;
    }
}

//   d_pred_k = w_k d_out ; d_w_k = sum_c pred_k d_out + [k == K-1] d_aux / B ; d_logits through the soft path
__global__ void __launch_bounds__(256) ml_blend_bwd_kernel(const float* __restrict__ d_out, const float* __restrict__ d_aux,
                                                           const float* __restrict__ logits, MlPreds P, int K, int C,
                                                           const float* __restrict__ weight, float temp, MlGrads dP,
                                                           float* __restrict__ d_logits, int B) {
    const float da = d_aux ? d_aux[0] / (float)B : 0.f;
    for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256) {
        float z[4], w[4], dw[4] = {0.f, 0.f, 0.f, 0.f};
        ml_gate(logits, b, K, temp, 0, z, w);
        for (int k = 0; k < K; ++k) w[k] = weight[(size_t)b * K + k];
        for (int c = 0; c < C; ++c) {
            const size_t o = (size_t)b * C + c;
            const float g = d_out ? d_out[o] : 0.f;
            for (int k = 0; k < K; ++k) {
                if (dP.p[k]) dP.p[k][o] = w[k] * g;
                dw[k] += P.p[k][o] * g;
            }
        }
        dw[K - 1] += da;
        float dot = 0.f;
        for (int k = 0; k < K; ++k) dot += z[k] * dw[k];
        if (d_logits)
            for (int k = 0; k < K; ++k) d_logits[(size_t)b * K + k] = z[k] * (dw[k] - dot) / temp;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Multilabel evaluation counts (Supervised_Learning.test, task "multilabel"): pred = round(sigmoid(x)) in fp32 (0.5 rounds
// to 0, so a logit must exceed ~1.2e-7 to count), y = target > 0.5; counts [3, C] += (TP, FP, FN) per class, loss_sum[0] +=
// sum of BCEWithLogits over the batch (double).  One workgroup: integer LDS counters (order-independent) and one ordered
// double reduction, so repeated evaluations give identical sums.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kMlMaxC = 256;

__global__ void __launch_bounds__(256) ml_counts_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                        int B, int C, int* __restrict__ counts,
                                                        double* __restrict__ loss_sum) {
    __shared__ int cnt[3 * kMlMaxC];
    __shared__ double red[4];
    for (int i = threadIdx.x; i < 3 * C; i += 256) cnt[i] = 0;
    __syncthreads();
    double ls = 0.0;
    const size_t n = (size_t)B * C;
    for (size_t i = threadIdx.x; i < n; i += 256) {
        const int c = (int)(i % (size_t)C);
        const float x = logits[i];
        const float y = target[i];
        const float s = 1.f / (1.f + expf(-x));
        const bool pred = rintf(s) > 0.5f;
        const bool pos = y > 0.5f;
        if (pred && pos) atomicAdd(&cnt[c], 1);
        else if (pred) atomicAdd(&cnt[C + c], 1);
        else if (pos) atomicAdd(&cnt[2 * C + c], 1);
        ls += (double)bce_logits(x, y);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * C; i += 256) counts[i] += cnt[i];
    const double t = block_reduce_sum_256<double>(ls, red);
    if (loss_sum && threadIdx.x == 0) loss_sum[0] += t;
}

// ---------------------------------------------------------------------------------------------------------------
// Hard-gate partition: branch[b] = first arg-max of weight[b, 0..K-1]; order = the samples grouped by branch (ascending),
// stable; inv = its inverse; counts[k] = #samples of branch k.  One workgroup: a counting pass, then a ballot scan per
// 256-sample chunk.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ml_branch(const float* __restrict__ weight, int b, int K) {
    int arg = 0;
    float best = weight[(size_t)b * K];
    for (int k = 1; k < K; ++k) {
        const float v = weight[(size_t)b * K + k];
        if (v > best) { best = v; arg = k; }
    }
    return arg;
}

__global__ void __launch_bounds__(256) ml_partition_kernel(const float* __restrict__ weight, int K, int B,
                                                           int* __restrict__ order, int* __restrict__ inv,
                                                           int* __restrict__ counts) {
    __shared__ int tot[4];
    __shared__ int wsum[4][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x < 4) tot[threadIdx.x] = 0;
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += 256) atomicAdd(&tot[ml_branch(weight, b, K)], 1);
    __syncthreads();
    int base[4];
    int acc = 0;
    for (int k = 0; k < 4; ++k) {
        base[k] = acc;
        acc += k < K ? tot[k] : 0;
    }
    if (threadIdx.x < K) counts[threadIdx.x] = tot[threadIdx.x];
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int b = b0 + threadIdx.x;
        const int br = b < B ? ml_branch(weight, b, K) : -1;
        int pre = 0;
        __syncthreads();
        for (int k = 0; k < K; ++k) {
            const unsigned long long m = __ballot(br == k);
            if (br == k) pre = __popcll(m & below);
            if (lane == 0) wsum[k][w] = __popcll(m);
        }
        __syncthreads();
        if (br >= 0) {
            int pos = base[br] + pre;
            for (int v = 0; v < w; ++v) pos += wsum[br][v];
            order[pos] = b;
            inv[b] = pos;
        }
        __syncthreads();
        for (int k = 0; k < K; ++k) base[k] += wsum[k][0] + wsum[k][1] + wsum[k][2] + wsum[k][3];
    }
}

}  // namespace dynmm

using namespace dynmm;

#define ST ((hipStream_t)stream)

extern "C" int dynmm_maxout_bn_fwd(const float* z, float* y, float* save_mean, float* save_rstd, float* running_mean,
                                   float* running_var, long long* num_batches_tracked, const float* gamma, const float* beta,
                                   int B, int M, int maxout, float eps, float momentum, int train, const dynmm_dropout* drop,
                                   void* stream) {
    (void)hipGetLastError();
    if (!z || !y || !save_mean || !save_rstd || !gamma || !beta || B <= 0 || M <= 0) return DYNMM_EINVAL;
    if (train && B < 2) return DYNMM_EINVAL;                       // torch: "Expected more than 1 value per channel"
    if (!train && (!running_mean || !running_var)) return DYNMM_EINVAL;
    if (drop && !(drop->p >= 0.f && drop->p < 1.f)) return DYNMM_EINVAL;
    if (maxout && (((uintptr_t)z) & 7)) return DYNMM_EINVAL;
    const dim3 grid(ceil_div(M, kMoCols));
    const DropSpec spec = drop_spec(train ? drop : nullptr);
    if (maxout)
        hipLaunchKernelGGL(mo_bn_fwd_kernel<true>, grid, dim3(256), 0, ST, z, y, save_mean, save_rstd, running_mean, running_var,
                           num_batches_tracked, gamma, beta, B, M, eps, momentum, train, spec);
    else
        hipLaunchKernelGGL(mo_bn_fwd_kernel<false>, grid, dim3(256), 0, ST, z, y, save_mean, save_rstd, running_mean,
                           running_var, num_batches_tracked, gamma, beta, B, M, eps, momentum, train, spec);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_maxout_bn_bwd(const float* dy, const float* z, const float* save_mean, const float* save_rstd,
                                   const float* gamma, float* dz, float* dgamma, float* dbeta, int B, int M, int maxout,
                                   int train, const dynmm_dropout* drop, void* stream) {
    (void)hipGetLastError();
    if (!dy || !z || !save_mean || !save_rstd || !gamma || B <= 0 || M <= 0) return DYNMM_EINVAL;
    if (drop && !(drop->p >= 0.f && drop->p < 1.f)) return DYNMM_EINVAL;
    if (maxout && ((((uintptr_t)z) & 7) || (((uintptr_t)dz) & 7))) return DYNMM_EINVAL;
    const dim3 grid(ceil_div(M, kMoCols));
    const DropSpec spec = drop_spec(train ? drop : nullptr);
    if (maxout)
        hipLaunchKernelGGL(mo_bn_bwd_kernel<true>, grid, dim3(256), 0, ST, dy, z, save_mean, save_rstd, gamma, dz, dgamma, dbeta,
                           B, M, train, spec);
    else
        hipLaunchKernelGGL(mo_bn_bwd_kernel<false>, grid, dim3(256), 0, ST, dy, z, save_mean, save_rstd, gamma, dz, dgamma,
                           dbeta, B, M, train, spec);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_ml_head(const float* logits, const float* const* preds, int K, int C, const float* target, float temp,
                             int hard, float reg, float* out, float* weight, float* scalars, float* const* d_preds,
                             float* d_logits, int B, void* stream) {
    (void)hipGetLastError();
    if (!logits || K < 1 || K > 4 || C < 1 || B < 1 || !weight || !scalars || !(temp != 0.f) || (preds && !out))
        return DYNMM_EINVAL;
    MlPreds P{};
    MlGrads G{};
    for (int k = 0; preds && k < K; ++k) {
        if (!preds[k]) return DYNMM_EINVAL;
        P.p[k] = preds[k];
        G.p[k] = d_preds ? d_preds[k] : nullptr;
    }
    if (!preds) target = nullptr;                                   // the gate alone: weight and aux
    hipLaunchKernelGGL(ml_head_kernel, dim3(1), dim3(256), 0, ST, logits, P, K, preds ? C : 0, target, temp, hard, reg, out,
                       weight, scalars, G, target ? d_logits : nullptr, B);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_ml_blend_bwd(const float* d_out, const float* d_aux, const float* logits, const float* const* preds,
                                  int K, int C, const float* weight, float temp, float* const* d_preds, float* d_logits, int B,
                                  void* stream) {
    (void)hipGetLastError();
    if (!logits || !preds || !weight || K < 1 || K > 4 || C < 1 || B < 1 || !(temp != 0.f)) return DYNMM_EINVAL;
    MlPreds P{};
    MlGrads G{};
    for (int k = 0; k < K; ++k) {
        if (!preds[k]) return DYNMM_EINVAL;
        P.p[k] = preds[k];
        G.p[k] = d_preds ? d_preds[k] : nullptr;
    }
    hipLaunchKernelGGL(ml_blend_bwd_kernel, dim3(ceil_div(B, 256)), dim3(256), 0, ST, d_out, d_aux, logits, P, K, C, weight,
                       temp, G, d_logits, B);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_ml_counts(const float* logits, const float* target, int B, int C, int* counts, double* loss_sum,
                               void* stream) {
    (void)hipGetLastError();
    if (!logits || !target || !counts || B < 1 || C < 1 || C > kMlMaxC) return DYNMM_EINVAL;
    hipLaunchKernelGGL(ml_counts_kernel, dim3(1), dim3(256), 0, ST, logits, target, B, C, counts, loss_sum);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_ml_partition(const float* weight, int K, int B, int* order, int* inv, int* counts, void* stream) {
    (void)hipGetLastError();
    if (!weight || !order || !inv || !counts || K < 1 || K > 4 || B < 1) return DYNMM_EINVAL;
    hipLaunchKernelGGL(ml_partition_kernel, dim3(1), dim3(256), 0, ST, weight, K, B, order, inv, counts);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}
