// Multi-head self-attention for head dimensions up to 64 on the fp32 matrix cores (v_mfma_f32_16x16x4_f32, exact fp32): the
// attention core of nn.TransformerEncoderLayer(d_model = 300, nhead = 5) (dh = 60), which the register-resident kernels of
// seq.hip (a whole query row and a key row per lane) cannot hold beyond dh = 32.  Same tensors as mha_fwd_kernel / mha_bwd_kernel:
//   qkv [B, 3D, T] (q | k | v along channels), out [B, D, T], probs [B*heads, T, T] (BEFORE dropout), dqkv [B, 3D, T],
//   P = softmax_j((q_i / sqrt(dh)) . k_j),  out[c][i] = sum_j P'[i][j] v[c][j],  P' = P * keep / (1 - p).
// 1 <= dh <= 64, 1 <= T <= 64.  DESIGN.md section 7l.
//
// Tiling.  One workgroup of four waves per (sample, head); wave w owns the 16 QUERIES 16 w .. 16 w + 15 (waves whose tile lies
// past T leave after the staging barrier).  The operands sit in LDS TOKEN-major, [token][LD] with LD = DH + 4 (DH = the compiled
// bound on dh): both operand shapes of the instruction are then conflict-free 4-byte reads,
//   * token = lane & 15, channel = 4 s + (lane >> 4)   (k = channels: scores, dP)   bank = 4 (lane & 15) + (lane >> 4)
//   * token = 4 (lane >> 4) + r, channel = lane & 15   (k = tokens: P'V, dQ, dK, dV) bank = 16 (lane >> 4) + (lane & 15)
// because LD = 4 (mod 16) for DH = 32 and 64.  Channels dh .. DH - 1 and tokens T .. 16 ceil(T / 16) - 1 are staged as zeros
// (unconditional loads on clamped addresses, the value masked afterwards: see seq.hip on `ok ? p[i] : 0`), so the unrolled tile
// loops carry no predicates; only the stores are bounded.
//
// The score tile is computed TRANSPOSED (rows = keys, columns = queries): the C/D layout (row = 4 (lane >> 4) + register, column
// = lane & 15) then leaves lane (i = lane & 15, g = lane >> 4) with keys 16 jt + 4 g + r of query i in register r of tile jt:
//   * a query's 64 scores are 16 registers of 4 lanes: maximum, denominator and the backward's sum_j P dP are register sums and two
//     lane exchanges (xor 16, 32) — no LDS, no barrier;
//   * register r is at once a valid B operand (k = lane >> 4, column = lane & 15) of the next product, whose k-steps walk the keys
//     in the order {4 g + r}: out^T[c][i] = sum_j V^T[c][j] P'^T[j][i] and dQ^T = K^T dS^T take P' and dS straight from the
//     accumulators, and their results have the queries along the lanes — 64-byte runs of out / dqkv.
// Only dK and dV, sums over the QUERIES, cross the waves: dS and P' go to LDS as [query][key], and after one barrier wave w owns
// the 16 KEYS of tile w.
//
// Dropout.  The keep decisions are read through DropState::row8 with seq.hip's indexing (row = flat query row, 8-key chunk), so
// injected flags are the flat [B*heads, T, T] bytes and the generator draws what mha_fwd_kernel draws.  A query's eight chunks are
// drawn ONCE, two by each of its four lanes (chunks g and g + 4; a Philox call is ~900 issue cycles), kept as bits and exchanged
// with one lane read per tile.
#include "attn_tile.h"

namespace dynmm {

constexpr int kAttnMaxT = 64;
constexpr int kAttnMaxDh = 64;

template <int DH>
__global__ void __launch_bounds__(256) attn_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                       float* __restrict__ probs, int D, int T, int H, const DropSpec spec) {
    constexpr int KS = AttnShape<DH>::KS, CT = AttnShape<DH>::CT, LD = AttnShape<DH>::LD;
    extern __shared__ __align__(16) float smem[];
    const int nt = (T + 15) >> 4, rows = 16 * nt;
    float* qs = smem;                    // [rows][LD], scaled by 1 / sqrt(dh) (torch scales q before q @ k^T)
    float* ks = qs + rows * LD;          // [rows][LD]
    float* vs = ks + rows * LD;          // [rows][LD]
    const DropState drop(spec);
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const int dh = D / H;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 15, g = lane >> 4;
    const float* base = qkv + ((size_t)b * 3 * D + (size_t)h * dh) * T;
    if (w < nt) {
        float rq[KS], rk[KS], rv[KS];
        attn_load<DH>(base, rq, dh, T, 0, w, lane);
        attn_load<DH>(base + (size_t)D * T, rk, dh, T, 0, w, lane);
        attn_load<DH>(base + (size_t)2 * D * T, rv, dh, T, 0, w, lane);
        attn_store<DH>(qs, rq, dh, T, 0, w, lane, rsqrtf((float)dh));
        attn_store<DH>(ks, rk, dh, T, 0, w, lane, 1.f);
        attn_store<DH>(vs, rv, dh, T, 0, w, lane, 1.f);
    }
    __syncthreads();
    if (w >= nt) return;
    const int i = 16 * w + li;                                   // this lane's query
    const size_t row = (size_t)blockIdx.x * T + min(i, T - 1);   // probs (and their keep flags) are [B*H][T][T]
    const bool dropping = drop.p > 0.f;
    const unsigned bits = dropping ? attn_draw(drop, row, T, g) : 0u;

    // S^T[j][i] = sum_c K[j][c] Q[i][c]: four key tiles side by side (independent accumulators cover the 40-cycle latency)
    f32x4 s[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) s[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KS; ++k) {
        const float qv = qs[i * LD + 4 * k + g];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
            if (jt < nt) s[jt] = mfma_16x16x4(ks[(16 * jt + li) * LD + 4 * k + g], qv, s[jt]);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[jt][r] = 16 * jt + 4 * g + r < T ? s[jt][r] : -INFINITY;        // (tiles past nt: all -inf, exp = 0)
            mx = fmaxf(mx, s[jt][r]);
        }
    mx = attn_query_max(mx);
    float den = 0.f;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[jt][r] = expf(s[jt][r] - mx);
            den += s[jt][r];
        }
    const float inv = 1.f / attn_query_sum(den);
    float* pg = probs + row * T;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
        const unsigned k4 = dropping ? attn_keep4(bits, jt, lane) : 0xfu;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = 16 * jt + 4 * g + r;
            const float p = s[jt][r] * inv;
            if (i < T && j < T) pg[j] = p;                       // saved for the backward: the probabilities BEFORE dropout
            s[jt][r] = ((k4 >> r) & 1u) ? p * drop.inv : 0.f;
        }
    }
    // out^T[c][i] = sum_j V[j][c] P'[i][j]: k-step (jt, r) = keys 16 jt + 4 g + r, P' straight from the accumulators
    f32x4 o[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) o[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
        if (jt < nt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* vr = vs + (16 * jt + 4 * g + r) * LD + li;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) o[ct] = mfma_16x16x4(vr[16 * ct], s[jt][r], o[ct]);
            }
        }
    float* ob = out + ((size_t)b * D + (size_t)h * dh) * T;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = 16 * ct + 4 * g + r;
            if (c < dh && i < T) ob[(size_t)c * T + i] = o[ct][r];
        }
}

template <int DH>
__global__ void __launch_bounds__(256) attn_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ qkv,
                                                       const float* __restrict__ probs, float* __restrict__ dqkv, int D, int T,
                                                       int H, const DropSpec spec) {
    constexpr int KS = AttnShape<DH>::KS, CT = AttnShape<DH>::CT, LD = AttnShape<DH>::LD;
    constexpr int LP = 68;                                       // [query][key] tiles: 4 (mod 16) as LD
    extern __shared__ __align__(16) float smem[];
    const int nt = (T + 15) >> 4, rows = 16 * nt;
    float* qs = smem;                    // [rows][LD] each; q UNscaled
    float* ks = qs + rows * LD;
    float* vs = ks + rows * LD;
    float* gs = vs + rows * LD;          // dOut
    float* dss = gs + rows * LD;         // [rows][LP]  dS
    float* pps = dss + rows * LP;        // [rows][LP]  P'
    const DropState drop(spec);
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const int dh = D / H;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 15, g = lane >> 4;
    const float* base = qkv + ((size_t)b * 3 * D + (size_t)h * dh) * T;
    if (w < nt) {
        float rq[KS], rk[KS], rv[KS], rg[KS];
        attn_load<DH>(base, rq, dh, T, 0, w, lane);
        attn_load<DH>(base + (size_t)D * T, rk, dh, T, 0, w, lane);
        attn_load<DH>(base + (size_t)2 * D * T, rv, dh, T, 0, w, lane);
        attn_load<DH>(gout + ((size_t)b * D + (size_t)h * dh) * T, rg, dh, T, 0, w, lane);
        attn_store<DH>(qs, rq, dh, T, 0, w, lane, 1.f);
        attn_store<DH>(ks, rk, dh, T, 0, w, lane, 1.f);
        attn_store<DH>(vs, rv, dh, T, 0, w, lane, 1.f);
        attn_store<DH>(gs, rg, dh, T, 0, w, lane, 1.f);
    }
    __syncthreads();
    const bool live = w < nt;                                    // (waves past T idle until the second barrier)
    const int i = 16 * w + li;
    const float scale = rsqrtf((float)dh);
    if (live) {
        const size_t row = (size_t)blockIdx.x * T + min(i, T - 1);
        const bool dropping = drop.p > 0.f;
        const unsigned bits = dropping ? attn_draw(drop, row, T, g) : 0u;
        // P of this lane's query, keys 16 jt + 4 g + r (clamped addresses, zeros outside T x T)
        f32x4 p[4], pk[4], d[4];
        const float* pg = probs + row * T;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 16 * jt + 4 * g + r;
                p[jt][r] = attn_keep_if(pg[min(j, T - 1)], i < T && j < T);
            }
        // dP'^T[j][i] = sum_c V[j][c] dOut[i][c]
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) d[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const float gv = gs[i * LD + 4 * k + g];
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
                if (jt < nt) d[jt] = mfma_16x16x4(vs[(16 * jt + li) * LD + 4 * k + g], gv, d[jt]);
        }
        // dP = dP' * keep / (1 - p);  P' = P * keep / (1 - p);  dS = P (dP - sum_j P dP)
        float dot = 0.f;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            const unsigned k4 = dropping ? attn_keep4(bits, jt, lane) : 0xfu;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float kf = ((k4 >> r) & 1u) ? drop.inv : 0.f;
                d[jt][r] *= kf;
                pk[jt][r] = p[jt][r] * kf;
                dot += p[jt][r] * d[jt][r];
            }
        }
        dot = attn_query_sum(dot);
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = i * LP + 16 * jt + 4 * g + r;
                d[jt][r] = p[jt][r] * (d[jt][r] - dot);
                dss[o] = d[jt][r];
                pps[o] = pk[jt][r];
            }
        // dQ^T[c][i] = scale sum_j K[j][c] dS[i][j]: dS straight from the registers
        f32x4 a[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) a[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
            if (jt < nt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float* kr = ks + (16 * jt + 4 * g + r) * LD + li;
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) a[ct] = mfma_16x16x4(kr[16 * ct], d[jt][r], a[ct]);
                }
            }
        float* dq = dqkv + ((size_t)b * 3 * D + (size_t)h * dh) * T;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 16 * ct + 4 * g + r;
                if (c < dh && i < T) dq[(size_t)c * T + i] = a[ct][r] * scale;
            }
    }
    __syncthreads();
    if (!live) return;
    // wave w now owns KEYS 16 w + li:  dK^T[c][j] = scale sum_i Q[i][c] dS[i][j],  dV^T[c][j] = sum_i dOut[i][c] P'[i][j]
    f32x4 ak[CT], av[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) ak[ct] = av[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < nt; ++it) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = 16 * it + 4 * g + r;
            const float dsv = dss[q * LP + i], ppv = pps[q * LP + i];
            const float* qr = qs + q * LD + li;
            const float* gr = gs + q * LD + li;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                ak[ct] = mfma_16x16x4(qr[16 * ct], dsv, ak[ct]);
                av[ct] = mfma_16x16x4(gr[16 * ct], ppv, av[ct]);
            }
        }
    }
    float* dk = dqkv + ((size_t)b * 3 * D + (size_t)D + (size_t)h * dh) * T;
    float* dv = dk + (size_t)D * T;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = 16 * ct + 4 * g + r;
            if (c < dh && i < T) {
                dk[(size_t)c * T + i] = ak[ct][r] * scale;
                dv[(size_t)c * T + i] = av[ct][r];
            }
        }
}

}  // namespace dynmm

using namespace dynmm;

#define ST ((hipStream_t)stream)

template <int DH, bool BWD>
static int launch_attn(const float* g, const float* qkv, float* out_or_dqkv, float* probs, int B, int D, int T, int heads,
                       const DropSpec& spec, hipStream_t st) {
    const size_t rows = (size_t)16 * ceil_div(T, 16);
    const size_t lds = (BWD ? 4 * rows * (DH + 4) + 2 * rows * 68 : 3 * rows * (DH + 4)) * sizeof(float);
    static size_t attr_done = 64 * 1024;                      // the runtime's default bound on dynamic LDS
    if (lds > attr_done) {
        const void* fn = BWD ? reinterpret_cast<const void*>(&attn_bwd_kernel<DH>) : reinterpret_cast<const void*>(&attn_fwd_kernel<DH>);
        DYNMM_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_done = lds;
    }
    if (BWD)
        hipLaunchKernelGGL((attn_bwd_kernel<DH>), dim3(B * heads), dim3(256), lds, st, g, qkv, (const float*)probs, out_or_dqkv, D,
                           T, heads, spec);
    else
        hipLaunchKernelGGL((attn_fwd_kernel<DH>), dim3(B * heads), dim3(256), lds, st, qkv, out_or_dqkv, probs, D, T, heads, spec);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_attn_supported(int D, int T, int heads) {
    return D > 0 && T > 0 && heads > 0 && D % heads == 0 && T <= kAttnMaxT && D / heads <= kAttnMaxDh;
}

extern "C" int dynmm_attn_fwd(const float* qkv, float* out, float* probs, int B, int D, int T, int heads,
                              const dynmm_dropout* drop, void* stream) {
    (void)hipGetLastError();
    if (!qkv || !out || !probs || B <= 0 || D <= 0 || T <= 0 || heads <= 0 || D % heads != 0 || !drop_ok(drop)) return DYNMM_EINVAL;
    if (!dynmm_attn_supported(D, T, heads)) return DYNMM_EUNSUPPORTED;
    if (D / heads <= 32) return launch_attn<32, false>(nullptr, qkv, out, probs, B, D, T, heads, drop_spec(drop), ST);
    return launch_attn<64, false>(nullptr, qkv, out, probs, B, D, T, heads, drop_spec(drop), ST);
}

extern "C" int dynmm_attn_bwd(const float* g, const float* qkv, const float* probs, float* dqkv, int B, int D, int T, int heads,
                              const dynmm_dropout* drop, void* stream) {
    (void)hipGetLastError();
    if (!g || !qkv || !probs || !dqkv || B <= 0 || D <= 0 || T <= 0 || heads <= 0 || D % heads != 0 || !drop_ok(drop)) return DYNMM_EINVAL;
    if (!dynmm_attn_supported(D, T, heads)) return DYNMM_EUNSUPPORTED;
    if (D / heads <= 32) return launch_attn<32, true>(g, qkv, dqkv, const_cast<float*>(probs), B, D, T, heads, drop_spec(drop), ST);
    return launch_attn<64, true>(g, qkv, dqkv, const_cast<float*>(probs), B, D, T, heads, drop_spec(drop), ST);
}
