// MULT (MultiBench fusions.mult.MULTModel, affect_mm.py --fusion 4): what its pre-norm cross-modal transformers need beside the
// GEMMs (every Linear / Conv1d(k=1) stays a 1x1 convolution on the implicit-GEMM kernels):
//   * masked cross-modal attention with separate query and key lengths, forward + backward (dynmm_xattn_*),
//   * the embedding dropout(scale x + pos(x)) with the padding rule, one or two dropout sites per launch (dynmm_posembed_*).
// The pre-norm layer's `r + dropout(x)` fused with the LayerNorm that follows it (dynmm_prenorm_*) runs on seq.hip's LayerNorm
// kernels.  DESIGN.md section 7m.
#include "attn_tile.h"

namespace dynmm {

constexpr int kXaMaxT = 64;
constexpr int kXaMaxDh = 32;

// q . k as an unevaluated sum hi + lo of two floats (TwoProd / TwoSum, Ogita-Rump-Oishi Dot2: fp32 operations only, about twice
// the working precision).  A score of magnitude 1e3 rounded to one float carries 6e-5 into the exponent, and the few rows whose two
// largest scores nearly tie then decide the error of the whole gradient; the difference to the row maximum taken on (hi, lo) is
// exact to ~1e-7 of itself, whatever the scores' magnitude.
template <int DH>
__device__ __forceinline__ void xa_dot2(const float q[DH], const float k[DH], float& hi, float& lo) {
    float p = 0.f, s = 0.f;
#pragma unroll
    for (int c = 0; c < DH; ++c) {
        const float h = __fmul_rn(q[c], k[c]);
        const float r = fmaf(q[c], k[c], -h);                        // the product's rounding error, exactly
        const float x = __fadd_rn(p, h);
        const float z = __fsub_rn(x, p);
        const float y = __fadd_rn(__fsub_rn(p, __fsub_rn(x, z)), __fsub_rn(h, z));      // the sum's rounding error, exactly
        p = x;
        s = __fadd_rn(s, __fadd_rn(y, r));
    }
    hi = p;
    lo = s;
}

// ---------------------------------------------------------------------------------------------------------------
// Cross attention.  q [B, D, Tq], k / v [B, D, Tk] (channel stride = the sequence length, batch strides free), heads H,
// dh = D / H:  P = softmax_j((q_i . k_j) / sqrt(dh) + mask),  out[c][i] = sum_j P'[i][j] v[c][j],  P' = dropout(P).
// causal: key j is visible to query i iff j <= i + |Tk - Tq| (torch.triu(-inf, 1 + |Tk - Tq|)); key 0 is always visible.
// One wave per (sample, head): lane i owns query i (forward; dS and dq in the backward) and key i (dk, dv).  K and V sit in
// LDS token-major ([Tk][DH], a row is read by every lane at one address: a broadcast of 16-byte reads), the [Tq][Tk|1]
// probability tile is read as conflict-free rows and columns.  A lane's key loop ends at its own last visible key, so the
// causal mask removes the masked half of the work instead of computing and discarding it.  With one wave per workgroup no
// reduction crosses waves, LDS is sized for the launch's lengths (12 KB at dh = 4, T = 50), and at B = 32, H = 10 the grid
// is 320 independent waves.  DH = compile-time bound on dh (channels dh .. DH-1 are zero-filled unless EXACT).
// ---------------------------------------------------------------------------------------------------------------
template <int DH, bool EXACT>
__global__ void __launch_bounds__(64) xattn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                       const float* __restrict__ v, size_t sq, size_t sk, size_t sv,
                                                       float* __restrict__ out, float* __restrict__ probs, int D, int Tq,
                                                       int Tk, int H, int causal, float scale, const DropSpec spec) {
    extern __shared__ __align__(16) float smem[];
    const int ld = Tk | 1;
    float* ks = smem;                    // [Tk][DH]
    float* vs = ks + Tk * DH;            // [Tk][DH]
    float* ps = vs + Tk * DH;            // [Tq][ld]  exp
    float* invs = ps + Tq * ld;          // [64]
    const DropState drop(spec);
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const int dh = D / H;
    const int i = threadIdx.x;
    const bool actq = i < Tq, actk = i < Tk;
    // (unconditional loads on clamped indices, values selected afterwards)
    const int iq = min(i, Tq - 1), ik = min(i, Tk - 1);
    const float* qb = q + (size_t)b * sq + (size_t)h * dh * Tq;
    const float* kb = k + (size_t)b * sk + (size_t)h * dh * Tk;
    const float* vb = v + (size_t)b * sv + (size_t)h * dh * Tk;
    float qr[DH];
#pragma unroll
    for (int c = 0; c < DH; ++c) {
        const int cc = EXACT ? c : min(c, dh - 1);
        const float t = qb[(size_t)cc * Tq + iq];
        const float kv = kb[(size_t)cc * Tk + ik];
        const float vv = vb[(size_t)cc * Tk + ik];
        const bool in = EXACT || c < dh;
        qr[c] = (in && actq) ? t : 0.f;
        if (actk) {
            ks[i * DH + c] = in ? kv : 0.f;
            vs[i * DH + c] = in ? vv : 0.f;
        }
    }
    __syncthreads();
    const int off = Tk > Tq ? Tk - Tq : Tq - Tk;
    const int jmax = actq ? (causal ? attn_visible(i, off, Tk) : Tk) : 0;    // keys 0 .. jmax-1 are visible to query i
    const size_t row = (size_t)blockIdx.x * Tq + i;                  // probs and their keep flags are [B*H][Tq][Tk]
    float* pr = ps + iq * ld;
    // pass 1: the row maximum of the raw scores, as (hi, lo); the scores are recomputed in pass 2 instead of stored
    float mxh = -INFINITY, mxl = 0.f;
    for (int j = 0; j < jmax; ++j) {
        float kr[DH], hi, lo;
        row_ld<DH>(ks + j * DH, kr);
        xa_dot2<DH>(qr, kr, hi, lo);
        if (hi > mxh) {
            mxh = hi;
            mxl = lo;
        }
    }
    float den = 0.f;
    float o[DH];
#pragma unroll
    for (int c = 0; c < DH; ++c) o[c] = 0.f;
    for (int j0 = 0; j0 < jmax; j0 += 8) {
        float kp[8];
        drop.row8(row, j0 >> 3, Tk, kp);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = j0 + e;
            if (j < jmax) {
                float kr[DH], hi, lo;
                row_ld<DH>(ks + j * DH, kr);
                xa_dot2<DH>(qr, kr, hi, lo);
                // (q . k_j - max) / sqrt(dh): the difference first, then the scale (torch scales q; the same function)
                const float ex = expf(((hi - mxh) + (lo - mxl)) * scale);
                pr[j] = ex;
                den += ex;
                const float w = ex * kp[e];                          // dropout acts on the normalised probabilities: linear in ex
                float vr[DH];
                row_ld<DH>(vs + j * DH, vr);
#pragma unroll
                for (int c = 0; c < DH; ++c) o[c] += w * vr[c];
            }
        }
    }
    if (actq)
        for (int j = jmax; j < Tk; ++j) pr[j] = 0.f;                 // masked entries are saved as exact zeros
    const float inv = actq ? 1.f / den : 0.f;
    invs[i] = inv;
    if (actq) {
        float* ob = out + ((size_t)b * D + (size_t)h * dh) * Tq;
#pragma unroll
        for (int c = 0; c < DH; ++c)
            if (EXACT || c < dh) ob[(size_t)c * Tq + i] = o[c] * inv;
    }
    __syncthreads();
    // saved for the backward: the probabilities BEFORE dropout, coalesced
    float* pg = probs + (size_t)blockIdx.x * Tq * Tk;
    for (int r = 0; r < Tq; ++r)
        if (i < Tk) pg[(size_t)r * Tk + i] = ps[r * ld + i] * invs[r];
}

// Phase A (lane = query i): dP'[i][j] = sum_c g[c][i] v[c][j], dP = dP' keep, dS = P (dP - sum_j P dP), dq_i = sum_j dS k_j.
// Phase B (lane = key j): dk_j = sum_i dS[i][j] q_i, dv_j = sum_i P'[i][j] g_i over the queries that see key j; the Q and dOut
// tiles take the LDS of K and V, which phase A is done with.
template <int DH, bool EXACT>
__global__ void __launch_bounds__(64) xattn_bwd_kernel(const float* __restrict__ g, const float* __restrict__ q,
                                                       const float* __restrict__ k, const float* __restrict__ v, size_t sq,
                                                       size_t sk, size_t sv, const float* __restrict__ probs,
                                                       float* __restrict__ dq, float* __restrict__ dk, float* __restrict__ dv,
                                                       size_t sdq, size_t sdk, size_t sdv, int D, int Tq, int Tk, int H,
                                                       int causal, float scale, const DropSpec spec) {
    extern __shared__ __align__(16) float smem[];
    const int ld = Tk | 1;
    const int Tm = max(Tq, Tk);
    float* as = smem;                    // [Tm][DH]  K, then Q
    float* bs = as + Tm * DH;            // [Tm][DH]  V, then dOut
    float* ps = bs + Tm * DH;            // [Tq][ld]  P -> P' = P * keep / (1 - p)
    float* ds = ps + Tq * ld;            // [Tq][ld]  dP -> dS
    const DropState drop(spec);
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const int dh = D / H;
    const int i = threadIdx.x;
    const bool actq = i < Tq, actk = i < Tk;
    const int iq = min(i, Tq - 1), ik = min(i, Tk - 1);
    const float* qb = q + (size_t)b * sq + (size_t)h * dh * Tq;
    const float* kb = k + (size_t)b * sk + (size_t)h * dh * Tk;
    const float* vb = v + (size_t)b * sv + (size_t)h * dh * Tk;
    const float* gb = g + ((size_t)b * D + (size_t)h * dh) * Tq;
    float gq[DH], qv[DH];                                            // dOut and Q column of query i
#pragma unroll
    for (int c = 0; c < DH; ++c) {
        const int cc = EXACT ? c : min(c, dh - 1);
        const float gv = gb[(size_t)cc * Tq + iq];
        const float qq = qb[(size_t)cc * Tq + iq];
        const float kv = kb[(size_t)cc * Tk + ik];
        const float vv = vb[(size_t)cc * Tk + ik];
        const bool in = EXACT || c < dh;
        gq[c] = (in && actq) ? gv : 0.f;
        qv[c] = (in && actq) ? qq : 0.f;
        if (actk) {
            as[i * DH + c] = in ? kv : 0.f;
            bs[i * DH + c] = in ? vv : 0.f;
        }
    }
    const float* pg = probs + (size_t)blockIdx.x * Tq * Tk;
    for (int r = 0; r < Tq; ++r)
        if (i < Tk) ps[r * ld + i] = pg[(size_t)r * Tk + i];
    __syncthreads();
    const int off = Tk > Tq ? Tk - Tq : Tq - Tk;
    const int jmax = actq ? (causal ? attn_visible(i, off, Tk) : Tk) : 0;
    const size_t row = (size_t)blockIdx.x * Tq + i;
    float* pr = ps + iq * ld;
    float* dr = ds + iq * ld;
    float dot = 0.f;
    unsigned long long kept = 0ull;                                  // keep decisions of row i (bit j), drawn once
    for (int j0 = 0; j0 < jmax; j0 += 8) {
        float kp[8];
        drop.row8(row, j0 >> 3, Tk, kp);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = j0 + e;
            if (j < jmax) {
                float vr[DH];
                row_ld<DH>(bs + j * DH, vr);
                float sacc = 0.f;
#pragma unroll
                for (int c = 0; c < DH; ++c) sacc += gq[c] * vr[c];
                sacc *= kp[e];
                if (kp[e] != 0.f) kept |= 1ull << j;
                dr[j] = sacc;
                dot += pr[j] * sacc;
            }
        }
    }
    float dqa[DH];
#pragma unroll
    for (int c = 0; c < DH; ++c) dqa[c] = 0.f;
    for (int j = 0; j < jmax; ++j) {
        const float pv = pr[j];
        const float dsv = pv * (dr[j] - dot);
        dr[j] = dsv;
        pr[j] = ((kept >> j) & 1ull) ? pv * drop.inv : 0.f;
        float kr[DH];
        row_ld<DH>(as + j * DH, kr);
#pragma unroll
        for (int c = 0; c < DH; ++c) dqa[c] += dsv * kr[c];
    }
    if (actq) {
        for (int j = jmax; j < Tk; ++j) {
            dr[j] = 0.f;
            pr[j] = 0.f;
        }
        float* db = dq + (size_t)b * sdq + (size_t)h * dh * Tq;
#pragma unroll
        for (int c = 0; c < DH; ++c)
            if (EXACT || c < dh) db[(size_t)c * Tq + i] = dqa[c] * scale;
    }
    __syncthreads();                                                 // every lane is done with K and V
    if (actq) {
#pragma unroll
        for (int c = 0; c < DH; ++c) {
            as[i * DH + c] = qv[c];
            bs[i * DH + c] = gq[c];
        }
    }
    __syncthreads();
    if (!actk) return;
    // key i is visible to queries r >= i - off
    const int r0 = causal ? max(0, i - off) : 0;
    float dka[DH], dva[DH];
#pragma unroll
    for (int c = 0; c < DH; ++c) dka[c] = dva[c] = 0.f;
    for (int r = r0; r < Tq; ++r) {
        const float dsc = ds[r * ld + i], pc = ps[r * ld + i];
        float qr[DH], gr[DH];
        row_ld<DH>(as + r * DH, qr);
        row_ld<DH>(bs + r * DH, gr);
#pragma unroll
        for (int c = 0; c < DH; ++c) {
            dka[c] += dsc * qr[c];
            dva[c] += pc * gr[c];
        }
    }
    float* dkb = dk + (size_t)b * sdk + (size_t)h * dh * Tk;
    float* dvb = dv + (size_t)b * sdv + (size_t)h * dh * Tk;
#pragma unroll
    for (int c = 0; c < DH; ++c)
        if (EXACT || c < dh) {
            dkb[(size_t)c * Tk + i] = dka[c] * scale;
            dvb[(size_t)c * Tk + i] = dva[c];
        }
}

// ---------------------------------------------------------------------------------------------------------------
// Embedding: y_s = keep_s (scale x + pos) for x [B, E, T] and one or two dropout sites s (the key and the value embedding of one
// source draw their own decisions); pos [E, T] is the sinusoid table, dropped where x[b, 0, t] == 0 exactly (a padded step).
// A thread owns the eight channels of one Philox call (DropState::keep8); lanes walk consecutive t.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) posembed_fwd_kernel(const float* __restrict__ x, const float* __restrict__ pos,
                                                           float* __restrict__ y1, float* __restrict__ y2, int B, int E,
                                                           int T, float scale, const DropSpec s1, const DropSpec s2) {
    const int C8 = (E + 7) / 8;
    const size_t n = (size_t)B * C8 * T;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int t = (int)(idx % T), c8 = (int)((idx / T) % C8), b = (int)(idx / ((size_t)T * C8));
    const DropState d1(s1), d2(s2);
    const size_t base = (size_t)b * E * T + t;
    const bool pad = x[base] == 0.f;
    float k1[8], k2[8], xv[8], pv[8];
    d1.keep8(b, c8, t, E, T, k1);
    if (y2) d2.keep8(b, c8, t, E, T, k2);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int cc = min(c8 * 8 + e, E - 1);
        xv[e] = x[base + (size_t)cc * T];
        pv[e] = pos[(size_t)cc * T + t];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = c8 * 8 + e;
        if (c < E) {
            const float val = scale * xv[e] + (pad ? 0.f : pv[e]);
            y1[base + (size_t)c * T] = val * k1[e];
            if (y2) y2[base + (size_t)c * T] = val * k2[e];
        }
    }
}

// dx = scale (keep_1 g1 + keep_2 g2); the positional term carries no gradient
__global__ void __launch_bounds__(256) posembed_bwd_kernel(const float* __restrict__ g1, const float* __restrict__ g2,
                                                           float* __restrict__ dx, int B, int E, int T, float scale,
                                                           const DropSpec s1, const DropSpec s2) {
    const int C8 = (E + 7) / 8;
    const size_t n = (size_t)B * C8 * T;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int t = (int)(idx % T), c8 = (int)((idx / T) % C8), b = (int)(idx / ((size_t)T * C8));
    const DropState d1(s1), d2(s2);
    const size_t base = (size_t)b * E * T + t;
    float k1[8], k2[8], a[8], c2[8];
    d1.keep8(b, c8, t, E, T, k1);
    if (g2) d2.keep8(b, c8, t, E, T, k2);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const size_t i = base + (size_t)min(c8 * 8 + e, E - 1) * T;
        a[e] = g1[i];
        c2[e] = g2 ? g2[i] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = c8 * 8 + e;
        if (c < E) dx[base + (size_t)c * T] = scale * (a[e] * k1[e] + (g2 ? c2[e] * k2[e] : 0.f));
    }
}

}  // namespace dynmm

using namespace dynmm;

#define ST ((hipStream_t)stream)

extern "C" int dynmm_xattn_supported(int D, int Tq, int Tk, int heads) {
    if (D <= 0 || Tq <= 0 || Tk <= 0 || heads <= 0 || D % heads != 0) return 0;
    return (D / heads <= kXaMaxDh && Tq <= kXaMaxT && Tk <= kXaMaxT) ? 1 : 0;
}

static size_t xattn_lds(int DH, int Tq, int Tk, bool bwd) {
    const size_t ld = (size_t)(Tk | 1);
    const size_t Tm = (size_t)(Tq > Tk ? Tq : Tk);
    return (bwd ? 2 * Tm * DH + 2 * (size_t)Tq * ld : 2 * (size_t)Tk * DH + (size_t)Tq * ld + 64) * sizeof(float);
}

// the instantiations: dh = 4 (MULT's cross-modal transformers) and 12 (its memory transformers) exactly, the rest padded to 8 / 32
#define DYNMM_XA_DISPATCH(dh, CALL)                      \
    do {                                                 \
        if ((dh) == 4) { CALL(4, true); }                \
        else if ((dh) == 12) { CALL(12, true); }         \
        else if ((dh) <= 8) { CALL(8, false); }          \
        else { CALL(32, false); }                        \
    } while (0)

extern "C" int dynmm_xattn_fwd(const float* q, const float* k, const float* v, long long q_bstride, long long k_bstride,
                               long long v_bstride, float* out, float* probs, int B, int D, int Tq, int Tk, int heads,
                               int causal, const dynmm_dropout* drop, void* stream) {
    (void)hipGetLastError();
    if (!q || !k || !v || !out || !probs || !attn_args_ok(B, D, Tq, Tk, heads, drop)) return DYNMM_EINVAL;
    if (!attn_bstrides_ok(D, Tq, Tk, q_bstride, k_bstride, v_bstride)) return DYNMM_EINVAL;
    if (!dynmm_xattn_supported(D, Tq, Tk, heads)) return DYNMM_EUNSUPPORTED;
    const DropSpec spec = drop_spec(drop);
    const int dh = D / heads;
#define DYNMM_XA_F(DH, EX) hipLaunchKernelGGL((xattn_fwd_kernel<DH, EX>), dim3(B * heads), dim3(64), xattn_lds(DH, Tq, Tk, false), \
                                              ST, q, k, v, (size_t)q_bstride, (size_t)k_bstride, (size_t)v_bstride, out, probs, D, \
                                              Tq, Tk, heads, causal ? 1 : 0, attn_scale(dh), spec)
    DYNMM_XA_DISPATCH(dh, DYNMM_XA_F);
#undef DYNMM_XA_F
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_xattn_bwd(const float* g, const float* q, const float* k, const float* v, long long q_bstride,
                               long long k_bstride, long long v_bstride, const float* probs, float* dq, float* dk, float* dv,
                               long long dq_bstride, long long dk_bstride, long long dv_bstride, int B, int D, int Tq, int Tk,
                               int heads, int causal, const dynmm_dropout* drop, void* stream) {
    (void)hipGetLastError();
    if (!g || !q || !k || !v || !probs || !dq || !dk || !dv || !attn_args_ok(B, D, Tq, Tk, heads, drop)) return DYNMM_EINVAL;
    if (!attn_bstrides_ok(D, Tq, Tk, q_bstride, k_bstride, v_bstride) ||
        !attn_bstrides_ok(D, Tq, Tk, dq_bstride, dk_bstride, dv_bstride))
        return DYNMM_EINVAL;
    if (!dynmm_xattn_supported(D, Tq, Tk, heads)) return DYNMM_EUNSUPPORTED;
    const DropSpec spec = drop_spec(drop);
    const int dh = D / heads;
#define DYNMM_XA_B(DH, EX) hipLaunchKernelGGL((xattn_bwd_kernel<DH, EX>), dim3(B * heads), dim3(64), xattn_lds(DH, Tq, Tk, true), \
                                              ST, g, q, k, v, (size_t)q_bstride, (size_t)k_bstride, (size_t)v_bstride, probs, dq, \
                                              dk, dv, (size_t)dq_bstride, (size_t)dk_bstride, (size_t)dv_bstride, D, Tq, Tk, \
                                              heads, causal ? 1 : 0, attn_scale(dh), spec)
    DYNMM_XA_DISPATCH(dh, DYNMM_XA_B);
#undef DYNMM_XA_B
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_posembed_fwd(const float* x, const float* pos, float* y1, float* y2, int B, int E, int T, float scale,
                                  const dynmm_dropout* drop1, const dynmm_dropout* drop2, void* stream) {
    (void)hipGetLastError();
    if (!x || !pos || !y1 || B <= 0 || E <= 0 || T <= 0 || !drop_ok(drop1) || !drop_ok(drop2)) return DYNMM_EINVAL;
    const size_t n = (size_t)B * ((E + 7) / 8) * T;
    hipLaunchKernelGGL(posembed_fwd_kernel, dim3((unsigned)ceil_div_sz(n, 256)), dim3(256), 0, ST, x, pos, y1, y2, B, E, T, scale,
                       drop_spec(drop1), drop_spec(drop2));
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_posembed_bwd(const float* g1, const float* g2, float* dx, int B, int E, int T, float scale,
                                  const dynmm_dropout* drop1, const dynmm_dropout* drop2, void* stream) {
    (void)hipGetLastError();
    if (!g1 || !dx || B <= 0 || E <= 0 || T <= 0 || !drop_ok(drop1) || !drop_ok(drop2)) return DYNMM_EINVAL;
    const size_t n = (size_t)B * ((E + 7) / 8) * T;
    hipLaunchKernelGGL(posembed_bwd_kernel, dim3((unsigned)ceil_div_sz(n, 256)), dim3(256), 0, ST, g1, g2, dx, B, E, T, scale,
                       drop_spec(drop1), drop_spec(drop2));
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}
