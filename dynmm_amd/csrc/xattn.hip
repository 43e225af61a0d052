// MULT (MultiBench fusions.mult.MULTModel, affect_mm.py --fusion 4): what its pre-norm cross-modal transformers need beside the
// GEMMs (every Linear / Conv1d(k=1) stays a 1x1 convolution on the implicit-GEMM kernels):
//   * masked cross-modal attention with separate query and key lengths, forward + backward (dynmm_xattn_*),
//   * the embedding dropout(scale x + pos(x)) with the padding rule, one or two dropout sites per launch (dynmm_posembed_*),
//   * the pre-norm layer's `r + dropout(x)` fused with the LayerNorm that follows it (dynmm_prenorm_*): the launch returns the
//     sum AND its normalisation.
// DESIGN.md section 7m.
#include "common.h"
#include "dropout.h"

namespace dynmm {

constexpr int kXaMaxT = 64;
constexpr int kXaMaxDh = 32;

template <int N>
__device__ __forceinline__ void xa_ld(const float* __restrict__ p, float r[N]) {       // p: aligned to the widest unit used
    if constexpr (N % 4 == 0) {
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            const float4 t = reinterpret_cast<const float4*>(p)[q];
            r[4 * q] = t.x; r[4 * q + 1] = t.y; r[4 * q + 2] = t.z; r[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < N; ++q) r[q] = p[q];
    }
}

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
    const int jmax = actq ? (causal ? min(Tk, i + off + 1) : Tk) : 0;    // keys 0 .. jmax-1 are visible to query i
    const size_t row = (size_t)blockIdx.x * Tq + i;                  // probs and their keep flags are [B*H][Tq][Tk]
    float* pr = ps + iq * ld;
    // pass 1: the row maximum of the raw scores, as (hi, lo); the scores are recomputed in pass 2 instead of stored
    float mxh = -INFINITY, mxl = 0.f;
    for (int j = 0; j < jmax; ++j) {
        float kr[DH], hi, lo;
        xa_ld<DH>(ks + j * DH, kr);
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
                xa_ld<DH>(ks + j * DH, kr);
                xa_dot2<DH>(qr, kr, hi, lo);
                // (q . k_j - max) / sqrt(dh): the difference first, then the scale (torch scales q; the same function)
                const float ex = expf(((hi - mxh) + (lo - mxl)) * scale);
                pr[j] = ex;
                den += ex;
                const float w = ex * kp[e];                          // dropout acts on the normalised probabilities: linear in ex
                float vr[DH];
                xa_ld<DH>(vs + j * DH, vr);
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
    const int jmax = actq ? (causal ? min(Tk, i + off + 1) : Tk) : 0;
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
                xa_ld<DH>(bs + j * DH, vr);
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
        xa_ld<DH>(as + j * DH, kr);
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
        xa_ld<DH>(as + r * DH, qr);
        xa_ld<DH>(bs + r * DH, gr);
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

// ---------------------------------------------------------------------------------------------------------------
// Pre-norm plumbing: s = res + dropout(x) (x optional) and y = LayerNorm_D(s) in one launch, both returned; gamma == nullptr:
// the residual sum alone.  Thread layout and register cache of seq.hip's LayerNorm (16 tokens x 16 groups of 8 channels, NP
// passes).  Backward: ds = LayerNorm backward of gy + gs (gs = the gradient that reaches the sum directly, optional);
// dres = ds, dx = ds keep; per-workgroup parameter sums in `part`, added in a fixed order by pn_param_reduce_kernel.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kPnTok = 16, kPnGrp = 16, kPnCh = 8;

__device__ __forceinline__ float pn_group_sum(float v, float (*sh)[kPnTok], int tl, int grp) {
    sh[grp][tl] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kPnGrp; ++k) s += sh[k][tl];               // fixed order: deterministic
    __syncthreads();
    return s;
}

template <int NP>
__global__ void __launch_bounds__(256) prenorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* __restrict__ sum, float* __restrict__ y,
                                                          float* __restrict__ mean, float* __restrict__ rstd, int B, int D,
                                                          int T, float eps, const DropSpec spec) {
    __shared__ float sh[kPnGrp][kPnTok];
    const DropState ds(spec);
    const int tl = threadIdx.x & (kPnTok - 1), grp = threadIdx.x / kPnTok;
    const int tok = blockIdx.x * kPnTok + tl;
    const bool ok = tok < B * T;
    const int b = ok ? tok / T : 0, t = ok ? tok - b * T : 0;
    const size_t base = (size_t)b * D * T + t;
    const float* gp = gamma ? gamma : res;                          // (clamped, in-range reads either way; unused without gamma)
    const float* bp = gamma ? beta : res;
    float v[NP][kPnCh], gm[NP][kPnCh], bt[NP][kPnCh];
    float s = 0.f;
#pragma unroll
    for (int pp = 0; pp < NP; ++pp) {
        const int c8 = pp * kPnGrp + grp;
        float k[kPnCh], xv[kPnCh], rv[kPnCh];
        ds.keep8(b, min(c8, (D - 1) / kPnCh), t, D, T, k);
#pragma unroll
        for (int e = 0; e < kPnCh; ++e) {                          // unconditional loads on clamped addresses, selected below
            const int cc = min(c8 * kPnCh + e, D - 1);
            const size_t i = base + (size_t)cc * T;
            xv[e] = x ? x[i] : 0.f;
            rv[e] = res[i];
            gm[pp][e] = gp[gamma ? cc : 0];
            bt[pp][e] = bp[gamma ? cc : 0];
        }
#pragma unroll
        for (int e = 0; e < kPnCh; ++e) {
            const int c = c8 * kPnCh + e;
            const bool valid = ok && c < D;
            v[pp][e] = valid ? xv[e] * k[e] + rv[e] : 0.f;
            s += v[pp][e];
            if (valid && sum) sum[base + (size_t)c * T] = v[pp][e];
        }
    }
    if (!gamma) return;                                             // (uniform over the launch)
    const float mu = pn_group_sum(s, sh, tl, grp) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int pp = 0; pp < NP; ++pp)
#pragma unroll
        for (int e = 0; e < kPnCh; ++e)
            if (ok && (pp * kPnGrp + grp) * kPnCh + e < D) {
                const float d = v[pp][e] - mu;
                q += d * d;
            }
    const float rs = rsqrtf(pn_group_sum(q, sh, tl, grp) / (float)D + eps);
    if (!ok) return;
    if (grp == 0) {
        mean[tok] = mu;
        rstd[tok] = rs;
    }
#pragma unroll
    for (int pp = 0; pp < NP; ++pp)
#pragma unroll
        for (int e = 0; e < kPnCh; ++e) {
            const int c = (pp * kPnGrp + grp) * kPnCh + e;
            if (c < D) y[base + (size_t)c * T] = (v[pp][e] - mu) * rs * gm[pp][e] + bt[pp][e];
        }
}

template <int NP>
__global__ void __launch_bounds__(256) prenorm_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ gs,
                                                          const float* __restrict__ sum, const float* __restrict__ gamma,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          float* __restrict__ dx, float* __restrict__ dres,
                                                          float* __restrict__ part, int B, int D, int T,
                                                          const DropSpec spec) {
    __shared__ float sh[kPnGrp][kPnTok];
    const DropState ds(spec);
    const int tl = threadIdx.x & (kPnTok - 1), grp = threadIdx.x / kPnTok;
    const int tok = blockIdx.x * kPnTok + tl;
    const bool ok = tok < B * T;
    const int b = ok ? tok / T : 0, t = ok ? tok - b * T : 0;
    const size_t base = (size_t)b * D * T + t;
    const float mu = ok ? mean[tok] : 0.f, rs = ok ? rstd[tok] : 0.f;
    float gv[NP][kPnCh], xh[NP][kPnCh], kk[NP][kPnCh], gm[NP][kPnCh], sv[NP][kPnCh];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int pp = 0; pp < NP; ++pp) {
        const int c8 = pp * kPnGrp + grp;
        ds.keep8(b, min(c8, (D - 1) / kPnCh), t, D, T, kk[pp]);
        float xv[kPnCh];
#pragma unroll
        for (int e = 0; e < kPnCh; ++e) {
            const int cc = min(c8 * kPnCh + e, D - 1);
            const size_t i = base + (size_t)cc * T;
            gv[pp][e] = gy[i];
            sv[pp][e] = gs ? gs[i] : 0.f;
            xv[e] = sum[i];
            gm[pp][e] = gamma[cc];
        }
#pragma unroll
        for (int e = 0; e < kPnCh; ++e) {
            const bool valid = ok && c8 * kPnCh + e < D;
            gv[pp][e] = valid ? gv[pp][e] : 0.f;
            xh[pp][e] = valid ? (xv[e] - mu) * rs : 0.f;
            const float gg = gv[pp][e] * gm[pp][e];
            s1 += gg;
            s2 += gg * xh[pp][e];
        }
    }
    s1 = pn_group_sum(s1, sh, tl, grp) / (float)D;
    s2 = pn_group_sum(s2, sh, tl, grp) / (float)D;
#pragma unroll
    for (int pp = 0; pp < NP; ++pp)
#pragma unroll
        for (int e = 0; e < kPnCh; ++e) {
            const int c = (pp * kPnGrp + grp) * kPnCh + e;
            if (ok && c < D) {
                const size_t i = base + (size_t)c * T;
                const float dv = rs * (gv[pp][e] * gm[pp][e] - s1 - xh[pp][e] * s2) + sv[pp][e];
                if (dres) dres[i] = dv;
                if (dx) dx[i] = dv * kk[pp][e];
            }
        }
    if (part) {
        // the 16 tokens of a channel sit in the 16 lanes of one row of the wave: xor-butterfly inside the row
        float* pr = part + (size_t)blockIdx.x * 2 * D;
#pragma unroll
        for (int pp = 0; pp < NP; ++pp)
#pragma unroll
            for (int e = 0; e < kPnCh; ++e) {
                float a = gv[pp][e] * xh[pp][e], bsum = gv[pp][e];
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) {
                    a += __shfl_xor(a, o, 16);
                    bsum += __shfl_xor(bsum, o, 16);
                }
                const int c = (pp * kPnGrp + grp) * kPnCh + e;
                if (tl == 0 && c < D) {
                    pr[c] = a;
                    pr[D + c] = bsum;
                }
            }
    }
}

// dgamma[c], dbeta[c] = the workgroups' rows of `part` added in a fixed order: one wave per column, lane = a 64-way split of rows
// `accumulate`: the sums are ADDED to dgamma / dbeta (a LayerNorm applied to several inputs in one step: the launches of one stream
// run in order, one thread owns a column, so the result is still a fixed-order sum).
__global__ void __launch_bounds__(256) pn_param_reduce_kernel(const float* __restrict__ part, int nrows, int D,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              int accumulate) {
    const int sp = threadIdx.x & 63;
    const int col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= 2 * D) return;
    const int per = (nrows + 63) / 64;
    const int r0 = min(nrows, sp * per), r1 = min(nrows, (sp + 1) * per);
    float s = 0.f;
    for (int r = r0; r < r1; ++r) s += part[(size_t)r * 2 * D + col];
    s = wave_reduce_sum<float>(s);
    if (sp == 0) {
        float* dst = col < D ? dgamma + col : dbeta + (col - D);
        *dst = accumulate ? *dst + s : s;
    }
}

}  // namespace dynmm

using namespace dynmm;

#define ST ((hipStream_t)stream)

static bool xattn_args_ok(int B, int D, int Tq, int Tk, int heads, const dynmm_dropout* drop) {
    return B > 0 && D > 0 && Tq > 0 && Tk > 0 && heads > 0 && D % heads == 0 && drop_ok(drop);
}

extern "C" int dynmm_xattn_supported(int D, int Tq, int Tk, int heads) {
    if (D <= 0 || Tq <= 0 || Tk <= 0 || heads <= 0 || D % heads != 0) return 0;
    return (D / heads <= kXaMaxDh && Tq <= kXaMaxT && Tk <= kXaMaxT) ? 1 : 0;
}

// 1 / sqrt(dh), correctly rounded (the device's reciprocal square root is not)
static float xattn_scale(int dh) { return (float)(1.0 / sqrt((double)dh)); }

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
    if (!q || !k || !v || !out || !probs || !xattn_args_ok(B, D, Tq, Tk, heads, drop)) return DYNMM_EINVAL;
    if (q_bstride < (long long)D * Tq || k_bstride < (long long)D * Tk || v_bstride < (long long)D * Tk) return DYNMM_EINVAL;
    if (!dynmm_xattn_supported(D, Tq, Tk, heads)) return DYNMM_EUNSUPPORTED;
    const DropSpec spec = drop_spec(drop);
    const int dh = D / heads;
#define DYNMM_XA_F(DH, EX) hipLaunchKernelGGL((xattn_fwd_kernel<DH, EX>), dim3(B * heads), dim3(64), xattn_lds(DH, Tq, Tk, false), \
                                              ST, q, k, v, (size_t)q_bstride, (size_t)k_bstride, (size_t)v_bstride, out, probs, D, \
                                              Tq, Tk, heads, causal ? 1 : 0, xattn_scale(dh), spec)
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
    if (!g || !q || !k || !v || !probs || !dq || !dk || !dv || !xattn_args_ok(B, D, Tq, Tk, heads, drop)) return DYNMM_EINVAL;
    if (q_bstride < (long long)D * Tq || k_bstride < (long long)D * Tk || v_bstride < (long long)D * Tk ||
        dq_bstride < (long long)D * Tq || dk_bstride < (long long)D * Tk || dv_bstride < (long long)D * Tk)
        return DYNMM_EINVAL;
    if (!dynmm_xattn_supported(D, Tq, Tk, heads)) return DYNMM_EUNSUPPORTED;
    const DropSpec spec = drop_spec(drop);
    const int dh = D / heads;
#define DYNMM_XA_B(DH, EX) hipLaunchKernelGGL((xattn_bwd_kernel<DH, EX>), dim3(B * heads), dim3(64), xattn_lds(DH, Tq, Tk, true), \
                                              ST, g, q, k, v, (size_t)q_bstride, (size_t)k_bstride, (size_t)v_bstride, probs, dq, \
                                              dk, dv, (size_t)dq_bstride, (size_t)dk_bstride, (size_t)dv_bstride, D, Tq, Tk, \
                                              heads, causal ? 1 : 0, xattn_scale(dh), spec)
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

#define DYNMM_PN_DISPATCH(D, CALL)                 \
    do {                                           \
        if ((D) <= 128) { CALL(1); }               \
        else if ((D) <= 256) { CALL(2); }          \
        else if ((D) <= 512) { CALL(4); }          \
        else { CALL(8); }                          \
    } while (0)
constexpr int kPnMaxD = 1024;

extern "C" int dynmm_prenorm_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* sum, float* y,
                                 float* mean, float* rstd, int B, int D, int T, float eps, const dynmm_dropout* drop,
                                 void* stream) {
    (void)hipGetLastError();
    if (!res || B <= 0 || D <= 0 || T <= 0 || !drop_ok(drop)) return DYNMM_EINVAL;
    if (gamma ? (!beta || !y || !mean || !rstd) : (!sum || !x)) return DYNMM_EINVAL;
    if (D > kPnMaxD) return DYNMM_EUNSUPPORTED;
    const DropSpec spec = drop_spec(drop);
#define DYNMM_PN_F(NP) hipLaunchKernelGGL((prenorm_fwd_kernel<NP>), dim3(ceil_div(B * T, kPnTok)), dim3(256), 0, ST, x, res, gamma, \
                                          beta, sum, y, mean, rstd, B, D, T, eps, spec)
    DYNMM_PN_DISPATCH(D, DYNMM_PN_F);
#undef DYNMM_PN_F
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" size_t dynmm_prenorm_bwd_workspace_bytes(int B, int D, int T) {
    if (B <= 0 || D <= 0 || T <= 0) return 0;
    return (size_t)ceil_div(B * T, kPnTok) * 2 * D * sizeof(float);
}

extern "C" int dynmm_prenorm_bwd(const float* gy, const float* gs, const float* sum, const float* gamma, const float* mean,
                                 const float* rstd, float* dx, float* dres, float* dgamma, float* dbeta, int B, int D, int T,
                                 const dynmm_dropout* drop, int accumulate, float* workspace, size_t workspace_bytes,
                                 void* stream) {
    (void)hipGetLastError();
    if (!gy || !sum || !gamma || !mean || !rstd || B <= 0 || D <= 0 || T <= 0 || !drop_ok(drop)) return DYNMM_EINVAL;
    if ((dgamma == nullptr) != (dbeta == nullptr)) return DYNMM_EINVAL;
    if (dgamma && (!workspace || workspace_bytes < dynmm_prenorm_bwd_workspace_bytes(B, D, T))) return DYNMM_EWORKSPACE;
    if (D > kPnMaxD) return DYNMM_EUNSUPPORTED;
    const DropSpec spec = drop_spec(drop);
    const int nblk = ceil_div(B * T, kPnTok);
    float* part = dgamma ? workspace : nullptr;
#define DYNMM_PN_B(NP) hipLaunchKernelGGL((prenorm_bwd_kernel<NP>), dim3(nblk), dim3(256), 0, ST, gy, gs, sum, gamma, mean, rstd, dx, \
                                          dres, part, B, D, T, spec)
    DYNMM_PN_DISPATCH(D, DYNMM_PN_B);
#undef DYNMM_PN_B
    DYNMM_LAUNCH_CHECK();
    if (dgamma) {
        hipLaunchKernelGGL(pn_param_reduce_kernel, dim3(ceil_div(2 * D, 4)), dim3(256), 0, ST, workspace, nblk, D, dgamma, dbeta,
                           accumulate ? 1 : 0);
        DYNMM_LAUNCH_CHECK();
    }
    return DYNMM_OK;
}
