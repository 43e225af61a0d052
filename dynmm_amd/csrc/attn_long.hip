// Streaming (online-softmax) attention with separate query and key lengths and no cap on either: the attention of sequences the
// whole-row kernels of seq.hip, attn.hip and xattn.hip (T <= 64, the probabilities stored) cannot hold.  Same tensors as xattn.hip:
//   q [B, D, Tq], k / v [B, D, Tk] (channel stride = the sequence length, a batch stride each: the thirds of a packed [B, 3D, T]
//   serve without a copy), out [B, D, Tq], lse [B*heads, Tq] = log sum_j exp(s_ij) of the masked, scaled scores,
//   P = softmax_j((q_i / sqrt(dh)) . k_j + mask),  out[c][i] = sum_j P'[i][j] v[c][j],  P' = P * keep / (1 - p).
// causal: key j is visible to query i iff j <= i + |Tk - Tq| (xattn.hip's rule; key 0 is always visible, no row is empty).
// 1 <= dh <= 64, 1 <= Tq, Tk <= kAlMaxT, B * heads * ceil(T / 64) workgroups must fit a grid.  DESIGN.md section 7p.
//
// No [B*heads, Tq, Tk] tensor exists in either pass: the forward keeps a running maximum and denominator per query and saves the
// log-sum-exp, the backward recomputes P = exp(s - lse) from it.
//
// Tiling (attn.hip's, made to stream).  A workgroup of four waves owns 64 consecutive rows of one (sample, head), wave w rows
// 16 w .. 16 w + 15, and walks the OTHER sequence in tiles of 64 tokens staged in LDS token-major, [token][LD] with LD = 4 (mod
// 16) — both operand shapes of v_mfma_f32_16x16x4_f32 are conflict-free 4-byte reads (attn.hip's header has the bank arithmetic).
// The owned rows never touch LDS: a lane's values of its own row are at once the B operand of the products over the channels.
//   forward, dq pass: rows = queries; K and V stream.  The score tile is computed TRANSPOSED (rows = keys, columns = queries), so
//     lane (i = lane & 15, g = lane >> 4) holds keys 16 jt + 4 g + r of query i in register r of tile jt: a query's 64 scores are
//     16 registers of 4 lanes (maximum / sums = register work and two lane exchanges), and register r is a valid B operand of the
//     product over the KEYS that follows (out^T = V^T P'^T, dQ^T = K^T dS^T).
//   dk / dv pass: rows = keys; Q (scaled), dOut, lse and delta stream.  The tile is not transposed (rows = queries, columns = the
//     wave's keys), and P' and dS are again B operands of the products over the QUERIES (dV^T = dOut^T P', dK^T = Q^T dS).
// Each workgroup owns the rows it writes — dq by query tiles, dk / dv by key tiles — so there are no atomics and no workspace, and
// equal inputs give equal bits.  delta_i = sum_c dOut[c][i] out[c][i] (= sum_j P dP) is formed in both passes from the values a
// wave loads anyway, as the diagonal of one more 16 x 16 product (al_diag).  Tiles that the mask hides from the whole workgroup
// are not visited (the loops' bounds), tiles and 16-token sub-tiles it hides from a whole wave are not computed; hidden positions
// inside a computed tile are selected to exact zeros (never multiplied away: a hidden key's score may be anything).
// The next tile's global loads are issued before the current tile's arithmetic (registers), so they fly under it.
//
// Dropout: DropState::row8 with row = the flat query row bh * Tq + i and 8-key chunks — the indexing of seq.hip, attn.hip and
// xattn.hip: injected flags are the flat [B*heads, Tq, Tk] bytes and the generator draws their decisions.  A chunk is drawn once
// per query and pass and kept as bits (~900 issue cycles per Philox call): in the query-row passes each of a query's four lanes
// draws chunks g and g + 4 of the tile (attn_draw, as in attn.hip), in the key-row pass lane l draws the wave's two chunks of query l.
//
// Loads are unconditional on clamped addresses with the value masked afterwards (a bit mask, attn_keep_if); only stores are
// bounded.  The tile helpers (attn_load / attn_store, attn_draw / attn_keep4, the query reductions), the mask rule and the host
// checks are attn_tile.h's.
#include "attn_tile.h"

namespace dynmm {

constexpr int kAlMaxDh = 64;
constexpr int kAlMaxT = 1 << 24;          // flat indices are size_t; 64 * (tile index) and i + |Tk - Tq| stay far inside int
constexpr int kAlTile = 64;               // rows per workgroup and tokens per streamed tile

// delta of this lane's token from the 16 x 16 product of the wave's out and dOut rows: the diagonal element (t, t) sits in
// register t & 3 of lane t + 16 (t >> 2).  delta is formed by the instruction and operand order that forms dP, so that with ONE
// visible key (out = v_0, P = 1) dS = P (dP - delta) is exactly 0, as it is for the whole-row kernels' sum_j P dP.
__device__ __forceinline__ float al_diag(f32x4 c, int lane) {
    const int t = lane & 15, r = t & 3;
    const float mine = r == 0 ? c[0] : r == 1 ? c[1] : r == 2 ? c[2] : c[3];
    return __shfl(mine, t + 16 * (t >> 2), 64);
}

struct AlArgs {
    const float *q, *k, *v;             // batch strides sq, sk, sv
    size_t sq, sk, sv;
    int D, Tq, Tk, H, causal;
    float scale;
};

// ---------------------------------------------------------------------------------------------------------------
// forward: grid = ceil(Tq / 64) * B * H
// ---------------------------------------------------------------------------------------------------------------
template <int DH>
__global__ void __launch_bounds__(256) al_fwd_kernel(const AlArgs a, float* __restrict__ out, float* __restrict__ lse, int nqt,
                                                     const DropSpec spec) {
    constexpr int KS = AttnShape<DH>::KS, CT = AttnShape<DH>::CT, LD = AttnShape<DH>::LD;
    __shared__ __align__(16) float ks[kAlTile * LD];
    __shared__ __align__(16) float vs[kAlTile * LD];
    const DropState drop(spec);
    const int Tq = a.Tq, Tk = a.Tk, H = a.H;
    const int bh = blockIdx.x / nqt, qt = blockIdx.x - bh * nqt;
    const int b = bh / H, h = bh - b * H;
    const int dh = a.D / H;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int q0 = kAlTile * qt;
    const int i = q0 + 16 * w + li, ic = min(i, Tq - 1);         // this lane's query (past Tq: a copy of the last one, not stored)
    const float* qb = a.q + (size_t)b * a.sq + (size_t)h * dh * Tq;
    const float* kb = a.k + (size_t)b * a.sk + (size_t)h * dh * Tk;
    const float* vb = a.v + (size_t)b * a.sv + (size_t)h * dh * Tk;
    float rq[KS], rk[KS], rv[KS];
    attn_load<DH>(qb, rq, dh, Tq, q0, w, lane);
    attn_load<DH>(kb, rk, dh, Tk, 0, w, lane);
    attn_load<DH>(vb, rv, dh, Tk, 0, w, lane);
    float qv[KS];                                                // scaled by 1 / sqrt(dh) (torch scales q before q @ k^T)
#pragma unroll
    for (int k = 0; k < KS; ++k) qv[k] = attn_keep_if(rq[k] * a.scale, 4 * k + g < dh);
    const int off = Tk > Tq ? Tk - Tq : Tq - Tk;
    // keys 0 .. n-1 are visible: to the workgroup's last query (jend), the wave's last query (wvis), this lane's query (jvis)
    const int jend = a.causal ? attn_visible(min(q0 + kAlTile - 1, Tq - 1), off, Tk) : Tk;
    const int wvis = a.causal ? attn_visible(min(q0 + 16 * w + 15, Tq - 1), off, Tk) : Tk;
    const int jvis = a.causal ? attn_visible(ic, off, Tk) : Tk;
    const int nkt = (jend + kAlTile - 1) / kAlTile;
    const bool live = q0 + 16 * w < Tq;                          // (a wave past Tq only helps staging)
    const size_t row = (size_t)bh * Tq + ic;                     // the keep flags are [B*H][Tq][Tk]
    const bool dropping = drop.p > 0.f;

    float m = -INFINITY, l = 0.f;                                // running maximum and denominator of this lane's query
    f32x4 o[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) o[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nkt; ++kt) {
        const int j0 = kAlTile * kt;
        __syncthreads();                                         // every wave is done with the previous tile
        attn_store<DH>(ks, rk, dh, Tk, j0, w, lane, 1.f);
        attn_store<DH>(vs, rv, dh, Tk, j0, w, lane, 1.f);
        __syncthreads();
        if (kt + 1 < nkt) {
            attn_load<DH>(kb, rk, dh, Tk, j0 + kAlTile, w, lane);
            attn_load<DH>(vb, rv, dh, Tk, j0 + kAlTile, w, lane);
        }
        if (!(live && j0 < wvis)) continue;
        const unsigned bits = dropping ? attn_draw<true>(drop, row, Tk, 8 * kt + g, jvis) : 0u;
        // S^T[j][i] = sum_c K[j][c] Q[i][c]
        f32x4 s[4];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) s[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KS; ++k)
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
                if (j0 + 16 * jt < wvis) s[jt] = mfma_16x16x4(ks[(16 * jt + li) * LD + 4 * k + g], qv[k], s[jt]);
        float mx = m;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[jt][r] = j0 + 16 * jt + 4 * g + r < jvis ? s[jt][r] : -INFINITY;
                mx = fmaxf(mx, s[jt][r]);
            }
        mx = attn_query_max(mx);                                   // finite from tile 0 on: key 0 is visible to every query
        const float alpha = expf(m - mx);                        // (tile 0: exp(-inf) = 0)
        float sum = 0.f;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            const unsigned k4 = dropping ? attn_keep4(bits, jt, lane) : 0xfu;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = expf(s[jt][r] - mx);
                sum += e;
                s[jt][r] = ((k4 >> r) & 1u) ? e * drop.inv : 0.f; // dropout acts on the normalised probabilities: linear in e
            }
        }
        l = l * alpha + attn_query_sum(sum);
        m = mx;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) o[ct] *= alpha;
        // out^T[c][i] += sum_j V[j][c] P'[i][j]: k-step (jt, r) = keys 16 jt + 4 g + r, P' straight from the accumulators
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
            if (j0 + 16 * jt < wvis) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float* vr = vs + (16 * jt + 4 * g + r) * LD + li;
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) o[ct] = mfma_16x16x4(vr[16 * ct], s[jt][r], o[ct]);
                }
            }
    }
    if (!(live && i < Tq)) return;
    const float inv = 1.f / l;
    float* ob = out + ((size_t)b * a.D + (size_t)h * dh) * Tq;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = 16 * ct + 4 * g + r;
            if (c < dh) ob[(size_t)c * Tq + i] = o[ct][r] * inv;
        }
    if (g == 0) lse[(size_t)bh * Tq + i] = m + logf(l);
}

// ---------------------------------------------------------------------------------------------------------------
// backward, query rows: dq.  grid = ceil(Tq / 64) * B * H
//   P = exp(s - lse), dP'^T[j][i] = sum_c V[j][c] dOut[i][c], dS = P (dP' keep / (1 - p) - delta), dQ^T[c][i] = scale sum_j K[j][c] dS
// ---------------------------------------------------------------------------------------------------------------
template <int DH>
__global__ void __launch_bounds__(256) al_bwd_dq_kernel(const AlArgs a, const float* __restrict__ gout,
                                                        const float* __restrict__ out, const float* __restrict__ lse,
                                                        float* __restrict__ dq, size_t sdq, int nqt, const DropSpec spec) {
    constexpr int KS = AttnShape<DH>::KS, CT = AttnShape<DH>::CT, LD = AttnShape<DH>::LD;
    __shared__ __align__(16) float ks[kAlTile * LD];
    __shared__ __align__(16) float vs[kAlTile * LD];
    const DropState drop(spec);
    const int Tq = a.Tq, Tk = a.Tk, H = a.H;
    const int bh = blockIdx.x / nqt, qt = blockIdx.x - bh * nqt;
    const int b = bh / H, h = bh - b * H;
    const int dh = a.D / H;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int q0 = kAlTile * qt;
    const int i = q0 + 16 * w + li, ic = min(i, Tq - 1);
    const float* qb = a.q + (size_t)b * a.sq + (size_t)h * dh * Tq;
    const float* kb = a.k + (size_t)b * a.sk + (size_t)h * dh * Tk;
    const float* vb = a.v + (size_t)b * a.sv + (size_t)h * dh * Tk;
    const size_t ooff = ((size_t)b * a.D + (size_t)h * dh) * Tq;
    float rq[KS], rg[KS], ro[KS], rk[KS], rv[KS];
    attn_load<DH>(qb, rq, dh, Tq, q0, w, lane);
    attn_load<DH>(gout + ooff, rg, dh, Tq, q0, w, lane);
    attn_load<DH>(out + ooff, ro, dh, Tq, q0, w, lane);
    attn_load<DH>(kb, rk, dh, Tk, 0, w, lane);
    attn_load<DH>(vb, rv, dh, Tk, 0, w, lane);
    const size_t row = (size_t)bh * Tq + ic;
    const float lse_i = lse[row];
    float qv[KS], gv[KS];
    f32x4 dd = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KS; ++k) {
        qv[k] = attn_keep_if(rq[k] * a.scale, 4 * k + g < dh);
        gv[k] = attn_keep_if(rg[k], 4 * k + g < dh);
        dd = mfma_16x16x4(ro[k], gv[k], dd);                     // out (rows) x dOut (columns) of the wave's 16 queries
    }
    const float delta = al_diag(dd, lane);                       // sum_c dOut[c][i] out[c][i]
    const int off = Tk > Tq ? Tk - Tq : Tq - Tk;
    const int jend = a.causal ? attn_visible(min(q0 + kAlTile - 1, Tq - 1), off, Tk) : Tk;
    const int wvis = a.causal ? attn_visible(min(q0 + 16 * w + 15, Tq - 1), off, Tk) : Tk;
    const int jvis = a.causal ? attn_visible(ic, off, Tk) : Tk;
    const int nkt = (jend + kAlTile - 1) / kAlTile;
    const bool live = q0 + 16 * w < Tq;
    const bool dropping = drop.p > 0.f;

    f32x4 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nkt; ++kt) {
        const int j0 = kAlTile * kt;
        __syncthreads();
        attn_store<DH>(ks, rk, dh, Tk, j0, w, lane, 1.f);
        attn_store<DH>(vs, rv, dh, Tk, j0, w, lane, 1.f);
        __syncthreads();
        if (kt + 1 < nkt) {
            attn_load<DH>(kb, rk, dh, Tk, j0 + kAlTile, w, lane);
            attn_load<DH>(vb, rv, dh, Tk, j0 + kAlTile, w, lane);
        }
        if (!(live && j0 < wvis)) continue;
        const unsigned bits = dropping ? attn_draw<true>(drop, row, Tk, 8 * kt + g, jvis) : 0u;
        f32x4 s[4], d[4];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) s[jt] = d[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KS; ++k)
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
                if (j0 + 16 * jt < wvis) {
                    s[jt] = mfma_16x16x4(ks[(16 * jt + li) * LD + 4 * k + g], qv[k], s[jt]);
                    d[jt] = mfma_16x16x4(vs[(16 * jt + li) * LD + 4 * k + g], gv[k], d[jt]);
                }
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            const unsigned k4 = dropping ? attn_keep4(bits, jt, lane) : 0xfu;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool vis = j0 + 16 * jt + 4 * g + r < jvis;
                const float p = expf((vis ? s[jt][r] : -INFINITY) - lse_i);
                const float kf = ((k4 >> r) & 1u) ? drop.inv : 0.f;
                s[jt][r] = vis ? p * (d[jt][r] * kf - delta) : 0.f;                 // dS
            }
        }
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
            if (j0 + 16 * jt < wvis) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float* kr = ks + (16 * jt + 4 * g + r) * LD + li;
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) acc[ct] = mfma_16x16x4(kr[16 * ct], s[jt][r], acc[ct]);
                }
            }
    }
    if (!(live && i < Tq)) return;
    float* db = dq + (size_t)b * sdq + (size_t)h * dh * Tq;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = 16 * ct + 4 * g + r;
            if (c < dh) db[(size_t)c * Tq + i] = acc[ct][r] * a.scale;
        }
}

// ---------------------------------------------------------------------------------------------------------------
// backward, key rows: dk, dv.  grid = ceil(Tk / 64) * B * H.  Lane (li, g) of wave w owns key k0 + 16 w + li; register r of
// query sub-tile `it` is query 16 it + 4 g + r of the streamed tile.
//   dV^T[c][j] = sum_i dOut[i][c] P'[i][j],  dK^T[c][j] = sum_i (scale Q[i][c]) dS[i][j]
// ---------------------------------------------------------------------------------------------------------------
template <int DH>
__global__ void __launch_bounds__(256) al_bwd_dkv_kernel(const AlArgs a, const float* __restrict__ gout,
                                                         const float* __restrict__ out, const float* __restrict__ lse,
                                                         float* __restrict__ dk, float* __restrict__ dv, size_t sdk, size_t sdv,
                                                         int nkt, const DropSpec spec) {
    constexpr int KS = AttnShape<DH>::KS, CT = AttnShape<DH>::CT, LD = AttnShape<DH>::LD;
    __shared__ __align__(16) float qs[kAlTile * LD];             // scaled as the forward scaled it: the same scores
    __shared__ __align__(16) float gs[kAlTile * LD];
    __shared__ float lse_s[kAlTile], del_s[kAlTile];
    const DropState drop(spec);
    const int Tq = a.Tq, Tk = a.Tk, H = a.H;
    const int bh = blockIdx.x / nkt, kt = blockIdx.x - bh * nkt;
    const int b = bh / H, h = bh - b * H;
    const int dh = a.D / H;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int k0 = kAlTile * kt, kmin = k0 + 16 * w;             // the wave's keys: kmin .. kmin + 15
    const int j = kmin + li;
    const float* qb = a.q + (size_t)b * a.sq + (size_t)h * dh * Tq;
    const float* kb = a.k + (size_t)b * a.sk + (size_t)h * dh * Tk;
    const float* vb = a.v + (size_t)b * a.sv + (size_t)h * dh * Tk;
    const size_t ooff = ((size_t)b * a.D + (size_t)h * dh) * Tq;
    const float* gb = gout + ooff;
    const float* ob = out + ooff;
    const float* lb = lse + (size_t)bh * Tq;
    const int off = Tk > Tq ? Tk - Tq : Tq - Tk;
    // key j is visible to the queries i >= j - off: the first query tile that sees any key of the workgroup
    const int nqt = (Tq + kAlTile - 1) / kAlTile;
    const int qt0 = a.causal ? max(0, k0 - off) / kAlTile : 0;
    float rk[KS], rv[KS], rq[KS], rg[KS], ro[KS];
    attn_load<DH>(kb, rk, dh, Tk, k0, w, lane);
    attn_load<DH>(vb, rv, dh, Tk, k0, w, lane);
    attn_load<DH>(qb, rq, dh, Tq, kAlTile * qt0, w, lane);
    attn_load<DH>(gb, rg, dh, Tq, kAlTile * qt0, w, lane);
    attn_load<DH>(ob, ro, dh, Tq, kAlTile * qt0, w, lane);
    float rl = lb[min(kAlTile * qt0 + 16 * w + li, Tq - 1)];
    float kv[KS], vv[KS];
#pragma unroll
    for (int k = 0; k < KS; ++k) {
        kv[k] = attn_keep_if(rk[k], 4 * k + g < dh);
        vv[k] = attn_keep_if(rv[k], 4 * k + g < dh);
    }
    const bool live = kmin < Tk;
    const bool dropping = drop.p > 0.f;

    f32x4 ak[CT], av[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) ak[ct] = av[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int qt = qt0; qt < nqt; ++qt) {
        const int i0 = kAlTile * qt;
        __syncthreads();
        attn_store<DH>(qs, rq, dh, Tq, i0, w, lane, a.scale);
        attn_store<DH>(gs, rg, dh, Tq, i0, w, lane, 1.f);
        {
            f32x4 dd = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < KS; ++k) dd = mfma_16x16x4(attn_keep_if(rg[k], 4 * k + g < dh), ro[k], dd);
            const float dl = al_diag(dd, lane);
            if (g == 0) {
                lse_s[16 * w + li] = rl;
                del_s[16 * w + li] = dl;
            }
        }
        __syncthreads();
        if (qt + 1 < nqt) {
            attn_load<DH>(qb, rq, dh, Tq, i0 + kAlTile, w, lane);
            attn_load<DH>(gb, rg, dh, Tq, i0 + kAlTile, w, lane);
            attn_load<DH>(ob, ro, dh, Tq, i0 + kAlTile, w, lane);
            rl = lb[min(i0 + kAlTile + 16 * w + li, Tq - 1)];
        }
        // the tile's last query does not see the wave's first key: nothing of the tile does
        if (!(live && (!a.causal || i0 + kAlTile - 1 + off >= kmin))) continue;
        unsigned bits = 0u;                                      // bit e: the decision of (query i0 + lane, key kmin + e)
        if (dropping) {
            const int iq = i0 + lane;
            const int lastvis = a.causal ? iq + off : Tk - 1;    // the last key query iq sees (before the bound Tk)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int j8 = (kmin >> 3) + c;
                if (iq < Tq && 8 * j8 < Tk && 8 * j8 <= lastvis) {
                    float kp[8];
                    drop.row8((size_t)bh * Tq + iq, j8, Tk, kp);
#pragma unroll
                    for (int e = 0; e < 8; ++e) bits |= (kp[e] != 0.f ? 1u : 0u) << (8 * c + e);
                }
            }
        }
        f32x4 s[4], d[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) s[it] = d[it] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KS; ++k)
#pragma unroll
            for (int it = 0; it < 4; ++it)
                if (!a.causal || i0 + 16 * it + 15 + off >= kmin) {
                    s[it] = mfma_16x16x4(qs[(16 * it + li) * LD + 4 * k + g], kv[k], s[it]);
                    d[it] = mfma_16x16x4(gs[(16 * it + li) * LD + 4 * k + g], vv[k], d[it]);
                }
#pragma unroll
        for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int il = 16 * it + 4 * g + r, iq = i0 + il;
                const bool vis = iq < Tq && j < Tk && (!a.causal || j <= iq + off);
                const unsigned kb1 = dropping ? ((unsigned)__shfl((int)bits, il, 64) >> li) & 1u : 1u;
                const float p = expf((vis ? s[it][r] : -INFINITY) - lse_s[il]);
                const float kf = kb1 ? drop.inv : 0.f;
                s[it][r] = vis ? p * (d[it][r] * kf - del_s[il]) : 0.f;             // dS
                d[it][r] = p * kf;                                                   // P'
            }
#pragma unroll
        for (int it = 0; it < 4; ++it)
            if (!a.causal || i0 + 16 * it + 15 + off >= kmin) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float* qr = qs + (16 * it + 4 * g + r) * LD + li;
                    const float* gr = gs + (16 * it + 4 * g + r) * LD + li;
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) {
                        ak[ct] = mfma_16x16x4(qr[16 * ct], s[it][r], ak[ct]);
                        av[ct] = mfma_16x16x4(gr[16 * ct], d[it][r], av[ct]);
                    }
                }
            }
    }
    if (!(live && j < Tk)) return;
    float* dkb = dk + (size_t)b * sdk + (size_t)h * dh * Tk;
    float* dvb = dv + (size_t)b * sdv + (size_t)h * dh * Tk;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = 16 * ct + 4 * g + r;
            if (c < dh) {
                dkb[(size_t)c * Tk + j] = ak[ct][r];
                dvb[(size_t)c * Tk + j] = av[ct][r];
            }
        }
}

}  // namespace dynmm

using namespace dynmm;

#define ST ((hipStream_t)stream)

extern "C" int dynmm_attn_long_supported(int D, int Tq, int Tk, int heads) {
    if (D <= 0 || Tq <= 0 || Tk <= 0 || heads <= 0 || D % heads != 0) return 0;
    return (D / heads <= kAlMaxDh && Tq <= kAlMaxT && Tk <= kAlMaxT) ? 1 : 0;
}

// workgroups of a pass over T rows, or 0 when B * heads * ceil(T / 64) does not fit a grid
static unsigned al_grid(int B, int heads, int T) {
    const unsigned long long n = (unsigned long long)B * (unsigned long long)heads * (unsigned long long)ceil_div(T, kAlTile);
    return n < (1ull << 31) ? (unsigned)n : 0u;
}

// the instantiations: dh <= 4 (MULT's cross-modal transformers), <= 16 (its memory transformers: 12), <= 32, <= 64 (ef_tran: 60)
#define DYNMM_AL_DISPATCH(dh, CALL)          \
    do {                                     \
        if ((dh) <= 4) { CALL(4); }          \
        else if ((dh) <= 16) { CALL(16); }   \
        else if ((dh) <= 32) { CALL(32); }   \
        else { CALL(64); }                   \
    } while (0)

extern "C" int dynmm_attn_long_fwd(const float* q, const float* k, const float* v, long long q_bstride, long long k_bstride,
                                   long long v_bstride, float* out, float* lse, int B, int D, int Tq, int Tk, int heads, int causal,
                                   const dynmm_dropout* drop, void* stream) {
    (void)hipGetLastError();
    if (!q || !k || !v || !out || !lse || !attn_args_ok(B, D, Tq, Tk, heads, drop)) return DYNMM_EINVAL;
    if (!attn_bstrides_ok(D, Tq, Tk, q_bstride, k_bstride, v_bstride)) return DYNMM_EINVAL;
    const unsigned nq = al_grid(B, heads, Tq);
    if (!dynmm_attn_long_supported(D, Tq, Tk, heads) || !nq) return DYNMM_EUNSUPPORTED;
    const DropSpec spec = drop_spec(drop);
    const int dh = D / heads;
    const AlArgs a{q, k, v, (size_t)q_bstride, (size_t)k_bstride, (size_t)v_bstride, D, Tq, Tk, heads, causal ? 1 : 0,
                   attn_scale(dh)};
#define DYNMM_AL_F(DH) hipLaunchKernelGGL((al_fwd_kernel<DH>), dim3(nq), dim3(256), 0, ST, a, out, lse, ceil_div(Tq, kAlTile), spec)
    DYNMM_AL_DISPATCH(dh, DYNMM_AL_F);
#undef DYNMM_AL_F
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_attn_long_bwd(const float* g, const float* q, const float* k, const float* v, long long q_bstride,
                                   long long k_bstride, long long v_bstride, const float* out, const float* lse, float* dq,
                                   float* dk, float* dv, long long dq_bstride, long long dk_bstride, long long dv_bstride, int B,
                                   int D, int Tq, int Tk, int heads, int causal, const dynmm_dropout* drop, void* stream) {
    (void)hipGetLastError();
    if (!g || !q || !k || !v || !out || !lse || !dq || !dk || !dv || !attn_args_ok(B, D, Tq, Tk, heads, drop)) return DYNMM_EINVAL;
    if (!attn_bstrides_ok(D, Tq, Tk, q_bstride, k_bstride, v_bstride) ||
        !attn_bstrides_ok(D, Tq, Tk, dq_bstride, dk_bstride, dv_bstride))
        return DYNMM_EINVAL;
    const unsigned nq = al_grid(B, heads, Tq), nk = al_grid(B, heads, Tk);
    if (!dynmm_attn_long_supported(D, Tq, Tk, heads) || !nq || !nk) return DYNMM_EUNSUPPORTED;
    const DropSpec spec = drop_spec(drop);
    const int dh = D / heads;
    const AlArgs a{q, k, v, (size_t)q_bstride, (size_t)k_bstride, (size_t)v_bstride, D, Tq, Tk, heads, causal ? 1 : 0,
                   attn_scale(dh)};
#define DYNMM_AL_B(DH)                                                                                                         \
    do {                                                                                                                       \
        hipLaunchKernelGGL((al_bwd_dq_kernel<DH>), dim3(nq), dim3(256), 0, ST, a, g, out, lse, dq, (size_t)dq_bstride,         \
                           ceil_div(Tq, kAlTile), spec);                                                                       \
        hipLaunchKernelGGL((al_bwd_dkv_kernel<DH>), dim3(nk), dim3(256), 0, ST, a, g, out, lse, dk, dv, (size_t)dk_bstride,    \
                           (size_t)dv_bstride, ceil_div(Tk, kAlTile), spec);                                                   \
    } while (0)
    DYNMM_AL_DISPATCH(dh, DYNMM_AL_B);
#undef DYNMM_AL_B
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}
