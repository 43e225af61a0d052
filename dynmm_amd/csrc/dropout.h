// Dropout with regenerated keep decisions (Philox sites), shared by the sequence kernels (seq.hip, seq_ffn.hip, attn.hip) and
// the MaxOut_MLP kernels (mlp.hip); the one Philox-4x32-10 of the library (gate_se.hip draws its Gumbel noise from it too).
#pragma once
#include "common.h"

namespace dynmm {

// ---------------------------------------------------------------------------------------------------------------
// Dropout (nn.TransformerEncoderLayer trains with p = 0.1 at four places: the attention probabilities, the attention
// block's output, the feed-forward hidden layer and the feed-forward output).  An element survives with probability
// 1 - p and is scaled by 1/(1 - p).  The decision for element `idx` of a site is a pure function of
// (seed, offset + *step, idx) through Philox-4x32-10, so the backward pass regenerates it instead of storing masks and a
// captured hipGraph draws new masks at every replay (`step` is a device counter the training step advances).
// `mask` (tests): explicit keep flags, one byte per element, instead of the generator.
// ---------------------------------------------------------------------------------------------------------------
struct DropSpec {
    const unsigned char* mask;
    const unsigned long long* step;
    unsigned long long seed, offset;
    float p;
};

// The kernels' DropSpec of an entry point's dynmm_dropout: all zero (no dropout) for none or p = 0.
static inline DropSpec drop_spec(const dynmm_dropout* d) {
    DropSpec s{};
    if (d && d->p > 0.f) {
        s.mask = d->mask; s.step = d->step; s.seed = d->seed; s.offset = d->offset; s.p = d->p;
    }
    return s;
}
static inline bool drop_ok(const dynmm_dropout* d) { return !d || (d->p >= 0.f && d->p < 1.f); }

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// 0 (dropped) or 1/(1-p) (kept); 1 when the site has no dropout.
// A Philox call costs a wave ~900 issue cycles (forty quarter-rate 32-bit multiplies): the shaped accessors below draw
// EIGHT decisions from one call (16 random bits each, keep iff u16 >= round(65536 p), as ffn_kernel does) for the eight
// elements a lane owns — eight consecutive channels of a token (LayerNorm sites) or eight consecutive keys of a query row
// (attention probabilities).  A site is read through ONE accessor by its forward and backward kernels; which element a
// counter serves is therefore a property of the site's kernel family, not of the flat index.
struct DropState {
    const unsigned char* mask;
    unsigned long long off;
    uint32_t k0, k1, thr16;
    float p, inv;
    __device__ __forceinline__ explicit DropState(const DropSpec& d)
        : mask(d.mask), off(d.offset + (d.step ? *d.step : 0ull)), k0((uint32_t)d.seed), k1((uint32_t)(d.seed >> 32)),
          thr16((uint32_t)(d.p * 65536.f + 0.5f)), p(d.p), inv(d.p > 0.f ? 1.f / (1.f - d.p) : 1.f) {}
    // flat sites (dropout_kernel): element idx = counter idx, 24 random bits
    __device__ __forceinline__ float operator()(size_t idx) const {
        if (!(p > 0.f)) return 1.f;
        if (mask) return mask[idx] ? inv : 0.f;
        uint32_t r[4];
        philox4x32_10((uint32_t)idx, (uint32_t)((unsigned long long)idx >> 32), (uint32_t)off, (uint32_t)(off >> 32), k0, k1, r);
        const float u = (float)(r[0] >> 8) * (1.f / 16777216.f);        // [0, 1)
        return u >= p ? inv : 0.f;
    }
    __device__ __forceinline__ void philox8(unsigned long long ctr, float k[8]) const {
        uint32_t r[4];
        philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)off, (uint32_t)(off >> 32), k0, k1, r);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            k[2 * q] = (r[q] & 0xffffu) >= thr16 ? inv : 0.f;
            k[2 * q + 1] = (r[q] >> 16) >= thr16 ? inv : 0.f;
        }
    }
    // [B, D, T] sites: channels 8 c8 ... 8 c8 + 7 of token (b, t).  Injected flags are indexed by the tensor's flat layout.
    __device__ __forceinline__ void keep8(int b, int c8, int t, int D, int T, float k[8]) const {
        if (!(p > 0.f)) {
#pragma unroll
            for (int e = 0; e < 8; ++e) k[e] = 1.f;
        } else if (mask) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = c8 * 8 + e;
                k[e] = (c < D && mask[((size_t)b * D + c) * T + t]) ? inv : 0.f;
            }
        } else {
            philox8(((unsigned long long)b * ((D + 7) / 8) + c8) * T + t, k);
        }
    }
    __device__ __forceinline__ float keep1(int b, int c, int t, int D, int T) const {
        if (!(p > 0.f)) return 1.f;
        if (mask) return mask[((size_t)b * D + c) * T + t] ? inv : 0.f;
        float k[8];
        philox8(((unsigned long long)b * ((D + 7) / 8) + (c >> 3)) * T + t, k);
        float r = k[0];
#pragma unroll
        for (int e = 1; e < 8; ++e) r = (c & 7) == e ? k[e] : r;
        return r;
    }
    // [R, T] sites (attention probabilities, R = B * heads * T query rows): keys 8 j8 ... 8 j8 + 7 of row r
    __device__ __forceinline__ void row8(size_t r, int j8, int T, float k[8]) const {
        if (!(p > 0.f)) {
#pragma unroll
            for (int e = 0; e < 8; ++e) k[e] = 1.f;
        } else if (mask) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int j = j8 * 8 + e;
                k[e] = (j < T && mask[r * T + j]) ? inv : 0.f;
            }
        } else {
            philox8((unsigned long long)r * ((T + 7) / 8) + j8, k);
        }
    }
};

}  // namespace dynmm
