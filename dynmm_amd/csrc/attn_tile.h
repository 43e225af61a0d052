// What the attention families share: the tile helpers of the matrix-core kernels (attn.hip's whole rows, attn_long.hip's streamed
// tiles), the causal mask rule and the host-side argument checks of the entry points with separate query and key lengths
// (xattn.hip, attn_long.hip).  One definition each: the families' dropout decisions and masks must agree bit for bit.
#pragma once
#include <math.h>

#include "common.h"
#include "dropout.h"
#include "mfma.h"

namespace dynmm {

// A 16-token x DH-channel operand tile, token-major in LDS ([token][LD]; attn.hip's header has the bank arithmetic).
template <int DH>
struct AttnShape {
    static constexpr int KS = (DH + 3) / 4;        // k-steps of a product over the channels
    static constexpr int CT = (DH + 15) / 16;      // 16-channel tiles of a product over tokens
    static constexpr int LD = 16 * CT + 4;         // 4 (mod 16)
};

// v where ok, else +0.  A bit mask, not a select on the loaded value: a select lets the compiler sink the load into a branch on
// `ok`, which is the predicated load these kernels must not have.
__device__ __forceinline__ float attn_keep_if(float v, bool ok) { return __uint_as_float(__float_as_uint(v) & (ok ? ~0u : 0u)); }

// Staging of tokens t0 + 16 w .. t0 + 16 w + 15 of src [channel][T] into rows 16 w .. 16 w + 15 of a token-major tile [.][LD]:
// wave w's lanes take token t0 + 16 w + (lane & 15), channels 4 s + (lane >> 4).  attn_load issues the KS loads of a lane
// (unconditional, on clamped addresses; nothing depends on them yet, so the loads of ALL the tensors of a kernel are in flight
// together), attn_store writes the values, or zeros outside (T, dh): every channel below 16 CT is written.
template <int DH>
__device__ __forceinline__ void attn_load(const float* __restrict__ src, float (&v)[AttnShape<DH>::KS], int dh, int T, int t0,
                                          int w, int lane) {
    const int tc = min(t0 + 16 * w + (lane & 15), T - 1), g = lane >> 4;
#pragma unroll
    for (int s = 0; s < AttnShape<DH>::KS; ++s) v[s] = src[(size_t)min(4 * s + g, dh - 1) * T + tc];
}
template <int DH>
__device__ __forceinline__ void attn_store(float* dst, const float (&v)[AttnShape<DH>::KS], int dh, int T, int t0, int w, int lane,
                                           float mul) {
    constexpr int KS = AttnShape<DH>::KS, CT = AttnShape<DH>::CT, LD = AttnShape<DH>::LD;
    const int t = 16 * w + (lane & 15), g = lane >> 4;
#pragma unroll
    for (int s = 0; s < 4 * CT; ++s)
        dst[t * LD + 4 * s + g] = s < KS ? attn_keep_if(v[s < KS ? s : 0] * mul, t0 + t < T && 4 * s + g < dh) : 0.f;
}

// The keep decisions of a query's 64 keys (eight 8-key chunks) are drawn ONCE (a Philox call is ~900 issue cycles), two chunks by
// each of the query's four lanes g = lane >> 4: bits e of byte 0 / 1 = keys 8 j8 + e of query row `row` (DropState::row8, seq.hip's
// indexing), j8 = j8g / j8g + 4, where j8g = (the first chunk of the 64 keys) + g.  Chunks that begin at or past the end of the
// query's keys are not drawn: Tk, or with MASKED jvis, the end of its visible keys.  (A template, not a bound every caller
// passes: this function is simplified before it is inlined, and only where the bound IS the row length does row8's own `j < Tk`
// of a chunk's first key fold into the test here; attn.hip's kernels compile to other, longer code when handed T twice.)
template <bool MASKED = false>
__device__ __forceinline__ unsigned attn_draw(const DropState& drop, size_t row, int Tk, int j8g, int jvis = 0) {
    const int end = MASKED ? jvis : Tk;
    unsigned bits = 0u;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int j8 = j8g + 4 * s;
        if (8 * j8 < end) {
            float kp[8];
            drop.row8(row, j8, Tk, kp);
#pragma unroll
            for (int e = 0; e < 8; ++e) bits |= (kp[e] != 0.f ? 1u : 0u) << (8 * s + e);
        }
    }
    return bits;
}
// the four decisions of keys 16 jt + 4 g + r (bit r) of the 64, from the lane of this query that drew their chunk
__device__ __forceinline__ unsigned attn_keep4(unsigned bits, int jt, int lane) {
    const int g = lane >> 4;
    const int chunk = 2 * jt + (g >> 1);
    const unsigned v = (unsigned)__shfl((int)bits, (lane & 15) + 16 * (chunk & 3), 64);
    return (v >> (8 * (chunk >> 2) + 4 * (g & 1))) & 0xfu;
}

// maximum / sum over the four lanes (lane & 15, g = 0 .. 3) that share a query
__device__ __forceinline__ float attn_query_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float attn_query_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// The causal mask: key j is visible to query i iff j <= i + off, off = |Tk - Tq| (torch.triu(-inf, 1 + |Tk - Tq|)); key 0 is
// always visible, no row is empty.  Keys 0 .. attn_visible - 1 are visible to query i.
__device__ __forceinline__ int attn_visible(int i, int off, int Tk) { return min(Tk, i + off + 1); }

// ---------------------------------------------------------------------------------------------------------------
// host: the checks of the q / k / v entry points, in the order they are made
// ---------------------------------------------------------------------------------------------------------------
static inline bool attn_args_ok(int B, int D, int Tq, int Tk, int heads, const dynmm_dropout* drop) {
    return B > 0 && D > 0 && Tq > 0 && Tk > 0 && heads > 0 && D % heads == 0 && drop_ok(drop);
}
// a sample of q (dq) holds D x Tq values, one of k, v (dk, dv) D x Tk
static inline bool attn_bstrides_ok(int D, int Tq, int Tk, long long sq, long long sk, long long sv) {
    return sq >= (long long)D * Tq && sk >= (long long)D * Tk && sv >= (long long)D * Tk;
}
// 1 / sqrt(dh), correctly rounded (the device's reciprocal square root is not)
static inline float attn_scale(int dh) { return (float)(1.0 / sqrt((double)dh)); }

}  // namespace dynmm
