// Multiplicative interactions fusion (MultiBench fusions.common_fusions.MultiplicativeInteractions2Modal, output='matrix';
// imdb_mm.py --fuse 3), forward and backward:
//   out[b,d] = sum_{n,m} m1[b,n] m2[b,m] W[n,m,d] + sum_m m2[b,m] V[m,d] + sum_n m1[b,n] U[n,d] + bias[d]
//   m1 [B, N], m2 [B, M], W [N, M, D], U [N, D], V [M, D], bias [D] -> out [B, D]
// Nothing of shape [B, M, D] or [B, N M] exists in memory, forward or backward.  Every index into W is 64-bit.
//
// Tiling (v_mfma_f32_32x32x2_f32; A: row = lane & 31, k = lane >> 5; B: k = lane >> 5, col = lane & 31; C/D: col = lane & 31,
// row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)).  Every workgroup is four waves on a 128 x 128 tile, each wave 2 x 2
// accumulators of 32 x 32.  Operand tiles are staged through LDS by 16-byte global loads (Tile; scalar loads when a row length
// is no multiple of four), unconditional on clamped addresses, with the elements past a tail zeroed afterwards.
//   forward   a GEMM over K = (n, m) whose A operand m1[b,n] m2[b,m] is made in registers: grid (D tiles, B tiles, n splits).
//             For 32 values of m the wave holds its m2 fragments in registers and walks the n of its split: the W tile
//             [32 m][128 d] of the next n is fetched while the current one multiplies (two LDS buffers, one barrier per tile).
//             Split s writes slab s + 1 of the workspace; slab 0 is the U, V, bias term (mim_lin_fwd_kernel); reduce_slabs sums
//             them in a fixed order.
//   weights   dW[n] = (m1[:, n] * m2)^T g: grid (M tiles, D tiles, n splits).  The m2 and g tiles of 128 samples stay in LDS for
//             the whole n range; m1[:, n] scales the A operand; the tile goes straight to dW (later sample chunks of a batch
//             above 128 add to what the same lane stored).  dU, dV, dbias: mim_small_grads_kernel.
//   inputs    T_n^T = W[n] g^T over K = D: grid (M tiles, B tiles, n splits).  W[n] and g tiles [128][32 d] are read back
//             from LDS 16 bytes per lane along d (the pairing of k within an MFMA is the same on both operands, so the sum is
//             over all d).  The epilogue of every n takes dm1[b,n] += sum_m m2[b,m] T (per M tile, a partial slab) and
//             dm2[b,m] += m1[b,n] T in accumulators (per n split, a partial slab).  reduce_slabs sums the slabs together with
//             the g U^T / g V^T slab of mim_lin_bwd_kernel.
// No floating-point atomics: equal inputs give equal bits.
#include "common.h"
#include "mfma.h"

namespace dynmm {
namespace {

constexpr int kThreads = 256;
constexpr int kBT = 128;                   // a workgroup's tile edge
constexpr int kKM = 32;                    // forward: values of m per W tile
constexpr int kKD = 32;                    // input pass: values of d per tile
constexpr int kPitchD = kKD + 4;           // its row pitch in floats: consecutive rows in consecutive 16-byte slots
constexpr int kNG = 8;                     // weight pass: columns of m1 per LDS trip
constexpr int kFwdGroups = 512;
constexpr int kWgradGroups = 256;          // one workgroup per CU: 132 KB of LDS
constexpr int kIgradGroups = 512;

// a macro: through mfma.h's inline wrapper the compiler allocates this file's registers differently
#define MIM_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

__device__ __forceinline__ void zero(f32x16 (&a)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) a[i][j][r] = 0.f;
}

// A thread's share of the R x C tile at (row0, col0) of a row-major [nrows, ncols] matrix: R C / 1024 pieces of four floats.
// VEC: ncols % 4 == 0, col0 % 4 == 0 and a 16-byte aligned base.
template <int R, int C, bool VEC>
struct Tile {
    static constexpr int kN = R * C / (4 * kThreads);
    float4 v[kN];

    __device__ __forceinline__ void load(const float* __restrict__ base, int nrows, int ncols, int row0, int col0, int tid) {
#pragma unroll
        for (int q = 0; q < kN; ++q) {
            const int idx = tid + q * kThreads, row = row0 + idx / (C / 4), col = col0 + 4 * (idx % (C / 4));
            const float* p = base + (size_t)min(row, nrows - 1) * ncols;
            float4 x;
            if constexpr (VEC) {
                x = *reinterpret_cast<const float4*>(p + min(col, ncols - 4));
                const bool ok = row < nrows && col < ncols;
                x.x = ok ? x.x : 0.f;
                x.y = ok ? x.y : 0.f;
                x.z = ok ? x.z : 0.f;
                x.w = ok ? x.w : 0.f;
            } else {
                x.x = p[min(col, ncols - 1)];
                x.y = p[min(col + 1, ncols - 1)];
                x.z = p[min(col + 2, ncols - 1)];
                x.w = p[min(col + 3, ncols - 1)];
                const bool rok = row < nrows;
                x.x = (rok && col < ncols) ? x.x : 0.f;
                x.y = (rok && col + 1 < ncols) ? x.y : 0.f;
                x.z = (rok && col + 2 < ncols) ? x.z : 0.f;
                x.w = (rok && col + 3 < ncols) ? x.w : 0.f;
            }
            v[q] = x;
        }
    }

    __device__ __forceinline__ void store(float* lds, int pitch, int tid) const {
#pragma unroll
        for (int q = 0; q < kN; ++q) {
            const int idx = tid + q * kThreads;
            *reinterpret_cast<float4*>(lds + (idx / (C / 4)) * pitch + 4 * (idx % (C / 4))) = v[q];
        }
    }
};

// ---- forward ------------------------------------------------------------------------------------------------------------
// part: the slabs [nsplit][B, D] of the n splits; per = values of n per split
template <bool VEC>
__global__ void __launch_bounds__(kThreads) mim_fwd_kernel(const float* __restrict__ m1, const float* __restrict__ m2,
                                                           const float* __restrict__ W, float* __restrict__ part, int B, int N,
                                                           int M, int D, int per) {
    __shared__ float smem[2][kKM * kBT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5, wr = wave >> 1, wc = wave & 1;
    const int d0 = blockIdx.x * kBT, b0 = blockIdx.y * kBT, split = blockIdx.z;
    const int n0 = split * per, nn = min(N, n0 + per) - n0;
    const int ntiles = (M + kKM - 1) / kKM * nn;
    const size_t slab = (size_t)M * D;
    int brc[2];
    bool bok[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const int b = b0 + wr * 64 + rt * 32 + i;
        bok[rt] = b < B;
        brc[rt] = min(b, B - 1);
    }
    f32x16 acc[2][2];
    zero(acc);
    Tile<kKM, kBT, VEC> t;
    t.load(W + (size_t)n0 * slab, M, D, 0, d0, tid);
    t.store(smem[0], kBT, tid);
    __syncthreads();
    float m2f[2][kKM / 2];
    int mc = 0, ni = 0;                      // tile idx = (chunk mc of m, n0 + ni), n fastest
    for (int idx = 0; idx < ntiles; ++idx) {
        if (ni == 0) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int s = 0; s < kKM / 2; ++s) {
                    const int k = mc * kKM + 2 * s + h;
                    const float v = m2[(size_t)brc[rt] * M + min(k, M - 1)];
                    m2f[rt][s] = (k < M && bok[rt]) ? v : 0.f;
                }
        }
        const float s0 = m1[(size_t)brc[0] * N + n0 + ni], s1 = m1[(size_t)brc[1] * N + n0 + ni];
        int nni = ni + 1, nmc = mc;
        if (nni == nn) {
            nni = 0;
            ++nmc;
        }
        const bool more = idx + 1 < ntiles;
        if (more) t.load(W + (size_t)(n0 + nni) * slab, M, D, nmc * kKM, d0, tid);
        const float* ws = smem[idx & 1] + wc * 64 + i;
#pragma unroll
        for (int s = 0; s < kKM / 2; ++s) {
            const float a0 = s0 * m2f[0][s], a1 = s1 * m2f[1][s];
            const float v0 = ws[(2 * s + h) * kBT], v1 = ws[(2 * s + h) * kBT + 32];
            acc[0][0] = MIM_MFMA(a0, v0, acc[0][0]);
            acc[0][1] = MIM_MFMA(a0, v1, acc[0][1]);
            acc[1][0] = MIM_MFMA(a1, v0, acc[1][0]);
            acc[1][1] = MIM_MFMA(a1, v1, acc[1][1]);
        }
        if (more) t.store(smem[(idx + 1) & 1], kBT, tid);
        __syncthreads();
        ni = nni;
        mc = nmc;
    }
    float* out = part + (size_t)split * B * D;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int b = b0 + wr * 64 + rt * 32 + acc_row(reg, h), d = d0 + wc * 64 + ct * 32 + i;
                if (b < B && d < D) out[(size_t)b * D + d] = acc[rt][ct][reg];
            }
}

// dst[b,d] = sum_n m1[b,n] U[n,d] + sum_m m2[b,m] V[m,d] + bias[d]: a workgroup owns 64 outputs of 4 samples; its four waves take
// every fourth k and their sums meet in LDS in a fixed order
__global__ void __launch_bounds__(kThreads) mim_lin_fwd_kernel(const float* __restrict__ m1, const float* __restrict__ m2,
                                                               const float* __restrict__ U, const float* __restrict__ V,
                                                               const float* __restrict__ bias, float* __restrict__ dst, int B,
                                                               int N, int M, int D) {
    __shared__ float red[4][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int d = blockIdx.x * 64 + lane, dc = min(d, D - 1), bq = blockIdx.y * 4;
    int bc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bc[r] = min(bq + r, B - 1);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k = wave; k < N; k += 4) {
        const float u = U[(size_t)k * D + dc];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += m1[(size_t)bc[r] * N + k] * u;
    }
#pragma unroll 4
    for (int k = wave; k < M; k += 4) {
        const float u = V[(size_t)k * D + dc];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += m2[(size_t)bc[r] * M + k] * u;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][r][lane] = acc[r];
    __syncthreads();
    const float v = (((red[0][wave][lane] + red[1][wave][lane]) + red[2][wave][lane]) + red[3][wave][lane]) + bias[dc];
    if (bq + wave < B && d < D) dst[(size_t)(bq + wave) * D + d] = v;
}

// ---- backward: weights --------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(kThreads) mim_wgrad_kernel(const float* __restrict__ m1, const float* __restrict__ m2,
                                                             const float* __restrict__ g, float* __restrict__ dW, int B, int N,
                                                             int M, int D, int per) {
    __shared__ float smem[2 * kBT * kBT + kBT * kNG];
    float* m2s = smem;                        // [128 samples][128 m]
    float* gs = smem + kBT * kBT;             // [128 samples][128 d]
    float* m1s = smem + 2 * kBT * kBT;        // [128 samples][kNG n]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5, wr = wave >> 1, wc = wave & 1;
    const int mt0 = blockIdx.x * kBT, d0 = blockIdx.y * kBT, split = blockIdx.z;
    const int n0 = split * per, n1 = min(N, n0 + per);
    const size_t slab = (size_t)M * D;
    for (int bc = 0; bc < B; bc += kBT) {
        const bool first = bc == 0;
        __syncthreads();
#pragma unroll 1
        for (int part = 0; part < 4; ++part) {
            Tile<32, kBT, VEC> ta, tb;
            ta.load(m2, B, M, bc + 32 * part, mt0, tid);
            tb.load(g, B, D, bc + 32 * part, d0, tid);
            ta.store(m2s + 32 * part * kBT, kBT, tid);
            tb.store(gs + 32 * part * kBT, kBT, tid);
        }
        const int ns = (min(kBT, B - bc) + 15) >> 4 << 3;          // k steps of two samples, a multiple of 8 (zero rows beyond B)
        for (int ng = n0; ng < n1; ng += kNG) {
            __syncthreads();
#pragma unroll
            for (int q = 0; q < kBT * kNG / kThreads; ++q) {
                const int e = tid + q * kThreads, b = bc + e / kNG, n = ng + e % kNG;
                const float v = m1[(size_t)min(b, B - 1) * N + min(n, N - 1)];
                m1s[e] = b < B ? v : 0.f;
            }
            __syncthreads();
            const int nj = min(kNG, n1 - ng);
            for (int j = 0; j < nj; ++j) {
                f32x16 acc[2][2];
                zero(acc);
                const float* ap = m2s + wr * 64 + i;
                const float* bp = gs + wc * 64 + i;
                for (int s8 = 0; s8 < ns; s8 += 8) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int k = 2 * (s8 + u) + h;
                        const float sc = m1s[k * kNG + j];
                        const float a0 = ap[k * kBT] * sc, a1 = ap[k * kBT + 32] * sc;
                        const float v0 = bp[k * kBT], v1 = bp[k * kBT + 32];
                        acc[0][0] = MIM_MFMA(a0, v0, acc[0][0]);
                        acc[0][1] = MIM_MFMA(a0, v1, acc[0][1]);
                        acc[1][0] = MIM_MFMA(a1, v0, acc[1][0]);
                        acc[1][1] = MIM_MFMA(a1, v1, acc[1][1]);
                    }
                }
                float* dst = dW + (size_t)(ng + j) * slab;
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                        for (int reg = 0; reg < 16; ++reg) {
                            const int m = mt0 + wr * 64 + rt * 32 + acc_row(reg, h), d = d0 + wc * 64 + ct * 32 + i;
                            if (m < M && d < D) {
                                float* p = dst + (size_t)m * D + d;
                                float v = acc[rt][ct][reg];
                                if (!first) v += *p;
                                *p = v;
                            }
                        }
            }
        }
    }
}

// rows r of [m1 | m2 | 1]^T g: dU [N, D], dV [M, D], dbias [D]; a thread owns one d of 8 rows
__global__ void __launch_bounds__(kThreads) mim_small_grads_kernel(const float* __restrict__ m1, const float* __restrict__ m2,
                                                                   const float* __restrict__ g, float* __restrict__ dU,
                                                                   float* __restrict__ dV, float* __restrict__ db, int B, int N,
                                                                   int M, int D) {
    const int d = blockIdx.x * kThreads + threadIdx.x, dc = min(d, D - 1);
    const int r0 = blockIdx.y * 8, R = N + M + 1;
    const float* xp[8];
    int xs[8];
    bool ones[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int r = min(r0 + q, R - 1);
        ones[q] = r == N + M;
        xp[q] = r < N ? m1 + r : (r < N + M ? m2 + (r - N) : m1);
        xs[q] = r < N ? N : (r < N + M ? M : 0);
    }
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < B; ++b) {
        const float gv = g[(size_t)b * D + dc];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float x = xp[q][(size_t)b * xs[q]];
            acc[q] += (ones[q] ? 1.f : x) * gv;
        }
    }
    if (d >= D) return;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int r = r0 + q;
        if (r < N)
            dU[(size_t)r * D + d] = acc[q];
        else if (r < N + M)
            dV[(size_t)(r - N) * D + d] = acc[q];
        else if (r == N + M)
            db[d] = acc[q];
    }
}

// ---- backward: inputs ---------------------------------------------------------------------------------------------------
// p1: slabs [M tiles][B, N] of dm1, p2: slabs [n splits][B, M] of dm2
template <bool VEC>
__global__ void __launch_bounds__(kThreads) mim_igrad_kernel(const float* __restrict__ m1, const float* __restrict__ m2,
                                                             const float* __restrict__ W, const float* __restrict__ g,
                                                             float* __restrict__ p1, float* __restrict__ p2, int B, int N, int M,
                                                             int D, int per) {
    __shared__ float smem[2 * 2 * kBT * kPitchD + 2 * kBT];
    float* red = smem + 2 * 2 * kBT * kPitchD;            // [2 waves along m][128 samples]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5, wr = wave >> 1, wc = wave & 1;
    const int mt0 = blockIdx.x * kBT, b0 = blockIdx.y * kBT, split = blockIdx.z;
    const int n0 = split * per, nn = min(N, n0 + per) - n0;
    const int nkc = (D + kKD - 1) / kKD, ntiles = nn * nkc;
    const size_t slab = (size_t)M * D;
    f32x16 acc[2][2], dm2a[2][2];
    zero(acc);
    zero(dm2a);
    Tile<kBT, kKD, VEC> tw, tg;
    tw.load(W + (size_t)n0 * slab, M, D, mt0, 0, tid);
    tg.load(g, B, D, b0, 0, tid);
    tw.store(smem, kPitchD, tid);
    tg.store(smem + kBT * kPitchD, kPitchD, tid);
    __syncthreads();
    int ni = 0, kc = 0;                      // tile idx = (n0 + ni, chunk kc of d), d fastest
    for (int idx = 0; idx < ntiles; ++idx) {
        int nkc_ = kc + 1, nni = ni;
        if (nkc_ == nkc) {
            nkc_ = 0;
            ++nni;
        }
        const bool more = idx + 1 < ntiles;
        if (more) {
            tw.load(W + (size_t)(n0 + nni) * slab, M, D, mt0, nkc_ * kKD, tid);
            tg.load(g, B, D, b0, nkc_ * kKD, tid);
        }
        const float* ws = smem + (idx & 1) * 2 * kBT * kPitchD + (wr * 64 + i) * kPitchD + 4 * h;
        const float* gt = smem + (idx & 1) * 2 * kBT * kPitchD + kBT * kPitchD + (wc * 64 + i) * kPitchD + 4 * h;
#pragma unroll
        for (int q = 0; q < kKD / 8; ++q) {
            const float4 a0 = *reinterpret_cast<const float4*>(ws + 8 * q);
            const float4 a1 = *reinterpret_cast<const float4*>(ws + 32 * kPitchD + 8 * q);
            const float4 v0 = *reinterpret_cast<const float4*>(gt + 8 * q);
            const float4 v1 = *reinterpret_cast<const float4*>(gt + 32 * kPitchD + 8 * q);
            const float a0s[4] = {a0.x, a0.y, a0.z, a0.w}, a1s[4] = {a1.x, a1.y, a1.z, a1.w};
            const float v0s[4] = {v0.x, v0.y, v0.z, v0.w}, v1s[4] = {v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc[0][0] = MIM_MFMA(a0s[u], v0s[u], acc[0][0]);
                acc[0][1] = MIM_MFMA(a0s[u], v1s[u], acc[0][1]);
                acc[1][0] = MIM_MFMA(a1s[u], v0s[u], acc[1][0]);
                acc[1][1] = MIM_MFMA(a1s[u], v1s[u], acc[1][1]);
            }
        }
        if (kc == nkc - 1) {
            // acc[rt][ct][reg] = T_n[b = b0 + 64 wc + 32 ct + i, m = mt0 + 64 wr + 32 rt + acc_row(reg, h)]; 0 past B and M
            const int n = n0 + ni;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const int bcl = min(b0 + wc * 64 + ct * 32 + i, B - 1);
                const float s = m1[(size_t)bcl * N + n];
                float p = 0.f;
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int m = mt0 + wr * 64 + rt * 32 + acc_row(reg, h);
                        const float x = m2[(size_t)bcl * M + min(m, M - 1)];
                        const float tv = acc[rt][ct][reg];
                        dm2a[rt][ct][reg] += s * tv;
                        p += (m < M ? x : 0.f) * tv;
                    }
                p += __shfl_xor(p, 32, 64);
                if (h == 0) red[wr * kBT + wc * 64 + ct * 32 + i] = p;
            }
            zero(acc);
            __syncthreads();
            if (p1 != nullptr && tid < kBT && b0 + tid < B)
                p1[((size_t)blockIdx.x * B + b0 + tid) * N + n] = red[tid] + red[kBT + tid];
        }
        if (more) {
            float* nx = smem + ((idx + 1) & 1) * 2 * kBT * kPitchD;
            tw.store(nx, kPitchD, tid);
            tg.store(nx + kBT * kPitchD, kPitchD, tid);
        }
        __syncthreads();
        ni = nni;
        kc = nkc_;
    }
    if (p2 == nullptr) return;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int b = b0 + wc * 64 + ct * 32 + i, m = mt0 + wr * 64 + rt * 32 + acc_row(reg, h);
                if (b < B && m < M) p2[((size_t)split * B + b) * M + m] = dm2a[rt][ct][reg];
            }
}

// dst[b, r] = sum_d g[b,d] X[r,d] for the rows r of X [R, D]: a workgroup owns one r, its waves every fourth sample
__global__ void __launch_bounds__(kThreads) mim_lin_bwd_kernel(const float* __restrict__ g, const float* __restrict__ X,
                                                               float* __restrict__ dst, int B, int R, int D) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = blockIdx.x;
    const float* xr = X + (size_t)r * D;
    for (int b = wave; b < B; b += 4) {
        const float* gr = g + (size_t)b * D;
        float s = 0.f;
        for (int d = lane; d < D; d += 64) s += gr[d] * xr[d];
        s = wave_reduce_sum(s);
        if (lane == 0) dst[(size_t)b * R + r] = s;
    }
}

struct Split {
    int n, per;
};

// n splits of `per` values each (the last may hold fewer, none is empty)
Split make_split(int N, int want) {
    int n = want < 1 ? 1 : (want > N ? N : want);
    const int per = ceil_div(N, n);
    n = ceil_div(N, per);
    return Split{n, per};
}

Split fwd_split(int B, int N, int D) { return make_split(N, kFwdGroups / (ceil_div(B, kBT) * ceil_div(D, kBT))); }
Split wgrad_split(int N, int M, int D) { return make_split(N, kWgradGroups / (ceil_div(M, kBT) * ceil_div(D, kBT))); }
Split igrad_split(int B, int N, int M) { return make_split(N, kIgradGroups / (ceil_div(B, kBT) * ceil_div(M, kBT))); }

size_t round4(size_t n) { return (n + 3) & ~(size_t)3; }

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int check_shapes(int B, int N, int M, int D) {
    if (B <= 0 || N <= 0 || M <= 0 || D <= 0) return DYNMM_EINVAL;
    const size_t lim = (size_t)1 << 31;
    // W itself may hold any number of elements; what is indexed in 32 bits or goes through reduce_slabs must fit
    if ((size_t)B * D >= lim || (size_t)B * N >= lim || (size_t)B * M >= lim || (size_t)N + M + 1 >= lim) return DYNMM_EUNSUPPORTED;
    if (ceil_div(B, 4) > 65535 || ceil_div(D, kBT) > 65535 || ((size_t)N + M + 8) / 8 > 65535)
        return DYNMM_EUNSUPPORTED;
    return DYNMM_OK;
}

}  // namespace
}  // namespace dynmm

using namespace dynmm;

extern "C" size_t dynmm_mim_fwd_workspace_bytes(int B, int N, int M, int D) {
    if (check_shapes(B, N, M, D)) return 0;
    return ((size_t)fwd_split(B, N, D).n + 1) * B * D * sizeof(float);
}

extern "C" int dynmm_mim_fwd(const float* m1, const float* m2, const float* W, const float* U, const float* V, const float* bias,
                             float* out, float* workspace, size_t workspace_bytes, int B, int N, int M, int D, void* stream) {
    (void)hipGetLastError();
    const int s = check_shapes(B, N, M, D);
    if (s) return s;
    if (!m1 || !m2 || !W || !U || !V || !bias || !out) return DYNMM_EINVAL;
    if (!workspace || workspace_bytes < dynmm_mim_fwd_workspace_bytes(B, N, M, D)) return DYNMM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Split sp = fwd_split(B, N, D);
    hipLaunchKernelGGL(mim_lin_fwd_kernel, dim3(ceil_div(D, 64), ceil_div(B, 4)), dim3(kThreads), 0, st, m1, m2, U, V, bias,
                       workspace, B, N, M, D);
    DYNMM_LAUNCH_CHECK();
    float* part = workspace + (size_t)B * D;
    const dim3 grid(ceil_div(D, kBT), ceil_div(B, kBT), sp.n);
    if (D % 4 == 0 && aligned16(W))
        hipLaunchKernelGGL(mim_fwd_kernel<true>, grid, dim3(kThreads), 0, st, m1, m2, W, part, B, N, M, D, sp.per);
    else
        hipLaunchKernelGGL(mim_fwd_kernel<false>, grid, dim3(kThreads), 0, st, m1, m2, W, part, B, N, M, D, sp.per);
    DYNMM_LAUNCH_CHECK();
    launch_reduce_slabs(workspace, out, B * D, sp.n + 1, st);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

// [g U^T | dm1 slabs of the M tiles] then [g V^T | dm2 slabs of the n splits]
extern "C" size_t dynmm_mim_bwd_workspace_bytes(int B, int N, int M, int D) {
    if (check_shapes(B, N, M, D)) return 0;
    const size_t n1 = round4(((size_t)ceil_div(M, kBT) + 1) * B * N);
    const size_t n2 = round4(((size_t)igrad_split(B, N, M).n + 1) * B * M);
    return (n1 + n2) * sizeof(float);
}

extern "C" int dynmm_mim_bwd(const float* g, const float* m1, const float* m2, const float* W, const float* U, const float* V,
                             float* dm1, float* dm2, float* dW, float* dU, float* dV, float* dbias, float* workspace,
                             size_t workspace_bytes, int B, int N, int M, int D, void* stream) {
    (void)hipGetLastError();
    const int s = check_shapes(B, N, M, D);
    if (s) return s;
    if (!g || !m1 || !m2 || !W || !U || !V) return DYNMM_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (dW) {
        // parameter gradients: all of them or none
        if (!dU || !dV || !dbias) return DYNMM_EINVAL;
        const Split sp = wgrad_split(N, M, D);
        const dim3 grid(ceil_div(M, kBT), ceil_div(D, kBT), sp.n);
        if (D % 4 == 0 && M % 4 == 0 && aligned16(m2) && aligned16(g))
            hipLaunchKernelGGL(mim_wgrad_kernel<true>, grid, dim3(kThreads), 0, st, m1, m2, g, dW, B, N, M, D, sp.per);
        else
            hipLaunchKernelGGL(mim_wgrad_kernel<false>, grid, dim3(kThreads), 0, st, m1, m2, g, dW, B, N, M, D, sp.per);
        DYNMM_LAUNCH_CHECK();
        hipLaunchKernelGGL(mim_small_grads_kernel, dim3(ceil_div(D, kThreads), ceil_div(N + M + 1, 8)), dim3(kThreads), 0, st,
                           m1, m2, g, dU, dV, dbias, B, N, M, D);
        DYNMM_LAUNCH_CHECK();
    }
    if (dm1 || dm2) {
        if (!workspace || workspace_bytes < dynmm_mim_bwd_workspace_bytes(B, N, M, D)) return DYNMM_EWORKSPACE;
        const Split sp = igrad_split(B, N, M);
        const int mt = ceil_div(M, kBT);
        float* w1 = workspace;
        float* w2 = workspace + round4(((size_t)mt + 1) * B * N);
        float* p1 = dm1 ? w1 + (size_t)B * N : nullptr;
        float* p2 = dm2 ? w2 + (size_t)B * M : nullptr;
        if (dm1) {
            hipLaunchKernelGGL(mim_lin_bwd_kernel, dim3(N), dim3(kThreads), 0, st, g, U, w1, B, N, D);
            DYNMM_LAUNCH_CHECK();
        }
        if (dm2) {
            hipLaunchKernelGGL(mim_lin_bwd_kernel, dim3(M), dim3(kThreads), 0, st, g, V, w2, B, M, D);
            DYNMM_LAUNCH_CHECK();
        }
        const dim3 grid(mt, ceil_div(B, kBT), sp.n);
        if (D % 4 == 0 && aligned16(W) && aligned16(g))
            hipLaunchKernelGGL(mim_igrad_kernel<true>, grid, dim3(kThreads), 0, st, m1, m2, W, g, p1, p2, B, N, M, D, sp.per);
        else
            hipLaunchKernelGGL(mim_igrad_kernel<false>, grid, dim3(kThreads), 0, st, m1, m2, W, g, p1, p2, B, N, M, D, sp.per);
        DYNMM_LAUNCH_CHECK();
        if (dm1) {
            launch_reduce_slabs(w1, dm1, B * N, mt + 1, st);
            DYNMM_LAUNCH_CHECK();
        }
        if (dm2) {
            launch_reduce_slabs(w2, dm2, B * M, sp.n + 1, st);
            DYNMM_LAUNCH_CHECK();
        }
    }
    return DYNMM_OK;
}
