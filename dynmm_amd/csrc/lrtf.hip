// Low-rank tensor fusion (MultiBench fusions.common_fusions.LowRankTensorFusion; imdb_mm.py --fuse 2, affect_mm.py --fusion 5),
// forward and backward, for M = 2 or 3 modalities:
//   P_m[r,b,o] = F_m[r,0,o] + sum_k z_m[b,k] F_m[r,k+1,o]        z_m [B, d_m], F_m [R, d_m + 1, O]
//   out[b,o]   = sum_r w[r] prod_m P_m[r,b,o] + bias[o]          -> [B, O]
// No [R, B, O] tensor exists in memory, forward or backward: P_m lives in MFMA accumulators and is recomputed by the backward.
//
// Tiling (v_mfma_f32_16x16x4_f32; A: row = lane & 15, k = lane >> 4; B: k = lane >> 4, col = lane & 15; C/D: row = 4 (lane >> 4)
// + register, col = lane & 15).  A wave computes a 32-sample x 32-output tile of every P_m of one rank (p_tiles: 2 x 2
// accumulators per modality, rows = samples, columns = outputs, initialised with the factor's row 0).  The backward's p_tiles
// reads both operands straight from global memory: the factor rows are contiguous in o, and a z line is re-used by the next k
// steps out of L1.
//   forward   grid (output tiles, sample tiles, rank splits); the four waves of a workgroup share the sample and output tile and
//             take every fourth rank of the split, so the z tile goes through LDS (lrtf_fwd_kernel) while the factor rows come
//             from global memory; the waves multiply their P_m elementwise, scale by w[r] and accumulate, and the four sums meet
//             in LDS in a fixed order.  With one split the result (+ bias) is the output; with more, every split writes a
//             partial slab and reduce_slabs sums them.
//   factors   grid (output tiles, ranks): the workgroup owns dF_m[r, :, 32 outputs] of every m and walks the samples 128 at a
//             time: phase 1 = the P tiles and dP_m = g w[r] prod_{n != m} P_n into LDS (each wave 32 samples), phase 2 = dF_m +=
//             z_m^T dP_m (contraction over the samples; the 16-feature tiles dealt to the waves) and the column sums for row 0.
//             Nobody else touches the slab: no atomics, later sample chunks add to what the same lane stored before.
//   inputs    grid (sample tiles, rank splits): dz_m[b,k] = sum_{r,o} dP_m[b,o] F_m[r,k+1,o].  Per rank and 128 outputs: phase 1
//             as above (each wave 32 outputs), phase 2 = dP_m F_m^T (contraction over the outputs) added into the split's own
//             partial slab; reduce_slabs sums the splits.  Modalities whose input needs no gradient are skipped.
// dw[r] = sum g prod_m P_m: per-workgroup sums of the factor kernel, reduced over the output tiles in a fixed order.
// All loads are unconditional on clamped addresses; the value is selected afterwards (sample, output and k tails).
#include "common.h"
#include "mfma.h"

namespace dynmm {
namespace {

constexpr int kMaxM = 3;
constexpr int kThreads = 256;
constexpr int kTile = 32;                  // a wave's tile: 32 samples x 32 outputs
constexpr int kChunk = 4 * kTile;          // samples (factor kernel) / outputs (input kernel) per phase-1 pass of a workgroup
constexpr int kZChunk = 128;               // forward: features of the z tile per LDS trip
constexpr int kZStride = kZChunk + 4;      // its row pitch in floats
constexpr int kTargetGroups = 1024;        // four workgroups (16 waves) per CU

struct Args {
    const float* z[kMaxM];
    const float* f[kMaxM];
    int d[kMaxM];
    const float* w;
    const float* bias;
    int B, O, R;
};

struct Ptrs {
    float* p[kMaxM];
};

// acc[m][i][j][reg] = P_m[r, b0 + 16 i + 4 (lane >> 4) + reg, o0 + 16 j + (lane & 15)] (rows / columns past B / O: clamped copies)
template <int M>
__device__ __forceinline__ void p_tiles(const Args& a, int r, int b0, int o0, int lane, f32x4 (&acc)[M][2][2]) {
    const int col = lane & 15, kq = lane >> 4;
    const int oc0 = min(o0 + col, a.O - 1), oc1 = min(o0 + 16 + col, a.O - 1);
    const int bc0 = min(b0 + col, a.B - 1), bc1 = min(b0 + 16 + col, a.B - 1);
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int d = a.d[m];
        const float* F = a.f[m] + (size_t)r * (d + 1) * a.O;
        const float* z0 = a.z[m] + (size_t)bc0 * d;
        const float* z1 = a.z[m] + (size_t)bc1 * d;
        const float f0 = F[oc0], f1 = F[oc1];
        f32x4 c00 = {f0, f0, f0, f0}, c01 = {f1, f1, f1, f1}, c10 = c00, c11 = c01;
        // four k steps per trip, so that their sixteen loads are in flight together; steps past d are clamped loads times zero
        const int nk16 = (d + 15) >> 4;
        for (int kb = 0; kb < nk16; ++kb) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = 16 * kb + 4 * u + kq, kcl = min(k, d - 1);
                float a0 = z0[kcl], a1 = z1[kcl];
                a0 = k < d ? a0 : 0.f;
                a1 = k < d ? a1 : 0.f;
                const float* Fr = F + (size_t)(kcl + 1) * a.O;
                const float v0 = Fr[oc0], v1 = Fr[oc1];
                c00 = mfma_16x16x4(a0, v0, c00);
                c01 = mfma_16x16x4(a0, v1, c01);
                c10 = mfma_16x16x4(a1, v0, c10);
                c11 = mfma_16x16x4(a1, v1, c11);
            }
        }
        acc[m][0][0] = c00;
        acc[m][0][1] = c01;
        acc[m][1][0] = c10;
        acc[m][1][1] = c11;
    }
}

// dst = out (one split: + bias) or the partial slabs [nsplit][B, O] (bias in slab 0).  per = ranks per split.
// The four waves of the workgroup share the sample tile and differ in the rank, so the z tile goes through LDS: 32 samples x
// kZChunk features per trip, loaded coalesced along k by all 256 threads into one of two buffers (one barrier per trip; the rows
// are 132 floats apart, which spreads a wave's A operand over all 64 banks).  Columns past d_m are stored as zeros.  A wave
// without a rank of its own (the split's remainder) walks a clamped rank with weight 0, so every wave meets every barrier.
template <int M>
__global__ void __launch_bounds__(kThreads) lrtf_fwd_kernel(Args a, float* __restrict__ dst, int per) {
    __shared__ float smem[2 * kTile * kZStride];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4;
    const int o0 = blockIdx.x * kTile, b0 = blockIdx.y * kTile, split = blockIdx.z;
    const int rs0 = split * per, rs1 = min(a.R, rs0 + per);
    const int oc0 = min(o0 + col, a.O - 1), oc1 = min(o0 + 16 + col, a.O - 1);
    const int lrow = tid >> 7, lk = tid & (kZChunk - 1);                 // the loader's element: rows lrow + 2 q, column lk
    f32x4 s[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) s[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    int trip = 0;
    for (int rg = rs0; rg < rs1; rg += 4) {
        const bool live = rg + wave < rs1;
        const int r = live ? rg + wave : rs1 - 1;
        f32x4 prod[2][2];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const int d = a.d[m];
            const float* F = a.f[m] + (size_t)r * (d + 1) * a.O;
            const float* zm = a.z[m];
            const float f0 = F[oc0], f1 = F[oc1];
            f32x4 c00 = {f0, f0, f0, f0}, c01 = {f1, f1, f1, f1}, c10 = c00, c11 = c01;
            for (int k0 = 0; k0 < d; k0 += kZChunk, ++trip) {
                float* buf = smem + (trip & 1) * kTile * kZStride;
                {
                    const int k = k0 + lk, kcl = min(k, d - 1);
                    float v[kTile / 2];
#pragma unroll
                    for (int q = 0; q < kTile / 2; ++q) v[q] = zm[(size_t)min(b0 + lrow + 2 * q, a.B - 1) * d + kcl];
#pragma unroll
                    for (int q = 0; q < kTile / 2; ++q) buf[(lrow + 2 * q) * kZStride + lk] = k < d ? v[q] : 0.f;
                }
                __syncthreads();
                const int nk16 = (min(kZChunk, d - k0) + 15) >> 4;
                for (int kb = 0; kb < nk16; ++kb) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int kl = 16 * kb + 4 * u + kq;
                        const float a0 = buf[col * kZStride + kl], a1 = buf[(16 + col) * kZStride + kl];
                        const float* Fr = F + (size_t)(min(k0 + kl, d - 1) + 1) * a.O;
                        const float v0 = Fr[oc0], v1 = Fr[oc1];
                        c00 = mfma_16x16x4(a0, v0, c00);
                        c01 = mfma_16x16x4(a0, v1, c01);
                        c10 = mfma_16x16x4(a1, v0, c10);
                        c11 = mfma_16x16x4(a1, v1, c11);
                    }
                }
            }
            prod[0][0] = m == 0 ? c00 : prod[0][0] * c00;
            prod[0][1] = m == 0 ? c01 : prod[0][1] * c01;
            prod[1][0] = m == 0 ? c10 : prod[1][0] * c10;
            prod[1][1] = m == 0 ? c11 : prod[1][1] * c11;
        }
        const float wv = a.w[r];
        const float wr = live ? wv : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) s[i][j] += wr * prod[i][j];
    }
    __syncthreads();                                     // the z buffers become the four waves' sums [4][16][64]
    float* red = smem;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) red[(wave * 16 + (2 * i + j) * 4 + reg) * 64 + lane] = s[i][j][reg];
    __syncthreads();
    const int i = wave >> 1, j = wave & 1;              // wave w finishes sub-tile (w >> 1, w & 1)
    float* out = dst + (size_t)split * a.B * a.O;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int q = (wave * 4 + reg) * 64 + lane;
        float v = ((red[q] + red[16 * 64 + q]) + red[2 * 16 * 64 + q]) + red[3 * 16 * 64 + q];
        const int b = b0 + 16 * i + 4 * kq + reg, o = o0 + 16 * j + col;
        const float bv = a.bias[min(o, a.O - 1)];
        v += split == 0 ? bv : 0.f;
        if (b < a.B && o < a.O) out[(size_t)b * a.O + o] = v;
    }
}

// g masked to the tile's valid elements
__device__ __forceinline__ float g_at(const float* __restrict__ g, int b, int o, int B, int O) {
    const float v = g[(size_t)min(b, B - 1) * O + min(o, O - 1)];
    return (b < B && o < O) ? v : 0.f;
}

// the product of p[n], n != m
template <int M>
__device__ __forceinline__ float others(const float (&p)[M], int m) {
    float v = 1.f;
    bool any = false;
#pragma unroll
    for (int n = 0; n < M; ++n)
        if (n != m) {
            v = any ? v * p[n] : p[n];
            any = true;
        }
    return v;
}

// factor gradients and the per-workgroup sums of dw: grid (output tiles, R)
template <int M>
__global__ void __launch_bounds__(kThreads) lrtf_bwd_factor_kernel(Args a, const float* __restrict__ g, Ptrs df,
                                                                   float* __restrict__ dwpart) {
    __shared__ float dps[M][kChunk][kTile];
    __shared__ float wred[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4;
    const int o0 = blockIdx.x * kTile, r = blockIdx.y;
    const int B = a.B, O = a.O;
    const float wr = a.w[r];
    float dwp = 0.f;
    for (int cb = 0; cb < B; cb += kChunk) {
        const bool first = cb == 0;
        {
            const int b0 = cb + kTile * wave;
            f32x4 acc[M][2][2];
            p_tiles<M>(a, r, b0, o0, lane, acc);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int bl = 16 * i + 4 * kq + reg, ol = 16 * j + col;
                        const float gv = g_at(g, b0 + bl, o0 + ol, B, O);
                        float p[M];
                        float all = 1.f;
#pragma unroll
                        for (int m = 0; m < M; ++m) {
                            p[m] = acc[m][i][j][reg];
                            all = m == 0 ? p[0] : all * p[m];
                        }
                        dwp += gv * all;
                        const float gw = gv * wr;
#pragma unroll
                        for (int m = 0; m < M; ++m) dps[m][kTile * wave + bl][ol] = gw * others<M>(p, m);
                    }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const int d = a.d[m], nkf = (d + 15) >> 4;
            float* dF = df.p[m] + (size_t)r * (d + 1) * O;
            const float* zm = a.z[m];
            for (int kt = wave; kt < nkf; kt += 4) {
                const int kf = 16 * kt + col, kfc = min(kf, d - 1);
                f32x4 e0 = {0.f, 0.f, 0.f, 0.f}, e1 = e0;
#pragma unroll 8
                for (int s = 0; s < kChunk / 4; ++s) {
                    const int bl = 4 * s + kq, b = cb + bl;
                    float av = zm[(size_t)min(b, B - 1) * d + kfc];        // A[row = feature][k = sample]
                    av = (b < B && kf < d) ? av : 0.f;
                    e0 = mfma_16x16x4(av, dps[m][bl][col], e0);               // B[k = sample][col = output]
                    e1 = mfma_16x16x4(av, dps[m][bl][16 + col], e1);
                }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int kfo = 16 * kt + 4 * kq + reg;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int o = o0 + 16 * j + col;
                        if (kfo < d && o < O) {
                            float* dst = dF + (size_t)(kfo + 1) * O + o;
                            float v = j == 0 ? e0[reg] : e1[reg];
                            if (!first) v += *dst;
                            *dst = v;
                        }
                    }
                }
            }
            // row 0 (the "ones" column): the column sums of dP_m, one thread per output
            if ((tid >> 5) == m) {
                const int ol = tid & 31, o = o0 + ol;
                float sum = 0.f;
                for (int bl = 0; bl < kChunk; ++bl) sum += dps[m][bl][ol];
                if (o < O) {
                    if (!first) sum += dF[o];
                    dF[o] = sum;
                }
            }
        }
        __syncthreads();
    }
    dwp = wave_reduce_sum(dwp);
    if (lane == 0) wred[wave] = dwp;
    __syncthreads();
    if (tid == 0) dwpart[(size_t)blockIdx.x * a.R + r] = ((wred[0] + wred[1]) + wred[2]) + wred[3];
}

// input gradients, partial over the rank splits: grid (sample tiles, splits); part.p[m] [nsplit][B, d_m] or NULL (skipped)
template <int M>
__global__ void __launch_bounds__(kThreads) lrtf_bwd_input_kernel(Args a, const float* __restrict__ g, Ptrs part, int per) {
    __shared__ float dps[M][kTile][kChunk + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4;
    const int b0 = blockIdx.x * kTile, split = blockIdx.y;
    const int B = a.B, O = a.O;
    const int rs0 = split * per, rs1 = min(a.R, rs0 + per);
    bool first = true;
    for (int r = rs0; r < rs1; ++r) {
        const float wr = a.w[r];
        for (int co = 0; co < O; co += kChunk) {
            {
                const int o0 = co + kTile * wave;
                f32x4 acc[M][2][2];
                p_tiles<M>(a, r, b0, o0, lane, acc);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) {
                            const int bl = 16 * i + 4 * kq + reg, ol = 16 * j + col;
                            const float gw = g_at(g, b0 + bl, o0 + ol, B, O) * wr;
                            float p[M];
#pragma unroll
                            for (int m = 0; m < M; ++m) p[m] = acc[m][i][j][reg];
#pragma unroll
                            for (int m = 0; m < M; ++m) dps[m][bl][kTile * wave + ol] = gw * others<M>(p, m);
                        }
            }
            __syncthreads();
#pragma unroll
            for (int m = 0; m < M; ++m) {
                if (part.p[m] == nullptr) continue;
                const int d = a.d[m], nkf = (d + 15) >> 4;
                const float* F = a.f[m] + (size_t)r * (d + 1) * O;
                float* dst = part.p[m] + (size_t)split * B * d;
                for (int kt = wave; kt < nkf; kt += 4) {
                    const int kf = 16 * kt + col, kfc = min(kf, d - 1);
                    const float* Fr = F + (size_t)(kfc + 1) * O;
                    f32x4 e0 = {0.f, 0.f, 0.f, 0.f}, e1 = e0;
    #pragma unroll 8
                for (int s = 0; s < kChunk / 4; ++s) {
                        const int ol = 4 * s + kq;
                        const float bv = Fr[min(co + ol, O - 1)];          // B[k = output][col = feature]; dP is 0 past O
                        e0 = mfma_16x16x4(dps[m][col][ol], bv, e0);           // A[row = sample][k = output]
                        e1 = mfma_16x16x4(dps[m][16 + col][ol], bv, e1);
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) {
                            const int b = b0 + 16 * i + 4 * kq + reg;
                            if (b < B && kf < d) {
                                float* q = dst + (size_t)b * d + kf;
                                float v = i == 0 ? e0[reg] : e1[reg];
                                if (!first) v += *q;
                                *q = v;
                            }
                        }
                }
            }
            __syncthreads();
            first = false;
        }
    }
}

// dbias[o] = sum_b g[b, o]
__global__ void __launch_bounds__(kThreads) lrtf_dbias_kernel(const float* __restrict__ g, float* __restrict__ dbias, int B, int O) {
    const int o = blockIdx.x * kThreads + threadIdx.x;
    if (o >= O) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += g[(size_t)b * O + o];
    dbias[o] = s;
}

struct Split {
    int n, per;
};

// n rank splits of `per` ranks each (the last may hold fewer, none is empty)
Split make_split(int R, int want) {
    int n = want < 1 ? 1 : (want > R ? R : want);
    const int per = ceil_div(R, n);
    n = ceil_div(R, per);
    return Split{n, per};
}

Split fwd_split(int B, int O, int R) {
    const int tiles = ceil_div(B, kTile) * ceil_div(O, kTile);
    const int want = ceil_div(kTargetGroups, tiles), most = ceil_div(R, 4);      // a workgroup's 4 waves take a rank each
    return make_split(R, want < most ? want : most);
}

Split input_split(int B, int R) {
    const int want = ceil_div(kTargetGroups, ceil_div(B, kTile));
    return make_split(R, want < 64 ? want : 64);
}

size_t round4(size_t n) { return (n + 3) & ~(size_t)3; }

int check_shapes(int M, const int* dims, int B, int O, int R) {
    if (!dims || B <= 0 || O <= 0 || R <= 0 || M <= 0) return DYNMM_EINVAL;
    if (M < 2 || M > kMaxM) return DYNMM_EUNSUPPORTED;
    const size_t lim = (size_t)1 << 31;
    if ((size_t)B * O >= lim || R > 65535 || ceil_div(B, kTile) > 65535) return DYNMM_EUNSUPPORTED;
    for (int m = 0; m < M; ++m) {
        if (dims[m] <= 0) return DYNMM_EINVAL;
        if ((size_t)B * dims[m] >= lim || ((size_t)dims[m] + 1) * O >= lim) return DYNMM_EUNSUPPORTED;
    }
    return DYNMM_OK;
}

int fill_args(Args& a, const float* const* zs, const float* const* factors, const int* dims, int M, const float* w,
              const float* bias, int B, int O, int R) {
    if (!zs || !factors || !w) return DYNMM_EINVAL;
    for (int m = 0; m < kMaxM; ++m) {
        const int s = m < M ? m : 0;
        if (!zs[s] || !factors[s]) return DYNMM_EINVAL;
        a.z[m] = zs[s];
        a.f[m] = factors[s];
        a.d[m] = dims[s];
    }
    a.w = w;
    a.bias = bias;
    a.B = B;
    a.O = O;
    a.R = R;
    return DYNMM_OK;
}

}  // namespace
}  // namespace dynmm

using namespace dynmm;

extern "C" size_t dynmm_lrtf_fwd_workspace_bytes(int B, int O, int R) {
    if (B <= 0 || O <= 0 || R <= 0) return 0;
    const Split sp = fwd_split(B, O, R);
    return sp.n > 1 ? (size_t)sp.n * B * O * sizeof(float) : 0;
}

extern "C" int dynmm_lrtf_fwd(const float* const* zs, const float* const* factors, const int* dims, int M, const float* w,
                              const float* bias, float* out, float* workspace, size_t workspace_bytes, int B, int O, int R,
                              void* stream) {
    (void)hipGetLastError();
    int s = check_shapes(M, dims, B, O, R);
    if (s) return s;
    if (!bias || !out) return DYNMM_EINVAL;
    Args a;
    s = fill_args(a, zs, factors, dims, M, w, bias, B, O, R);
    if (s) return s;
    const Split sp = fwd_split(B, O, R);
    if (sp.n > 1 && (!workspace || workspace_bytes < dynmm_lrtf_fwd_workspace_bytes(B, O, R))) return DYNMM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* dst = sp.n > 1 ? workspace : out;
    const dim3 grid(ceil_div(O, kTile), ceil_div(B, kTile), sp.n);
    if (M == 2)
        hipLaunchKernelGGL(lrtf_fwd_kernel<2>, grid, dim3(kThreads), 0, st, a, dst, sp.per);
    else
        hipLaunchKernelGGL(lrtf_fwd_kernel<3>, grid, dim3(kThreads), 0, st, a, dst, sp.per);
    DYNMM_LAUNCH_CHECK();
    if (sp.n > 1) {
        launch_reduce_slabs(workspace, out, B * O, sp.n, st);
        DYNMM_LAUNCH_CHECK();
    }
    return DYNMM_OK;
}

extern "C" size_t dynmm_lrtf_bwd_workspace_bytes(int M, const int* dims, int B, int O, int R) {
    if (check_shapes(M, dims, B, O, R)) return 0;
    size_t n = round4((size_t)ceil_div(O, kTile) * R);
    const Split sp = input_split(B, R);
    for (int m = 0; m < M; ++m) n += round4((size_t)sp.n * B * dims[m]);
    return n * sizeof(float);
}

extern "C" int dynmm_lrtf_bwd(const float* g, const float* const* zs, const float* const* factors, const int* dims, int M,
                              const float* w, float* const* dzs, float* const* dfs, float* dw, float* dbias, float* workspace,
                              size_t workspace_bytes, int B, int O, int R, void* stream) {
    (void)hipGetLastError();
    int s = check_shapes(M, dims, B, O, R);
    if (s) return s;
    if (!g) return DYNMM_EINVAL;
    Args a;
    s = fill_args(a, zs, factors, dims, M, w, nullptr, B, O, R);
    if (s) return s;
    if (!workspace || workspace_bytes < dynmm_lrtf_bwd_workspace_bytes(M, dims, B, O, R)) return DYNMM_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int not_ = ceil_div(O, kTile);
    if (dfs) {
        // parameter gradients: all of them or none
        if (!dw || !dbias) return DYNMM_EINVAL;
        Ptrs df{};
        for (int m = 0; m < M; ++m) {
            if (!dfs[m]) return DYNMM_EINVAL;
            df.p[m] = dfs[m];
        }
        float* dwpart = workspace;
        const dim3 grid(not_, R);
        if (M == 2)
            hipLaunchKernelGGL(lrtf_bwd_factor_kernel<2>, grid, dim3(kThreads), 0, st, a, g, df, dwpart);
        else
            hipLaunchKernelGGL(lrtf_bwd_factor_kernel<3>, grid, dim3(kThreads), 0, st, a, g, df, dwpart);
        DYNMM_LAUNCH_CHECK();
        launch_reduce_slabs(dwpart, dw, R, not_, st);
        DYNMM_LAUNCH_CHECK();
        hipLaunchKernelGGL(lrtf_dbias_kernel, dim3(ceil_div(O, kThreads)), dim3(kThreads), 0, st, g, dbias, B, O);
        DYNMM_LAUNCH_CHECK();
    }
    bool any = false;
    for (int m = 0; dzs && m < M; ++m) any = any || dzs[m] != nullptr;
    if (any) {
        const Split sp = input_split(B, R);
        Ptrs part{};
        float* p = workspace + round4((size_t)not_ * R);
        for (int m = 0; m < M; ++m) {
            part.p[m] = dzs[m] ? p : nullptr;
            p += round4((size_t)sp.n * B * dims[m]);
        }
        const dim3 grid(ceil_div(B, kTile), sp.n);
        if (M == 2)
            hipLaunchKernelGGL(lrtf_bwd_input_kernel<2>, grid, dim3(kThreads), 0, st, a, g, part, sp.per);
        else
            hipLaunchKernelGGL(lrtf_bwd_input_kernel<3>, grid, dim3(kThreads), 0, st, a, g, part, sp.per);
        DYNMM_LAUNCH_CHECK();
        for (int m = 0; m < M; ++m)
            if (dzs[m]) {
                launch_reduce_slabs(part.p[m], dzs[m], B * dims[m], sp.n, st);
                DYNMM_LAUNCH_CHECK();
            }
    }
    return DYNMM_OK;
}
