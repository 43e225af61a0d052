// The recurrence of a one-layer, one-direction GRU (torch.nn.GRU, gate order r | z | n, h0 = 0), forward and backward, for the
// GRU experts of the modality-level DynMM (MultiBench unimodals.common_models.GRU; affect_uni.py --enc gru, affect_mm.py
// --fusion 0 / 1).  The input projection gi = W_ih x + b_ih of ALL time steps and both weight gradients are 1x1-convolution
// problems the library already serves (dynmm_conv2d_fwd / _wgrad); this file is what is serial in t.
//
// Layout: time is the convolution's batch axis.  gi [T, 3H, B], states [T, H, B], saved gates [T, 4H, B] (r | z | n | W_hn h +
// b_hn), dgi / dgh [T, 3H, B]: every time step is one contiguous slab with the batch innermost, and the recurrent product of a
// step is W_hh [3H, H] . h [H, B] (M = gate rows, N = samples, K = hidden units) on v_mfma_f32_16x16x4_f32.
//
// Tiling: a wave owns a 16-unit x 16-sample tile and accumulates its r, z and n rows side by side (three independent
// accumulators, which also covers the instruction's 40-cycle dependent latency), so the gate arithmetic of an element happens in
// the lane that holds its three sums (C/D layout: sample = lane & 15, unit = 4 (lane >> 4) + register).  W_hh is packed once per
// call (gru_pack_kernel) as [unit tile][k step][gate][lane] so that a wave's A operand of one MFMA is 64 consecutive floats, H
// padded to a multiple of 16 with zero rows and columns; the second half of the pack is the same thing for W_hh^T (backward:
// dh_prev = dh z + W_hh^T dgh, the sum over the 3H gate rows again split by gate into three accumulators).
//
// Two arms (dynmm_gru_arm):
//   resident  one launch for the sequence; a workgroup owns 16 samples and ALL units (unit tiles dealt round-robin to up to 16
//             waves).  h (forward) / dgh and the carried dh (backward) live in LDS, W_hh too where it fits beside them, else it
//             streams from L2.  H <= 512.
//   stepped   one launch per time step, grid (unit tiles) x (sample tiles); the four waves of a workgroup split K and their
//             partial sums meet in LDS in a fixed order.  States / dgh travel between steps through their own output slabs.
// No workgroup ever waits for another one inside a kernel.  All loads are unconditional on clamped addresses, the value is
// selected afterwards (batch tail, unit tail, length mask).
#include "common.h"
#include "mfma.h"

namespace dynmm {
namespace {

constexpr int kArmResident = 1, kArmStepped = 2;
constexpr int kResidentMaxHp = 512;
constexpr int kMaxWaves = 16;
constexpr size_t kLdsBytes = 160 * 1024;
constexpr int kStepThreads = 256;

inline int gru_hp(int H) { return ceil_div(H, 16) * 16; }

// packed[0 .. 3Hp^2): element (tile ut, k step kc, gate g, lane l) = W[g H + 16 ut + (l & 15)][4 kc + (l >> 4)];
// packed[3Hp^2 ..):   the same of W^T per gate:                      W[g H + 4 kc + (l >> 4)][16 ut + (l & 15)].
__global__ void __launch_bounds__(256) gru_pack_kernel(const float* __restrict__ w, float* __restrict__ packed, int H, int Hp) {
    const int half = 3 * Hp * Hp;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 2 * half) return;
    const bool tr = idx >= half;
    const int i = tr ? idx - half : idx;
    const int nkc = Hp / 4;
    const int lane = i & 63, g = (i >> 6) % 3, kc = (i / 192) % nkc, ut = i / (192 * nkc);
    const int m = 16 * ut + (lane & 15), k = 4 * kc + (lane >> 4);
    const int row = tr ? k : m, col = tr ? m : k;
    const float v = w[(size_t)(g * H + min(row, H - 1)) * H + min(col, H - 1)];
    packed[idx] = (row < H && col < H) ? v : 0.f;
}

// Three accumulators of one tile over the k steps [kc0, kc1): acc[g] += Wtile_g . vec_g, vec_g element (k, sample) at
// vec[g * gstride + min(k, kmax) * vstride + coloff].  wt = the tile's packed weights + lane.
__device__ __forceinline__ void tile_mma(const float* wt, const float* vec, int gstride, int vstride, int kmax, int coloff,
                                         int kc0, int kc1, int lane, f32x4& a0, f32x4& a1, f32x4& a2) {
    const int kq = lane >> 4;
    for (int kc = kc0; kc < kc1; ++kc) {
        const float w0 = wt[kc * 192], w1 = wt[kc * 192 + 64], w2 = wt[kc * 192 + 128];
        const int off = min(4 * kc + kq, kmax) * vstride + coloff;
        const float v0 = vec[off], v1 = vec[gstride + off], v2 = vec[2 * gstride + off];
        a0 = mfma_16x16x4(w0, v0, a0);
        a1 = mfma_16x16x4(w1, v1, a1);
        a2 = mfma_16x16x4(w2, v2, a2);
    }
}

struct FwdArgs {
    const float* gi;       // [T, 3H, B]
    const float* wp;       // packed W_hh (forward half)
    const float* bhh;      // [3H]
    const int* len;        // [B] or NULL
    float* hbuf;           // [T + 1, H, B], slab 0 = zeros
    float* gates;          // [T, 4H, B]
    float* hn;             // [H, B]
    int T, B, H, Hp;
};

// One element of one step: the sums (ghr, ghz, ghn WITHOUT bias) of unit u (clamped uc), sample b (clamped bc).
__device__ __forceinline__ float fwd_cell(const FwdArgs& a, int t, int u, int uc, int b, int bc, bool bok, bool active,
                                          float ghr, float ghz, float ghn, float hp, bool last) {
    const int H = a.H, B = a.B;
    const float* git = a.gi + (size_t)t * 3 * H * B;
    const float gir = git[(size_t)uc * B + bc], giz = git[(size_t)(H + uc) * B + bc], gin = git[(size_t)(2 * H + uc) * B + bc];
    const float r = sigmoid_f(gir + (ghr + a.bhh[uc]));
    const float z = sigmoid_f(giz + (ghz + a.bhh[H + uc]));
    const float hh = ghn + a.bhh[2 * H + uc];
    const float n = tanhf(gin + r * hh);
    const float hnew = active ? (1.f - z) * n + z * hp : hp;
    if (u < H && bok) {
        float* gt = a.gates + (size_t)t * 4 * H * B;
        gt[(size_t)u * B + b] = r;
        gt[(size_t)(H + u) * B + b] = z;
        gt[(size_t)(2 * H + u) * B + b] = n;
        gt[(size_t)(3 * H + u) * B + b] = hh;
        a.hbuf[(size_t)(t + 1) * H * B + (size_t)u * B + b] = hnew;
        if (last) a.hn[(size_t)u * B + b] = hnew;
    }
    return u < H ? hnew : 0.f;
}

// resident forward.  LDS: h ping-pong [2][Hp][16] (+ packed W_hh [3 Hp Hp] when WLDS).
template <bool WLDS>
__global__ void __launch_bounds__(64 * kMaxWaves) gru_fwd_resident_kernel(FwdArgs a) {
    extern __shared__ float smem[];
    const int Hp = a.Hp, H = a.H, B = a.B, T = a.T;
    float* hs = smem;
    float* wl = smem + 2 * Hp * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int col = lane & 15, b = blockIdx.x * 16 + col, bc = min(b, B - 1);
    const bool bok = b < B;
    const int len = a.len ? a.len[bc] : T;
    for (int i = tid; i < 2 * Hp * 16; i += blockDim.x) hs[i] = 0.f;
    if (WLDS)
        for (int i = tid; i < 3 * Hp * Hp; i += blockDim.x) wl[i] = a.wp[i];
    __syncthreads();
    const float* wsrc = WLDS ? wl : a.wp;
    const int nkc = Hp / 4, ntile = Hp / 16;
    for (int t = 0; t < T; ++t) {
        const float* cur = hs + (t & 1) * Hp * 16;
        float* nxt = hs + ((t & 1) ^ 1) * Hp * 16;
        const bool active = t < len;
        for (int ut = wave; ut < ntile; ut += nw) {
            f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, an = ar;
            if (t > 0) tile_mma(wsrc + (size_t)ut * nkc * 192 + lane, cur, 0, 16, Hp - 1, col, 0, nkc, lane, ar, az, an);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int u = 16 * ut + 4 * (lane >> 4) + reg, uc = min(u, H - 1);
                nxt[u * 16 + col] = fwd_cell(a, t, u, uc, b, bc, bok, active, ar[reg], az[reg], an[reg], cur[u * 16 + col], t == T - 1);
            }
        }
        __syncthreads();
    }
}

// stepped forward: step t, grid (unit tiles, sample tiles), 4 waves split K.
__global__ void __launch_bounds__(kStepThreads) gru_fwd_step_kernel(FwdArgs a, int t) {
    __shared__ float red[4][3][4][64];
    const int Hp = a.Hp, H = a.H, B = a.B;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ut = blockIdx.x, col = lane & 15, b = blockIdx.y * 16 + col, bc = min(b, B - 1);
    const bool bok = b < B;
    const int len = a.len ? a.len[bc] : a.T;
    const int nkc = Hp / 4, per = nkc / 4;              // Hp % 16 == 0: the k steps divide evenly over the 4 waves
    const float* hprev = a.hbuf + (size_t)t * H * B;
    f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, an = ar;
    if (t > 0) tile_mma(a.wp + (size_t)ut * nkc * 192 + lane, hprev, 0, B, H - 1, bc, wave * per, (wave + 1) * per, lane, ar, az, an);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        red[wave][0][reg][lane] = ar[reg];
        red[wave][1][reg][lane] = az[reg];
        red[wave][2][reg][lane] = an[reg];
    }
    __syncthreads();
    const int reg = wave;                               // wave w finishes register w of every lane
    float s[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) s[g] = ((red[0][g][reg][lane] + red[1][g][reg][lane]) + red[2][g][reg][lane]) + red[3][g][reg][lane];
    const int u = 16 * ut + 4 * (lane >> 4) + reg, uc = min(u, H - 1);
    const float hp = hprev[(size_t)uc * B + bc];
    (void)fwd_cell(a, t, u, uc, b, bc, bok, t < len, s[0], s[1], s[2], hp, t == a.T - 1);
}

struct BwdArgs {
    const float* dhn;      // [H, B] or NULL
    const float* dhseq;    // [T, H, B] or NULL
    const float* wpt;      // packed W_hh^T (backward half)
    const int* len;
    const float* hbuf;     // [T + 1, H, B]
    const float* gates;    // [T, 4H, B]
    float* dgi;            // [T, 3H, B]
    float* dgh;            // [T, 3H, B]
    float* ws;             // stepped: carried dh z, ping-pong [2][H, B]
    int T, B, H, Hp;
};

// One element of one backward step.  dh = the gradient carried into h_t WITHOUT this step's external terms; returns dh z (what is
// carried on besides W_hh^T dgh) and the three dgh values.  Masked steps: zeros, dh passes through.
__device__ __forceinline__ float bwd_cell(const BwdArgs& a, int t, int j, int jc, int b, int bc, bool bok, int len, float dh,
                                          float& g0, float& g1, float& g2) {
    const int H = a.H, B = a.B;
    const size_t e = (size_t)jc * B + bc;
    if (a.dhseq) dh += a.dhseq[(size_t)t * H * B + e];
    if (a.dhn) {
        const float v = a.dhn[e];
        dh += (t == len - 1) ? v : 0.f;
    }
    const float* gt = a.gates + (size_t)t * 4 * H * B;
    const float r = gt[e], z = gt[(size_t)H * B + e], n = gt[(size_t)2 * H * B + e], hh = gt[(size_t)3 * H * B + e];
    const float hp = a.hbuf[(size_t)t * H * B + e];
    const bool active = t < len;
    const float dnp = active ? dh * (1.f - z) * (1.f - n * n) : 0.f;
    const float dzp = active ? dh * (hp - n) * z * (1.f - z) : 0.f;
    const float drp = dnp * hh * r * (1.f - r);
    g0 = drp;
    g1 = dzp;
    g2 = dnp * r;
    if (j < H && bok) {
        const size_t o = (size_t)t * 3 * H * B + (size_t)j * B + b;
        a.dgi[o] = drp;
        a.dgi[o + (size_t)H * B] = dzp;
        a.dgi[o + (size_t)2 * H * B] = dnp;
        a.dgh[o] = g0;
        a.dgh[o + (size_t)H * B] = g1;
        a.dgh[o + (size_t)2 * H * B] = g2;
    }
    return active ? dh * z : dh;
}

// resident backward.  LDS: dgh of the step above [3][Hp][16], carried dh [Hp][16] (+ packed W_hh^T when WLDS).
template <bool WLDS>
__global__ void __launch_bounds__(64 * kMaxWaves) gru_bwd_resident_kernel(BwdArgs a) {
    extern __shared__ float smem[];
    const int Hp = a.Hp, H = a.H, B = a.B, T = a.T;
    float* dgs = smem;
    float* dhs = smem + 3 * Hp * 16;
    float* wl = smem + 4 * Hp * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int col = lane & 15, b = blockIdx.x * 16 + col, bc = min(b, B - 1);
    const bool bok = b < B;
    const int len = a.len ? a.len[bc] : T;
    for (int i = tid; i < 4 * Hp * 16; i += blockDim.x) smem[i] = 0.f;
    if (WLDS)
        for (int i = tid; i < 3 * Hp * Hp; i += blockDim.x) wl[i] = a.wpt[i];
    __syncthreads();
    const float* wsrc = WLDS ? wl : a.wpt;
    const int nkc = Hp / 4, ntile = Hp / 16;
    for (int t = T - 1; t >= 0; --t) {
        if (t < T - 1) {
            // dh_t = (dh z)_{t+1} + W_hh^T dgh_{t+1}; an element of dhs is touched by its owner lane alone
            for (int jt = wave; jt < ntile; jt += nw) {
                f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0;
                tile_mma(wsrc + (size_t)jt * nkc * 192 + lane, dgs, Hp * 16, 16, Hp - 1, col, 0, nkc, lane, a0, a1, a2);
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int j = 16 * jt + 4 * (lane >> 4) + reg;
                    dhs[j * 16 + col] += (a0[reg] + a1[reg]) + a2[reg];
                }
            }
            __syncthreads();                             // every wave has read dgh_{t+1}
        }
        for (int jt = wave; jt < ntile; jt += nw) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int j = 16 * jt + 4 * (lane >> 4) + reg, jc = min(j, H - 1);
                float g0, g1, g2;
                const float dhz = bwd_cell(a, t, j, jc, b, bc, bok, len, dhs[j * 16 + col], g0, g1, g2);
                const bool ok = j < H;
                dhs[j * 16 + col] = ok ? dhz : 0.f;
                dgs[j * 16 + col] = ok ? g0 : 0.f;
                dgs[(Hp + j) * 16 + col] = ok ? g1 : 0.f;
                dgs[(2 * Hp + j) * 16 + col] = ok ? g2 : 0.f;
            }
        }
        __syncthreads();
    }
}

// stepped backward: step t, grid (unit tiles, sample tiles), 4 waves split the k steps of each gate.
__global__ void __launch_bounds__(kStepThreads) gru_bwd_step_kernel(BwdArgs a, int t) {
    __shared__ float red[4][4][64];
    const int Hp = a.Hp, H = a.H, B = a.B, T = a.T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int jt = blockIdx.x, col = lane & 15, b = blockIdx.y * 16 + col, bc = min(b, B - 1);
    const bool bok = b < B;
    const int len = a.len ? a.len[bc] : T;
    const int nkc = Hp / 4, per = nkc / 4;
    const bool carry = t < T - 1;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0;
    if (carry)
        tile_mma(a.wpt + (size_t)jt * nkc * 192 + lane, a.dgh + (size_t)(t + 1) * 3 * H * B, H * B, B, H - 1, bc, wave * per,
                 (wave + 1) * per, lane, a0, a1, a2);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) red[wave][reg][lane] = (a0[reg] + a1[reg]) + a2[reg];
    __syncthreads();
    const int reg = wave;
    const float s = ((red[0][reg][lane] + red[1][reg][lane]) + red[2][reg][lane]) + red[3][reg][lane];
    const int j = 16 * jt + 4 * (lane >> 4) + reg, jc = min(j, H - 1);
    const float* zin = a.ws + (size_t)((t + 1) & 1) * H * B;
    float* zout = a.ws + (size_t)(t & 1) * H * B;
    const float zprev = zin[(size_t)jc * B + bc];
    const float dh = carry ? zprev + s : 0.f;
    float g0, g1, g2;
    const float dhz = bwd_cell(a, t, j, jc, b, bc, bok, len, dh, g0, g1, g2);
    if (j < H && bok) zout[(size_t)j * B + b] = dhz;
}

int auto_arm(int B, int H, int T) {
    (void)B;
    (void)T;
    // measured on an MI355X at T = 50 (profiles/gru_arms.md): H = 64, where W_hh sits in LDS, is the one measured size at which
    // the resident arm wins (by 25 % at B = 32, level at B = 128); at H = 128 and 512 the stepped arm wins by 36 % and 7x
    return gru_hp(H) <= 64 ? kArmResident : kArmStepped;
}

int resolve_arm(int B, int H, int T, int arm) {
    if (arm == 0) return auto_arm(B, H, T);
    if (arm != kArmResident && arm != kArmStepped) return DYNMM_EINVAL;
    if (arm == kArmResident && gru_hp(H) > kResidentMaxHp) return DYNMM_EUNSUPPORTED;
    return arm;
}

template <typename K>
int raise_lds(K kernel, size_t lds, size_t& done) {
    if (lds > done) {
        DYNMM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        done = lds;
    }
    return DYNMM_OK;
}

}  // namespace
}  // namespace dynmm

using namespace dynmm;

extern "C" size_t dynmm_gru_packed_floats(int H) {
    if (H <= 0) return 0;
    const size_t hp = (size_t)gru_hp(H);
    return 6 * hp * hp;
}

extern "C" int dynmm_gru_pack(const float* w_hh, float* packed, int H, void* stream) {
    (void)hipGetLastError();
    if (!w_hh || !packed || H <= 0 || H > 4096) return DYNMM_EINVAL;
    const int Hp = gru_hp(H);
    const int n = 6 * Hp * Hp;
    hipLaunchKernelGGL(gru_pack_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, w_hh, packed, H, Hp);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

extern "C" int dynmm_gru_arm(int B, int H, int T) {
    if (B <= 0 || H <= 0 || T <= 0) return 0;
    return auto_arm(B, H, T);
}

extern "C" size_t dynmm_gru_bwd_workspace_bytes(int B, int H) {
    if (B <= 0 || H <= 0) return 0;
    return 2 * (size_t)B * H * sizeof(float);
}

extern "C" int dynmm_gru_seq_fwd(const float* gi, const float* packed, const float* b_hh, const int* lengths, float* hbuf,
                                 float* gates, float* hn, int T, int B, int H, int arm, void* stream) {
    (void)hipGetLastError();
    if (!gi || !packed || !b_hh || !hbuf || !gates || !hn || T <= 0 || B <= 0 || H <= 0 || H > 4096) return DYNMM_EINVAL;
    if ((size_t)T * 4 * H * B >= ((size_t)1 << 31)) return DYNMM_EUNSUPPORTED;
    arm = resolve_arm(B, H, T, arm);
    if (arm < 0) return arm;
    hipStream_t st = (hipStream_t)stream;
    const int Hp = gru_hp(H);
    DYNMM_HIP_TRY(hipMemsetAsync(hbuf, 0, (size_t)H * B * sizeof(float), st));
    FwdArgs a{gi, packed, b_hh, lengths, hbuf, gates, hn, T, B, H, Hp};
    const int nbt = ceil_div(B, 16), ntile = Hp / 16;
    if (arm == kArmResident) {
        const size_t vec = (size_t)2 * Hp * 16 * sizeof(float), wb = (size_t)3 * Hp * Hp * sizeof(float);
        const bool wlds = vec + wb <= kLdsBytes;
        const size_t lds = vec + (wlds ? wb : 0);
        const int threads = 64 * (ntile < kMaxWaves ? ntile : kMaxWaves);
        static size_t done_w = 0, done_g = 0;
        if (wlds) {
            const int s = raise_lds(&gru_fwd_resident_kernel<true>, lds, done_w);
            if (s) return s;
            hipLaunchKernelGGL(gru_fwd_resident_kernel<true>, dim3(nbt), dim3(threads), lds, st, a);
        } else {
            const int s = raise_lds(&gru_fwd_resident_kernel<false>, lds, done_g);
            if (s) return s;
            hipLaunchKernelGGL(gru_fwd_resident_kernel<false>, dim3(nbt), dim3(threads), lds, st, a);
        }
        DYNMM_LAUNCH_CHECK();
        return DYNMM_OK;
    }
    for (int t = 0; t < T; ++t) {
        hipLaunchKernelGGL(gru_fwd_step_kernel, dim3(ntile, nbt), dim3(kStepThreads), 0, st, a, t);
        DYNMM_LAUNCH_CHECK();
    }
    return DYNMM_OK;
}

extern "C" int dynmm_gru_seq_bwd(const float* d_hn, const float* d_hseq, const float* packed, const int* lengths,
                                 const float* hbuf, const float* gates, float* dgi, float* dgh, float* workspace,
                                 size_t workspace_bytes, int T, int B, int H, int arm, void* stream) {
    (void)hipGetLastError();
    if ((!d_hn && !d_hseq) || !packed || !hbuf || !gates || !dgi || !dgh || T <= 0 || B <= 0 || H <= 0 || H > 4096) return DYNMM_EINVAL;
    if ((size_t)T * 4 * H * B >= ((size_t)1 << 31)) return DYNMM_EUNSUPPORTED;
    arm = resolve_arm(B, H, T, arm);
    if (arm < 0) return arm;
    hipStream_t st = (hipStream_t)stream;
    const int Hp = gru_hp(H);
    BwdArgs a{d_hn, d_hseq, packed + (size_t)3 * Hp * Hp, lengths, hbuf, gates, dgi, dgh, workspace, T, B, H, Hp};
    const int nbt = ceil_div(B, 16), ntile = Hp / 16;
    if (arm == kArmResident) {
        const size_t vec = (size_t)4 * Hp * 16 * sizeof(float), wb = (size_t)3 * Hp * Hp * sizeof(float);
        const bool wlds = vec + wb <= kLdsBytes;
        const size_t lds = vec + (wlds ? wb : 0);
        const int threads = 64 * (ntile < kMaxWaves ? ntile : kMaxWaves);
        static size_t done_w = 0, done_g = 0;
        if (wlds) {
            const int s = raise_lds(&gru_bwd_resident_kernel<true>, lds, done_w);
            if (s) return s;
            hipLaunchKernelGGL(gru_bwd_resident_kernel<true>, dim3(nbt), dim3(threads), lds, st, a);
        } else {
            const int s = raise_lds(&gru_bwd_resident_kernel<false>, lds, done_g);
            if (s) return s;
            hipLaunchKernelGGL(gru_bwd_resident_kernel<false>, dim3(nbt), dim3(threads), lds, st, a);
        }
        DYNMM_LAUNCH_CHECK();
        return DYNMM_OK;
    }
    if (!workspace || workspace_bytes < dynmm_gru_bwd_workspace_bytes(B, H)) return DYNMM_EWORKSPACE;
    for (int t = T - 1; t >= 0; --t) {
        hipLaunchKernelGGL(gru_bwd_step_kernel, dim3(ntile, nbt), dim3(kStepThreads), 0, st, a, t);
        DYNMM_LAUNCH_CHECK();
    }
    return DYNMM_OK;
}
