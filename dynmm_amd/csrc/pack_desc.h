// The multi-tensor weight packs (ops.PackedWeights: every conv weight of a training step in ONE launch per operand family): what
// the four families — conv_igemm.hip's direct layouts and the F(2,3) / F(4,3) / F(2x2,3x3) filter transforms of conv_wino.hip,
// conv_wino43.hip, conv_wino2d.hip — share.  A launch holds the workgroups of all its tensors back to back; descriptor d says where
// tensor d's begin (blk0), and a workgroup finds its tensor by binary search.
#pragma once
#include "common.h"

namespace dynmm {

// Descriptor of the three Winograd families: {src, dst: float offsets from the two bases; Co | Ci << 32; kk | first workgroup << 32}
// with kk = KH | KW << 8 | dgrad << 16 (F(2,3): dgrad 0 forward | 1 input gradient | 2 stride-2 input gradient; F(2x2,3x3): 0 | 1,
// KH = KW = 3 implied; F(4,3): the input gradient only; its dst is the record's ut4, the ut2 block follows it).
// (The direct family's PackDesc, conv_igemm.hip, has two destinations: 40 bytes.)
struct WinoPackDesc {
    long long src, dst;
    int Co, Ci, kk, blk0;
};
static_assert(sizeof(WinoPackDesc) == 32, "descriptor layout is part of the ABI (4 x int64 words)");

// the last descriptor whose first workgroup is <= blockIdx.x
template <typename Desc>
__device__ __forceinline__ Desc pack_desc_find(const Desc* __restrict__ desc, int ndesc) {
    int lo = 0, hi = ndesc - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[mid].blk0 <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    return desc[lo];
}

// body of the dynmm_*_pack_multi entry points of the three Winograd families (dst_base: 16-byte stores)
template <typename Kernel>
static int launch_wino_pack_multi(Kernel kernel, const float* src_base, float* dst_base, const void* desc, int ndesc,
                                  int total_blocks, void* stream) {
    (void)hipGetLastError();
    if (!src_base || !dst_base || !desc || ndesc <= 0 || total_blocks <= 0) return DYNMM_EINVAL;
    if (reinterpret_cast<uintptr_t>(dst_base) & 15u) return DYNMM_EINVAL;
    hipLaunchKernelGGL(kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, src_base, dst_base,
                       (const WinoPackDesc*)desc, ndesc);
    DYNMM_LAUNCH_CHECK();
    return DYNMM_OK;
}

}  // namespace dynmm
