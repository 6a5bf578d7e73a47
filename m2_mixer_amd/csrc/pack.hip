// Operand packing: the fp32 masters into the 16-byte lane slots the MFMA kernels read -- one operand, one tower or one embedding per
// launch (tests, the module path).  A whole model in one launch: adam.hip.
#include "dispatch.h"
#include "pack.h"

// ---------------------------------------------------------------------------------------------------
// packing: one thread per 16-byte lane slot
// ---------------------------------------------------------------------------------------------------
template <int P>
__global__ void pack_kernel(int mode, int order_k_major, const float* __restrict__ src, long stride_i, long stride_k,
                            long I, long K, char* __restrict__ dst, long nIB, long nKB) {
    pack_slot<P>(src, stride_i, stride_k, I, K, nIB * 16, nKB * Prec<P>::KB, mode, order_k_major, dst,
                 (long)blockIdx.x * blockDim.x + threadIdx.x);
}

// I, K: valid extents (reads are guarded); Ip, Kp: extents of the zero-padded image
static int pack_impl(int prec, int mode, int order_k_major, const float* src, int64_t stride_i, int64_t stride_k,
                     int64_t I, int64_t K, int64_t Ip, int64_t Kp, void* dst, void* stream) {
    if (prec != PREC_BF16 && prec != PREC_F32) { m2m_set_error("bad prec", __FILE__, __LINE__); return -1; }
    const long KB = prec == PREC_BF16 ? 32 : 16;
    const long nIB = ceil_div(Ip, 16), nKB = ceil_div(Kp, KB);
    const long nslots = nIB * nKB * 64;
    const int threads = 256;
    const long grid = ceil_div(nslots, threads);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (prec == PREC_BF16)
        hipLaunchKernelGGL(pack_kernel<PREC_BF16>, dim3((unsigned)grid), dim3(threads), 0, st, mode, order_k_major, src,
                           (long)stride_i, (long)stride_k, (long)I, (long)K, (char*)dst, nIB, nKB);
    else
        hipLaunchKernelGGL(pack_kernel<PREC_F32>, dim3((unsigned)grid), dim3(threads), 0, st, mode, order_k_major, src,
                           (long)stride_i, (long)stride_k, (long)I, (long)K, (char*)dst, nIB, nKB);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int m2m_pack(int prec, int mode, int order_k_major, const float* src, int64_t stride_i, int64_t stride_k,
                        int64_t I, int64_t K, void* dst, void* stream) {
    return pack_impl(prec, mode, order_k_major, src, stride_i, stride_k, I, K, I, K, dst, stream);
}

// Packed copies of one tower block.  which: 0 w1n, 1 w1tc, 2 w2c, 3 w2tn, 4 ch_b1p.
template <int P, class TW>
__device__ __forceinline__ void pack_block_job(const TW& tw, int block, int which, long slot) {
    const m2m_block& k = tw.blk[block];
    const long D = tw.D, C = tw.C, Cp = tw.Cp;
    if (which == 4) {
        if (slot < Cp) k.ch_b1p[slot] = slot < C ? k.ch_b1[slot] : 0.f;
    } else if (which == 0) pack_slot<P>(k.ch_w1, D, 1, C, D, Cp, D, PACK_NAT, 0, (char*)k.w1n, slot);
    else if (which == 1)   pack_slot<P>(k.ch_w1, 1, D, D, C, D, Cp, PACK_CHN, 1, (char*)k.w1tc, slot);
    else if (which == 2)   pack_slot<P>(k.ch_w2, C, 1, D, C, D, Cp, PACK_CHN, 1, (char*)k.w2c, slot);
    else                   pack_slot<P>(k.ch_w2, 1, C, C, D, Cp, D, PACK_NAT, 0, (char*)k.w2tn, slot);
}

// All packed copies of every block of a tower in ONE launch: blockIdx.y = 5 * block + which.
template <int P>
__global__ void pack_tower_kernel(const m2m_tower tw) {
    pack_block_job<P>(tw, blockIdx.y / 5, blockIdx.y % 5, (long)blockIdx.x * blockDim.x + threadIdx.x);
}

extern "C" int m2m_pack_tower(const m2m_tower* t, void* stream) {
    if (int rc = m2m_check_tower(t, 1)) return rc;
    const long KB = t->prec == PREC_BF16 ? 32 : 16;
    const long nslots = (long)(t->Cp / 16) * (t->D / KB) * 64;
    const long need = nslots > t->Cp ? nslots : t->Cp;
    const dim3 grid((unsigned)ceil_div(need, 256), (unsigned)(5 * t->nblocks));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (t->prec == PREC_BF16) hipLaunchKernelGGL(pack_tower_kernel<PREC_BF16>, grid, dim3(256), 0, st, *t);
    else hipLaunchKernelGGL(pack_tower_kernel<PREC_F32>, grid, dim3(256), 0, st, *t);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int m2m_pack_embed(const m2m_embed* e, void* stream) {
    if (!e) { m2m_set_error("null embed", __FILE__, __LINE__); return -1; }
    return pack_impl(e->prec, PACK_NAT, 0, e->w, e->K, 1, e->D, e->K, e->D, e->Kp, e->wn, stream);
}
