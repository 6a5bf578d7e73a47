// The packed 16-byte lane slot, as pack.hip (one operand, one tower, one embedding) and adam.hip (a whole model) build it.
#pragma once
#include "tile.h"

// eight floats -> the 16 bytes of one lane slot: four bf16 pairs, or the first four as fp32
template <int P>
static __device__ __forceinline__ u32x4_t pack_frag(const float (&v)[8]) {
    Frag f;
    if (P == PREC_BF16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) f.u[e] = pack_bf2(v[2 * e], v[2 * e + 1]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) f.f[e] = v[e];
    }
    return f.u;
}

// One packed 16-byte slot: logical operand X[i][k] = src[i * si + kk * sk], i < I, kk < K, image padded to (Ip, Kp).
template <int P>
__device__ __forceinline__ void pack_slot(const float* src, long si, long sk, long I, long K, long Ip, long Kp, int mode,
                                          int kmajor, char* dst, long slot) {
    typedef Prec<P> Pr;
    const long nIB = Ip / 16, nKB = Kp / Pr::KB;
    if (slot >= nIB * nKB * 64) return;
    const long blk = slot >> 6;
    const int lane = (int)(slot & 63), g = lane >> 4, il = lane & 15;
    long ib, kb;
    if (kmajor) { kb = blk / nIB; ib = blk % nIB; } else { ib = blk / nKB; kb = blk % nKB; }
    const long i = ib * 16 + il;
    float v[8];
#pragma unroll
    for (int e = 0; e < Pr::EPL; ++e) {
        const long kk = kb * Pr::KB + Pr::kmap(mode, g, e);
        v[e] = (i < I && kk < K) ? src[i * si + kk * sk] : 0.f;
    }
    *reinterpret_cast<u32x4_t*>(dst + slot * 16) = pack_frag<P>(v);
}
