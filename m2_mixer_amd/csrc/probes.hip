// The small probe kernels the tests use: GELU and its LDS tables, the dropout masks, the packed-operand MFMA chain, the shader clock.
#include "dispatch.h"

// ---------------------------------------------------------------------------------------------------
__global__ void gelu_probe_kernel(const float* x, float* y, float* dy, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        float a, b;
        gelu_grad_f(x[i], a, b);
        y[i] = gelu_f(x[i]);
        dy[i] = b;
        (void)a;
    }
}
extern "C" int m2m_gelu_probe(const float* x, float* y, float* dy, int64_t n, void* stream) {
    hipLaunchKernelGGL(gelu_probe_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, y, dy, (long)n);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}

// gelu / gelu' through the bf16 path's LDS tables: one workgroup fills the table with the chain kernels' own fill function and
// evaluates through the functions they call.  form 0: fp32 table {a, b, c, d}; 1: forward-only table {a, b} (dy not written);
// 2: fp16 table; 3: fp16 table through gelu_grad_tabh_masked with mask 0 (a dropped element: exact zeros);
// 4: y = the exp(-x^2 / 2) factor of gelu_grad_f as the device evaluates it (no table; dy not written).
__global__ __launch_bounds__(256) void gelu_table_probe_kernel(int form, const float* __restrict__ x, float* __restrict__ y,
                                                               float* __restrict__ dy, long n, float scale) {
    __shared__ __attribute__((aligned(16))) char tabmem[GELU_TAB_N * sizeof(gtab_t)];
    gtab_t* tab = reinterpret_cast<gtab_t*>(tabmem);
    gtab2_t* tab2 = reinterpret_cast<gtab2_t*>(tabmem);
    gtabh_t* tabh = reinterpret_cast<gtabh_t*>(tabmem);
    const int tid = threadIdx.x;
    if (form == 0) gelu_tab_fill(tab, scale, tid, 256);
    else if (form == 1) gelu_tab2_fill(tab2, scale, tid, 256);
    else if (form == 2 || form == 3) gelu_tabh_fill(tabh, scale, tid, 256);
    __syncthreads();
    for (long i = tid; i < n; i += 256) {
        const float v = x[i];
        float g = 0.f, dg = 0.f;
        if (form == 0) Act<PREC_BF16>::gelu_grad_scaled(tab, v, scale, g, dg);
        else if (form == 1) g = Act<PREC_BF16>::gelu_scaled(tab2, v, scale);
        else if (form == 2) Act<PREC_BF16>::gelu_grad_scaled(tabh, v, scale, g, dg);
        else if (form == 3) gelu_grad_tabh_masked(tabh, v, 0u, g, dg);
        else g = gelu_exp_f(v);
        y[i] = g;
        if (form != 1 && form != 4) dy[i] = dg;
    }
}
extern "C" int m2m_gelu_table_probe(int form, const float* x, float* y, float* dy, int64_t n, float scale, void* stream) {
    if (form < 0 || form > 4 || !x || !y || n < 0 || (!dy && form != 1 && form != 4)) { m2m_set_error("gelu_table_probe: bad arguments", __FILE__, __LINE__); return -1; }
    if (n == 0) return 0;
    hipLaunchKernelGGL(gelu_table_probe_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), form, x, y, dy, (long)n, scale);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}

// Mirrors the kernels' mask functions.  mode 0: generic 16-bit draw per element index;
// mode 1 (token sites at p == 0.5): one word per row (row = sample*D + channel), bit = column;
// mode 2 (channel-hidden site): drop_keep_mc on (row, column).
__global__ void dropout_mask_kernel(unsigned int key, unsigned int thr, long n, unsigned int cols, int mode, uint8_t* mask) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        Drop d; d.key = key; d.thr = thr; d.scale = 1.f;
        bool k;
        if (mode == 1) {
            const unsigned int row = (unsigned int)(i / cols), col = (unsigned int)(i % cols), nw = (cols + 31u) >> 5;
            k = (mix32(key ^ (row * nw + (col >> 5))) >> (col & 31u)) & 1u;
        }
        else if (mode == 2) k = drop_keep_mc(d, (unsigned int)(i / cols), (unsigned int)(i % cols), cols);
        else k = drop_keep(d, (unsigned int)i);
        mask[i] = k ? 1 : 0;
    }
}
extern "C" int m2m_dropout_mask(const m2m_tower* t, int blk, int site, int B, uint32_t seed, uint32_t step, uint8_t* mask, void* stream) {
    if (int rc = m2m_check_tower(t, B)) return rc;
    if (site < 0 || site > 3 || blk < 0 || blk >= t->nblocks) { m2m_set_error("bad site/blk", __FILE__, __LINE__); return -1; }
    // element counts in kernel index order: 0 (B,D,T)  1 (B,D,N)  2 (B*N, Cp)  3 (B*N, D)
    long n = 0;
    if (site == 0) n = (long)B * t->D * t->T;
    if (site == 1) n = (long)B * t->D * t->N;
    if (site == 2) n = (long)B * t->N * t->Cp;
    if (site == 3) n = (long)B * t->N * t->D;
    const unsigned int key = m2m_site_key(seed, step, t->site_base + 4u * blk + site);
    const unsigned int thr = m2m_drop_thr(t->p_drop);
    unsigned int cols = 1;
    int mode = 0;
    if (site == 2) { cols = t->Cp; mode = 2; }
    else if (site == 0 && thr == 32768u) { cols = t->T; mode = 1; }
    else if (site == 1 && thr == 32768u) { cols = t->N; mode = 1; }
    hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       key, thr, n, cols, mode, mask);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}

// C = A B^T with every operand going through the packed layouts; then C2 = C Bc^T with C's
// accumulators chained as the second product's A operand.  One wave per 16 rows of A.
template <int P>
__global__ void gemm_probe_kernel(const char* Ap /*NAT [i][k] k-minor*/, const char* Bp /*NAT [j][k] k-minor*/,
                                  const char* Bcp /*CHN [j2][k=j] k-major*/, int I, int J, int K, int J2, float* C, float* C2) {
    typedef Prec<P> Pr;
    const int lane = threadIdx.x & 63, g = lane >> 4, il = lane & 15;
    const int it = blockIdx.x;                 // 16-row tile of A
    const int nKB = (K + Pr::KB - 1) / Pr::KB;
    const int nJT = (J + 15) / 16;
    const int nJ2T = (J2 + 15) / 16;
    const int nKBc = (J + Pr::KB - 1) / Pr::KB;      // k-blocks of the packed Bc image (k = j)
    // swapped product: Ct[j][i] = B A^T so that the accumulator (rows j) chains into k = j
    for (int jp = 0; jp < (nJT + 1) / 2; ++jp) {
        f32x4_t acc[2];
        for (int t = 0; t < 2; ++t) {
            acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            const int jt = 2 * jp + t;
            if (jt < nJT)
                for (int kb = 0; kb < nKB; ++kb) {
                    const Frag b = ld_frag_global(Bp, (long)jt * nKB + kb, lane);
                    const Frag a = ld_frag_global(Ap, (long)it * nKB + kb, lane);
                    Pr::mma(acc[t], b, a);
                }
            // acc[t][r] = C[i = 16 it + il][j = 16 jt + 4g + r]
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * it + il, j = 16 * jt + 4 * g + r;
                if (jt < nJT && i < I && j < J) C[(long)i * J + j] = acc[t][r];
            }
        }
        if (C2) {
            Frag hf[Chain<P>::NF];
            Chain<P>::make(acc[0], acc[1], hf);
            for (int f = 0; f < Chain<P>::NF; ++f) {
                // fp32 chains one k-block per j tile: with an odd number of j tiles the pair's second fragment is empty and its
                // k-block lies past the packed image (zero accumulator x unowned bytes: NaN bytes there would poison C2)
                if (jp * Chain<P>::NF + f >= nKBc) continue;
                for (int j2t = 0; j2t < nJ2T; ++j2t) {
                    const Frag w = ld_frag_global(Bcp, (long)(jp * Chain<P>::NF + f) * nJ2T + j2t, lane);
                    f32x4_t o = f32x4_t{0.f, 0.f, 0.f, 0.f};
                    Pr::mma(o, hf[f], w);
                    for (int r = 0; r < 4; ++r) {
                        const int i = 16 * it + 4 * g + r, j2 = 16 * j2t + il;
                        if (i < I && j2 < J2) atomicAdd(&C2[(long)i * J2 + j2], o[r]);
                    }
                }
            }
        }
    }
}

extern "C" int m2m_gemm_probe(int prec, const float* A, const float* Bm, int I, int J, int K, const float* Bc, int J2,
                              float* C, float* C2, void* workspace, void* stream) {
    char* ws = reinterpret_cast<char*>(workspace);
    const int64_t ab = m2m_packed_bytes(prec, I, K), bb = m2m_packed_bytes(prec, J, K);
    char* Ap = ws; char* Bp = ws + ab; char* Bcp = Bp + bb;
    int rc;
    if ((rc = m2m_pack(prec, PACK_NAT, 0, A, K, 1, I, K, Ap, stream))) return rc;
    if ((rc = m2m_pack(prec, PACK_NAT, 0, Bm, K, 1, J, K, Bp, stream))) return rc;
    if (Bc && (rc = m2m_pack(prec, PACK_CHN, 1, Bc, J, 1, J2, J, Bcp, stream))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (C2) M2M_CHECK_HIP(hipMemsetAsync(C2, 0, sizeof(float) * (size_t)I * J2, st));
    const int grid = (I + 15) / 16;
    if (prec == PREC_BF16)
        hipLaunchKernelGGL(gemm_probe_kernel<PREC_BF16>, dim3(grid), dim3(64), 0, st, Ap, Bp, Bc ? Bcp : nullptr, I, J, K, J2, C, Bc ? C2 : nullptr);
    else
        hipLaunchKernelGGL(gemm_probe_kernel<PREC_F32>, dim3(grid), dim3(64), 0, st, Ap, Bp, Bc ? Bcp : nullptr, I, J, K, J2, C, Bc ? C2 : nullptr);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- shader clock under load (include/m2mixer.h: m2m_clock_probe) ---------------------------------------------------------
// Every wave runs the same bounded loop: 32 bf16 MFMAs + a few VALU instructions per trip, the wall clock read once per trip;
// the loop ends when spin_ticks have passed (an exit condition every wave reaches: the 100 MHz counter always advances).
__global__ __launch_bounds__(512) void clock_probe_kernel(unsigned long long* __restrict__ out, unsigned int spin_ticks) {
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long c0 = __builtin_amdgcn_s_memtime();
    Frag a, b;
    const unsigned int seed = mix32(threadIdx.x * 2654435761u + blockIdx.x);
    a.u = u32x4_t{0x3F803F80u ^ (seed & 0x00070007u), 0x3F003F00u, 0x3E803E80u ^ ((seed >> 8) & 0x00030003u), 0x3F803F00u};
    b.u = u32x4_t{0x3F003F80u, 0x3E803F00u ^ ((seed >> 16) & 0x00070007u), 0x3F803E80u, 0x3F003F00u};
    f32x4_t acc[4] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
    float v = (float)(seed & 1023u) * 1e-3f;
    unsigned long long r1 = r0;
    for (int guard = 0; guard < (1 << 22); ++guard) {                 // (hard bound on top of the time condition)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.h, acc[j], 0, 0, 0);
            v = __builtin_fmaf(v, 0.999f, 0.001f);
            v = __builtin_fmaf(v, 1.001f, -0.001f);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = acc[j] * 0.5f;           // keep the sums finite
        r1 = __builtin_amdgcn_s_memrealtime();
        if (r1 - r0 >= (unsigned long long)spin_ticks) break;
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    float sink = v;
#pragma unroll
    for (int j = 0; j < 4; ++j) sink += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = c1 - c0;
        out[2 * blockIdx.x + 1] = (r1 - r0) | (sink == 12345.678f ? 1ull << 63 : 0ull);     // (the sink keeps the work alive)
    }
}
extern "C" int m2m_clock_probe(uint64_t* out, int nwg, int spin_ticks, void* stream) {
    if (!out || nwg < 1 || nwg > 4096 || spin_ticks < 1) { m2m_set_error("clock_probe: bad arguments", __FILE__, __LINE__); return -1; }
    if (spin_ticks > 1000000) spin_ticks = 1000000;
    hipLaunchKernelGGL(clock_probe_kernel, dim3(nwg), dim3(512), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<unsigned long long*>(out), (unsigned int)spin_ticks);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}
