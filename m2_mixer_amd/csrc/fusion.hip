// Fusion functions other than ConcatFusion: SumFusion, MeanFusion, MaxFusion and BiModalGatedUnit
// (reference: modules/fusion.py:7-55, :190-221, :258-272), forward and backward.
//
// Every tensor is fp32 (rows = B * N, D), rows contiguous.  ConcatFusion needs no launch (the towers write the halves of the
// fused buffer); the other fusions read the two towers' own output buffers and write the fusion tower's input.
//
// The gate runs in exact fp32 (VALU FMAs) in both precisions and reads its weights from the fp32 masters: Adam and the operand
// re-pack need no packed image of them.  tanh(W1 a + b1), tanh(W2 b + b2) and z are saved by a training forward; the backward
// reads them instead of recomputing three products.  Its weight gradients are per-workgroup partial sums over fixed row chunks,
// added in chunk order by a second launch (no float atomics: a bf16 step stays bit-reproducible).
#include "host.h"

#define FUS_THREADS 256
// rows per thread of the forward / backward tiles (template argument GATE_RPT): 16, or 4 where 16 would leave the chip
// under-filled (gate_rpt16)
#define GATE_RS 32           // rows per LDS stage of the weight-gradient partial kernel

// ---- sum / mean / max ---------------------------------------------------------------------------------------------------
template <int MODE>
__device__ __forceinline__ float fuse1(float a, float b) {
    if (MODE == M2M_FUSION_SUM) return a + b;
    if (MODE == M2M_FUSION_MEAN) return (a + b) * 0.5f;
    return fmaxf(a, b);
}

template <int MODE>
__global__ __launch_bounds__(FUS_THREADS) void fusion_fwd_kernel(const float4* __restrict__ a, const float4* __restrict__ b,
                                                                 float4* __restrict__ y, int64_t n4) {
    for (int64_t i = blockIdx.x * (int64_t)FUS_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * FUS_THREADS) {
        const float4 u = a[i], v = b[i];
        y[i] = make_float4(fuse1<MODE>(u.x, v.x), fuse1<MODE>(u.y, v.y), fuse1<MODE>(u.z, v.z), fuse1<MODE>(u.w, v.w));
    }
}

// torch.maximum's backward: the larger input takes the gradient, a tie gives each input half of it
__device__ __forceinline__ void max_bwd1(float a, float b, float g, float& da, float& db) {
    da = a > b ? g : (a == b ? 0.5f * g : 0.f);
    db = b > a ? g : (a == b ? 0.5f * g : 0.f);
}

template <int MODE>
__global__ __launch_bounds__(FUS_THREADS) void fusion_bwd_kernel(const float4* __restrict__ a, const float4* __restrict__ b,
                                                                 const float4* __restrict__ dy, float4* __restrict__ da,
                                                                 float4* __restrict__ db, int64_t n4) {
    for (int64_t i = blockIdx.x * (int64_t)FUS_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * FUS_THREADS) {
        const float4 g = dy[i];
        if (MODE == M2M_FUSION_MAX) {
            const float4 u = a[i], v = b[i];
            float4 p, q;
            max_bwd1(u.x, v.x, g.x, p.x, q.x);
            max_bwd1(u.y, v.y, g.y, p.y, q.y);
            max_bwd1(u.z, v.z, g.z, p.z, q.z);
            max_bwd1(u.w, v.w, g.w, p.w, q.w);
            da[i] = p;
            db[i] = q;
        } else {
            const float s = MODE == M2M_FUSION_MEAN ? 0.5f : 1.f;
            const float4 h = make_float4(g.x * s, g.y * s, g.z * s, g.w * s);
            da[i] = h;
            db[i] = h;
        }
    }
}

static int elem_grid(int64_t n4) {
    const int64_t g = (n4 + FUS_THREADS - 1) / FUS_THREADS;
    return (int)(g < 2048 ? (g < 1 ? 1 : g) : 2048);
}

static bool elem_args_ok(int mode, int64_t n, std::initializer_list<const void*> ptrs) {
    if (mode != M2M_FUSION_SUM && mode != M2M_FUSION_MEAN && mode != M2M_FUSION_MAX) {
        m2m_set_error("fusion: mode must be M2M_FUSION_SUM, _MEAN or _MAX", __FILE__, __LINE__);
        return false;
    }
    if (n < 0 || (n & 3)) {
        m2m_set_error("fusion: the element count must be a non-negative multiple of 4", __FILE__, __LINE__);
        return false;
    }
    for (const void* p : ptrs)
        if (!p || (reinterpret_cast<uintptr_t>(p) & 15)) {
            m2m_set_error("fusion: every buffer must be given and 16-byte aligned", __FILE__, __LINE__);
            return false;
        }
    return true;
}

extern "C" int m2m_fusion_forward(int mode, const float* a, const float* b, float* y, int64_t n, void* stream) {
    if (!elem_args_ok(mode, n, {a, b, y})) return -1;
    if (n == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t n4 = n / 4;
    const float4 *a4 = reinterpret_cast<const float4*>(a), *b4 = reinterpret_cast<const float4*>(b);
    float4* y4 = reinterpret_cast<float4*>(y);
    if (mode == M2M_FUSION_SUM) hipLaunchKernelGGL(fusion_fwd_kernel<M2M_FUSION_SUM>, dim3(elem_grid(n4)), dim3(FUS_THREADS), 0, st, a4, b4, y4, n4);
    else if (mode == M2M_FUSION_MEAN) hipLaunchKernelGGL(fusion_fwd_kernel<M2M_FUSION_MEAN>, dim3(elem_grid(n4)), dim3(FUS_THREADS), 0, st, a4, b4, y4, n4);
    else hipLaunchKernelGGL(fusion_fwd_kernel<M2M_FUSION_MAX>, dim3(elem_grid(n4)), dim3(FUS_THREADS), 0, st, a4, b4, y4, n4);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int m2m_fusion_backward(int mode, const float* a, const float* b, const float* dy, float* da, float* db, int64_t n,
                                   void* stream) {
    if (!elem_args_ok(mode, n, {a, b, dy, da, db})) return -1;
    if (n == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t n4 = n / 4;
    const float4 *a4 = reinterpret_cast<const float4*>(a), *b4 = reinterpret_cast<const float4*>(b);
    const float4* g4 = reinterpret_cast<const float4*>(dy);
    float4 *da4 = reinterpret_cast<float4*>(da), *db4 = reinterpret_cast<float4*>(db);
    if (mode == M2M_FUSION_SUM) hipLaunchKernelGGL(fusion_bwd_kernel<M2M_FUSION_SUM>, dim3(elem_grid(n4)), dim3(FUS_THREADS), 0, st, a4, b4, g4, da4, db4, n4);
    else if (mode == M2M_FUSION_MEAN) hipLaunchKernelGGL(fusion_bwd_kernel<M2M_FUSION_MEAN>, dim3(elem_grid(n4)), dim3(FUS_THREADS), 0, st, a4, b4, g4, da4, db4, n4);
    else hipLaunchKernelGGL(fusion_bwd_kernel<M2M_FUSION_MAX>, dim3(elem_grid(n4)), dim3(FUS_THREADS), 0, st, a4, b4, g4, da4, db4, n4);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- BiModalGatedUnit ----------------------------------------------------------------------------------------------------
// Forward / backward tile: TR = GATE_RPT * 256 / D rows per workgroup; thread t owns column t % D of rows
// (t / D) + (256 / D) * i, i < GATE_RPT.  The tile's rows of both inputs (forward) or of the three pre-activation
// gradients (backward) sit in LDS and are read as float4 broadcasts.

__device__ __forceinline__ float fast_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

template <int D, int GATE_RPT>
__global__ __launch_bounds__(FUS_THREADS) void gate_fwd_kernel(const m2m_gate g, const float* __restrict__ a,
                                                               const float* __restrict__ b, float* __restrict__ y,
                                                               int64_t rows, int save) {
    constexpr int RG = FUS_THREADS / D, TR = GATE_RPT * RG, D4 = D / 4;
    __shared__ __attribute__((aligned(16))) float sa[TR * D], sb[TR * D];
    const int64_t r0 = (int64_t)blockIdx.x * TR;
    for (int i = threadIdx.x; i < TR * D4; i += FUS_THREADS) {
        const int r = i / D4, c = i % D4;
        const bool in = r0 + r < rows;
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        reinterpret_cast<float4*>(sa)[i] = in ? reinterpret_cast<const float4*>(a + (r0 + r) * D)[c] : z4;
        reinterpret_cast<float4*>(sb)[i] = in ? reinterpret_cast<const float4*>(b + (r0 + r) * D)[c] : z4;
    }
    __syncthreads();
    const int j = threadIdx.x % D, rg = threadIdx.x / D;
    float h1[GATE_RPT], h2[GATE_RPT], hz[GATE_RPT];
#pragma unroll
    for (int i = 0; i < GATE_RPT; ++i) h1[i] = h2[i] = hz[i] = 0.f;
    // (the parameters sit in the flat buffer at whatever offset the reference's creation order gives them: 4-byte aligned only)
    const float* w1 = g.w1 + (int64_t)j * D;
    const float* w2 = g.w2 + (int64_t)j * D;
    const float* wza = g.wz + (int64_t)j * 2 * D;
    const float* wzb = wza + D;
    auto ld4 = [](const float* w, int k4) { return make_float4(w[4 * k4], w[4 * k4 + 1], w[4 * k4 + 2], w[4 * k4 + 3]); };
    for (int k4 = 0; k4 < D4; ++k4) {
        const float4 p = ld4(w1, k4), q = ld4(w2, k4), u = ld4(wza, k4), v = ld4(wzb, k4);
#pragma unroll
        for (int i = 0; i < GATE_RPT; ++i) {
            const int r = rg + RG * i;
            const float4 x = reinterpret_cast<const float4*>(sa + r * D)[k4];
            const float4 w = reinterpret_cast<const float4*>(sb + r * D)[k4];
            h1[i] = fmaf(x.x, p.x, h1[i]); h1[i] = fmaf(x.y, p.y, h1[i]); h1[i] = fmaf(x.z, p.z, h1[i]); h1[i] = fmaf(x.w, p.w, h1[i]);
            h2[i] = fmaf(w.x, q.x, h2[i]); h2[i] = fmaf(w.y, q.y, h2[i]); h2[i] = fmaf(w.z, q.z, h2[i]); h2[i] = fmaf(w.w, q.w, h2[i]);
            hz[i] = fmaf(x.x, u.x, hz[i]); hz[i] = fmaf(x.y, u.y, hz[i]); hz[i] = fmaf(x.z, u.z, hz[i]); hz[i] = fmaf(x.w, u.w, hz[i]);
            hz[i] = fmaf(w.x, v.x, hz[i]); hz[i] = fmaf(w.y, v.y, hz[i]); hz[i] = fmaf(w.z, v.z, hz[i]); hz[i] = fmaf(w.w, v.w, hz[i]);
        }
    }
    const float c1 = g.b1[j], c2 = g.b2[j], cz = g.bz[j];
#pragma unroll
    for (int i = 0; i < GATE_RPT; ++i) {
        const int64_t row = r0 + rg + RG * i;
        if (row >= rows) continue;
        const float t1 = tanhf(h1[i] + c1), t2 = tanhf(h2[i] + c2), z = fast_sigmoid(hz[i] + cz);
        const int64_t o = row * D + j;
        y[o] = z * t1 + (1.f - z) * t2;
        if (save) {
            g.t1[o] = t1;
            g.t2[o] = t2;
            g.z[o] = z;
        }
    }
}

// d_a = dh1 W1 + dhz Wz[:, :D], d_b = dh2 W2 + dhz Wz[:, D:]; the three pre-activation gradients also go to g.dh
// ((rows, 3 D): dh1 | dh2 | dhz) for the weight-gradient launch.
template <int D, int GATE_RPT>
__global__ __launch_bounds__(FUS_THREADS) void gate_bwd_kernel(const m2m_gate g, const float* __restrict__ dy,
                                                               float* __restrict__ da, float* __restrict__ db, int64_t rows) {
    constexpr int RG = FUS_THREADS / D, TR = GATE_RPT * RG, D4 = D / 4;
    __shared__ __attribute__((aligned(16))) float s1[TR * D], s2[TR * D], sz[TR * D];
    const int64_t r0 = (int64_t)blockIdx.x * TR;
    for (int i = threadIdx.x; i < TR * D; i += FUS_THREADS) {
        const int r = i / D, c = i % D;
        const int64_t row = r0 + r;
        float d1 = 0.f, d2 = 0.f, dz = 0.f;
        if (row < rows) {
            const int64_t o = row * D + c;
            const float gy = dy[o], t1 = g.t1[o], t2 = g.t2[o], z = g.z[o];
            d1 = gy * z * (1.f - t1 * t1);
            d2 = gy * (1.f - z) * (1.f - t2 * t2);
            dz = gy * (t1 - t2) * (z * (1.f - z));
            float* dh = g.dh + row * 3 * D;
            dh[c] = d1;
            dh[D + c] = d2;
            dh[2 * D + c] = dz;
        }
        s1[i] = d1;
        s2[i] = d2;
        sz[i] = dz;
    }
    __syncthreads();
    const int k = threadIdx.x % D, rg = threadIdx.x / D;
    float ga[GATE_RPT], gb[GATE_RPT];
#pragma unroll
    for (int i = 0; i < GATE_RPT; ++i) ga[i] = gb[i] = 0.f;
    for (int j4 = 0; j4 < D4; ++j4) {
        float w1[4], w2[4], wa[4], wb[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int jj = 4 * j4 + e;
            w1[e] = g.w1[(int64_t)jj * D + k];
            w2[e] = g.w2[(int64_t)jj * D + k];
            wa[e] = g.wz[(int64_t)jj * 2 * D + k];
            wb[e] = g.wz[(int64_t)jj * 2 * D + D + k];
        }
#pragma unroll
        for (int i = 0; i < GATE_RPT; ++i) {
            const int r = rg + RG * i;
            const float4 p = reinterpret_cast<const float4*>(s1 + r * D)[j4];
            const float4 q = reinterpret_cast<const float4*>(s2 + r * D)[j4];
            const float4 u = reinterpret_cast<const float4*>(sz + r * D)[j4];
            ga[i] = fmaf(p.x, w1[0], ga[i]); ga[i] = fmaf(p.y, w1[1], ga[i]); ga[i] = fmaf(p.z, w1[2], ga[i]); ga[i] = fmaf(p.w, w1[3], ga[i]);
            ga[i] = fmaf(u.x, wa[0], ga[i]); ga[i] = fmaf(u.y, wa[1], ga[i]); ga[i] = fmaf(u.z, wa[2], ga[i]); ga[i] = fmaf(u.w, wa[3], ga[i]);
            gb[i] = fmaf(q.x, w2[0], gb[i]); gb[i] = fmaf(q.y, w2[1], gb[i]); gb[i] = fmaf(q.z, w2[2], gb[i]); gb[i] = fmaf(q.w, w2[3], gb[i]);
            gb[i] = fmaf(u.x, wb[0], gb[i]); gb[i] = fmaf(u.y, wb[1], gb[i]); gb[i] = fmaf(u.z, wb[2], gb[i]); gb[i] = fmaf(u.w, wb[3], gb[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < GATE_RPT; ++i) {
        const int64_t row = r0 + rg + RG * i;
        if (row >= rows) continue;
        da[row * D + k] = ga[i];
        db[row * D + k] = gb[i];
    }
}

// Weight gradients.  The flat gradient image P (4 D^2 + 3 D floats) is laid out as the parameters are created:
// W1 (D x D) | b1 | W2 (D x D) | b2 | Wz (D x 2D) | bz.  Four D x D products: dh1^T a -> W1, dh2^T b -> W2,
// dhz^T a -> Wz[:, :D], dhz^T b -> Wz[:, D:]; the biases are the column sums of dh1, dh2, dhz.
// Partial kernel: grid (tiles of T x T, 4 products, row chunks); workgroup (tile, product, chunk) writes its tile of the
// chunk's sum into part[chunk * P + ...] -- every element of P is written exactly once per chunk.
// Reduce kernel: g += sum over chunks in chunk order.
static int gate_tile(int D) { return D < 64 ? D : 64; }

static int64_t gate_chunks(int64_t rows, int D) {
    const int T = gate_tile(D);
    const int64_t wgs = 4LL * (D / T) * (D / T);
    int64_t c = 1024 / wgs;
    const int64_t cap = (rows + 4 * GATE_RS - 1) / (4 * GATE_RS);    // at least four row stages per chunk
    if (c > cap) c = cap;
    return c < 1 ? 1 : c;
}

static int64_t gate_p(int D) { return 4LL * D * D + 3LL * D; }

template <int D, int T>
__global__ __launch_bounds__((T / 4) * (T / 4)) void gate_wgrad_part_kernel(const m2m_gate g, const float* __restrict__ a,
                                                                            const float* __restrict__ b, int64_t rows,
                                                                            int64_t chunk_rows) {
    constexpr int NT = (T / 4) * (T / 4), TQ = T / 4;
    __shared__ __attribute__((aligned(16))) float sh[GATE_RS * T], sx[GATE_RS * T];
    const int tiles = D / T;
    const int tj = blockIdx.x / tiles, tk = blockIdx.x % tiles, prod = blockIdx.y;
    const int64_t chunk = blockIdx.z;
    const int hcol = (prod == 0 ? 0 : prod == 1 ? D : 2 * D) + tj * T;      // column of g.dh
    const float* x = (prod == 0 || prod == 2) ? a : b;
    const int xcol = tk * T;
    const int jq = threadIdx.x / TQ, kq = threadIdx.x % TQ;
    float acc[4][4], bias[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        bias[u] = 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.f;
    }
    const int64_t lo = chunk * chunk_rows;
    const int64_t hi = lo + chunk_rows < rows ? lo + chunk_rows : rows;
    for (int64_t s = lo; s < hi; s += GATE_RS) {
        __syncthreads();
        for (int i = threadIdx.x; i < GATE_RS * TQ; i += NT) {
            const int r = i / TQ, c = i % TQ;
            const bool in = s + r < hi;
            const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
            reinterpret_cast<float4*>(sh)[i] = in ? reinterpret_cast<const float4*>(g.dh + (s + r) * 3 * D + hcol)[c] : z4;
            reinterpret_cast<float4*>(sx)[i] = in ? reinterpret_cast<const float4*>(x + (s + r) * D + xcol)[c] : z4;
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < GATE_RS; ++r) {
            const float4 h = reinterpret_cast<const float4*>(sh + r * T)[jq];
            const float4 w = reinterpret_cast<const float4*>(sx + r * T)[kq];
            const float hv[4] = {h.x, h.y, h.z, h.w}, wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                bias[u] += hv[u];
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(hv[u], wv[v], acc[u][v]);
            }
        }
    }
    // destination inside P
    int64_t wofs, ld, bofs;
    if (prod == 0) { wofs = 0; ld = D; bofs = (int64_t)D * D; }
    else if (prod == 1) { wofs = (int64_t)D * D + D; ld = D; bofs = 2LL * D * D + D; }
    else { wofs = 2LL * D * D + 2 * D + (prod == 3 ? D : 0); ld = 2 * D; bofs = prod == 2 ? 4LL * D * D + 2 * D : -1; }
    float* P = g.part + chunk * (4LL * D * D + 3LL * D);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int j = tj * T + 4 * jq + u;
        float4 o = make_float4(acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
        *reinterpret_cast<float4*>(P + wofs + (int64_t)j * ld + xcol + 4 * kq) = o;
        if (bofs >= 0 && tk == 0 && kq == 0) P[bofs + j] = bias[u];
    }
}

__global__ __launch_bounds__(FUS_THREADS) void gate_wgrad_reduce_kernel(const m2m_gate g, int D, int64_t nchunks) {
    const int64_t P = 4LL * D * D + 3LL * D;
    const int64_t dd = (int64_t)D * D;
    for (int64_t i = blockIdx.x * (int64_t)FUS_THREADS + threadIdx.x; i < P; i += (int64_t)gridDim.x * FUS_THREADS) {
        float s = 0.f;
        for (int64_t c = 0; c < nchunks; ++c) s += g.part[c * P + i];
        float* dst;
        if (i < dd) dst = g.g_w1 + i;
        else if (i < dd + D) dst = g.g_b1 + (i - dd);
        else if (i < 2 * dd + D) dst = g.g_w2 + (i - dd - D);
        else if (i < 2 * dd + 2 * D) dst = g.g_b2 + (i - 2 * dd - D);
        else if (i < 4 * dd + 2 * D) dst = g.g_wz + (i - 2 * dd - 2 * D);
        else dst = g.g_bz + (i - 4 * dd - 2 * D);
        *dst += s;
    }
}

static bool gate_ok(const m2m_gate* g, int64_t rows, bool need_grads) {
    if (!g || (g->D != 32 && g->D != 64 && g->D != 128 && g->D != 256) || rows < 0) {
        m2m_set_error("gate: D must be 32, 64, 128 or 256", __FILE__, __LINE__);
        return false;
    }
    const void* w[] = {g->w1, g->b1, g->w2, g->b2, g->wz, g->bz};
    for (const void* p : w)
        if (!p || (reinterpret_cast<uintptr_t>(p) & 3)) {
            m2m_set_error("gate: the six parameters must be given (4-byte aligned)", __FILE__, __LINE__);
            return false;
        }
    if (need_grads) {
        const void* gr[] = {g->g_w1, g->g_b1, g->g_w2, g->g_b2, g->g_wz, g->g_bz};
        const void* q[] = {g->t1, g->t2, g->z, g->dh, g->part};
        for (const void* p : gr)
            if (!p || (reinterpret_cast<uintptr_t>(p) & 3)) {
                m2m_set_error("gate: backward needs the six gradients (4-byte aligned)", __FILE__, __LINE__);
                return false;
            }
        for (const void* p : q)
            if (!p || (reinterpret_cast<uintptr_t>(p) & 15)) {
                m2m_set_error("gate: backward needs the saved activations, dh and part (16-byte aligned)", __FILE__, __LINE__);
                return false;
            }
    }
    return true;
}

extern "C" int64_t m2m_gate_part_floats(int64_t rows, int D) {
    if (D != 32 && D != 64 && D != 128 && D != 256) return -1;
    return gate_chunks(rows < 1 ? 1 : rows, D) * gate_p(D);
}

// 16 rows per thread where that still gives >= 512 workgroups (two per CU), else 4 (M2-Mixer-B at batch 512: 2048 rows were
// 64 workgroups of 16 rows per thread)
static bool gate_rpt16(int64_t rows, int D) { return rows >= 512LL * 16 * (FUS_THREADS / D); }

template <int D>
static void launch_gate_fwd(const m2m_gate& g, const float* a, const float* b, float* y, int64_t rows, int save, hipStream_t st) {
    if (gate_rpt16(rows, D)) {
        constexpr int TR = 16 * (FUS_THREADS / D);
        hipLaunchKernelGGL((gate_fwd_kernel<D, 16>), dim3((unsigned)((rows + TR - 1) / TR)), dim3(FUS_THREADS), 0, st, g, a, b, y, rows, save);
    } else {
        constexpr int TR = 4 * (FUS_THREADS / D);
        hipLaunchKernelGGL((gate_fwd_kernel<D, 4>), dim3((unsigned)((rows + TR - 1) / TR)), dim3(FUS_THREADS), 0, st, g, a, b, y, rows, save);
    }
}

extern "C" int m2m_gate_forward(const m2m_gate* g, const float* a, const float* b, float* y, int64_t rows, int save, void* stream) {
    if (!gate_ok(g, rows, false)) return -1;
    if (!a || !b || !y || (save && (!g->t1 || !g->t2 || !g->z))) {
        m2m_set_error("gate: forward needs a, b, y (and t1, t2, z when saving)", __FILE__, __LINE__);
        return -1;
    }
    if (rows == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (g->D) {
        case 32: launch_gate_fwd<32>(*g, a, b, y, rows, save, st); break;
        case 64: launch_gate_fwd<64>(*g, a, b, y, rows, save, st); break;
        case 128: launch_gate_fwd<128>(*g, a, b, y, rows, save, st); break;
        default: launch_gate_fwd<256>(*g, a, b, y, rows, save, st); break;
    }
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}

template <int D>
static void launch_gate_bwd(const m2m_gate& g, const float* dy, float* da, float* db, int64_t rows, hipStream_t st) {
    if (gate_rpt16(rows, D)) {
        constexpr int TR = 16 * (FUS_THREADS / D);
        hipLaunchKernelGGL((gate_bwd_kernel<D, 16>), dim3((unsigned)((rows + TR - 1) / TR)), dim3(FUS_THREADS), 0, st, g, dy, da, db, rows);
    } else {
        constexpr int TR = 4 * (FUS_THREADS / D);
        hipLaunchKernelGGL((gate_bwd_kernel<D, 4>), dim3((unsigned)((rows + TR - 1) / TR)), dim3(FUS_THREADS), 0, st, g, dy, da, db, rows);
    }
}

extern "C" int m2m_gate_backward(const m2m_gate* g, const float* dy, float* da, float* db, int64_t rows, void* stream) {
    if (!gate_ok(g, rows, true)) return -1;
    if (!dy || !da || !db) {
        m2m_set_error("gate: backward needs dy, da and db", __FILE__, __LINE__);
        return -1;
    }
    if (rows == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (g->D) {
        case 32: launch_gate_bwd<32>(*g, dy, da, db, rows, st); break;
        case 64: launch_gate_bwd<64>(*g, dy, da, db, rows, st); break;
        case 128: launch_gate_bwd<128>(*g, dy, da, db, rows, st); break;
        default: launch_gate_bwd<256>(*g, dy, da, db, rows, st); break;
    }
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}

template <int D>
static void launch_gate_part(const m2m_gate& g, const float* a, const float* b, int64_t rows, int64_t nch, int64_t chunk_rows,
                             hipStream_t st) {
    constexpr int T = D < 64 ? D : 64;
    hipLaunchKernelGGL((gate_wgrad_part_kernel<D, T>), dim3((D / T) * (D / T), 4, (unsigned)nch), dim3((T / 4) * (T / 4)), 0, st,
                       g, a, b, rows, chunk_rows);
}

extern "C" int m2m_gate_wgrad(const m2m_gate* g, const float* a, const float* b, int64_t rows, void* stream) {
    if (!gate_ok(g, rows, true)) return -1;
    if (!a || !b) {
        m2m_set_error("gate: wgrad needs a and b", __FILE__, __LINE__);
        return -1;
    }
    if (rows == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int D = g->D;
    const int64_t nch = gate_chunks(rows, D);
    int64_t chunk_rows = (rows + nch - 1) / nch;
    chunk_rows = (chunk_rows + GATE_RS - 1) / GATE_RS * GATE_RS;
    switch (D) {
        case 32: launch_gate_part<32>(*g, a, b, rows, nch, chunk_rows, st); break;
        case 64: launch_gate_part<64>(*g, a, b, rows, nch, chunk_rows, st); break;
        case 128: launch_gate_part<128>(*g, a, b, rows, nch, chunk_rows, st); break;
        default: launch_gate_part<256>(*g, a, b, rows, nch, chunk_rows, st); break;
    }
    M2M_CHECK_HIP(hipGetLastError());
    const int64_t P = gate_p(D);
    const int grid = (int)((P + FUS_THREADS - 1) / FUS_THREADS < 1024 ? (P + FUS_THREADS - 1) / FUS_THREADS : 1024);
    hipLaunchKernelGGL(gate_wgrad_reduce_kernel, dim3(grid), dim3(FUS_THREADS), 0, st, *g, D, nch);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}
