// The classification heads' kernel body around the loss, shared by heads.hip (cross-entropy, BCE) and edl.hip (evidential):
// one Linear on the token mean per head, forward and backward in one launch on a grid of m2m_heads_part_tiles(B) sample tiles x
// heads.  A kernel is
//     HEADS_TILE(ha)  HEADS_STAGE()  barrier  HEADS_LOGITS()  barrier  <its loss phase>  barrier  heads_loss_sum  HEADS_BACKWARD()
// where the loss phase reads the logits from `lg`, overwrites them with d loss / d logits (0 for samples >= ns) and leaves one
// loss term per sample in `red`.  The phases carry three contracts: the bits of the token-mean pooling (those of the towers' own
// token mean), the slot layout m2m_towers_wgrad_heads adds, and the tile count of m2m_heads_part_tiles.
//
// Why three phases are macros and not __forceinline__ templates: the pass pipeline optimises an always_inline callee on its own
// before it inlines it, and with any of these three behind a call every heads_kernel<...> instantiation compiled to other
// instructions than before (block layout, address arithmetic, 2 to 40 instructions' difference; scripts/isa_compare.sh).  Text
// expands before the first pass, so the kernel of the measured step is instruction for instruction what it was when the phases
// stood written out in heads.hip -- profiles/heads_body_isa.txt.  heads_loss_sum is a function because as one it changes nothing.
// The macros use the names of the kernel they expand in: the template parameters S (samples per workgroup) and DD (hidden_dim),
// the arguments B, K, logits_out, and what HEADS_TILE declares.
#pragma once
#include "dispatch.h"

#define HEAD_S 16       // samples per workgroup (small: the launch sits between forward and backward on the critical path)
#define HEAD_MAXK 32
#define HEAD_MAXH 4

struct HeadArgs {
    m2m_head h[HEAD_MAXH];
    // ABI 18 (the _w entry points, m2m_heads_edl): the heads' loss coefficients in device memory, nheads floats, read in place of
    // m2m_head.weight -- a captured graph then follows a loss-weight schedule (models/avmnist.py:332-339).  NULL: m2m_head.weight.
    const float* weights;
};
// (the kernels index h by blockIdx.y < nheads; the rest repeats the first head)
static inline HeadArgs heads_args(const m2m_head* heads, int nheads, const float* weights) {
    HeadArgs ha;
    for (int i = 0; i < HEAD_MAXH; ++i) ha.h[i] = heads[i < nheads ? i : 0];
    ha.weights = weights;
    return ha;
}

// Dynamic LDS of a launch: the arrays of HEADS_TILE, then the `ext` floats of the loss phase's own.
constexpr size_t heads_lds_bytes(int S, int D, int ext) {
    return sizeof(float) * ((size_t)S * (D + 4) + (size_t)HEAD_MAXK * (D + 4) + (size_t)S * HEAD_MAXK + S + ext);
}

// S: HEAD_S, or 4 at small batch (heads_samples_per_wg: at the MM-IMDb cfg batch 32 samples x 3 heads were 6 workgroups).
// DD: compile time, so that the dot-product loops unroll and their LDS reads are requested in batches.  Round 4: the kernel was a
// chain of ~300 dependent LDS round trips (runtime loop bounds: nothing unrolled, every ds_read followed by s_waitcnt
// lgkmcnt(0)) -- 13.3 us for 4 MFLOP on the critical path between forward and backward.  Now: 16-byte LDS accesses on rows padded
// to D + 4, four lanes x eight float4 per logit, the loss on 32 lanes per sample, the gradient phases with the sample / class
// loops unrolled.

// ---- the LDS layout and the workgroup's place in the grid; `args`: the kernel's HeadArgs ----
#define HEADS_TILE(args)                                                                                                          \
    extern __shared__ __attribute__((aligned(16))) char smem[];                                                                   \
    constexpr int D = DD, DL = DD + 4, D4 = DD / 4;                                                                               \
    float* pl = reinterpret_cast<float*>(smem);          /* pooled tile [S][DL] */                                                \
    float* wl = pl + S * DL;                              /* weights     [HEAD_MAXK][DL] */                                        \
    float* lg = wl + HEAD_MAXK * DL;                      /* logits / dlogits [S][HEAD_MAXK] */                                    \
    float* red = lg + S * HEAD_MAXK;                      /* [S] loss terms */                                                     \
    float* ext = red + S;                                 /* the loss phase's own floats (heads_lds_bytes) */                      \
    const int tid = threadIdx.x;                                                                                                  \
    const int hI = blockIdx.y;                                                                                                    \
    const m2m_head& hd = (args).h[hI];                                                                                            \
    const float hw = (args).weights ? (args).weights[hI] : hd.weight;      /* this head's coefficient in the total loss */        \
    const int s0 = blockIdx.x * S;                                                                                                \
    const int ns = min(S, B - s0);

// ---- pooled rows and head weights -> LDS (16-byte accesses; every global load requested before the first LDS write).
// ---- A head with `tokens` pools the tower output itself: x.mean(dim=1), tokens in order, eight loads in flight per round trip,
// ---- then * (1 / N) -- the order and the product of the towers' token-mean launch this replaces: same bits.
// ---- Rows >= ns of the pooled tile and rows >= K of the weights are zeros.
#define HEADS_STAGE()                                                                                                             \
    {                                                                                                                             \
        constexpr int NP = (S * D4 + NTHREADS - 1) / NTHREADS, NW = (HEAD_MAXK * D4 + NTHREADS - 1) / NTHREADS;                   \
        f32x4_t pv[NP], wv[NW];                                                                                                   \
        _Pragma("unroll") for (int i = 0; i < NP; ++i) {                                                                          \
            const int idx = tid + i * NTHREADS, sI = idx / D4, c = (idx % D4) * 4;                                                \
            pv[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};                                                                                  \
            if (idx < S * D4 && sI < ns) {                                                                                        \
                if (hd.tokens) {                                                                                                  \
                    const float* col = hd.tokens + (long)(s0 + sI) * hd.tok_sample_stride + c;                                    \
                    const int N = hd.ntok;                                                                                        \
                    f32x4_t a = f32x4_t{0.f, 0.f, 0.f, 0.f};                                                                      \
                    for (int n0 = 0; n0 < N; n0 += 8) {                                                                           \
                        f32x4_t t8[8];                                                                                            \
                        _Pragma("unroll") for (int j = 0; j < 8; ++j)                                                             \
                            t8[j] = *reinterpret_cast<const f32x4_t*>(col + (long)min(n0 + j, N - 1) * D);                        \
                        _Pragma("unroll") for (int j = 0; j < 8; ++j)                                                             \
                            if (n0 + j < N) a += t8[j];                                                                           \
                    }                                                                                                             \
                    pv[i] = a * (1.0f / (float)N);                                                                                \
                } else pv[i] = *reinterpret_cast<const f32x4_t*>(hd.pooled + (long)(s0 + sI) * D + c);                            \
            }                                                                                                                     \
        }                                                                                                                         \
        _Pragma("unroll") for (int i = 0; i < NW; ++i) {                                                                          \
            const int idx = tid + i * NTHREADS;                                                                                   \
            wv[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};                                                                                  \
            if (idx < K * D4) wv[i] = *reinterpret_cast<const f32x4_t*>(hd.w + (long)idx * 4);                                    \
        }                                                                                                                         \
        _Pragma("unroll") for (int i = 0; i < NP; ++i) {                                                                          \
            const int idx = tid + i * NTHREADS;                                                                                   \
            if (idx < S * D4) *reinterpret_cast<f32x4_t*>(pl + (idx / D4) * DL + (idx % D4) * 4) = pv[i];                         \
        }                                                                                                                         \
        _Pragma("unroll") for (int i = 0; i < NW; ++i) {                                                                          \
            const int idx = tid + i * NTHREADS;                                                                                   \
            if (idx < HEAD_MAXK * D4) *reinterpret_cast<f32x4_t*>(wl + (idx / D4) * DL + (idx % D4) * 4) = wv[i];                 \
        }                                                                                                                         \
    }

// ---- logits: 4 adjacent lanes split each D-long dot product, float4 chunks interleaved over the lanes (NC chunks per lane) ----
#define HEADS_LOGITS()                                                                                                            \
    for (int idx = tid >> 2; idx < S * K; idx += NTHREADS / 4) {                                                                  \
        const int sI = idx / K, k = idx % K, part = tid & 3;                                                                      \
        constexpr int NC = D4 / 4;                                                                                                \
        f32x4_t a4[NC], b4[NC];                                                                                                   \
        _Pragma("unroll") for (int c = 0; c < NC; ++c) {                                                                          \
            a4[c] = *reinterpret_cast<const f32x4_t*>(pl + sI * DL + 4 * (part + 4 * c));                                         \
            b4[c] = *reinterpret_cast<const f32x4_t*>(wl + k * DL + 4 * (part + 4 * c));                                          \
        }                                                                                                                         \
        float a = 0.f;                                                                                                            \
        _Pragma("unroll") for (int c = 0; c < NC; ++c)                                                                            \
            _Pragma("unroll") for (int e = 0; e < 4; ++e) a = __builtin_fmaf(a4[c][e], b4[c][e], a);                              \
        a = wave_sum_xor(a, 4) + hd.b[k];                                                                                         \
        if (part == 0) {                                                                                                          \
            lg[sI * HEAD_MAXK + k] = a;                                                                                           \
            if (sI < ns) logits_out[((long)hI * B + s0 + sI) * K + k] = a;                                                        \
        }                                                                                                                         \
    }

// ---- the workgroup's share of the batch-mean loss: thread 0 adds `red` in sample order (behind a barrier after the loss phase).
// ---- red2 (or NULL): a second term -- the evidential KL -- that enters the loss times coef2 and goes to out2 (or NULL) as it is.
template <int S>
static __device__ __forceinline__ void heads_loss_sum(const float* red, int tid, int hI, float hw, int B, float* losses, int nheads,
                                                      const float* red2 = nullptr, float coef2 = 0.f, float* out2 = nullptr) {
    if (tid != 0) return;
    float t = 0.f;
#pragma unroll
    for (int sI = 0; sI < S; ++sI) t += red[sI];
    t /= (float)B;
    if (red2) {
        float t2 = 0.f;
#pragma unroll
        for (int sI = 0; sI < S; ++sI) t2 += red2[sI];
        t2 /= (float)B;
        t += coef2 * t2;
        if (out2) atomicAdd(out2 + hI, t2);
    }
    atomicAdd(losses + hI, t);
    atomicAdd(losses + nheads, t * hw);
}

// ---- backward, where the head has d_pooled (training).
// ---- d_pooled[s][d..d+3] = sum_k dl[s][k] w[k][d..d+3]: thread = (sample, float4 of d), k ascending, four k per batch of reads.
// ---- g_w[k][d..d+3] = sum_s dl[s][k] pooled[s][d..d+3]: thread = (class, float4 of d), samples ascending, the loop unrolled;
// ---- g_b likewise.  They are added with atomics, or -- g_part -- stored to this workgroup's slot, whose two trailing loss entries
// ---- are zeroed (the losses stay atomics); m2m_towers_wgrad_heads adds the slots in a fixed order.
#define HEADS_BACKWARD()                                                                                                          \
    if (hd.d_pooled) {                                                                                                            \
        for (int idx = tid; idx < ns * D4; idx += NTHREADS) {                                                                     \
            const int sI = idx / D4, c = (idx % D4) * 4;                                                                          \
            f32x4_t a = f32x4_t{0.f, 0.f, 0.f, 0.f};                                                                              \
            int k = 0;                                                                                                            \
            for (; k + 4 <= K; k += 4) {                                                                                          \
                f32x4_t w4[4];                                                                                                    \
                float d4[4];                                                                                                      \
                _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                                   \
                    w4[j] = *reinterpret_cast<const f32x4_t*>(wl + (k + j) * DL + c);                                             \
                    d4[j] = lg[sI * HEAD_MAXK + k + j];                                                                           \
                }                                                                                                                 \
                _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                                     \
                    _Pragma("unroll") for (int e = 0; e < 4; ++e) a[e] = __builtin_fmaf(d4[j], w4[j][e], a[e]);                   \
            }                                                                                                                     \
            for (; k < K; ++k) {                                                                                                  \
                const f32x4_t w4 = *reinterpret_cast<const f32x4_t*>(wl + k * DL + c);                                            \
                const float dk = lg[sI * HEAD_MAXK + k];                                                                          \
                _Pragma("unroll") for (int e = 0; e < 4; ++e) a[e] = __builtin_fmaf(dk, w4[e], a[e]);                             \
            }                                                                                                                     \
            *reinterpret_cast<f32x4_t*>(hd.d_pooled + (long)(s0 + sI) * D + c) = a;                                               \
        }                                                                                                                         \
        float* slot = hd.g_part ? hd.g_part + (long)blockIdx.x * M2M_SPLIT_GPART : nullptr;                                       \
        for (int idx = tid; idx < K * D4; idx += NTHREADS) {                                                                      \
            const int k = idx / D4, c = (idx % D4) * 4;                                                                           \
            f32x4_t p4[S];                                                                                                        \
            float d1[S];                                                                                                          \
            _Pragma("unroll") for (int sI = 0; sI < S; ++sI) {                                                                    \
                p4[sI] = *reinterpret_cast<const f32x4_t*>(pl + sI * DL + c);                                                     \
                d1[sI] = lg[sI * HEAD_MAXK + k];                                                                                  \
            }                                                                                                                     \
            f32x4_t a = f32x4_t{0.f, 0.f, 0.f, 0.f};                                                                              \
            _Pragma("unroll") for (int sI = 0; sI < S; ++sI)                                                                      \
                _Pragma("unroll") for (int e = 0; e < 4; ++e) a[e] = __builtin_fmaf(d1[sI], p4[sI][e], a[e]);                     \
            if (slot) *reinterpret_cast<f32x4_t*>(slot + (long)k * D + c) = a;                                                    \
            else {                                                                                                                \
                _Pragma("unroll") for (int e = 0; e < 4; ++e) atomicAdd(hd.g_w + (long)k * D + c + e, a[e]);                      \
            }                                                                                                                     \
        }                                                                                                                         \
        if (tid < K) {                                                                                                            \
            float a = 0.f;                                                                                                        \
            _Pragma("unroll") for (int sI = 0; sI < S; ++sI) a += lg[sI * HEAD_MAXK + tid];                                       \
            if (slot) slot[K * D + tid] = a;                                                                                      \
            else atomicAdd(hd.g_b + tid, a);                                                                                      \
        }                                                                                                                         \
        if (slot && tid < 2) slot[K * D + K + tid] = 0.f;                                                                         \
    }
