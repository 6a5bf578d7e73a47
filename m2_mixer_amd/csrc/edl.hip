// Classification heads + multi-head evidential (EDL) squared-error Bayes risk, forward and backward in one launch, and the
// uncertainty-based late fusion of the heads' predictions in a second, small one behind it.
//
// Reference: models/avmnist.py:447-572 (AVMnistMixerMultiLossUQ) with modules/losses.py:5-31 (EDLMSELoss).  Per head and sample,
// z = the head's K logits (the same Linear on the token mean as heads.hip), y = the one-hot label:
//     e = relu(z), a = e + 1, S = sum_k a_k, p = a / S
//     L = sum_k [(y_k - p_k)^2 + p_k (1 - p_k) / (S + 1)]        loss_h = mean over the batch        (losses.py:24-31)
//     total = sum_h coef_h loss_h                                  (avmnist.py:511: coefficients 1, 1, 1, no x 3)
//     preds_h = argmax_k relu(z), first index on ties: all-negative logits give class 0             (avmnist.py:517-523)
//     u_h = K / S                                                                                   (avmnist.py:525-531)
//     combined = preds_h of the head whose u_h is strictly below every other head's, else 0         (avmnist.py:533-537)
// The reference multiplies its KL term by annealing_coef * 0 (losses.py:20): it adds nothing to the value or the gradient and the
// epoch number has no effect, so m2m_heads_edl leaves it out (m2m_heads_edl_risk, below, has it as an option).
// Gradient (closed form; sums over k):
//     dz_j = [z_j > 0] (dE_j + dV_j) coef_h / B
//     dE_j = (-2 / S) [(y_j - p_j) - sum_k (y_k - p_k) p_k]
//     dV_j = (-2 / (S (S + 1))) (p_j - sum_k p_k^2) - (1 - sum_k p_k^2) / (S + 1)^2
// with every 1 / (S (S + 1)) and 1 / (S + 1)^2 taken as two divisions (a very large S must not overflow a product).
// Everything is fp32.  The phases around the loss -- pooled rows and weights into LDS, logits, d_pooled, g_w / g_b or the g_part
// slots -- are those of heads.hip's cross-entropy kernel on the same grid (m2m_heads_part_tiles(B) sample tiles x heads), so the
// unchanged m2m_towers_wgrad_heads adds the slots.
//
// m2m_heads_edl_risk adds the two pieces of modules/losses.py the reference's UQ model does not train with -- the cross-entropy
// Bayes risk (EDLCELoss, modules/losses.py:71-93) and the Dirichlet KL regulariser (modules/losses.py:33-49 and :52-68, the same
// function twice) under an annealed coefficient lambda (:15-18, :81-84: min(1, epoch / annealing_step), times the caller's weight):
//     CE risk   L = psi(S) - psi(a_y)                          dL/dz_j = [z_j > 0] (psi1(S) - [j == y] psi1(a_j))       (:89-93)
//     KL        at_k = a_k (k != y), at_y = 1, St = sum_k at_k = S - a_y + 1                                            (:52-68)
//               KL = lgamma(St) - lgamma(K) - sum_k lgamma(at_k) + sum_k (at_k - 1)(psi(at_k) - psi(St))
//               dKL/dz_j = [z_j > 0][j != y] ((at_j - 1) psi1(at_j) - psi1(St)(St - K))
//     loss_h = mean_B(risk) + lambda mean_B(KL);  dlogits carries coef_h / B, and lambda on the KL part
// psi = digamma, psi1 = trigamma: fp32 device functions below, for arguments >= 1 only (a >= 1, S >= K, St >= K).  The risk and
// the presence of the KL term are template parameters: <MSE, no KL> is the kernel m2m_heads_edl always launched.  lambda is one
// device float (a captured graph follows it); lambda == 0 takes a workgroup-uniform branch round all KL arithmetic, so that form
// costs nothing, equals the no-KL result bit for bit, and an overflowing lgamma never meets a zero factor.
#include "dispatch.h"

#define EDL_S 16        // samples per workgroup (4 at B <= 64): the grid of heads.hip
#define EDL_MAXK 32
#define EDL_MAXH 4

struct EdlArgs {
    m2m_head h[EDL_MAXH];
    const float* weights;       // nheads device floats read in place of m2m_head.weight, or NULL
    const float* kl_coef;       // (KL instantiations) one device float: lambda
    float* kl_out;              // (KL instantiations) nheads floats += the unscaled batch-mean KL, or NULL
    float lgamma_k;             // lgamma(K), from the host
};

// ---- digamma, trigamma and lgamma for x >= 1: the recurrence up to x >= 6 (five steps at the most, taken without a branch), then
// ---- the asymptotic series, whose first dropped term is below 3e-9 of the value at x = 6 ------------------------------------------
// psi(x) = psi(x + 1) - 1 / x;  psi(x) ~ ln x - 1/(2x) - 1/(12 x^2) + 1/(120 x^4) - 1/(252 x^6) + 1/(240 x^8)
static __device__ __forceinline__ float edl_digamma(float x) {
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const bool low = x < 6.f;
        r -= low ? 1.f / x : 0.f;
        x += low ? 1.f : 0.f;
    }
    const float ix = 1.f / x, ix2 = ix * ix;
    const float series = ix2 * (1.f / 12.f - ix2 * (1.f / 120.f - ix2 * (1.f / 252.f - ix2 * (1.f / 240.f))));
    return r + (logf(x) - 0.5f * ix - series);
}

// psi1(x) = psi1(x + 1) + 1 / x^2;  psi1(x) ~ 1/x + 1/(2 x^2) + 1/(6 x^3) - 1/(30 x^5) + 1/(42 x^7) - 1/(30 x^9)
static __device__ __forceinline__ float edl_trigamma(float x) {
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const bool low = x < 6.f;
        const float ix = 1.f / x;
        r += low ? ix * ix : 0.f;
        x += low ? 1.f : 0.f;
    }
    const float ix = 1.f / x, ix2 = ix * ix;
    const float series = ix * (1.f + ix * (0.5f + ix * (1.f / 6.f - ix2 * (1.f / 30.f - ix2 * (1.f / 42.f - ix2 * (1.f / 30.f))))));
    return r + series;
}

// lgamma(x) = lgamma(x + n) - ln(x (x + 1) ... (x + n - 1))  (the product stays below 6^5);
// lgamma(x) ~ (x - 1/2) ln x - x + ln(2 pi) / 2 + 1/(12 x) - 1/(360 x^3) + 1/(1260 x^5)
static __device__ __forceinline__ float edl_lgamma(float x) {
    float prod = 1.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const bool low = x < 6.f;
        prod *= low ? x : 1.f;
        x += low ? 1.f : 0.f;
    }
    const float ix = 1.f / x, ix2 = ix * ix;
    const float series = ix * (1.f / 12.f - ix2 * (1.f / 360.f - ix2 * (1.f / 1260.f)));
    return ((x - 0.5f) * logf(x) - x + 0.91893853320467274f + series) - logf(prod);
}

template <int S, int DD, int RISK, bool KL>
__global__ __launch_bounds__(NTHREADS) void heads_edl_kernel(const EdlArgs ha, const int64_t* __restrict__ labels, int B, int K,
                                                             float* __restrict__ logits_out, float* __restrict__ losses,
                                                             int32_t* __restrict__ preds, float* __restrict__ uncertainty,
                                                             int nheads) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int D = DD, DL = DD + 4, D4 = DD / 4;
    float* pl = reinterpret_cast<float*>(smem);          // pooled tile [S][DL]
    float* wl = pl + S * DL;                              // weights     [EDL_MAXK][DL]
    float* lg = wl + EDL_MAXK * DL;                       // logits / dlogits [S][EDL_MAXK]
    float* red = lg + S * EDL_MAXK;                       // [S] loss terms
    float* klr = red + S;                                 // [S] KL terms (KL instantiations only: the others have no such array)

    const int tid = threadIdx.x;
    const int hI = blockIdx.y;
    const m2m_head& hd = ha.h[hI];
    const float hw = ha.weights ? ha.weights[hI] : hd.weight;      // this head's coefficient in the total loss
    const int s0 = blockIdx.x * S;
    const int ns = min(S, B - s0);

    // ---- pooled rows and head weights -> LDS (16-byte accesses; every global load requested before the first LDS write) ----
    {
        constexpr int NP = (S * D4 + NTHREADS - 1) / NTHREADS, NW = (EDL_MAXK * D4 + NTHREADS - 1) / NTHREADS;
        f32x4_t pv[NP], wv[NW];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int idx = tid + i * NTHREADS, sI = idx / D4, c = (idx % D4) * 4;
            pv[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            if (idx < S * D4 && sI < ns) {
                if (hd.tokens) {
                    // x.mean(dim=1): tokens in order, eight loads in flight, the 1 / N product (the bits of heads.hip's pooling)
                    const float* col = hd.tokens + (long)(s0 + sI) * hd.tok_sample_stride + c;
                    const int N = hd.ntok;
                    f32x4_t a = f32x4_t{0.f, 0.f, 0.f, 0.f};
                    for (int n0 = 0; n0 < N; n0 += 8) {
                        f32x4_t t8[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) t8[j] = *reinterpret_cast<const f32x4_t*>(col + (long)min(n0 + j, N - 1) * D);
#pragma unroll
                        for (int j = 0; j < 8; ++j)
                            if (n0 + j < N) a += t8[j];
                    }
                    pv[i] = a * (1.0f / (float)N);
                } else pv[i] = *reinterpret_cast<const f32x4_t*>(hd.pooled + (long)(s0 + sI) * D + c);
            }
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int idx = tid + i * NTHREADS;
            wv[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            if (idx < K * D4) wv[i] = *reinterpret_cast<const f32x4_t*>(hd.w + (long)idx * 4);
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int idx = tid + i * NTHREADS;
            if (idx < S * D4) *reinterpret_cast<f32x4_t*>(pl + (idx / D4) * DL + (idx % D4) * 4) = pv[i];      // rows >= ns: zeros
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int idx = tid + i * NTHREADS;
            if (idx < EDL_MAXK * D4) *reinterpret_cast<f32x4_t*>(wl + (idx / D4) * DL + (idx % D4) * 4) = wv[i];     // rows >= K: zeros
        }
    }
    __syncthreads();
    // ---- logits: 4 adjacent lanes split each D-long dot product, float4 chunks interleaved over the lanes ----
    for (int idx = tid >> 2; idx < S * K; idx += NTHREADS / 4) {
        const int sI = idx / K, k = idx % K, part = tid & 3;
        constexpr int NC = D4 / 4;                        // float4 chunks per lane
        f32x4_t a4[NC], b4[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            a4[c] = *reinterpret_cast<const f32x4_t*>(pl + sI * DL + 4 * (part + 4 * c));
            b4[c] = *reinterpret_cast<const f32x4_t*>(wl + k * DL + 4 * (part + 4 * c));
        }
        float a = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) a = __builtin_fmaf(a4[c][e], b4[c][e], a);
        a = wave_sum_xor(a, 4) + hd.b[k];
        if (part == 0) {
            lg[sI * EDL_MAXK + k] = a;
            if (sI < ns) logits_out[((long)hI * B + s0 + sI) * K + k] = a;
        }
    }
    __syncthreads();
    // ---- loss / prediction / uncertainty / dlogits: 32 lanes per sample, lane k holds logit k (K <= EDL_MAXK = 32) ----
    if (tid < S * 32) {
        const int sI = tid >> 5, k = tid & 31;
        const bool live = k < K;
        const float z = live ? lg[sI * EDL_MAXK + k] : 0.f;
        const float ev = __builtin_fmaxf(z, 0.f);             // evidence
        const float al = live ? ev + 1.f : 0.f;               // alpha (dead lanes add nothing to the sums)
        float mx = live ? ev : -1.f;                          // argmax of the evidence, first index of the maximum
        int am = live ? k : 0x7fffffff;
        float st = al;                                        // S: the Dirichlet strength
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(mx, o, 64);
            const int oa = __shfl_xor(am, o, 64);
            if (ov > mx || (ov == mx && oa < am)) { mx = ov; am = oa; }
            st += __shfl_xor(st, o, 64);
        }
        const int y = sI < ns ? (int)labels[s0 + sI] : 0;
        float term, dl;
        if constexpr (RISK == M2M_EDL_MSE) {
            const float p = al / st;
            const float d = live ? (k == y ? 1.f : 0.f) - p : 0.f;
            const float s1 = st + 1.f;
            term = d * d + p * (1.f - p) / s1;                // dead lanes: p = d = 0
            float sdp = d * p, sp2 = p * p;
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) {
                term += __shfl_xor(term, o, 64);
                sdp += __shfl_xor(sdp, o, 64);
                sp2 += __shfl_xor(sp2, o, 64);
            }
            const float dE = (-2.f / st) * (d - sdp);
            const float dV = ((-2.f / st) / s1) * (p - sp2) - ((1.f - sp2) / s1) / s1;
            dl = (sI < ns && z > 0.f) ? (hw / (float)B) * (dE + dV) : 0.f;
        } else {
            // lane k evaluates its own class: psi(a_k) is read on the label's lane only, psi1(S) is the same on all 32
            const bool hit = live && k == y;
            const float ak = live ? al : 1.f;
            term = hit ? edl_digamma(st) - edl_digamma(ak) : 0.f;
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) term += __shfl_xor(term, o, 64);
            const float g = edl_trigamma(st) - (hit ? edl_trigamma(ak) : 0.f);
            dl = (sI < ns && z > 0.f) ? (hw / (float)B) * g : 0.f;
        }
        if constexpr (KL) {
            const float lam = *ha.kl_coef;                    // one uniform load; the branch is the same for the whole grid
            if (lam != 0.f) {
                const bool other = live && k != y;            // the label's lane has at = 1: lgamma(1) = 0, at - 1 = 0
                const float at = other ? al : 1.f;
                float stt = live ? at : 0.f;                  // St = sum_k at_k
#pragma unroll
                for (int o = 16; o >= 1; o >>= 1) stt += __shfl_xor(stt, o, 64);
                const float psit = edl_digamma(stt);
                float kl = other ? (at - 1.f) * (edl_digamma(at) - psit) - edl_lgamma(at) : 0.f;
#pragma unroll
                for (int o = 16; o >= 1; o >>= 1) kl += __shfl_xor(kl, o, 64);
                kl += edl_lgamma(stt) - ha.lgamma_k;
                const float gk = (at - 1.f) * edl_trigamma(at) - edl_trigamma(stt) * (stt - (float)K);
                if (sI < ns && z > 0.f && other) dl += (hw / (float)B) * (lam * gk);
                if (k == 0) klr[sI] = sI < ns ? kl : 0.f;
            }
        }
        if (live) lg[sI * EDL_MAXK + k] = dl;
        if (k == 0) {
            red[sI] = sI < ns ? term : 0.f;
            if (sI < ns) {
                preds[(long)hI * B + s0 + sI] = am;
                uncertainty[(long)hI * B + s0 + sI] = (float)K / st;
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
#pragma unroll
        for (int sI = 0; sI < S; ++sI) t += red[sI];
        t /= (float)B;
        if constexpr (KL) {
            const float lam = *ha.kl_coef;
            if (lam != 0.f) {                                 // (the loss phase's branch: klr was written)
                float tk = 0.f;
#pragma unroll
                for (int sI = 0; sI < S; ++sI) tk += klr[sI];
                tk /= (float)B;
                t += lam * tk;
                if (ha.kl_out) atomicAdd(ha.kl_out + hI, tk);
            }
        }
        atomicAdd(losses + hI, t);
        atomicAdd(losses + nheads, t * hw);
    }
    if (hd.d_pooled) {
        // d_pooled[s][d..d+3] = sum_k dl[s][k] w[k][d..d+3]: thread = (sample, float4 of d)
        for (int idx = tid; idx < ns * D4; idx += NTHREADS) {
            const int sI = idx / D4, c = (idx % D4) * 4;
            f32x4_t a = f32x4_t{0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < K; ++k) {
                const f32x4_t w4 = *reinterpret_cast<const f32x4_t*>(wl + k * DL + c);
                const float dk = lg[sI * EDL_MAXK + k];
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] = __builtin_fmaf(dk, w4[e], a[e]);
            }
            *reinterpret_cast<f32x4_t*>(hd.d_pooled + (long)(s0 + sI) * D + c) = a;
        }
        // g_part: this workgroup's sums go to its slot (plain stores; m2m_towers_wgrad_heads adds the slots in a fixed order)
        // g_w[k][d..d+3] = sum_s dl[s][k] pooled[s][d..d+3]: thread = (class, float4 of d), the sample loop unrolled
        float* slot = hd.g_part ? hd.g_part + (long)blockIdx.x * M2M_SPLIT_GPART : nullptr;
        for (int idx = tid; idx < K * D4; idx += NTHREADS) {
            const int k = idx / D4, c = (idx % D4) * 4;
            f32x4_t a = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int sI = 0; sI < S; ++sI) {
                const f32x4_t p4 = *reinterpret_cast<const f32x4_t*>(pl + sI * DL + c);
                const float d1 = lg[sI * EDL_MAXK + k];       // samples >= ns: 0
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] = __builtin_fmaf(d1, p4[e], a[e]);
            }
            if (slot) *reinterpret_cast<f32x4_t*>(slot + (long)k * D + c) = a;
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) atomicAdd(hd.g_w + (long)k * D + c + e, a[e]);
            }
        }
        if (tid < K) {
            float a = 0.f;
#pragma unroll
            for (int sI = 0; sI < S; ++sI) a += lg[sI * EDL_MAXK + tid];
            if (slot) slot[K * D + tid] = a;
            else atomicAdd(hd.g_b + tid, a);
        }
        if (slot && tid < 2) slot[K * D + K + tid] = 0.f;           // (the slot layout's loss entries: the losses stay atomics)
    }
}

// The late fusion of avmnist.py:533-537, one thread per sample: the prediction of the head whose uncertainty is strictly below
// every other head's; no such head (a tie for the minimum; all heads without evidence, u == 1 everywhere): 0.  A thread reads its
// sample's per-head values before it writes, so `combined` may alias a row of `preds`.
__global__ void edl_combine_kernel(const int32_t* preds, const float* __restrict__ uncertainty, int32_t* combined, int B, int nheads) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    float best = uncertainty[i];
    int pick = preds[i];
    bool strict = true;
    for (int h = 1; h < nheads; ++h) {
        const float u = uncertainty[(long)h * B + i];
        const int p = preds[(long)h * B + i];
        if (u < best) { best = u; pick = p; strict = true; }
        else if (u == best) strict = false;
    }
    combined[i] = strict ? pick : 0;
}

// (the losses are cleared by a kernel, as in heads.hip: a small memset node misbehaved on hipGraph replay)
__global__ void edl_zero_floats_kernel(float* p, int n, float* q, int nq) {
    if ((int)threadIdx.x < n) p[threadIdx.x] = 0.f;
    if ((int)threadIdx.x < nq) q[threadIdx.x] = 0.f;         // (kl_out, cleared together with the losses)
}

template <int S, int RISK, bool KL>
static int launch_edl_s(const EdlArgs& ha, int nheads, const int64_t* labels, int B, int D, int K, float* logits, float* losses,
                        int32_t* preds, float* uncertainty, hipStream_t st) {
    return m2m_dispatch(m2m_wide_dims{}, D, M2M_NO_BUILD, [&](auto DD) {
        constexpr int Dc = decltype(DD)::value;
        const size_t lds = sizeof(float) * ((size_t)S * (Dc + 4) + (size_t)EDL_MAXK * (Dc + 4) + S * EDL_MAXK + S + (KL ? S : 0));
        return m2m_launch<heads_edl_kernel<S, Dc, RISK, KL>>(dim3((B + S - 1) / S, nheads), dim3(NTHREADS), lds, 160 * 1024, st, ha, labels,
                                                             B, K, logits, losses, preds, uncertainty, nheads);
    });
}

template <int RISK, bool KL>
static int launch_edl(int S, const EdlArgs& ha, int nheads, const int64_t* labels, int B, int D, int K, float* logits, float* losses,
                      int32_t* preds, float* uncertainty, hipStream_t st) {
    return S == 4 ? launch_edl_s<4, RISK, KL>(ha, nheads, labels, B, D, K, logits, losses, preds, uncertainty, st)
                  : launch_edl_s<EDL_S, RISK, KL>(ha, nheads, labels, B, D, K, logits, losses, preds, uncertainty, st);
}

extern "C" int m2m_heads_edl_risk(const m2m_head* heads, int nheads, const int64_t* labels, int B, int D, int K, float* logits,
                                  float* losses, int32_t* preds, float* uncertainty, int32_t* combined, int zero_losses,
                                  const float* weights, int risk, const float* kl_coef, float* kl_out, void* stream) {
    if (risk != M2M_EDL_MSE && risk != M2M_EDL_CE) {
        m2m_set_error("heads_edl: risk must be M2M_EDL_MSE (0) or M2M_EDL_CE (1)", __FILE__, __LINE__);
        return -1;
    }
    if (kl_out && !kl_coef) {
        m2m_set_error("heads_edl: kl_out needs kl_coef (without the KL term there is nothing to report)", __FILE__, __LINE__);
        return -1;
    }
    if (!heads || nheads < 1 || nheads > EDL_MAXH || K < 2 || K > EDL_MAXK || B < 1) {
        m2m_set_error("heads_edl: unsupported (1..4 heads, K in 2..32, B >= 1)", __FILE__, __LINE__);
        return -1;
    }
    if (D != 32 && D != 64 && D != 128 && D != 256) {      // before anything is launched (the losses' zero fill below)
        m2m_set_error("heads_edl: hidden_dim must be 32, 64, 128 or 256", __FILE__, __LINE__);
        return -1;
    }
    if (!labels || !logits || !losses || !preds || !uncertainty || !combined) {
        m2m_set_error("heads_edl: labels, logits, losses, preds, uncertainty and combined are required", __FILE__, __LINE__);
        return -1;
    }
    const int S = B <= 64 ? 4 : EDL_S;
    if ((B + S - 1) / S != m2m_heads_part_tiles(B)) {      // the slot count m2m_towers_wgrad_heads adds
        m2m_set_error("heads_edl: its sample tiles are not those of m2m_heads_part_tiles", __FILE__, __LINE__);
        return -1;
    }
    EdlArgs ha;
    for (int i = 0; i < nheads; ++i) {
        if (heads[i].tokens ? (heads[i].ntok < 1 || heads[i].tok_sample_stride < (int64_t)heads[i].ntok * D || (heads[i].tok_sample_stride & 3) ||
                               (reinterpret_cast<uintptr_t>(heads[i].tokens) & 15))
                            : !heads[i].pooled) {
            m2m_set_error("heads_edl: a head needs pooled, or 16-byte aligned tokens with ntok >= 1 and a sample stride >= ntok * D (multiple of 4)", __FILE__, __LINE__);
            return -1;
        }
        if (!heads[i].w || !heads[i].b || (heads[i].d_pooled && !heads[i].g_part && (!heads[i].g_w || !heads[i].g_b))) {
            m2m_set_error("heads_edl: a head needs w and b, and with d_pooled either g_part or g_w and g_b", __FILE__, __LINE__);
            return -1;
        }
        if (heads[i].g_part && (long)K * D + K + 2 > M2M_SPLIT_GPART) {
            m2m_set_error("heads_edl: g_part needs K*D + K + 2 <= M2M_SPLIT_GPART", __FILE__, __LINE__);
            return -1;
        }
    }
    ha.weights = weights;
    ha.kl_coef = kl_coef;
    ha.kl_out = kl_out;
    ha.lgamma_k = (float)lgamma((double)K);
    for (int i = 0; i < nheads; ++i) ha.h[i] = heads[i];
    for (int i = nheads; i < EDL_MAXH; ++i) ha.h[i] = heads[0];
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (zero_losses) hipLaunchKernelGGL(edl_zero_floats_kernel, dim3(1), dim3(64), 0, st, losses, nheads + 1, kl_out, kl_out ? nheads : 0);
    int rc;
    if (risk == M2M_EDL_MSE) {
        rc = kl_coef ? launch_edl<M2M_EDL_MSE, true>(S, ha, nheads, labels, B, D, K, logits, losses, preds, uncertainty, st)
                     : launch_edl<M2M_EDL_MSE, false>(S, ha, nheads, labels, B, D, K, logits, losses, preds, uncertainty, st);
    } else {
        rc = kl_coef ? launch_edl<M2M_EDL_CE, true>(S, ha, nheads, labels, B, D, K, logits, losses, preds, uncertainty, st)
                     : launch_edl<M2M_EDL_CE, false>(S, ha, nheads, labels, B, D, K, logits, losses, preds, uncertainty, st);
    }
    if (rc != 0) return rc;
    hipLaunchKernelGGL(edl_combine_kernel, dim3((B + 255) / 256), dim3(256), 0, st, preds, uncertainty, combined, B, nheads);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int m2m_heads_edl(const m2m_head* heads, int nheads, const int64_t* labels, int B, int D, int K, float* logits,
                             float* losses, int32_t* preds, float* uncertainty, int32_t* combined, int zero_losses,
                             const float* weights, void* stream) {
    return m2m_heads_edl_risk(heads, nheads, labels, B, D, K, logits, losses, preds, uncertainty, combined, zero_losses, weights,
                              M2M_EDL_MSE, nullptr, nullptr, stream);
}
