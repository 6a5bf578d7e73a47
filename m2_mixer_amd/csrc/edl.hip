// Classification heads + multi-head evidential (EDL) squared-error Bayes risk, forward and backward in one launch, and the
// uncertainty-based late fusion of the heads' predictions in a second, small one behind it.
//
// Reference: models/avmnist.py:447-572 (AVMnistMixerMultiLossUQ) with modules/losses.py:5-31 (EDLMSELoss).  Per head and sample,
// z = the head's K logits (a Linear on the token mean: heads_body.h), y = the one-hot label:
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
// Everything is fp32.  This file holds the loss phase; the phases around it -- pooled rows and weights into LDS, logits, the block's
// loss sum, d_pooled, g_w / g_b or the g_part slots that m2m_towers_wgrad_heads adds -- the grid and the argument checks are
// heads_body.h's and heads.hip's host side (host.h).
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
#include "heads_body.h"

struct EdlArgs {
    HeadArgs heads;
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
    HEADS_TILE(ha.heads)
    float* klr = ext;                                     // [S] KL terms (KL instantiations only: the others have no such array)

    HEADS_STAGE()
    __syncthreads();
    HEADS_LOGITS()
    __syncthreads();
    // ---- loss / prediction / uncertainty / dlogits: 32 lanes per sample, lane k holds logit k (K <= HEAD_MAXK = 32) ----
    if (tid < S * 32) {
        const int sI = tid >> 5, k = tid & 31;
        const bool live = k < K;
        const float z = live ? lg[sI * HEAD_MAXK + k] : 0.f;
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
        if (live) lg[sI * HEAD_MAXK + k] = dl;
        if (k == 0) {
            red[sI] = sI < ns ? term : 0.f;
            if (sI < ns) {
                preds[(long)hI * B + s0 + sI] = am;
                uncertainty[(long)hI * B + s0 + sI] = (float)K / st;
            }
        }
    }
    __syncthreads();
    if constexpr (KL) {
        const float lam = *ha.kl_coef;                        // (the loss phase's branch: klr was written where lam != 0)
        heads_loss_sum<S>(red, tid, hI, hw, B, losses, nheads, lam != 0.f ? klr : nullptr, lam, ha.kl_out);
    } else heads_loss_sum<S>(red, tid, hI, hw, B, losses, nheads);
    HEADS_BACKWARD()
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

template <int S, int RISK, bool KL>
static int launch_edl_s(const EdlArgs& ha, int nheads, const int64_t* labels, int B, int D, int K, float* logits, float* losses,
                        int32_t* preds, float* uncertainty, hipStream_t st) {
    return m2m_dispatch(m2m_wide_dims{}, D, M2M_NO_BUILD, [&](auto DD) {
        return m2m_launch<heads_edl_kernel<S, DD(), RISK, KL>>(dim3((B + S - 1) / S, nheads), dim3(NTHREADS), heads_lds_bytes(S, DD(), KL ? S : 0),
                                                               160 * 1024, st, ha, labels, B, K, logits, losses, preds, uncertainty, nheads);
    });
}

template <int RISK, bool KL>
static int launch_edl(const EdlArgs& ha, int nheads, const int64_t* labels, int B, int D, int K, float* logits, float* losses,
                      int32_t* preds, float* uncertainty, hipStream_t st) {
    return heads_samples_per_wg(B) == 4 ? launch_edl_s<4, RISK, KL>(ha, nheads, labels, B, D, K, logits, losses, preds, uncertainty, st)
                                        : launch_edl_s<HEAD_S, RISK, KL>(ha, nheads, labels, B, D, K, logits, losses, preds, uncertainty, st);
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
    if (int rc = m2m_check_heads("heads_edl", heads, nheads, labels, B, D, K, logits, losses, preds, false, M2M_SPLIT_GPART)) return rc;
    if (!uncertainty || !combined) {
        m2m_set_error("heads_edl: uncertainty and combined are required", __FILE__, __LINE__);
        return -1;
    }
    const EdlArgs ha{heads_args(heads, nheads, weights), kl_coef, kl_out, (float)lgamma((double)K)};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (zero_losses) m2m_heads_zero(losses, nheads + 1, kl_out, nheads, st);
    int rc;
    if (risk == M2M_EDL_MSE) {
        rc = kl_coef ? launch_edl<M2M_EDL_MSE, true>(ha, nheads, labels, B, D, K, logits, losses, preds, uncertainty, st)
                     : launch_edl<M2M_EDL_MSE, false>(ha, nheads, labels, B, D, K, logits, losses, preds, uncertainty, st);
    } else {
        rc = kl_coef ? launch_edl<M2M_EDL_CE, true>(ha, nheads, labels, B, D, K, logits, losses, preds, uncertainty, st)
                     : launch_edl<M2M_EDL_CE, false>(ha, nheads, labels, B, D, K, logits, losses, preds, uncertainty, st);
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
