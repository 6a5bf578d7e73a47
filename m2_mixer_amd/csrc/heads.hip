// Classification heads + multi-head cross-entropy, forward and backward in one launch.
//
// Reference: models/avmnist.py:271-298 -- classifier_image/audio = nn.Linear on tokens.mean(dim=1),
// classifier_fusion = StandardClassifier (mean over tokens -> Linear, modules/classification.py:89-90),
// three nn.CrossEntropyLoss() (mean), loss = (w Lf + ow Li + ow La) * 3, preds = softmax(.).argmax(1).
// The token means ("pooled") are produced by the tower forward kernel and consumed here -- or, for towers whose forward does not
// own whole samples (the wide path), computed here from the tower output (m2m_head.tokens).
// BCE = true is the MM-IMDb variant (models/mmimdb.py:47-50, :115-133): nn.BCEWithLogitsLoss(pos_weight) with mean
// reduction over all B*K elements per head, preds = sigmoid(logits) > 0.5 per label.
// This file holds the two loss phases, and the host side of every heads launch (host.h: the samples per workgroup, the argument
// check, the losses' zero fill), which edl.hip uses as well; the kernel body round the loss phase is heads_body.h.
#include "heads_body.h"

// The loss phases: cross-entropy, the softmax on 32 lanes per sample (cross-lane max / sum); BCE, one thread per (sample, label)
// element, whose loss terms go through `ext` ([S][HEAD_MAXK]).  Summation orders -- logits: four interleaved partial sums of
// float4 chunks; loss terms per workgroup in sample order: parity with the oracle is that of fp32, ~1e-7.
template <bool BCE, int S, int DD>
__global__ __launch_bounds__(NTHREADS) void heads_kernel(const HeadArgs ha, const void* __restrict__ labels_v,
                                                         const float* __restrict__ pos_weight, int B, int D_rt,
                                                         int K, float* __restrict__ logits_out, float* __restrict__ losses,
                                                         int32_t* __restrict__ preds, int nheads) {
    const int64_t* labels = reinterpret_cast<const int64_t*>(labels_v);       // CE: class index (B)
    const float* targets = reinterpret_cast<const float*>(labels_v);          // BCE: multi-hot (B, K)
    HEADS_TILE(ha)
    float* tm = ext;                                      // [S][HEAD_MAXK] per-element loss terms (BCE)

    HEADS_STAGE()
    __syncthreads();
    HEADS_LOGITS()
    __syncthreads();
    // ---- loss / prediction / dlogits ----
    if (BCE) {
        // every (sample, label) element is independent -- one thread each
        const float scale = hw / ((float)B * (float)K);
        for (int idx = tid; idx < S * K; idx += NTHREADS) {
            const int sI = idx / K, k = idx % K;
            float term = 0.f, dl = 0.f;
            if (sI < ns) {
                const float x = lg[sI * HEAD_MAXK + k], y = targets[(long)(s0 + sI) * K + k], pw = pos_weight[k];
                // log sigmoid(x) = min(x, 0) - log1p(exp(-|x|));  log(1 - sigmoid(x)) = log sigmoid(x) - x
                const float ls = __builtin_fminf(x, 0.f) - log1pf(__expf(-__builtin_fabsf(x)));
                term = -(pw * y * ls + (1.f - y) * (ls - x));
                const float sg = 1.0f / (1.0f + __expf(-x));
                dl = scale * ((1.f - y) * sg - pw * y * (1.f - sg));
                preds[((long)hI * B + s0 + sI) * K + k] = x > 0.f ? 1 : 0;
            }
            lg[sI * HEAD_MAXK + k] = dl;
            tm[sI * HEAD_MAXK + k] = term;
        }
        __syncthreads();
        if (tid < S) {
            float term = 0.f;
            for (int k = 0; k < K; ++k) term += tm[tid * HEAD_MAXK + k];      // label order, as the single-thread loop summed
            red[tid] = term / (float)K;
        }
    } else if (tid < S * 32) {
        // cross-entropy: 32 lanes per sample, lane k holds logit k (K <= HEAD_MAXK = 32); max / argmax / sum across the lanes.
        // (first index of the maximum, like torch.argmax on distinct values; the sums run over a butterfly instead of k = 0..K-1:
        // last-bit differences in a printed loss, none in the predictions)
        const int sI = tid >> 5, k = tid & 31;
        const bool live = k < K;
        const float v = live ? lg[sI * HEAD_MAXK + k] : -3.0e38f;
        float mx = v;
        int am = live ? k : 0x7fffffff;
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(mx, o, 64);
            const int oa = __shfl_xor(am, o, 64);
            if (ov > mx || (ov == mx && oa < am)) { mx = ov; am = oa; }
        }
        const float ex = live ? __expf(v - mx) : 0.f;
        float se = ex;
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) se += __shfl_xor(se, o, 64);
        const int y = sI < ns ? (int)labels[s0 + sI] : 0;
        const float scale = hw / (float)B;
        const float dl = sI < ns ? scale * (ex * (1.0f / se) - (k == y ? 1.f : 0.f)) : 0.f;
        const float vy = __shfl(v, (tid & 32) + y, 64);       // the label's logit (lane y of this sample's 32 lanes)
        if (live) lg[sI * HEAD_MAXK + k] = dl;
        if (k == 0) {
            red[sI] = sI < ns ? (__logf(se) + mx) - vy : 0.f;
            if (sI < ns) preds[(long)hI * B + s0 + sI] = am;
        }
    }
    __syncthreads();
    heads_loss_sum<S>(red, tid, hI, hw, B, losses, nheads);
    HEADS_BACKWARD()
}


// ---- the host side the three losses share (host.h) -----------------------------------------------------------------------------
int heads_samples_per_wg(int B) { return B <= 64 ? 4 : HEAD_S; }

extern "C" int m2m_heads_part_tiles(int B) { const int S = heads_samples_per_wg(B); return B < 1 ? 0 : (B + S - 1) / S; }

// losses are accumulated with atomics; they are cleared by a kernel (not a memset node: a 16-byte
// hipMemsetAsync node was observed to write stale bytes on hipGraph replay).
__global__ void zero_floats_kernel(float* p, int n, float* q, int nq) {
    if ((int)threadIdx.x < n) p[threadIdx.x] = 0.f;
    if ((int)threadIdx.x < nq) q[threadIdx.x] = 0.f;
}
void m2m_heads_zero(float* losses, int n, float* kl_out, int nkl, hipStream_t st) {
    hipLaunchKernelGGL(zero_floats_kernel, dim3(1), dim3(64), 0, st, losses, n, kl_out, kl_out ? nkl : 0);
}

static int heads_error(const char* call, const char* what) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", call, what);
    m2m_set_error(msg, __FILE__, __LINE__);
    return -1;
}
int m2m_check_heads(const char* call, const m2m_head* heads, int nheads, const void* labels, int B, int D, int K, const float* logits,
                    const float* losses, const int32_t* preds, bool bce, long slot_floats) {
    if (!heads || nheads < 1 || nheads > HEAD_MAXH || K < 2 || K > HEAD_MAXK || B < 1) return heads_error(call, "unsupported (1..4 heads, K in 2..32, B >= 1)");
    if (D != 32 && D != 64 && D != 128 && D != 256) return heads_error(call, "hidden_dim must be 32, 64, 128 or 256");
    if (!labels || !logits || !losses || !preds) return heads_error(call, "labels (targets), logits, losses and preds are required");
    for (int i = 0; i < nheads; ++i) {
        const m2m_head& h = heads[i];
        if (h.tokens ? (h.ntok < 1 || h.tok_sample_stride < (int64_t)h.ntok * D || (h.tok_sample_stride & 3) || (reinterpret_cast<uintptr_t>(h.tokens) & 15))
                     : !h.pooled)
            return heads_error(call, "a head needs pooled, or 16-byte aligned tokens with ntok >= 1 and a sample stride >= ntok * D (multiple of 4)");
        if (!h.w || !h.b || (h.d_pooled && !h.g_part && (!h.g_w || !h.g_b))) return heads_error(call, "a head needs w and b, and with d_pooled either g_part or g_w and g_b");
        if (h.g_part && (bce || (long)K * D + K + 2 > slot_floats)) return heads_error(call, "g_part needs cross-entropy or evidential heads with K*D + K + 2 <= M2M_SPLIT_GPART");
    }
    return 0;
}

// ---- cross-entropy and BCE -------------------------------------------------------------------------------------------------------
template <bool BCE, int S>
static int launch_heads_s(const HeadArgs& ha, int nheads, const void* labels, const float* pos_weight, int B, int D, int K,
                          float* logits, float* losses, int32_t* preds, hipStream_t st) {
    return m2m_dispatch(m2m_wide_dims{}, D, M2M_NO_BUILD, [&](auto DD) {
        return m2m_launch<heads_kernel<BCE, S, DD()>>(dim3((B + S - 1) / S, nheads), dim3(NTHREADS), heads_lds_bytes(S, DD(), S * HEAD_MAXK), 160 * 1024, st,
                                                      ha, labels, pos_weight, B, (int)DD(), K, logits, losses, preds, nheads);
    });
}

template <bool BCE>
static int launch_heads(const char* call, const m2m_head* heads, int nheads, const void* labels, const float* pos_weight, int B, int D,
                        int K, float* logits, float* losses, int32_t* preds, int zero_losses, const float* weights, void* stream) {
    if (BCE && !pos_weight) { m2m_set_error("heads_bce: targets and pos_weight are required", __FILE__, __LINE__); return -1; }
    if (int rc = m2m_check_heads(call, heads, nheads, labels, B, D, K, logits, losses, preds, BCE, M2M_SPLIT_GPART)) return rc;
    const HeadArgs ha = heads_args(heads, nheads, weights);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (zero_losses) m2m_heads_zero(losses, nheads + 1, nullptr, 0, st);
    if (heads_samples_per_wg(B) == 4) return launch_heads_s<BCE, 4>(ha, nheads, labels, pos_weight, B, D, K, logits, losses, preds, st);
    return launch_heads_s<BCE, HEAD_S>(ha, nheads, labels, pos_weight, B, D, K, logits, losses, preds, st);
}

extern "C" int m2m_heads_ce(const m2m_head* heads, int nheads, const int64_t* labels, int B, int D, int K, float* logits,
                            float* losses, int32_t* preds, int zero_losses, void* stream) {
    return launch_heads<false>("heads_ce", heads, nheads, labels, nullptr, B, D, K, logits, losses, preds, zero_losses, nullptr, stream);
}

extern "C" int m2m_heads_bce(const m2m_head* heads, int nheads, const float* targets, const float* pos_weight, int B, int D, int K,
                             float* logits, float* losses, int32_t* preds, int zero_losses, void* stream) {
    return launch_heads<true>("heads_bce", heads, nheads, targets, pos_weight, B, D, K, logits, losses, preds, zero_losses, nullptr, stream);
}

// ABI 18: the same two launches with the heads' loss coefficients read from device memory (weights: nheads floats, or NULL)
extern "C" int m2m_heads_ce_w(const m2m_head* heads, int nheads, const int64_t* labels, int B, int D, int K, float* logits,
                              float* losses, int32_t* preds, int zero_losses, const float* weights, void* stream) {
    return launch_heads<false>("heads_ce", heads, nheads, labels, nullptr, B, D, K, logits, losses, preds, zero_losses, weights, stream);
}

extern "C" int m2m_heads_bce_w(const m2m_head* heads, int nheads, const float* targets, const float* pos_weight, int B, int D,
                               int K, float* logits, float* losses, int32_t* preds, int zero_losses, const float* weights,
                               void* stream) {
    return launch_heads<true>("heads_bce", heads, nheads, targets, pos_weight, B, D, K, logits, losses, preds, zero_losses, weights, stream);
}
