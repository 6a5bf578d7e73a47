// Every host function and predicate of libm2mixer that crosses a translation unit, declared ONCE and grouped by the file that
// defines it.  Every .hip that defines or calls one of them includes this header, so each definition is compiled against its
// declaration.  The public extern "C" entry points are declared by include/m2mixer.h alone (tile.h brings it in).
#pragma once
#include "split.h"   // the argument structs of the split path; brings tile.h, common.h and include/m2mixer.h

// ---- api.hip -------------------------------------------------------------------------------------------------------------------
// the calling thread's last error message (m2m_last_error)
void m2m_set_error(const char* msg, const char* file, int line);
// 0, or -1 with the error set: descriptor fields the kernels are built for (precision, hidden_dim, N, T, blocks, buffers at batch B)
int m2m_check_tower(const m2m_tower* t, int B);
// 0, or -1 with the error set ("<call>: <argument> ..."): the caller's buffers of a forward (f) and / or backward (g) call of tower t,
// before the call chooses a path -- x0, out and d_x0 given; every buffer (pooled, d_out and d_pooled where given) 16-byte aligned;
// sample strides (d_out's where d_out is given) at least N * D and, as x0_part_stride with x0_parts > 1, multiples of 4 floats
int m2m_check_tower_io(const char* call, const m2m_tower* t, const m2m_tower_io* f, const m2m_tower_gio* g);

// (grid and packed-image sizes in api.hip, pack.hip, adam.hip and probes.hip)
static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- pack.hip, adam.hip, probes.hip: public entry points only (include/m2mixer.h); the packed slot they share: pack.h ----------

// ---- scores.hip, rank.hip: public entry points only (include/m2mixer.h); they use m2m_set_error and ceil_div above -------------

// ---- embed.hip -----------------------------------------------------------------------------------------------------------------
int m2m_check_embed(const m2m_embed* e, int B);

// ---- heads.hip: the host side that the cross-entropy, BCE and evidential (edl.hip) heads share ---------------------------------
// Samples per workgroup of every heads launch at batch B: its grid, and the slot count of m2m_heads_part_tiles.
int heads_samples_per_wg(int B);
// 0, or -1 with the error set ("<call>: ..."), before anything is launched: 1..4 heads, K in 2..32, B >= 1, a hidden_dim that is
// built; labels (BCE: targets), logits, losses and preds given; per head pooled or well-formed tokens, w and b, and with d_pooled
// either g_part or both of g_w and g_b.  g_part is refused for `bce` heads and where K*D + K + 2 exceeds slot_floats.
int m2m_check_heads(const char* call, const m2m_head* heads, int nheads, const void* labels, int B, int D, int K, const float* logits,
                    const float* losses, const int32_t* preds, bool bce, long slot_floats);
// One launch that clears losses[0..n) and, where kl_out is given, kl_out[0..nkl).
void m2m_heads_zero(float* losses, int n, float* kl_out, int nkl, hipStream_t st);

// ---- tower_fwd.hip -------------------------------------------------------------------------------------------------------------
// True when two towers can share one chain launch: both on the fused path, same kernel instantiation, <= 4 blocks each.
bool m2m_can_group(const m2m_tower* a, const m2m_tower* b);
// Channel-mixing half of ONE block (+ final LayerNorm if the view has it) over B*N independent rows: the wide path's
// per-block launch.  `view` is a one-block copy of the tower (token parameters unused).
int m2m_chain_forward_rows(const m2m_tower* t, const float* x0, long x0_ss, int B, float* out, long out_ss, int training,
                           unsigned int seed, unsigned int step, const unsigned int* step_dev, hipStream_t st);
// Channel-mixing halves (wide path) of two towers' blocks in one launch: v[i] = block views (token_wide.hip: m2m_forward_wide_group).
int m2m_chain_forward_rows_group(const m2m_tower* const* v, const float* const* x0, const long* x0_ss, int B, float* const* out,
                                 const long* out_ss, int training, unsigned int seed, unsigned int step, const unsigned int* step_dev,
                                 hipStream_t st);

// ---- tower_bwd.hip -------------------------------------------------------------------------------------------------------------
// Fills `x` for the slot reduction of tower t's fused single-tower backward launch at batch B; returns false if that launch does
// not use slots.  (The caller reduces: immediately, or inside the next weight-gradient launch when the tower's wgrad_flags carry
// M2M_WGRAD_REDUCES_SMALL.)
bool m2m_small_part_deferred(SplitReduceTower& x, const m2m_tower* t, int B);
// Backward of the channel-mixing half of ONE block (+ final LayerNorm if the view has it) over B*N independent rows.
int m2m_chain_backward_rows(const m2m_tower* t, int B, const float* d_out, long d_out_ss, const float* d_pooled, float* d_x0,
                            long d_x0_ss, unsigned int seed, unsigned int step, const unsigned int* step_dev, hipStream_t st);
// Channel-mixing halves (wide path) of two towers' blocks in one launch (token_wide.hip: m2m_backward_wide_group).
int m2m_chain_backward_rows_group(const m2m_tower* const* v, int B, const float* const* d_out, const long* d_out_ss,
                                  const float* const* d_pooled, float* const* d_x0, const long* d_x0_ss, unsigned int seed,
                                  unsigned int step, const unsigned int* step_dev, hipStream_t st);

// ---- tower_wgrad.hip -----------------------------------------------------------------------------------------------------------
// Form of the channel-mixing weight gradients of a tower at batch B.  true: the weight-gradient launch recomputes the hidden
// activation from the packed image of A = LN2(x_mid) that the backward chain leaves in m2m_block.h_chn (tower_bwd_body<HREC>),
// and only dHpre^T is streamed; false: both hidden operands are stored and streamed.
bool m2m_wgrad_recompute(const m2m_tower* t, int B);

// ---- token_wide.hip: the wide path (N > 8 or D > 128) ----------------------------------------------------------------------------
// Two wide towers per launch: same precision, hidden_dim 256, dropout, token_dim class and block count (<= 4), small launches.
bool m2m_can_group_wide(const m2m_tower* a, const m2m_tower* b, int B);
int m2m_forward_wide(const m2m_tower* t, const float* x0, long x0_ss, int B, float* out, long out_ss, float* pooled,
                     int training, unsigned int seed, unsigned int step, const unsigned int* step_dev, hipStream_t st);
int m2m_backward_wide(const m2m_tower* t, int B, const float* d_out, long d_out_ss, const float* d_pooled, float* d_x0,
                      long d_x0_ss, unsigned int seed, unsigned int step, const unsigned int* step_dev, hipStream_t st);
int m2m_forward_wide_group(const m2m_tower* const* tw, const m2m_tower_io* io, int B, int training, unsigned int seed,
                           unsigned int step, const unsigned int* step_dev, hipStream_t st);
int m2m_backward_wide_group(const m2m_tower* const* tw, const m2m_tower_gio* io, int B, unsigned int seed, unsigned int step,
                            const unsigned int* step_dev, hipStream_t st);

// ---- split_api.hip: the column-split path (split.h) ------------------------------------------------------------------------------
// Whether tower t takes the split path at batch B (its backward then stores both hidden operands and does not write the d_x0^T
// image); M2M_SPLIT / M2M_SPLIT_MIN_ROWS.
bool m2m_split_eligible(const m2m_tower* t, int B, int training);
// Towers that can share the launches of the split path: same instantiation of the mix kernels and the same split count.
bool m2m_split_can_group(const m2m_tower* a, const m2m_tower* b);
int m2m_split_forward(const m2m_tower* const* towers, const m2m_tower_io* io, int ntow, int B, int training, unsigned int seed,
                      unsigned int step, const unsigned int* step_dev, hipStream_t st);
int m2m_split_backward(const m2m_tower* const* towers, const m2m_tower_gio* io, int ntow, int B, unsigned int seed, unsigned int step,
                       const unsigned int* step_dev, hipStream_t st);

// ---- split_mix.hip ---------------------------------------------------------------------------------------------------------------
int m2m_split_mix_forward(const SplitMixArgs& a, int D, int training, float p_drop, unsigned int seed, unsigned int step,
                          const unsigned int* step_dev, hipStream_t st);
int m2m_split_mix_backward(const SplitMixBwdArgs& a, int D, float p_drop, unsigned int seed, unsigned int step,
                           const unsigned int* step_dev, hipStream_t st);
// sum of the per-workgroup slots into the gradients
int m2m_split_small_grads(const SplitReduceArgs& a, hipStream_t st);

// ---- split_chain.hip -------------------------------------------------------------------------------------------------------------
int m2m_split_chain_forward(const SplitChainArgs& a, int D, int training, float p_drop, unsigned int seed, unsigned int step,
                            const unsigned int* step_dev, hipStream_t st);
int m2m_split_chain_backward(const SplitChainArgs& a, int D, float p_drop, unsigned int seed, unsigned int step,
                             const unsigned int* step_dev, hipStream_t st);
