// Library plumbing: the thread-local error, the ABI version, packed sizes, the tower descriptor check and the step-head launches.
#include "dispatch.h"
#include <stdio.h>

static thread_local char g_err[512] = "";

void m2m_set_error(const char* msg, const char* file, int line) {
    snprintf(g_err, sizeof(g_err), "%s (%s:%d)", msg, file, line);
}

extern "C" const char* m2m_last_error(void) { return g_err; }
extern "C" int m2m_abi_version(void) { return M2M_ABI_VERSION; }

extern "C" int64_t m2m_packed_bytes(int prec, int64_t I, int64_t K) {
    const int64_t kb = prec == PREC_BF16 ? 32 : 16;
    return ceil_div(I, 16) * ceil_div(K, kb) * 1024;
}

int m2m_check_tower(const m2m_tower* t, int B) {
    if (!t) { m2m_set_error("null tower", __FILE__, __LINE__); return -1; }
    if (t->prec != PREC_BF16 && t->prec != PREC_F32) { m2m_set_error("bad prec", __FILE__, __LINE__); return -1; }
    // (the chain kernels load block 0's / the last block's hidden bias and x_mid rows in their prologue, whatever nblocks is)
    if (t->nblocks < 1 || t->nblocks > M2M_MAX_BLOCKS) { m2m_set_error("nblocks out of range: a tower has 1 <= nblocks <= M2M_MAX_BLOCKS blocks (a tower of no blocks is not supported)", __FILE__, __LINE__); return -1; }
    if (t->D != 32 && t->D != 64 && t->D != 128 && t->D != 256) { m2m_set_error("hidden_dim D must be 32, 64, 128 or 256 in this build", __FILE__, __LINE__); return -1; }
    if (t->N < 1 || t->N > 128) { m2m_set_error("num_patch N must be in [1, 128] in this build", __FILE__, __LINE__); return -1; }
    if (t->T < 1 || t->T > 32) { m2m_set_error("token_dim T must be in [1, 32] in this build", __FILE__, __LINE__); return -1; }
    if (!m2m_is_wide(t) && (t->T % 8) != 0) { m2m_set_error("token_dim T must be a multiple of 8 on the fused path (N <= 8)", __FILE__, __LINE__); return -1; }
    if (t->Cp % 32 != 0 || t->Cp < t->C || t->C < 1) { m2m_set_error("Cp must be C rounded up to a multiple of 32", __FILE__, __LINE__); return -1; }
    if (B < 1) { m2m_set_error("B < 1", __FILE__, __LINE__); return -1; }
    if ((int64_t)B * t->N * (int64_t)t->Cp >= (1LL << 32)) { m2m_set_error("B*N*Cp exceeds the 32-bit dropout counter", __FILE__, __LINE__); return -1; }
    return 0;
}

// The caller's buffers of a tower call (include/m2mixer.h: m2m_tower_forward / _backward): the fused, split and chain kernels
// move every one of them as float4 and walk them by the sample strides.
static int io_error(const char* call, const char* what, const char* why) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s %s", call, what, why);
    m2m_set_error(msg, __FILE__, __LINE__);
    return -1;
}
static int io_check_ptr(const char* call, const char* what, const void* p, bool required) {
    if (!p) return required ? io_error(call, what, "is NULL") : 0;
    return (reinterpret_cast<uintptr_t>(p) & 15) ? io_error(call, what, "is not 16-byte aligned") : 0;
}
static int io_check_stride(const char* call, const char* what, const m2m_tower* t, int64_t ss) {
    if (ss < (int64_t)t->N * t->D) return io_error(call, what, "is smaller than N * D");
    return (ss % 4) ? io_error(call, what, "is not a multiple of 4 floats") : 0;
}
int m2m_check_tower_io(const char* call, const m2m_tower* t, const m2m_tower_io* f, const m2m_tower_gio* g) {
    if (f) {
        if (int rc = io_check_ptr(call, "x0", f->x0, true)) return rc;
        if (int rc = io_check_ptr(call, "out", f->out, true)) return rc;
        if (int rc = io_check_ptr(call, "pooled", f->pooled, false)) return rc;
        if (int rc = io_check_stride(call, "x0_sample_stride", t, f->x0_sample_stride)) return rc;
        if (int rc = io_check_stride(call, "out_sample_stride", t, f->out_sample_stride)) return rc;
        if (f->x0_parts > 1 && (f->x0_part_stride % 4)) return io_error(call, "x0_part_stride", "is not a multiple of 4 floats");
    }
    if (g) {
        if (int rc = io_check_ptr(call, "d_x0", g->d_x0, true)) return rc;
        if (int rc = io_check_ptr(call, "d_out", g->d_out, false)) return rc;
        if (int rc = io_check_ptr(call, "d_pooled", g->d_pooled, false)) return rc;
        if (int rc = io_check_stride(call, "d_x0_sample_stride", t, g->d_x0_sample_stride)) return rc;
        if (g->d_out)
            if (int rc = io_check_stride(call, "d_out_sample_stride", t, g->d_out_sample_stride)) return rc;
    }
    return 0;
}

// One tiny launch at the head of a training step instead of three scattered through it (each tiny kernel costs
// 3-9 us on the critical path of a replayed graph): Adam step count += 1, dropout step counter += 1, losses = 0.
__global__ void step_prologue_kernel(float* adam_state, unsigned int* drop_counter, float* losses, int nlosses) {
    const int t = threadIdx.x;
    if (t == 0 && adam_state) adam_state[0] += 1.0f;
    if (t == 1 && drop_counter) *drop_counter += 1u;
    if (losses && t < nlosses) losses[t] = 0.f;
}
extern "C" int m2m_step_prologue(float* adam_state, uint32_t* drop_counter, float* losses, int nlosses, void* stream) {
    if (nlosses < 0 || nlosses > 64) { m2m_set_error("step_prologue: nlosses must be in [0, 64]", __FILE__, __LINE__); return -1; }
    return m2m_launch<step_prologue_kernel>(dim3(1), dim3(64), 0, 0, reinterpret_cast<hipStream_t>(stream), adam_state, drop_counter, losses, nlosses);
}

__global__ void counter_add_kernel(unsigned int* c, unsigned int d) { *c += d; }
extern "C" int m2m_counter_add(uint32_t* counter, uint32_t delta, void* stream) {
    return m2m_launch<counter_add_kernel>(dim3(1), dim3(1), 0, 0, reinterpret_cast<hipStream_t>(stream), counter, delta);
}
