// Count tables for accuracy / precision / recall / F1 (reference: the torchmetrics objects of setup_scores, updated per step in
// modules/train_test_module.py:72-151 from `preds` and `labels`).
//
// Every score the reference logs is a function of small integer tables, so a step only ADDS its batch's counts into a 64-bit
// device table (one launch at the end of the forward, inside the captured graph); the host reads the table once per epoch and
// derives the numbers in float64 (m2_mixer_amd/scores.py).  Integer adds commute: the table is exact and independent of the
// order in which workgroups arrive, so a bf16 step stays bit-reproducible with the launch in it.
//
// A workgroup histograms its rows in LDS (32-bit LDS atomics) and then issues ONE 64-bit global atomic add per non-zero cell:
// a 512-row batch costs tens of global atomics.  No float atomics.
#include "host.h"

#define SC_THREADS 256
#define SC_ROWS_PER_WG 1024                                  // multiclass rows of one workgroup (4 per thread)
#define SC_ELEMS_PER_WG 4096                                 // multilabel (row, label) elements of one workgroup (16 per thread)
#define SC_MC_CELLS (M2M_SCORES_MAX_CLASSES * M2M_SCORES_MAX_CLASSES + 1)
#define SC_ML_CELLS (M2M_SCORES_MAX_LABELS * 4)

// LDS histogram -> global table: one 64-bit add per non-zero cell (ncells <= the table's cells per head)
__device__ __forceinline__ void flush_cells(const unsigned int* hist, int ncells, unsigned long long* table) {
    for (int c = threadIdx.x; c < ncells; c += SC_THREADS) {
        const unsigned int v = hist[c];
        if (v) atomicAdd(table + c, (unsigned long long)v);
    }
}

// grid (workgroups, nheads).  table: (nheads, K * K + 1); cell [label * K + pred], the last one counts the skipped rows.
__global__ __launch_bounds__(SC_THREADS) void scores_multiclass_kernel(const int32_t* __restrict__ preds, const int64_t* __restrict__ labels,
                                                                      int B, int K, unsigned long long* __restrict__ table) {
    __shared__ unsigned int hist[SC_MC_CELLS];
    const int ncells = K * K + 1;
    const int h = blockIdx.y;
    for (int c = threadIdx.x; c < ncells; c += SC_THREADS) hist[c] = 0u;
    __syncthreads();
    const int32_t* p = preds + (int64_t)h * B;
    for (int64_t r0 = (int64_t)blockIdx.x * SC_ROWS_PER_WG; r0 < B; r0 += (int64_t)gridDim.x * SC_ROWS_PER_WG) {
        const int64_t r1 = r0 + SC_ROWS_PER_WG < B ? r0 + SC_ROWS_PER_WG : B;
        for (int64_t r = r0 + threadIdx.x; r < r1; r += SC_THREADS) {
            const int64_t l = labels[r];
            const int32_t q = p[r];
            const bool ok = l >= 0 && l < K && q >= 0 && q < K;
            atomicAdd(&hist[ok ? (int)l * K + q : K * K], 1u);
        }
    }
    __syncthreads();
    flush_cells(hist, ncells, table + (int64_t)h * ncells);
}

// grid (workgroups, nheads).  table: (nheads, K, 4) = tp, fp, fn, tn per label.
__global__ __launch_bounds__(SC_THREADS) void scores_multilabel_kernel(const int32_t* __restrict__ preds, const float* __restrict__ targets,
                                                                      int64_t n, int K, unsigned long long* __restrict__ table) {
    __shared__ unsigned int hist[SC_ML_CELLS];
    const int ncells = K * 4;
    const int h = blockIdx.y;
    for (int c = threadIdx.x; c < ncells; c += SC_THREADS) hist[c] = 0u;
    __syncthreads();
    const int32_t* p = preds + (int64_t)h * n;
    for (int64_t e0 = (int64_t)blockIdx.x * SC_ELEMS_PER_WG; e0 < n; e0 += (int64_t)gridDim.x * SC_ELEMS_PER_WG) {
        const int64_t e1 = e0 + SC_ELEMS_PER_WG < n ? e0 + SC_ELEMS_PER_WG : n;
        for (int64_t e = e0 + threadIdx.x; e < e1; e += SC_THREADS) {
            const int k = (int)(e % K);
            const bool pos = targets[e] >= 0.5f, hit = p[e] != 0;
            atomicAdd(&hist[k * 4 + (pos ? (hit ? 0 : 2) : (hit ? 1 : 3))], 1u);
        }
    }
    __syncthreads();
    flush_cells(hist, ncells, table + (int64_t)h * ncells);
}

static bool scores_args_ok(const void* preds, const void* truth, const void* table, int nheads, int B, int K, int kmax, const char* too_many) {
    if (!preds || !truth || !table || nheads < 1 || nheads > 65535 || B < 1 || K < 1) {
        m2m_set_error("scores: preds, labels / targets and the table must be given; nheads in [1, 65535], B >= 1, K >= 1", __FILE__, __LINE__);
        return false;
    }
    if (K > kmax) {
        m2m_set_error(too_many, __FILE__, __LINE__);
        return false;
    }
    if (reinterpret_cast<uintptr_t>(table) % 8 != 0) {
        m2m_set_error("scores: the count table must be 8-byte aligned", __FILE__, __LINE__);
        return false;
    }
    return true;
}

extern "C" int m2m_scores_multiclass(const int32_t* preds, const int64_t* labels, int nheads, int B, int K, uint64_t* table, void* stream) {
    if (!scores_args_ok(preds, labels, table, nheads, B, K, M2M_SCORES_MAX_CLASSES,
                        "scores: multiclass K exceeds M2M_SCORES_MAX_CLASSES (64)")) return -1;
    const int wgs = (B + SC_ROWS_PER_WG - 1) / SC_ROWS_PER_WG;
    hipLaunchKernelGGL(scores_multiclass_kernel, dim3(wgs < 64 ? wgs : 64, nheads), dim3(SC_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       preds, labels, B, K, reinterpret_cast<unsigned long long*>(table));
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int m2m_scores_multilabel(const int32_t* preds, const float* targets, int nheads, int B, int K, uint64_t* table, void* stream) {
    if (!scores_args_ok(preds, targets, table, nheads, B, K, M2M_SCORES_MAX_LABELS,
                        "scores: multilabel K exceeds M2M_SCORES_MAX_LABELS (128)")) return -1;
    const int64_t n = (int64_t)B * K;
    const int64_t wgs = (n + SC_ELEMS_PER_WG - 1) / SC_ELEMS_PER_WG;
    hipLaunchKernelGGL(scores_multilabel_kernel, dim3((unsigned)(wgs < 128 ? wgs : 128), nheads), dim3(SC_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), preds, targets, n, K, reinterpret_cast<unsigned long long*>(table));
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}
