// Ranking buffers for average precision (the reference's `auroc`) and ROC-AUC (reference: models/mimic.py:126-128 softmax of the
// heads' logits, :162-180 torchmetrics.AveragePrecision(task="multiclass", average="macro") under the name `auroc`).
//
// Both scores are functions of four integers per sample.  For a sample i of class c with score s_i = p_i[c]: n_ge / p_ge = the
// samples / the class-c samples whose class-c score is >= s_i, n_gt / p_gt the same with >.  So a step only
// APPENDS its batch's softmax rows to a device buffer (m2m_rank_append: one launch at the place of the count-table launch, inside
// the captured graph; the row cursor lives in device memory), and m2m_rank_counts produces the integers once per epoch: O(n^2)
// compares per head, exact, independent of the order of arrival and of execution, no sort.  The host derives the numbers in
// float64 (m2_mixer_amd/scores.py: rank_scores).
//
// Buffer layout: probs[h][c][row] -- row stride 1, class stride `capacity`, head stride K * capacity: the class column the
// counting kernel scans is contiguous, and the append's stores of one class are coalesced over the batch.
// Integer atomics only (the arrival ticket, the cursor, the skipped-label count); every other store is a plain vector store.
#include "host.h"

#define RK_APPEND_THREADS 64                                  // one softmax row per thread: B = 512, 3 heads -> 24 workgroups
#define RK_TI 256                                             // rows i of one counting workgroup (one per thread)
#define RK_TJ 128                                             // rows j of one LDS tile
#define RK_COL (RK_TJ + 1)                                    // LDS column stride, odd: lanes on different columns at one j hit different banks

// grid (ceil(B / RK_APPEND_THREADS), nheads).  state: M2M_RANK_STATE_WORDS uint32.
__global__ __launch_bounds__(RK_APPEND_THREADS) void rank_append_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                                       int B, int K, float* __restrict__ probs, int32_t* __restrict__ row_labels,
                                                                       int64_t capacity, unsigned int* state) {
    __shared__ unsigned int base;
    const int h = blockIdx.y;
    if (threadIdx.x == 0) base = __hip_atomic_load(&state[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int b = blockIdx.x * RK_APPEND_THREADS + threadIdx.x;
    // maximum and sum need no row: they run while thread 0's read of the cursor is in flight
    const float* x = logits + ((int64_t)h * B + (b < B ? b : 0)) * K;
    int64_t l = 0;
    if (h == 0 && b < B) l = labels[b];
    float m = x[0];
    for (int k = 1; k < K; ++k) m = fmaxf(m, x[k]);
    float sum = 0.f;
    for (int k = 0; k < K; ++k) sum += expf(x[k] - m);                     // index order
    __syncthreads();
    const int64_t row = (int64_t)base + b;
    const bool skipped = l < 0 || l >= K;                                  // (l = 0 off head 0 and past B: never skipped)
    if (b < B && row < capacity) {
        if (h == 0) row_labels[row] = skipped ? -1 : (int32_t)l;
        float* out = probs + (int64_t)h * K * capacity + row;
        for (int k = 0; k < K; ++k) out[(int64_t)k * capacity] = expf(x[k] - m) / sum;          // (the same expf of the same operand)
    }
    if (h == 0) {
        const unsigned long long bad = __ballot(skipped);                  // one wavefront per workgroup
        if (threadIdx.x == 0 && bad) atomicAdd(&state[2], (unsigned int)__popcll(bad));
    }
    // The cursor: every workgroup has read state[0] before it takes its ticket; the last one to arrive advances the cursor and
    // clears the ticket for the next launch.  Nobody waits for anybody.
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        const unsigned int total = gridDim.x * gridDim.y;
        if (atomicAdd(&state[1], 1u) == total - 1u) {
            atomicAdd(&state[0], (unsigned int)B);
            atomicExch(&state[1], 0u);
        }
    }
}

// grid (ceil(n / RK_TI), nheads).  counts: (nheads, n, 4) uint32 = n_ge, p_ge, n_gt, p_gt.
// A row without a label (-1) enters the LDS tile as NaN in every column: it compares false both ways, so it is invisible to the
// other rows without a test in the inner loop; so is the padding of the ragged last tile.  A row i without a label scans with
// s = NaN and gets four zeros the same way.
__global__ __launch_bounds__(RK_TI) void rank_counts_kernel(const float* __restrict__ probs, const int32_t* __restrict__ row_labels,
                                                           int64_t n, int K, int64_t capacity, uint4* __restrict__ counts) {
    __shared__ float col[M2M_SCORES_MAX_CLASSES * RK_COL];
    __shared__ int lab[RK_TJ];
    const float nan = __builtin_nanf("");
    const float* p = probs + (int64_t)blockIdx.y * K * capacity;
    const int64_t i = (int64_t)blockIdx.x * RK_TI + threadIdx.x;
    int y = -1;
    float s = nan;
    if (i < n) {
        y = row_labels[i];
        if (y >= 0 && y < K) s = p[(int64_t)y * capacity + i];
        else y = -1;
    }
    const float* mine = col + (y < 0 ? 0 : y) * RK_COL;
    unsigned int n_ge = 0, p_ge = 0, n_gt = 0, p_gt = 0;
    for (int64_t j0 = 0; j0 < n; j0 += RK_TJ) {
        __syncthreads();
        if (threadIdx.x < RK_TJ) {
            const int64_t j = j0 + threadIdx.x;
            int l = j < n ? row_labels[j] : -1;
            lab[threadIdx.x] = (l >= 0 && l < K) ? l : -1;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < K * RK_TJ; e += RK_TI) {
            const int c = e / RK_TJ, jj = e % RK_TJ;
            col[c * RK_COL + jj] = lab[jj] >= 0 ? p[(int64_t)c * capacity + j0 + jj] : nan;      // (lab < 0 covers j >= n: no read there)
        }
        __syncthreads();
#pragma unroll 8
        for (int jj = 0; jj < RK_TJ; ++jj) {
            const float v = mine[jj];
            const unsigned int same = lab[jj] == y;
            const unsigned int ge = v >= s, gt = v > s;
            n_ge += ge;
            n_gt += gt;
            p_ge += ge & same;
            p_gt += gt & same;
        }
    }
    if (i < n) counts[(int64_t)blockIdx.y * n + i] = make_uint4(n_ge, p_ge, n_gt, p_gt);
}

static bool rank_args_ok(bool pointers, int nheads, int K, int64_t capacity) {
    if (!pointers || nheads < 1 || nheads > 65535 || K < 1) {
        m2m_set_error("rank: every buffer must be given (no NULL pointers); nheads in [1, 65535], K >= 1", __FILE__, __LINE__);
        return false;
    }
    if (K > M2M_SCORES_MAX_CLASSES) {
        m2m_set_error("rank: K exceeds M2M_SCORES_MAX_CLASSES (64)", __FILE__, __LINE__);
        return false;
    }
    if (capacity < 1) {
        m2m_set_error("rank: capacity must be >= 1", __FILE__, __LINE__);
        return false;
    }
    return true;
}

extern "C" int m2m_rank_append(const float* logits, const int64_t* labels, int nheads, int B, int K, float* probs, int32_t* row_labels,
                               int64_t capacity, uint32_t* state, void* stream) {
    if (!rank_args_ok(logits && labels && probs && row_labels && state, nheads, K, capacity)) return -1;
    if (B < 1) {
        m2m_set_error("rank: append needs B >= 1", __FILE__, __LINE__);
        return -1;
    }
    hipLaunchKernelGGL(rank_append_kernel, dim3((unsigned)ceil_div(B, RK_APPEND_THREADS), nheads), dim3(RK_APPEND_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), logits, labels, B, K, probs, row_labels, capacity, state);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int m2m_rank_counts(const float* probs, const int32_t* row_labels, int nheads, int64_t n, int K, int64_t capacity,
                               uint32_t* counts, void* stream) {
    if (!rank_args_ok(probs && row_labels && counts, nheads, K, capacity)) return -1;
    if (n < 0 || n > capacity) {
        m2m_set_error("rank: counts needs 0 <= n <= capacity (n > capacity: the buffer holds no such rows)", __FILE__, __LINE__);
        return -1;
    }
    if (n >= ((int64_t)1 << 31)) {
        m2m_set_error("rank: counts are 32-bit: n must be below 2^31", __FILE__, __LINE__);
        return -1;
    }
    if (reinterpret_cast<uintptr_t>(counts) % 16 != 0) {
        m2m_set_error("rank: the counts buffer must be 16-byte aligned", __FILE__, __LINE__);
        return -1;
    }
    if (n == 0) return 0;
    hipLaunchKernelGGL(rank_counts_kernel, dim3((unsigned)ceil_div(n, RK_TI), nheads), dim3(RK_TI), 0,
                       reinterpret_cast<hipStream_t>(stream), probs, row_labels, n, K, capacity, reinterpret_cast<uint4*>(counts));
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}
