// Epoch feed: a captured training step fetches its own batch.
//
// The split's tensors, a permutation and a cursor live in device memory.  m2m_feed_gather, at the head of the step, copies rows
// perm[(cursor + r) % n], r < B, of every source into the step's static input slots; a one-thread launch behind it advances the
// cursor (stream order is the barrier: nobody waits, nobody takes a ticket).  m2m_epoch_accumulate, one launch at the tail of the
// step, adds the step's losses and hit counts into the epoch's accumulators.  A replayed graph therefore needs no argument from
// the host, and an epoch is read back once.
//
// The gather is a pure copy: no float arithmetic, no LDS, no atomics.
//
// m2m_feed_gather_muted is the same gather with a muting schedule in device memory: per step one source may
// be zero-filled instead of copied (stage two of the reference's two-stage training); its advance launch also moves the schedule's
// step index.  m2m_feed_gather's kernels and launches are not shared with it, only the host-side checks are.
#include "host.h"

#define FD_THREADS 256
#define FD_UNROLL 4                                           // loads in flight per lane before the first store
#define FD_TILE (FD_THREADS * FD_UNROLL)                      // copy units (16 or 4 bytes) of one workgroup tile
#define FD_MAX_WG 2048                                        // grid cap: 8 workgroups per CU; larger batches stride

struct FeedSource {
    const char* src;
    char* dst;
    long long row_bytes;
    unsigned int units_per_row;                               // row_bytes / 16 (vec) or / 4
    unsigned int units;                                       // B * units_per_row
    unsigned int tile0;                                       // first tile of this source in the launch's tile list
    int vec;                                                  // 16 bytes per lane: row_bytes and both base addresses are multiples of 16
};

struct FeedArgs {
    FeedSource s[M2M_FEED_MAX_SOURCES];
    int nsrc;
    unsigned int tiles;
};

template <typename T>
__device__ __forceinline__ void feed_copy_tile(const FeedSource& f, unsigned int u0, const int32_t* __restrict__ perm, unsigned int c0,
                                               unsigned int n) {
    // Every lane issues all FD_UNROLL loads before its first store.  A lane past the end of the source (the ragged last tile only)
    // re-reads the source's last unit, so that the loads need no branch between them, and stores nothing.
    unsigned int row[FD_UNROLL], col[FD_UNROLL], idx[FD_UNROLL];
    T v[FD_UNROLL];
    const unsigned int last = f.units - 1u;
#pragma unroll
    for (int j = 0; j < FD_UNROLL; ++j) {
        const unsigned int u = min(u0 + j * FD_THREADS + threadIdx.x, last);          // consecutive lanes: consecutive units of a row
        row[j] = u / f.units_per_row;
        col[j] = u - row[j] * f.units_per_row;
        const unsigned int at = (c0 + row[j]) % n;                                    // (c0 < n, row < B < 2^31: no overflow)
        idx[j] = perm ? (unsigned int)perm[at] : at;
    }
#pragma unroll
    for (int j = 0; j < FD_UNROLL; ++j)
        v[j] = *reinterpret_cast<const T*>(f.src + (long long)idx[j] * f.row_bytes + (long long)col[j] * (long long)sizeof(T));
#pragma unroll
    for (int j = 0; j < FD_UNROLL; ++j)
        if (u0 + j * FD_THREADS + threadIdx.x <= last)
            *reinterpret_cast<T*>(f.dst + (long long)row[j] * f.row_bytes + (long long)col[j] * (long long)sizeof(T)) = v[j];
}

// grid (min(tiles, FD_MAX_WG)).  state: M2M_FEED_STATE_WORDS uint32 = cursor, arrival ticket (unused, zero), n, wrapped rows.
// The gather only READS the state; the launch behind it on the same stream advances the cursor (feed_advance_kernel).
__global__ __launch_bounds__(FD_THREADS) void feed_gather_kernel(const FeedArgs a, const int32_t* __restrict__ perm,
                                                                 const unsigned int* __restrict__ state) {
    const unsigned int cursor = state[0], n = state[2];                   // (uniform: one read per wavefront, cached)
    if (n == 0 || n >= 0x80000000u) return;                                // (an unset state copies nothing: no read without a row count)
    const unsigned int c0 = cursor % n;
    for (unsigned int t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        int s = 0;
        while (s + 1 < a.nsrc && t >= a.s[s + 1].tile0) ++s;
        const FeedSource& f = a.s[s];
        const unsigned int u0 = (t - f.tile0) * FD_TILE;
        if (f.vec) feed_copy_tile<uint4>(f, u0, perm, c0, n);
        else feed_copy_tile<unsigned int>(f, u0, perm, c0, n);
    }
}

// One thread, behind the gather on the same stream: launches on one stream are ordered, so every workgroup of the gather has read
// the cursor before this moves it, and the next gather sees it moved.  (The rank_append_kernel form -- every workgroup takes an
// arrival ticket, the last one advances -- was built first and measured: 1667 workgroups' tickets on one address cost 50 ns
// each, 83 us of a 101 us launch at M2-Mixer-B; DESIGN.md section 13.  The ticket word keeps its place in `state` and stays zero.)
__global__ __launch_bounds__(64) void feed_advance_kernel(int B, unsigned int* state) {
    if (threadIdx.x != 0) return;
    const unsigned int cursor = state[0], n = state[2];
    const unsigned int end = cursor + (unsigned int)B;
    if (end > n) state[3] += end - n;
    state[0] = end;
    state[1] = 0u;
}

// ---- the muted gather (m2m_feed_gather_muted): stage two of the reference's two-stage training zeroes one input per step -------
// feed_copy_tile with the tile's muting decision taken BETWEEN its index phase and its data phase.  The step's code is the end of
// a dependent pair of loads (mute_state[0] -> codes[step]) as the row index is (state -> perm[...]).  The kernel asks for the code
// through the VECTOR memory path before the tile loop (code_v: every lane the same address) and this function makes it uniform
// only after the perm loads are out: vector loads return in order, so waiting for the code leaves the perm loads in flight, and
// the two pairs overlap.  (As a scalar load ahead of the branch the code sat on every workgroup's critical path -- scalar loads
// are waited for all at once, and the source descriptors are scalar loads too: +0.9 us on a 26.8 us launch at M2-Mixer-B,
// DESIGN.md section 14.)  A muted tile stores zero bytes (what torch.zeros_like gives) and reads no source row; its perm entries
// were read.
template <typename T>
__device__ __forceinline__ void feed_tile_muted(const FeedSource& f, unsigned int u0, const int32_t* __restrict__ perm, unsigned int c0,
                                                unsigned int n, int s, int code_v) {
    unsigned int row[FD_UNROLL], col[FD_UNROLL], idx[FD_UNROLL];
    T v[FD_UNROLL];
    const unsigned int last = f.units - 1u;
#pragma unroll
    for (int j = 0; j < FD_UNROLL; ++j) {
        const unsigned int u = min(u0 + j * FD_THREADS + threadIdx.x, last);
        row[j] = u / f.units_per_row;
        col[j] = u - row[j] * f.units_per_row;
        const unsigned int at = (c0 + row[j]) % n;
        idx[j] = perm ? (unsigned int)perm[at] : at;
    }
    const int muted = __builtin_amdgcn_readfirstlane(code_v) - 1;                 // -1: nothing (a code outside [1, nsrc] matches no source)
    if (s == muted) {                                                             // workgroup-uniform
        memset(v, 0, sizeof(v));
    } else {
#pragma unroll
        for (int j = 0; j < FD_UNROLL; ++j)
            v[j] = *reinterpret_cast<const T*>(f.src + (long long)idx[j] * f.row_bytes + (long long)col[j] * (long long)sizeof(T));
    }
#pragma unroll
    for (int j = 0; j < FD_UNROLL; ++j)
        if (u0 + j * FD_THREADS + threadIdx.x <= last)
            *reinterpret_cast<T*>(f.dst + (long long)row[j] * f.row_bytes + (long long)col[j] * (long long)sizeof(T)) = v[j];
}

// feed_gather_kernel with a muting schedule: codes[mute_state[0]] is 0 (mute nothing) or s + 1 (mute source s); a step index past
// the schedule mutes nothing.  The code is one uniform load per workgroup, the decision is per tile (a tile belongs to one source):
// no atomics, no LDS, no ticket.  mute_state is only READ here; feed_advance_muted_kernel behind it moves the step index.
__global__ __launch_bounds__(FD_THREADS) void feed_gather_muted_kernel(const FeedArgs a, const int32_t* __restrict__ perm,
                                                                       const unsigned int* __restrict__ state,
                                                                       const int32_t* __restrict__ codes, int ncodes,
                                                                       const unsigned int* __restrict__ mute_state) {
    const unsigned int cursor = state[0], n = state[2], mstep = mute_state[0];
    // (all three uniform loads in flight together: without this the compiler sinks each below the branch before its first use and
    // waits for them one after the other)
    asm volatile("" ::"s"(cursor), "s"(n), "s"(mstep));
    if (n == 0 || n >= 0x80000000u) return;
    const unsigned int c0 = cursor % n;
    int code_v = 0;                                                               // (lane offset 0, opaque to the compiler: a vector load)
    if (mstep < (unsigned int)(ncodes > 0 ? ncodes : 0)) code_v = codes[mstep + __builtin_amdgcn_mbcnt_lo(0u, 0u)];
    for (unsigned int t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        int s = 0;
        while (s + 1 < a.nsrc && t >= a.s[s + 1].tile0) ++s;
        const FeedSource& f = a.s[s];
        const unsigned int u0 = (t - f.tile0) * FD_TILE;
        if (f.vec) feed_tile_muted<uint4>(f, u0, perm, c0, n, s, code_v);
        else feed_tile_muted<unsigned int>(f, u0, perm, c0, n, s, code_v);
    }
}

// feed_advance_kernel + the muting schedule's step index: mute_state[0] += 1; a step that ran past the schedule (it muted nothing)
// is counted in mute_state[1].
__global__ __launch_bounds__(64) void feed_advance_muted_kernel(int B, unsigned int* state, int ncodes, unsigned int* mute_state) {
    if (threadIdx.x != 0) return;
    const unsigned int cursor = state[0], n = state[2];
    const unsigned int end = cursor + (unsigned int)B;
    if (end > n) state[3] += end - n;
    state[0] = end;
    state[1] = 0u;
    const unsigned int mstep = mute_state[0];
    if (mstep >= (unsigned int)(ncodes > 0 ? ncodes : 0)) mute_state[1] += 1u;
    mute_state[0] = mstep + 1u;
}

// One wavefront, no atomics (launches on one stream are ordered).  sums: 2 * nloss doubles; counts: nheads + 2 uint64.
__global__ __launch_bounds__(64) void epoch_accumulate_kernel(const float* __restrict__ losses, int nloss, const int32_t* __restrict__ preds,
                                                              const int64_t* __restrict__ labels, int nheads, int B, double* sums,
                                                              unsigned long long* counts) {
    const int lane = threadIdx.x;
    for (int i = lane; i < nloss; i += 64) {
        const double l = (double)losses[i];
        sums[i] += l;
        sums[nloss + i] += l * (double)B;
    }
    for (int h = 0; h < nheads; ++h) {
        unsigned long long hits = 0;
        for (int r0 = 0; r0 < B; r0 += 64) {                               // (uniform trip count: every lane reaches the ballot)
            const int r = r0 + lane;
            const bool hit = r < B && (int64_t)preds[(int64_t)h * B + r] == labels[r];
            hits += (unsigned long long)__popcll(__ballot(hit));
        }
        if (lane == 0) counts[h] += hits;
    }
    if (lane == 0) {
        counts[nheads] += 1ull;
        counts[nheads + 1] += (unsigned long long)B;
    }
}

// The evidential model's epoch means (models/avmnist.py:556-572 logs the mean over steps of the step's batch-mean uncertainty):
// sums[h] += mean_r uncertainty[h][r], one value per step.  One wavefront, no atomics; the batch sum is taken in float64, lanes
// striding the rows, then a butterfly: the same order on every call.
__global__ __launch_bounds__(64) void epoch_accumulate_uq_kernel(const float* __restrict__ uncertainty, int nheads, int B, double* sums) {
    const int lane = threadIdx.x;
    for (int h = 0; h < nheads; ++h) {
        double s = 0.0;
        for (int r = lane; r < B; r += 64) s += (double)uncertainty[(int64_t)h * B + r];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) sums[h] += s / (double)B;
    }
}

// The checks and the tile list both gathers share; -1 (m2m_last_error) before anything is launched.
static int feed_build_args(const m2m_feed_src* srcs, int nsrc, int B, const uint32_t* state, FeedArgs& a) {
    if (!srcs || !state) {
        m2m_set_error("feed: srcs and state must be given (no NULL pointers)", __FILE__, __LINE__);
        return -1;
    }
    if (nsrc < 1 || nsrc > M2M_FEED_MAX_SOURCES) {
        m2m_set_error("feed: nsrc must be in [1, M2M_FEED_MAX_SOURCES (4)]", __FILE__, __LINE__);
        return -1;
    }
    if (B < 1) {
        m2m_set_error("feed: gather needs B >= 1", __FILE__, __LINE__);
        return -1;
    }
    a.nsrc = nsrc;
    unsigned long long tiles = 0;
    for (int i = 0; i < M2M_FEED_MAX_SOURCES; ++i) {
        FeedSource& f = a.s[i];
        if (i >= nsrc) {
            f = FeedSource{nullptr, nullptr, 0, 1u, 0u, 0xFFFFFFFFu, 0};
            continue;
        }
        if (!srcs[i].src || !srcs[i].dst) {
            m2m_set_error("feed: every source needs src and dst (no NULL pointers)", __FILE__, __LINE__);
            return -1;
        }
        const int64_t rb = srcs[i].row_bytes;
        if (rb < 4 || rb % 4 != 0) {
            m2m_set_error("feed: row_bytes must be a positive multiple of 4", __FILE__, __LINE__);
            return -1;
        }
        const uintptr_t ps = reinterpret_cast<uintptr_t>(srcs[i].src), pd = reinterpret_cast<uintptr_t>(srcs[i].dst);
        if (ps % 4 != 0 || pd % 4 != 0) {
            m2m_set_error("feed: src and dst must be 4-byte aligned", __FILE__, __LINE__);
            return -1;
        }
        f.vec = (rb % 16 == 0 && ps % 16 == 0 && pd % 16 == 0) ? 1 : 0;
        const int64_t upr = rb / (f.vec ? 16 : 4);
        if (upr * (int64_t)B >= ((int64_t)1 << 31) - FD_TILE) {
            m2m_set_error("feed: B * row_bytes / 4 (/ 16 on the 16-byte path) must stay below 2^31", __FILE__, __LINE__);
            return -1;
        }
        f.src = static_cast<const char*>(srcs[i].src);
        f.dst = static_cast<char*>(srcs[i].dst);
        f.row_bytes = rb;
        f.units_per_row = (unsigned int)upr;
        f.units = (unsigned int)(upr * B);
        f.tile0 = (unsigned int)tiles;
        tiles += (unsigned long long)ceil_div(f.units, FD_TILE);
    }
    if (tiles >= 0x80000000ull) {
        m2m_set_error("feed: the batch is too large for one gather launch", __FILE__, __LINE__);
        return -1;
    }
    a.tiles = (unsigned int)tiles;
    return 0;
}

extern "C" int m2m_feed_gather(const m2m_feed_src* srcs, int nsrc, const int32_t* perm, int B, uint32_t* state, void* stream) {
    FeedArgs a;
    if (int rc = feed_build_args(srcs, nsrc, B, state, a)) return rc;
    const unsigned int grid = a.tiles < FD_MAX_WG ? a.tiles : FD_MAX_WG;
    hipLaunchKernelGGL(feed_gather_kernel, dim3(grid), dim3(FD_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a, perm,
                       static_cast<const unsigned int*>(state));
    M2M_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(feed_advance_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), B, state);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int m2m_feed_gather_muted(const m2m_feed_src* srcs, int nsrc, const int32_t* perm, int B, uint32_t* state, const int32_t* codes,
                                     int ncodes, uint32_t* mute_state, void* stream) {
    if (!mute_state) {
        m2m_set_error("feed: the muted gather needs mute_state (no NULL pointer)", __FILE__, __LINE__);
        return -1;
    }
    if (ncodes < 0 || (ncodes > 0 && !codes)) {
        m2m_set_error("feed: ncodes >= 0, and ncodes > 0 needs codes (no NULL pointer)", __FILE__, __LINE__);
        return -1;
    }
    FeedArgs a;
    if (int rc = feed_build_args(srcs, nsrc, B, state, a)) return rc;
    const unsigned int grid = a.tiles < FD_MAX_WG ? a.tiles : FD_MAX_WG;
    hipLaunchKernelGGL(feed_gather_muted_kernel, dim3(grid), dim3(FD_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a, perm,
                       static_cast<const unsigned int*>(state), codes, ncodes, static_cast<const unsigned int*>(mute_state));
    M2M_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(feed_advance_muted_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), B, state, ncodes, mute_state);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int m2m_epoch_accumulate(const float* losses, int nloss, const int32_t* preds, const int64_t* labels, int nheads, int B,
                                    double* sums, uint64_t* counts, void* stream) {
    if (!losses || !sums || !counts || nloss < 1) {
        m2m_set_error("epoch_accumulate: losses, sums and counts must be given (no NULL pointers); nloss >= 1", __FILE__, __LINE__);
        return -1;
    }
    if (nheads < 0 || (nheads > 0 && (!preds || !labels))) {
        m2m_set_error("epoch_accumulate: nheads >= 0, and nheads > 0 needs preds and labels", __FILE__, __LINE__);
        return -1;
    }
    if (B < 1) {
        m2m_set_error("epoch_accumulate: needs B >= 1", __FILE__, __LINE__);
        return -1;
    }
    hipLaunchKernelGGL(epoch_accumulate_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), losses, nloss, preds, labels,
                       nheads, B, sums, reinterpret_cast<unsigned long long*>(counts));
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int m2m_epoch_accumulate_uq(const float* uncertainty, int nheads, int B, double* sums, void* stream) {
    if (!uncertainty || !sums) {
        m2m_set_error("epoch_accumulate_uq: uncertainty and sums must be given (no NULL pointers)", __FILE__, __LINE__);
        return -1;
    }
    if (nheads < 1 || B < 1) {
        m2m_set_error("epoch_accumulate_uq: needs nheads >= 1 and B >= 1", __FILE__, __LINE__);
        return -1;
    }
    hipLaunchKernelGGL(epoch_accumulate_uq_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), uncertainty, nheads, B, sums);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}
