// Prediction record: an evaluation step appends its own outputs to a record of the split.
//
// The mirror image of the feed's gather (feed.hip).  The record's buffers and a cursor live in device memory.  m2m_record_append,
// behind the launch that writes a step's logits and predictions, copies row r < B of every source (a step's output buffer) to row
// cursor + r of its destination (the record's buffer of `capacity` rows); a one-thread launch behind it advances the cursor
// (stream order is the barrier, as for the feed: feed.hip says why a ticket was measured and rejected).  A replayed graph
// therefore needs no argument from the host, and a split's predictions are read back once.
//
// A row at or past `capacity` is never written; the advance launch counts it in state[3].
//
// The append is a pure copy: no float arithmetic, no LDS, no atomics.  Tile sizes are the feed gather's.
#include "host.h"

#define RC_THREADS 256
#define RC_UNROLL 4                                           // loads in flight per lane before the first store
#define RC_TILE (RC_THREADS * RC_UNROLL)                      // copy units (16 or 4 bytes) of one workgroup tile
#define RC_MAX_WG 2048                                        // grid cap: 8 workgroups per CU; larger batches stride

struct RecordSource {
    const char* src;
    char* dst;
    long long row_bytes;
    unsigned int units_per_row;                               // row_bytes / 16 (vec) or / 4
    unsigned int units;                                       // B * units_per_row
    unsigned int tile0;                                       // first tile of this source in the launch's tile list
    int vec;                                                  // 16 bytes per lane: row_bytes and both base addresses are multiples of 16
};

struct RecordArgs {
    RecordSource s[M2M_RECORD_MAX_SOURCES];
    int nsrc;
    unsigned int tiles;
};

template <typename T>
__device__ __forceinline__ void record_copy_tile(const RecordSource& f, unsigned int u0, unsigned long long cursor,
                                                 unsigned long long capacity) {
    // Every lane issues all RC_UNROLL loads before its first store.  A lane past the end of the source (the ragged last tile only)
    // re-reads the source's last unit, so that the loads need no branch between them, and stores nothing.  A row at or past the
    // capacity is read (it is a row of the step's own buffer) and not stored.
    unsigned int row[RC_UNROLL], col[RC_UNROLL];
    T v[RC_UNROLL];
    const unsigned int last = f.units - 1u;
#pragma unroll
    for (int j = 0; j < RC_UNROLL; ++j) {
        const unsigned int u = min(u0 + j * RC_THREADS + threadIdx.x, last);          // consecutive lanes: consecutive units of a row
        row[j] = u / f.units_per_row;
        col[j] = u - row[j] * f.units_per_row;
    }
#pragma unroll
    for (int j = 0; j < RC_UNROLL; ++j)
        v[j] = *reinterpret_cast<const T*>(f.src + (long long)row[j] * f.row_bytes + (long long)col[j] * (long long)sizeof(T));
#pragma unroll
    for (int j = 0; j < RC_UNROLL; ++j) {
        const unsigned long long at = cursor + row[j];                                // (cursor < 2^32, row < 2^31: no overflow)
        if (u0 + j * RC_THREADS + threadIdx.x <= last && at < capacity)
            *reinterpret_cast<T*>(f.dst + (long long)at * f.row_bytes + (long long)col[j] * (long long)sizeof(T)) = v[j];
    }
}

// grid (min(tiles, RC_MAX_WG)).  state: M2M_RECORD_STATE_WORDS uint32 = rows appended, reserved, reserved, rows dropped.
// The append only READS the state; the launch behind it on the same stream advances the cursor (record_advance_kernel).
__global__ __launch_bounds__(RC_THREADS) void record_append_kernel(const RecordArgs a, unsigned long long capacity,
                                                                   const unsigned int* __restrict__ state) {
    const unsigned long long cursor = state[0];                           // (uniform: one read per wavefront, cached)
    if (cursor >= capacity) return;                                       // (a full record: every row of this step is dropped)
    for (unsigned int t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        int s = 0;
        while (s + 1 < a.nsrc && t >= a.s[s + 1].tile0) ++s;
        const RecordSource& f = a.s[s];
        const unsigned int u0 = (t - f.tile0) * RC_TILE;
        if (f.vec) record_copy_tile<uint4>(f, u0, cursor, capacity);
        else record_copy_tile<unsigned int>(f, u0, cursor, capacity);
    }
}

// One thread, behind the append on the same stream: every workgroup of the append has read the cursor before this moves it, and
// the next append sees it moved (feed_advance_kernel's form).  The cursor keeps counting past the capacity; words 1 and 2 are
// reserved and left alone (the caller's clear zeroed them).
__global__ __launch_bounds__(64) void record_advance_kernel(int B, unsigned long long capacity, unsigned int* state) {
    if (threadIdx.x != 0) return;
    const unsigned long long cursor = state[0];
    const unsigned long long end = cursor + (unsigned long long)B;
    if (end > capacity) {
        const unsigned long long over = end - capacity;
        state[3] += (unsigned int)(over < (unsigned long long)B ? over : (unsigned long long)B);
    }
    state[0] = (unsigned int)end;
}

// The checks and the tile list; -1 (m2m_last_error) before anything is launched.
static int record_build_args(const m2m_feed_src* srcs, int nsrc, int B, int64_t capacity, const uint32_t* state, RecordArgs& a) {
    if (!srcs || !state) {
        m2m_set_error("record: srcs and state must be given (no NULL pointers)", __FILE__, __LINE__);
        return -1;
    }
    if (nsrc < 1 || nsrc > M2M_RECORD_MAX_SOURCES) {
        m2m_set_error("record: nsrc must be in [1, M2M_RECORD_MAX_SOURCES (16)]", __FILE__, __LINE__);
        return -1;
    }
    if (B < 1) {
        m2m_set_error("record: append needs B >= 1", __FILE__, __LINE__);
        return -1;
    }
    if (capacity < 1) {
        m2m_set_error("record: append needs capacity >= 1", __FILE__, __LINE__);
        return -1;
    }
    a.nsrc = nsrc;
    unsigned long long tiles = 0;
    for (int i = 0; i < M2M_RECORD_MAX_SOURCES; ++i) {
        RecordSource& f = a.s[i];
        if (i >= nsrc) {
            f = RecordSource{nullptr, nullptr, 0, 1u, 0u, 0xFFFFFFFFu, 0};
            continue;
        }
        if (!srcs[i].src || !srcs[i].dst) {
            m2m_set_error("record: every source needs src and dst (no NULL pointers)", __FILE__, __LINE__);
            return -1;
        }
        const int64_t rb = srcs[i].row_bytes;
        if (rb < 4 || rb % 4 != 0) {
            m2m_set_error("record: row_bytes must be a positive multiple of 4", __FILE__, __LINE__);
            return -1;
        }
        const uintptr_t ps = reinterpret_cast<uintptr_t>(srcs[i].src), pd = reinterpret_cast<uintptr_t>(srcs[i].dst);
        if (ps % 4 != 0 || pd % 4 != 0) {
            m2m_set_error("record: src and dst must be 4-byte aligned", __FILE__, __LINE__);
            return -1;
        }
        // (as a quotient: B * row_bytes itself may not fit 64 bits.  Below 2^31 four-byte units, a tile's last unit index
        // -- at most RC_TILE - 1 past the source's last -- fits 32 bits.)
        if (rb / 4 > (((int64_t)1 << 31) - 1) / (int64_t)B) {
            m2m_set_error("record: B * row_bytes / 4 must stay below 2^31", __FILE__, __LINE__);
            return -1;
        }
        // 16 bytes per lane: then every destination row is 16-byte aligned whatever the cursor is
        f.vec = (rb % 16 == 0 && ps % 16 == 0 && pd % 16 == 0) ? 1 : 0;
        const int64_t upr = rb / (f.vec ? 16 : 4);
        f.src = static_cast<const char*>(srcs[i].src);
        f.dst = static_cast<char*>(srcs[i].dst);
        f.row_bytes = rb;
        f.units_per_row = (unsigned int)upr;
        f.units = (unsigned int)(upr * B);
        f.tile0 = (unsigned int)tiles;
        tiles += (unsigned long long)ceil_div(f.units, RC_TILE);
    }
    a.tiles = (unsigned int)tiles;                            // (at most 16 x 2^21 tiles)
    return 0;
}

extern "C" int m2m_record_append(const m2m_feed_src* srcs, int nsrc, int B, int64_t capacity, uint32_t* state, void* stream) {
    RecordArgs a;
    if (int rc = record_build_args(srcs, nsrc, B, capacity, state, a)) return rc;
    const unsigned int grid = a.tiles < RC_MAX_WG ? a.tiles : RC_MAX_WG;
    hipLaunchKernelGGL(record_append_kernel, dim3(grid), dim3(RC_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a,
                       (unsigned long long)capacity, static_cast<const unsigned int*>(state));
    M2M_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(record_advance_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), B,
                       (unsigned long long)capacity, state);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}
