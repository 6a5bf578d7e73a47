// From run-time (precision, hidden_dim, token class, dropout mode) to a kernel instantiation, and the one launch helper.
//
// The value lists below are the ONE place that says which instantiations the library contains: an entry point dispatches over
// the list named at its site and over nothing else, so adding or retiring a shape is an edit here (and to m2m_check_tower's
// message).  tests/test_host_cpu.py::test_shape_envelope_covers_every_build restates them.
#pragma once
#include "host.h"
#include <type_traits>

template <int V> using ic = std::integral_constant<int, V>;
template <int... Vs> struct m2m_list {};

using m2m_precs = m2m_list<PREC_BF16, PREC_F32>;
using m2m_fused_dims = m2m_list<32, 64, 128>;           // hidden_dim of the fused path (whole samples per workgroup: N <= 8)
using m2m_wide_dims = m2m_list<32, 64, 128, 256>;       // hidden_dim of the row-wise launches: *_rows chains, weight gradients, embeddings
using m2m_pair_dims = m2m_list<256>;                    // hidden_dim of the two-towers-per-launch wide chains
using m2m_drop_modes = m2m_list<DM_NONE, DM_HALF, DM_GEN>;

enum { M2M_NO_BUILD = -1000 };                          // "the library has no instantiation for these values" (never a launch's result)

// f(ic<V>{}) for the V in Vs equal to v; `miss` if none
template <int... Vs, class F> int m2m_dispatch(int v, int miss, F&& f) {
    int rc = miss;
    (void)((v == Vs ? (rc = f(ic<Vs>{}), true) : false) || ...);
    return rc;
}
template <int... Vs, class F> int m2m_dispatch(m2m_list<Vs...>, int v, int miss, F&& f) { return m2m_dispatch<Vs...>(v, miss, f); }

// f(P, D) over both precisions and the hidden_dims of `dims`; M2M_NO_BUILD if (prec, D) is not built
template <int... Ds, class F> int m2m_dispatch_pd(m2m_list<Ds...>, int prec, int D, F&& f) {
    return m2m_dispatch(m2m_precs{}, prec, M2M_NO_BUILD, [&](auto P) {
        return m2m_dispatch<Ds...>(D, M2M_NO_BUILD, [&](auto DD) { return f(P, DD); });
    });
}
// f(DM) for the dropout mode of a launch (tile.h: m2m_drop_mode)
template <class F> int m2m_dispatch_dm(int training, float p_drop, F&& f) {
    return m2m_dispatch(m2m_drop_modes{}, m2m_drop_mode(training, p_drop), M2M_NO_BUILD, f);
}
// f(NMAX, TG): token class of a fused-path tower.  NMAX: tokens per sample the kernel holds (4 or 8); TG: lanes that share a
// column in the backward's token mixing (16 when they divide token_dim, else 8; the forward kernels do not depend on it).
template <class F> int m2m_fused_class(int N, int T, F&& f) {
    if (N <= 4) return f(ic<4>{}, ic<8>{});
    if (T % 16 == 0) return f(ic<8>{}, ic<16>{});
    return f(ic<8>{}, ic<8>{});
}

// Launch kernel K.  First raises K's dynamic-LDS limit to `lds_attr` bytes if that exceeds what this process has set for K so
// far (0: never touches it).  A site that passes a constant thereby sets the limit once, on K's first launch; a site that passes
// the size it asks for grows it.  The first launch of every kernel happens in an eager warm-up step, outside stream capture.
template <auto K> static size_t& m2m_lds_limit() { static size_t set = 0; return set; }
template <auto K, class... A>
static int m2m_launch(dim3 grid, dim3 block, size_t lds, size_t lds_attr, hipStream_t st, const A&... args) {
    if (lds_attr > m2m_lds_limit<K>()) {
        M2M_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_attr));
        m2m_lds_limit<K>() = lds_attr;
    }
    hipLaunchKernelGGL(K, grid, block, lds, st, args...);
    M2M_CHECK_HIP(hipGetLastError());
    return 0;
}
