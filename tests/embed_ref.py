"""float64 references of the patch embedding (forward, weight gradient, bias gradient), the derived error bound, and the
seeded inputs of tests/embed_cases.py.  CPU only: tests/test_host_embed_forms.py checks the references and the bound
themselves, tests/test_gpu_embed_forms.py holds the kernels to them.

    x0[m][d] = sum_k P[m][k] W[d][k] + b[d]      g_w[d][k] = sum_m dx0[m][d] P[m][k]      g_b[d] = sum_m dx0[m][d]
    P = the input as (B N, K) patches, m = b N + gy GW + gx, k = c ph pw + py pw + px  (plain reshapes, no unfold)

bf16 mode: the kernels round their MFMA operands to bf16 (round to nearest even) and accumulate in fp32, so the references
round the same operands first (`.bfloat16()`: the input and W in the forward; d_x0 and the input in both weight-gradient
forms; d_x0 also for g_b in the single-owner form, which sums the bf16 image) and what remains is fp32 accumulation alone.

The bound, componentwise:   |got - ref| <= (n + 2) 2^-23 S,   S = sum_i |a_i| |b_i| + |bias or sentinel|
n = every fp32 addition that can touch the element (contraction length + parts / wave reductions / row groups + the bias or
the "+="); one truncated ulp (2^-23 relative to the running sum, itself bounded by S) per addition.
"""
import torch

from embed_cases import geomK, geomN

ULP = 2.0 ** -23
GUARD = 64


def rnd(t, prec):
    """The operand as the MFMA sees it, in float64."""
    t = t.detach().float().cpu()
    return (t.bfloat16() if prec == "bf16" else t).double()


def patches(x, g):
    """(B, Cin, H, W) -> (B N, K)"""
    B = x.shape[0]
    GH, GW = g.H // g.ph, g.W // g.pw
    return x.reshape(B, g.Cin, GH, g.ph, GW, g.pw).permute(0, 2, 4, 1, 3, 5).reshape(B * GH * GW, g.Cin * g.ph * g.pw)


def bound(n, S):
    return (n + 2) * ULP * S


def fwd_ref(x, w, b, g, prec):
    """(x0, S): float64 forward and the magnitude sum of its bound."""
    P, W = patches(rnd(x, prec), g), rnd(w, prec).reshape(w.shape[0], -1)
    b = b.detach().double().cpu()
    return P @ W.t() + b, P.abs() @ W.abs().t() + b.abs()


def fwd_ref_short(x, w, b, g, prec):
    """The forward with the last k column left out: what a kernel that drops it would give."""
    P, W = patches(rnd(x, prec), g), rnd(w, prec).reshape(w.shape[0], -1)
    return P[:, :-1] @ W[:, :-1].t() + b.detach().double().cpu()


def wgrad_ref(x, dx0, g, prec, owner, rows=None):
    """(g_w, S_w, g_b, S_b); owner: the single-owner form (g_b sums the rounded d_x0); rows: use only the first `rows` token rows."""
    P = patches(rnd(x, prec), g)
    dx = dx0.detach().float().cpu().reshape(P.shape[0], -1)
    dr, db = rnd(dx, prec), (rnd(dx, prec) if owner else dx.double())
    if rows is not None:
        P, dr, db = P[:rows], dr[:rows], db[:rows]
    return dr.t() @ P, dr.abs().t() @ P.abs(), db.sum(0), db.abs().sum(0)


# ---- seeded inputs: sign * U(0.5, 1.5), so every product has magnitude >= 0.25 ---------------------------------------------
def signed_uniform(shape, gen):
    mag = torch.rand(shape, generator=gen) + 0.5
    sign = (torch.rand(shape, generator=gen) < 0.5).float() * 2 - 1
    return mag * sign


def make_inputs(g, D, B, seed):
    """x (B, Cin, H, W), w (D, Cin, ph, pw), b (D), dx0 (B N, D) -- float32, CPU"""
    gen = torch.Generator().manual_seed(seed)
    return (signed_uniform((B, g.Cin, g.H, g.W), gen), signed_uniform((D, g.Cin, g.ph, g.pw), gen), signed_uniform((D,), gen),
            signed_uniform((B * geomN(g), D), gen))


def sentinel(n):
    """A known finite pattern for "+=" outputs (exact in fp32, magnitudes up to 8)."""
    i = torch.arange(n, dtype=torch.int64)
    return ((i * 37) % 129 - 64).float() * 0.125


def check_bound(got, ref, n, S):
    """Largest err / bound over the elements (<= 1 passes).  `got`: float32 or float64 CPU tensor."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.reshape(-1)
    assert not torch.isnan(got).any(), "an output element was never written"
    return float(((got - ref).abs() / bound(n, S.reshape(-1))).max())


def is_sharp(ref, ref_short, n, S):
    """The bar is sharp: the reference with one term left out violates it somewhere."""
    return bool(((ref_short.reshape(-1) - ref.reshape(-1)).abs() > bound(n, S.reshape(-1))).any())


def count_fwd(g, nsplit=1):
    return geomK(g) + nsplit            # the contraction, the parts, the bias


def count_rows(g, B, groups):
    return B * geomN(g) + groups + 1     # the contraction, one atomic per row group, the "+="


def count_owner(g, B, waves):
    return B * geomN(g) + waves + 1      # the contraction, the wave reduction, the "+="
