"""The library's test hooks, run on the device (-m gpu): m2m_gemm_probe and m2m_pack (the packed fragment layouts and the
accumulator -> operand chaining every tower kernel is built on), m2m_gelu_probe (the fp32 GELU with the hardware reciprocal and
exp), m2m_gelu_table_probe (the 512-cell piecewise-linear tables every bf16 step evaluates GELU and GELU' through), and the
plain MLP's large-batch (VALU) kernels.  References are float64 (tests/leaf_ref.py, oracle.mlp); every bar is derived in the
docstring of its test, and every error goes through conftest.observe."""
import math

import numpy as np
import pytest
import torch

import drop_ref as DR
import leaf_ref as R
from conftest import observe
from oracle import m2mixer_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -24             # unit roundoff of fp32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------------
# packed layouts and chaining
# ---------------------------------------------------------------------------------------------------------------------------
def operand(rows, cols, a, b, mod, div, fine):
    """Distinct, signed values per element: ((a r + b c) mod `mod` - mod // 2) / div is exact in bf16; `fine` adds
    (r cols + c) 2^-12 in fp32 mode, so that every element differs and a transposed or permuted fragment cannot pass."""
    r, c = torch.arange(rows).view(-1, 1), torch.arange(cols).view(1, -1)
    v = ((a * r + b * c) % mod - mod // 2).float() / div
    return v + (r * cols + c).float() * 2.0 ** -12 if fine else v


def gemm_inputs(prec, I, J, K, J2):
    fine = prec == 1
    return operand(I, K, 7, 13, 61, 16.0, fine), operand(J, K, 11, 5, 53, 16.0, fine), operand(J2, J, 5, 9, 47, 32.0, fine)


def run_probe(prec, A, Bm, Bc, dev):
    from m2_mixer_amd import _lib as L
    (I, K), J, J2 = A.shape, Bm.shape[0], Bc.shape[0]
    sizes = [L.lib().m2m_packed_bytes(prec, I, K), L.lib().m2m_packed_bytes(prec, J, K), L.lib().m2m_packed_bytes(prec, J2, J)]
    assert sizes == [L.packed_bytes(prec, I, K), L.packed_bytes(prec, J, K), L.packed_bytes(prec, J2, J)]
    ws = torch.zeros(sum(sizes) + 65536, dtype=torch.uint8, device=dev)          # zero-filled, generous
    a, b, bc = A.to(dev).contiguous(), Bm.to(dev).contiguous(), Bc.to(dev).contiguous()
    C1, C2 = torch.zeros(I, J, device=dev), torch.zeros(I, J2, device=dev)
    L.check(L.lib().m2m_gemm_probe(prec, a.data_ptr(), b.data_ptr(), I, J, K, bc.data_ptr(), J2, C1.data_ptr(), C2.data_ptr(),
                                   ws.data_ptr(), L.stream_ptr()), "gemm_probe")
    torch.cuda.synchronize()
    return C1.cpu(), C2.cpu(), ws.cpu(), sizes


def gamma(k):
    return k * U / (1.0 - k * U)


def bf16_ulp(x):
    """One unit in the last place of bf16 at |x| (8 significand bits)."""
    _, e = torch.frexp(x.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 8)


PROBE_SHAPES = [(1, 1, 1, 1), (16, 15, 16, 16), (17, 16, 17, 33), (40, 17, 32, 1), (1, 32, 48, 16), (16, 33, 80, 33),
                (17, 100, 17, 1), (40, 100, 80, 33), (40, 1, 48, 16), (16, 16, 1, 33), (17, 15, 32, 16), (1, 33, 80, 1)]     # (I, K, J, J2)


@pytest.mark.parametrize("I,K,J,J2", PROBE_SHAPES)
@pytest.mark.parametrize("prec", [0, 1], ids=["bf16", "fp32"])
def test_gemm_probe_product_and_chained_product(prec, I, K, J, J2, dev):
    """C = A B^T and the chained C2 = C Bc^T through pack + MFMA.  Reference: the float64 product of the operands as the kernel
    rounds them (bf16 mode: round-to-nearest-even to bf16; fp32 mode: unrounded); for C2 the first operand is the kernel's own C
    (rounded to bf16 in bf16 mode).  Bar, derived: |err| <= gamma_n sum_k |a_k| |b_k| elementwise with gamma_n = n u / (1 - n u),
    u = 2^-24, n the contraction length (K for C, J for C2) -- the classical bound of an n-term fp32 dot product in any order;
    the chained product in bf16 mode adds one bf16 ulp of C per term (sum_j ulp_bf16(C_ij) |Bc_j|).  A layout mistake gives O(1)
    errors.  J = 17, 48, 80: an odd number of j tiles, where the second accumulator of a pair is empty."""
    A, Bm, Bc = gemm_inputs(prec, I, J, K, J2)
    C1, C2, _, _ = run_probe(prec, A, Bm, Bc, dev)
    rnd = (lambda t: t.bfloat16().double()) if prec == 0 else (lambda t: t.double())
    a, b, bc = rnd(A), rnd(Bm), rnd(Bc)
    name = "bf16" if prec == 0 else "fp32"
    bar1 = gamma(K) * (a.abs() @ b.abs().T)
    err1 = (C1.double() - a @ b.T).abs()
    observe(f"gemm probe {name} C (err / bar)", float((err1 / bar1.clamp_min(1e-300)).max()), 1.0)
    assert bool((err1 <= bar1).all()), float((err1 - bar1).max())
    c = rnd(C1)
    bar2 = gamma(J) * (c.abs() @ bc.abs().T) + (bf16_ulp(C1) @ bc.abs().T if prec == 0 else 0.0)
    err2 = (C2.double() - c @ bc.T).abs()
    observe(f"gemm probe {name} C2 (err / bar)", float((err2 / bar2.clamp_min(1e-300)).max()), 1.0)
    assert bool((err2 <= bar2).all()), float((err2 - bar2).max())


@pytest.mark.parametrize("prec", [0, 1], ids=["bf16", "fp32"])
def test_padding_contributes_exactly_zero(prec, dev):
    """A product with ragged K (17: one element into the second fp32 k-block, 15 short of the bf16 one) equals, bit for bit, the
    product over K = 32 with columns 17.. explicitly zero: same k-blocks, and the padding the pack wrote is exactly zero."""
    I, K, J, J2 = 17, 17, 48, 16
    A, Bm, Bc = gemm_inputs(prec, I, J, K, J2)
    Az, Bz = torch.zeros(I, 32), torch.zeros(J, 32)
    Az[:, :K], Bz[:, :K] = A, Bm
    r, z = run_probe(prec, A, Bm, Bc, dev), run_probe(prec, Az, Bz, Bc, dev)
    assert torch.equal(r[0], z[0]) and torch.equal(r[1], z[1])


@pytest.mark.parametrize("prec", [0, 1], ids=["bf16", "fp32"])
def test_pack_images_agree_with_the_probe(prec, dev):
    """m2m_pack called directly, I and K ragged (I = 17, K = 33; J2 = 33, J = 48): from a strided source with NaN outside the valid
    (I, K) region, and from the transposed source with stride_i / stride_k swapped, it must produce the very images
    m2m_gemm_probe packed for the same operands (whose products the tests above hold to float64) -- agreement, no assertion on
    the opaque bytes; order_k_major = 1 holds block (ib, kb) at kb * nIB + ib where order 0 holds it at ib * nKB + kb (the
    header's rule).  The image is exactly m2m_packed_bytes long: every 16-byte slot inside is written, none after it."""
    from m2_mixer_amd import _lib as L
    I, K, J, J2 = 17, 33, 48, 33
    A, Bm, Bc = gemm_inputs(prec, I, J, K, J2)
    _, _, ws, sizes = run_probe(prec, A, Bm, Bc, dev)
    img_a, img_bc = ws[:sizes[0]], ws[sizes[0] + sizes[1]:sum(sizes)]
    GUARD, FILL = 4096, 0xAB

    def pack(mode, kmajor, src, si, sk, rows, cols):
        n = L.lib().m2m_packed_bytes(prec, rows, cols)
        dst = torch.full((n + GUARD,), FILL, dtype=torch.uint8, device=dev)
        L.check(L.lib().m2m_pack(prec, mode, kmajor, src.data_ptr(), si, sk, rows, cols, dst.data_ptr(), L.stream_ptr()), "pack")
        torch.cuda.synchronize()
        dst = dst.cpu()
        assert bool((dst[n:] == FILL).all())                                              # nothing past the image
        assert not bool((dst[:n].view(-1, 16) == FILL).all(dim=1).any())                  # every slot of it written
        return dst[:n]

    def strided(X):                       # X inside a larger NaN-filled buffer
        big = torch.full((X.shape[0] + 3, X.shape[1] + 5), float("nan"))
        big[:X.shape[0], :X.shape[1]] = X
        return big.to(dev), X.shape[1] + 5

    src, ld = strided(A)
    assert torch.equal(pack(0, 0, src, ld, 1, I, K), img_a)                               # NAT, order 0, row-major source
    srcT, ldT = strided(A.T.contiguous())
    nat0 = pack(0, 0, srcT, 1, ldT, I, K)                                                 # the transposed source
    assert torch.equal(nat0, img_a)
    src, ld = strided(Bc)
    chn1 = pack(1, 1, src, ld, 1, J2, J)
    assert torch.equal(chn1, img_bc)                                                      # CHN, order 1 (the probe's Bc image)
    srcT, ldT = strided(Bc.T.contiguous())
    assert torch.equal(pack(1, 1, srcT, 1, ldT, J2, J), img_bc)
    for mode, X, rows, cols, k_major_img in ((0, A, I, K, None), (1, Bc, J2, J, chn1)):
        kb = 32 if prec == 0 else 16
        nIB, nKB = (rows + 15) // 16, (cols + kb - 1) // kb
        src, ld = strided(X)
        o0 = pack(mode, 0, src, ld, 1, rows, cols).view(nIB, nKB, 1024)
        o1 = pack(mode, 1, src, ld, 1, rows, cols).view(nKB, nIB, 1024)
        assert torch.equal(o0.transpose(0, 1), o1)
        if k_major_img is not None:
            assert torch.equal(o1.reshape(-1), k_major_img)


# ---------------------------------------------------------------------------------------------------------------------------
# GELU on the device
# ---------------------------------------------------------------------------------------------------------------------------
H_CELL = 12.0 / 512


def gelu_points(table):
    """The host test's dense grid over [-8, 8] plus the edges: +-0, the clamp of the erf argument (+-4 sqrt 2 (1 +- 2^-23)),
    +-1e-20, +-40, +-inf; for the tables also +-6 and their neighbours (cells 0 / 1 and 512 / 513), every cell boundary, NaN."""
    f32 = lambda v: np.asarray(v, dtype=np.float32)
    c = f32(4.0 * math.sqrt(2.0))
    pts = [np.linspace(-8.0, 8.0, 200001).astype(np.float32), f32([0.0, -0.0, 1e-20, -1e-20, 40.0, -40.0, np.inf, -np.inf]),
           f32([c * (1 + 2.0 ** -23), c * (1 - 2.0 ** -23), -c * (1 + 2.0 ** -23), -c * (1 - 2.0 ** -23)])]
    if table:
        six = f32(6.0)
        pts += [f32([6.0, -6.0]), np.nextafter(six, f32(0)).reshape(1), np.nextafter(six, f32(7)).reshape(1),
                np.nextafter(-six, f32(0)).reshape(1), np.nextafter(-six, f32(-7)).reshape(1),
                (-6.0 + H_CELL * np.arange(513)).astype(np.float32), f32([np.nan])]
    return torch.from_numpy(np.concatenate(pts))


def held(kind, got, ref, bar):
    """got within bar of ref wherever the float64 formula is a number (it is NaN at -inf, and for gelu' at +-inf: 0 x inf);
    infinities must match exactly.  Returns the mask of compared points."""
    got, ok = got.double(), ~torch.isnan(ref)
    fin = ok & torch.isfinite(ref)
    assert torch.equal(got[ok & ~fin], ref[ok & ~fin])
    err = (got[fin] - ref[fin]).abs()
    assert not bool(torch.isnan(err).any())
    observe(f"{kind} (max abs err)", float(err.max()), float(bar[fin][err.argmax()]))
    ratio = float((err / bar[fin].clamp_min(1e-300)).max())         # (bar = 0 at x = 0, where the result is exact)
    observe(f"{kind} (err / bar)", ratio, 1.0)
    assert bool((err <= bar[fin]).all()), (kind, ratio)
    return fin


def test_fp32_gelu_and_its_derivative_on_the_device(dev):
    """m2m_gelu_probe -- gelu_f / gelu_grad_f with the hardware reciprocal and exp -- against float64 erf GELU and
    Phi(x) + x phi(x).

    gelu_f(x) = 0.5 x (1 + erf_fast(x / sqrt 2)).  Error of the device erf: E_erf = 6e-7 (the rational's bound, held on the host
    by test_erf_rational_coefficients) + 4 u: the reciprocal (1 ulp = 2 u |erf| <= 2 u), the product p x rcp (u), and the rounded
    argument x / sqrt 2 (relative 2 u, times max |z erf'(z)| = 0.48: < u); u = 2^-24.  The sum 1 + erf rounds by u |1 + erf|
    <= 2 u, the factor 0.5 x is exact up to the last product (u |gelu|; 2 u with the intermediate 0.5 x cdf of the gradient form).
        bar_y(x)  = 0.5 |x| (E_erf + 2 u) + 2 u |gelu(x)|
    gelu'(x) = fma(x, 0.3989.. exp(-x^2 / 2), cdf): the cdf term carries 0.5 (E_erf + 2 u); the exp factor carries its absolute
    error E_exp times 0.399 |x|, E_exp MEASURED here on the same grid (m2m_gelu_table_probe form 4 returns the device's
    exp(-x^2 / 2) itself; float64 exp on the same float x) and recorded; the constant's product and the fma round by
    u (|x| phi(x) + |gelu'(x)|) each at most twice.
        bar_dy(x) = 0.5 (E_erf + 2 u) + 0.3989423 |x| E_exp + 2 u (|x| phi(x) + |gelu'(x)|)
    Measured on an MI355X: E_exp = 5.84e-8 (reference side: float64 exp, exact to 1e-16); with it the kernel's largest errors
    are 9.2e-7 for gelu (bar there 2.6e-6) and 2.3e-7 for gelu' (bar there 7.3e-7; 0.31 of the bar at the tightest point)."""
    from m2_mixer_amd import _lib as L
    x = gelu_points(False).to(dev)
    y, dy, ex = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    L.check(L.lib().m2m_gelu_probe(x.data_ptr(), y.data_ptr(), dy.data_ptr(), x.numel(), L.stream_ptr()), "gelu_probe")
    L.check(L.lib().m2m_gelu_table_probe(4, x.data_ptr(), ex.data_ptr(), 0, x.numel(), 1.0, L.stream_ptr()), "gelu_table_probe")
    torch.cuda.synchronize()
    xd = x.cpu().double()
    e_exp = float((ex.cpu().double() - torch.exp(-0.5 * xd * xd)).abs().max())
    observe("gelu fp32 device exp(-x^2/2) (max abs err, measured)", e_exp, 2.0 ** -20)
    # sanity only (the bar below uses the measured value): the argument -x^2 / 2 and its scaling to base 2 round three times, an
    # absolute error |t| e^-|t| 3 u <= 0.37 x 3 u of the result, and the hardware exp2 is good to ~2 ulp of a result <= 1: < 2^-20
    assert e_exp < 2.0 ** -20
    ref_y, ref_dy = R.gelu(xd), R.gelu_grad(xd)
    e_erf = 6e-7 + 4 * U
    ax = xd.abs()
    fy, fdy = torch.nan_to_num(ref_y.abs(), nan=0.0, posinf=0.0), torch.nan_to_num(ref_dy.abs(), nan=0.0, posinf=0.0)
    phi = torch.exp(-0.5 * xd * xd) / math.sqrt(2 * math.pi)
    bar_y = 0.5 * ax * (e_erf + 2 * U) + 2 * U * fy
    bar_dy = 0.5 * (e_erf + 2 * U) + 0.3989423 * ax * e_exp + 2 * U * (torch.nan_to_num(ax * phi, nan=0.0) + fdy)
    held("gelu fp32 y", y.cpu(), ref_y, bar_y)
    held("gelu fp32 dy", dy.cpu(), ref_dy, bar_dy)


def pwl_terms(xd, scale):
    """|a_i| + |b_i x| and |c_i| + |d_i x| of the cell x falls in (float64 restatement of pwl_cell), for the fp16 form's bar."""
    i = torch.floor(xd * (512 / 12.0) + 257.0).clamp(0, 513)
    x0 = -6.0 + H_CELL * (i - 1)
    x1 = x0 + H_CELL
    inside = (i >= 1) & (i <= 512)
    b = (R.gelu(x1) - R.gelu(x0)) / H_CELL
    d = (R.gelu_grad(x1) - R.gelu_grad(x0)) / H_CELL
    a, c = R.gelu(x0) - b * x0, R.gelu_grad(x0) - d * x0
    top = i >= 513
    zero = torch.zeros_like(xd)
    ty = torch.where(inside, a.abs() + (b * xd).abs(), torch.where(top, xd.abs(), zero))
    tdy = torch.where(inside, c.abs() + (d * xd).abs(), torch.where(top, torch.ones_like(xd), zero))
    return scale * torch.nan_to_num(ty, nan=0.0, posinf=0.0), scale * torch.nan_to_num(tdy, nan=0.0, posinf=0.0)


@pytest.mark.parametrize("scale", [1.0, 2.0, 1.0 / 0.9], ids=["1", "2", "1/0.9"])
@pytest.mark.parametrize("form", [0, 1, 2], ids=["fp32 table", "forward-only table", "fp16 table"])
def test_gelu_tables_hold_the_bounds_the_source_claims(form, scale, dev):
    """The tables as the chain kernels fill and read them (m2m_gelu_table_probe), against float64 GELU x scale at the bounds
    csrc/common.h states: 6e-5 x scale for gelu and 9e-5 x scale for gelu' through the fp32 tables; the fp16 table adds 2^-11
    relative of each coefficient term (|a_i| + |b_i x|, resp. |c_i| + |d_i x|) and, like every fp32 result, u = 2^-24 of the
    value.  (Interpolation alone: max |gelu''| h^2 / 8 = 0.80 x 5.5e-4 / 8 = 5.5e-5 and max |gelu'''| h^2 / 8 = 0.78 x 5.5e-4 / 8
    = 5.4e-5 with h = 12 / 512.)  NaN in gives NaN out; the zero keep-mask form returns exact zeros.
    Observed on an MI355X, as a share of these bars: gelu 0.91 and gelu' 0.59 through the fp32 tables (5.5e-5 and 5.3e-5 at
    scale 1: the claims hold), 0.94 and 0.83 through the fp16 table."""
    from m2_mixer_amd import _lib as L
    x = gelu_points(True).to(dev)
    y, dy = torch.full_like(x, -5.0), torch.full_like(x, -5.0)
    L.check(L.lib().m2m_gelu_table_probe(form, x.data_ptr(), y.data_ptr(), dy.data_ptr() if form != 1 else 0, x.numel(), scale,
                                         L.stream_ptr()), "gelu_table_probe")
    torch.cuda.synchronize()
    xd = x.cpu().double()
    nan = torch.isnan(xd)
    assert int(nan.sum()) == 1 and bool(torch.isnan(y.cpu()[nan]).all())
    xs = xd[~nan]
    ty, tdy = pwl_terms(xs, scale)
    name = ("fp32 table", "forward-only table", "fp16 table")[form]
    sc = np.float32(scale).item()                     # the scale as the kernel receives it
    ref_y, ref_dy = R.gelu(xs) * sc, R.gelu_grad(xs) * sc
    extra = 2.0 ** -11 if form == 2 else 0.0
    bar_y = 6e-5 * sc + extra * ty + U * torch.nan_to_num(ref_y.abs(), nan=0.0, posinf=0.0)
    held(f"gelu {name} y", y.cpu()[~nan], ref_y, bar_y)
    if form != 1:
        assert bool(torch.isnan(dy.cpu()[nan]).all())
        bar_dy = 9e-5 * sc + extra * tdy + U * torch.nan_to_num(ref_dy.abs(), nan=0.0, posinf=0.0)
        held(f"gelu {name} dy", dy.cpu()[~nan], ref_dy, bar_dy)
    else:
        assert bool((dy == -5.0).all())               # the forward-only form writes no derivative


def test_masked_gelu_table_returns_exact_zeros(dev):
    from m2_mixer_amd import _lib as L
    x = gelu_points(True)
    x = x[torch.isfinite(x)].to(dev)                  # (0 x inf and NaN are NaN in any arithmetic)
    y, dy = torch.full_like(x, -5.0), torch.full_like(x, -5.0)
    L.check(L.lib().m2m_gelu_table_probe(3, x.data_ptr(), y.data_ptr(), dy.data_ptr(), x.numel(), 2.0, L.stream_ptr()), "gelu_table_probe")
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0 and float(dy.abs().max()) == 0.0
    for form, yy, dd, n in ((5, y, dy, x.numel()), (0, 0, dy, x.numel()), (0, y, 0, x.numel()), (0, y, dy, -1)):
        rc = L.lib().m2m_gelu_table_probe(form, x.data_ptr(), yy if isinstance(yy, int) else yy.data_ptr(),
                                          dd if isinstance(dd, int) else dd.data_ptr(), n, 1.0, L.stream_ptr())
        assert rc == -1


# ---------------------------------------------------------------------------------------------------------------------------
# the plain MLP above 2048 samples (VALU kernels, 32 samples per workgroup)
# ---------------------------------------------------------------------------------------------------------------------------
MLP_BAR = 1e-4


def mlp_setup(dims, has_out, p_drop, B, dev, seed=5):
    from m2_mixer_amd.runtime import MlpRuntime
    gen = torch.Generator().manual_seed(seed)
    nl = len(dims) - 1
    params = {}
    for i in range(nl):
        params[f"module_list.{3 * i}.weight"] = torch.randn(dims[i + 1], dims[i], generator=gen) / math.sqrt(dims[i])
        params[f"module_list.{3 * i}.bias"] = 0.1 * torch.randn(dims[i + 1], generator=gen)
    x = torch.randn(B, dims[0], generator=gen)
    dp = {k: v.to(dev) for k, v in params.items()}
    grads = {k: torch.zeros_like(v) for k, v in dp.items()}
    rt = MlpRuntime(list(dims), has_out, p_drop, 77)
    pairs = lambda d: [(d[f"module_list.{3 * i}.weight"], d[f"module_list.{3 * i}.bias"]) for i in range(nl)]
    rt.bind(pairs(dp), pairs(grads), B)
    return rt, params, dp, grads, x


def mlp_forward(rt, x, B, dout, training, step, dev, step_dev=None):
    out = torch.zeros(B, 3, dout, device=dev)                          # strided destination: token 0 of a (B, 3, dout) buffer
    dense = torch.zeros(B, dout, device=dev)
    acts = rt.fresh_acts(B, dev)
    rt.forward(x, B, out, 3 * dout, dense, training, 123, step, step_dev)
    torch.cuda.synchronize()
    return out, dense, acts


def relmax(a, b):
    a, b = R.f64(a), R.f64(b)
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-300)


@pytest.mark.parametrize("B", [2049, 2081])
@pytest.mark.parametrize("p_drop", [0.0, 0.3])
@pytest.mark.parametrize("dims,has_out", [((3, 17, 128, 2), True), ((7, 100, 33), False)], ids=["3-17-128-2 out", "7-100-33"])
def test_mlp_large_batch_vs_float64(dims, has_out, p_drop, B, dev):
    """Training and evaluation forward, and the backward, of the VALU kernels (B > 2048: one sample past the switch, and a ragged
    last workgroup) against float64 oracle.mlp fed the masks read from the saved activations; bar 1e-4 of each tensor's max.
    Keep rate over the positive pre-activations within 6 binomial standard deviations of round((1 - p) 65536) / 65536."""
    rt, params, dp, grads, x = mlp_setup(dims, has_out, p_drop, B, dev)
    xg, dout, nhid = x.to(dev), dims[-1], len(dims) - 1 - int(has_out)
    out, dense, acts = mlp_forward(rt, xg, B, dout, True, 1, dev)
    thr = DR.drop_thr(p_drop)
    keep_q = thr / 65536
    leaves = {k: v.double().requires_grad_(True) for k, v in params.items()}
    h, masks = x.double(), []
    for i in range(nhid):
        z = torch.relu(O.linear(h, leaves[f"module_list.{3 * i}.weight"], leaves[f"module_list.{3 * i}.bias"]))
        mask = (acts[i].cpu() != 0).double() if p_drop > 0 else torch.ones_like(z)
        pos = z.detach() > 1e-6
        if p_drop > 0:
            n, rate = int(pos.sum()), float(mask[pos].mean())
            sd = math.sqrt(keep_q * (1 - keep_q) / n)
            assert observe(f"mlp large-batch keep rate (binomial sd)", abs(rate - keep_q) / sd, 6.0) < 6.0, (i, rate, n)
        masks.append(mask)
        h = z * mask / keep_q
        assert observe("mlp large-batch activations (rel to max)", relmax(acts[i], h), MLP_BAR) < MLP_BAR, i
    ref = O.mlp(x.double(), leaves, "", nhid, has_out, 1 - keep_q, masks if p_drop > 0 else None)
    assert observe("mlp large-batch output (rel to max)", relmax(dense, ref), MLP_BAR) < MLP_BAR
    assert torch.equal(out[:, 0, :], dense) and float(out[:, 1:, :].abs().max()) == 0.0
    gen = torch.Generator().manual_seed(9)
    d1, d2 = torch.randn(B, 3, dout, generator=gen), torch.randn(B, dout, generator=gen)
    rt.backward(xg, B, d1.to(dev), 3 * dout, d2.to(dev))
    torch.cuda.synchronize()
    (ref * (d1[:, 0, :] + d2).double()).sum().backward()
    for k, g in grads.items():
        assert observe("mlp large-batch gradients (rel to max)", relmax(g, leaves[k].grad), MLP_BAR) < MLP_BAR, k
    # evaluation: no dropout, nothing saved
    out_e, dense_e, acts_e = mlp_forward(rt, xg, B, dout, False, 2, dev)
    ref_e = O.mlp(x.double(), {k: v.double() for k, v in params.items()}, "", nhid, has_out)
    assert observe("mlp large-batch output (rel to max)", relmax(dense_e, ref_e), MLP_BAR) < MLP_BAR
    assert all(float(a.abs().max()) == 0.0 for a in acts_e)


def test_mlp_large_batch_dropout_stream(dev):
    """The same (seed, step) draws the same masks, another step different ones, and a step split between the host argument and
    the device counter (step_dev) the same as their sum."""
    dims, B = (7, 100, 33), 2049
    rt, _, _, _, x = mlp_setup(dims, False, 0.3, B, dev)
    xg = x.to(dev)
    a = mlp_forward(rt, xg, B, 33, True, 5, dev)
    b = mlp_forward(rt, xg, B, 33, True, 5, dev)
    c = mlp_forward(rt, xg, B, 33, True, 6, dev)
    d = mlp_forward(rt, xg, B, 33, True, 2, dev, step_dev=torch.tensor([3], dtype=torch.int32, device=dev))
    for i in range(2):
        assert torch.equal(a[2][i], b[2][i]) and torch.equal(a[2][i], d[2][i])
        differ = float(((a[2][i] != 0) != (c[2][i] != 0)).float().mean())
        assert differ > 0.05, differ                  # (independent masks at keep 0.7 differ on 42 % of the positive half)
    assert torch.equal(a[1], b[1]) and torch.equal(a[1], d[1]) and not torch.equal(a[1], c[1])


@pytest.mark.parametrize("dims,has_out", [((3, 17, 128, 2), True), ((7, 100, 33), False)], ids=["3-17-128-2 out", "7-100-33"])
def test_mlp_paths_agree_bit_for_bit(dims, has_out, dev):
    """csrc/mlp_body.h: the MFMA body (B <= 2048) and the VALU kernels produce bitwise the same forward values.  Rows 0..2047 of
    a B = 2049 forward therefore equal the B = 2048 forward of the same rows, dropout on (the masks index by sample, not by
    workgroup)."""
    rt, _, _, _, x = mlp_setup(dims, has_out, 0.3, 2049, dev)
    xg = x.to(dev)
    big = mlp_forward(rt, xg, 2049, dims[-1], True, 4, dev)
    small = mlp_forward(rt, xg[:2048].contiguous(), 2048, dims[-1], True, 4, dev)
    assert torch.equal(big[1][:2048], small[1])
    for a, b in zip(big[2], small[2]):
        assert torch.equal(a[:2048], b)
