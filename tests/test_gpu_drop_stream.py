"""The library's dropout stream against its host replica (-m gpu): tests/drop_ref.py, numpy uint32 written from the specification
("Dropout stream"), shares no code with the library -- unlike the mask probe, which is built from the kernels' own
mix32 / m2m_site_key / m2m_drop_thr / drop_keep and moves with them.

  towers   m2m_dropout_mask (TowerRuntime.dropout_mask) equals the replica BIT FOR BIT at every site of three tiny towers, over
           rates, seeds, steps, site bases and the first / last block.  The kernels are tied to the probe by the float64 oracle
           tests (engine_ref.tower_masks and the shape / split envelopes feed the oracle the probe's masks), so the equality
           carries over to them.
           A second test at B = 512 pins the threshold's rounding, which moves one element in 65536.
  MLP      the plain MLP has no probe.  Its saved activations are exactly 0 wherever the replica drops and non-zero wherever it
           keeps and the float64 pre-activation is clearly positive; outputs, activations and all gradients agree with
           oracle.mlp fed the REPLICA's masks within MLP_BAR (1e-4 of each tensor's maximum, tests/test_gpu_probes.py): the MFMA
           body (B <= 2048), the VALU kernels (B = 2049), the recorded call flushed on its own, and a step split between the host
           argument and the device counter, also across 2^32; at p = 0.95 the scale 65536 / thr tells a truncated threshold."""
import numpy as np
import pytest
import torch

import drop_ref as DR
import gen_util as G
from conftest import observe
from oracle import m2mixer_oracle as O
from test_gpu_probes import MLP_BAR, dev, mlp_forward, mlp_setup, relmax  # noqa: F401

pytestmark = pytest.mark.gpu

U32MAX = 2 ** 32 - 1
# name -> (N, D, T, C, blocks): a fused tower with a padded hidden width (Cp = 64); a fused one at hidden_dim 128; a wide one whose
# token-out rows (N = 33 columns) take two words in the one-bit mode
TOWERS = {"fused n3 d32 c33": (3, 32, 24, 33, 2), "fused n8 d128": (8, 128, 16, 100, 3), "wide n33 d64": (33, 64, 20, 33, 2)}
# (p, seed, step, site_base, last block?): every rate of the host test's grid (0.5 -- the one-bit draws -- three times), seeds
# {0, 123, 2^32 - 1}, steps {0, 1, 2^32 - 1}, bases {0, 1024, 2^20}, both blocks; x 4 sites x 3 towers = 96 probe launches
DRAWS = [(0.1, 0, 0, 0, False), (0.3, U32MAX, 1, 1024, True), (0.5, 123, U32MAX, 1 << 20, False), (0.9, 0, 1, 1 << 20, True),
         (0.5, U32MAX, 0, 1024, True), (0.5, 0, 1, 0, True), (0.1, 123, U32MAX, 1024, False), (0.3, 123, 0, 0, True)]
TOWER_B = 3


@pytest.mark.parametrize("name", list(TOWERS))
def test_mask_probe_equals_the_host_replica(name, dev):
    from m2_mixer_amd import _lib as L
    from m2_mixer_amd.runtime import TowerRuntime
    N, D, T, C, nb = TOWERS[name]
    assert {d[0] for d in DRAWS} == {0.1, 0.3, 0.5, 0.9} and {d[1] for d in DRAWS} == {0, 123, U32MAX}
    assert {d[2] for d in DRAWS} == {0, 1, U32MAX} and {d[3] for d in DRAWS} == {0, 1024, 1 << 20} and {d[4] for d in DRAWS} == {True, False}
    bad = []
    for p, seed, step, base, last in DRAWS:
        rt = TowerRuntime(D, N, T, C, nb, True, p, L.PREC_F32, base)
        rt.device = dev                                   # (the probe reads the descriptor only: no parameters bound)
        blk = nb - 1 if last else 0
        for site in range(4):
            got = rt.dropout_mask(blk, site, TOWER_B, seed, step).cpu().numpy()
            want = DR.tower_mask(seed, step, base, blk, site, p, TOWER_B, N, D, T, rt.Cp)
            assert got.shape == want.shape and got.dtype == np.uint8
            if not np.array_equal(got, want):
                first = int(np.flatnonzero(got != want)[0])
                bad.append(f"p {p} seed {seed} step {step} base {base} block {blk} site {site}: {int((got != want).sum())} of "
                           f"{got.size} differ, first at {first}")
    assert not bad, f"{name}: " + "; ".join(bad)


TIE = 0.25 - 2.0 ** -17            # a float32; (1 - p) 65536 = 49152.5: half up gives 49153, truncation and half-even 49152


@pytest.mark.parametrize("p", [0.9, TIE], ids=["0.9", "tie"])
def test_mask_probe_rounds_the_threshold_as_the_replica(p, dev):
    """A threshold off by one moves one element in 65536, which the tiny towers above cannot see.  At B = 512 the channel sites of
    the D = 128 tower have 2^19 elements: the replica's own masks for thr - 1 and thr + 1 differ from the one for thr (asserted
    here, so the comparison is known to be sharp), and the probe equals the one for thr = (long)((1 - p) 65536 + 0.5): at 0.9
    truncation gives 6553 for 6554, at the tie truncation and round-half-even give 49152 for 49153."""
    from m2_mixer_amd import _lib as L
    from m2_mixer_amd.runtime import TowerRuntime
    N, D, T, C, nb = TOWERS["fused n8 d128"]
    B, seed, step, base = 512, 123, 1, 1024
    thr = DR.drop_thr(p)
    assert thr == {0.9: 6554, TIE: 49153}[p] and int((1 - float(np.float32(p))) * 65536) == thr - 1
    rt = TowerRuntime(D, N, T, C, nb, True, p, L.PREC_F32, base)
    rt.device = dev
    for site in range(4):
        got = rt.dropout_mask(0, site, B, seed, step).cpu().numpy()
        want = DR.tower_mask(seed, step, base, 0, site, p, B, N, D, T, rt.Cp)
        if site >= 2:
            key = DR.site_key(seed, step, base + site)
            for other in (thr - 1, thr + 1):
                assert not np.array_equal(DR.generic_mask(key, other, want.size), want), (site, other)
        assert np.array_equal(got, want), f"site {site}: {int((got != want).sum())} of {got.size} elements differ"


# ---- the plain MLP ----------------------------------------------------------------------------------------------------------------
MLP_SEED, MLP_BASE = 123, 77                               # what test_gpu_probes.mlp_forward / mlp_setup pass


def replica_masks(dims, has_out, p, B, step):
    nhid = len(dims) - 1 - int(has_out)
    return [torch.from_numpy(DR.mlp_mask(MLP_SEED, step, MLP_BASE, l, p, B, dims[l + 1])).double() for l in range(nhid)]


def check_forward(params, x, dims, has_out, p, masks, acts, dense, kind):
    """Saved activations and output of a training forward against the replica's masks and float64; returns (reference output,
    float64 leaves) for the backward."""
    nhid, keep_q = len(dims) - 1 - int(has_out), DR.drop_thr(p) / 65536
    leaves = {k: v.double().requires_grad_(True) for k, v in params.items()}
    h = x.double()
    for i in range(nhid):
        z = torch.relu(O.linear(h, leaves[f"module_list.{3 * i}.weight"], leaves[f"module_list.{3 * i}.bias"]))
        a, m = acts[i].cpu(), masks[i]
        dropped, live = m == 0, (m == 1) & (z.detach() > 1e-6 * float(z.detach().max()))
        assert 0.02 < float(dropped.double().mean()) < 0.98 and int(live.sum()) > 0, (kind, i)
        assert float(a[dropped].abs().max()) == 0.0, f"{kind}: layer {i} kept units the replica drops"
        assert bool((a[live] != 0).all()), f"{kind}: layer {i} dropped {int((a[live] == 0).sum())} units the replica keeps"
        h = z * m / keep_q
        assert observe(f"mlp vs replica masks [{kind}] activations (rel to max)", relmax(a, h), MLP_BAR) < MLP_BAR, i
    ref = O.mlp(x.double(), leaves, "", nhid, has_out, 1 - keep_q, masks)
    assert observe(f"mlp vs replica masks [{kind}] output (rel to max)", relmax(dense, ref), MLP_BAR) < MLP_BAR
    return ref, leaves


def check_backward(ref, leaves, grads, d1, d2, kind):
    (ref * (d1[:, 0, :] + d2).double()).sum().backward()
    for k, g in grads.items():
        assert observe(f"mlp vs replica masks [{kind}] gradients (rel to max)", relmax(g, leaves[k].grad), MLP_BAR) < MLP_BAR, k


@pytest.mark.parametrize("B", [37, 2048, 2049])
@pytest.mark.parametrize("p_drop", [0.3, 0.5])
@pytest.mark.parametrize("dims,has_out", [((3, 17, 128, 2), True), ((7, 100, 33), False)], ids=["3-17-128-2 out", "7-100-33"])
def test_mlp_draws_the_replicas_masks(dims, has_out, p_drop, B, dev):
    """MFMA body (B = 37: ragged 16-sample tiles; B = 2048: the last batch it takes) and VALU kernels (B = 2049), 16-bit draws at
    both rates (the MLP has no one-bit mode: p = 0.5 too compares halves of a word with 32768)."""
    rt, params, dp, grads, x = mlp_setup(dims, has_out, p_drop, B, dev)
    assert rt.desc.site_base == MLP_BASE
    xg, dout, step = x.to(dev), dims[-1], 3
    out, dense, acts = mlp_forward(rt, xg, B, dout, True, step, dev)
    kind = "mfma" if B <= 2048 else "valu"
    ref, leaves = check_forward(params, x, dims, has_out, p_drop, replica_masks(dims, has_out, p_drop, B, step), acts, dense, kind)
    assert torch.equal(out[:, 0, :], dense)
    gen = torch.Generator().manual_seed(9)
    d1, d2 = torch.randn(B, 3, dout, generator=gen), torch.randn(B, dout, generator=gen)
    rt.backward(xg, B, d1.to(dev), 3 * dout, d2.to(dev))
    torch.cuda.synchronize()
    check_backward(ref, leaves, grads, d1, d2, kind)


@pytest.mark.parametrize("p_drop", [0.3, 0.5])
def test_flushed_mlp_ride_draws_the_replicas_masks(p_drop, dev):
    """m2m_mlp_forward_ride / _backward_ride with no carrier (m2m_mlp_ride_flush launches the recorded call), on the MIMIC static
    MLP's widths at the batch of test_gpu_parity.test_mlp_ride_is_the_mlp_launch_with_or_without_a_carrier."""
    cs = G.MIMIC_H["static"]
    dims, B, step = (cs["input_dim"], cs["hidden_dim"], cs["hidden_dim"], cs["output_dim"]), 48, 6
    rt, params, dp, grads, x = mlp_setup(dims, True, p_drop, B, dev)
    xg, dout = x.to(dev), dims[-1]
    out, dense = torch.zeros(B, 3, dout, device=dev), torch.zeros(B, dout, device=dev)
    acts = rt.fresh_acts(B, dev)
    rt.forward_ride(xg, B, out, 3 * dout, dense, True, MLP_SEED, step)
    rt.ride_flush()
    torch.cuda.synchronize()
    ref, leaves = check_forward(params, x, dims, True, p_drop, replica_masks(dims, True, p_drop, B, step), acts, dense, "ride flush")
    gen = torch.Generator().manual_seed(9)
    d1, d2 = torch.randn(B, 3, dout, generator=gen), torch.randn(B, dout, generator=gen)
    rt.backward_ride(xg, B, d1.to(dev), 3 * dout, d2.to(dev))
    rt.ride_flush()
    torch.cuda.synchronize()
    check_backward(ref, leaves, grads, d1, d2, "ride flush")


@pytest.mark.parametrize("B", [37, 2049])
def test_mlp_split_step_draws_the_replicas_mask_of_the_sum(B, dev):
    """step = host argument + device counter modulo 2^32: every split draws the replica's mask of the sum, also when the sum (or the
    device counter read as a signed integer) wraps."""
    dims, p_drop = (7, 100, 33), 0.3
    rt, params, dp, grads, x = mlp_setup(dims, False, p_drop, B, dev)
    xg = x.to(dev)
    for host, devc in ((2, 3), (0, 5), (U32MAX, 2), (7, U32MAX - 1), (1 << 31, 1 << 31), (U32MAX, U32MAX)):
        ctr = torch.tensor([devc - (1 << 32) if devc >= 1 << 31 else devc], dtype=torch.int32, device=dev)
        out, dense, acts = mlp_forward(rt, xg, B, 33, True, host, dev, step_dev=ctr)
        step = DR.add_steps(host, devc)
        assert step == (host + devc) % (1 << 32)
        check_forward(params, x, dims, False, p_drop, replica_masks(dims, False, p_drop, B, step), acts, dense, "split step")


@pytest.mark.parametrize("B", [37, 2049])
def test_mlp_scales_by_65536_over_the_rounded_threshold(B, dev):
    """p = 0.95: (1 - p) 65536 = 3276.8, thr 3277; a truncated 3276 leaves the masks alone at these sizes and moves every kept
    activation and gradient by 3e-4 of its value, three times MLP_BAR.  (At 0.3 and 0.5 rounding and truncation agree.)"""
    dims, p_drop, step = (7, 100, 33), 0.95, 3
    assert DR.drop_thr(p_drop) == 3277 and int((1 - float(np.float32(p_drop))) * 65536) == 3276
    rt, params, dp, grads, x = mlp_setup(dims, False, p_drop, B, dev)
    xg = x.to(dev)
    out, dense, acts = mlp_forward(rt, xg, B, 33, True, step, dev)
    kind = "mfma p 0.95" if B <= 2048 else "valu p 0.95"
    ref, leaves = check_forward(params, x, dims, False, p_drop, replica_masks(dims, False, p_drop, B, step), acts, dense, kind)
    gen = torch.Generator().manual_seed(9)
    d1, d2 = torch.randn(B, 3, 33, generator=gen), torch.randn(B, 33, generator=gen)
    rt.backward(xg, B, d1.to(dev), 3 * 33, d2.to(dev))
    torch.cuda.synchronize()
    check_backward(ref, leaves, grads, d1, d2, kind)
