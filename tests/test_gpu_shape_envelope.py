"""Shape envelope of the module path (-m gpu): every case of tests/shape_cases.py runs forward and backward in training mode,
in fp32 and in bf16, and is compared with the oracle evaluated in float64 on the CPU -- the output, dx and every parameter
gradient, each over the whole tensor and over its tail (the last sample / token, the last channel rows, the last token
column, the last k columns of an embedding), where masking and padding bugs land.

Bars: fp32 (exact MFMA) 1e-4 relative to the tensor's (or the tail slice's) max; bf16 the parity bars of
tests/test_gpu_parity.py (BF16_REL for outputs and dx, BF16_GRAD_REL for parameter gradients).  Dropout cases feed the
oracle the kernels' own keep-masks (TowerRuntime.dropout_mask).  Every error is recorded per path / precision / tensor
class (conftest.observe).
"""
import numpy as np
import pytest
import torch

import drop_ref as DR
import gen_util as G
from conftest import observe
from oracle import m2mixer_oracle as O
from shape_cases import CASES

pytestmark = pytest.mark.gpu

FP32_REL = 1e-4
BF16_REL = 2e-2
BF16_GRAD_REL = 4e-2
TAIL_CH = 32          # channel rows in a channel-mixing weight's tail
TAIL_K = 16           # embedding columns in the embedding weight's tail


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture
def precision():
    import m2_mixer_amd as M
    before = M.config.get_precision()
    yield M.set_precision
    M.set_precision(before)


def path_of(case):
    if case.kind == "mlp":
        return "mlp"
    return "wide" if case.N > 8 or case.D > 128 else "fused"


def tensor_class(key):
    if key.endswith("token_mix.0.weight") or key.endswith("token_mix.0.bias") or "channel_mix.0." in key or "layer_norm." in key:
        return "LN"
    if key.startswith("to_patch_embedding.") or key.startswith("proj."):
        return "embed W" if key.endswith("weight") else "embed bias"
    if key.endswith("bias"):
        return "bias"
    if "token_mix." in key:
        return "token W"
    if "channel_mix." in key:
        return "channel W"
    return "W"                 # MLP linears


def tail_of(key, t, case):
    """The slice of a parameter gradient where a tail bug lands (None: no tail beyond the whole tensor)."""
    if key.endswith("token_mix.2.net.0.weight"):        # (T, N): the last token's column
        return t[:, -1]
    if key.endswith("token_mix.2.net.3.weight"):        # (N, T): the last token's row
        return t[-1]
    if key.endswith("channel_mix.1.net.0.weight"):      # (C, D): the last channel rows
        return t[-TAIL_CH:]
    if key.endswith("channel_mix.1.net.0.bias"):
        return t[-TAIL_CH:]
    if key.endswith("channel_mix.1.net.3.weight"):      # (D, C)
        return t[:, -TAIL_CH:]
    if key.startswith("to_patch_embedding.0.weight") or key.startswith("proj.weight"):
        return t.reshape(t.shape[0], -1)[:, -TAIL_K:]    # (D, K): the last k columns
    return None


def rel(a, b, floor=0.0):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), floor, 1e-30)


def case_shapes(case):
    if case.kind == "mlp":
        i, h, nb, o = case.mlp
        s = {}
        for b in range(nb):
            s[f"module_list.{3 * b}.weight"] = (h, i if b == 0 else h)
            s[f"module_list.{3 * b}.bias"] = (h,)
        if o is not None:
            s[f"module_list.{3 * nb}.weight"] = (o, h)
            s[f"module_list.{3 * nb}.bias"] = (o,)
        return s
    if case.kind == "block":
        return G.block_shapes("", case.D, case.N, case.T, case.C)
    c = dict(hidden_dim=case.D, token_dim=case.T, channel_dim=case.C, num_mixers=case.nb)
    if case.kind == "fusion":
        return G.tower_shapes("", c, case.N, "none")
    if case.kind == "mixer":
        cin, _, patch = case.emb
        return G.tower_shapes("", dict(c, in_channels=cin, patch_size=patch), case.N, "patch")
    return G.tower_shapes("", dict(c, embedding_dim=case.emb, proj_dim=case.D), case.N, "proj")


def make_module(case):
    from m2_mixer_amd import modules as MM
    if case.kind == "block":
        return MM.MixerBlock(case.D, case.N, case.T, case.C, dropout=case.p)
    if case.kind == "fusion":
        return MM.FusionMixer(case.D, case.N, case.nb, case.T, case.C, dropout=case.p)
    if case.kind == "mixer":
        cin, hw, patch = case.emb
        m = MM.MLPMixer(cin, case.D, patch, list(hw), case.nb, case.T, case.C, dropout=case.p)
        assert m.num_patch == case.N
        return m
    if case.kind == "nopatch":
        return MM.MLPMixerNoPatching(case.D, case.N, case.nb, case.T, case.C, case.emb, case.D, dropout=case.p)
    i, h, nb, o = case.mlp
    return MM.MLP(i, h, nb, o, dropout=case.p)


def make_input(case, rng):
    if case.kind == "mlp":
        shape = (case.B, case.mlp[0])
    elif case.kind == "mixer":
        cin, (h, w), _ = case.emb
        shape = (case.B, cin, h, w)
    elif case.kind == "nopatch":
        shape = (case.B, case.N, case.emb)
    else:
        shape = (case.B, case.N, case.D)
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def kernel_masks(mod, case):
    """The keep-masks the kernels drew in the forward just run, per block, in the oracle's layout."""
    import m2_mixer_amd as M
    rt, B = mod._rts[0], case.B
    seed, step = M.config.dropout_seed(), mod._drop_step
    masks = []
    for b in range(rt.nblocks):
        m = {"tok_h": rt.dropout_mask(b, 0, B, seed, step).view(B, rt.D, rt.T),
             "tok_o": rt.dropout_mask(b, 1, B, seed, step).view(B, rt.D, rt.N),
             "ch_h": rt.dropout_mask(b, 2, B, seed, step).view(B, rt.N, rt.Cp)[:, :, :rt.C],
             "ch_o": rt.dropout_mask(b, 3, B, seed, step).view(B, rt.N, rt.D)}
        masks.append({k: v.double().cpu() for k, v in m.items()})
    return masks


def oracle(case, x, p, drop_p, masks):
    if case.kind == "mlp":
        return O.mlp(x, p, "", case.mlp[2], case.mlp[3] is not None)
    if case.kind == "block":
        return O.mixer_block(x, p, "", drop_p, None if masks is None else masks[0])
    if case.kind == "fusion":
        return O.fusion_mixer(x, p, "", case.nb, drop_p, masks)
    if case.kind == "mixer":
        return O.mlp_mixer(x, p, "", case.emb[2], case.nb, drop_p, masks)
    return O.mlp_mixer_no_patching(x, p, "", case.nb, drop_p, masks)


def run_case(case, prec, dev, seed=0, transform=None):
    """(module, params, x, dy, y, x_dev) after one training-mode forward + backward on the GPU.  transform: (params, x) ->
    (params, x) applied to the generated tensors first (tests/value_cases.py)."""
    params = G.make_params(case_shapes(case), 4242 + seed)
    rng = np.random.default_rng(977 + seed)
    x = make_input(case, rng)
    if transform is not None:
        params, x = transform(params, x)
    mod = make_module(case).to(dev)
    mod.load_state_dict(params)
    mod.train()
    xd = x.to(dev).requires_grad_(case.kind in ("block", "fusion"))
    y = mod(xd)
    dy = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32))
    (y * dy.to(dev)).sum().backward()
    torch.cuda.synchronize()
    return mod, params, x, dy, y, xd


def check(kind, got, ref, tol, floor=0.0):
    err = rel(got, ref, floor)
    observe(kind, err, tol)
    return err < tol, err


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_shape_envelope_vs_float64_oracle(case, prec, dev, precision):
    precision(prec)
    mod, params, x, dy, y, xd = run_case(case, prec, dev)
    drop_p, masks = 0.0, None
    if case.p > 0:
        thr = DR.drop_thr(case.p)
        drop_p = 1 - thr / 65536                 # the kernels' 16-bit keep probability
        masks = kernel_masks(mod, case)
    leaves = {k: v.double().requires_grad_(True) for k, v in params.items()}
    xr = x.double().requires_grad_(case.kind in ("block", "fusion"))
    yo = oracle(case, xr, leaves, drop_p, masks)
    (yo * dy.double()).sum().backward()

    path = path_of(case)
    act_tol = FP32_REL if prec == "fp32" else BF16_REL
    grad_tol = FP32_REL if prec == "fp32" else BF16_GRAD_REL
    bad = []

    def want(kind, got, ref, tol, what, floor=0.0):
        ok, err = check(kind, got, ref, tol, floor)
        if not ok:
            bad.append(f"{what}: {err:.3e} > {tol:.0e}")

    acts = [("out", y, yo)] + ([("dx", xd.grad, xr.grad)] if xr.grad is not None else [])
    for what, got, ref in acts:
        assert got is not None, what
        want(f"{path} {prec} {what} (rel to max)", got, ref, act_tol, what)
        if got.dim() == 3:
            want(f"{path} {prec} {what} tail (rel to slice max)", got[-1], ref[-1], act_tol, f"{what}[last sample]")
            want(f"{path} {prec} {what} tail (rel to slice max)", got[:, -1], ref[:, -1], act_tol, f"{what}[:, last token]")
        else:
            want(f"{path} {prec} {what} tail (rel to slice max)", got[-1], ref[-1], act_tol, f"{what}[last sample]")
    for k, prm in mod.named_parameters():
        assert prm.grad is not None, k
        ref = leaves[k].grad
        cls = tensor_class(k)
        kpath = "embed" if cls.startswith("embed") else path
        floor = 0.0
        if k.endswith("token_mix.2.net.3.bias"):
            # in a tower that ends in a LayerNorm the token-mixing output bias shifts a whole token row, which every later
            # LayerNorm removes: its true gradient is exactly zero, so it is measured against its weight's gradient scale
            floor = float(leaves[k[:-4] + "weight"].grad.abs().max())
            if float(ref.abs().max()) > 1e-6 * floor:
                floor = 0.0
        want(f"{kpath} {prec} {cls} (rel to max)", prm.grad, ref, grad_tol, k, floor)
        tg, tr = tail_of(k, prm.grad, case), tail_of(k, ref, case)
        if tg is not None:
            want(f"{kpath} {prec} {cls} tail (rel to slice max)", tg, tr, grad_tol, f"{k}[tail]", floor)
    assert not bad, f"{case.name} [{prec}]: " + "; ".join(bad)
