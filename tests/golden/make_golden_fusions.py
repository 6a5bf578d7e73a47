"""Writes tests/golden/fusions.npz from the reference's modules/fusion.py (loaded by file path; it needs only torch):
float64 outputs and input gradients of SumFusion, MeanFusion and MaxFusion (with deliberate ties for max) and of
BiModalGatedUnit, whose parameter gradients are stored too.  Runs only where a reference checkout exists:

    python tests/golden/make_golden_fusions.py /path/to/reference

The tests read only the committed .npz (tests/test_host_fusions.py)."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref_root: str):
    spec = importlib.util.spec_from_file_location("ref_fusion", os.path.join(ref_root, "modules", "fusion.py"))
    F = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(F)
    torch.manual_seed(0)
    B, N, D = 3, 5, 8
    a = torch.randn(B, N, D, dtype=torch.float64)
    b = torch.randn(B, N, D, dtype=torch.float64)
    b[:, ::2, ::3] = a[:, ::2, ::3]                           # ties for MaxFusion
    dy = torch.randn(B, N, D, dtype=torch.float64)
    out = {"a": a.numpy(), "b": b.numpy(), "dy": dy.numpy()}
    for name in ("SumFusion", "MeanFusion", "MaxFusion"):
        x, y = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        f = getattr(F, name)()
        r = f(x, y)
        r.backward(dy)
        out[f"{name}.y"], out[f"{name}.da"], out[f"{name}.db"] = r.detach().numpy(), x.grad.numpy(), y.grad.numpy()
    gate = F.BiModalGatedUnit(D, D, D).double()
    x, y = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    r = gate(x, y)
    r.backward(dy)
    out["gate.y"], out["gate.da"], out["gate.db"] = r.detach().numpy(), x.grad.numpy(), y.grad.numpy()
    for k, p in gate.named_parameters():
        out[f"gate.fusion_function.{k}"] = p.detach().numpy()
        out[f"grad.fusion_function.{k}"] = p.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "fusions.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("M2M_REFERENCE", "../reference"))
