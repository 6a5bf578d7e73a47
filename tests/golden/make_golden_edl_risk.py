"""Writes tests/golden/edl_risk.npz from the reference's modules/losses.py (loaded by file path; it needs only torch): values and
gradients with respect to the logits of
    ce    EDLCELoss(K, 10)(logits, labels, epoch)                                  (modules/losses.py:71-93)
    kl    kl_divergence_loss(relu(logits), one_hot(labels)), the module function   (:52-68)
    klm   EDLMSELoss(K, 10).kl_divergence_loss(...), the method copy of it         (:33-49)
    mse   EDLMSELoss(K, 10).squared_error_bayes_risk(...)                          (:24-31)
in float32 and in float64, at epoch_num 0, 3 and 50 (only `ce` is handed the epoch; it computes the annealing coefficient and does
not use it: the stored results show that).  Cases: (B, K) in (1, 2), (5, 10), (9, 32) with logits 2 N(0, 1), and (5, 10), (9, 32)
again with logits 50 N(0, 1), which takes digamma, trigamma and lgamma past x = 6 into their asymptotic range.  Every case has one
logit exactly 0 (relu'(0) = 0) and one row whose label class has no evidence (a negative logit at the label).
Data only: logits, labels, losses, gradients.  Runs only where a reference checkout exists:

    python tests/golden/make_golden_edl_risk.py /path/to/reference

The tests read only the committed .npz (tests/test_host_edl_risk.py)."""
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = ((1, 2, 2), (5, 10, 2), (9, 32, 2), (5, 10, 50), (9, 32, 50))          # (B, K, logit scale)
EPOCHS = (0, 3, 50)


def tag_of(B, K, scale):
    return f"B{B}K{K}" + ("" if scale == 2 else f"s{scale}")


def draw(B, K, scale):
    gen = torch.Generator().manual_seed(1000 * B + K + scale)
    logits = float(scale) * torch.randn(B, K, generator=gen, dtype=torch.float64)
    labels = torch.randint(0, K, (B,), generator=gen)
    logits[0, (int(labels[0]) + 1) % K] = 0.0                      # a logit exactly on the gate, off the label
    logits[B - 1, labels[B - 1]] = -logits[B - 1, labels[B - 1]].abs() - 0.5        # a label class without evidence
    return logits, labels


def main(ref_root: str):
    spec = importlib.util.spec_from_file_location("ref_losses", os.path.join(ref_root, "modules", "losses.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    out = {}
    for B, K, scale in CASES:
        logits, labels = draw(B, K, scale)
        tag = tag_of(B, K, scale)
        out[f"{tag}.logits"], out[f"{tag}.labels"] = logits.numpy(), labels.numpy()
        for epoch in EPOCHS:
            for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
                target = torch.eye(K, dtype=dtype)[labels]
                fns = {"ce": lambda z: M.EDLCELoss(K, 10)(z, labels, epoch),
                       "kl": lambda z: M.kl_divergence_loss(torch.relu(z), target),
                       "klm": lambda z: M.EDLMSELoss(K, 10).kl_divergence_loss(torch.relu(z), target),
                       "mse": lambda z: M.EDLMSELoss(K, 10).squared_error_bayes_risk(torch.relu(z), target)}
                for what, fn in fns.items():
                    z = logits.detach().to(dtype).clone().requires_grad_(True)
                    loss = fn(z)
                    loss.backward()
                    out[f"{tag}.e{epoch}.{name}.{what}.loss"] = loss.detach().numpy()
                    out[f"{tag}.e{epoch}.{name}.{what}.dlogits"] = z.grad.numpy()
    # an .npz with fixed member timestamps (numpy.savez stamps the current time): the same bytes on every run
    with zipfile.ZipFile(os.path.join(HERE, "edl_risk.npz"), "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("M2M_REFERENCE", "../reference"))
