"""Writes tests/golden/edl.npz from the reference's modules/losses.py (loaded by file path; it needs only torch): the value of
EDLMSELoss and its gradient with respect to the logits, in float32 and in float64, for (B, K) in (1, 2), (5, 10), (9, 32) at
epoch_num 0, 3 and 50 -- the KL term is multiplied by annealing_coef * 0 (modules/losses.py:20), so the epoch changes nothing,
which the stored results show.  Data only: logits, labels, losses, gradients.  Runs only where a reference checkout exists:

    python tests/golden/make_golden_edl.py /path/to/reference

The tests read only the committed .npz (tests/test_host_edl.py)."""
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = ((1, 2), (5, 10), (9, 32))
EPOCHS = (0, 3, 50)


def main(ref_root: str):
    spec = importlib.util.spec_from_file_location("ref_losses", os.path.join(ref_root, "modules", "losses.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    out = {}
    for B, K in CASES:
        gen = torch.Generator().manual_seed(1000 * B + K)
        logits = 2.0 * torch.randn(B, K, generator=gen, dtype=torch.float64)
        logits[0, 0] = 0.0                                          # a logit exactly on the gate: relu'(0) = 0
        labels = torch.randint(0, K, (B,), generator=gen)
        tag = f"B{B}K{K}"
        out[f"{tag}.logits"], out[f"{tag}.labels"] = logits.numpy(), labels.numpy()
        for epoch in EPOCHS:
            for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
                z = logits.detach().to(dtype).clone().requires_grad_(True)
                loss = M.EDLMSELoss(K, 10)(z, labels, epoch)
                loss.backward()
                out[f"{tag}.e{epoch}.{name}.loss"] = loss.detach().numpy()
                out[f"{tag}.e{epoch}.{name}.dlogits"] = z.grad.numpy()
    # an .npz with fixed member timestamps (numpy.savez stamps the current time): the same bytes on every run
    with zipfile.ZipFile(os.path.join(HERE, "edl.npz"), "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("M2M_REFERENCE", "../reference"))
