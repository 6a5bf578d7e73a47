"""Writes tests/golden/gradblend.npz from the reference's modules/gradblend.py run on the CPU: the twelve loss sums and the three
normalised weights of GradBlend.get_weights() for the schedule of blend_cases.py (AV-MNIST S towers, dropout 0, 16 val + 48 / 40
train samples, batch 16, 10 epochs), in float32 and in float64 (same initial weights, models converted with .double()).  Data
only: the seed, sums, weights.  Parameters, inputs and sample orders are regenerated from the seed (gen_util, blend_cases).

The reference's models/*.py cannot be imported here (pytorch_lightning is absent): the three sub-models are composed from the
reference's `modules` package as make_golden.py composes them.  Model order image, audio, fusion (the model's own: the
reference's on_train_epoch_start hands [audio, image] over, so its multimodal copy concatenates the tokens in an order the
fusion mixer was not trained on -- DESIGN.md section 15).  Batches are tuples (image, audio, labels), device 'cpu', tqdm silenced.
Both loaders yield the stored order, except that the i-th pass over the train loader inside one model's training uses that
epoch's permutation (blend_cases.orders) -- every one of the three models sees the same schedule.

The generator searches seeds from 0 until, for BOTH train sizes and per model of the float64 run,
|G| >= 1e-2 N_val, |O| >= 5e-2 N_val and the three normalised weights are pairwise >= 0.1 apart -- so that w = |O / G^2| is
well conditioned and the weights' order means something.  Runs only where a reference checkout exists:

    python tests/golden/make_golden_gradblend.py /path/to/reference

The tests read only the committed .npz (tests/test_host_gradblend.py, tests/test_gpu_gradblend.py)."""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import blend_cases as BC  # noqa: E402


class Loader:
    """Tuple batches of BC.B rows over (image, audio, labels); pass i (counted per reset) uses schedule[i] (None: stored order)."""

    def __init__(self, tensors, schedule=None):
        self.tensors, self.schedule, self.passes = tensors, schedule, 0

    def __iter__(self):
        n = self.tensors[0].shape[0]
        order = None
        if self.schedule is not None:
            order = self.schedule[self.passes % len(self.schedule)]
        self.passes += 1
        for lo in range(0, n, BC.B):
            if order is None:
                yield tuple(t[lo:lo + BC.B] for t in self.tensors)
            else:
                yield tuple(t[order[lo:lo + BC.B]] for t in self.tensors)


def build(R, dtype):
    cfg = BC.CFG
    img = dict(cfg["image"], block_type="MLPMixer")
    aud = dict(cfg["audio"], block_type="MLPMixer")
    mm = dict(cfg["multimodal"], block_type="FusionMixer", fusion_function="ConcatFusion")
    cls = dict(num_classes=cfg["num_classes"], classifier="StandardClassifier", input_shape=[16, 49, cfg["multimodal"]["hidden_dim"]])
    m = torch.nn.Module()
    m.image_mixer = R.get_block_by_name(**img, dropout=0.0)
    m.audio_mixer = R.get_block_by_name(**aud, dropout=0.0)
    fusion = R.get_fusion_by_name(**mm)
    m.fusion_mixer = R.get_block_by_name(**mm, num_patches=fusion.get_output_shape(m.image_mixer.num_patch, m.audio_mixer.num_patch, dim=1),
                                         dropout=0.0)
    m.classifier_image = torch.nn.Linear(cfg["image"]["hidden_dim"], cfg["num_classes"])
    m.classifier_audio = torch.nn.Linear(cfg["audio"]["hidden_dim"], cfg["num_classes"])
    m.classifier_fusion = R.get_classifier_by_name(**cls)
    return m.to(dtype)


def run(R, GB, seed, ntrain, dtype):
    """(sums (3, 4) float64 in BC.HEADS x BC.SUMS order, weights (3,))."""
    m = build(R, dtype)
    sd = BC.params(seed)
    assert list(m.state_dict().keys()) == list(sd.keys())
    m.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
    m.train()
    image, audio, labels = BC.data(seed, ntrain)
    tensors = (image.to(dtype), audio.to(dtype), labels)
    val = Loader(tuple(t[:BC.NVAL] for t in tensors))
    schedule = [None] + BC.orders(seed, ntrain) + [None]         # probe, EPOCHS training passes, probe -- per model
    train = Loader(tuple(t[BC.NVAL:] for t in tensors), schedule)
    gb = GB.GradBlend(m, [m.image_mixer, m.audio_mixer], [m.classifier_image, m.classifier_audio], m.fusion_mixer,
                      m.classifier_fusion, torch.nn.CrossEntropyLoss, train, val, epochs=BC.EPOCHS)
    seen = []
    inner = gb.get_loss

    def recording(*a, **k):
        v = inner(*a, **k)
        seen.append(float(v.detach().double()))
        return v

    gb.get_loss = recording
    weights = gb.get_weights(device="cpu")
    assert len(seen) == 12 and train.passes == 3 * len(schedule)
    return np.asarray(seen, dtype=np.float64).reshape(3, 4), np.asarray(weights, dtype=np.float64)


def well_conditioned(sums, weights):
    for n_tr, n_va, nn_tr, nn_va in sums:
        o, g = (nn_va - nn_tr) - (n_va - n_tr), nn_va - n_va
        if abs(g) < 1e-2 * n_va or abs(o) < 5e-2 * n_va:
            return False
    gaps = [abs(weights[i] - weights[j]) for i in range(3) for j in range(i)]
    return min(gaps) >= 0.1


def main(ref_root: str):
    sys.path.insert(0, ref_root)
    import tqdm
    tqdm.tqdm = lambda it, *a, **k: it                 # silence the progress bars (modules/gradblend.py imports the name)
    import modules as R
    import modules.gradblend as GB
    torch.set_num_threads(8)
    for seed in range(64):
        runs = {n: run(R, GB, seed, n, torch.float64) for n in BC.TRAIN_SIZES}
        if all(well_conditioned(*r) for r in runs.values()):
            break
        print("seed", seed, "rejected")
    else:
        raise SystemExit("no seed in 0..63 meets the conditioning bounds")
    out = {"seed": np.int64(seed)}
    for n in BC.TRAIN_SIZES:
        s64, w64 = runs[n]
        assert well_conditioned(s64, w64)
        s32, w32 = run(R, GB, seed, n, torch.float32)
        out[f"n{n}.f64.sums"], out[f"n{n}.f64.weights"] = s64, w64
        out[f"n{n}.f32.sums"], out[f"n{n}.f32.weights"] = s32, w32
        print(f"seed {seed} n {n}: weights {w64}, fp32 - fp64 sums rel {np.abs(s32 / s64 - 1).max():.2e}, weights {np.abs(w32 - w64).max():.2e}")
    # an .npz with fixed member timestamps (numpy.savez stamps the current time): the same bytes on every run
    with zipfile.ZipFile(os.path.join(HERE, "gradblend.npz"), "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("M2M_REFERENCE", "../reference"))
