"""The Gradient-Blending fixture's schedule, shared by make_golden_gradblend.py (which feeds the reference) and the tests:
AV-MNIST S towers without dropout, 16 val samples followed by 48 (or 40: a ragged tail of 8) train samples, batch 16, 10
retraining epochs.  Everything derives from one seed (gen_util generators): parameters, data, the per-epoch sample orders."""
import numpy as np
import torch

import gen_util as G

CFG = dict(G.AVMNIST["S"], dropout=0.0)
B, NVAL, EPOCHS = 16, 16, 10
TRAIN_SIZES = (48, 40)
HEADS = ("image", "audio", "fusion")                    # the model's own order
SUMS = ("n_train", "n_val", "nn_train", "nn_val")


def val_fraction(ntrain: int) -> float:
    """A fraction f with int((NVAL + ntrain) * f) == NVAL, safely inside the integer step."""
    return (NVAL + 0.5) / (NVAL + ntrain)


def params(seed: int):
    return G.make_params(G.avmnist_shapes(CFG), seed)


def data(seed: int, ntrain: int):
    """(image, audio, labels) of NVAL + ntrain samples: uniform inputs, random labels; the first NVAL rows are the val part."""
    return G.avmnist_batch(NVAL + ntrain, seed + 1000, CFG)


def orders(seed: int, ntrain: int):
    """One permutation of the train part per retraining epoch (int64 tensors)."""
    return [torch.from_numpy(np.random.default_rng(seed + 2000 + e).permutation(ntrain).astype(np.int64)) for e in range(EPOCHS)]
