"""Gradient-Blending loss weights (the reference's modules/gradblend.py) on the fused engines.

The reference retrains three deep copies of the current weights -- each modality tower with its head, and the fusion mixer
over frozen towers with the fusion head -- for `epochs` passes over 90 % of the training split, sums the batch-mean losses
over that part ("train") and over the first 10 % ("val") before and after, and turns the four sums of each model into a
weight (gradblend.py:85-90), normalised over the three (:107-108).  Here

  * clone A (engine.clone) enters the modalities-only stage (engine.train_modalities_only) and trains BOTH unimodal models
    at once: they share no parameter and Adam is element-wise, so this is the reference's two separate trainings;
  * clone B enters stage two (engine.freeze_modalities): the reference's frozen-tower multimodal model;
  * the sums before training come from one probing pass (engine.probe: training mode, nothing updated) of the unchanged
    weights, the sums after from one probing pass of each clone;
  * every pass runs through EpochFeed: training through capture_feed + run_epoch_fed, the ragged tail through the kept
    sibling, the sums are feed.read()'s raw per-head sums (float64 on the device).

Deviations from the reference, both deliberate: its batches are indexed as tuples (`batch[m]`, `batch[-1]`) where its AV-MNIST
dataset yields dicts -- here the batch is the engine's; and it hands the encoders over as [audio, image], so its multimodal copy
concatenates [audio; image], which is not the order the fusion mixer was trained on -- here the model's own order is used (as
stage two does) and the weights are returned by head name; the task module maps them into the reference's list order."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

SUM_KEYS = ("n_train", "n_val", "nn_train", "nn_val")


def blend_weight(n_train: float, n_val: float, nn_train: float, nn_val: float) -> float:
    """gradblend.py:85-90 from the four loss sums of one model (N: before its training, Nn: after): the change of the
    overfitting O = (Nn_val - Nn_train) - (N_val - N_train), the generalisation G = Nn_val - N_val, w = |O / G^2|.  float64 host
    arithmetic in the reference's order of operations."""
    on = float(n_val) - float(n_train)
    onn = float(nn_val) - float(nn_train)
    o = onn - on
    g = float(nn_val) - float(n_val)
    return abs(o / (g ** 2))


def normalise(ws: Sequence[float]) -> List[float]:
    """gradblend.py:107-108: every weight over their sum (Python's sum: left to right from 0)."""
    z = sum(float(w) for w in ws)
    return [float(w) / z for w in ws]


class GradBlend:
    """engine: a ConcatFusion AVMnistEngine / MMIMDBEngine / MimicEngine (left untouched: all work happens on clones);
    data: anything with `.splits[split]`, the engine's batch tensors resident on its device (data.ResidentTensors,
    data.ResidentAVMnist); the first int(n * val_fraction) rows are "val", the rest "train" (models/avmnist.py:224-229).
    epochs, lr: the retraining (gradblend.py:27, :65: Adam's defaults -- betas (0.9, 0.999), eps 1e-8, no weight decay).
    seed: the generator of the training epochs' sample orders (torch.randperm per epoch).
    orders: explicit orders instead, one index tensor over the train part per epoch (tests).  Probing passes read both parts in
    their stored order."""

    def __init__(self, engine, data, split: str = "train", val_fraction: float = 0.1, epochs: int = 20, lr: float = 1e-3,
                 seed: int = 0, orders: Optional[Sequence] = None):
        from .engine import AVMnistUQEngine
        if isinstance(engine, AVMnistUQEngine):
            raise NotImplementedError("GradBlend: the evidential model (AVMnistUQEngine) is not covered: the reference's GradBlend "
                                      "retrains with one criterion class on plain logits (models/avmnist.py:230-232)")
        if not getattr(engine, "concat", True):
            raise NotImplementedError(f"GradBlend: multimodal.fusion_function = {engine.fusion_name}: the reference's multimodal copy "
                                      "concatenates the towers' tokens (gradblend.py:15-21); only ConcatFusion is covered")
        self.engine, self.data, self.split = engine, data, split
        self.val_fraction, self.epochs, self.lr, self.seed = float(val_fraction), int(epochs), float(lr), int(seed)
        if self.epochs < 0:
            raise ValueError("GradBlend: epochs >= 0")
        if orders is not None and len(orders) != self.epochs:
            raise ValueError(f"GradBlend: {self.epochs} epochs need {self.epochs} orders, got {len(orders)}")
        self.orders = orders
        self.sums: Dict[str, Dict[str, float]] = {}
        self.weights: Dict[str, float] = {}

    # ---- pieces ----------------------------------------------------------------------------------------------
    def _parts(self):
        src = self.data.splits[self.split]
        n = int(src[0].shape[0])
        nv = int(n * self.val_fraction)
        B = self.engine.B
        if nv < 1 or n - nv < B:
            raise ValueError(f"GradBlend: {n} samples at val_fraction {self.val_fraction} give {nv} val / {n - nv} train rows; it needs "
                             f"at least one val row and one full training batch of {B}")
        return tuple(t[:nv].contiguous() for t in src), tuple(t[nv:].contiguous() for t in src)

    def _clone(self):
        c = self.engine.clone()
        c.set_lr(self.lr)
        c.betas, c.eps, c.weight_decay = (0.9, 0.999), 1e-8, 0.0        # a fresh torch.optim.Adam(params) (gradblend.py:65)
        return c

    @staticmethod
    def _probe_sums(eng, feed, tails: dict):
        """tails: the clone's evaluating siblings, one per tail size, kept for its later passes."""
        from .data import run_epoch_fed, tail_engine_for
        tail = feed.n % eng.B
        run_epoch_fed(eng, feed, None, train=False, probe=True,
                      tail_engine=tail_engine_for(eng, tail, trains=False, keep=tails) if tail else None)
        return [float(v) for v in feed.read()[0][:3]]

    def _train(self, eng, feed):
        """`epochs` passes over the train part: the captured fed step, the ragged tail through the kept training sibling (built
        before the capture: sibling()'s rule)."""
        import torch
        from .data import run_epoch_fed, tail_engine_for
        if feed.n % eng.B:
            tail_engine_for(eng, feed.n % eng.B)
        replay = eng.capture_feed(feed, 1)
        gen = torch.Generator(device=eng.device)
        gen.manual_seed(self.seed)
        for e in range(self.epochs):
            order = self.orders[e] if self.orders is not None else torch.randperm(feed.n, device=eng.device, generator=gen)
            run_epoch_fed(eng, feed, replay, order=order)

    # ---- the weights -----------------------------------------------------------------------------------------
    def get_weights(self) -> Dict[str, float]:
        """{head name: normalised weight} in the engine's head order (HEAD_NAMES); the twelve sums they come from are kept in
        `self.sums` ({head: {"n_train", "n_val", "nn_train", "nn_val"}}).  The engine itself is not touched."""
        from .engine import EpochFeed
        eng = self.engine
        names = eng.HEAD_NAMES
        val, train = self._parts()
        dev, B = eng.device, eng.B
        uni, tails = self._clone(), {}                    # clone A
        feed_tr, feed_va = EpochFeed(train, B, dev), EpochFeed(val, B, dev)
        # before training: one probing pass of the unchanged weights gives all three heads' sums
        n_tr, n_va = self._probe_sums(uni, feed_tr, tails), self._probe_sums(uni, feed_va, tails)
        uni.train_modalities_only()
        self._train(uni, feed_tr)
        u_tr, u_va = self._probe_sums(uni, feed_tr, tails), self._probe_sums(uni, feed_va, tails)
        del uni, tails
        multi, tails = self._clone(), {}                  # clone B
        multi.freeze_modalities()
        feed_tr, feed_va = EpochFeed(train, B, dev), EpochFeed(val, B, dev)
        self._train(multi, feed_tr)
        m_tr, m_va = self._probe_sums(multi, feed_tr, tails), self._probe_sums(multi, feed_va, tails)
        del multi, tails
        after_tr, after_va = [u_tr[0], u_tr[1], m_tr[2]], [u_va[0], u_va[1], m_va[2]]
        self.sums = {h: dict(zip(SUM_KEYS, (n_tr[i], n_va[i], after_tr[i], after_va[i]))) for i, h in enumerate(names)}
        ws = normalise([blend_weight(*(self.sums[h][k] for k in SUM_KEYS)) for h in names])
        self.weights = dict(zip(names, ws))
        return dict(self.weights)

    __call__ = get_weights
