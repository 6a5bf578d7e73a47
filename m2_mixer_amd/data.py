"""Resident-in-HBM input pipeline and the epoch loop around the fused engines.

The reference feeds the model through a torch DataLoader with `num_workers: 2` (datasets/avmnist.py:163-190) and pulls
`loss.cpu().item()` to the host every step (modules/train_test_module.py:72-84).  At > 600 k samples/s neither survives:
the whole AV-MNIST training split is 55 000 x 53 KB = 2.9 GB in fp32, a rounding error of one MI355X's 288 GB, so it
is loaded ONCE into device memory in the reference's on-disk format and batches are views (train / val: `shuffle=False`
in the reference) or one device-side gather (test: `shuffle=True`); per-step losses and hit counts accumulate in device
memory and reach the host once per `log_interval_steps`, so the captured graph is never interrupted by a sync.
"""
from __future__ import annotations

import os
from contextlib import contextmanager, nullcontext
from typing import Dict, Iterator, Optional, Sequence, Tuple

import numpy as np
import torch

from .accumulators import pass_accumulators


class ResidentAVMnist:
    """`root/{image,audio}/{train,test}_data.npy`, `root/{train,test}_labels.npy` (datasets/avmnist.py:105-114):
    image (N, 784) or (N, 28, 28) -> (N, 1, 28, 28); audio (N, 112, 112) -> (N, 1, 112, 112); `astype(float32)` only
    (datasets/avmnist.py:17-21).  Splits as AVMnistDataModule.setup (:175-181): the first 55 000 training samples train,
    the rest validate; smaller sets (tests, subsets) keep the 11 : 1 proportion."""

    TRAIN_SPLIT = 55000

    def __init__(self, root_dir: str, device="cuda:0", rank: int = 0, world: int = 1):
        self.device = torch.device(device)
        self.rank, self.world = rank, world
        self.splits: Dict[str, Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}
        tr = self._load(root_dir, "train")
        n = tr[2].shape[0]
        cut = self.TRAIN_SPLIT if n > self.TRAIN_SPLIT else (n * 11) // 12
        self.splits["train"] = tuple(t[:cut] for t in tr)
        self.splits["val"] = tuple(t[cut:] for t in tr)
        if os.path.exists(os.path.join(root_dir, "test_labels.npy")):
            self.splits["test"] = self._load(root_dir, "test")

    def _load(self, root: str, stage: str):
        image = np.load(os.path.join(root, "image", f"{stage}_data.npy"))
        audio = np.load(os.path.join(root, "audio", f"{stage}_data.npy"))
        labels = np.load(os.path.join(root, f"{stage}_labels.npy"))
        if image.shape[0] != audio.shape[0] or image.shape[0] != labels.shape[0]:
            raise ValueError(f"{stage}: image / audio / label counts differ")
        image = torch.from_numpy(image.astype(np.float32)).reshape(image.shape[0], 1, 28, 28)
        audio = torch.from_numpy(audio.astype(np.float32))[:, None, :, :]
        labels = torch.from_numpy(labels.astype(np.int64))
        return image.to(self.device), audio.to(self.device), labels.to(self.device)

    def num_samples(self, split: str) -> int:
        """Samples of `split` this rank sees.  As torch's DistributedSampler(drop_last=False) -- what Lightning puts in
        front of the reference's loaders under DDP (datasets/avmnist.py:180-190, run.py:69-70) -- EVERY rank gets
        ceil(n / world): the index list is padded with its own head until it divides evenly, then rank r takes
        r, r + world, ...  Equal counts are what keeps the ranks' collectives in step (an epoch is the same number of
        batches, of the same sizes, on every rank)."""
        n = self.splits[split][2].shape[0]
        return (n + self.world - 1) // self.world

    def num_batches(self, split: str, batch_size: int, drop_last: bool = False) -> int:
        """The reference's DataLoaders keep the ragged last batch (`drop_last` is left False, datasets/avmnist.py:180-190)."""
        n = self.num_samples(split)
        return n // batch_size if drop_last else (n + batch_size - 1) // batch_size

    def batches(self, split: str, batch_size: int, shuffle: bool = False, generator: Optional[torch.Generator] = None,
                drop_last: bool = False) -> Iterator[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
        """Rank r takes samples r, r + world, ... of the padded index list (see num_samples: DistributedSampler semantics;
        under `shuffle` every rank must pass a generator in the same state).  The last batch may be smaller than batch_size
        (drop_last=False, as the reference)."""
        image, audio, labels = self.splits[split]
        n = labels.shape[0]
        if shuffle:
            order = torch.randperm(n, device=self.device, generator=generator)
        elif self.world > 1:
            order = torch.arange(n, device=self.device)
        else:
            order = None
        if order is not None and self.world > 1:
            pad = self.num_samples(split) * self.world - n
            if pad:
                order = torch.cat([order, order[:pad]])         # (n >= world: one wrap-around suffices)
            order = order[self.rank::self.world]
        mine = self.num_samples(split)
        for b in range(self.num_batches(split, batch_size, drop_last)):
            lo, hi = b * batch_size, min((b + 1) * batch_size, mine)
            if order is None:
                yield image[lo:hi], audio[lo:hi], labels[lo:hi]          # views: zero copies
            else:
                idx = order[lo:hi]
                yield image.index_select(0, idx), audio.index_select(0, idx), labels.index_select(0, idx)


class ResidentTensors:
    """Any task's splits resident in device memory: split name -> the tensors of the engine's batch, in its order (AV-MNIST:
    image, audio, labels; MIMIC: static, time, labels; MM-IMDb: image, text, targets), all with the same number of rows.
    ResidentAVMnist has the same `splits` / `device` and serves wherever one of these is taken.  (Loaders for MIMIC's im.pk and
    MM-IMDb's files are out of scope: build the tensors, hand them in.)"""

    def __init__(self, splits: Dict[str, Tuple[torch.Tensor, ...]], device=None):
        self.splits: Dict[str, Tuple[torch.Tensor, ...]] = {}
        self.device = torch.device(device) if device is not None else next(iter(splits.values()))[0].device
        self.rank, self.world = 0, 1
        for name, tensors in splits.items():
            tensors = tuple(t.to(self.device).contiguous() for t in tensors)
            if not tensors or any(t.dim() < 1 or t.shape[0] != tensors[0].shape[0] for t in tensors):
                raise ValueError(f"{name}: every tensor of a split needs the same number of rows")
            self.splits[name] = tensors

    def num_samples(self, split: str) -> int:
        return int(self.splits[split][0].shape[0])

    def num_batches(self, split: str, batch_size: int, drop_last: bool = False) -> int:
        n = self.num_samples(split)
        return n // batch_size if drop_last else (n + batch_size - 1) // batch_size


class PlateauLR:
    """torch.optim.lr_scheduler.ReduceLROnPlateau(mode='min', factor=0.1, threshold=1e-4 rel) on the engine's device-side
    learning rate (models/avmnist.py:416-422: monitor `val_loss`, patience from `scheduler_patience`)."""

    def __init__(self, engine, lr: float, patience: int = 5, factor: float = 0.1, threshold: float = 1e-4, min_lr: float = 0.0):
        self.engine, self.lr, self.patience, self.factor, self.threshold, self.min_lr = engine, lr, patience, factor, threshold, min_lr
        self.best, self.bad = float("inf"), 0

    def step(self, metric: float) -> float:
        if metric < self.best * (1 - self.threshold):
            self.best, self.bad = metric, 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            self.lr = max(self.lr * self.factor, self.min_lr)
            self.engine.set_lr(self.lr)
            self.bad = 0
        return self.lr


def tail_engine_for(engine, rows: int, trains: bool = True, given=None, reuse: Optional[bool] = None, keep: Optional[dict] = None):
    """The engine that takes a batch of `rows` rows beside `engine` (the ragged last batch of a split): `given` if there is one,
    else the kept training sibling of that size (engine._tail_engines), else a new engine.sibling(rows, trains=trains) -- kept
    there only if it trains: an evaluating sibling is never kept as the training one.
    reuse: whether the kept training sibling may serve (default: a training step only; run_epoch also evaluates on it).
    keep: a dict of the caller's in which an EVALUATING sibling is found and kept (GradBlend's probing passes)."""
    if given is not None:
        return given
    found = engine._tail_engines.get(rows) if (trains if reuse is None else reuse) else None
    if found is None and not trains and keep is not None:
        found = keep.get(rows)
    if found is None:
        found = engine.sibling(rows, trains=trains)
        if trains:
            engine._tail_engines[rows] = found
        elif keep is not None:
            keep[rows] = found
    return found


@contextmanager
def tail_step(engine, tail, trains: bool):
    """Around one step of `tail` (tail_engine_for) on weights it shares with `engine`: its packed operand copies missed every step
    since its last use -- pack() before; a training step changed the weights under the parent's copies -- engine.pack() after."""
    tail.pack()
    yield tail
    if trains:
        engine.pack()


def prepare_tail_engine(engine, data: "ResidentAVMnist", split: str, batch_size: int):
    """The training engine of `split`'s ragged last batch, built NOW (before engine.capture()) and kept on the engine for
    run_epoch; None when the split divides evenly."""
    rem = data.num_samples(split) % batch_size
    return tail_engine_for(engine, rem) if rem else None


def epoch_metrics(heads: Sequence[str], loss_sums, weighted_loss, steps: int, samples: int, hits=None, unc=None) -> Dict[str, float]:
    """The metrics dict of one pass (run_epoch's docstring names the keys).  heads: the two modality names; loss_sums: the step
    losses [a, b, fusion, total] summed over the steps; weighted_loss: the total weighted by each step's batch size; hits:
    [a, b, fusion] correct predictions, or None (multilabel predictions have no hit count); unc: [a, b, fusion] sums of the
    steps' batch-mean uncertainties, or None."""
    a, b = heads
    ds, dn = max(steps, 1), max(samples, 1)
    out = {"loss": float(weighted_loss) / dn, "loss_step_mean": float(loss_sums[3]) / ds, f"loss_{a}": float(loss_sums[0]) / ds,
           f"loss_{b}": float(loss_sums[1]) / ds, "loss_fusion": float(loss_sums[2]) / ds, "steps": steps, "samples": samples}
    if hits is not None:
        ha, hb, hf = (int(round(float(h))) for h in hits)
        out.update({"acc": float(hits[2]) / dn, f"acc_{a}": float(hits[0]) / dn, f"acc_{b}": float(hits[1]) / dn,
                    "hits": hf, f"hits_{a}": ha, f"hits_{b}": hb})
    if unc is not None:
        # the mean over the steps of each step's batch mean, the ragged tail as one step (models/avmnist.py:556-572); the plain
        # name is the fusion head's
        out.update({"uncertainty": float(unc[2]) / ds, f"uncertainty_{a}": float(unc[0]) / ds, f"uncertainty_{b}": float(unc[1]) / ds})
    return out


def run_epoch(engine, data: ResidentAVMnist, split: str, batch_size: int, train: bool, log_interval_steps: int = 50,
              replay=None, log=None, tail_engine=None, grad_sync=None, epoch: int = 0, shuffle_seed: int = 0) -> Dict[str, float]:
    """One pass over EVERY sample of `split` (the reference's loaders keep the ragged last batch,
    datasets/avmnist.py:180-190).  train=True drives the captured step (`replay`, from engine.capture) or
    engine.train_step.  A last batch smaller than batch_size -- the captured graph and the engine's buffers have a static
    batch size -- goes through `tail_engine` (default: engine.sibling(remainder), same parameters / Adam state, built on
    first use and kept on the engine), eagerly; packed operand copies are re-synchronised around it.
    A TRAINING tail engine must exist before engine.capture() (engine.sibling narrows the gradient ranges the captured
    optimizer leaves uncleared and refuses to do so under a captured graph): prepare_tail_engine(engine, data, split, batch).
    Data parallel (world > 1): the test split is shuffled (as the reference's loader) with a generator seeded `shuffle_seed +
    epoch` on EVERY rank (torch's DistributedSampler does the same), so the ranks' strided shards partition one permutation.
    Pass the `grad_sync` the replay was captured with -- EVERY training step exchanges gradients,
    the eager ones (no replay, the ragged last batch) included, as Lightning's DDP does; the ranks see equally many samples
    (ResidentAVMnist.num_samples), hence the same sequence of collectives.  Returned metrics are this rank's (the reference
    logs without sync_dist).

    Per-step values are summed on the device and read back every `log_interval_steps` steps and at the end (cfg
    `log_interval_steps`, cfg/avmnist/*.yml:3): the four losses (modules/train_test_module.py:72-92: step losses), the three
    heads' hit counts (torchmetrics Accuracy on `preds`, :79-82, :105-110).  Returned:
      loss              sample-weighted mean of the step losses = what `self.log('val_loss', ..., on_epoch=True)` reduces to,
                        the quantity ReduceLROnPlateau / EarlyStopping monitor (run.py:61-67, models/avmnist.py:416-422)
      loss_step_mean    plain mean over steps = the wandb `val_loss` / `train_loss` number (train_test_module.py:92, :113)
      loss_image / loss_audio / loss_fusion   step means (models/avmnist.py:326-337)
      acc, acc_image, acc_audio, hits*, steps, samples
    An engine built with scores=True also counts the pass into its table of `split` (engine.score_table: cleared here at the
    start, read once at the end -- it stays readable until the next pass over the split) and the reference's scores derived
    from it are added under their own names (`f1m`, `prec_m`, `rec_m`, ..., `f1m_image`, ...: scores.TASK_SCORES); the keys
    above keep their values -- the table's `acc` is the same quotient as the hit count's.
    An engine built with rank_scores=True also appends the pass to its ranking buffer of `split` (engine.rank_buffer: emptied
    here at the start, counted once at the end) and the ranking scores are added under their own names (`ap_macro`,
    `roc_auc_macro`, `ap_macro_image`, ...: scores.RANK_SCORES); the split must fit the engine's rank_capacity."""
    dev = engine.device
    accs = pass_accumulators(engine, split, train)
    accs.reset()
    # [loss_a, loss_b, loss_fusion, loss] step sums | the same weighted by the step's batch size | hits a, b, fusion
    acc = torch.zeros(11, device=dev, dtype=torch.float64)
    seen, host = 0, np.zeros(11)
    if train and grad_sync is None and getattr(data, "world", 1) > 1:
        raise RuntimeError("run_epoch: world > 1 needs the gradient exchange (grad_sync=parallel.GradSync(...))")
    nb = data.num_batches(split, batch_size)
    shuffle, gen = split == "test", None
    if shuffle and getattr(data, "world", 1) > 1:
        gen = torch.Generator(device=data.device)
        gen.manual_seed(int(shuffle_seed) + int(epoch))

    def step(eng, *batch):
        if not train:
            eng.evaluate(*batch, **accs.kwargs())
        elif replay is not None and eng is engine:
            replay(*batch)
        else:
            eng.train_step(*batch, grad_sync=grad_sync)

    for i, (image, audio, labels) in enumerate(data.batches(split, batch_size, shuffle=shuffle, generator=gen)):
        bs = labels.shape[0]
        eng = engine
        if bs == batch_size:
            step(engine, image, audio, labels)
        else:                                                      # the ragged last batch (a kept training sibling evaluates too)
            eng = tail_engine_for(engine, bs, train, tail_engine, reuse=True)
            with tail_step(engine, eng, train):
                step(eng, image.contiguous(), audio.contiguous(), labels.contiguous())
        acc[:4] += eng.losses                                      # device-side: no host round trip
        acc[4:8] += eng.losses * bs
        acc[8:11] += (eng.preds == labels.to(eng.preds.dtype)[None, :]).sum(dim=1)
        seen += bs
        if (i + 1) % log_interval_steps == 0 or i + 1 == nb:
            host = acc.cpu().numpy()                               # the only sync of the interval
            if log is not None:
                log({"split": split, "step": i + 1, "loss": host[3] / (i + 1), "acc": host[10] / seen})
    out = accs.compute()
    out.update(epoch_metrics(getattr(engine, "MODS", ("image", "audio")), host[:4], host[7], nb, seen, hits=host[8:11]))
    return out


def feed_plan(n: int, batch_size: int, steps: int, drop_last: bool = False) -> Tuple[int, int, int]:
    """How a fed epoch over n samples runs: (replays of the `steps`-step graph, full batches left for single steps, rows of the
    ragged tail -- 0 under drop_last).  Pure host arithmetic."""
    if n < 0 or batch_size < 1 or steps < 1:
        raise ValueError("feed_plan: n >= 0, batch_size >= 1, steps >= 1")
    full = n // batch_size
    return full // steps, full % steps, 0 if drop_last else n % batch_size


def run_epoch_fed(engine, feed, replay, n: Optional[int] = None, train: bool = True, tail_engine=None, drop_last: bool = False,
                  order=None, split: str = "train", muting=None, probe: bool = False, record=None) -> Dict[str, float]:
    """run_epoch with the batches fetched on the device (engine.EpochFeed): one pass over the first `n`
    samples (default: all) of `order` (an index tensor for feed.start; None: the split's own order), every sample exactly once,
    in order.  Any of the engines; single GPU.

    train=True: `replay` is engine.capture_feed(feed, steps).  feed_plan(n, B, steps) replays of the graph, then the full
    batches that do not fill a graph one at a time, eagerly (feed.gather_into + train_step + feed.accumulate on the graph's
    first slots), then the ragged tail through `tail_engine` (default: the engine's kept training sibling of that size, which
    must exist before the capture -- prepare_tail_engine's rule -- or engine.sibling(tail)), fed by gather_into, with pack()
    before and after, as run_epoch does.  Nothing is read back until the end.
    train=False: `replay` None: every batch is gathered eagerly, evaluated and accumulated.  `replay` from
    engine.capture_feed_eval(feed, steps, scores=, rank=, record=): feed_plan(n, B, steps) replays of the graph, then the full batches
    that do not fill a graph one at a time, eagerly, on the graph's first slots, then the ragged tail through an evaluating sibling
    -- all into the same table, ranking buffer and record.  The graph must have been captured on this feed and with the table, the
    ranking buffer and the record this pass uses (the engine's own of `split`, and `record`): anything else is refused by name.  A
    training graph is refused in an evaluation pass, and an evaluation graph in a training pass.
    record (train=False): an engine.PredictionRecord (engine.prediction_record(split, capacity)) every evaluated batch is appended
    to; emptied here at the start, left for the caller to read().
    probe=True (with train=False): engine.probe in place of engine.evaluate -- the training-mode forward (dropout on, the stage's
    training coefficients) that updates nothing: GradBlend's loss sums (modules/gradblend.py:43-60).  Score tables and ranking
    buffers are not fed by a probing pass.
    muting (train=True, a feed built with muting=True): the epoch's muting codes, one per training step (models.muting_codes),
    handed to feed.start; evaluation never mutes (its schedule is all zeros).

    Returns run_epoch's keys from feed.read(): loss, loss_step_mean, the per-head losses, steps, samples and -- for engines whose
    predictions are classes -- acc*, hits*; the score table's and ranking buffer's numbers (scores=True / rank_scores=True) are
    merged in as run_epoch does, under the table of `split`.  A feed built with uncertainty=True (the evidential engine) adds
    uncertainty, uncertainty_<a>, uncertainty_<b>: the epoch means of the steps' batch-mean uncertainties.  Ends with feed.check():
    a pass that ran beyond the order raises."""
    n = feed.n if n is None else int(n)
    B = feed.B
    if not 0 <= n <= feed.n:
        raise ValueError(f"run_epoch_fed: n = {n} samples of a split of {feed.n}")
    if B != engine.B:
        raise ValueError(f"run_epoch_fed: the feed's batch size {B} is not the engine's {engine.B}")
    accs = pass_accumulators(engine, split, train, record)
    if record is not None and (train or probe):
        raise ValueError("run_epoch_fed: record= goes with an evaluating pass (train=False, probe=False)")
    feed.bind(engine)
    if muting is not None and not train:
        raise ValueError("run_epoch_fed: evaluation never mutes (muting= goes with train=True)")
    if probe and train:
        raise ValueError("run_epoch_fed: probe=True goes with train=False (a probing pass updates nothing)")
    if replay is not None:
        if bool(getattr(replay, "eval", False)) == train:
            kinds = ("a training graph (engine.capture_feed)", "an evaluation graph (engine.capture_feed_eval)")
            raise ValueError(f"run_epoch_fed: train={train} takes {kinds[not train]}; `replay` is {kinds[train]}")
        if probe:
            raise ValueError("run_epoch_fed: a probing pass runs eagerly (replay=None)")
        if replay.feed is not feed:
            raise ValueError("run_epoch_fed: `replay` was captured on another feed")
        if not train:
            for name, mine in accs._asdict().items():
                if getattr(replay, name) is not mine:
                    raise ValueError(f"run_epoch_fed: `replay` was captured with another {name} than this pass uses "
                                     f"(capture_feed_eval(..., {name}=) against the pass's own: None where it has none)")
    accs.reset()
    feed.start(order, muting=muting)
    # one step, whatever the pass: the graph's replays, the full batches that fill none on its first slots, the ragged tail
    kind = "train_step" if train else ("probe" if probe else "evaluate")
    kwargs = accs.kwargs() if kind == "evaluate" else {}

    def fed_step(eng, slots, around=nullcontext()):
        with around:
            feed.gather_into(slots)
            getattr(eng, kind)(*slots, **kwargs)
        feed.accumulate(eng, slots[-1])

    replays, singles, tail = feed_plan(n, B, replay.steps if replay is not None else 1, drop_last)
    if replay is None:
        replays, singles = 0, replays                              # (a graph of one step: every full batch is a single step)
    for _ in range(replays):
        replay()
    slots = replay.slots[0] if replay is not None else feed.new_slots()
    for _ in range(singles):
        fed_step(engine, slots)
    if tail:
        sib = tail_engine_for(engine, tail, train, tail_engine)
        fed_step(sib, feed.new_slots(tail), tail_step(engine, sib, train))
    unc = None
    if feed.nunc:
        sums, counts, unc = feed.read(with_uncertainty=True)       # the only sync of the epoch
    else:
        sums, counts = feed.read()
    feed.check()
    nl, nh = feed.nloss, feed.nheads
    out = accs.compute()
    # heads: (image, audio) / (image, text) / (static, time); multilabel predictions have no hit count (nh == 0)
    out.update(epoch_metrics(engine.HEAD_NAMES[:2], sums[:4], sums[nl + 3], int(counts[nh]), int(counts[nh + 1]),
                             hits=counts[:3] if nh == 3 else None, unc=unc))
    return out
