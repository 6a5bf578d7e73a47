"""Device-side accumulators of the fused engines (engine.py): what a step adds to beside its own work, read back once per epoch.
  ScoreTable   integer count table of one split (csrc/scores.hip)      -> accuracy / precision / recall / F1 (scores.py)
  RankBuffer   softmax rows and labels of one split (csrc/rank.hip)    -> average precision / ROC-AUC (scores.py)
  PredictionRecord  logits, predictions and labels of one split, row by row (csrc/record.hip) -> the reference's test_preds.pt
  PassAccumulators  the three above as one pass over a split uses them (pass_accumulators picks them)
  EpochFeed    one split's resident tensors behind a device-side order and cursor, with the epoch's loss sums and hit counts
               (csrc/feed.hip); engine.capture_feed captures steps that feed themselves from it
Of an engine they use `losses`, `logits`, `preds`, `uncertainty` and `B` only: this module imports the library (_lib) and scores,
never engine, which re-exports the classes.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib as L


class ScoreTable:
    """The count table of one split (train / val / test) in device memory: every step ADDS its batch's counts (csrc/scores.hip,
    one launch, capturable), the host reads it once per epoch and derives the reference's scores in float64 (scores.py).
    kind "multiclass": per head a (K, K) confusion matrix [label][pred] + one cell of skipped rows (label or prediction outside
    [0, K)); "multilabel": per head (K, 4) = tp, fp, fn, tn per label."""

    def __init__(self, task: str, head_names: Sequence[str], K: int, device):
        from . import scores as S
        self.task, self.kind, self.head_names, self.K = task, S.TASK_KIND[task], tuple(head_names), int(K)
        lim = L.SCORES_MAX_LABELS if self.kind == "multilabel" else L.SCORES_MAX_CLASSES
        if not 1 <= self.K <= lim:
            raise RuntimeError(f"ScoreTable: {self.kind} K = {K}: the scores kernel takes 1..{lim}")
        self.cells = self.K * 4 if self.kind == "multilabel" else self.K * self.K + 1
        self.table = torch.zeros(len(self.head_names), self.cells, dtype=torch.int64, device=device)
        self.skipped = None                          # multiclass: per-head skipped rows as of the last counts()

    def add(self, preds: torch.Tensor, truth: torch.Tensor):
        """Enqueue the launch that adds one batch: preds int32 (nheads, B) / (nheads, B, K), truth int64 labels (B) / float
        targets (B, K).  Nothing synchronises."""
        nh, B = len(self.head_names), int(preds.shape[1])
        ml = self.kind == "multilabel"
        want_p, want_t = ((nh, B, self.K), (B, self.K)) if ml else ((nh, B), (B,))
        if (tuple(preds.shape) != want_p or tuple(truth.shape) != want_t or preds.dtype != torch.int32
                or truth.dtype != (torch.float32 if ml else torch.int64) or not preds.is_contiguous() or not truth.is_contiguous()
                or preds.device != self.table.device or truth.device != self.table.device):
            raise RuntimeError(f"ScoreTable.add: {self.kind} needs contiguous device tensors preds int32 {want_p} and "
                               f"{'targets float32' if ml else 'labels int64'} {want_t}")
        fn = L.lib().m2m_scores_multilabel if ml else L.lib().m2m_scores_multiclass
        L.check(fn(preds.data_ptr(), truth.data_ptr(), nh, B, self.K, self.table.data_ptr(), L.stream_ptr()), "scores_" + self.kind)

    def reset(self):
        """Clear the table: an asynchronous fill on the current stream, in place -- captured graphs keep adding into it."""
        self.table.zero_()

    def counts(self) -> torch.Tensor:
        """The table on the host, int64: (nheads, K, K) or (nheads, K, 4).  One device-to-host copy: the only synchronisation."""
        host = self.table.cpu()
        if self.kind == "multilabel":
            return host.view(-1, self.K, 4)
        self.skipped = host[:, -1].clone()
        return host[:, :-1].reshape(-1, self.K, self.K)

    def compute(self) -> Dict[str, float]:
        """The reference's score names of this task -> float (fusion head: plain names; other heads: `_<modality>` appended)."""
        from . import scores as S
        return S.task_scores(self.task, self.counts().numpy(), self.head_names)


class RankBuffer:
    """The ranking buffer of one split in device memory: every step APPENDS the fp32 softmax of its batch's logits and the
    labels (csrc/rank.hip: m2m_rank_append, one launch, capturable; the row cursor lives in `state` on the device), the host
    asks once per epoch for four integers per row (m2m_rank_counts) and derives average precision / ROC-AUC in float64
    (scores.rank_scores).  probs (nheads, K, capacity): a class column is contiguous; labels (capacity) int32, -1 where the
    label was outside [0, K); state: L.RANK_STATE_WORDS uint32 (held as int32) = rows appended (keeps counting past capacity),
    arrival ticket, rows without a label, reserved."""

    def __init__(self, task: str, head_names: Sequence[str], K: int, capacity: int, device):
        from . import scores as S
        if task not in S.RANK_SCORES:
            raise RuntimeError(f"RankBuffer: no ranking scores for task {task!r} (built: {', '.join(S.RANK_SCORES)}; multilabel "
                               "ranking is not)")
        self.task, self.head_names, self.K, self.capacity = task, tuple(head_names), int(K), int(capacity)
        if not 1 <= self.K <= L.SCORES_MAX_CLASSES:
            raise RuntimeError(f"RankBuffer: K = {K}: the ranking kernels take 1..{L.SCORES_MAX_CLASSES}")
        if self.capacity < 1:
            raise RuntimeError(f"RankBuffer: capacity = {capacity}: at least one row")
        self.probs = torch.zeros(len(self.head_names), self.K, self.capacity, device=device)
        self.labels = torch.full((self.capacity,), -1, dtype=torch.int32, device=device)
        self.state = torch.zeros(L.RANK_STATE_WORDS, dtype=torch.int32, device=device)
        self.skipped = None                          # rows without a label as of the last counts()

    def add(self, logits: torch.Tensor, labels: torch.Tensor):
        """Enqueue the launch that appends one batch: logits float32 (nheads, B, K), labels int64 (B).  Nothing synchronises."""
        nh, B = len(self.head_names), int(logits.shape[1]) if logits.dim() == 3 else -1
        want_x, want_l = (nh, B, self.K), (B,)
        if (tuple(logits.shape) != want_x or tuple(labels.shape) != want_l or logits.dtype != torch.float32
                or labels.dtype != torch.int64 or not logits.is_contiguous() or not labels.is_contiguous()
                or logits.device != self.state.device or labels.device != self.state.device):
            raise RuntimeError(f"RankBuffer.add: needs contiguous device tensors logits float32 ({nh}, B, {self.K}) and labels "
                               f"int64 (B), got {tuple(logits.shape)} {logits.dtype} and {tuple(labels.shape)} {labels.dtype}")
        L.check(L.lib().m2m_rank_append(logits.data_ptr(), labels.data_ptr(), nh, B, self.K, self.probs.data_ptr(),
                                        self.labels.data_ptr(), self.capacity, self.state.data_ptr(), L.stream_ptr()), "rank_append")

    def reset(self):
        """Empty the buffer: an asynchronous fill of `state` on the current stream, in place -- captured graphs keep appending
        into the same memory (the rows behind the cursor are dead)."""
        self.state.zero_()

    def rows(self) -> int:
        """Rows appended since the last reset (one device-to-host copy; may exceed `capacity`: see counts)."""
        return int(self.state[0].item()) & 0xFFFFFFFF

    def counts(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(counts (nheads, n, 4) int64 = n_ge, p_ge, n_gt, p_gt per row, labels (n) int64) on the host.  Reads `state`, launches
        m2m_rank_counts over the n rows, copies back: the only synchronisation."""
        st = self.state.cpu().numpy().view("uint32")
        n = int(st[0])
        if n > self.capacity:
            raise RuntimeError(f"RankBuffer: overflow: capacity {self.capacity} rows, {n} rows seen since the last reset "
                               "(rank_capacity= sets the capacity)")
        self.skipped = int(st[2])
        nh = len(self.head_names)
        out = torch.zeros(nh, n, 4, dtype=torch.int32, device=self.state.device)
        if n:
            L.check(L.lib().m2m_rank_counts(self.probs.data_ptr(), self.labels.data_ptr(), nh, n, self.K, self.capacity,
                                            out.data_ptr(), L.stream_ptr()), "rank_counts")
        return out.cpu().to(torch.int64), self.labels[:n].cpu().to(torch.int64)

    def compute(self, names: Optional[Sequence[str]] = None) -> Dict[str, float]:
        """The task's ranking score names (scores.RANK_SCORES; `names`: any of auroc / ap_macro / roc_auc_macro) -> float
        (fusion head: plain names; other heads: `_<modality>` appended)."""
        from . import scores as S
        counts, labels = self.counts()
        return S.task_rank_scores(self.task, counts.numpy(), labels.numpy(), self.K, self.head_names, names)


def record_key_names(task: str, head_names: Sequence[str]) -> Dict[str, Tuple[str, ...]]:
    """The names PredictionRecord.read() gives the per-head rows of `task` (head order: modality a, modality b, fusion): the keys
    of the engines' _eval_outputs and of a bound module's test_step.  {"logits": (...), "preds": (...), "uncertainty": (...)}; the
    fusion head carries the plain name.  MIMIC spells its logits `logits_<modality>` (models/mimic.py:126-129), the two-tower
    models `<modality>_logits` (models/avmnist.py:303-312).  A pure function."""
    a, b = head_names[0], head_names[1]
    logits = (f"logits_{a}", f"logits_{b}", "logits") if task == "mimic" else (f"{a}_logits", f"{b}_logits", "logits")
    return {"logits": logits, "preds": (f"preds_{a}", f"preds_{b}", "preds"),
            "uncertainty": (f"uncertainty_{a}", f"uncertainty_{b}", "uncertainty")}


class PredictionRecord:
    """The prediction record of one split in device memory (csrc/record.hip): every evaluation step APPENDS
    its logits, its predictions and its labels -- on the evidential engine its per-sample uncertainties too -- at a row cursor that
    lives in `state` on the device (m2m_record_append: one copy launch and a one-thread advance, capturable), and the host reads
    the split's rows once: what the reference's test_epoch_end concatenates on the host and dumps as test_preds.pt
    (models/avmnist.py:382-398, models/mmimdb.py:194-209).  Rows are in arrival order.  Allocated once: captured graphs keep the
    pointers.
      logits       (nheads, capacity, K) float32
      preds        (nheads, capacity) int32; multilabel (MM-IMDb): (nheads, capacity, K) int32
      labels       (capacity) int64; multilabel: (capacity, K) float32
      uncertainty  (nheads, capacity) float32 -- uncertainty=True (AVMnistUQEngine) only
      state        L.RECORD_STATE_WORDS uint32 (held as int32): rows appended (keeps counting past capacity), reserved, reserved,
                   rows dropped
    A row at or past `capacity` is never written; read() then raises."""

    def __init__(self, task: str, head_names: Sequence[str], K: int, capacity: int, device, uncertainty: bool = False):
        from . import scores as S
        self.task, self.kind, self.head_names, self.K = task, S.TASK_KIND[task], tuple(head_names), int(K)
        self.capacity = int(capacity)
        if self.K < 1:
            raise RuntimeError(f"PredictionRecord: K = {K}: at least one class")
        if self.capacity < 1:
            raise RuntimeError(f"PredictionRecord: capacity = {capacity}: at least one row")
        nh, ml, dev = len(self.head_names), self.kind == "multilabel", torch.device(device)
        if nh * (3 if uncertainty else 2) + 1 > L.RECORD_MAX_SOURCES:
            raise RuntimeError(f"PredictionRecord: {nh} heads need more than the {L.RECORD_MAX_SOURCES} sources of one append")
        self.names = record_key_names(task, self.head_names)
        self.logits = torch.zeros(nh, self.capacity, self.K, device=dev)
        self.preds = torch.zeros((nh, self.capacity, self.K) if ml else (nh, self.capacity), dtype=torch.int32, device=dev)
        self.labels = (torch.zeros(self.capacity, self.K, device=dev) if ml
                       else torch.zeros(self.capacity, dtype=torch.int64, device=dev))
        self.uncertainty = torch.zeros(nh, self.capacity, device=dev) if uncertainty else None
        self.state = torch.zeros(L.RECORD_STATE_WORDS, dtype=torch.int32, device=dev)
        self.dropped = None                          # rows dropped as of the last read()

    @property
    def save_keys(self) -> Tuple[str, ...]:
        """The keys save() writes, in the order of the reference's dump (models/avmnist.py:382-398: the task modules'
        TEST_PRED_KEYS)."""
        lg, pr = self.names["logits"], self.names["preds"]
        return (pr[2], pr[0], pr[1], "labels", lg[0], lg[1], lg[2])

    def add(self, engine, labels: torch.Tensor):
        """Enqueue the append of `engine`'s step: its `logits` and `preds` -- and `uncertainty` where the record holds one -- one
        source per head and tensor, plus `labels`.  One m2m_record_append; nothing synchronises."""
        nh, B, K, ml, dev = len(self.head_names), int(engine.B), self.K, self.kind == "multilabel", self.state.device
        want = [("logits", engine.logits, (nh, B, K), torch.float32),
                ("preds", engine.preds, (nh, B, K) if ml else (nh, B), torch.int32)]
        if self.uncertainty is not None:
            want.append(("uncertainty", getattr(engine, "uncertainty", None), (nh, B), torch.float32))
        want.append(("labels", labels, (B, K) if ml else (B,), torch.float32 if ml else torch.int64))
        for name, t, shape, dtype in want:
            if (t is None or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev):
                got = "None" if t is None else f"{tuple(t.shape)} {t.dtype} on {t.device}"
                raise RuntimeError(f"PredictionRecord.add: {name} must be a contiguous {dtype} tensor {shape} on {dev}, got {got}")
        pairs = []
        for name, t, _, _ in want[:-1]:
            mine = getattr(self, name)
            pairs += [(t[h], mine[h]) for h in range(nh)]
        pairs.append((labels, self.labels))
        desc = (L.FeedSrc * len(pairs))()
        for d, (s, t) in zip(desc, pairs):
            d.src, d.dst, d.row_bytes = s.data_ptr(), t.data_ptr(), int(s[0].numel()) * s.element_size()
        L.check(L.lib().m2m_record_append(desc, len(pairs), B, self.capacity, self.state.data_ptr(), L.stream_ptr()), "record_append")

    def reset(self):
        """Empty the record: an asynchronous fill of `state` on the current stream, in place -- captured graphs keep appending
        into the same memory (the rows behind the cursor are dead)."""
        self.state.zero_()

    def rows(self) -> int:
        """Rows appended since the last reset (one small device-to-host copy; may exceed `capacity`: see read)."""
        return int(self.state[0].item()) & 0xFFFFFFFF

    def read(self) -> Dict[str, torch.Tensor]:
        """The record on the host under the names the task's test_step returns: per-head logits (n, K) float32 and preds, `labels`,
        on the evidential engine per-sample `uncertainty*` (n) -- with the dtypes a bound module's test_step gives: preds int64
        (MIMIC: `preds*` are the softmax of the recorded logits, models/mimic.py:126), labels as recorded.  No loss keys: losses
        are per step, not per row.  Reads `state`, then copies the first n rows of every buffer: the only synchronisation."""
        st = self.state.cpu().numpy().view("uint32")
        n, self.dropped = int(st[0]), int(st[3])
        if n > self.capacity or self.dropped:
            raise RuntimeError(f"PredictionRecord: overflow: capacity {self.capacity} rows, {n} rows seen since the last reset "
                               f"({self.dropped} dropped; record_capacity= / prediction_record(split, capacity) sets the capacity)")
        logits = self.logits[:, :n].cpu()
        out = dict(zip(self.names["logits"], logits.unbind(0)))
        if self.task == "mimic":
            out.update(zip(self.names["preds"], torch.softmax(logits, dim=2).unbind(0)))
        else:
            out.update(zip(self.names["preds"], self.preds[:, :n].cpu().long().unbind(0)))
        out["labels"] = self.labels[:n].cpu()
        if self.uncertainty is not None:
            out.update(zip(self.names["uncertainty"], self.uncertainty[:, :n].cpu().unbind(0)))
        return out

    def save(self, path: str, keys: Optional[Sequence[str]] = None) -> str:
        """torch.save of read()'s `keys` (default: save_keys, the reference's dump) as one dict, in that order."""
        got = self.read()
        torch.save({k: got[k].clone() for k in (self.save_keys if keys is None else keys)}, path)
        return path


class PassAccumulators(NamedTuple):
    """What one pass over a split adds into beside its losses: the count table, the ranking buffer and the prediction record,
    each None where the pass has none.  The one place that knows how the three are reset, handed to evaluate(), read and put
    back after a warm-up."""

    scores: Optional[ScoreTable] = None
    rank: Optional[RankBuffer] = None
    record: Optional[PredictionRecord] = None

    def kwargs(self) -> Dict[str, object]:
        """evaluate(**kwargs()): the members present, under evaluate's names (none: {} -- an evaluate without keywords serves)."""
        return {k: a for k, a in zip(self._fields, self) if a is not None}

    def reset(self):
        for a in self.kwargs().values():
            a.reset()

    def compute(self) -> Dict[str, float]:
        """The table's numbers, then the ranking buffer's merged over them (the record is read by its owner: read() / save())."""
        out = {} if self.scores is None else self.scores.compute()
        if self.rank is not None:
            out.update(self.rank.compute())
        return out

    def state(self) -> List[torch.Tensor]:
        """The tensors a warm-up step changes and must put back: the table's counts, the two cursors (rows behind a cursor are dead)."""
        return [getattr(a, attr) for a, attr in zip(self, ("table", "state", "state")) if a is not None]


def pass_accumulators(engine, split: str, train: bool = False, record: Optional[PredictionRecord] = None) -> PassAccumulators:
    """The accumulators of a pass over `split` on `engine` (anything run_epoch drives: an engine without `scores` / `rank` has
    none).  A training pass counts into the training table and buffer (the captured step adds there), an evaluating pass into
    `split`'s own -- the training split's under "train_eval"."""
    which = "train" if train else (split if split != "train" else "train_eval")
    return PassAccumulators(engine.score_table(which) if getattr(engine, "scores", None) is not None else None,
                            engine.rank_buffer(which) if getattr(engine, "rank", None) is not None else None, record)


class EpochFeed:
    """One split's resident tensors behind a device-side permutation and cursor (csrc/feed.hip): a step
    gathers its own batch (m2m_feed_gather: rows perm[(cursor + r) % n] of every source into the step's input slots, the cursor
    advanced on the device) and adds its own losses and hit counts to the epoch's accumulators (m2m_epoch_accumulate) -- both
    capturable, so a graph from engine.capture_feed replays without arguments and an epoch is read back once.

    sources: the split's tensors in the engine's batch order (AV-MNIST: image, audio, labels), contiguous, on `device`, with the
    dtypes the engine's inputs have; rows of a multiple of 4 bytes.  The feed owns
      perm    (n) int32, the epoch's sample order
      state   L.FEED_STATE_WORDS uint32 (held as int32): cursor, reserved (zero), n, wrapped rows
      sums    (2 * nloss) float64: step losses | the same weighted by the step's batch size
      counts  (nheads + 2) int64: hits per head | steps | samples
    nloss / nheads follow the first engine the feed is used with (multilabel predictions have no hit count: nheads = 0).
    Single GPU only: every rank of a data-parallel run would need its shard of the order (out of scope).

    muting=True (stage two's random modality muting, models/avmnist.py:243-256): the feed also owns
      mute_codes  (ceil(n / B)) int32, one code per step of the epoch: 0 mutes nothing, s + 1 mutes source s (start writes them)
      mute_state  L.FEED_MUTE_STATE_WORDS uint32 (held as int32): the step index, steps that ran past the schedule
    and gather_into uses m2m_feed_gather_muted: the muted source's slot is filled with zero bytes, its rows are not read.
    Both are allocated once: a captured graph keeps their pointers.  Off (the default): neither exists, nothing new is launched.

    uncertainty=True (the evidential engine, AVMnistUQEngine): the feed also holds
      unc_sums  (nheads of the engine's `uncertainty` buffer) float64: per step += the batch mean of each head's uncertainty
    behind the counts in the same buffer (m2m_epoch_accumulate_uq, one more launch per step; models/avmnist.py:556-572 logs the
    mean over steps of the step means, the ragged tail as one step).  Refused on an engine without an `uncertainty` buffer.  Off
    (the default): a captured feed graph keeps exactly the nodes it had."""

    def __init__(self, sources: Sequence[torch.Tensor], batch_size: int, device, muting: bool = False, uncertainty: bool = False):
        self.device = torch.device(device)
        self.sources = tuple(sources)
        self.B = int(batch_size)
        if not 1 <= len(self.sources) <= L.FEED_MAX_SOURCES:
            raise ValueError(f"EpochFeed: 1..{L.FEED_MAX_SOURCES} sources, got {len(self.sources)}")
        if self.B < 1:
            raise ValueError("EpochFeed: batch_size >= 1")
        self.n = int(self.sources[0].shape[0])
        if not 1 <= self.n < 2 ** 31:
            raise ValueError(f"EpochFeed: the split needs 1 <= n < 2^31 rows, got {self.n}")
        for i, t in enumerate(self.sources):
            if t.device != self.device or not t.is_contiguous() or t.dim() < 1 or int(t.shape[0]) != self.n:
                raise ValueError(f"EpochFeed: source {i} must be a contiguous tensor of {self.n} rows on {self.device}")
            if self._row_bytes(t) < 4 or self._row_bytes(t) % 4:
                raise ValueError(f"EpochFeed: source {i} has rows of {self._row_bytes(t)} bytes; the gather copies multiples of 4")
        self.perm = torch.arange(self.n, dtype=torch.int32, device=self.device)
        self._state0 = torch.tensor([0, 0, self.n, 0], dtype=torch.int32, device=self.device)
        self.state = self._state0.clone()
        self.mute_codes = self.mute_state = None
        if muting:
            self.mute_codes = torch.zeros((self.n + self.B - 1) // self.B, dtype=torch.int32, device=self.device)
            self.mute_state = torch.zeros(L.FEED_MUTE_STATE_WORDS, dtype=torch.int32, device=self.device)
        self._acc: Optional[torch.Tensor] = None         # sums and counts in one 8-byte-cell buffer: one copy reads both
        self.nloss = self.nheads = None
        self.sums = self.counts = None
        self.uncertainty = bool(uncertainty)
        self.nunc = 0
        self.unc_sums = None

    @staticmethod
    def _row_bytes(t: torch.Tensor) -> int:
        return int(t[0].numel()) * t.element_size()

    def bind(self, engine):
        """Size the accumulators for `engine`'s losses and heads (first use), or check that they fit it."""
        nloss = int(engine.losses.numel())
        nheads = int(engine.preds.shape[0]) if engine.preds.dim() == 2 else 0
        nunc = 0
        if self.uncertainty:
            u = getattr(engine, "uncertainty", None)
            if u is None:
                raise RuntimeError(f"EpochFeed(uncertainty=True): {type(engine).__name__} has no `uncertainty` buffer (the "
                                   "evidential engine, AVMnistUQEngine, has)")
            nunc = int(u.shape[0])
        if self._acc is None:
            self.nloss, self.nheads, self.nunc = nloss, nheads, nunc
            self._acc = torch.zeros(2 * nloss + nheads + 2 + nunc, dtype=torch.int64, device=self.device)
            self.sums, self.counts = self._acc[:2 * nloss].view(torch.float64), self._acc[2 * nloss:2 * nloss + nheads + 2]
            if nunc:
                self.unc_sums = self._acc[2 * nloss + nheads + 2:].view(torch.float64)
        elif (nloss, nheads, nunc) != (self.nloss, self.nheads, self.nunc):
            raise RuntimeError(f"EpochFeed: accumulators sized for {self.nloss} losses / {self.nheads} heads / {self.nunc} "
                               f"uncertainties, the engine has {nloss} / {nheads} / {nunc}")

    def new_slots(self, batch_size: Optional[int] = None) -> Tuple[torch.Tensor, ...]:
        """Zeroed input slots of one step: the sources' row shapes and dtypes at `batch_size` rows (default: the feed's)."""
        B = self.B if batch_size is None else int(batch_size)
        return tuple(torch.zeros(B, *t.shape[1:], dtype=t.dtype, device=self.device) for t in self.sources)

    def start(self, order=None, muting=None):
        """Begin an epoch: write its sample order (a host or device index tensor of n values in [0, n); None: identity) IN PLACE
        and zero the cursor, the wrapped count and the accumulators, all on the current stream -- captured graphs keep reading
        the same memory.  A given order is checked against [0, n) first (the one synchronisation: an index outside the split
        would read outside it).
        muting (a feed built with muting=True): the epoch's codes, one per step, at most ceil(n / B), each in [0, nsrc - 1] -- the
        last source, the labels, cannot be muted; written in place, the rest of the schedule zero; None: all zeros.  The step
        index and the overflow word are reset."""
        codes = None
        if muting is not None:
            if self.mute_codes is None:
                raise ValueError("EpochFeed.start: a muting schedule needs a feed built with muting=True")
            codes = torch.as_tensor(muting).detach().cpu()
            cap, hi_code = int(self.mute_codes.numel()), len(self.sources) - 1
            if codes.dim() != 1 or codes.dtype.is_floating_point or codes.dtype == torch.bool or int(codes.numel()) > cap:
                raise ValueError(f"EpochFeed.start: the muting schedule must hold at most {cap} integer codes, got "
                                 f"{tuple(codes.shape)} {codes.dtype}")
            if codes.numel() and (int(codes.min()) < 0 or int(codes.max()) > hi_code):
                raise ValueError(f"EpochFeed.start: muting codes span [{int(codes.min())}, {int(codes.max())}]; allowed are 0 (nothing) "
                                 f"and 1..{hi_code} (source s + 1; the last source, the labels, cannot be muted)")
        if order is None:
            torch.arange(self.n, out=self.perm)
        else:
            order = torch.as_tensor(order)
            if order.dim() != 1 or int(order.numel()) != self.n or order.dtype.is_floating_point or order.dtype == torch.bool:
                raise ValueError(f"EpochFeed.start: the order must hold {self.n} integer indices, got {tuple(order.shape)} {order.dtype}")
            lo, hi = (int(v) for v in torch.stack((order.min(), order.max())).cpu())
            if lo < 0 or hi >= self.n:
                raise ValueError(f"EpochFeed.start: the order's indices span [{lo}, {hi}], the split has rows [0, {self.n})")
            self.perm.copy_(order.to(torch.int32))
        self.state.copy_(self._state0)
        if self.mute_codes is not None:
            self.mute_codes.zero_()
            if codes is not None and codes.numel():
                self.mute_codes[:codes.numel()].copy_(codes.to(torch.int32))
            self.mute_state.zero_()
        if self._acc is not None:
            self._acc.zero_()

    def _state_host(self):
        return self.state.cpu().numpy().view("uint32")

    def rows(self) -> int:
        """Rows handed out since start() (the cursor; one device-to-host copy)."""
        return int(self._state_host()[0])

    def check(self):
        """Raise when a gather ran past the end of the epoch (its rows wrapped around to the order's head)."""
        st = self._state_host()
        if int(st[3]):
            raise RuntimeError(f"EpochFeed: {int(st[0])} rows were fed from a split of {self.n}: {int(st[3])} row(s) wrapped around "
                               "to the head of the order (a replay past the end of the epoch)")
        if self.mute_state is not None:
            ms = self.mute_state.cpu().numpy().view("uint32")
            if int(ms[1]):
                raise RuntimeError(f"EpochFeed: {int(ms[0])} gathers ran against a muting schedule of {int(self.mute_codes.numel())} "
                                   f"steps: {int(ms[1])} step(s) past its end muted nothing")

    def read(self, with_uncertainty: bool = False):
        """(sums float64 (2 * nloss), counts int64 (nheads + 2)) on the host as numpy: one copy, the epoch's only synchronisation.
        with_uncertainty (a feed built with uncertainty=True): a third array, unc_sums float64 (nunc), from the same copy."""
        if self._acc is None:
            raise RuntimeError("EpochFeed.read: no engine has used this feed yet")
        if with_uncertainty and not self.nunc:
            raise RuntimeError("EpochFeed.read: the uncertainty sums need a feed built with uncertainty=True")
        host = self._acc.cpu().numpy()
        end = 2 * self.nloss + self.nheads + 2
        out = (host[:2 * self.nloss].view("float64").copy(), host[2 * self.nloss:end].copy())
        return out + (host[end:].view("float64").copy(),) if with_uncertainty else out

    def gather_into(self, slots: Sequence[torch.Tensor]):
        """Enqueue the gather of the next slots[0].shape[0] rows of the order into `slots` (one per source, as new_slots makes
        them; any batch size: the ragged tail's engine has its own).  Nothing synchronises."""
        if len(slots) != len(self.sources):
            raise ValueError(f"EpochFeed.gather_into: {len(self.sources)} slots (one per source), got {len(slots)}")
        B = int(slots[0].shape[0])
        desc = (L.FeedSrc * len(slots))()
        for d, s, t in zip(desc, self.sources, slots):
            if (t.dtype != s.dtype or tuple(t.shape) != (B, *s.shape[1:]) or not t.is_contiguous() or t.device != self.device):
                raise ValueError(f"EpochFeed.gather_into: a slot must be a contiguous {s.dtype} tensor ({B}, {', '.join(map(str, s.shape[1:]))}) "
                                 f"on {self.device}, got {t.dtype} {tuple(t.shape)}")
            d.src, d.dst, d.row_bytes = s.data_ptr(), t.data_ptr(), self._row_bytes(s)
        if self.mute_codes is not None:
            L.check(L.lib().m2m_feed_gather_muted(desc, len(slots), self.perm.data_ptr(), B, self.state.data_ptr(),
                                                  self.mute_codes.data_ptr(), int(self.mute_codes.numel()), self.mute_state.data_ptr(),
                                                  L.stream_ptr()), "feed_gather_muted")
            return
        L.check(L.lib().m2m_feed_gather(desc, len(slots), self.perm.data_ptr(), B, self.state.data_ptr(), L.stream_ptr()), "feed_gather")

    def accumulate(self, engine, labels: Optional[torch.Tensor]):
        """Enqueue the launch that adds `engine`'s step (its losses, its preds against `labels`, its batch size) to the epoch's
        accumulators.  Nothing synchronises."""
        self.bind(engine)
        preds = engine.preds if self.nheads else None
        if self.nheads and (labels is None or labels.dtype != torch.int64 or tuple(labels.shape) != (engine.B,) or not labels.is_contiguous()
                            or preds.dtype != torch.int32 or not preds.is_contiguous()):
            raise RuntimeError(f"EpochFeed.accumulate: hit counts need contiguous labels int64 ({engine.B},) and preds int32")
        L.check(L.lib().m2m_epoch_accumulate(engine.losses.data_ptr(), self.nloss, L.ptr(preds), L.ptr(labels) if self.nheads else 0,
                                             self.nheads, engine.B, self.sums.data_ptr(), self.counts.data_ptr(), L.stream_ptr()),
                "epoch_accumulate")
        if self.nunc:
            u = engine.uncertainty
            if tuple(u.shape) != (self.nunc, engine.B) or u.dtype != torch.float32 or not u.is_contiguous():
                raise RuntimeError(f"EpochFeed.accumulate: uncertainty must be contiguous float32 ({self.nunc}, {engine.B})")
            L.check(L.lib().m2m_epoch_accumulate_uq(u.data_ptr(), self.nunc, engine.B, self.unc_sums.data_ptr(), L.stream_ptr()),
                    "epoch_accumulate_uq")
