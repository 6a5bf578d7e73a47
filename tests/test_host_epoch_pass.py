"""Host tests (no GPU) of the pieces every pass over a split shares: accumulators.PassAccumulators / pass_accumulators, data.tail_engine_for
/ tail_step and data.epoch_metrics, on stubs of the surface run_epoch drives (tests/test_host_cpu.py::_StubEngine)."""
import pytest
import torch

from m2_mixer_amd import data as D
from m2_mixer_amd.accumulators import PassAccumulators, pass_accumulators


class _Acc:
    """A table / buffer / record: counts its resets, names the tensor a warm-up must put back."""

    def __init__(self, name, **tensors):
        self.name, self.resets = name, 0
        self.__dict__.update(tensors)

    def reset(self):
        self.resets += 1

    def compute(self):
        return {self.name: 1.0, "shared": self.name}


class _Engine:
    """_StubEngine's surface: no `scores`, `rank` or `score_table` unless asked for; evaluate takes no keywords."""

    MODS = ("image", "audio")

    def __init__(self, batch_size, scores=False, rank=False, parent=None, trains=True):
        self.B, self.device, self.parent, self.trains = batch_size, torch.device("cpu"), parent, trains
        self.losses, self.preds = torch.zeros(4), torch.zeros(3, batch_size, dtype=torch.int32)
        self.packs, self.built, self.asked = 0, [], []
        self._tail_engines = {}
        if scores:
            self.scores = _Acc("train table", table="T", state="not this one")
            self.score_table = lambda which: self._of(which, "table", self.scores)
        if rank:
            self.rank = _Acc("train buffer", state="R", table="not this one")
            self.rank_buffer = lambda which: self._of(which, "buffer", self.rank)

    def _of(self, which, kind, training):
        self.asked.append((kind, which))
        return training if which == "train" else _Acc(f"{which} {kind}", table="T", state="R")

    def sibling(self, bs, trains=True):
        self.built.append((bs, trains))
        return _Engine(bs, parent=self, trains=trains)

    def pack(self):
        self.packs += 1

    def train_step(self, *batch, grad_sync=None):
        assert self.trains and batch[0].shape[0] == self.B
        return self.losses

    def evaluate(self, *batch):
        assert batch[0].shape[0] == self.B
        return {}


# ---- the accumulators of a pass ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("split,train,which", [("train", True, "train"), ("val", True, "train"), ("train", False, "train_eval"),
                                               ("val", False, "val"), ("test", False, "test")])
def test_pass_accumulators_names_the_split(split, train, which):
    eng = _Engine(8, scores=True, rank=True)
    accs = pass_accumulators(eng, split, train)
    assert eng.asked == [("table", which), ("buffer", which)]
    assert (accs.scores is eng.scores) == (accs.rank is eng.rank) == (which == "train")
    assert accs.scores.name == f"{which} table" and accs.rank.name == f"{which} buffer" and accs.record is None
    assert accs.kwargs() == {"scores": accs.scores, "rank": accs.rank}


def test_pass_accumulators_of_an_engine_without_any():
    accs = pass_accumulators(_Engine(8), "val")
    assert accs == PassAccumulators(None, None, None) and accs.kwargs() == {} and accs.state() == [] and accs.compute() == {}
    accs.reset()                                                 # nothing to reset: no error
    _Engine(8).evaluate(torch.zeros(8), **accs.kwargs())         # an evaluate without keywords serves


def test_pass_accumulators_with_a_ranking_buffer_only_and_a_record():
    eng, record = _Engine(8, rank=True), _Acc("record", state="P", table="not this one")
    accs = pass_accumulators(eng, "test", record=record)
    assert accs.scores is None and eng.asked == [("buffer", "test")]
    assert accs.kwargs() == {"rank": accs.rank, "record": record} and list(accs.kwargs()) == ["rank", "record"]
    assert accs.state() == ["R", "P"]
    assert accs.compute() == {"test buffer": 1.0, "shared": "test buffer"}       # the record is read by its owner
    accs.reset()
    assert (accs.rank.resets, record.resets) == (1, 1)


def test_pass_accumulators_state_and_compute_order():
    """state(): the table's `table`, then the two cursors' `state`; compute(): the ranking buffer's numbers over the table's."""
    scores, rank, record = _Acc("s", table="T", state="x"), _Acc("r", state="R", table="x"), _Acc("p", state="P", table="x")
    accs = PassAccumulators(scores, rank, record)
    assert accs.state() == ["T", "R", "P"]
    assert accs.compute() == {"s": 1.0, "r": 1.0, "shared": "r"}
    assert PassAccumulators(scores).state() == ["T"] and PassAccumulators(scores).kwargs() == {"scores": scores}
    accs.reset()
    assert (scores.resets, rank.resets, record.resets) == (1, 1, 1)


# ---- the ragged tail's engine -----------------------------------------------------------------------------------------
def test_tail_engine_a_given_one_wins():
    eng, given = _Engine(8), _Engine(3)
    eng._tail_engines[3] = _Engine(3)
    for trains in (True, False):
        assert D.tail_engine_for(eng, 3, trains, given, reuse=True, keep={}) is given
    assert eng.built == []


def test_tail_engine_training_is_kept_and_reused():
    eng = _Engine(8)
    first = D.tail_engine_for(eng, 3)
    assert eng._tail_engines == {3: first} and first.trains
    assert D.tail_engine_for(eng, 3, True) is first and D.tail_engine_for(eng, 5) is not first
    assert eng.built == [(3, True), (5, True)] and set(eng._tail_engines) == {3, 5}


def test_tail_engine_evaluating_is_never_the_kept_training_one():
    eng = _Engine(8)
    a, b = D.tail_engine_for(eng, 3, False), D.tail_engine_for(eng, 3, False)
    assert a is not b and not a.trains and eng._tail_engines == {}        # built per pass, as run_epoch_fed's evaluating tail
    kept = D.tail_engine_for(eng, 3)
    assert D.tail_engine_for(eng, 3, False) is not kept                   # run_epoch_fed looks there only when training
    assert D.tail_engine_for(eng, 3, False, reuse=True) is kept           # run_epoch evaluates on the kept training sibling
    assert eng._tail_engines == {3: kept}
    assert eng.built == [(3, False), (3, False), (3, True), (3, False)]


def test_tail_engine_evaluating_kept_where_asked():
    """GradBlend's probing passes: the evaluating sibling is found and kept in the caller's dict, never in _tail_engines."""
    eng, mine = _Engine(8), {}
    a = D.tail_engine_for(eng, 3, False, keep=mine)
    assert mine == {3: a} and D.tail_engine_for(eng, 3, False, keep=mine) is a and eng._tail_engines == {}
    training = D.tail_engine_for(eng, 3)
    assert training is not a and D.tail_engine_for(eng, 3, False, keep=mine) is a and mine == {3: a}
    assert eng.built == [(3, False), (3, True)]


def test_prepare_tail_engine_uses_the_rule():
    data = D.ResidentTensors({"train": (torch.zeros(19, 2), torch.zeros(19))})
    eng = _Engine(8)
    tail = D.prepare_tail_engine(eng, data, "train", 8)
    assert eng._tail_engines == {3: tail} and D.prepare_tail_engine(eng, data, "train", 8) is tail and eng.built == [(3, True)]
    assert D.prepare_tail_engine(eng, data, "train", 19) is None


@pytest.mark.parametrize("trains,parent_packs", [(True, 1), (False, 0)])
def test_tail_step_packs(trains, parent_packs):
    eng, tail = _Engine(8), _Engine(3)
    with D.tail_step(eng, tail, trains) as t:
        assert t is tail and (tail.packs, eng.packs) == (1, 0)            # pack() before the step, the parent's only after it
    assert (tail.packs, eng.packs) == (1, parent_packs)


class _Resident(D.ResidentTensors):
    batches = D.ResidentAVMnist.batches


@pytest.mark.parametrize("train", [True, False])
def test_run_epoch_on_an_engine_without_accumulators(train):
    """19 rows at batch 8: two full batches and a tail of 3 through tail_engine_for / tail_step; evaluate takes no keywords."""
    data = _Resident({"train": (torch.zeros(19, 1), torch.zeros(19, 1), torch.zeros(19, dtype=torch.int64))})
    eng = _Engine(8)
    out = D.run_epoch(eng, data, "train", 8, train=train)
    assert (out["steps"], out["samples"], out["hits"], out["acc"]) == (3, 19, 19, 1.0)
    assert eng.built == [(3, train)] and eng.packs == int(train)
    assert set(eng._tail_engines) == ({3} if train else set())
    if train:
        assert eng._tail_engines[3].packs == 1


# ---- the metrics of a pass --------------------------------------------------------------------------------------------
# One hand-made set of sums, laid out as run_epoch's host vector: [loss_a, loss_b, loss_fusion, loss] summed over 4 steps | the
# same weighted by the batch sizes (only the total is read) | hits a, b, fusion; 20 samples.
HOST = [1.5, 2.5, 3.0, 7.0, 0.0, 0.0, 0.0, 50.0, 12.0, 8.0, 15.0]
# what run_epoch built from it: loss = host[7] / samples, the step means host[0..3] / steps, acc* = hits / samples
EXPECTED = {"loss": 2.5, "loss_step_mean": 1.75, "loss_image": 0.375, "loss_audio": 0.625, "loss_fusion": 0.75,
            "acc": 0.75, "acc_image": 0.6, "acc_audio": 0.4, "hits": 15, "hits_image": 12, "hits_audio": 8, "steps": 4, "samples": 20}


def test_epoch_metrics_reproduces_run_epoch():
    out = D.epoch_metrics(("image", "audio"), HOST[:4], HOST[7], 4, 20, hits=HOST[8:11])
    assert out == EXPECTED
    assert all(type(out[k]) is int for k in ("hits", "hits_image", "hits_audio", "steps", "samples"))
    assert all(type(v) is float for k, v in out.items() if not k.startswith(("hits", "steps", "samples")))


def test_epoch_metrics_without_hits_with_uncertainty():
    """Multilabel predictions have no hit count; uncertainty sums [a, b, fusion] become step means, the fusion head's plain."""
    losses = {k: v for k, v in EXPECTED.items() if not k.startswith(("acc", "hits"))}
    assert D.epoch_metrics(("image", "text"), HOST[:4], HOST[7], 4, 20) == {
        "loss": 2.5, "loss_step_mean": 1.75, "loss_image": 0.375, "loss_text": 0.625, "loss_fusion": 0.75, "steps": 4, "samples": 20}
    out = D.epoch_metrics(("image", "audio"), HOST[:4], HOST[7], 4, 20, hits=torch.tensor([12, 8, 15]).numpy(), unc=[0.8, 1.2, 2.0])
    assert out == dict(EXPECTED, uncertainty=0.5, uncertainty_image=0.2, uncertainty_audio=0.3)
    assert D.epoch_metrics(("image", "audio"), HOST[:4], HOST[7], 4, 20, unc=[0.8, 1.2, 2.0]) == dict(
        losses, uncertainty=0.5, uncertainty_image=0.2, uncertainty_audio=0.3)


def test_epoch_metrics_of_an_empty_pass():
    """No step ran: the denominators are max(., 1), the counts stay 0 (run_epoch's steps, n = max(nb, 1), max(seen, 1))."""
    out = D.epoch_metrics(("image", "audio"), [0.0] * 4, 0.0, 0, 0, hits=[0, 0, 0])
    assert out == dict({k: 0.0 for k in EXPECTED}, hits=0, hits_image=0, hits_audio=0, steps=0, samples=0)
