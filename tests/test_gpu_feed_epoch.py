"""Fed epochs on the engines (-m gpu): engine.capture_feed + data.run_epoch_fed on the golden M2-Mixer-B shape and on tiny
configurations of tests/engine_cases.py.  Every case: batch 8 over a split of 43 samples (five full batches and a ragged tail of
3) in a shuffled order.

AV-MNIST (M2-Mixer-B, the configuration test_gpu_parity.test_bf16_training_is_bit_reproducible gives its guarantee for; bf16,
dropout 0.5.  The smaller AV-MNIST configurations do not repeat their own bits at batch 8: two engines driven by the SAME manual
loop ended 3e-8 .. 2e-7 apart in their parameters on M2-Mixer-S / -M and on av_grouped_n2_n4_d64_half, 0.0 on M2-Mixer-B):
a fed epoch against a second engine of the same seed driven by capture() / replay(index_select ...)
over the same order, the tail through its sibling.  The feed's launches only write input slots and accumulators, so parameters
and both Adam moments are BIT-identical; hits, steps and samples are exact; the losses are held to 1e-6 relative (the heads kernel
sums a batch's loss with float atomics, so the two runs may differ in the last bits).  steps = 1, steps = 2 (two replays, one
eager single step, the tail), and with scores=True / rank_scores=True, whose tables and ranking counts must equal the manual
loop's.

MIMIC and MM-IMDb (fp32, dropout 0; the MIMIC step does not repeat its own bits from run to run, so nothing bit-level is
asserted): a fed epoch against the float64 reference of tests/engine_ref.py stepped over the same sample order, at the fp32 bars
of tests/test_gpu_engine_envelope.py (losses 1e-3 absolute, parameters 2e-3 absolute with the rounding-level key left out) and its
learning rate.

train=False: fed evaluation of a 19-sample split equals engine.evaluate over the same batches; logits bit-equal."""
import numpy as np
import pytest
import torch

import engine_ref as R
import gen_util as G
from engine_cases import CASES, Case

pytestmark = pytest.mark.gpu

B, N, NVAL = 8, 43, 19
LR = 2e-3                                              # tests/test_gpu_engine_envelope.py
FP32_LOSSES, FP32_PARAMS = 1e-3, 2e-3                  # its fp32 bars
LOSS_REL = 1e-6
AV_CASE = Case("avmnist_B", "avmnist", dict(G.AVMNIST["B"]), B, 0.5, {})          # dropout 0.5; repeats its own bits (see above)
ORACLE_CASES = ("mimic_patches_7", "mm_token_dim_32")

_ORACLE = {}                                           # case name -> the float64 epoch: computed once, shared by the step counts


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def case_of(name, **over):
    c = name if isinstance(name, Case) else next(c for c in CASES if c.name == name)
    return c._replace(B=B, **over)


def split_of(case, n, seed, dev):
    return tuple(t.to(dev) for t in R.case_batch(case._replace(B=n), seed))


def order_of(n, seed, dev):
    return torch.from_numpy(np.random.default_rng(seed).permutation(n)).to(dev)


def av_engine(case, dev, **kw):
    from m2_mixer_amd.engine import AVMnistEngine
    return AVMnistEngine(case.cfg, B, device=dev, precision="bf16", lr=1e-3, seed=9, **kw)


class Tally:
    """What run_epoch accumulates, on the host in float64."""

    def __init__(self):
        self.sums, self.hits, self.steps, self.samples = np.zeros(8), np.zeros(3, dtype=np.int64), 0, 0

    def add(self, losses, preds, labels, bs):
        l = losses.detach().double().cpu().numpy()
        self.sums[:4] += l
        self.sums[4:] += l * bs
        if preds.dim() == 2:
            self.hits += (preds == labels[None, :].to(preds.dtype)).sum(dim=1).cpu().numpy()
        self.steps += 1
        self.samples += bs

    def result(self, mods):
        a, b = mods
        return {"loss": self.sums[7] / self.samples, "loss_step_mean": self.sums[3] / self.steps, f"loss_{a}": self.sums[0] / self.steps,
                f"loss_{b}": self.sums[1] / self.steps, "loss_fusion": self.sums[2] / self.steps, "hits": int(self.hits[2]),
                f"hits_{a}": int(self.hits[0]), f"hits_{b}": int(self.hits[1]), "steps": self.steps, "samples": self.samples}


def manual_epoch(eng, srcs, order, steps):
    """The parent's way: capture(steps) + replay(index_select ...) per graph, train_step for the full batches that do not fill a
    graph, the tail through the kept sibling."""
    from m2_mixer_amd.data import feed_plan
    replays, singles, tail = feed_plan(int(order.numel()), B, steps)
    pick = lambda lo, bs: tuple(t.index_select(0, order[lo:lo + bs]) for t in srcs)
    replay = eng.capture(*pick(0, B), steps=steps)
    tally, pos = Tally(), 0
    for _ in range(replays):
        batches = [pick(pos + i * B, B) for i in range(steps)]
        replay(*[t for b in batches for t in b])
        torch.cuda.synchronize()
        for i, b in enumerate(batches):
            tally.add(*((eng.losses, eng.preds) if steps == 1 else (eng.losses_steps[i], eng.preds_steps[i])), b[-1], B)
        pos += steps * B
    for _ in range(singles):
        b = pick(pos, B)
        eng.train_step(*b)
        tally.add(eng.losses, eng.preds, b[-1], B)
        pos += B
    if tail:
        sib = eng._tail_engines[tail]
        b = pick(pos, tail)
        sib.pack()
        sib.train_step(*b)
        eng.pack()
        tally.add(sib.losses, sib.preds, b[-1], tail)
    torch.cuda.synchronize()
    return tally.result(eng.HEAD_NAMES[:2])


def fed_epoch(eng, srcs, order, steps):
    from m2_mixer_amd.data import run_epoch_fed
    from m2_mixer_amd.engine import EpochFeed
    feed = EpochFeed(srcs, B, eng.device)
    replay = eng.capture_feed(feed, steps=steps)
    assert feed.rows() == 0 and not feed.read()[1].any(), "capture_feed must put the feed's cursor and accumulators back"
    out = run_epoch_fed(eng, feed, replay, int(order.numel()), order=order)
    torch.cuda.synchronize()
    assert feed.rows() == int(order.numel())
    return out


def with_tail(eng):
    eng._tail_engines[N % B] = eng.sibling(N % B)          # prepare_tail_engine's rule: the training sibling exists before capture
    return eng


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "scores_and_rank"])
@pytest.mark.parametrize("steps", [1, 2])
def test_avmnist_fed_epoch_is_the_manual_epoch_bit_for_bit(steps, extras, dev):
    case = case_of(AV_CASE)
    srcs, order = split_of(case, N, 301, dev), order_of(N, 17, dev)
    kw = dict(scores=True, rank_scores=True) if extras else {}
    manual, fed = with_tail(av_engine(case, dev, **kw)), with_tail(av_engine(case, dev, **kw))
    assert torch.equal(manual.flat_p, fed.flat_p)
    want = manual_epoch(manual, srcs, order, steps)
    got = fed_epoch(fed, srcs, order, steps)
    for name in ("flat_p", "flat_m", "flat_v"):
        assert torch.equal(getattr(manual, name), getattr(fed, name)), f"{name} differs from the manual loop's"
    assert float(fed.adam_state[0]) == float(manual.adam_state[0]) == 6.0 and int(fed.drop_step[0]) == int(manual.drop_step[0]) == 6
    for k in ("hits", "hits_image", "hits_audio", "steps", "samples"):
        assert got[k] == want[k], k
    assert got["steps"] == 6 and got["samples"] == N
    assert got["acc"] == want["hits"] / N
    for k in ("loss", "loss_step_mean", "loss_image", "loss_audio", "loss_fusion"):
        rel = abs(got[k] - want[k]) / abs(want[k])
        print(f"steps {steps} {k}: fed {got[k]:.9g} manual {want[k]:.9g} rel {rel:.2e}")
        assert rel < LOSS_REL, k
    if extras:
        assert torch.equal(fed.scores.table, manual.scores.table)
        (cf, lf), (cm, lm) = fed.rank.counts(), manual.rank.counts()
        assert torch.equal(cf, cm) and torch.equal(lf, lm) and lf.numel() == N
        scores = {**manual.scores.compute(), **manual.rank.compute()}
        assert scores and all(got[k] == v or (np.isnan(v) and np.isnan(got[k])) for k, v in scores.items())


def oracle_epoch(case, params, srcs, order):
    """The float64 reference stepped over the same order: per-step losses and batch sizes, the parameters after the epoch."""
    if case.name not in _ORACLE:
        ref, rows, o = R.Step(case, params, LR), [], order.cpu()
        host = tuple(t.cpu() for t in srcs)
        for lo in range(0, N, B):
            idx = o[lo:lo + B]
            out = ref.step(tuple(t.index_select(0, idx) for t in host))
            rows.append([float(v) for v in out["losses"]] + [int(idx.numel())])
        _ORACLE[case.name] = (np.array(rows), {k: v.clone() for k, v in ref.p.items()})
    return _ORACLE[case.name]


@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_mimic_and_mmimdb_fed_epoch_against_float64(name, steps, dev):
    case = case_of(name)
    assert case.p == 0.0
    params = G.make_params(R.case_shapes(case), 31)
    srcs, order = split_of(case, N, 302, dev), order_of(N, 18, dev)
    eng = R.engine_class(case)(case.cfg, B, device=dev, precision="fp32", lr=LR, init=False)
    eng.load_state_dict(params)
    with_tail(eng)
    got = fed_epoch(eng, srcs, order, steps)
    rows, p_ref = oracle_epoch(case, params, srcs, order)
    assert got["steps"] == len(rows) == 6 and got["samples"] == N and float(eng.adam_state[0]) == 6.0
    a, b = eng.HEAD_NAMES[:2]
    want = {f"loss_{a}": rows[:, 0].mean(), f"loss_{b}": rows[:, 1].mean(), "loss_fusion": rows[:, 2].mean(),
            "loss_step_mean": rows[:, 3].mean(), "loss": (rows[:, 3] * rows[:, 4]).sum() / N}
    for k, v in want.items():
        print(f"{name} steps {steps} {k}: fed {got[k]:.7g} float64 {v:.7g} abs {abs(got[k] - v):.2e}")
        assert abs(got[k] - v) < FP32_LOSSES, k
    worst = max(float((eng.params[k].double().cpu() - v).abs().max()) for k, v in p_ref.items() if not k.endswith(R.NOISE_KEYS))
    print(f"{name} steps {steps} parameters after the epoch: abs {worst:.2e}")
    assert worst < FP32_PARAMS
    assert ("hits" in got) == (case.engine == "mimic")                     # multilabel predictions have no hit count


def test_fed_evaluation_equals_evaluate_over_the_same_batches(dev):
    from m2_mixer_amd.data import run_epoch_fed
    from m2_mixer_amd.engine import EpochFeed
    case = case_of(AV_CASE)
    srcs, order = split_of(case, NVAL, 303, dev), order_of(NVAL, 19, dev)
    eng = av_engine(case, dev)
    before = eng.flat_p.clone()
    feed = EpochFeed(srcs, B, dev)
    got = run_epoch_fed(eng, feed, None, train=False, order=order, split="val")
    tally, tail = Tally(), eng.sibling(NVAL % B, trains=False)
    for lo in range(0, NVAL, B):
        batch = tuple(t.index_select(0, order[lo:lo + B]) for t in srcs)
        e = eng if batch[-1].numel() == B else tail
        e.evaluate(*batch)
        tally.add(e.losses, e.preds, batch[-1], batch[-1].numel())
    want = tally.result(eng.HEAD_NAMES[:2])
    for k in ("hits", "hits_image", "hits_audio", "steps", "samples"):
        assert got[k] == want[k], k
    assert got["steps"] == 3 and got["samples"] == NVAL and torch.equal(eng.flat_p, before)
    for k in ("loss", "loss_step_mean", "loss_image", "loss_audio", "loss_fusion"):
        assert abs(got[k] - want[k]) / abs(want[k]) < LOSS_REL, k
    # logits of a gathered batch against the same batch handed in: bit-equal
    feed.start(order)
    slots = feed.new_slots()
    for lo in (0, B):
        feed.gather_into(slots)
        eng.evaluate(*slots)
        fed_logits = eng.logits.clone()
        eng.evaluate(*(t.index_select(0, order[lo:lo + B]) for t in srcs))
        assert torch.equal(eng.logits, fed_logits), lo


def test_capture_feed_is_single_gpu_and_sized_like_the_engine(dev):
    from m2_mixer_amd.engine import EpochFeed
    case = case_of(AV_CASE)
    srcs = split_of(case, NVAL, 304, dev)
    eng = av_engine(case, dev)
    with pytest.raises(ValueError, match="gradient exchange"):
        eng.capture_feed(EpochFeed(srcs, B, dev), grad_sync=lambda g: 1.0)
    with pytest.raises(ValueError):
        eng.capture_feed(EpochFeed(srcs, B, dev), steps=0)
    with pytest.raises(ValueError, match="batch size"):
        eng.capture_feed(EpochFeed(srcs, B + 1, dev))
