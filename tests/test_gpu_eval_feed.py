"""Captured evaluation epochs and the prediction record on the engines (-m gpu): engine.capture_feed_eval,
engine.PredictionRecord and data.run_epoch_fed(train=False, replay=, record=).  Every case: batch 8 over a split of 43 samples (five
full batches and a ragged tail of 3) in a shuffled order, as tests/test_gpu_feed_epoch.py.

(a) the golden M2-Mixer-B shape in bf16 and the tests/engine_cases.py entries mimic_patches_7 and mm_token_dim_32 in fp32: the
    eager fed pass with a record against a manual loop of engine.evaluate (record bit-equal to the concatenated clones), then the
    same pass through capture_feed_eval with steps = 1 and steps = 2 (two replays, one eager single, the tail) held to the eager
    pass: record bit-equal, count tables and ranking counts equal, hits / steps / samples equal, losses to 1e-6 relative (the
    heads kernel sums a batch's loss with float atomics); fp32: recorded fusion logits within 1e-3 absolute of the float64
    reference (the fp32 bar of tests/test_gpu_engine_envelope.py).
(b) AVMnistUQEngine: recorded uncertainties bit-equal to evaluate's; the epoch means of a feed built with uncertainty=True are
    EXACTLY equal between the captured and the eager pass: m2m_epoch_accumulate_uq has no atomics and a fixed summation order, and
    the uncertainties it sums are functions of bit-equal logits.
(c) capture_feed_eval leaves no trace, and a training feed graph captured before it still trains to the same bits.
(d) refusals.  (e) bound modules: save_test_preds() from the record against save_test_preds(list)."""
import numpy as np
import pytest
import torch

import engine_ref as R
import gen_util as G
from engine_cases import CASES, Case

pytestmark = pytest.mark.gpu

B, N = 8, 43
CAP = 64
LR = 2e-3
LOSS_REL = 1e-6
FP32_LOGITS = 1e-3                                     # tests/test_gpu_engine_envelope.py BARS["fp32"]["logits"]
AV_CASE = Case("avmnist_B", "avmnist", dict(G.AVMNIST["B"]), B, 0.5, {})
CASE_NAMES = ("avmnist_B", "mimic_patches_7", "mm_token_dim_32")
LOSS_KEYS = ("loss", "loss_step_mean", "loss_fusion")

_PASSES = {}                                           # case name -> the engine, its split and the eager pass: made once, shared


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def case_of(name):
    c = AV_CASE if name == "avmnist_B" else next(c for c in CASES if c.name == name)
    return c._replace(B=B)


def split_of(case, n, seed, dev):
    return tuple(t.to(dev) for t in R.case_batch(case._replace(B=n), seed))


def order_of(n, seed, dev):
    return torch.from_numpy(np.random.default_rng(seed).permutation(n)).to(dev)


def build(case, dev):
    """(engine with scores and, where built, ranking scores; its parameters as loaded, or None for the seeded bf16 engine)."""
    from m2_mixer_amd.engine import AVMnistEngine
    if case.name == "avmnist_B":
        return AVMnistEngine(case.cfg, B, device=dev, precision="bf16", lr=1e-3, seed=9, scores=True, rank_scores=True), None
    params = G.make_params(R.case_shapes(case), 31)
    eng = R.engine_class(case)(case.cfg, B, device=dev, precision="fp32", lr=LR, init=False, scores=True,
                               rank_scores=case.engine == "mimic")
    eng.load_state_dict(params)
    return eng, params


def snapshot(eng, out, rec):
    """What a finished pass left: its result dict, the count table, the ranking counts, the record."""
    torch.cuda.synchronize()
    got = dict(out=out, table=eng.score_table("val").table.clone(), rows=rec.rows(), record=rec.read())
    if eng.rank is not None:
        got["rank"] = eng.rank_buffer("val").counts()
    return got


def passes_of(name, dev):
    if name not in _PASSES:
        from m2_mixer_amd.data import run_epoch_fed
        from m2_mixer_amd.engine import EpochFeed
        case = case_of(name)
        eng, params = build(case, dev)
        srcs, order = split_of(case, N, 311, dev), order_of(N, 23, dev)
        feed, tail, rec = EpochFeed(srcs, B, dev), eng.sibling(N % B, trains=False), eng.prediction_record("val", CAP)
        out = run_epoch_fed(eng, feed, None, train=False, order=order, split="val", record=rec, tail_engine=tail)
        _PASSES[name] = dict(case=case, eng=eng, params=params, srcs=srcs, order=order, feed=feed, tail=tail, rec=rec,
                             eager=snapshot(eng, out, rec))
    return _PASSES[name]


def same_record(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), f"{what}: {k}"


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_eager_pass_records_what_evaluate_gives(name, dev):
    P = passes_of(name, dev)
    eng, tail, srcs, order, eager = P["eng"], P["tail"], P["srcs"], P["order"], P["eager"]
    assert eager["rows"] == N and eager["out"]["steps"] == 6 and eager["out"]["samples"] == N
    lg, pr, lb = [], [], []
    for lo in range(0, N, B):
        batch = tuple(t.index_select(0, order[lo:lo + B]) for t in srcs)
        e = eng if batch[-1].shape[0] == B else tail
        e.evaluate(*batch)
        lg.append(e.logits.clone()), pr.append(e.preds.clone()), lb.append(batch[-1].clone())
    logits, preds, labels = torch.cat(lg, dim=1).cpu(), torch.cat(pr, dim=1).cpu(), torch.cat(lb).cpu()
    names = P["rec"].names
    want = dict(zip(names["logits"], logits.unbind(0)), labels=labels)
    want.update(zip(names["preds"], (torch.softmax(logits, dim=2) if P["case"].engine == "mimic" else preds.long()).unbind(0)))
    same_record(eager["record"], want, f"{name}: record against the manual loop")
    assert set(eager["record"]) == set(names["logits"]) | set(names["preds"]) | {"labels"}
    if P["params"] is not None:
        # fp32: the recorded fusion logits against the float64 reference over the same rows, in arrival order
        host = tuple(t.index_select(0, order).cpu() for t in srcs)
        ref = R.case_forward(P["case"], host, {k: v.double() for k, v in P["params"].items()})["logits"][2]
        err = float((eager["record"]["logits"].double() - ref).abs().max())
        print(f"{name}: recorded fusion logits against float64: abs {err:.2e}")
        assert err < FP32_LOGITS


@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_captured_pass_is_the_eager_pass(name, steps, dev):
    from m2_mixer_amd.data import feed_plan, run_epoch_fed
    P = passes_of(name, dev)
    eng, feed, rec, eager = P["eng"], P["feed"], P["rec"], P["eager"]
    table = eng.score_table("val")
    rank = eng.rank_buffer("val") if eng.rank is not None else None
    replay = eng.capture_feed_eval(feed, steps=steps, scores=table, rank=rank, record=rec)
    assert replay.eval is True and replay.steps == steps and replay.feed is feed and len(replay.slots) == steps
    assert feed_plan(N, B, steps) == ((5, 0, 3) if steps == 1 else (2, 1, 3))
    out = run_epoch_fed(eng, feed, replay, train=False, order=P["order"], split="val", record=rec, tail_engine=P["tail"])
    got = snapshot(eng, out, rec)
    assert got["rows"] == N
    same_record(got["record"], eager["record"], f"{name} steps {steps}: record against the eager pass")
    assert torch.equal(got["table"], eager["table"]) and int(got["table"].sum()) > 0
    if rank is not None:
        (cg, lg), (ce, le) = got["rank"], eager["rank"]
        assert torch.equal(cg, ce) and torch.equal(lg, le) and lg.numel() == N
    a, b = eng.HEAD_NAMES[:2]
    exact = [k for k in eager["out"] if not k.startswith("loss")]
    assert {"steps", "samples"} <= set(exact)
    if P["case"].engine != "mmimdb":
        assert {"hits", f"hits_{a}", f"hits_{b}", "acc"} <= set(exact)
    for k in exact:                                                        # hits, steps, samples and every score of the tables
        v = eager["out"][k]
        assert out[k] == v or (np.isnan(v) and np.isnan(out[k])), k
    for k in LOSS_KEYS + (f"loss_{a}", f"loss_{b}"):
        rel = abs(out[k] - eager["out"][k]) / abs(eager["out"][k])
        print(f"{name} steps {steps} {k}: captured {out[k]:.9g} eager {eager['out'][k]:.9g} rel {rel:.2e}")
        assert rel < LOSS_REL, k


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
def test_the_evidential_engine_records_its_uncertainties(dev):
    from m2_mixer_amd.data import run_epoch_fed
    from m2_mixer_amd.engine import AVMnistUQEngine, EpochFeed
    case = case_of("avmnist_B")
    eng = AVMnistUQEngine(case.cfg, B, device=dev, precision="bf16", lr=1e-3, seed=9, scores=True)
    srcs, order = split_of(case, N, 312, dev), order_of(N, 24, dev)
    feed, tail, rec = EpochFeed(srcs, B, dev, uncertainty=True), eng.sibling(N % B, trains=False), eng.prediction_record("val", CAP)
    assert rec.uncertainty is not None
    eager_out = run_epoch_fed(eng, feed, None, train=False, order=order, split="val", record=rec, tail_engine=tail)
    eager = rec.read()
    un, pr = [], []
    for lo in range(0, N, B):
        batch = tuple(t.index_select(0, order[lo:lo + B]) for t in srcs)
        e = eng if batch[-1].shape[0] == B else tail
        e.evaluate(*batch)
        un.append(e.uncertainty.clone()), pr.append(e.preds.clone())
    unc, preds = torch.cat(un, dim=1).cpu(), torch.cat(pr, dim=1).cpu().long()
    for h, k in enumerate(("uncertainty_image", "uncertainty_audio", "uncertainty")):
        assert torch.equal(eager[k], unc[h]) and eager[k].dtype == torch.float32, k
    assert torch.equal(eager["preds"], preds[2])                           # the combined prediction
    replay = eng.capture_feed_eval(feed, steps=2, scores=eng.score_table("val"), record=rec)
    out = run_epoch_fed(eng, feed, replay, train=False, order=order, split="val", record=rec, tail_engine=tail)
    same_record(rec.read(), eager, "UQ: captured record against the eager pass")
    for k in ("uncertainty", "uncertainty_image", "uncertainty_audio"):    # no atomics, a fixed order: exactly equal
        assert out[k] == eager_out[k] and out[k] > 0.0, k
    for k in LOSS_KEYS:
        assert abs(out[k] - eager_out[k]) / abs(eager_out[k]) < LOSS_REL, k
    with pytest.raises(RuntimeError, match="ranking buffers"):
        eng.evaluate(*feed.new_slots(), rank=object(), record=rec)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
def av_train_engine(case, dev):
    from m2_mixer_amd.engine import AVMnistEngine
    return AVMnistEngine(case.cfg, B, device=dev, precision="bf16", lr=1e-3, seed=9, scores=True, rank_scores=True)


def test_capture_feed_eval_leaves_no_trace(dev):
    from m2_mixer_amd.engine import EpochFeed
    case = case_of("avmnist_B")
    eng = av_train_engine(case, dev)
    srcs, order = split_of(case, N, 313, dev), order_of(N, 25, dev)
    for lo in (0, B):                                                      # non-zero Adam moments and counters
        eng.train_step(*(t.index_select(0, order[lo:lo + B]) for t in srcs))
    feed = EpochFeed(srcs, B, dev)
    table, rank, rec = eng.score_table("val"), eng.rank_buffer("val"), eng.prediction_record("val", CAP)
    feed.start(order)
    slots = feed.new_slots()
    for _ in range(2):                                                     # a non-empty table, ranking buffer, record and feed
        feed.gather_into(slots)
        eng.evaluate(*slots, scores=table, rank=rank, record=rec)
        feed.accumulate(eng, slots[-1])
    watched = dict(flat_p=eng.flat_p, flat_m=eng.flat_m, flat_v=eng.flat_v, adam_state=eng.adam_state, drop_step=eng.drop_step,
                   feed_state=feed.state, feed_acc=feed._acc, table=table.table, rank_state=rank.state, record_state=rec.state,
                   train_table=eng.scores.table, train_rank_state=eng.rank.state)
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in watched.items()}
    assert rec.rows() == 2 * B and feed.rows() == 2 * B and int(table.table.sum()) > 0 and float(eng.adam_state[0]) == 2.0
    replay = eng.capture_feed_eval(feed, steps=2, scores=table, rank=rank, record=rec)
    torch.cuda.synchronize()
    for k, v in watched.items():
        assert torch.equal(v, before[k]), f"{k} changed under capture_feed_eval"
    replay()                                                               # and the graph does append: two more steps
    assert rec.rows() == 4 * B and feed.rows() == 4 * B
    for k in ("flat_p", "flat_m", "flat_v", "adam_state", "drop_step"):
        assert torch.equal(watched[k], before[k]), f"{k} changed under an evaluation replay"


def test_a_training_feed_graph_survives_an_evaluation_capture(dev):
    from m2_mixer_amd.data import run_epoch_fed
    from m2_mixer_amd.engine import EpochFeed
    case = case_of("avmnist_B")
    srcs, order = split_of(case, N, 314, dev), order_of(N, 26, dev)
    vsrcs = split_of(case, 2 * B, 315, dev)
    engines = []
    for captures_eval in (False, True):
        eng = av_train_engine(case, dev)
        feed = EpochFeed(srcs, B, dev)
        replay = eng.capture_feed(feed, steps=1)
        if captures_eval:
            vfeed = EpochFeed(vsrcs, B, dev)
            rec = eng.prediction_record("val", CAP)
            ev = eng.capture_feed_eval(vfeed, steps=2, scores=eng.score_table("val"), rank=eng.rank_buffer("val"), record=rec)
            run_epoch_fed(eng, vfeed, ev, train=False, split="val", record=rec)
            assert rec.rows() == 2 * B
        out = run_epoch_fed(eng, feed, replay, 4 * B, order=order)            # four captured training steps, no tail
        assert out["steps"] == 4
        engines.append(eng)
    torch.cuda.synchronize()
    plain, mixed = engines
    for k in ("flat_p", "flat_m", "flat_v", "adam_state", "drop_step"):
        assert torch.equal(getattr(plain, k), getattr(mixed, k)), f"{k} differs after an evaluation capture"
    assert float(mixed.adam_state[0]) == 4.0


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from m2_mixer_amd.data import run_epoch_fed
    from m2_mixer_amd.engine import EpochFeed
    P = passes_of("mimic_patches_7", dev)
    eng, feed, rec, order, tail = P["eng"], P["feed"], P["rec"], P["order"], P["tail"]
    table, rank = eng.score_table("val"), eng.rank_buffer("val")
    ev = eng.capture_feed_eval(feed, scores=table, rank=rank, record=rec)
    with pytest.raises(ValueError, match="train=True takes a training graph"):
        run_epoch_fed(eng, feed, ev, train=True, order=order)
    tr = eng.capture_feed(feed)
    with pytest.raises(ValueError, match="train=False takes an evaluation graph"):
        run_epoch_fed(eng, feed, tr, train=False, order=order, split="val", record=rec)
    other = eng.new_prediction_record(CAP)
    with pytest.raises(ValueError, match="another record"):
        run_epoch_fed(eng, feed, ev, train=False, order=order, split="val", record=other, tail_engine=tail)
    with pytest.raises(ValueError, match="another record"):
        run_epoch_fed(eng, feed, ev, train=False, order=order, split="val", tail_engine=tail)
    with pytest.raises(ValueError, match="another scores"):
        run_epoch_fed(eng, feed, ev, train=False, order=order, split="test", record=rec, tail_engine=tail)
    with pytest.raises(ValueError, match="another feed"):
        run_epoch_fed(eng, EpochFeed(P["srcs"], B, dev), ev, train=False, order=order, split="val", record=rec, tail_engine=tail)
    with pytest.raises(ValueError, match="gradient exchange"):
        eng.capture_feed_eval(feed, grad_sync=lambda g: 1.0)
    with pytest.raises(ValueError):
        eng.capture_feed_eval(feed, steps=0)
    with pytest.raises(RuntimeError, match=f"holds {CAP} rows"):
        eng.prediction_record("val", CAP + 1)
    with pytest.raises(RuntimeError, match="first use"):
        eng.prediction_record("never_made")
    with pytest.raises(RuntimeError, match="labels"):
        rec.add(eng, feed.new_slots()[-1].int())
    # a record smaller than the split: read() names both numbers, the rows below the capacity are still right
    small = eng.new_prediction_record(20)
    run_epoch_fed(eng, feed, None, train=False, order=order, split="val", record=small, tail_engine=tail)
    with pytest.raises(RuntimeError, match=rf"capacity 20 rows, {N} rows seen"):
        small.read()
    assert small.rows() == N and small.dropped == N - 20
    full = P["eager"]["record"]
    assert torch.equal(small.logits[2, :20].cpu(), full["logits"][:20]) and torch.equal(small.labels[:20].cpu(), full["labels"][:20])
    assert torch.equal(small.logits[0, :20].cpu(), full["logits_static"][:20])


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------
def _model_cfg(task, c):
    a, b = ("image", "audio") if task == "avmnist" else ("image", "text")
    mods = {a: dict(c[a], block_type="MLPMixer"), b: dict(c[b], block_type="MLPMixer")}
    mods["multimodal"] = dict(c["multimodal"], block_type="FusionMixer", fusion_function="ConcatFusion")
    mods["classification"] = dict(classifier="StandardClassifier", num_classes=c["num_classes"],
                                  input_shape=[16, 49, c["multimodal"]["hidden_dim"]])
    cfg = {"dropout": c["dropout"], "modalities": mods}
    if task == "mmimdb":
        cfg["pos_weight"] = c["pos_weight"]
    return cfg


def make_net(task, c, seed, dev):
    from m2_mixer_amd import models as MD
    cls = {"avmnist": MD.AVMnistMixerMultiLoss, "mmimdb": MD.MMIMDBMixerMultiLoss}[task]
    shapes = {"avmnist": G.avmnist_shapes, "mmimdb": G.mmimdb_shapes}[task](c)
    net = cls(_model_cfg(task, c), {"lr": 1e-3, "betas": (0.9, 0.999), "scheduler_patience": 1}).to(dev)
    net.load_state_dict(dict(G.make_params(shapes, seed)), strict=False)
    return net


def module_batch(task, bs, seed, c, dev):
    xa, xb, labels = (G.avmnist_batch if task == "avmnist" else G.mmimdb_batch)(bs, seed, c)
    a, b = ("image", "audio") if task == "avmnist" else ("image", "text")
    return {a: xa.to(dev), b: xb.to(dev), "label": labels.to(dev)}


@pytest.mark.parametrize("task", ["avmnist", "mmimdb"])
def test_a_bound_module_dumps_its_test_predictions_from_the_record(task, dev, tmp_path):
    c = dict(G.AVMNIST["S"], dropout=0.0) if task == "avmnist" else dict(next(x for x in CASES if x.name == "mm_token_dim_32").cfg)
    net = make_net(task, c, 52, dev)
    eng = net.bind_engine(8, precision="fp32", scores=True, test_record=True, record_capacity=CAP)
    outs = [net.test_step(module_batch(task, bs, 80 + i, c, dev), i) for i, bs in enumerate((8, 8, 3))]
    assert eng.prediction_record("test").rows() == 19
    from_list = torch.load(net.save_test_preds(outs, save_dir=str(tmp_path / "list")))
    from_record = torch.load(net.save_test_preds(save_dir=str(tmp_path / "record")))
    assert tuple(from_record) == net.TEST_PRED_KEYS and set(from_list) == set(from_record)
    for k in net.TEST_PRED_KEYS:
        assert from_record[k].dtype == from_list[k].dtype and torch.equal(from_record[k], from_list[k]), k
    assert from_record["preds"].shape[0] == 19
    assert eng.prediction_record("test").rows() == 0                       # emptied for the next test pass
    plain = make_net(task, c, 52, dev)
    with pytest.raises(RuntimeError, match="not bound"):
        plain.save_test_preds(save_dir=str(tmp_path))
    plain.bind_engine(8, precision="fp32")
    plain.test_step(module_batch(task, 8, 80, c, dev), 0)
    with pytest.raises(RuntimeError, match="test_record=True"):
        plain.save_test_preds(save_dir=str(tmp_path))
