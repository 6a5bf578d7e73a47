"""GPU tests (-m gpu) of the device-side score tables: every comparison is exact integer equality against tables built by plain
loops on the host (tests/scores_ref.py) from the `preds` / `labels` the steps held; the derived numbers are compared with the
numpy restatement on those same host tables.

  * m2m_scores_multiclass / m2m_scores_multilabel on random inputs over the accepted K range and ragged B, accumulation over
    calls, rows outside [0, K), the refused K;
  * AVMnistEngine / MMIMDBEngine / MimicEngine with scores=True: captured replays (one- and three-step graphs), a ragged batch
    through a training sibling, reset() between replays, evaluate(..., scores=table);
  * scores off (the default): no table, and logits / gradients / parameters bit-identical to scores on, in bf16;
  * the bound task modules' epoch-end hooks and data.run_epoch.
"""
import numpy as np
import pytest
import torch

import gen_util as G
import scores_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _mc_table(nheads, K, dev):
    return torch.zeros(nheads, K * K + 1, dtype=torch.int64, device=dev)


def _run_mc(preds, labels, K, table):
    from m2_mixer_amd import _lib as L
    nh, B = preds.shape
    L.check(L.lib().m2m_scores_multiclass(preds.data_ptr(), labels.data_ptr(), nh, B, K, table.data_ptr(), L.stream_ptr()), "scores")


def _run_ml(preds, targets, K, table):
    from m2_mixer_amd import _lib as L
    nh, B = preds.shape[:2]
    L.check(L.lib().m2m_scores_multilabel(preds.data_ptr(), targets.data_ptr(), nh, B, K, table.data_ptr(), L.stream_ptr()), "scores")


def _host_mc(preds, labels, K):
    """(nheads, K * K + 1) int64 from plain loops."""
    out = []
    for h in range(preds.shape[0]):
        cm, skipped = R.confusion_matrix(preds[h].cpu().numpy(), labels.cpu().numpy(), K)
        out.append(np.concatenate([cm.reshape(-1), [skipped]]))
    return np.stack(out).astype(np.int64)


def _host_ml(preds, targets, K):
    return np.stack([R.multilabel_table(preds[h].cpu().numpy(), targets.cpu().numpy(), K) for h in range(preds.shape[0])])


# ---------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 37, 512, 2500])
@pytest.mark.parametrize("K", [2, 6, 10, 64])
def test_multiclass_table_equals_the_plain_loop(K, B, dev):
    gen = torch.Generator().manual_seed(1000 * K + B)
    nh = 3
    total = np.zeros((nh, K * K + 1), dtype=np.int64)
    table = _mc_table(nh, K, dev)
    for call in range(2):                                       # two calls in a row add up
        preds = torch.randint(0, K, (nh, B), generator=gen, dtype=torch.int32).to(dev)
        labels = torch.randint(0, K, (B,), generator=gen, dtype=torch.int64).to(dev)
        _run_mc(preds, labels, K, table)
        total += _host_mc(preds, labels, K)
        got = table.cpu().numpy()
        assert np.array_equal(got, total), (K, B, call)
    assert got[:, :-1].sum() == 2 * nh * B and (got[:, -1] == 0).all()


@pytest.mark.parametrize("B", [1, 37, 512, 2500])
@pytest.mark.parametrize("K", [1, 23, 128])
def test_multilabel_table_equals_the_plain_loop(K, B, dev):
    gen = torch.Generator().manual_seed(2000 * K + B)
    nh = 3
    total = np.zeros((nh, K, 4), dtype=np.int64)
    table = torch.zeros(nh, K, 4, dtype=torch.int64, device=dev)
    for call in range(2):
        preds = (torch.rand(nh, B, K, generator=gen) < 0.3).to(torch.int32).to(dev)
        targets = (torch.rand(B, K, generator=gen) < 0.25).float().to(dev)
        _run_ml(preds, targets, K, table)
        total += _host_ml(preds, targets, K)
        got = table.cpu().numpy()
        assert np.array_equal(got, total), (K, B, call)
    assert got.sum() == 2 * nh * B * K


def test_out_of_range_rows_land_in_skipped_only(dev):
    K, B, nh = 10, 300, 3
    gen = torch.Generator().manual_seed(5)
    preds = torch.randint(0, K, (nh, B), generator=gen, dtype=torch.int32)
    labels = torch.randint(0, K, (B,), generator=gen, dtype=torch.int64)
    labels[3], labels[50], labels[299] = -1, K, 2 ** 40         # rows every head skips
    preds[0, 7], preds[1, 8], preds[2, 9], preds[2, 10] = -1, K, 2 ** 31 - 1, -(2 ** 31)
    # guard cells on both sides of the table: nothing may be written outside it
    buf = torch.full((nh * (K * K + 1) + 16,), -7, dtype=torch.int64, device=dev)
    table = buf[8:-8].view(nh, K * K + 1)
    table.zero_()
    _run_mc(preds.to(dev), labels.to(dev), K, table)
    want = _host_mc(preds, labels, K)
    assert want[:, -1].tolist() == [4, 4, 5]
    assert np.array_equal(table.cpu().numpy(), want)
    assert (buf[:8] == -7).all() and (buf[-8:] == -7).all()
    # multilabel: any non-zero prediction counts as predicted, a target counts as positive from 0.5 on
    Kl = 5
    p = torch.tensor([[[0, 1, -3, 7, 0]]], dtype=torch.int32).to(dev)
    t = torch.tensor([[0.49, 0.5, 1.0, 0.0, float("nan")]]).to(dev)
    tab = torch.zeros(1, Kl, 4, dtype=torch.int64, device=dev)
    _run_ml(p, t, Kl, tab)
    assert tab.cpu()[0].tolist() == [[0, 0, 0, 1], [1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]]


def test_a_k_past_the_limit_is_refused_by_name(dev):
    from m2_mixer_amd import _lib as L
    from m2_mixer_amd.engine import ScoreTable
    B, nh = 8, 3
    for K, ml, word in ((L.SCORES_MAX_CLASSES + 1, False, "M2M_SCORES_MAX_CLASSES"), (L.SCORES_MAX_LABELS + 1, True, "M2M_SCORES_MAX_LABELS")):
        table = torch.zeros(nh, K * 4 if ml else K * K + 1, dtype=torch.int64, device=dev)
        preds = torch.zeros((nh, B, K) if ml else (nh, B), dtype=torch.int32, device=dev)
        truth = torch.zeros(B, K, device=dev) if ml else torch.zeros(B, dtype=torch.int64, device=dev)
        with pytest.raises(RuntimeError, match=word):
            (_run_ml if ml else _run_mc)(preds, truth, K, table)
        assert int(table.sum()) == 0
        with pytest.raises(RuntimeError, match="scores kernel takes"):
            ScoreTable("mmimdb" if ml else "avmnist", ("a", "b", "fusion"), K, dev)
    # the limits themselves are accepted (the K = 64 / 128 cases above run them)


# ---------------------------------------------------------------------------------------------------------------
# the engines
# ---------------------------------------------------------------------------------------------------------------
def _make(task, B, dev, scores, precision="bf16", cfg=None, **kw):
    from m2_mixer_amd.engine import AVMnistEngine, MimicEngine, MMIMDBEngine
    cls, c = {"avmnist": (AVMnistEngine, G.AVMNIST["B"]), "mimic": (MimicEngine, G.MIMIC_H), "mmimdb": (MMIMDBEngine, G.MMIMDB)}[task]
    return cls(cfg or c, B, device=dev, precision=precision, lr=1e-3, seed=42, scores=scores, **kw), (cfg or c)


def _batch(task, B, seed, c, dev):
    fn = {"avmnist": G.avmnist_batch, "mimic": G.mimic_batch, "mmimdb": G.mmimdb_batch}[task]
    return tuple(t.to(dev) for t in fn(B, seed, c))


def _host_counts(task, K, steps):
    """Per-head count tables of [(preds, truth), ...] as ScoreTable.counts() lays them out."""
    if task == "mmimdb":
        return sum(_host_ml(p, t, K) for p, t in steps)
    return sum(_host_mc(p, t, K)[:, :-1].reshape(-1, K, K) for p, t in steps)


@pytest.mark.parametrize("task,B,tail", [("avmnist", 64, 5), ("mmimdb", 32, 3), ("mimic", 128, 17)])
def test_training_table_equals_the_host_tables_of_the_steps(task, B, tail, dev):
    """Capture, four replays with different batches, one ragged batch through a training sibling (it shares the table), one
    more replay: the training table is the sum of the per-step host tables.  bf16, the cfg's dropout (0.5 / 0.5 / 0.3)."""
    eng, c = _make(task, B, dev, scores=True)
    K = c["num_classes"]
    assert eng.scores is not None and eng.scores.kind == ("multilabel" if task == "mmimdb" else "multiclass")
    sib = eng.sibling(tail)                                     # before capture()
    assert sib.scores is eng.scores
    replay = eng.capture(*_batch(task, B, 1, c, dev))
    assert int(eng.scores.table.sum()) == 0, "capture() must not leave its warm-up steps in the table"
    steps = []
    for i in range(4):
        b = _batch(task, B, 10 + i, c, dev)
        replay(*b)
        steps.append((eng.preds.clone(), b[-1]))
    b = _batch(task, tail, 20, c, dev)
    sib.pack()
    sib.train_step(*b)
    eng.pack()
    steps.append((sib.preds.clone(), b[-1]))
    b = _batch(task, B, 21, c, dev)
    replay(*b)
    steps.append((eng.preds.clone(), b[-1]))
    torch.cuda.synchronize()
    want = _host_counts(task, K, steps)
    got = eng.scores.counts().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    n = 5 * B + tail
    assert got.sum() == 3 * n * (K if task == "mmimdb" else 1)
    if task != "mmimdb":
        assert eng.scores.skipped.tolist() == [0, 0, 0]
    # the derived numbers: the engine's names against the numpy restatement on the host tables
    scores, ref = eng.scores.compute(), R.task(task, want, eng.HEAD_NAMES)
    assert set(scores) == set(ref)
    for k in ref:
        assert abs(scores[k] - ref[k]) <= 1e-12, k
    # reset() between replays, no re-capture: only the later steps are in the table
    eng.scores.reset()
    later = []
    for i in range(2):
        b = _batch(task, B, 30 + i, c, dev)
        replay(*b)
        later.append((eng.preds.clone(), b[-1]))
    torch.cuda.synchronize()
    assert np.array_equal(eng.scores.counts().numpy(), _host_counts(task, K, later))


def test_three_step_graph_counts_every_step(dev):
    B, task = 64, "avmnist"
    eng, c = _make(task, B, dev, scores=True)
    bs = [_batch(task, B, 40 + i, c, dev) for i in range(6)]
    replay = eng.capture(*bs[0], steps=3)
    assert int(eng.scores.table.sum()) == 0
    steps = []
    for r in range(2):
        flat = [t for b in bs[3 * r:3 * r + 3] for t in b]
        replay(*flat)
        steps += [(eng.preds_steps[i].clone(), bs[3 * r + i][-1]) for i in range(3)]
    torch.cuda.synchronize()
    assert np.array_equal(eng.scores.counts().numpy(), _host_counts(task, 10, steps))


def test_evaluate_adds_into_the_table_it_is_given(dev):
    B, task = 16, "avmnist"
    cfg = G.AVMNIST["S"]
    eng, c = _make(task, B, dev, scores=True, precision="fp32", cfg=cfg)
    val, test = eng.score_table("val"), eng.score_table("test")
    assert val is not test and val is not eng.scores and eng.score_table("val") is val and eng.score_table("train") is eng.scores
    sv, st = [], []
    for i in range(3):
        b = _batch(task, B, 50 + i, c, dev)
        eng.evaluate(*b, scores=val)
        sv.append((eng.preds.clone(), b[-1]))
    b = _batch(task, B, 60, c, dev)
    eng.evaluate(*b, scores=test)
    st.append((eng.preds.clone(), b[-1]))
    eng.evaluate(*_batch(task, B, 61, c, dev))                  # no table given: counted nowhere
    torch.cuda.synchronize()
    assert np.array_equal(val.counts().numpy(), _host_counts(task, 10, sv))
    assert np.array_equal(test.counts().numpy(), _host_counts(task, 10, st))
    assert int(eng.scores.table.sum()) == 0


def test_scores_off_is_the_default_and_allocates_nothing(dev):
    from m2_mixer_amd.engine import AVMnistEngine
    eng = AVMnistEngine(G.AVMNIST["S"], 8, device=dev, precision="bf16")
    assert eng.scores is None and "_split_scores" not in eng.__dict__
    assert eng.sibling(3).scores is None
    with pytest.raises(RuntimeError, match="scores=False"):
        eng.score_table("train")


def _relerr(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("B", [64, 128])
def test_scores_on_and_off_are_bit_identical(B, dev):
    """Same seed, same batches, bf16, dropout 0.5, M2-Mixer-B (the configuration whose training is bit-reproducible:
    tests/test_gpu_parity.py test_bf16_training_is_bit_reproducible): the scores launch only reads.  Logits, predictions and
    every gradient after forward_backward, then logits, predictions, parameters and both Adam moments after captured replays
    are BIT-identical between scores on and off.
    The reported losses are held to 1e-6 relative instead, as in that test: the heads kernel sums them over its workgroups with
    float atomics (B / 4 or more adds per head in arrival order), so two runs of the SAME engine differ in their last bits with
    or without this feature; whether they came out equal is printed."""
    task = "avmnist"
    on, c = _make(task, B, dev, scores=True)
    off, _ = _make(task, B, dev, scores=False)
    assert off.scores is None and torch.equal(on.flat_p, off.flat_p)
    b = _batch(task, B, 70, c, dev)
    for e in (on, off):
        e.forward_backward(*b)
    torch.cuda.synchronize()
    differing = [k for k in on.grads if not torch.equal(on.grads[k], off.grads[k])]
    assert not differing and float(on.flat_g.abs().sum()) > 0, differing
    assert torch.equal(on.logits, off.logits) and torch.equal(on.preds, off.preds)
    print(f"B={B}: losses after forward_backward bit-equal: {torch.equal(on.losses, off.losses)}, rel {_relerr(on.losses, off.losses):.2e}")
    assert _relerr(on.losses, off.losses) < 1e-6
    for e in (on, off):
        e.optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(on.flat_p, off.flat_p)
    on.scores.reset()
    r_on, r_off = on.capture(*b), off.capture(*b)
    for i in range(3):
        b = _batch(task, B, 71 + i, c, dev)
        r_on(*b)
        r_off(*b)
        torch.cuda.synchronize()
        assert torch.equal(on.logits, off.logits) and torch.equal(on.preds, off.preds), i
        print(f"B={B} replay {i}: losses bit-equal: {torch.equal(on.losses, off.losses)}, rel {_relerr(on.losses, off.losses):.2e}")
        assert _relerr(on.losses, off.losses) < 1e-6
    assert torch.equal(on.flat_p, off.flat_p) and torch.equal(on.flat_m, off.flat_m) and torch.equal(on.flat_v, off.flat_v)
    assert int(on.scores.counts().sum()) == 3 * 3 * B


# ---------------------------------------------------------------------------------------------------------------
# the task modules and the epoch loop
# ---------------------------------------------------------------------------------------------------------------
def _module_batch(task, B, seed, c, dev):
    b = _batch(task, B, seed, c, dev)
    if task == "mimic":
        return b
    a, m = ("image", "audio") if task == "avmnist" else ("image", "text")
    return {a: b[0], m: b[1], "label": b[2]}


@pytest.mark.parametrize("task,B,tail", [("avmnist", 16, 5), ("mmimdb", 32, 3), ("mimic", 128, 7)])
def test_bound_module_epoch_end_hooks(task, B, tail, dev):
    """An epoch of training / validation / test steps with a ragged tail, then the three epoch-end hooks: the fusion head's
    values equal the numpy restatement on the concatenated per-step outputs; a second epoch starts from zero; the loss-weight
    schedule still runs in validation_epoch_end."""
    from test_gpu_engine_backed import make_net
    c = {"avmnist": dict(G.AVMNIST["S"], dropout=0.5), "mimic": G.MIMIC_H, "mmimdb": G.MMIMDB}[task]
    K = c["num_classes"]
    extra = {} if task == "mmimdb" else {"fusion_loss_change": 0.05}
    net, _ = make_net(task, c, 301, dev, **extra)
    eng = net.bind_engine(B, precision="bf16", scores=True)
    assert eng.scores is not None
    names = R.NAMES[task]

    def fusion_table(outs):
        if task == "mmimdb":
            return sum(R.multilabel_table(o["preds"].cpu().numpy(), o["labels"].cpu().numpy(), K) for o in outs)
        # MIMIC's `preds` are the fusion head's probabilities (models/mimic.py:126): the class is their argmax
        cls = [(o["preds"].argmax(dim=1) if o["preds"].dim() == 2 else o["preds"]) for o in outs]
        return sum(R.confusion_matrix(p.cpu().numpy(), o["labels"].cpu().numpy(), K)[0] for p, o in zip(cls, outs))

    def check(got, outs, split):
        fn = R.multilabel if task == "mmimdb" else R.multiclass
        want = fn(fusion_table(outs))
        for name, key in names.items():
            assert abs(got[f"{split}_{name}"] - want[key]) <= 1e-12, (split, name)
        heads = eng.HEAD_NAMES
        assert set(got) == {f"{split}_{n}" for n in names} | {f"{split}_{n}_{h}" for n in names for h in heads[:2]}
        assert all(isinstance(v, float) for v in got.values())

    w0 = net.fusion_loss_weight
    for epoch in range(2):
        net.current_epoch = epoch
        sizes = [B, B, tail, B] if epoch == 0 else [B, tail]
        tr = [net.training_step(_module_batch(task, n, 400 + 10 * epoch + i, c, dev), i) for i, n in enumerate(sizes)]
        va = [net.validation_step(_module_batch(task, n, 500 + 10 * epoch + i, c, dev), i) for i, n in enumerate([B, tail])]
        te = [net.test_step(_module_batch(task, n, 600 + 10 * epoch + i, c, dev), i) for i, n in enumerate([tail, B, B])]
        assert set(tr[0]) >= {"loss", "preds", "labels"} and "logits" in va[0]
        check(net.training_epoch_end(tr), tr, "train")
        check(net.validation_epoch_end(va), va, "val")
        check(net.test_epoch_end(te), te, "test")
        for split in ("train", "val", "test"):
            assert int(eng.score_table(split).table.sum()) == 0, "an epoch-end hook resets its table"
    if task == "mmimdb":
        assert net.fusion_loss_weight == w0
    else:
        assert abs(net.fusion_loss_weight - (w0 + 0.10)) < 1e-12 and abs(eng.fusion_loss_weight - net.fusion_loss_weight) < 1e-12


def test_bind_engine_without_the_argument_adds_nothing(dev):
    from test_gpu_engine_backed import make_net
    c = G.AVMNIST["S"]
    net, _ = make_net("avmnist", c, 302, dev)
    eng = net.bind_engine(8, precision="bf16")
    assert eng.scores is None
    net.training_step(_module_batch("avmnist", 8, 1, c, dev), 0)
    net.validation_step(_module_batch("avmnist", 8, 2, c, dev), 0)
    net.test_step(_module_batch("avmnist", 3, 3, c, dev), 0)
    assert eng.scores is None and "_split_scores" not in eng.__dict__
    assert all(s.scores is None and "_split_scores" not in s.__dict__ for s in net._eval_siblings.values())
    assert net.training_epoch_end([]) is None and net.validation_epoch_end([]) is None and net.test_epoch_end([]) is None
    assert net.to_engine(8, precision="bf16").scores is None and net.to_engine(8, precision="bf16", scores=True).scores is not None


def test_run_epoch_reports_the_table_scores(dev, tmp_path):
    from test_host_cpu import _write_avmnist
    from m2_mixer_amd.data import ResidentAVMnist, prepare_tail_engine, run_epoch
    from m2_mixer_amd.engine import AVMnistEngine
    root = str(tmp_path / "avmnist")
    _write_avmnist(root, 300, 37, seed=5, learnable=True)           # train 275, val 25, test 37
    data = ResidentAVMnist(root, device=dev)
    cfg, B = dict(G.AVMNIST["S"], dropout=0.1), 16
    eng = AVMnistEngine(cfg, B, device=dev, precision="bf16", lr=1e-3, scores=True)
    assert prepare_tail_engine(eng, data, "train", B).scores is eng.scores
    replay = eng.capture(*next(iter(data.batches("train", B))))
    # the keys run_epoch returns without scores
    base = {"loss", "loss_step_mean", "loss_image", "loss_audio", "loss_fusion", "acc", "acc_image", "acc_audio", "hits", "hits_image",
            "hits_audio", "steps", "samples"}
    for epoch in range(2):
        tr = run_epoch(eng, data, "train", B, train=True, replay=replay)
        assert set(tr) >= base and tr["steps"] == 18 and tr["samples"] == 275
        assert set(tr) - base == {n + s for n in R.NAMES["avmnist"] for s in ("", "_image", "_audio")} - base
        cm = eng.score_table("train").counts().numpy()
        assert cm.sum() == 3 * 275, "the table holds this epoch only"
        want = R.task("avmnist", cm, eng.HEAD_NAMES)
        assert tr["acc"] == want["acc"] == tr["hits"] / 275 and tr["acc_image"] == want["acc_image"] and tr["acc_audio"] == want["acc_audio"]
        assert [int(np.trace(cm[h])) for h in range(3)] == [tr["hits_image"], tr["hits_audio"], tr["hits"]]
        for k in ("f1m", "prec_m", "rec_m", "f1mi", "prec_mi", "rec_mi"):
            assert abs(tr[k] - want[k]) <= 1e-12, k
        for split, n in (("val", 25), ("test", 37)):
            ev = run_epoch(eng, data, split, B, train=False)
            cm = eng.score_table(split).counts().numpy()
            assert cm.sum() == 3 * n and ev["acc"] == R.multiclass(cm[2])["acc"] == ev["hits"] / n
            assert abs(ev["f1m"] - R.multiclass(cm[2])["f1_macro"]) <= 1e-12
