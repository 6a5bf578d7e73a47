"""GPU tests (-m gpu) of the ranking buffers (csrc/rank.hip, engine.RankBuffer).

  * m2m_rank_counts: exact integer equality with the plain loops of tests/rank_ref.py (the per-row numpy form of the same loops
    above 300 rows; tests/test_host_rank.py holds the two forms equal) at every tile boundary of both loops, on softmax rows,
    heavy ties, an all-equal column, an absent and a universal class and rows without a label; nothing is read behind n, nothing
    written behind the counts;
  * m2m_rank_append: the stored softmax against the float64 softmax within the bound derived below, labels, the state words,
    overflow, refusals;
  * the engines with rank_scores=True (eager, captured, multi-step graph, sibling, evaluate), on / off bit-identity, the bound
    MIMIC module's epoch-end hooks and data.run_epoch.

The bound on a stored probability p = expf(x - m) / sum_k expf(x_k - m), relative to the float64 softmax of the same fp32
logits: one rounding of x - m, amplified by the exponent's size (|x - m| units of 2^-24), 1 ulp for expf, K - 1 additions, the
division: (|x - m| + K + 4) 2^-24.  The largest observed ratio to the bound is printed.
"""
import numpy as np
import pytest
import torch

import gen_util as G
import rank_ref as R

pytestmark = pytest.mark.gpu

TI, TJ = 256, 128                      # csrc/rank.hip: RK_TI rows i per workgroup, RK_TJ rows j per LDS tile
HEADS = ("a", "b", "fusion")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _append(logits, labels, K, probs, row_labels, capacity, state):
    from m2_mixer_amd import _lib as L
    nh, B = logits.shape[:2]
    L.check(L.lib().m2m_rank_append(logits.data_ptr(), labels.data_ptr(), nh, B, K, probs.data_ptr(), row_labels.data_ptr(), capacity,
                                    state.data_ptr(), L.stream_ptr()), "rank_append")


def _counts(probs, row_labels, nh, n, K, capacity, out):
    from m2_mixer_amd import _lib as L
    L.check(L.lib().m2m_rank_counts(probs.data_ptr(), row_labels.data_ptr(), nh, n, K, capacity, out.data_ptr(), L.stream_ptr()), "rank_counts")


def _host_counts(probs, labels, K):
    """(nheads, n, 4) from the plain loops; probs (nheads, K, n) float32 values compared as they are."""
    fn = R.rank_counts if labels.shape[0] <= 300 else R.rank_counts_fast
    return np.stack([fn(probs[h], labels, K) for h in range(probs.shape[0])])


def _softmax32(rng, nh, n, K):
    return R.softmax64(rng.normal(size=(nh, n, K)) * 2).astype(np.float32).transpose(0, 2, 1).copy()        # (nh, K, n)


def _count_inputs(nh, n, K, seed):
    """name -> (probs (nh, K, n) float32, labels (n) int32)."""
    rng = np.random.default_rng(seed)
    out = {"softmax": (_softmax32(rng, nh, n, K), rng.integers(0, K, size=n))}
    levels = np.array([0.0, 0.125, 0.25, 0.5, 1.0], dtype=np.float32)
    lab = rng.integers(0, K, size=n)
    lab[::5] = -1                                                        # rows without a label: zeros out, invisible to the others
    out["five_levels_and_skipped_rows"] = (levels[rng.integers(0, 5, size=(nh, K, n))], lab)
    p = _softmax32(rng, nh, n, K)
    p[:, 0, :] = 0.375                                                   # an all-equal column
    out["equal_column_and_absent_class"] = (p, rng.integers(0, max(K - 1, 1), size=n))        # class K - 1 never occurs
    out["universal_class"] = (_softmax32(rng, nh, n, K), np.full(n, K - 1))
    return {k: (p, l.astype(np.int32)) for k, (p, l) in out.items()}


@pytest.mark.parametrize("nh", [1, 3])
@pytest.mark.parametrize("n,K", [(1, 2), (2, 2), (63, 2), (64, 6), (65, 6), (257, 10), (700, 64), (2 * TI + 3, 10)])
def test_counts_equal_the_plain_loop(n, K, nh, dev):
    cap = n + 37
    for name, (p, lab) in _count_inputs(nh, n, K, 100 * n + K).items():
        probs = torch.full((nh, K, cap), 2.0, device=dev)                # rows at and behind n: any read there changes a count
        labels = torch.zeros(cap, dtype=torch.int32, device=dev)
        probs[:, :, :n] = torch.from_numpy(p).to(dev)
        labels[:n] = torch.from_numpy(lab).to(dev)
        buf = torch.full((nh * n * 4 + 64,), -7, dtype=torch.int32, device=dev)
        _counts(probs, labels, nh, n, K, cap, buf)
        got = buf.cpu().numpy()
        assert (got[nh * n * 4:] == -7).all(), (name, "the 64 guard words behind the counts")
        want = _host_counts(p, lab, K)
        assert np.array_equal(got[:nh * n * 4].reshape(nh, n, 4), want), name
        if name == "five_levels_and_skipped_rows":
            assert (want[:, ::5] == 0).all() and want[:, :, 0].max() <= n - len(range(0, n, 5))
        if name == "universal_class":
            assert np.array_equal(want[:, :, 0], want[:, :, 1]) and (want[:, :, 0] >= 1).all()


def _bound_ratio(stored, logits):
    """max over the elements of |stored - p64| / (p64 (|x - m| + K + 4) 2^-24); stored, logits (..., K)."""
    x = logits.astype(np.float64)
    p64 = R.softmax64(logits)
    bound = (np.abs(x - x.max(axis=-1, keepdims=True)) + x.shape[-1] + 4) * 2.0 ** -24 * p64
    return float((np.abs(stored.astype(np.float64) - p64) / bound).max())


@pytest.mark.parametrize("B", [1, 7, 64, 130])
@pytest.mark.parametrize("K", [2, 6, 10, 64])
def test_append_stores_the_softmax_the_labels_and_the_state(K, B, dev):
    nh, cap = 3, 4 * B + 5
    gen = torch.Generator().manual_seed(1000 * K + B)
    buf = torch.full((nh * K * cap + 64,), -3.0, device=dev)
    probs = buf[:nh * K * cap].view(nh, K, cap)
    lbuf = torch.full((cap + 16,), -9, dtype=torch.int32, device=dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    bad, worst = 0, 0.0
    all_logits, all_labels = [], []
    for call in range(4):
        logits = (torch.randn(nh, B, K, generator=gen) * 4).to(dev)
        labels = torch.randint(0, K, (B,), generator=gen, dtype=torch.int64)
        if B >= 7:
            labels[1], labels[3], labels[B - 1] = -1, K, 2 ** 40       # stored as -1 and counted
            bad += 3
        labels = labels.to(dev)
        _append(logits, labels, K, probs, lbuf, cap, state)
        assert state.cpu().tolist() == [(call + 1) * B, 0, bad, 0], call
        all_logits.append(logits.cpu().numpy())
        all_labels.append(labels.cpu().numpy())
    n = 4 * B
    x = np.concatenate(all_logits, axis=1)                             # (nh, n, K): batch order = row order
    got = probs.cpu().numpy()
    worst = _bound_ratio(got[:, :, :n].transpose(0, 2, 1), x)
    print(f"append K={K} B={B}: largest |p - p64| / bound = {worst:.3f}")
    assert worst <= 1.0
    assert (got[:, :, n:] == -3.0).all() and (buf[nh * K * cap:] == -3.0).all(), "nothing is written behind the appended rows"
    lab = np.concatenate(all_labels)
    want = np.where((lab >= 0) & (lab < K), lab, -1).astype(np.int32)
    got_l = lbuf.cpu().numpy()
    assert np.array_equal(got_l[:n], want) and (got_l[n:] == -9).all()


def test_append_past_the_capacity_keeps_counting_and_writes_nothing(dev):
    from m2_mixer_amd.engine import RankBuffer
    nh, K, B, cap = 3, 6, 64, 100
    rb = RankBuffer("mimic", ("static", "time", "fusion"), K, cap, dev)
    buf = torch.full((nh * K * cap + 64,), -3.0, device=dev)
    lbuf = torch.full((cap + 64,), -9, dtype=torch.int32, device=dev)
    rb.probs, rb.labels = buf[:nh * K * cap].view(nh, K, cap), lbuf[:cap]
    gen = torch.Generator().manual_seed(9)
    xs = [(torch.randn(nh, B, K, generator=gen) * 3).to(dev) for _ in range(2)]
    ls = [torch.randint(0, K, (B,), generator=gen).to(dev) for _ in range(2)]
    for x, l in zip(xs, ls):
        rb.add(x, l)
    assert rb.state.cpu().tolist() == [128, 0, 0, 0] and rb.rows() == 128
    x = torch.cat(xs, dim=1).cpu().numpy()[:, :cap]
    assert _bound_ratio(rb.probs.cpu().numpy().transpose(0, 2, 1), x) <= 1.0      # rows 0 .. 99 of every column: the first 100 rows
    assert np.array_equal(rb.labels.cpu().numpy(), torch.cat(ls).cpu().numpy()[:cap].astype(np.int32))
    assert (buf[nh * K * cap:] == -3.0).all() and (lbuf[cap:] == -9).all(), "the guards behind both buffers"
    with pytest.raises(RuntimeError, match="capacity 100 rows, 128 rows seen"):
        rb.counts()
    rb.reset()
    assert rb.rows() == 0
    rb.add(xs[0], ls[0])
    counts, labels = rb.counts()
    assert counts.shape == (nh, B, 4) and labels.tolist() == ls[0].cpu().tolist()


def test_refusals_name_the_limit(dev):
    from m2_mixer_amd import _lib as L
    from m2_mixer_amd.engine import RankBuffer
    nh, B = 3, 8
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    lab = torch.zeros(B, dtype=torch.int64, device=dev)
    rows = torch.zeros(64, dtype=torch.int32, device=dev)
    out = torch.zeros(nh * 64 * 4, dtype=torch.int32, device=dev)
    K = L.SCORES_MAX_CLASSES + 1
    probs = torch.zeros(nh, K, 64, device=dev)
    with pytest.raises(RuntimeError, match="M2M_SCORES_MAX_CLASSES"):
        _append(torch.zeros(nh, B, K, device=dev), lab, K, probs, rows, 64, state)
    with pytest.raises(RuntimeError, match="M2M_SCORES_MAX_CLASSES"):
        _counts(probs, rows, nh, 8, K, 64, out)
    with pytest.raises(RuntimeError, match="capacity must be >= 1"):
        _append(torch.zeros(nh, B, 6, device=dev), lab, 6, probs, rows, 0, state)
    with pytest.raises(RuntimeError, match="capacity must be >= 1"):
        _counts(probs, rows, nh, 0, 6, 0, out)
    with pytest.raises(RuntimeError, match="n <= capacity"):
        _counts(probs, rows, nh, 65, 6, 64, out)
    with pytest.raises(RuntimeError, match="NULL"):
        L.check(L.lib().m2m_rank_counts(probs.data_ptr(), 0, nh, 8, 6, 64, out.data_ptr(), L.stream_ptr()), "rank_counts")
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [0, 0, 0, 0] and int(out.abs().sum()) == 0
    with pytest.raises(RuntimeError, match="ranking kernels take"):
        RankBuffer("mimic", HEADS, K, 64, dev)
    with pytest.raises(RuntimeError, match="at least one row"):
        RankBuffer("mimic", HEADS, 6, 0, dev)
    with pytest.raises(RuntimeError, match="multilabel"):
        RankBuffer("mmimdb", HEADS, 6, 64, dev)
    rb = RankBuffer("mimic", HEADS, 6, 64, dev)
    with pytest.raises(RuntimeError, match="RankBuffer.add"):
        rb.add(torch.zeros(nh, B, 6, device=dev), lab.int())
    with pytest.raises(RuntimeError, match="RankBuffer.add"):
        rb.add(torch.zeros(nh, 6, B, device=dev).transpose(1, 2), lab)
    assert rb.rows() == 0 and rb.counts()[0].shape == (nh, 0, 4)


# ---------------------------------------------------------------------------------------------------------------
# the engines
# ---------------------------------------------------------------------------------------------------------------
def _make(task, B, dev, rank, precision="bf16", cfg=None, **kw):
    from m2_mixer_amd.engine import AVMnistEngine, MimicEngine
    cls, c = {"avmnist": (AVMnistEngine, G.AVMNIST["B"]), "mimic": (MimicEngine, G.MIMIC_H)}[task]
    return cls(cfg or c, B, device=dev, precision=precision, lr=1e-3, seed=42, rank_scores=rank, **kw), (cfg or c)


def _batch(task, B, seed, c, dev):
    fn = {"avmnist": G.avmnist_batch, "mimic": G.mimic_batch}[task]
    return tuple(t.to(dev) for t in fn(B, seed, c))


def _check_buffer(rb, steps, K):
    """steps: [(logits (3, B, K) cloned after the step, labels (B))] in step order.  The buffer's rows are the steps' rows in that
    order (labels exactly, probabilities within the bound), and compute() equals the restatement on the buffer's OWN contents."""
    n = sum(int(l.shape[0]) for _, l in steps)
    assert rb.rows() == n
    counts, labels = rb.counts()
    assert labels.tolist() == torch.cat([l for _, l in steps]).cpu().tolist()
    x = torch.cat([lg for lg, _ in steps], dim=1).cpu().numpy()
    stored = rb.probs[:, :, :n].cpu().numpy()
    ratio = _bound_ratio(stored.transpose(0, 2, 1), x)
    print(f"{rb.task}: {n} rows, largest |p - p64| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert np.array_equal(counts.numpy(), _host_counts(stored, labels.numpy(), K))
    got, want = rb.compute(), R.task(rb.task, stored, labels.numpy(), K, rb.head_names)
    assert set(got) == set(want)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12, k
    return got


@pytest.mark.parametrize("task,B,tail", [("mimic", 128, 17), ("avmnist", 64, 5)])
def test_eager_steps_append_in_step_order(task, B, tail, dev):
    eng, c = _make(task, B, dev, rank=True)
    K = c["num_classes"]
    assert eng.rank is not None and eng.scores is None and eng.rank.capacity == 65536 and eng.rank_buffer("train") is eng.rank
    sib = eng.sibling(tail)
    assert sib.rank is eng.rank
    steps = []
    for i in range(3):
        b = _batch(task, B, 10 + i, c, dev)
        eng.train_step(*b)
        steps.append((eng.logits.clone(), b[-1]))
    b = _batch(task, tail, 20, c, dev)
    sib.pack()
    sib.train_step(*b)
    eng.pack()
    steps.append((sib.logits.clone(), b[-1]))
    got = _check_buffer(eng.rank, steps, K)
    if task == "mimic":
        assert set(got) == {"auroc", "auroc_static", "auroc_time"}
        assert set(eng.rank.compute(names=("auroc", "roc_auc_macro"))) == {n + s for n in ("auroc", "roc_auc_macro") for s in ("", "_static", "_time")}
    else:
        assert set(got) == {n + s for n in ("ap_macro", "roc_auc_macro") for s in ("", "_image", "_audio")}
    assert all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in got.values())
    eng.rank.reset()
    assert eng.rank.rows() == 0


@pytest.mark.parametrize("task,B", [("mimic", 128), ("avmnist", 64)])
def test_captured_replays_append_and_capture_leaves_the_cursor(task, B, dev):
    eng, c = _make(task, B, dev, rank=True)
    K = c["num_classes"]
    b = _batch(task, B, 30, c, dev)
    eng.train_step(*b)
    steps = [(eng.logits.clone(), b[-1])]
    replay = eng.capture(*_batch(task, B, 31, c, dev))
    assert eng.rank.rows() == B, "capture() puts the cursor back where it found it"
    for i in range(3):
        b = _batch(task, B, 32 + i, c, dev)
        replay(*b)
        steps.append((eng.logits.clone(), b[-1]))
    _check_buffer(eng.rank, steps, K)


def test_three_step_graph_appends_every_step(dev):
    task, B = "mimic", 128
    eng, c = _make(task, B, dev, rank=True)
    bs = [_batch(task, B, 40 + i, c, dev) for i in range(6)]
    replay = eng.capture(*bs[0], steps=3)
    assert eng.rank.rows() == 0
    steps = []
    for r in range(2):
        replay(*[t for b in bs[3 * r:3 * r + 3] for t in b])
        steps += [(eng.logits_steps[i].clone(), bs[3 * r + i][-1]) for i in range(3)]
    _check_buffer(eng.rank, steps, c["num_classes"])


def test_evaluate_appends_only_into_the_buffer_it_is_given(dev):
    task, B = "mimic", 32
    eng, c = _make(task, B, dev, rank=True, precision="fp32")
    val, test = eng.rank_buffer("val"), eng.rank_buffer("test")
    assert val is not test and val is not eng.rank and eng.rank_buffer("val") is val
    sv = []
    for i in range(3):
        b = _batch(task, B, 50 + i, c, dev)
        eng.evaluate(*b, rank=val)
        sv.append((eng.logits.clone(), b[-1]))
    b = _batch(task, B, 60, c, dev)
    eng.evaluate(*b, rank=test)
    st = [(eng.logits.clone(), b[-1])]
    eng.evaluate(*_batch(task, B, 61, c, dev))                   # no buffer given: appended nowhere
    _check_buffer(val, sv, c["num_classes"])
    _check_buffer(test, st, c["num_classes"])
    assert eng.rank.rows() == 0


def test_rank_scores_off_is_the_default_and_allocates_nothing(dev):
    from m2_mixer_amd.engine import AVMnistEngine, MimicEngine
    for cls, cfg in ((AVMnistEngine, G.AVMNIST["S"]), (MimicEngine, G.MIMIC_H)):
        eng = cls(cfg, 8, device=dev, precision="bf16")
        assert eng.rank is None and "_split_ranks" not in eng.__dict__ and eng.sibling(3).rank is None
        with pytest.raises(RuntimeError, match="rank_scores=False"):
            eng.rank_buffer("train")


@pytest.mark.parametrize("B", [64, 128])
def test_rank_scores_on_and_off_are_bit_identical(B, dev):
    """Same seed, same batches, bf16, dropout 0.5, M2-Mixer-B (the configuration whose training is bit-reproducible:
    tests/test_gpu_parity.py test_bf16_training_is_bit_reproducible; the MIMIC step adds gradients with float atomics and does
    not repeat its own parameters from run to run, profiles/launch_trace_parity.txt row 21): the append launch only reads the
    step's logits and labels.  After each of three eager steps and three captured replays logits and predictions, and after
    each group every parameter and both Adam moments, are BIT-identical between rank_scores on and off.
    The reported losses are held to 1e-6 relative instead, as in tests/test_gpu_scores.py: the heads kernel sums them over its
    workgroups with float atomics in arrival order (csrc/heads.hip), so two runs of the SAME engine differ in their last bits
    with or without this feature; whether they came out bit-equal is printed (measured: never, 3e-8 .. 2e-7 relative)."""
    task = "avmnist"
    on, c = _make(task, B, dev, rank=True)
    off, _ = _make(task, B, dev, rank=False)
    assert off.rank is None and torch.equal(on.flat_p, off.flat_p)

    def same(where):
        torch.cuda.synchronize()
        assert torch.equal(on.logits, off.logits) and torch.equal(on.preds, off.preds), where
        rel = float((on.losses.double() - off.losses.double()).abs().max() / off.losses.double().abs().max())
        print(f"{task} B={B} {where}: losses bit-equal: {torch.equal(on.losses, off.losses)}, rel {rel:.2e}")
        assert rel < 1e-6, where

    for i in range(3):
        b = _batch(task, B, 70 + i, c, dev)
        for e in (on, off):
            e.train_step(*b)
        same(f"eager step {i}")
    assert torch.equal(on.flat_p, off.flat_p) and torch.equal(on.flat_m, off.flat_m) and torch.equal(on.flat_v, off.flat_v)
    r_on, r_off = on.capture(*b), off.capture(*b)
    for i in range(3):
        b = _batch(task, B, 80 + i, c, dev)
        r_on(*b)
        r_off(*b)
        same(f"replay {i}")
    assert torch.equal(on.flat_p, off.flat_p) and torch.equal(on.flat_m, off.flat_m) and torch.equal(on.flat_v, off.flat_v)
    assert on.rank.rows() == 6 * B


# ---------------------------------------------------------------------------------------------------------------
# the task modules and the epoch loop
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scores", [False, True])
def test_bound_mimic_module_epoch_end_hooks(scores, dev):
    """Two epochs of three training / two validation / two test steps: the hooks return `<split>_auroc*` (with scores=True
    merged with the count-table names), equal to the restatement on the buffer's contents, and leave the buffers empty."""
    from test_gpu_engine_backed import make_net
    from m2_mixer_amd import scores as S
    c, B, K = G.MIMIC_H, 128, G.MIMIC_H["num_classes"]
    net, _ = make_net("mimic", c, 301, dev)
    eng = net.bind_engine(B, precision="bf16", scores=scores, rank_scores=True)
    assert eng.rank is not None and (eng.scores is not None) == scores
    rank_names = {n + s for n in S.RANK_SCORES["mimic"] for s in ("", "_static", "_time")}
    table_names = {n + s for n in S.TASK_SCORES["mimic"] for s in ("", "_static", "_time")} if scores else set()
    for epoch in range(2):
        net.current_epoch = epoch
        for i in range(3):
            net.training_step(_batch("mimic", B, 400 + 10 * epoch + i, c, dev), i)
        for i, n in enumerate([B, 7]):
            net.validation_step(_batch("mimic", n, 500 + 10 * epoch + i, c, dev), i)
            net.test_step(_batch("mimic", n, 600 + 10 * epoch + i, c, dev), i)
        for split, hook, n in (("train", net.training_epoch_end, 3 * B), ("val", net.validation_epoch_end, B + 7), ("test", net.test_epoch_end, B + 7)):
            rb = eng.rank_buffer(split)
            assert rb.rows() == n, (epoch, split)
            stored, labels = rb.probs[:, :, :n].cpu().numpy(), rb.labels[:n].cpu().numpy()
            want = R.task("mimic", stored, labels, K, eng.HEAD_NAMES)
            got = hook([])
            assert set(got) == {f"{split}_{k}" for k in rank_names | table_names}
            for k, v in want.items():
                assert abs(got[f"{split}_{k}"] - v) <= 1e-12, (split, k)
            assert rb.rows() == 0, "an epoch-end hook resets its buffer"
            if scores:
                assert int(eng.score_table(split).table.sum()) == 0


def test_bind_engine_without_either_option_returns_none(dev):
    from test_gpu_engine_backed import make_net
    c = G.MIMIC_H
    net, _ = make_net("mimic", c, 302, dev)
    eng = net.bind_engine(16, precision="bf16")
    assert eng.rank is None and eng.scores is None
    net.training_step(_batch("mimic", 16, 1, c, dev), 0)
    net.validation_step(_batch("mimic", 5, 2, c, dev), 0)
    assert "_split_ranks" not in eng.__dict__ and all(s.rank is None for s in net._eval_siblings.values())
    assert net.training_epoch_end([]) is None and net.validation_epoch_end([]) is None and net.test_epoch_end([]) is None
    assert net.to_engine(16, precision="bf16").rank is None
    assert net.to_engine(16, precision="bf16", rank_scores=True, rank_capacity=99).rank.capacity == 99


def test_run_epoch_reports_the_rank_scores(dev, tmp_path):
    from test_host_cpu import _write_avmnist
    from m2_mixer_amd.data import ResidentAVMnist, prepare_tail_engine, run_epoch
    from m2_mixer_amd.engine import AVMnistEngine
    root = str(tmp_path / "avmnist")
    _write_avmnist(root, 300, 37, seed=5, learnable=True)           # train 275, val 25, test 37
    data = ResidentAVMnist(root, device=dev)
    cfg, B = dict(G.AVMNIST["S"], dropout=0.1), 16
    eng = AVMnistEngine(cfg, B, device=dev, precision="bf16", lr=1e-3, rank_scores=True, rank_capacity=512)
    assert prepare_tail_engine(eng, data, "train", B).rank is eng.rank
    replay = eng.capture(*next(iter(data.batches("train", B))))
    base = {"loss", "loss_step_mean", "loss_image", "loss_audio", "loss_fusion", "acc", "acc_image", "acc_audio", "hits", "hits_image",
            "hits_audio", "steps", "samples"}
    names = {n + s for n in ("ap_macro", "roc_auc_macro") for s in ("", "_image", "_audio")}
    for epoch in range(2):
        tr = run_epoch(eng, data, "train", B, train=True, replay=replay)
        assert set(tr) == base | names and tr["samples"] == 275
        rb = eng.rank_buffer("train")
        assert rb.rows() == 275, "the buffer holds this epoch only"
        want = R.task("avmnist", rb.probs[:, :, :275].cpu().numpy(), rb.labels[:275].cpu().numpy(), 10, eng.HEAD_NAMES)
        for k in names:
            assert abs(tr[k] - want[k]) <= 1e-12, k
        ev = run_epoch(eng, data, "test", B, train=False)
        assert set(ev) == base | names and eng.rank_buffer("test").rows() == 37 and rb.rows() == 275
