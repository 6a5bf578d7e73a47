"""Stage-two epochs (-m gpu): a fed epoch with a muting schedule on the device, and the bound task module through its freeze
epoch.

Fed epoch: M2-Mixer-B, bf16, dropout 0.5, batch 8 over a shuffled split of 43 samples -- the shape that repeats its own bits
(tests/test_gpu_feed_epoch.py).  Two engines of the same seed take one stage-one step and freeze.  One runs
capture_feed + run_epoch_fed(muting=codes) on a feed built with muting=True; the other capture() / replay(index_select ..., with
torch.zeros_like in place of the muted input) over the same order and codes, the tail through its sibling.  The muted gather
writes the bytes torch.zeros_like gives, so parameters and both Adam moments are BIT-identical, at steps = 1 and steps = 2; the
frozen ranges equal their snapshot at the freeze.

Bound module: AV-MNIST S, fp32, dropout 0, B = 24, bind_engine(two_stage=True), freeze_modalities_on_epoch = 1, random muting
drawn from a seeded np.random: two training_steps at epoch 0, three at epoch 1, against the float64 reference (engine_ref.Step,
then stage_ref.FrozenStep on the batches with the drawn input zeroed) at the bars of
test_gpu_engine_backed.test_bound_training_steps_match_the_oracle (losses and parameters 1e-3 absolute, LR 1e-3)."""
import numpy as np
import pytest
import torch

import engine_ref as R
import gen_util as G
import stage_ref as S
from engine_cases import Case

pytestmark = pytest.mark.gpu

B, N = 8, 43
AV_B = Case("avmnist_B", "avmnist", dict(G.AVMNIST["B"]), B, 0.5, {})
CODES = [1, 0, 2, 2, 0, 1]                               # one per step of the epoch, the ragged tail's included
FP32_ATOL, LR = 1e-3, 1e-3                               # tests/test_gpu_engine_backed.py


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture
def fp32_modules():
    import m2_mixer_amd as M
    prev = M.config.get_precision()
    M.set_precision("fp32")
    yield
    M.set_precision(prev)


def av_engine(dev):
    from m2_mixer_amd.engine import AVMnistEngine
    eng = AVMnistEngine(AV_B.cfg, B, device=dev, precision="bf16", lr=1e-3, seed=9)
    eng._tail_engines[N % B] = eng.sibling(N % B)        # the training sibling exists before any capture
    return eng


def pick(srcs, order, lo, bs, code):
    batch = [t.index_select(0, order[lo:lo + bs]) for t in srcs]
    if code:
        batch[code - 1] = torch.zeros_like(batch[code - 1])
    return tuple(batch)


def manual_epoch(eng, srcs, order, steps):
    from m2_mixer_amd.data import feed_plan
    replays, singles, tail = feed_plan(N, B, steps)
    replay = eng.capture(*pick(srcs, order, 0, B, 0), steps=steps)
    k = 0
    for _ in range(replays):
        flat = [t for i in range(steps) for t in pick(srcs, order, (k + i) * B, B, CODES[k + i])]
        replay(*flat)
        k += steps
    for _ in range(singles):
        eng.train_step(*pick(srcs, order, k * B, B, CODES[k]))
        k += 1
    if tail:
        sib = eng._tail_engines[tail]
        sib.pack()
        sib.train_step(*pick(srcs, order, k * B, tail, CODES[k]))
        eng.pack()
    torch.cuda.synchronize()


@pytest.mark.parametrize("steps", [1, 2])
def test_fed_stage_two_epoch_is_the_host_muted_epoch_bit_for_bit(steps, dev):
    from m2_mixer_amd.data import run_epoch_fed
    from m2_mixer_amd.engine import EpochFeed
    srcs = tuple(t.to(dev) for t in R.case_batch(AV_B._replace(B=N), 301))
    order = torch.from_numpy(np.random.default_rng(17).permutation(N)).to(dev)
    first = tuple(t[:B].contiguous() for t in srcs)
    manual, fed = av_engine(dev), av_engine(dev)
    assert torch.equal(manual.flat_p, fed.flat_p)
    for eng in (manual, fed):
        eng.fused_step(*first)                           # stage one: the frozen keys' moments are not zero
        eng.freeze_modalities()
    torch.cuda.synchronize()
    ranges = S.flat_ranges(fed.shapes, {k for k in fed.shapes if S.is_frozen(AV_B, k)})
    snap = [[t[lo:hi].clone() for lo, hi in ranges] for t in (fed.flat_p, fed.flat_m, fed.flat_v)]
    assert all(bool(row[0].any()) for row in snap[1:]), "the stage-one step left moments in the frozen ranges"

    manual_epoch(manual, srcs, order, steps)
    feed = EpochFeed(srcs, B, dev, muting=True)
    replay = fed.capture_feed(feed, steps=steps)
    assert feed.rows() == 0 and feed.mute_state.tolist() == [0, 0], "capture_feed puts the feed's cursor and step index back"
    got = run_epoch_fed(fed, feed, replay, N, order=order, muting=CODES)
    torch.cuda.synchronize()
    assert feed.rows() == N and feed.mute_state.tolist() == [6, 0]
    assert got["steps"] == 6 and got["samples"] == N
    assert abs(got["loss_step_mean"] - got["loss_fusion"]) < 1e-12, "stage two: the step's loss is loss_fusion"
    for name in ("flat_p", "flat_m", "flat_v"):
        assert torch.equal(getattr(manual, name), getattr(fed, name)), f"{name} differs from the host-muted loop's"
    assert float(fed.adam_state[0]) == float(manual.adam_state[0]) == 7.0 and int(fed.drop_step[0]) == int(manual.drop_step[0]) == 7
    for t, row in zip((fed.flat_p, fed.flat_m, fed.flat_v), snap):
        for (lo, hi), s in zip(ranges, row):
            assert torch.equal(t[lo:hi], s), "a frozen range changed during the epoch"
    with pytest.raises(ValueError, match="never mutes"):
        run_epoch_fed(fed, feed, None, train=False, muting=CODES)


# ---- the bound module ------------------------------------------------------------------------------------------------------
def model_cfg(c, **extra):
    mods = {"image": dict(c["image"], block_type="MLPMixer"), "audio": dict(c["audio"], block_type="MLPMixer"),
            "multimodal": dict(c["multimodal"], block_type="FusionMixer", fusion_function="ConcatFusion"),
            "classification": dict(classifier="StandardClassifier", num_classes=c["num_classes"],
                                   input_shape=[16, 49, c["multimodal"]["hidden_dim"]])}
    return {"dropout": c["dropout"], "modalities": mods, **extra}


def make_net(c, seed, dev, **extra):
    from m2_mixer_amd import models as MD
    params = dict(G.make_params(G.avmnist_shapes(c), seed))
    net = MD.AVMnistMixerMultiLoss(model_cfg(c, **extra), {"lr": LR, "betas": (0.9, 0.999), "scheduler_patience": 1}).to(dev)
    net.load_state_dict(params, strict=False)
    return net, params


def test_bound_module_trains_through_its_freeze_epoch(dev, fp32_modules):
    from m2_mixer_amd.models import muting_codes
    cfg, BB = dict(G.AVMNIST["S"], dropout=0.0), 24
    case = Case("avmnist_S_bound", "avmnist", cfg, BB, 0.0, {})
    probs = {"image": 0.3, "audio": 0.3, "multimodal": 0.4}
    extra = dict(freeze_modalities_on_epoch=1, random_modality_muting_on_freeze=True, muting_probs=probs)
    net, params = make_net(cfg, 11, dev, **extra)
    with pytest.raises(NotImplementedError, match="freeze_modalities_on_epoch"):
        net.bind_engine(BB)                              # without the keyword the refusal stays
    assert net.engine is None
    eng = net.bind_engine(BB, precision="fp32", two_stage=True)
    np.random.seed(77)
    codes = muting_codes(3, probs, ("image", "audio")).tolist()
    np.random.seed(77)                                   # training_step draws the same three

    def batch_of(seed):
        image, audio, labels = G.avmnist_batch(BB, seed, cfg)
        return (image, audio, labels), {"image": image.to(dev), "audio": audio.to(dev), "label": labels.to(dev)}

    ref = R.Step(case, params, LR)
    net.current_epoch = 0
    for step in range(2):
        host, batch = batch_of(20 + step)
        out = net.training_step(batch, step)
        want = ref.step(host)["losses"]
        for i, k in enumerate(("loss_image", "loss_audio", "loss_fusion", "loss")):
            assert abs(float(out[k]) - float(want[i])) < FP32_ATOL, (step, k)
    assert not net.modalities_freezed and not eng._frozen
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    two = S.FrozenStep(ref)
    net.current_epoch = 1
    for step in range(3):
        host, batch = batch_of(30 + step)
        out = net.training_step(batch, step)
        assert net.modalities_freezed and eng._frozen
        assert net.mute == ["multimodal", "image", "audio"][codes[step]], "the module drew what muting_codes draws"
        muted = list(host)
        if codes[step]:
            muted[codes[step] - 1] = torch.zeros_like(muted[codes[step] - 1])
        want = two.step(tuple(muted))["losses"]
        for i, k in enumerate(("loss_image", "loss_audio", "loss_fusion", "loss")):
            assert abs(float(out[k]) - float(want[i])) < FP32_ATOL, (step, k, codes[step])
        assert float(out["loss"]) == float(out["loss_fusion"])
    torch.cuda.synchronize()
    after = net.state_dict()
    for k in before:
        if S.is_frozen(case, k):
            assert torch.equal(after[k], before[k]), f"frozen {k} changed in stage two"
        elif not k.endswith(R.NOISE_KEYS):
            assert not torch.equal(after[k], before[k]), f"trainable {k} did not move"
    worst = max(float((after[k].double().cpu() - v).abs().max()) for k, v in two.p.items() if not k.endswith(R.NOISE_KEYS))
    print(f"bound two-stage parameters after 2 + 3 steps: abs {worst:.2e}")
    assert worst < FP32_ATOL
    out = net.validation_step(batch_of(40)[1])           # evaluation keeps the weighted total
    assert float(out["loss"]) != float(out["loss_fusion"])
