"""CPU-side checks of the engine-backed task modules (models._MultiLossModule.bind_engine): the loss-weight schedule of
validation_epoch_end, what bind_engine refuses, EngineOptimizer's mapping onto the engine (a stand-in engine object records the
calls) and the ABI 18 entry points of the binding."""
import pytest
import torch

import gen_util as G


def _model_cfg(task, **extra):
    if task == "avmnist":
        c = G.AVMNIST["S"]
        mods = {"image": dict(c["image"], block_type="MLPMixer"), "audio": dict(c["audio"], block_type="MLPMixer")}
    elif task == "mimic":
        c = G.MIMIC_H
        mods = {"static": dict(c["static"], block_type="MLP"), "time": dict(c["time"], block_type="MLPMixerNoPatching")}
    else:
        c = G.MMIMDB
        mods = {"image": dict(c["image"], block_type="MLPMixer"), "text": dict(c["text"], block_type="MLPMixer")}
    mods["multimodal"] = dict(c["multimodal"], block_type="FusionMixer", fusion_function="ConcatFusion")
    mods["classification"] = dict(classifier="StandardClassifier", num_classes=c["num_classes"],
                                  input_shape=[16, 49, c["multimodal"]["hidden_dim"]])
    cfg = {"dropout": 0.0, "modalities": mods, **extra}
    if task == "mmimdb":
        cfg["pos_weight"] = c["pos_weight"]
    return cfg


def _net(task, **extra):
    from m2_mixer_amd import models as MD
    cls = {"avmnist": MD.AVMnistMixerMultiLoss, "mimic": MD.MimicMixerMultiLoss, "mmimdb": MD.MMIMDBMixerMultiLoss}[task]
    return cls(_model_cfg(task, **extra), {"lr": 1e-2, "scheduler_patience": 1})


class _RecordingEngine:
    """Stands in for a fused engine: records set_fusion_loss_weight / set_lr and serves an Adam state dict."""

    def __init__(self, n_params, lr=1e-2):
        self.adam_state = torch.tensor([3.0, lr, 0.0, 0.0])
        self.betas, self.eps, self.weight_decay = (0.9, 0.999), 1e-8, 0.0
        self.calls = []
        self.n = n_params
        self.moments = [(torch.full((2,), float(i)), torch.full((2,), float(i) + 0.5)) for i in range(n_params)]

    def set_fusion_loss_weight(self, w):
        self.calls.append(("fusion_loss_weight", w))

    def set_lr(self, lr):
        self.calls.append(("lr", lr))
        self.adam_state[1] = lr

    def optimizer_state_dict(self):
        state = {i: {"step": torch.tensor(float(self.adam_state[0])), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
                 for i, (m, v) in enumerate(self.moments)}
        group = {"lr": float(self.adam_state[1]), "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay,
                 "amsgrad": False, "maximize": False, "params": list(range(self.n))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, osd):
        self.calls.append(("load", osd))
        self.set_lr(float(osd["param_groups"][0]["lr"]))


def test_fusion_loss_weight_schedule_host_arithmetic():
    """models/avmnist.py:338-339, models/mimic.py:149-150: from epoch loss_change_epoch on, += fusion_loss_change per validation
    epoch, clamped at 1; the reference's defaults (0, 0) leave the weight where it is; MM-IMDb (a plain sum) has no schedule."""
    for task in ("avmnist", "mimic"):
        net = _net(task, fusion_loss_change=0.3, loss_change_epoch=2)
        assert net.fusion_loss_change == 0.3 and net.loss_change_epoch == 2
        w0 = net.fusion_loss_weight
        assert w0 == pytest.approx(1.0 / 3)
        for epoch in (0, 1):
            net.current_epoch = epoch
            net.validation_epoch_end([])
            assert net.fusion_loss_weight == w0, (task, epoch)          # gated by loss_change_epoch
        net.current_epoch = 2
        net.validation_epoch_end([])
        assert net.fusion_loss_weight == pytest.approx(w0 + 0.3)
        net.current_epoch = 3
        net.validation_epoch_end([])
        assert net.fusion_loss_weight == pytest.approx(w0 + 0.6)
        for epoch in (4, 5):
            net.current_epoch = epoch
            net.validation_epoch_end([])
            assert net.fusion_loss_weight == 1                           # min(1, .)
    plain = _net("avmnist")
    assert plain.fusion_loss_change == 0 and plain.loss_change_epoch == 0
    plain.current_epoch = 7
    plain.validation_epoch_end([])
    assert plain.fusion_loss_weight == pytest.approx(1.0 / 3)
    mm = _net("mmimdb", fusion_loss_change=0.05)
    mm.validation_epoch_end([])
    assert mm.fusion_loss_weight == pytest.approx(1.0 / 3)


def test_validation_epoch_end_forwards_the_new_weight_to_a_bound_engine():
    net = _net("mimic", fusion_loss_change=0.05)
    eng = _RecordingEngine(4)
    net._engine = eng                                   # (what bind_engine leaves behind, without a GPU)
    net.validation_epoch_end([])
    assert eng.calls == [("fusion_loss_weight", pytest.approx(1.0 / 3 + 0.05))]
    assert net.fusion_loss_weight == pytest.approx(1.0 / 3 + 0.05)
    still = _net("avmnist")                             # no change configured: the engine is not touched
    still._engine = eng
    eng.calls.clear()
    still.validation_epoch_end([])
    assert eng.calls == []


def test_unbound_step_hooks_are_shared_step():
    """Unbound, the hooks are the reference's: shared_step(batch, mode=...) -- on the CPU that is the loud no-CPU-path error."""
    net = _net("mimic")
    assert net.engine is None
    seen = []
    net.shared_step = lambda batch, mode=None: seen.append(mode) or {"mode": mode}
    assert net.training_step(None, 0) == {"mode": "train"}
    assert net.validation_step(None, 0) == {"mode": "val"}
    assert net.test_step(None, 0) == {"mode": "test"}
    assert seen == ["train", "val", "test"]


def test_bind_engine_refusals():
    with pytest.raises(NotImplementedError, match="freeze_modalities_on_epoch"):
        _net("avmnist", freeze_modalities_on_epoch=3).bind_engine(8)
    with pytest.raises(NotImplementedError, match="random_modality_muting_on_freeze"):
        _net("mmimdb", random_modality_muting_on_freeze=True, muting_probs={"image": 0.3, "text": 0.3, "multimodal": 0.4}).bind_engine(8)
    with pytest.raises(RuntimeError, match="GPU"):
        _net("avmnist").bind_engine(8)                  # a CPU module
    net = _net("avmnist")
    net._engine = _RecordingEngine(1)
    with pytest.raises(RuntimeError, match="already bound"):
        net.bind_engine(8)


def test_engine_optimizer_maps_onto_the_engine_and_reduce_lr_on_plateau():
    from torch.optim.lr_scheduler import ReduceLROnPlateau
    from m2_mixer_amd.models import EngineOptimizer
    net = _net("avmnist")
    params = list(net.parameters())
    eng = _RecordingEngine(len(params))
    net._engine = eng
    conf = net.configure_optimizers()
    opt = conf["optimizer"]
    assert isinstance(opt, EngineOptimizer) and isinstance(opt, torch.optim.Optimizer)
    assert conf["monitor"] == "val_loss" and isinstance(conf["lr_scheduler"], ReduceLROnPlateau)
    assert net._engine_optimizer is opt and opt.param_groups[0]["lr"] == pytest.approx(1e-2)
    before = [p.detach().clone() for p in params]
    opt.zero_grad()
    opt.step()                                          # no-ops: the replayed step already updated the weights
    assert all(torch.equal(a, p) for a, p in zip(before, params))
    sched = conf["lr_scheduler"]
    sched.step(1.0)
    for v in (1.1, 1.2, 1.3):                           # patience 1: rising val_loss cuts the rate
        sched.step(v)
    assert opt.param_groups[0]["lr"] == pytest.approx(1e-3)
    assert eng.calls == []                              # pushed lazily, by the next training_step
    opt.sync_lr()
    assert eng.calls == [("lr", pytest.approx(1e-3))]
    opt.sync_lr()
    assert len(eng.calls) == 1                          # unchanged: nothing pushed
    sd = opt.state_dict()
    assert sd["param_groups"][0]["lr"] == pytest.approx(1e-3) and len(sd["state"]) == len(params)
    plain = torch.optim.Adam(_net("avmnist").parameters(), lr=5e-2)
    plain.load_state_dict(sd)                           # torch.optim.Adam's layout
    assert plain.param_groups[0]["lr"] == pytest.approx(1e-3)
    eng.calls.clear()
    opt.load_state_dict(plain.state_dict())
    assert eng.calls[0][0] == "load" and opt.param_groups[0]["lr"] == pytest.approx(1e-3)


def test_abi18_entry_points_are_declared():
    import ctypes as C
    from m2_mixer_amd import _lib
    assert _lib.ABI_VERSION == 18
    for name, nargs in (("m2m_heads_ce_w", 12), ("m2m_heads_bce_w", 13)):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, name
        base = _lib.SIGNATURES[name[:-2]][1]
        assert args[:-1] == base[:-1] + [_lib._fp] and args[-1] is _lib._fp, name     # + const float* weights, before the stream
