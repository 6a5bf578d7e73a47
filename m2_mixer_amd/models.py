"""The callers of the hot path: the reference's multi-loss task modules, Lightning-free.

    AVMnistMixerMultiLoss   models/avmnist.py:165-312, :413-422
    AVMnistMixerMultiLossUQ models/avmnist.py:447-572 (evidential losses, per-head uncertainty, late fusion of the predictions)
    MimicMixerMultiLoss     models/mimic.py:24-142
    MMIMDBMixerMultiLoss    models/mmimdb.py:22-147

Same constructor contract (`model_cfg`, `optimizer_cfg` with the keys of cfg/*/*.yml -- plain dicts or anything with
`.get` / attribute access), same sub-module names (hence the same state-dict keys as the published checkpoints), same
`shared_step(batch, mode=...)` result dict, same `configure_optimizers()` (Adam + ReduceLROnPlateau on `val_loss`).
What is NOT here is Lightning itself (trainer hooks, logging, metrics): a `pl.LightningModule` subclass can inherit from
these and add them.  The reference's step hooks (`training_step`, `validation_step`, `test_step`, `validation_epoch_end`,
modules/train_test_module.py:72-150) are here; after `bind_engine(batch_size)` they run the fused, hipGraph-captured step
(engine.py) over the module's OWN parameters -- `parameters()`, `state_dict()` and checkpoints see the live weights.
`to_engine()` is the lower-level alternative: an engine over a copy of the weights, driven by a loop of its own.
The towers are `m2_mixer_amd.modules` (HIP kernels under torch autograd); heads and losses are the same few torch ops the
reference uses.  Gradient-Blending (`gradblend: True`, models/avmnist.py:211-234) is accepted by the AV-MNIST and MIMIC modules:
`gb_weights` replaces the loss coefficients, and a bound module refreshes them on its engine (on_train_epoch_start, gradblend.py).
SoftAdapt weighting is outside the scope of this build and refused loudly.
"""
from __future__ import annotations

import os
import pickle
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import modules
from .accumulators import pass_accumulators
from .data import tail_engine_for, tail_step


class _LenientPickle:
    """`pickle_module` for torch.load that survives a Lightning `.ckpt` written by the reference's environment: its
    `hyper_parameters` / callback states pickle classes of packages this build does not need (omegaconf, pytorch_lightning).
    Unknown classes become inert placeholders; the tensors under `state_dict` load normally."""
    __name__ = "m2_mixer_amd.models._LenientPickle"

    class _Placeholder:
        def __init__(self, *a, **k):
            pass

        def __setstate__(self, state):
            pass

        def __call__(self, *a, **k):
            return self

    class Unpickler(pickle.Unpickler):
        def find_class(self, module, name):
            try:
                return super().find_class(module, name)
            except (ImportError, AttributeError):
                return type(name, (_LenientPickle._Placeholder,), {"__module__": module})

    load = staticmethod(pickle.load)
    dumps = staticmethod(pickle.dumps)
    dump = staticmethod(pickle.dump)
    Pickler = pickle.Pickler


#: the Lightning release the reference pins (requirements.txt:8); a PEP 440 string, because Lightning's checkpoint migration
#: parses this field with packaging.version.Version
LIGHTNING_VERSION = "1.8.6"


def _load_checkpoint_file(path, map_location, trusted: bool):
    """torch.load of a `.ckpt`.  First with `weights_only=True` (tensors and plain containers only: nothing in the file can
    run code) -- enough for checkpoints written by save_checkpoint.  A Lightning checkpoint written by the reference's
    environment pickles omegaconf / pytorch_lightning classes next to the `state_dict`; reading those needs the full
    unpickler, which executes whatever the file says -- only with `trusted=True`, i.e. for files the caller vouches for."""
    try:
        return torch.load(path, map_location=map_location, weights_only=True)
    except Exception as e:
        if not trusted:
            raise RuntimeError(
                f"{path}: not loadable with weights_only=True ({type(e).__name__}: {str(e)[:200]}).  A checkpoint that "
                "pickles foreign classes (Lightning hyper-parameters, omegaconf) needs load_from_checkpoint(..., trusted=True); "
                "unpickling runs code from the file, so pass it only for checkpoints from a source you trust") from e
    return torch.load(path, map_location=map_location, weights_only=False, pickle_module=_LenientPickle)


class _Cfg(dict):
    """dict with attribute access, recursively (stands in for omegaconf.DictConfig)."""

    def __init__(self, d=None):
        super().__init__()
        for k, v in dict(d or {}).items():
            self[k] = _Cfg(v) if isinstance(v, dict) else v

    __getattr__ = dict.__getitem__


def _plain(c) -> dict:
    return {k: (_plain(v) if isinstance(v, dict) else v) for k, v in dict(c).items()}


def muting_codes(steps: int, muting_probs, mods: Sequence[str], rng=np.random) -> np.ndarray:
    """The muting schedule of `steps` stage-two training steps as the codes engine.EpochFeed takes: `steps` calls of
    rng.choice([a, b, "multimodal"], p=...) in order -- shared_step's draw (models/avmnist.py:243-251), one per training step, so
    the generator is consumed exactly as a loop of training steps consumes it -- mapped to 0 ("multimodal": mute nothing), 1 (mute
    modality a, the feed's source 0) and 2 (modality b, source 1)."""
    names = list(mods) + ["multimodal"]
    code = {names[0]: 1, names[1]: 2, "multimodal": 0}
    p = [muting_probs[n] for n in names]
    return np.asarray([code[str(rng.choice(names, p=p))] for _ in range(int(steps))], dtype=np.int32)


class EngineOptimizer(torch.optim.Optimizer):
    """The optimizer of a module bound to a fused engine (_MultiLossModule.bind_engine): the engine's Adam, which every replayed
    training step has already applied.  step() / zero_grad() are no-ops (a LightningModule subclass sets
    `automatic_optimization = False` when bound); `param_groups[0]["lr"]` is what schedulers such as ReduceLROnPlateau write --
    the next training_step pushes a changed value to the engine (engine.set_lr); state_dict() / load_state_dict() are the
    engine's Adam state in torch.optim.Adam's layout (a plain Adam over the same parameters loads it, and vice versa)."""

    def __init__(self, engine, params):
        lr = float(engine.adam_state[1])
        super().__init__(params, dict(lr=lr, betas=tuple(engine.betas), eps=engine.eps, weight_decay=engine.weight_decay,
                                      amsgrad=False, maximize=False))
        self.engine = engine
        self._pushed_lr = lr

    def sync_lr(self) -> None:
        """Push a learning rate a scheduler wrote into param_groups to the engine (host floats compared: no sync)."""
        lr = self.param_groups[0]["lr"]
        if lr != self._pushed_lr:
            self.engine.set_lr(float(lr))
            self._pushed_lr = lr

    @torch.no_grad()
    def step(self, closure=None):
        return closure() if closure is not None else None

    def zero_grad(self, set_to_none: bool = True) -> None:
        pass

    def state_dict(self) -> dict:
        self.sync_lr()
        return self.engine.optimizer_state_dict()

    def load_state_dict(self, state_dict: dict) -> None:
        self.engine.load_optimizer_state_dict(state_dict)
        if state_dict.get("param_groups"):
            lr = state_dict["param_groups"][0]["lr"]
            for g in self.param_groups:
                g["lr"] = lr
            self._pushed_lr = lr


class _MultiLossModule(nn.Module):
    MODS: Tuple[str, str] = ("a", "b")

    def __init__(self, model_cfg, optimizer_cfg, **kwargs):
        super().__init__()
        self.model_cfg = _Cfg(model_cfg if isinstance(model_cfg, dict) else dict(model_cfg))
        self.optimizer_cfg = dict(optimizer_cfg)
        self.scheduler_patience = self.optimizer_cfg.pop("scheduler_patience", 5)       # models/avmnist.py:171
        if self.model_cfg.get("use_softadapt", False):
            raise NotImplementedError("use_softadapt: loss re-weighting schemes are outside this build's scope")
        # Gradient-Blending (models/avmnist.py:211-217, models/mimic.py:68-74): the reference reads `gradblend`; `use_gradblend`
        # is accepted as an alias.  gb_epochs (extension): the retraining epochs of a refresh (gradblend.py:27: 20)
        self.use_gradblend = bool(self.model_cfg.get("gradblend", False) or self.model_cfg.get("use_gradblend", False))
        if self.use_gradblend and self.GB_ORDER is None:
            raise NotImplementedError(f"gradblend: the reference has no Gradient-Blending for {type(self).__name__}")
        self.gb_update_freq = int(self.model_cfg.get("gb_update_freq", 20))
        self.gb_epochs = int(self.model_cfg.get("gb_epochs", 20))
        self.gb_weights = None                       # [w, w, w] in the reference's list order (GB_ORDER) once computed
        self.mute = self.model_cfg.get("mute", None)
        self.freeze_modalities_on_epoch = self.model_cfg.get("freeze_modalities_on_epoch", None)
        self.random_modality_muting_on_freeze = self.model_cfg.get("random_modality_muting_on_freeze", False)
        self.muting_probs = self.model_cfg.get("muting_probs", None)
        self.fusion_loss_weight = self.model_cfg.get("fusion_loss_weight", 1.0 / 3)
        # the loss-weight schedule of validation_epoch_end (models/avmnist.py:197-198, :338-339; models/mimic.py:54-55, :149-150)
        self.fusion_loss_change = self.model_cfg.get("fusion_loss_change", 0)
        self.loss_change_epoch = self.model_cfg.get("loss_change_epoch", 0)
        self.modalities_freezed = False
        self.current_epoch = 0                       # a trainer sets it (Lightning property in the reference)
        self.dropout = self.model_cfg.get("dropout", 0.0)
        self._engine = None                          # bind_engine: the fused engine whose buffers hold this module's parameters
        self._two_stage = False                      # bind_engine(..., two_stage=True): the bound engine follows the freeze epoch
        self._test_record = False                    # bind_engine(..., test_record=True): test_step appends to the engine's "test" record
        self._engine_optimizer: Optional[EngineOptimizer] = None     # the latest configure_optimizers() of a bound module

    #: the heads in the order of the reference's `gb_weights` list (None: the task has no Gradient-Blending)
    GB_ORDER: Optional[Tuple[str, str, str]] = None

    def _gb_loss(self, losses: Dict[str, torch.Tensor]):
        """The Gradient-Blending total (models/avmnist.py:283-288, models/mimic.py:116-124) of {head name: loss}, in every mode;
        None while there are no weights."""
        if not self.use_gradblend or self.gb_weights is None:
            return None
        w = dict(zip(self.GB_ORDER, self.gb_weights))
        a, b = self.MODS
        return w["fusion"] * losses["fusion"] + w[a] * losses[a] + w[b] * losses[b]

    def on_train_epoch_start(self, data=None, split: str = "train"):
        """models/avmnist.py:219-234: every `gb_update_freq` epochs recompute the Gradient-Blending weights.  A bound module
        runs gradblend.GradBlend on its engine over `data` (the resident training split: data.ResidentTensors /
        ResidentAVMnist; val = its first 10 %) and writes the weights into the engine's loss-weight table (set_loss_weights: the
        captured graph is kept and follows).  Returns the new {head: weight}, or None when nothing was due."""
        if not self.use_gradblend or self.current_epoch % self.gb_update_freq != 0:
            return None
        if self._engine is None:
            raise RuntimeError("on_train_epoch_start: Gradient-Blending runs on the fused engine: bind_engine(batch_size) first "
                               "(an unbound module takes gb_weights as given)")
        if data is None:
            raise ValueError("on_train_epoch_start: gradblend needs the resident training split (data=)")
        from .gradblend import GradBlend
        w = GradBlend(self._engine, data, split=split, epochs=self.gb_epochs, seed=self.current_epoch).get_weights()
        self.gb_weights = [w[h] for h in self.GB_ORDER]
        self._engine.set_loss_weights(*(w[h] for h in self._engine.HEAD_NAMES))
        return w

    # ---- pieces shared by the three tasks ----------------------------------------------------------------
    def _fusion_and_heads(self, n_a: int, n_b: int, dim_a: int, dim_b: int):
        m = self.model_cfg.modalities
        a, b = self.MODS
        self.fusion_function = modules.get_fusion_by_name(**m.multimodal)
        num_patches = self.fusion_function.get_output_shape(n_a, n_b, dim=1)
        self.fusion_mixer = modules.get_block_by_name(**m.multimodal, num_patches=num_patches, dropout=self.dropout)
        K = m.classification.num_classes
        setattr(self, f"classifier_{a}", nn.Linear(dim_a, K))
        setattr(self, f"classifier_{b}", nn.Linear(dim_b, K))
        self.classifier_fusion = modules.get_classifier_by_name(**m.classification)

    def _maybe_freeze_and_mute(self, mode: Optional[str]):
        """Epoch-triggered freezing / random muting, models/avmnist.py:243-251 (train mode only)."""
        if mode != "train":
            return None
        if self.freeze_modalities_on_epoch is not None and self.current_epoch == self.freeze_modalities_on_epoch \
                and not self.modalities_freezed:
            self._freeze_modalities()
        if self.random_modality_muting_on_freeze and self.freeze_modalities_on_epoch is not None \
                and self.current_epoch >= self.freeze_modalities_on_epoch:
            names = list(self.MODS) + ["multimodal"]
            self.mute = np.random.choice(names, p=[self.muting_probs[n] for n in names])
        return self.mute

    def _freeze_modalities(self):
        """models/avmnist.py:314-324: the two towers and their heads stop training, the fusion part continues."""
        a, b = self.MODS
        for name in (f"{a}_mixer", f"{b}_mixer", f"classifier_{a}", f"classifier_{b}", "static_extractor", "time_mixer"):
            mod = getattr(self, name, None)
            if mod is not None:
                for p in mod.parameters():
                    p.requires_grad = False
        self.modalities_freezed = True
        if self._engine is not None and self._two_stage:
            # bound: the engine family enters stage two; its captured graph is gone, the next full batch captures stage two's
            self._engine.freeze_modalities()
            self._replay = None

    # ---- checkpoint I/O ------------------------------------------------------------
    checkpoint_path: Optional[str] = None
    #: the per-step outputs the reference's test_epoch_end concatenates and dumps (models/avmnist.py:382-398)
    TEST_PRED_KEYS: Tuple[str, ...] = ()

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location=None, hparams_file=None, strict: bool = True, **kwargs):
        """Build the module from `model_cfg` / `optimizer_cfg` (passed as the reference's run.py:48-50 does) and load the
        weights of a Lightning `.ckpt` -- a torch.save'd dict whose `state_dict` uses exactly the sub-module names of this
        class (models/avmnist.py:400-411 remembers the path for the test_preds.pt dump; so does this).
        trusted=True allows the full unpickler for checkpoints that carry foreign pickled classes (see _load_checkpoint_file)."""
        if "model_cfg" not in kwargs or "optimizer_cfg" not in kwargs:
            raise TypeError("load_from_checkpoint needs model_cfg= and optimizer_cfg= (the reference passes both, run.py:48-50)")
        ckpt = _load_checkpoint_file(checkpoint_path, map_location or "cpu", kwargs.pop("trusted", False))
        state = ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt
        model = cls(kwargs.pop("model_cfg"), kwargs.pop("optimizer_cfg"), **kwargs)
        model.load_state_dict(state, strict=strict)
        model.checkpoint_path = str(checkpoint_path)
        model.current_epoch = int(ckpt.get("epoch", 0)) if isinstance(ckpt, dict) else 0
        return model

    def save_checkpoint(self, path, epoch: Optional[int] = None, global_step: int = 0, engine=None) -> str:
        """A `.ckpt` in Lightning's top-level layout (`state_dict`, `epoch`, `global_step`, `pytorch-lightning_version`,
        `optimizer_states`, `lr_schedulers`): what load_from_checkpoint -- this one or a LightningModule's -- reads.
        engine: a fused engine trained over these weights; its parameters are written instead of the module's and its Adam
        state goes to `optimizer_states[0]` in torch.optim.Adam's state_dict layout (parameter index = position in
        `parameters()` order), so training can resume (engine.load_optimizer_state_dict)."""
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        sd = {k: v.detach().cpu() for k, v in self.state_dict().items()}
        ckpt = {"state_dict": sd, "epoch": self.current_epoch if epoch is None else int(epoch), "global_step": int(global_step),
                "pytorch-lightning_version": LIGHTNING_VERSION, "optimizer_states": [], "lr_schedulers": []}
        if engine is None and self._engine is not None:
            engine = self._engine                    # bound: the optimizer state is the engine's
            if self._engine_optimizer is not None:
                self._engine_optimizer.sync_lr()
        if engine is not None:
            for k, v in engine.state_dict().items():
                sd[k] = v.detach().cpu()
            ckpt["optimizer_states"] = [engine.optimizer_state_dict()]
        torch.save(ckpt, path)
        self.checkpoint_path = str(path)
        return str(path)

    def save_test_preds(self, outputs: Optional[Sequence[Dict[str, torch.Tensor]]] = None, save_dir: Optional[str] = None) -> str:
        """test_epoch_end's dump (models/avmnist.py:382-398): the listed shared_step outputs of every test batch,
        concatenated, as `test_preds.pt` next to the checkpoint.  outputs=None (a module bound with test_record=True): the same
        file from the engine's "test" prediction record, which every test_step appended to on the device -- read back once, then
        emptied for the next test pass."""
        if save_dir is None:
            if self.checkpoint_path is None:
                raise RuntimeError("save_test_preds: no checkpoint path to save next to; pass save_dir")
            save_dir = os.path.dirname(self.checkpoint_path)
        os.makedirs(save_dir or ".", exist_ok=True)
        if not self.TEST_PRED_KEYS:
            raise NotImplementedError(f"{type(self).__name__}: the reference dumps no test predictions for this task")
        path = os.path.join(save_dir, "test_preds.pt")
        if outputs is None:
            if self._engine is None:
                raise RuntimeError("save_test_preds: outputs=None reads a bound engine's test record; this module is not bound "
                                   "(pass the list of test_step outputs)")
            if not self._test_record:
                raise RuntimeError("save_test_preds: outputs=None needs bind_engine(..., test_record=True); this module was bound "
                                   "without the record (pass the list of test_step outputs)")
            rec = self._engine.prediction_record("test")
            rec.save(path, self.TEST_PRED_KEYS)
            rec.reset()
            return path
        out = {k: torch.cat([o[k].detach().cpu() for o in outputs]) for k in self.TEST_PRED_KEYS}
        torch.save(out, path)
        return path

    def configure_optimizers(self) -> Dict[str, Any]:
        """models/avmnist.py:413-422.  Bound to an engine (bind_engine): the optimizer is an EngineOptimizer -- the engine's
        fused Adam, which every training_step already applies; ReduceLROnPlateau drives its learning rate as usual."""
        from torch.optim.lr_scheduler import ReduceLROnPlateau
        if self._engine is not None:
            optimizer = self._engine_optimizer = EngineOptimizer(self._engine, list(self.parameters()))
        else:
            optimizer = torch.optim.Adam(filter(lambda p: p.requires_grad, self.parameters()), **self.optimizer_cfg)
        return {"optimizer": optimizer, "lr_scheduler": ReduceLROnPlateau(optimizer, patience=self.scheduler_patience),
                "monitor": "val_loss"}

    def _engine_cfg(self) -> dict:
        m = _plain(self.model_cfg.modalities)
        cfg = {k: v for k, v in m.items() if k != "classification"}
        cfg["dropout"] = self.dropout
        cfg["num_classes"] = m["classification"]["num_classes"]
        return cfg

    def _engine_kwargs(self) -> dict:
        oc = self.optimizer_cfg
        return dict(lr=oc.get("lr", oc.get("learning_rate", 1e-3)), betas=tuple(oc.get("betas", (0.9, 0.999))),
                    eps=oc.get("eps", 1e-8), weight_decay=oc.get("weight_decay", 0.0))

    def to_engine(self, batch_size: int, precision: Optional[str] = None, scores: bool = False, rank_scores: bool = False,
                  rank_capacity: int = 65536):
        """The fused training engine (engine.py) over a copy of this module's weights.  scores, rank_scores, rank_capacity: see
        bind_engine."""
        eng = self._make_engine(self._engine_cfg(), batch_size, next(self.parameters()).device, precision, scores=scores,
                                rank_scores=rank_scores, rank_capacity=rank_capacity)
        eng.load_state_dict(self.state_dict())
        return eng

    # ---- engine-backed mode ----------------------------------------------------------------------------------
    @property
    def engine(self):
        """The fused engine this module is bound to (bind_engine), or None."""
        return self._engine

    def bind_engine(self, batch_size: int, precision: Optional[str] = None, scores: bool = False, rank_scores: bool = False,
                    rank_capacity: int = 65536, two_stage: bool = False, test_record: bool = False, record_capacity: int = 65536):
        """Engine-backed mode: build the fused engine (engine.py) for `batch_size`, copy this module's weights into it, then
        point every parameter's `.data` at the engine's buffer (`engine.params[key]`): the Parameter objects stay the same,
        `parameters()`, `state_dict()`, `save_checkpoint()` read the live weights, and no copy is taken again.  From then on
        training_step replays the engine's captured step, validation_step / test_step run its evaluation, configure_optimizers
        returns an EngineOptimizer and validation_epoch_end forwards the loss-weight schedule to the engine.
        A LightningModule subclass sets `automatic_optimization = False` when bound: the replayed step already updated the
        weights (EngineOptimizer.step is a no-op).  Refused by default: epoch-triggered freezing and random muting; a fixed `mute`
        is supported.
        two_stage=True accepts `freeze_modalities_on_epoch` and `random_modality_muting_on_freeze`: training_step then runs the
        reference's draw and freeze first (_maybe_freeze_and_mute); at the freeze epoch the engine enters stage two
        (engine.freeze_modalities: loss_fusion alone, the modality towers and their heads untouched, their backward skipped) and
        the next full batch captures the stage-two graph; the per-step draw reaches the engine as a zeroed input.  A module
        already frozen when bound freezes its engine at once.
        scores=True: training_step / validation_step / test_step also add their batch's counts into the train / val / test count
        tables on the device (the reference's three setup_scores dictionaries; one small launch per step, inside the captured
        graph for training), and training_epoch_end / validation_epoch_end / test_epoch_end return the reference's scores.
        Off (the default): no table, no launch.
        rank_scores=True (AV-MNIST, MIMIC): the steps also append the softmax of their logits to the train / val / test ranking
        buffers on the device (engine.RankBuffer, `rank_capacity` rows each: a split must fit), and the three epoch-end hooks
        return the ranking scores as well (scores.RANK_SCORES: MIMIC's `auroc`, the reference's name for macro average
        precision, models/mimic.py:162-180; AV-MNIST `ap_macro`, `roc_auc_macro`) -- merged with the count-table scores, or on
        their own with scores=False.  Off (the default): no buffer, no launch.
        test_record=True: test_step also appends its batch's logits, predictions and labels to the engine's "test" prediction
        record on the device (engine.PredictionRecord, `record_capacity` rows: the test split must fit; every batch size shares
        the one record), and save_test_preds() without a list writes test_preds.pt from it.  Off (the default): no record, no
        launch."""
        if self._engine is not None:
            raise RuntimeError("bind_engine: this module is already bound to an engine")
        if not two_stage:
            if self.freeze_modalities_on_epoch is not None or self.modalities_freezed:
                raise NotImplementedError("bind_engine: freeze_modalities_on_epoch -- the fused engine trains every parameter")
            if self.random_modality_muting_on_freeze:
                raise NotImplementedError("bind_engine: random_modality_muting_on_freeze -- the fused engine has no random muting")
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("bind_engine: the module must be on the GPU (.to('cuda')) first; the engine has no CPU path")
        eng = self._make_engine(self._engine_cfg(), batch_size, dev, precision, scores=scores, rank_scores=rank_scores,
                                rank_capacity=rank_capacity)
        eng.load_state_dict(self.state_dict())
        with torch.no_grad():
            for k, p in self.named_parameters():
                p.data = eng.params[k]
        self._bind_buffers(eng)
        self._engine = eng
        self._two_stage = bool(two_stage)
        self._test_record = bool(test_record)
        if self._test_record:
            eng.prediction_record("test", record_capacity)
        if self._two_stage and self.modalities_freezed:
            eng.freeze_modalities()
        self._replay = None
        self._eval_siblings: Dict[int, Any] = {}
        self._engine_version = 0                     # += 1 whenever the weights change (an engine step, a load_state_dict)
        self._hip_modules = [m for m in self.modules() if hasattr(m, "invalidate_packs")]
        self._invalidate_module_packs()
        return eng

    def _bind_buffers(self, eng):
        """Loss-module buffers that live in the engine (MM-IMDb's pos_weight)."""

    def _invalidate_module_packs(self):
        # the engine updates the weights without advancing autograd's version counters: the module's own tower / embedding
        # runtimes would keep their packed copies; a later shared_step / forward re-packs
        for m in self._hip_modules:
            m.invalidate_packs()

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        if self._engine is None:
            return super().load_state_dict(state_dict, strict=strict, assign=assign)
        if assign:
            raise RuntimeError("load_state_dict(assign=True) would detach the parameters from the bound engine")
        self._check_engine_state(state_dict)
        res = super().load_state_dict(state_dict, strict=strict)       # writes into the engine's buffers (the parameters' views)
        self._engine.pack()
        self._engine_version += 1
        self._invalidate_module_packs()
        return res

    def _check_engine_state(self, state_dict):
        pass

    def _engine_batch(self, batch, train: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(input a, input b, labels) in the engine's layout, with shared_step's fixed muting in train mode."""
        raise NotImplementedError

    def _two_tower_batch(self, batch, train: bool, labels):
        a, b = self.MODS
        xa, xb = batch[a], batch[b]
        if train and self.mute == a:                 # shared_step's fixed muting (train mode only)
            xa = torch.zeros_like(xa)
        elif train and self.mute == b:
            xb = torch.zeros_like(xb)
        return xa.float(), xb.float(), labels

    def _engine_train_outputs(self, eng, labels) -> Dict[str, torch.Tensor]:
        a, b = self.MODS
        l = eng.losses.clone()
        return {"loss": l[3], f"loss_{a}": l[0], f"loss_{b}": l[1], "loss_fusion": l[2], "preds": self._engine_preds(eng.preds[2], eng.logits[2]),
                "labels": labels}

    def _engine_preds(self, preds, logits) -> torch.Tensor:
        """shared_step's `preds` from the engine's (int32 decisions, logits) of one head -- a new tensor."""
        return preds.long()

    def _engine_eval_outputs(self, eng, batch, labels) -> Dict[str, torch.Tensor]:
        """shared_step(mode="val") of the two-tower models: same keys, same meanings."""
        a, b = self.MODS
        l, lg, pr = eng.losses.clone(), eng.logits.clone(), eng.preds.long()
        return {"preds": pr[2], f"preds_{a}": pr[0], f"preds_{b}": pr[1], "labels": batch["label"], "loss": l[3],
                f"loss_{a}": l[0], f"loss_{b}": l[1], "loss_fusion": l[2], f"{a}_logits": lg[0], f"{b}_logits": lg[1],
                "logits": lg[2]}

    def _train_sibling(self, bs: int):
        eng = self._engine
        if bs not in eng._tail_engines and self._replay is not None:
            # sibling() may narrow the gradient ranges the captured update leaves uncleared: capture again afterwards
            self._replay = None
            eng.release_capture()
        sib = tail_engine_for(eng, bs)               # (kept in engine._tail_engines, the one store of training tails)
        self._link_sibling(sib)
        return sib

    def _eval_sibling(self, bs: int):
        sib = self._eval_siblings.get(bs)
        if sib is None:
            sib = self._eval_siblings[bs] = self._engine.sibling(bs, trains=False)
            self._link_sibling(sib)
            sib._bound_version = -1
        if sib._bound_version != self._engine_version:
            sib.pack()                               # its packed copies missed the steps since its last use
            sib._bound_version = self._engine_version
        return sib

    def _link_sibling(self, sib):
        pass

    def training_step(self, batch, batch_idx: int = 0) -> Dict[str, torch.Tensor]:
        """modules/train_test_module.py:72-84.  Unbound: shared_step(batch, mode="train").  Bound: one fused training step --
        the captured graph for full batches (captured on the first one), a training sibling for any other batch size (the
        ragged last batch of an epoch).  Returns the loss keys of shared_step, `preds` and `labels`: device tensors CLONED out
        of the engine's buffers (the next replay overwrites those); nothing synchronises with the host."""
        eng = self._engine
        if eng is None:
            return self.shared_step(batch, mode="train")
        if self._two_stage:
            self._maybe_freeze_and_mute("train")     # the reference's freeze at its epoch and the per-step draw (self.mute)
        elif self.modalities_freezed:
            raise NotImplementedError("a bound module trains every parameter: freezing is not supported")
        xa, xb, labels = self._engine_batch(batch, train=True)
        if self._engine_optimizer is not None:
            self._engine_optimizer.sync_lr()         # ReduceLROnPlateau's cut (host floats compared: no sync)
        bs = labels.shape[0]
        if bs == eng.B:
            if self._replay is None:
                self._replay = eng.capture(xa, xb, labels)
            self._replay(xa, xb, labels)
            src = eng
        else:
            src = self._train_sibling(bs)
            with tail_step(eng, src, True):
                src.train_step(xa.contiguous(), xb.contiguous(), labels.contiguous())
        self._engine_version += 1
        self._invalidate_module_packs()
        return self._engine_train_outputs(src, labels)

    def _eval_step(self, batch, mode: str) -> Dict[str, torch.Tensor]:
        if self._engine is None:
            return self.shared_step(batch, mode=mode)
        xa, xb, labels = self._engine_batch(batch, train=False)
        sib = self._eval_sibling(labels.shape[0])
        record = self._engine.prediction_record("test") if mode == "test" and self._test_record else None
        accs = pass_accumulators(self._engine, mode, record=record)
        sib.evaluate(xa.contiguous(), xb.contiguous(), labels.contiguous(), **accs.kwargs())
        return self._engine_eval_outputs(sib, batch, labels)

    def _epoch_scores(self, split: str) -> Optional[Dict[str, float]]:
        """compute() of `split`'s table under the reference's logging names (`<split>_<metric>`), then reset it -- what the
        torchmetrics objects do at an epoch end under Lightning.  One device-to-host copy."""
        if self._engine is None:
            return None
        accs = pass_accumulators(self._engine, split, train=split == "train")      # ("train": the training steps' own)
        if not accs.kwargs():
            return None
        out = {f"{split}_{k}": v for k, v in accs.compute().items()}
        accs.reset()                                 # (the table and the ranking buffer restart empty)
        return out

    def training_epoch_end(self, outputs=None) -> Optional[Dict[str, float]]:
        """modules/train_test_module.py:86-92: {"train_<metric>": float} of the epoch's training steps (bound with scores=True;
        else None); the training table starts the next epoch empty."""
        return self._epoch_scores("train")

    def test_epoch_end(self, outputs=None) -> Optional[Dict[str, float]]:
        """modules/train_test_module.py:144-151: {"test_<metric>": float} (bound with scores=True; else None)."""
        return self._epoch_scores("test")

    def validation_step(self, batch, batch_idx: int = 0) -> Dict[str, torch.Tensor]:
        """modules/train_test_module.py:94-104.  Bound: the engine's evaluation (dropout off) through an evaluating sibling per
        batch size; the keys and meanings of shared_step(mode="val"), as cloned device tensors."""
        return self._eval_step(batch, "val")

    def test_step(self, batch, batch_idx: int = 0) -> Dict[str, torch.Tensor]:
        """modules/train_test_module.py:132-142 (see validation_step); save_test_preds takes a list of these."""
        return self._eval_step(batch, "test")

    #: whether validation_epoch_end applies the fusion-loss-weight schedule (the reference's AV-MNIST and MIMIC models do)
    LOSS_SCHEDULE = True
    #: whether the schedule reaches a bound engine (False: the model's loss ignores fusion_loss_weight, only the attribute moves)
    ENGINE_LOSS_SCHEDULE = True

    def validation_epoch_end(self, outputs=None) -> Optional[Dict[str, float]]:
        """The loss-weight schedule of models/avmnist.py:338-339 / models/mimic.py:149-150: from epoch `loss_change_epoch` on,
        fusion_loss_weight grows by `fusion_loss_change` per validation epoch, up to 1.  Bound: forwarded to the engine, whose
        captured step reads the new coefficients on its next replay.  Bound with scores=True it also returns
        {"val_<metric>": float} (modules/train_test_module.py:106-111) and resets the validation table; else None.
        (The reference's logging part is Lightning's.)"""
        scores = self._epoch_scores("val")
        if not self.LOSS_SCHEDULE or self.current_epoch < self.loss_change_epoch:
            return scores
        new = min(1, self.fusion_loss_weight + self.fusion_loss_change)
        if new == self.fusion_loss_weight:
            return scores
        if self._engine is not None and self.ENGINE_LOSS_SCHEDULE and self.gb_weights is None:
            # (with Gradient-Blending weights in place the reference's loss no longer reads fusion_loss_weight: only the
            # attribute moves)
            self._engine.set_fusion_loss_weight(float(new))
        self.fusion_loss_weight = new
        return scores


class AVMnistMixerMultiLoss(_MultiLossModule):
    """batch = {'image': (B,1,28,28), 'audio': (B,1,112,112), 'label': (B,)}"""

    MODS = ("image", "audio")
    GB_ORDER = ("audio", "image", "fusion")         # on_train_epoch_start hands the encoders over as [audio, image] (models/avmnist.py:221)

    TEST_PRED_KEYS = ("preds", "preds_image", "preds_audio", "labels", "image_logits", "audio_logits", "logits")

    def __init__(self, model_cfg, optimizer_cfg, **kwargs):
        super().__init__(model_cfg, optimizer_cfg, **kwargs)
        m = self.model_cfg.modalities
        self.image_mixer = modules.get_block_by_name(**m.image, dropout=self.dropout)
        self.audio_mixer = modules.get_block_by_name(**m.audio, dropout=self.dropout)
        self._fusion_and_heads(self.image_mixer.num_patch, self.audio_mixer.num_patch, m.image.hidden_dim, m.audio.hidden_dim)
        self.image_criterion = self.audio_criterion = self.fusion_criterion = nn.CrossEntropyLoss()

    def shared_step(self, batch, **kwargs):
        image, audio, labels = batch["image"], batch["audio"], batch["label"]
        mode = kwargs.get("mode", None)
        mute = self._maybe_freeze_and_mute(mode)
        if mode == "train" and mute == "image":
            image = torch.zeros_like(image)
        elif mode == "train" and mute == "audio":
            audio = torch.zeros_like(audio)
        image_tok = self.image_mixer(image)
        audio_tok = self.audio_mixer(audio)
        fused = self.fusion_mixer(self.fusion_function(image_tok, audio_tok))
        image_logits = self.classifier_image(image_tok.mean(dim=1))
        audio_logits = self.classifier_audio(audio_tok.mean(dim=1))
        logits = self.classifier_fusion(fused)
        loss_image = self.image_criterion(image_logits, labels)
        loss_audio = self.audio_criterion(audio_logits, labels)
        loss_fusion = self.fusion_criterion(logits, labels)
        ow = (1 - self.fusion_loss_weight) / 2
        loss = (self.fusion_loss_weight * loss_fusion + ow * loss_image + ow * loss_audio) * 3     # models/avmnist.py:289-290
        gb = self._gb_loss({"image": loss_image, "audio": loss_audio, "fusion": loss_fusion})
        if gb is not None:
            loss = gb                                                                              # models/avmnist.py:283-288 (no x3)
        if self.modalities_freezed and mode == "train":
            loss = loss_fusion
        return {"preds": logits.argmax(dim=1), "preds_image": image_logits.argmax(dim=1),
                "preds_audio": audio_logits.argmax(dim=1), "labels": labels, "loss": loss, "loss_image": loss_image,
                "loss_audio": loss_audio, "loss_fusion": loss_fusion, "image_logits": image_logits,
                "audio_logits": audio_logits, "logits": logits}

    def _engine_batch(self, batch, train):
        return self._two_tower_batch(batch, train, batch["label"].long())

    def _make_engine(self, cfg, batch_size, device, precision, scores=False, rank_scores=False, rank_capacity=65536):
        from .engine import AVMnistEngine
        return AVMnistEngine(cfg, batch_size, device=device, precision=precision,
                             fusion_loss_weight=self.fusion_loss_weight, init=False, scores=scores, rank_scores=rank_scores,
                            rank_capacity=rank_capacity, **self._engine_kwargs())


def edl_mse_loss(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """The reference's EDLMSELoss (modules/losses.py:5-31): the squared-error Bayes risk of the Dirichlet with evidence relu(logits),
    batch mean.  Its KL term is multiplied by annealing_coef * 0 (losses.py:20) -- no value, no gradient, no effect of the epoch --
    and is left out."""
    alpha = torch.relu(logits) + 1.0
    strength = alpha.sum(dim=-1, keepdim=True)
    p = alpha / strength
    target = torch.nn.functional.one_hot(labels, logits.shape[-1]).to(logits.dtype)
    return ((target - p) ** 2 + p * (1 - p) / (strength + 1)).sum(dim=-1).mean()


def edl_ce_loss(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """The cross-entropy Bayes risk of the reference's EDLCELoss (modules/losses.py:89-93): psi(S) - psi(alpha_y), batch mean."""
    alpha = torch.relu(logits) + 1.0
    alpha_y = alpha.gather(-1, labels.unsqueeze(-1)).squeeze(-1)
    return (torch.digamma(alpha.sum(dim=-1)) - torch.digamma(alpha_y)).mean()


def kl_divergence_loss(evidence: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """The reference's kl_divergence_loss (modules/losses.py:52-68; :33-49 is the same function as a method): KL(Dir(at) || Dir(1))
    with the label's evidence removed -- at = alpha off the label, 1 on it -- batch mean.  evidence (B, K) >= 0, target one-hot."""
    at = target + (1 - target) * (evidence + 1.0)
    st = at.sum(dim=-1)
    k = at.new_tensor(float(evidence.shape[-1]))
    log_norm = torch.lgamma(st) - torch.lgamma(k) - torch.lgamma(at).sum(dim=-1)
    spread = ((at - 1) * (torch.digamma(at) - torch.digamma(st).unsqueeze(-1))).sum(dim=-1)
    return (log_norm + spread).mean()


def annealing_coef(epoch_num, annealing_step) -> torch.Tensor:
    """min(1, epoch_num / annealing_step) as the reference takes it: float32 (modules/losses.py:15-18, :81-84)."""
    return torch.min(torch.tensor(1.0, dtype=torch.float32), torch.tensor(epoch_num / annealing_step, dtype=torch.float32))


class _EDLLoss(nn.Module):
    """A Bayes risk + kl_weight x annealing_coef(epoch_num) x kl_divergence_loss: no parameters, no buffers.  kl_weight = 0 (the
    default, what the reference's models train with) adds nothing, not even a zero."""

    risk = None

    def __init__(self, num_classes: int, annealing_step: int = 10, kl_weight: float = 0.0):
        super().__init__()
        self.num_classes, self.annealing_step, self.kl_weight = num_classes, annealing_step, float(kl_weight)

    def forward(self, output, y, epoch_num: int = 0):
        loss = type(self).risk(output, y)
        if self.kl_weight == 0.0:
            return loss
        target = torch.nn.functional.one_hot(y, output.shape[-1]).to(output.dtype)
        lam = self.kl_weight * annealing_coef(epoch_num, self.annealing_step).to(output.device)
        return loss + lam * kl_divergence_loss(torch.relu(output), target)


class EDLMSELoss(_EDLLoss):
    """The reference's criterion module (modules/losses.py:5-31) around edl_mse_loss.  With the default kl_weight = 0 `epoch_num`
    is accepted and has no effect (the reference's KL term is times 0); kl_weight > 0 is this build's extension."""

    risk = staticmethod(edl_mse_loss)


class EDLCELoss(_EDLLoss):
    """The reference's EDLCELoss (modules/losses.py:71-93) around edl_ce_loss, with the same optional KL term."""

    risk = staticmethod(edl_ce_loss)


EDL_LOSSES = {"mse": EDLMSELoss, "ce": EDLCELoss}


class AVMnistMixerMultiLossUQ(AVMnistMixerMultiLoss):
    """models/avmnist.py:447-572: AVMnistMixerMultiLoss with three EDLMSELoss criteria (which hold no parameters or buffers: the
    state-dict keys are the parent's), loss = loss_image + loss_audio + loss_fusion (:511; fusion_loss_weight is ignored),
    per-head uncertainties K / S and `preds` = the prediction of the strictly least uncertain head (:533-537).  Bound, it runs
    engine.AVMnistUQEngine; the inherited fusion_loss_change schedule still moves the module attribute, as in the reference, and
    does not reach the engine."""

    ENGINE_LOSS_SCHEDULE = False
    GB_ORDER = None                                  # (models/avmnist.py:447-572 has no Gradient-Blending)

    def __init__(self, model_cfg, optimizer_cfg, **kwargs):
        super().__init__(model_cfg, optimizer_cfg, **kwargs)
        self.num_classes = self.model_cfg.modalities.classification.num_classes
        # models/avmnist.py:451-453 hard-codes EDLMSELoss(num_classes, 10); the three keys are this build's extension
        self.edl_loss = self.model_cfg.get("edl_loss", "mse")
        self.kl_weight = float(self.model_cfg.get("kl_weight", 0.0))
        self.annealing_step = self.model_cfg.get("annealing_step", 10)
        if self.edl_loss not in EDL_LOSSES:
            raise ValueError(f"edl_loss must be one of {', '.join(EDL_LOSSES)}, got {self.edl_loss!r}")
        make = lambda: EDL_LOSSES[self.edl_loss](self.num_classes, self.annealing_step, self.kl_weight)
        self.image_criterion, self.audio_criterion, self.fusion_criterion = make(), make(), make()
        self._engine_epoch = None                    # the epoch the bound engine's lambda was last written for

    def shared_step(self, batch, **kwargs):
        image, audio, labels = batch["image"], batch["audio"], batch["label"]
        mode = kwargs.get("mode", None)
        mute = self._maybe_freeze_and_mute(mode)
        if mode == "train" and mute == "image":
            image = torch.zeros_like(image)
        elif mode == "train" and mute == "audio":
            audio = torch.zeros_like(audio)
        image_tok = self.image_mixer(image)                                                       # models/avmnist.py:485-500
        audio_tok = self.audio_mixer(audio)
        fused = self.fusion_mixer(self.fusion_function(image_tok, audio_tok))
        image_logits = self.classifier_image(image_tok.mean(dim=1))
        audio_logits = self.classifier_audio(audio_tok.mean(dim=1))
        logits = self.classifier_fusion(fused)
        loss_image = self.image_criterion(image_logits, labels, self.current_epoch)               # :503-505
        loss_audio = self.audio_criterion(audio_logits, labels, self.current_epoch)
        loss_fusion = self.fusion_criterion(logits, labels, self.current_epoch)
        loss = loss_image + loss_audio + loss_fusion                                              # :511
        if self.modalities_freezed and mode == "train":
            loss = loss_fusion
        ev, ev_i, ev_a = torch.relu(logits), torch.relu(image_logits), torch.relu(audio_logits)  # :517-531
        preds, preds_image, preds_audio = ev.argmax(dim=1), ev_i.argmax(dim=1), ev_a.argmax(dim=1)
        u, u_i, u_a = (self.num_classes / (e + 1).sum(dim=1) for e in (ev, ev_i, ev_a))
        combined = (preds * ((u < u_i) & (u < u_a)).long() + preds_image * ((u_i < u) & (u_i < u_a)).long()
                    + preds_audio * ((u_a < u) & (u_a < u_i)).long())                             # :533-537
        return {"preds": combined, "preds_image": preds_image, "preds_audio": preds_audio, "labels": labels, "loss": loss,
                "loss_image": loss_image, "loss_audio": loss_audio, "loss_fusion": loss_fusion, "image_logits": image_logits,
                "audio_logits": audio_logits, "logits": logits, "uncertainty": u.mean(), "uncertainty_image": u_i.mean(),
                "uncertainty_audio": u_a.mean()}

    @staticmethod
    def _engine_uncertainties(eng) -> Dict[str, torch.Tensor]:
        """shared_step's three batch means from the engine's (3, B) buffer (rows image, audio, fusion): new tensors."""
        m = eng.uncertainty.mean(dim=1)
        return {"uncertainty": m[2], "uncertainty_image": m[0], "uncertainty_audio": m[1]}

    def _engine_train_outputs(self, eng, labels):
        out = super()._engine_train_outputs(eng, labels)          # `preds`: the engine's row 2, the combined prediction
        out.update(self._engine_uncertainties(eng))
        return out

    def _engine_eval_outputs(self, eng, batch, labels):
        out = super()._engine_eval_outputs(eng, batch, labels)
        out.update(self._engine_uncertainties(eng))
        return out

    def _engine_cfg(self) -> dict:
        cfg = super()._engine_cfg()
        cfg.update(edl_loss=self.edl_loss, kl_weight=self.kl_weight, annealing_step=self.annealing_step)
        return cfg

    def _follow_epoch(self):
        """Bound: the engine's lambda follows current_epoch (a host comparison; one small fill when the epoch moved)."""
        if self._engine is not None and self._engine_epoch != self.current_epoch:
            self._engine.set_epoch(self.current_epoch)
            self._engine_epoch = self.current_epoch

    def on_train_epoch_start(self, data=None, split: str = "train"):
        self._follow_epoch()
        return super().on_train_epoch_start(data, split)

    def training_step(self, batch, batch_idx: int = 0):
        self._follow_epoch()                         # (ahead of the two-stage switch, which reads current_epoch as well)
        return super().training_step(batch, batch_idx)

    def _eval_step(self, batch, mode: str):
        self._follow_epoch()                         # the reference passes current_epoch in validation too (models/avmnist.py:503-505)
        return super()._eval_step(batch, mode)

    def _make_engine(self, cfg, batch_size, device, precision, scores=False, rank_scores=False, rank_capacity=65536):
        from .engine import AVMnistUQEngine
        return AVMnistUQEngine(cfg, batch_size, device=device, precision=precision, init=False, scores=scores,
                               rank_scores=rank_scores, rank_capacity=rank_capacity, **self._engine_kwargs())


class MMIMDBMixerMultiLoss(_MultiLossModule):
    """batch = {'image': (B,3,160,256), 'text': (B,1,160,256), 'label': (B,23) multi-hot}"""

    MODS = ("image", "text")

    TEST_PRED_KEYS = ("preds", "preds_image", "preds_text", "labels", "image_logits", "text_logits", "logits")   # models/mmimdb.py:194-209
    LOSS_SCHEDULE = False                            # a plain sum of the three losses (models/mmimdb.py:115-123): no schedule

    def __init__(self, model_cfg, optimizer_cfg, **kwargs):
        super().__init__(model_cfg, optimizer_cfg, **kwargs)
        m = self.model_cfg.modalities
        self.image_mixer = modules.get_block_by_name(**m.image, dropout=self.dropout)
        self.text_mixer = modules.get_block_by_name(**m.text, dropout=self.dropout)
        self._fusion_and_heads(self.image_mixer.num_patch, self.text_mixer.num_patch, m.image.hidden_dim, m.text.hidden_dim)
        # three BCEWithLogitsLoss modules under the reference's names (models/mmimdb.py:47-50): their persistent `pos_weight`
        # buffers are part of every reference state_dict (`image_criterion.pos_weight`, ...), so checkpoints round-trip
        pos_weight = torch.tensor(list(self.model_cfg.pos_weight), dtype=torch.float32)
        self.image_criterion = nn.BCEWithLogitsLoss(pos_weight=pos_weight.clone())
        self.text_criterion = nn.BCEWithLogitsLoss(pos_weight=pos_weight.clone())
        self.fusion_criterion = nn.BCEWithLogitsLoss(pos_weight=pos_weight.clone())

    def shared_step(self, batch, **kwargs):
        image, text, labels = batch["image"], batch["text"], batch["label"]
        mode = kwargs.get("mode", None)
        mute = self._maybe_freeze_and_mute(mode)
        if mode == "train" and mute == "image":
            image = torch.zeros_like(image)
        elif mode == "train" and mute == "text":
            text = torch.zeros_like(text)
        image_tok = self.image_mixer(image)
        text_tok = self.text_mixer(text)
        fused = self.fusion_mixer(self.fusion_function(image_tok, text_tok))
        image_logits = self.classifier_image(image_tok.mean(dim=1))
        text_logits = self.classifier_text(text_tok.mean(dim=1))
        logits = self.classifier_fusion(fused)
        y = labels.float()
        loss_image, loss_text = self.image_criterion(image_logits, y), self.text_criterion(text_logits, y)
        loss_fusion = self.fusion_criterion(logits, y)
        loss = loss_image + loss_text + loss_fusion                                              # models/mmimdb.py:115-123
        if self.modalities_freezed and mode == "train":
            loss = loss_fusion
        return {"preds": (logits > 0).long(), "preds_image": (image_logits > 0).long(), "preds_text": (text_logits > 0).long(),
                "labels": labels, "loss": loss, "loss_image": loss_image, "loss_text": loss_text, "loss_fusion": loss_fusion,
                "image_logits": image_logits, "text_logits": text_logits, "logits": logits}

    def _engine_cfg(self):
        cfg = super()._engine_cfg()
        pw = [c.pos_weight for c in (self.image_criterion, self.text_criterion, self.fusion_criterion)]
        if not (torch.equal(pw[0], pw[1]) and torch.equal(pw[0], pw[2])):
            raise RuntimeError("the fused engine takes one pos_weight for all three heads (models/mmimdb.py:47-50 builds them equal)")
        cfg["pos_weight"] = pw[0].detach().cpu().tolist()          # the loaded buffers, not the cfg: a checkpoint may carry its own
        return cfg

    def _engine_batch(self, batch, train):
        return self._two_tower_batch(batch, train, batch["label"].float())

    def _bind_buffers(self, eng):
        # the three criteria's pos_weight buffers ARE the engine's (one tensor: the fused heads take one pos_weight)
        for c in (self.image_criterion, self.text_criterion, self.fusion_criterion):
            c.pos_weight = eng.pos_weight

    def _link_sibling(self, sib):
        sib.pos_weight = self._engine.pos_weight

    def _check_engine_state(self, state_dict):
        keys = [f"{n}_criterion.pos_weight" for n in ("image", "text", "fusion")]
        pw = [state_dict[k] for k in keys if k in state_dict]
        if any(not torch.equal(pw[0].cpu(), p.cpu()) for p in pw[1:]):
            raise RuntimeError("the bound engine takes one pos_weight for all three heads (models/mmimdb.py:47-50 builds them equal)")

    def _make_engine(self, cfg, batch_size, device, precision, scores=False, rank_scores=False, rank_capacity=65536):
        from .engine import MMIMDBEngine
        return MMIMDBEngine(cfg, batch_size, device=device, precision=precision, init=False, scores=scores, rank_scores=rank_scores,
                            rank_capacity=rank_capacity, **self._engine_kwargs())


class MimicMixerMultiLoss(_MultiLossModule):
    """batch = (static (B,5), time (B,24,12), labels (B,))"""

    MODS = ("static", "time")
    GB_ORDER = ("static", "time", "fusion")         # models/mimic.py:116-124

    def __init__(self, model_cfg, optimizer_cfg, **kwargs):
        super().__init__(model_cfg, optimizer_cfg, **kwargs)
        m = self.model_cfg.modalities
        self.time_mixer = modules.get_block_by_name(**m.time, dropout=self.dropout)          # creation order: models/mimic.py:39-40
        self.static_extractor = modules.get_block_by_name(**m.static, dropout=self.dropout)
        self._fusion_and_heads(1, self.time_mixer.num_patch, m.static.output_dim, m.time.hidden_dim)
        self.criterion = nn.CrossEntropyLoss()

    def shared_step(self, batch, mode="train", **kwargs):
        static, time, labels = batch
        static_feat = self.static_extractor(static)
        time_tok = self.time_mixer(time)
        fused = self.fusion_mixer(self.fusion_function(static_feat.unsqueeze(1), time_tok))
        logits_static = self.classifier_static(static_feat)
        logits_time = self.classifier_time(time_tok.mean(1))
        logits = self.classifier_fusion(fused)
        loss_fusion = self.criterion(logits, labels)
        loss_static = self.criterion(logits_static, labels)
        loss_time = self.criterion(logits_time, labels)
        ow = (1 - self.fusion_loss_weight) / 2
        loss = self.fusion_loss_weight * loss_fusion + ow * loss_static + ow * loss_time          # models/mimic.py:115-121 (no x3)
        gb = self._gb_loss({"static": loss_static, "time": loss_time, "fusion": loss_fusion})
        if gb is not None:
            loss = gb                                                                             # models/mimic.py:116-124
        return {"preds": torch.softmax(logits, dim=1), "preds_static": torch.softmax(logits_static, dim=1),
                "preds_time": torch.softmax(logits_time, dim=1), "labels": labels.long(), "loss": loss,
                "loss_fusion": loss_fusion, "loss_static": loss_static, "loss_time": loss_time, "logits": logits,
                "logits_static": logits_static, "logits_time": logits_time}

    def _engine_batch(self, batch, train):
        static, time, labels = batch
        # bound two-stage: stage two's per-step draw (the reference's MIMIC shared_step itself never mutes: a fixed `mute` key
        # stays without effect, bound or not)
        if train and self._two_stage and self.mute == "static":
            static = torch.zeros_like(static)
        elif train and self._two_stage and self.mute == "time":
            time = torch.zeros_like(time)
        return static.float(), time.float(), labels.long()

    def _engine_preds(self, preds, logits):
        return torch.softmax(logits, dim=1)         # shared_step's `preds` are the fusion head's probabilities (models/mimic.py:126)

    def _engine_eval_outputs(self, eng, batch, labels):
        l, lg = eng.losses.clone(), eng.logits.clone()
        p = torch.softmax(lg, dim=2)
        return {"preds": p[2], "preds_static": p[0], "preds_time": p[1], "labels": labels, "loss": l[3],
                "loss_fusion": l[2], "loss_static": l[0], "loss_time": l[1], "logits": lg[2], "logits_static": lg[0],
                "logits_time": lg[1]}

    def _make_engine(self, cfg, batch_size, device, precision, scores=False, rank_scores=False, rank_capacity=65536):
        from .engine import MimicEngine
        return MimicEngine(cfg, batch_size, device=device, precision=precision,
                           fusion_loss_weight=self.fusion_loss_weight, init=False, scores=scores, rank_scores=rank_scores,
                            rank_capacity=rank_capacity, **self._engine_kwargs())
