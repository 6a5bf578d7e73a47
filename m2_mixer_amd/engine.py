"""Fused M2-Mixer training engines: the whole `shared_step` + backward + Adam of the reference's multi-loss
LightningModules as a fixed sequence of libm2mixer launches over flat fp32 parameter / gradient / Adam-state buffers.

  AVMnistEngine   AVMnistMixerMultiLoss   models/avmnist.py:236-312, :413-422   (two patch towers, CE, total x3)
  AVMnistUQEngine AVMnistMixerMultiLossUQ models/avmnist.py:447-572            (AVMnistEngine with evidential losses, plain sum,
                                                                                per-head uncertainty, combined prediction)
  MMIMDBEngine    MMIMDBMixerMultiLoss    models/mmimdb.py:96-147               (two patch towers, BCE(pos_weight), plain sum)
  MimicEngine     MimicMixerMultiLoss     models/mimic.py:93-142                (static MLP + time tower, CE, no x3)

What changes relative to the module path (modules/mixer.py + torch autograd):
  * parameters are views into ONE flat buffer (names = the reference's state-dict keys, in the reference's creation
    order), gradients into ONE flat buffer -> no memset (Adam clears what it consumes), one RCCL all-reduce;
  * the two modality towers write their outputs straight into their parts of the fused (B, N1+N2, D) buffer
    (ConcatFusion costs nothing) and hand the token means to the heads kernel;
  * the three heads, their losses and gradients are one launch;
  * Adam over the whole flat buffer and the re-pack of every operand copy are ONE launch at the end of the step
    (m2m_adam_pack_all); only the MIMIC step on side streams (large batches) updates and re-packs per parameter segment;
  * the step can be captured into a hipGraph (torch.cuda.CUDAGraph); the dropout step counter, the Adam
    step counter and the learning rate live in device memory so replays stay correct;
  * scores=True: the step also adds its batch's counts into an integer table on the device (ScoreTable, csrc/scores.hip), from
    which accuracy / precision / recall / F1 under the reference's names are derived once per epoch (scores.py);
  * rank_scores=True: the step also appends the softmax of its logits to a ranking buffer on the device (RankBuffer,
    csrc/rank.hip), from which MIMIC's `auroc` (macro average precision) and ROC-AUC are derived once per epoch (scores.py);
  * freeze_modalities(): stage two of the reference's two-stage training (models/avmnist.py:292-293, :314-324) -- the loss is
    loss_fusion alone, the modality towers, their embeddings and heads are never written again, and the step skips their
    backward, weight gradients, Adam and re-pack; EpochFeed(muting=True) zeroes one input per step from
    a schedule on the device (csrc/feed.hip: m2m_feed_gather_muted);
  * train_modalities_only(): the mirror image -- the loss is loss_a + loss_b, no fusion function or fusion tower runs, the fusion
    keys are never written (the unimodal models of Gradient-Blending); clone() and probe() are the other two pieces
    gradblend.GradBlend is built from.  Either stage is one Stage record held by the engine family and
    one pair of hooks per engine class (_stage_options, _stage_packs).
  * evaluate(..., record=): the evaluation step also appends its logits, predictions and labels to a prediction record on the
    device (PredictionRecord, csrc/record.hip: the reference's test_preds.pt, read back once); capture_feed_eval() captures whole
    evaluation steps that feed themselves, as capture_feed() captures training steps.
This file is the engines: the step, the stages, the optimizer, capture.  The device-side accumulators (ScoreTable, RankBuffer,
PredictionRecord, EpochFeed) live in accumulators.py, the parameter-layout functions in layout.py; every name stays importable from here.
"""
from __future__ import annotations

from collections import OrderedDict
from contextlib import contextmanager
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import ctypes as C
import weakref

import torch

from . import _lib as L
from . import config
# this module stays the import surface: the accumulators and the layout functions are re-exported under their old names
from .accumulators import EpochFeed, PassAccumulators, PredictionRecord, RankBuffer, ScoreTable  # noqa: F401
from .layout import (ENGINE_FUSIONS, _head_shapes, _is_layer_norm, _num_patch, _tower_shapes,  # noqa: F401
                     avmnist_param_shapes, frozen_key_prefixes, fusion_function_name, fusion_tokens, mimic_param_shapes,
                     trainable_flat_ranges, two_tower_param_shapes)
from .runtime import (AdamPackPlan, BLOCK_FIELDS, BLOCK_KEYS, EmbedRuntime, MlpRuntime, TowerRuntime, heads_bce,
                      heads_ce, heads_edl, can_group, can_group_embeds, can_pack_all, embeds_forward, pack_all,
                      towers_backward, towers_forward, towers_forward_embeds_ok, towers_wgrad, wgrad_slot_groups,
                      _embed_ptrs, _grad_ranges, _tower_ptrs)

_ELEM_FUSION_MODE = {"SumFusion": L.FUSION_SUM, "MeanFusion": L.FUSION_MEAN, "MaxFusion": L.FUSION_MAX}


class Stage(NamedTuple):
    """A training stage of an engine family: what it trains and under which loss.  Stage one (everything, `loss_weights`) is
    the absence of one."""
    name: str                                    # what `_frozen` / `_modal` test
    title: str                                   # the stage in the words of its messages
    weights: Tuple[float, float, float]          # the training coefficients of the heads (HEAD_NAMES order)
    invert: bool                                 # which side of frozen_key_prefixes trains (trainable_flat_ranges' `invert`)


FROZEN = Stage("frozen", "stage two (freeze_modalities)", (0.0, 0.0, 1.0), False)
MODAL = Stage("modal", "the modalities-only stage (train_modalities_only)", (1.0, 1.0, 0.0), True)


def config_fused_update(n_params: int = 0) -> bool:
    """Adam and the operand re-pack as ONE launch (m2m_adam_pack_all) or as two (flat Adam, then m2m_pack_all).
    M2M_FUSED_UPDATE=1 / 0 forces either; default: one launch.
    Measured (round 4): with 32-column-group tiles the one-launch form read W2 in 128-byte row segments 12 KB apart (M2-Mixer-B:
    70-78 us against 60-65 us as two launches); with W2 in 8-row x 512-column tiles (2 KiB runs) and the moment streams
    non-temporal it takes 55-56 us and the step 0.4856 against 0.4912 ms (profiles/r04_ab_results.txt r5l-r5n); MM-IMDb
    (2.7 M parameters, latency-bound launches) 0.4602 against 0.4637 ms per step."""
    env = config.switch("M2M_FUSED_UPDATE")
    if env is not None:
        return env == "1"
    return n_params > 0


def _exchange_mode(grad_sync) -> str:
    """How a step exchanges gradients: "none" (grad_sync None: single GPU), "pipelined" (an object with a true `pipelined`:
    parallel.PipelinedGradSync) or "single" (any other callable(flat_grad) -> scale)."""
    if grad_sync is None:
        return "none"
    return "pipelined" if getattr(grad_sync, "pipelined", False) else "single"


class _FlatEngine:
    """Flat parameter / gradient / Adam buffers, the optimizer, data-parallel hooks and hipGraph capture.
    Subclasses supply `_param_shapes(cfg)`, `_segment_of(key)`, `_build()` (which names `_towers` and `_embeds`),
    `_forward(...)`, `_backward(...)`, `_eval_outputs()` (evaluate's dict) and `_stage_packs()` (what a stage's update re-packs)."""

    #: the task whose score names a ScoreTable of this engine reports (scores.TASK_SCORES)
    SCORES_TASK: str = ""

    def __init__(self, cfg: dict, batch_size: int, device, precision, lr, betas, eps, weight_decay, seed, init, share=None,
                 scores: bool = False, rank_scores: bool = False, rank_capacity: int = 65536):
        """share: another engine of the same model; this one then works on ITS parameters, gradients, Adam state and
        step counters (its own activation buffers and packed operand copies, for another batch size) -- the second,
        smaller step that takes the ragged last batch of an epoch (data.run_epoch).  After a step on one of the two
        the other one's packed copies are stale: call its pack() before using it."""
        self.cfg, self.B = cfg, int(batch_size)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on the GPU only (MI355X); there is no CPU path")
        L.lib()  # fail loudly if the HIP library is absent
        self.prec = config.prec_id(precision)
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        self.p_drop = float(cfg.get("dropout", 0.0))
        self.K = cfg["num_classes"]
        self.shapes = self._param_shapes(cfg)
        n = sum(int(torch.Size(s).numel()) for s in self.shapes.values())
        self.n_params = n
        self._fused_update = config_fused_update(n)          # (read once: the environment at construction decides)
        dev = self.device
        if share is not None:
            if share.n_params != n or list(share.shapes.items()) != list(self.shapes.items()) or share.device != dev:
                raise RuntimeError("share=: the other engine must hold the same model on the same device")
            self.flat_p, self.flat_g, self.flat_m, self.flat_v = share.flat_p, share.flat_g, share.flat_m, share.flat_v
        else:
            self.flat_p, self.flat_g, self.flat_m, self.flat_v = (torch.zeros(n, device=dev) for _ in range(4))
        self.params: Dict[str, torch.Tensor] = OrderedDict()
        self.grads: Dict[str, torch.Tensor] = OrderedDict()
        self.exp_avg: Dict[str, torch.Tensor] = OrderedDict()        # Adam's first / second moments, same keys
        self.exp_avg_sq: Dict[str, torch.Tensor] = OrderedDict()
        bounds: Dict[str, Tuple[int, int]] = {}
        off = 0
        for k, shp in self.shapes.items():
            cnt = int(torch.Size(shp).numel())
            self.params[k] = self.flat_p[off:off + cnt].view(shp)
            self.grads[k] = self.flat_g[off:off + cnt].view(shp)
            self.exp_avg[k] = self.flat_m[off:off + cnt].view(shp)
            self.exp_avg_sq[k] = self.flat_v[off:off + cnt].view(shp)
            seg = self._segment_of(k)
            lo, hi = bounds.get(seg, (off, off))
            if hi != off:
                raise AssertionError(f"segment {seg} is not contiguous in the flat buffer")
            bounds[seg] = (lo, off + cnt)
            off += cnt
        # contiguous segments of the flat buffers, one per tower (the last one also holds the heads)
        self.segments = bounds
        if share is not None:
            self.adam_state, self.drop_step = share.adam_state, share.drop_step
            self.loss_weights, self._loss_weight_group = share.loss_weights, share._loss_weight_group
            self._stage_group = share._stage_group
        else:
            self.adam_state = torch.tensor([0.0, lr, 0.0, 0.0], device=dev)     # [step, lr, -, -]
            self.drop_step = torch.zeros(1, dtype=torch.int32, device=dev)       # device-side dropout step counter
            # the three heads' loss coefficients, read by the heads launch on every step (m2m_heads_ce_w / _bce_w): a captured
            # graph follows set_fusion_loss_weight / set_loss_weights without being captured again
            self.loss_weights = torch.tensor(self._head_weight_list(), dtype=torch.float32, device=dev)
            self._loss_weight_group = {"fused_heads": False}      # (shared by the siblings, like the table itself)
            # the training stage of the engine family (None: stage one; freeze_modalities: FROZEN, train_modalities_only: MODAL)
            # with its device table of coefficients: shared by existing and later siblings
            self._stage_group = {"stage": None, "weights": None, "members": []}
        self.seed = (share.seed if share is not None else seed) & 0xFFFFFFFF
        # scores=True: every training step ends its forward with one launch that adds the batch's counts into `self.scores`
        # (a sibling adds into its parent's table); off: no table, no launch -- the step is exactly the one without the feature
        # rank_scores=True: every training step also appends the softmax of its logits and its labels to `self.rank` (RankBuffer;
        # a sibling appends to its parent's), one launch where the count-table launch goes; off: no buffer, no launch
        if share is not None:
            self.scores, self.rank, self.rank_capacity = share.scores, share.rank, share.rank_capacity
        else:
            self.rank_capacity = int(rank_capacity)
            self.scores: Optional[ScoreTable] = self.new_score_table() if scores else None
            self.rank: Optional[RankBuffer] = self.new_rank_buffer() if rank_scores else None
        if init and share is None:
            self.reset_parameters(seed)
        self.logits = torch.zeros(3, self.B, self.K, device=dev)
        self.losses = torch.zeros(4, device=dev)
        self._graph = None
        self._static = None
        self._adam_plans: Dict[tuple, AdamPackPlan] = {}
        # weight-gradient launch options (_setup_wgrad): towers whose second row group lands in a slot, and the special
        # index ranges of the flat Adam: (lo, n, slot or None, keep)
        self._slot_towers: List[TowerRuntime] = []
        self._ranges_add: list = []
        self._slots_folded = False
        # every tower / embedding with packed operand copies, named once by _build (pack, the one-launch update)
        self._towers: List[TowerRuntime] = []
        self._embeds: List[EmbedRuntime] = []
        self._fused_heads = False                       # the heads ride in the fusion tower's backward launch (_TwoTowerEngine)
        self._eval_only = False                         # sibling(..., trains=False)
        self._probing = False                           # inside probe(): the step head leaves the Adam count alone
        self._tail_engines: Dict[int, "_FlatEngine"] = {}     # training siblings of ragged last batches (data.run_epoch)
        # side streams for the paths whose towers cannot share a launch (wide towers, mixed shapes, the MIMIC static MLP): the
        # second modality runs beside the first.  The AV-MNIST step needs none of them: nine launches on the main stream.
        self.s_b = torch.cuda.Stream(device=dev)
        self.s_fus = torch.cuda.Stream(device=dev)
        self.s_emb = torch.cuda.Stream(device=dev)
        self.concurrent = config.switch_on("M2M_CONCURRENT")      # 0: every launch on the main stream (A/B)
        # the loss coefficients the heads launch of the current pass reads: loss_weights, or in training stage two's (0, 0, 1) /
        # the modalities-only stage's (1, 1)
        self._step_weights = self.loss_weights
        self._trainable: List[Tuple[int, int]] = []      # stage two: the flat ranges Adam still updates (trainable_flat_ranges)
        self._build()
        if self._fused_heads:
            self._loss_weight_group["fused_heads"] = True
        self._stage_group["members"].append(weakref.ref(self))
        if self._staged:
            self._enter_stage()                      # a sibling built after freeze_modalities() / train_modalities_only()
        self.pack()

    # ---- helpers for subclasses ----------------------------------------------------------------------------
    def _make_tower(self, prefix: str, c: dict, N: int, site: int) -> TowerRuntime:
        rt = TowerRuntime(c["hidden_dim"], N, c["token_dim"], c["channel_dim"], c["num_mixers"], True, self.p_drop,
                          self.prec, site)
        nb = c["num_mixers"]
        blocks = [{f: self.params[f"{prefix}mixer_blocks.{i}.{BLOCK_KEYS[f]}"] for f in BLOCK_FIELDS} for i in range(nb)]
        rt.bind_params(blocks, (self.params[prefix + "layer_norm.weight"], self.params[prefix + "layer_norm.bias"]))
        rt.bind_grad_tensors([{f: self.grads[f"{prefix}mixer_blocks.{i}.{BLOCK_KEYS[f]}"] for f in BLOCK_FIELDS}
                              for i in range(nb)],
                             (self.grads[prefix + "layer_norm.weight"], self.grads[prefix + "layer_norm.bias"]))
        rt.ensure_buffers(self.B)
        rt.ensure_workspace(self.B)
        return rt

    def _setup_wgrad(self, launches: Sequence[Sequence[TowerRuntime]]):
        """Options of the channel-mixing weight-gradient launch for a step that runs ONE backward per optimizer step:
          * overwrite: a tower whose gradient elements have a single owner writes them with "=" (no read of the old values)
            and the flat Adam leaves those ranges uncleared (-66 MB per step on M2-Mixer-B);
          * slot: in a grouped launch a tower that needs two row groups (the fusion tower: twice the rows of its neighbours)
            stores the second group's sums into a slot that the flat Adam adds -- plain stores instead of float atomics.
        M2M_WGRAD_OVERWRITE=0 / M2M_WGRAD_SLOT=0 switch them off (A/B)."""
        self._slot_towers, self._ranges_add = [], []
        if not config.switch_on("M2M_WGRAD_OVERWRITE"):
            return
        # `launches`: the towers of each weight-gradient launch of the step (a launch of several towers is the grouped form)
        cand = []                                    # (tower, takes a slot)
        for towers in launches:
            bits = 0
            if len(towers) > 1 and config.switch_on("M2M_WGRAD_SLOT"):
                have = [t.alloc_wslot(self.flat_g) for t in towers]
                bits = wgrad_slot_groups(towers, self.B) if all(have) else 0
            cand += [(t, bool(bits >> i & 1)) for i, t in enumerate(towers)]
        table = []                                   # all-or-nothing per tower (the kernel's range table holds MAX_GRAD_RANGES)
        cand.sort(key=lambda c: not c[1])            # slot towers first: their ranges are mandatory
        for t, slot in cand:
            if not slot:
                t.clear_wslot()
            rng = t.channel_grad_ranges(self.flat_g)
            fits = rng is not None and len(table) + len(rng) <= L.MAX_GRAD_RANGES
            if slot and not fits:
                raise RuntimeError("more slot ranges than m2m_adam_step_ranges takes")
            if not fits or (t.wgrad_groups(self.B) != 1 and not slot):
                continue
            t.set_wgrad_overwrite(True)
            views = t.wslot_views() if slot else [None] * len(rng)
            if slot:
                self._slot_towers.append(t)
            table += [(lo, n, v, 1) for (lo, n), v in zip(rng, views)]
        self._ranges_add = sorted(table, key=lambda r: r[0])

    @property
    def _ranges_keep(self) -> list:
        """_ranges_add once the slots are folded into flat_g: all that is left is which ranges Adam leaves uncleared."""
        return [(lo, n, None, k) for lo, n, _, k in self._ranges_add]

    def _head(self, name: str, pooled, d_pooled, weight: float, with_grad: bool) -> dict:
        key = "classifier_fusion.classifer." if name == "fusion" else f"classifier_{name}."
        P, Gr = self.params, self.grads
        return dict(pooled=pooled, w=P[key + "weight"], b=P[key + "bias"], g_w=Gr[key + "weight"], g_b=Gr[key + "bias"],
                    d_pooled=d_pooled if with_grad else None, weight=weight)

    def _streams(self, concurrent: Optional[bool] = None):
        main = torch.cuda.current_stream()
        conc = self.concurrent if concurrent is None else (concurrent and self.concurrent)
        return main, (self.s_b if conc else main), (self.s_fus if conc else main)

    # ---- parameters --------------------------------------------------------------------------------------
    def reset_parameters(self, seed: int = 42):
        """torch default init (Linear / Conv2d: kaiming-uniform(a=sqrt(5)) == U(+-1/sqrt(fan_in)); LayerNorm 1/0),
        drawn on the CPU generator under `seed` in creation order (run.py:32 seeds 42)."""
        gen = torch.Generator().manual_seed(seed)
        for k, shp in self.shapes.items():
            if _is_layer_norm(k):
                v = torch.ones(shp) if k.endswith("weight") else torch.zeros(shp)
            else:
                wshape = self.shapes[k[:-4] + "weight"] if k.endswith("bias") else shp
                fan_in = int(torch.Size(wshape[1:]).numel())
                bound = 1.0 / fan_in ** 0.5
                v = (torch.rand(shp, generator=gen) * 2 - 1) * bound
            self.params[k].copy_(v)

    #: non-parameter entries a reference state_dict may carry for this model (buffers of its loss modules)
    EXTRA_STATE_KEYS: Tuple[str, ...] = ()

    def _consume_extra_state(self, key: str, value: torch.Tensor):
        raise KeyError(key)

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        missing = [k for k in self.shapes if k not in sd]
        extra = [k for k in sd if k not in self.shapes and k not in self.EXTRA_STATE_KEYS]
        if missing or extra:
            raise KeyError(f"state dict mismatch: missing {missing[:4]}, unexpected {extra[:4]}")
        for k in self.shapes:
            self.params[k].copy_(sd[k].to(self.device, torch.float32).reshape(self.shapes[k]))
        for k in self.EXTRA_STATE_KEYS:
            if k in sd:
                self._consume_extra_state(k, sd[k])
        self.pack()

    def _extra_state(self) -> "OrderedDict[str, torch.Tensor]":
        return OrderedDict()

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """The reference module's state_dict: parameters under its key names, in its order, then the loss-module buffers."""
        out = OrderedDict((k, v.detach().clone()) for k, v in self.params.items())
        out.update(self._extra_state())
        return out

    def optimizer_state_dict(self) -> dict:
        """torch.optim.Adam.state_dict() layout (what Lightning stores under `optimizer_states[0]`): per parameter index
        `step`, `exp_avg`, `exp_avg_sq`; one param group with this engine's hyper-parameters."""
        step = float(self.adam_state[0])
        state = {i: {"step": torch.tensor(step), "exp_avg": self.exp_avg[k].detach().cpu().clone(),
                     "exp_avg_sq": self.exp_avg_sq[k].detach().cpu().clone()} for i, k in enumerate(self.shapes)}
        group = {"lr": float(self.adam_state[1]), "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.weight_decay,
                 "amsgrad": False, "maximize": False, "params": list(range(len(self.shapes)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, osd: dict):
        """torch.optim.Adam.state_dict() as the reference writes it (Lightning: `optimizer_states[0]`).  Parameters without an
        entry -- a state dict saved before the first step, or with modalities frozen (`requires_grad=False` parameters never get
        Adam state: models/avmnist.py:314-324) -- start from zero moments; the ONE step count the fused Adam keeps is taken
        from the entries that are present (they must agree)."""
        keys = list(self.shapes)
        state = osd.get("state", {})
        bad = [i for i in state if not isinstance(i, int) or i < 0 or i >= len(keys)]
        if bad:
            raise KeyError(f"optimizer state: entries {bad[:4]} do not index this model's {len(keys)} parameters")
        steps = {float(st["step"]) for st in state.values() if "step" in st}
        if len(steps) > 1:
            raise RuntimeError("optimizer state: the fused Adam keeps ONE step count for all parameters")
        for i, k in enumerate(keys):
            st = state.get(i)
            if st is None or "exp_avg" not in st:
                self.exp_avg[k].zero_()
                self.exp_avg_sq[k].zero_()
                continue
            self.exp_avg[k].copy_(st["exp_avg"].to(self.device, torch.float32).reshape(self.shapes[k]))
            self.exp_avg_sq[k].copy_(st["exp_avg_sq"].to(self.device, torch.float32).reshape(self.shapes[k]))
        self.adam_state[0] = steps.pop() if steps else 0.0
        if osd.get("param_groups"):
            self.set_lr(float(osd["param_groups"][0]["lr"]))

    def set_lr(self, lr: float):
        self.adam_state[1] = lr

    # ---- loss weights -----------------------------------------------------------------------------------------
    HEAD_NAMES: Tuple[str, str, str] = ("a", "b", "fusion")

    def _head_weight_list(self) -> List[float]:
        return [float(self.head_weights[n]) for n in self.HEAD_NAMES]

    def set_loss_weights(self, *weights: float):
        """The heads' coefficients in the total loss (HEAD_NAMES order: modality a, modality b, fusion), written in place into the
        device table every heads launch reads -- this engine, its siblings and any graph captured from them use the new values
        from their next step on.  Enqueued on the current stream (behind the steps already enqueued there)."""
        if len(weights) != len(self.HEAD_NAMES):
            raise ValueError(f"set_loss_weights: {len(self.HEAD_NAMES)} coefficients ({', '.join(self.HEAD_NAMES)})")
        if self._loss_weight_group["fused_heads"]:
            # m2m_tower_backward_heads (M2M_FUSED_HEADS=1) takes the coefficients by value: a captured graph would keep the old ones
            raise RuntimeError("set_loss_weights: the fused heads + fusion backward launch (M2M_FUSED_HEADS=1) takes the loss "
                               "weights by value; a changing loss weight needs that switch off")
        vals = [float(w) for w in weights]
        self.loss_weights.copy_(torch.tensor(vals, dtype=torch.float32))
        self.head_weights = dict(zip(self.HEAD_NAMES, vals))

    def set_fusion_loss_weight(self, w: float):
        """The reference's `fusion_loss_weight` (the schedule of models/avmnist.py:332-339, models/mimic.py:144-150): the three
        coefficients by this model's formula, written in place (set_loss_weights)."""
        raise NotImplementedError(f"{type(self).__name__}: its loss has no fusion_loss_weight")

    def _sibling_kwargs(self) -> dict:
        return {"fusion_loss_weight": self.fusion_loss_weight} if hasattr(self, "fusion_loss_weight") else {}

    def _spawn(self, batch_size: int, share):
        """Another engine of this one's class, cfg, precision and hyper-parameters: over this engine's buffers (share=self:
        sibling) or over fresh ones (share=None: clone)."""
        prec = {v: k for k, v in L.PREC_BY_NAME.items() if k in ("bf16", "fp32")}[self.prec]
        new = type(self)(self.cfg, batch_size, device=self.device, precision=prec, lr=float(self.adam_state[1]),
                         betas=self.betas, eps=self.eps, weight_decay=self.weight_decay, seed=self.seed, init=False,
                         share=share, **self._sibling_kwargs())
        self._copy_loaded_state(new)
        return new

    def _copy_loaded_state(self, new):
        """Give `new` the non-parameter state a load_state_dict left on this engine (MM-IMDb: the criterion buffer)."""

    def sibling(self, batch_size: int, trains: bool = True):
        """An engine for another batch size over THIS engine's parameters, gradients, Adam state and step counters
        (constructor argument share=): the step that takes an epoch's ragged last batch, or a validation engine.
        trains=False: the sibling only evaluates (it never writes a gradient): nothing of this engine changes.

        Both engines work on ONE gradient buffer.  A range one of them leaves uncleared ("keep": its own next backward
        overwrites it) must be overwritten by the other one's backward too, or that one would accumulate onto stale values --
        so the keep flags of both are narrowed to the ranges BOTH overwrite.  A captured graph holds its range table BY VALUE
        (m2m_adam_step_ranges copies it into the kernel arguments), so narrowing after capture() would leave the graph with
        the old flags: that is refused -- build training siblings before capture(), or capture again."""
        sib = self._spawn(batch_size, share=self)
        if not trains:
            sib._eval_only = True
            return sib
        mine, theirs = {r[0] for r in self._ranges_add}, {r[0] for r in sib._ranges_add}
        narrowed = [lo for lo, n, v, k in self._ranges_add if k and lo not in theirs]
        if narrowed and self._graph is not None:
            raise RuntimeError(f"sibling({batch_size}): this engine's captured graph keeps {len(narrowed)} gradient range(s) uncleared "
                               "that the sibling's backward would not overwrite; build training siblings before capture() "
                               "(or capture again afterwards)")
        for eng, other in ((self, theirs), (sib, mine)):
            eng._ranges_add = [(lo, n, v, int(k and lo in other)) for lo, n, v, k in eng._ranges_add]
        return sib

    # ---- training stages (Stage): stage two with its frozen modality towers (models/avmnist.py:292-293, :314-324) and its mirror
    # ---- image, the modalities-only stage: the unimodal models of Gradient-Blending (modules/gradblend.py:92-98) ---------------
    def _frozen_prefixes(self) -> Tuple[str, ...]:
        return frozen_key_prefixes(self.HEAD_NAMES[:2])

    @property
    def _frozen(self) -> bool:
        return self._stage_group["stage"] is FROZEN

    @property
    def _modal(self) -> bool:
        return self._stage_group["stage"] is MODAL

    @property
    def _staged(self) -> bool:
        """In stage two or in the modalities-only stage: Adam runs per trainable range, a gradient exchange is refused."""
        return self._stage_group["stage"] is not None

    def freeze_modalities(self):
        """Enter stage two of the reference's two-stage training, for this engine, its siblings and siblings built later (there
        is no way back: the reference has none).  From the next training step on
          * the training loss is loss_fusion with coefficient 1: training passes read a second device table (0, 0, 1), evaluation
            keeps `loss_weights` and its schedule; losses[0..2] are still the three heads' losses, losses[3] == losses[2];
          * the parameters and both Adam moments of the frozen keys (the two modality towers with their embeddings and heads) are
            never written again; the shared step count keeps advancing, so the trainable ranges' bias correction continues;
          * the step launches no backward of a frozen tower, no embedding gradient, the weight gradients of the fusion tower
            alone, Adam over the trainable ranges only and the re-pack of the fusion tower only.
        Captured graphs are dropped as release_capture() drops them: capture again.  Refused with M2M_FUSED_HEADS=1 (that launch
        takes the loss weights by value); a gradient exchange is refused in stage two (single GPU)."""
        self._enter(FROZEN, "freeze_modalities", [
            (self._loss_weight_group["fused_heads"],
             "freeze_modalities: the fused heads + fusion backward launch (M2M_FUSED_HEADS=1) takes the loss "
             "weights by value; stage two needs that switch off")])

    def train_modalities_only(self):
        """Enter the mirror image of stage two, for this engine, its siblings and siblings built later (one-way, like the freeze):
        the two unimodal models of Gradient-Blending (modules/gradblend.py:92-98: each modality tower with its own head) trained
        at once -- they share no parameter and Adam is element-wise, so this is the reference's two separate trainings.  From the
        next training step on
          * the training loss is loss_a + loss_b, coefficients (1, 1): the heads launch takes the two modality heads only;
            losses[0..1] are their losses, losses[2] == 0, losses[3] == losses[0] + losses[1].  logits[2] / preds[2] keep what
            the last full forward left there;
          * the step runs no fusion function and no fusion tower, forward or backward: the modality towers' backward starts from
            their heads' d_pooled alone (d_out NULL);
          * the fusion function's and the fusion tower's parameters, classifier_fusion and both of their Adam moments are never
            written again; Adam runs over the complement of stage two's ranges, the re-pack over the modality towers and their
            embeddings.
        evaluate() stays the full model under `loss_weights`.  Captured graphs are dropped: capture again.  Refused with
        M2M_FUSED_HEADS=1, on engines built with scores / rank_scores (the fusion head's predictions are not produced), after
        freeze_modalities(); a gradient exchange is refused in this stage (single GPU)."""
        self._enter(MODAL, "train_modalities_only", [
            (self._loss_weight_group["fused_heads"],
             "train_modalities_only: the fused heads + fusion backward launch (M2M_FUSED_HEADS=1) belongs to the "
             "fusion tower's backward, which this stage does not run; it needs that switch off"),
            (self.scores is not None or self.rank is not None,
             "train_modalities_only: an engine built with scores=True / rank_scores=True counts the fusion head's "
             "predictions on every training step; this stage does not produce them")])

    def _enter(self, stage: Stage, method: str, refusals):
        """Take the engine family into `stage` (both stages are one-way).  refusals: [(condition, message)], the entering
        method's own, checked once the family is known to be in stage one."""
        grp = self._stage_group
        if grp["stage"] is stage:
            return
        if grp["stage"] is not None:
            raise RuntimeError(f"{method}: this engine family is in {grp['stage'].title}, which has no way back")
        for refused, message in refusals:
            if refused:
                raise RuntimeError(message)
        grp["weights"] = torch.tensor(stage.weights, dtype=torch.float32, device=self.device)
        grp["stage"] = stage
        members = [m for m in (r() for r in grp["members"]) if m is not None]
        grp["members"] = [weakref.ref(m) for m in members]
        # Stage one left the ranges its overwriting weight-gradient launch owned uncleared ("keep").  A range the new stage's
        # weight-gradient call accumulates into instead (another row plan: no slot) must start from zero: clear every trainable
        # range once, here, outside any graph.
        for lo, hi in trainable_flat_ranges(self.shapes, self._frozen_prefixes(), invert=stage.invert):
            self.flat_g[lo:hi].zero_()
        for m in members:
            m._enter_stage()
        # one gradient buffer: a range one engine leaves uncleared must be overwritten by every other training engine (sibling())
        trains = [m for m in members if not m._eval_only]
        for m in trains:
            others = [{r[0] for r in o._ranges_add} for o in trains if o is not m]
            m._ranges_add = [(lo, n, v, int(k and all(lo in o for o in others))) for lo, n, v, k in m._ranges_add]

    def _enter_stage(self):
        """One member's side of _enter; also what a sibling built after it does at construction."""
        self.release_capture()
        self._trainable = trainable_flat_ranges(self.shapes, self._frozen_prefixes(), invert=self._stage_group["stage"].invert)
        self._slots_folded = False
        self._stage_options()

    def _stage_options(self):
        """Launch options of the stage's step, re-derived for its own launches (subclasses)."""

    def _pass_weights(self, training: bool) -> torch.Tensor:
        """The device table of loss coefficients the heads launch of this pass reads."""
        return self._stage_group["weights"] if (training and self._staged) else self.loss_weights

    def _stage_total(self, training: bool):
        """A stage's training pass: the total loss as an exact function of the heads' losses.
        Stage two: losses[3] = losses[2].  The heads kernel adds each workgroup's term to its head's loss and, times the
        coefficient, to the total with two atomics; with coefficients (0, 0, 1) the total is the same terms, but three or more
        workgroups may arrive in another order at the second address -- one 4-byte copy makes the equality exact.
        Modalities-only stage: the two-head launch left its total in losses[2] (slot nheads).  losses[3] is written as the one
        fp32 sum of the two heads' losses (the atomics' arrival order does not show), losses[2] is the fusion head's loss, which
        this stage does not compute: zero."""
        if not training:
            return
        if self._frozen:
            self.losses[3:4].copy_(self.losses[2:3])
        elif self._modal:
            torch.add(self.losses[0:1], self.losses[1:2], out=self.losses[3:4])
            self.losses[2:3].copy_(self._stage_group["weights"][2:3])

    def _update_trainable_ranges(self, grad_scale: float, grad_bf16):
        """A stage's update: Adam over each trainable range, then the re-pack of what the stage trains."""
        if grad_bf16 is not None:
            raise RuntimeError("stage two (freeze_modalities) / the modalities-only stage is single GPU: no exchanged bf16 gradient")
        if not self._slots_folded:                   # (stage two's single-tower call has no slot; a grouped modality pair may)
            for t in self._slot_towers:
                t.wgrad_fold()
        self._slots_folded = False
        for lo, hi in self._trainable:               # the existing range form, one launch per trainable range
            self._adam_chunk(lo, hi, grad_scale)
        for m in self._stage_packs():                # the modules whose packed operand copies this stage's update rebuilds
            m.pack(force=True)

    def _refuse_exchange_in_a_stage(self, grad_sync):
        if grad_sync is not None and self._staged:
            raise RuntimeError(f"{self._stage_group['stage'].title} is single GPU: a grad_sync is refused")

    # ---- optimizer -------------------------------------------------------------------------------------------
    def _check_grad_bf16(self, grad_bf16: Optional[torch.Tensor]):
        if grad_bf16 is not None and (grad_bf16.dtype != torch.bfloat16 or grad_bf16.numel() != self.n_params or not grad_bf16.is_cuda):
            raise RuntimeError("grad_bf16 must be a bf16 device copy of the whole flat gradient")

    def _adam(self, lo: int, hi: int, scale: float, grad_bf16: Optional[torch.Tensor] = None, ranges=None):
        """Adam over flat elements [lo, hi); clears the gradients it consumes.  grad_bf16: a bf16 copy of the whole flat
        gradient (the compressed all-reduce result) to take the values from instead of flat_g.  ranges: the special gradient
        ranges inside [lo, hi), indexed from lo."""
        self._check_grad_bf16(grad_bf16)
        n = hi - lo
        p, g, m, v = (t.data_ptr() + lo * 4 for t in (self.flat_p, self.flat_g, self.flat_m, self.flat_v))
        g16 = 0 if grad_bf16 is None else grad_bf16.data_ptr() + lo * 2
        # (negative scale: the kernel clears the gradients; the step count was advanced by the step's prologue)
        tail = (self.adam_state.data_ptr(), self.betas[0], self.betas[1], self.eps, self.weight_decay, -abs(scale), 0)
        if ranges:
            L.check(L.lib().m2m_adam_step_ranges(p, g, g16, m, v, n, *tail, _grad_ranges(ranges), len(ranges), L.stream_ptr()),
                    "adam_step_ranges")
        elif grad_bf16 is None:
            L.check(L.lib().m2m_adam_step(p, g, m, v, n, *tail, L.stream_ptr()), "adam_step")
        else:
            L.check(L.lib().m2m_adam_step_bf16(p, g, g16, m, v, n, *tail, L.stream_ptr()), "adam_step_bf16")

    def _prologue(self):
        """Head of a training step: Adam step count += 1, dropout counter += 1, losses = 0 -- one tiny launch."""
        L.check(L.lib().m2m_step_prologue(L.ptr(self._head_adam()), self.drop_step.data_ptr(), self.losses.data_ptr(), 4,
                                          L.stream_ptr()), "step_prologue")

    def _head_adam(self) -> Optional[torch.Tensor]:
        """The Adam state the head of this pass advances: none under probe() (the prologue forms take NULL)."""
        return None if self._probing else self.adam_state

    @torch.no_grad()
    def probe(self, *batch):
        """The training-mode forward alone (GradBlend's get_loss, modules/gradblend.py:43-60: modules in train mode, nothing
        updated): dropout on, the dropout counter advanced as a training step advances it, `losses` / `logits` / `preds` filled
        under the stage's training coefficients -- and no gradient, parameter, moment or Adam count written.  Returns `losses`."""
        self._probing = True
        try:
            self._forward(*batch, training=True, with_grad=False, prologue=True)
        finally:
            self._probing = False
        return self.losses

    def clone(self, batch_size: Optional[int] = None):
        """An INDEPENDENT engine of the same cfg, precision and hyper-parameters (default: the same batch size) that starts from a
        copy of this one's parameters and loss weights, with zero Adam moments, step count and dropout counter, in stage one, and
        without score tables or ranking buffers.  Nothing is shared with this engine (unlike sibling())."""
        new = self._spawn(self.B if batch_size is None else int(batch_size), share=None)
        new.flat_p.copy_(self.flat_p)
        new.loss_weights.copy_(self.loss_weights)
        new.head_weights = dict(self.head_weights)
        new.pack()
        return new

    def forward_backward(self, *batch):
        """forward (dropout on) -> multi-head loss -> backward; gradients are ADDED into flat_g, which must be
        zero on entry: it is cleared at construction and again by every optimizer_step (the Adam kernel clears
        each element it consumes), so no separate fill pass is needed.  (Channel-mixing weight gradients of the
        overwriting towers -- _setup_wgrad -- are written, not added: those ranges need no clearing.)  On return flat_g
        holds the complete gradient: a row group the weight-gradient launch left in a slot is folded in here.
        After freeze_modalities() flat_g is UNSPECIFIED inside the frozen keys' ranges (no backward of a frozen tower runs, what
        stage one left there is neither cleared nor consumed); inside the trainable ranges it is the gradient of loss_fusion."""
        self._step(batch, fused_update=False)
        for t in self._slot_towers:
            t.wgrad_fold()
        self._slots_folded = True                       # (consumed by the optimizer_step that follows; fused_step resets it)

    def fused_step(self, *batch):
        """forward + backward + Adam + re-pack in one go (no gradient exchange: single-GPU training)."""
        self._step(batch, fused_update=True)
        return self.losses

    def _step(self, batch, fused_update: bool):
        self._check_trains()
        # (a forward_backward() without its optimizer_step() -- gradient inspection, a skipped step -- must not make THIS step's
        # Adam skip the slot of the two-group tower: the slot is folded by forward_backward only)
        self._slots_folded = False
        self._forward(*batch, training=True, with_grad=True, prologue=True)
        if not self._fused_heads:                    # the training forward left `preds` and `logits` written
            self._score_add(batch[-1])
        self._backward(*batch[:-1], fused_update=fused_update)
        if self._fused_heads:                        # the heads rode in the fusion tower's backward launch
            self._score_add(batch[-1])

    # ---- scores ----------------------------------------------------------------------------------------------
    def new_score_table(self) -> ScoreTable:
        """An empty count table for this model's heads (one per split: evaluate(..., scores=table) adds into the one given)."""
        return ScoreTable(self.SCORES_TASK, self.HEAD_NAMES, self.K, self.device)

    def score_table(self, split: str) -> ScoreTable:
        """The table of `split`, kept on the engine: "train" is the training table (`self.scores`, which needs scores=True),
        any other name gets a table of its own on first use."""
        return self._of_split(split, self.scores, "_split_scores", self.new_score_table,
                              "score_table('train'): this engine was built with scores=False")

    def _of_split(self, split: str, training, attr: str, new, refusal: str):
        """score_table / rank_buffer: `training` for "train" (refused when the engine was built without it), else the split's own
        accumulator, made by new() on first use and kept in the dict `attr` (which exists from the first such use on)."""
        if split == "train":
            if training is None:
                raise RuntimeError(refusal)
            return training
        kept = self.__dict__.setdefault(attr, {})
        if split not in kept:
            kept[split] = new()
        return kept[split]

    def _score_add(self, truth):
        """Behind the launch that writes `preds` and `logits`: the count-table launch and / or the ranking append."""
        if self.scores is not None:
            self.scores.add(self.preds, truth)
        if self.rank is not None:
            self.rank.add(self.logits, truth)

    @torch.no_grad()
    def evaluate(self, *batch, scores: Optional[ScoreTable] = None, rank: Optional[RankBuffer] = None,
                 record: Optional[PredictionRecord] = None):
        """validation/test step on `batch` (the inputs, then the labels): dropout off (the reference's shared_step under
        model.eval()).  scores: a table (new_score_table / score_table(split)) this batch's counts are added into.  rank: a
        ranking buffer (new_rank_buffer / rank_buffer(split)) this batch's softmax rows are appended to.  record: a prediction
        record (new_prediction_record / prediction_record(split)) this batch's logits, predictions and labels are appended to,
        behind the launch that writes them."""
        self._forward(*batch, False, False)
        if scores is not None:
            scores.add(self.preds, batch[-1])
        if rank is not None:
            rank.add(self.logits, batch[-1])
        if record is not None:
            record.add(self, batch[-1])
        return self._eval_outputs()                  # views of `logits` / `losses` / `preds` under the reference's names

    # ---- prediction records ----------------------------------------------------------------------------------
    def new_prediction_record(self, capacity: int) -> PredictionRecord:
        """An empty prediction record of `capacity` rows for this model's heads (one per split: evaluate(..., record=record)
        appends to the one given)."""
        return PredictionRecord(self.SCORES_TASK, self.HEAD_NAMES, self.K, capacity, self.device,
                                uncertainty=getattr(self, "uncertainty", None) is not None)

    def prediction_record(self, split: str, capacity: Optional[int] = None) -> PredictionRecord:
        """The record of `split`, kept on the engine as its tables and ranking buffers are: made with `capacity` rows on first use
        (which must give one); a later call may leave the capacity out, and one that names another capacity is refused (captured
        graphs keep the first one's pointers).  Training steps keep no record: "train" is refused (evaluate the training split
        under another name)."""
        def new():
            if capacity is None:
                raise RuntimeError(f"prediction_record({split!r}): the first use must give the capacity in rows")
            return self.new_prediction_record(capacity)

        rec = self._of_split(split, None, "_split_records", new,
                             "prediction_record('train'): training steps keep no record (evaluate the split under another name)")
        if capacity is not None and int(capacity) != rec.capacity:
            raise RuntimeError(f"prediction_record({split!r}, {capacity}): the record of this split holds {rec.capacity} rows")
        return rec

    # ---- ranking buffers -------------------------------------------------------------------------------------
    def new_rank_buffer(self) -> RankBuffer:
        """An empty ranking buffer for this model's heads (one per split: evaluate(..., rank=buffer) appends to the one given)."""
        return RankBuffer(self.SCORES_TASK, self.HEAD_NAMES, self.K, self.rank_capacity, self.device)

    def rank_buffer(self, split: str) -> RankBuffer:
        """The buffer of `split`, kept on the engine: "train" is the training buffer (`self.rank`, which needs
        rank_scores=True), any other name gets a buffer of its own on first use."""
        return self._of_split(split, self.rank, "_split_ranks", self.new_rank_buffer,
                              "rank_buffer('train'): this engine was built with rank_scores=False")

    def _check_trains(self):
        if self._eval_only:
            raise RuntimeError("this engine was built with sibling(..., trains=False): it only evaluates")

    def pack(self):
        """Rebuild the packed MFMA-operand copies from the fp32 masters: every tower and embedding in ONE launch on the main
        stream (~100 MB of traffic at the HBM roofline on M2-Mixer-B).  Replaced five launches forked over the side streams,
        whose fork and join edges cost more inside the replayed graph than the concurrency returned."""
        if can_pack_all(self._towers, self._embeds):
            pack_all(self._towers, self._embeds)
            return
        for m in self._towers + self._embeds:
            m.pack(force=True)

    def _adam_pack_modules(self):
        """(towers, embeds) whose parameters all live in the flat buffers and whose operand copies one m2m_adam_pack_all
        launch can rebuild -- None: the model needs the two-launch form (Adam, then pack())."""
        return (self._towers, self._embeds) if can_pack_all(self._towers, self._embeds) else None

    def _update(self, grad_scale: float = 1.0, grad_bf16: Optional[torch.Tensor] = None):
        """Adam over every parameter + operand re-pack.  One launch (m2m_adam_pack_all) where the model allows it: the
        re-pack then takes the updated weights from the workgroup that computed them instead of re-reading the masters."""
        if self._staged:
            self._update_trainable_ranges(grad_scale, grad_bf16)
            return
        mods = self._adam_pack_modules() if self._fused_update else None
        # the slot of a two-group tower: added inside Adam (fused step) unless forward_backward has folded it in already
        ranges = self._ranges_keep if (self._slots_folded or grad_bf16 is not None) else self._ranges_add
        self._slots_folded = False
        if mods is None:
            self._adam(0, self.n_params, grad_scale, grad_bf16, ranges)
            self.pack()
            return
        key = (abs(float(grad_scale)), 0 if grad_bf16 is None else grad_bf16.data_ptr(), tuple((lo, n, 0 if v is None else v.data_ptr(), k) for lo, n, v, k in ranges))
        plan = self._adam_plans.get(key)
        if plan is None:
            self._check_grad_bf16(grad_bf16)
            plan = AdamPackPlan(mods[0], mods[1], self.flat_p, self.flat_g, grad_bf16, self.flat_m, self.flat_v, self.adam_state,
                                self.betas, self.eps, self.weight_decay, grad_scale, ranges)
            self._adam_plans[key] = plan
        plan.run()

    def optimizer_step(self, grad_scale: float = 1.0, grad_bf16: Optional[torch.Tensor] = None):
        self._update(grad_scale, grad_bf16)                                    # (the step counters were advanced by _prologue)

    def train_step(self, *batch, grad_sync=None):
        """One optimisation step.  grad_sync: optional callable(flat_grad) doing the data-parallel
        all-reduce (parallel.GradSync); it returns the factor the summed gradient must be scaled by."""
        self._run_step(grad_sync, *self._phases(batch, grad_sync))
        return self.losses

    # ---- a step in its exchange mode -------------------------------------------------------------------------------------
    def _run_step(self, grad_sync, first, update) -> float:
        """One step in grad_sync's exchange mode (_exchange_mode); returns the gradient scale.  first(): everything up to the
        exchange (the whole step when there is none); update(k, scale): the update behind the exchange -- of chunk k of
        _update_chunks() when pipelined (chunk k + 1 .. are still on the communication stream), else k = 0: everything.
        Eager steps pass _phases(), a captured step its graphs' replays."""
        self._refuse_exchange_in_a_stage(grad_sync)
        mode = _exchange_mode(grad_sync)
        first()
        if mode == "none":
            return 1.0
        if mode == "single":
            scale = grad_sync(self.flat_g)
            update(0, scale)
            return scale
        chunks = self._update_chunks()
        scale = grad_sync.start(self.flat_g, [(lo, hi) for lo, hi, _ in chunks])
        for k in range(len(chunks)):
            grad_sync.wait(k)
            update(k, scale)
        self._slots_folded = False
        return scale

    def _phases(self, batch, grad_sync):
        """(first, update) of _run_step for an eager step on `batch`."""
        mode = _exchange_mode(grad_sync)
        if mode == "none":
            return (lambda: self.fused_step(*batch)), None
        if mode == "single":      # (reduced_bf16 is read behind the exchange: the buffer exists from the first one on)
            return (lambda: self.forward_backward(*batch)), (lambda k, scale: self.optimizer_step(scale, getattr(grad_sync, "reduced_bf16", None)))
        return (lambda: self.forward_backward(*batch)), self._update_one_chunk

    # ---- exchange pipelined with the optimizer (parallel.PipelinedGradSync) ------------------------------------------------
    def _update_chunks(self):
        """[(lo, hi, [modules to re-pack]), ...]: a partition of the flat buffers into pieces whose Adam update and operand
        re-pack need nothing outside the piece -- the parameter segments (one per tower; the last also holds the heads).
        Engines without per-segment packers return the whole buffer as one chunk."""
        return [(0, self.n_params, None)]

    def _adam_chunk(self, lo: int, hi: int, scale: float):
        """Adam over flat elements [lo, hi) with the engine's kept ranges cut to the chunk (the slots were folded in by
        forward_backward: `keep` is all that is left of the range table)."""
        ranges = []
        for rlo, rn, _, keep in self._ranges_keep:
            a, b = max(rlo, lo), min(rlo + rn, hi)
            if a < b:
                ranges.append((a - lo, b - a, None, keep))
        self._adam(lo, hi, scale, None, ranges)

    def _update_one_chunk(self, k: int, scale: float):
        lo, hi, mods = self._update_chunks()[k]
        self._adam_chunk(lo, hi, scale)
        if mods is None:
            self.pack()
        else:
            for m in mods:
                m.pack(force=True)

    # ---- hipGraph capture -----------------------------------------------------------------------------------
    def release_capture(self):
        """Forget the captured graph(s) (drop the replay callable too): a training sibling may then narrow the kept gradient
        ranges (sibling()); capture() again before replaying."""
        self._graph = None
        self._static = None

    def capture(self, *batch, grad_sync=None, steps: int = 1):
        """Capture train_step on static input buffers; returns a callable replay(*batch).
        With a grad_sync the step is captured as two graphs with the all-reduce between them.
        steps > 1 (single-GPU path only) captures that many consecutive training steps in ONE graph -- every replayed
        graph costs ~17 us of launch gap on this platform, which is 2 % of a step -- with one static input slot per step:
        replay(*batch_0, *batch_1, ...) or replay() to reuse what the slots hold; losses / logits / preds of step i land
        in self.losses_steps[i] etc. (replay() returns, and replay.losses is, that (steps, 4) buffer; the engine's own
        losses / logits / preds are left to the single-step paths).
        capture() does not train: the warm-up steps it needs are undone (parameters, Adam moments, step counters)."""
        if steps < 1 or (steps > 1 and grad_sync is not None):
            raise ValueError("steps > 1 is only supported without a gradient exchange")
        self._refuse_exchange_in_a_stage(grad_sync)
        nb = len(batch)
        slots = [tuple(t.clone() for t in batch) for _ in range(steps)]
        if steps > 1 and config.switch_on("M2M_CAPTURE_SHARE_SLOTS"):
            slots = [slots[0]] * steps                  # diagnostic (scripts/spg_probe.sh): every step reads the SAME (cache-resident) batch
        self._static = slots[0] if steps == 1 else slots
        first, update = self._phases(slots[0], grad_sync)
        scale = self._undo_warmup(lambda: self._run_step(grad_sync, first, update))
        with self._per_step_outputs(steps) as (outs, enter):
            if steps > 1:
                self.losses_steps, self.logits_steps, self.preds_steps = outs

                def first():
                    for i in range(steps):
                        enter(i)
                        self.fused_step(*slots[i])

            # forward + backward (no exchange: the whole step, `steps` times) | [the all-reduce lands] Adam + re-pack: one graph, or
            # one small graph per chunk when pipelined (the scale, and a bf16 exchange's buffer, exist since the warm-up)
            nupd = {"none": 0, "single": 1, "pipelined": len(self._update_chunks())}[_exchange_mode(grad_sync)]
            graphs = (self._graph_of(first), *[self._graph_of(lambda k=k: update(k, scale)) for k in range(nupd)])
        out_losses = self.losses if outs is None else outs[0]
        self._slots_folded = False
        self._graph = graphs

        def replay(*new_batch):
            if new_batch and new_batch[0] is not None:
                if len(new_batch) != nb * steps:
                    raise ValueError(f"replay expects {nb * steps} tensors ({steps} step(s) x {nb}), got {len(new_batch)}")
                for i in range(steps):
                    for dst, src in zip(slots[i], new_batch[i * nb:(i + 1) * nb]):
                        dst.copy_(src, non_blocking=True)
            self._run_step(grad_sync, graphs[0].replay, lambda k, scale: graphs[1 + k].replay())
            return out_losses                     # this graph's own buffer: (4,) or, for a multi-step graph, (steps, 4)

        replay.losses = out_losses
        return replay

    def _undo_warmup(self, step, extra_state: Sequence[torch.Tensor] = ()):
        """Run step() twice on a side stream and put back what it changed; returns the second call's value.  The warm-up runs
        REAL training steps (lazy initialisation of the launches -- LDS attributes, allocations -- must happen outside the
        capture); everything they change is restored afterwards, so a capture leaves the model exactly as it found it.
        extra_state: the tensors a caller's step changes beyond the engine's own (a feed's cursor and accumulators)."""
        # (the warm-up steps count and append their batch too: the training table and the ranking cursor go back)
        state = [self.flat_p, self.flat_m, self.flat_v, self.flat_g, self.adam_state, self.drop_step, *extra_state,
                 *PassAccumulators(self.scores, self.rank).state()]
        snap = [t.clone() for t in state]
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                out = step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        for dst, src in zip(state, snap):
            dst.copy_(src)
        self.pack()
        torch.cuda.synchronize()
        return out

    @contextmanager
    def _per_step_outputs(self, steps: int):
        """The output slots of ONE captured graph of `steps` steps.  Yields (outs, enter): outs = (losses, logits, preds), each
        with a leading `steps` axis, or None for a single step; enter(i) points self.losses / logits / preds at slot i for the
        step captured next.  On the way out, capture error or not, the engine's own buffers are back: they stay what they were
        (other captured graphs and evaluate() write those)."""
        home = (self.losses, self.logits, self.preds)
        outs = None
        if steps > 1:
            outs = tuple(torch.zeros(steps, *t.shape, dtype=t.dtype, device=self.device) for t in home)

        def enter(i):
            if outs is not None:
                self.losses, self.logits, self.preds = (t[i] for t in outs)

        try:
            yield outs, enter
        finally:
            self.losses, self.logits, self.preds = home

    @staticmethod
    def _graph_of(fn):
        # thread_local capture mode: a data-parallel process has other threads (the RCCL watchdog) that may touch the HIP
        # runtime while this thread captures; only this thread's calls belong to the graph
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            fn()
        return g

    def capture_feed(self, feed: EpochFeed, steps: int = 1, grad_sync=None):
        """Capture `steps` consecutive training steps that feed themselves from `feed` (EpochFeed); returns a callable replay()
        without arguments.  Each captured step is: m2m_feed_gather into that step's input slots (the cursor advances on the
        device), fused_step on the slots, m2m_epoch_accumulate of its losses and hits into the feed's accumulators -- so an epoch
        is n / (B * steps) replays and one feed.read().  feed.start(order) between replays changes the order in place; the graph
        follows it.  replay.slots[i] are step i's input slots, replay.losses the (4,) / (steps, 4) loss buffer as for capture().
        Like capture() it does not train: the warm-up steps are undone, the feed's cursor and accumulators included.
        Single GPU only: a grad_sync is refused (every rank would need its shard of the order)."""
        if grad_sync is not None:
            raise ValueError("capture_feed is only supported without a gradient exchange (single GPU)")
        self._check_trains()
        replay, graph = self._capture_fed("capture_feed", feed, steps, self.fused_step, [], {})
        self._slots_folded = False
        self._graph = (graph,)
        return replay

    def _capture_fed(self, name: str, feed: EpochFeed, steps: int, step, restore: Sequence[torch.Tensor], attrs: dict):
        """The scaffold capture_feed and capture_feed_eval share: `steps` times gather into the step's slots, step(*slots), accumulate
        -- warmed up outside the capture and undone (the feed's cursor, accumulators and muting step index, and `restore`: what
        step() changes beyond the engine's own state), captured as one graph.  Returns (replay, the graph): replay() with the
        attributes both forms have (losses, slots, steps, feed; logits and preds of a multi-step graph) and `attrs`."""
        if steps < 1:
            raise ValueError(f"{name}: steps >= 1")
        if feed.B != self.B or feed.device != self.device:
            raise ValueError(f"{name}: the feed's batch size / device ({feed.B}, {feed.device}) are not the engine's "
                             f"({self.B}, {self.device})")
        feed.bind(self)
        slots = [feed.new_slots() for _ in range(steps)]

        def fed_step(i):
            feed.gather_into(slots[i])
            step(*slots[i])
            feed.accumulate(self, slots[i][-1])

        # (the warm-up gathers advance the muting schedule's step index too)
        mute = [] if feed.mute_state is None else [feed.mute_state]
        self._undo_warmup(lambda: fed_step(0), [feed.state, feed._acc, *mute, *restore])
        with self._per_step_outputs(steps) as (outs, enter):
            def all_steps():
                for i in range(steps):
                    enter(i)
                    fed_step(i)

            g = self._graph_of(all_steps)
        out_losses = self.losses if outs is None else outs[0]

        def replay():
            g.replay()
            return out_losses

        replay.losses, replay.slots, replay.steps, replay.feed = out_losses, slots, steps, feed
        if steps > 1:
            replay.logits, replay.preds = outs[1], outs[2]
        for k, v in attrs.items():
            setattr(replay, k, v)
        return replay, g

    def capture_feed_eval(self, feed: EpochFeed, steps: int = 1, scores: Optional[ScoreTable] = None,
                          rank: Optional[RankBuffer] = None, record: Optional[PredictionRecord] = None, grad_sync=None):
        """capture_feed's evaluation counterpart: capture `steps` consecutive EVALUATION steps that feed themselves from `feed`;
        returns a callable replay() without arguments.  Each captured step is: m2m_feed_gather into that step's input slots,
        evaluate() on the slots (dropout off) with its count-table launch, ranking append and record append where `scores`,
        `rank`, `record` are given, m2m_epoch_accumulate into the feed's accumulators -- so a validation or test pass is
        n / (B * steps) replays, one feed.read() and, with a record, one record.read().  On a training engine or on
        sibling(B, trains=False).  replay.slots / .steps / .feed / .losses as for capture_feed; replay.eval is True and
        replay.scores / .rank / .record are the accumulators the graph adds into (data.run_epoch_fed checks them against the
        pass's own).
        Like capture() it leaves everything as it found it: the warm-up runs outside the capture and is undone -- the feed's cursor
        and accumulators, the table, the ranking state and the record's state included; parameters, Adam moments and the step and
        dropout counters are not touched by an evaluation in the first place.  Captured training graphs stay valid.
        A bf16 engine whose weights changed since its last pack() -- an evaluating sibling after training steps on its parent --
        must be packed before a replay, as before any evaluation on a sibling; the graph does not hide a pack().
        Single GPU only: a grad_sync is refused, as in capture_feed."""
        if grad_sync is not None:
            raise ValueError("capture_feed_eval is only supported without a gradient exchange (single GPU)")
        accs = PassAccumulators(scores, rank, record)
        return self._capture_fed("capture_feed_eval", feed, steps, lambda *batch: self.evaluate(*batch, **accs.kwargs()),
                                 accs.state(), dict(accs._asdict(), eval=True))[0]


class _TwoTowerEngine(_FlatEngine):
    """Two MLPMixer towers (patch embedding) -> fusion function -> FusionMixer -> three heads.
    ConcatFusion(dim=1) (the default) costs nothing: the towers write the halves of the fusion tower's input.  Sum / mean / max
    and BiModalGatedUnit: the towers write buffers of their own, one launch fuses them (m2m_fusion_forward / m2m_gate_forward)
    and its backward splits the fusion tower's input gradient (the gate adds a weight-gradient launch)."""

    MODS: Tuple[str, str] = ("image", "audio")

    def _param_shapes(self, cfg):
        return two_tower_param_shapes(cfg, self.MODS)

    def _segment_of(self, k: str) -> str:
        a, b = self.MODS
        return a if k.startswith(f"{a}_mixer.") else (b if k.startswith(f"{b}_mixer.") else "fusion")

    def _build(self):
        a, b = self.MODS
        cfg = self.cfg
        ca, cb, cm = cfg[a], cfg[b], cfg["multimodal"]
        self.D = ca["hidden_dim"]
        self.fusion_name = fusion_function_name(cm)
        self.concat = self.fusion_name == "ConcatFusion"
        if not (cb["hidden_dim"] == self.D == cm["hidden_dim"]):
            raise RuntimeError(f"both towers and the fusion mixer must share hidden_dim ({self.fusion_name} on dim 1)")
        if self.fusion_name == "BiModalGatedUnit" and not (cm["mod1_in"] == cm["mod2_in"] == cm["out_size"] == self.D):
            raise RuntimeError(f"multimodal.mod1_in / mod2_in / out_size = {cm['mod1_in']} / {cm['mod2_in']} / {cm['out_size']}: "
                               f"the engine's BiModalGatedUnit takes and gives the towers' hidden_dim {self.D} (one D for the heads)")
        self.Na, self.Nb = _num_patch(ca), _num_patch(cb)
        self.Nf = fusion_tokens(cm, self.Na, self.Nb)
        self.t_a = self._make_tower(f"{a}_mixer.", ca, self.Na, 0)
        self.t_b = self._make_tower(f"{b}_mixer.", cb, self.Nb, 1024)
        self.t_fus = self._make_tower("fusion_mixer.", cm, self.Nf, 2048)

        def make_embed(prefix, c):
            e = EmbedRuntime(c["in_channels"], c["image_size"][0], c["image_size"][1], c["patch_size"], c["patch_size"],
                             self.D, self.prec)
            e.bind_params(self.params[prefix + "to_patch_embedding.0.weight"], self.params[prefix + "to_patch_embedding.0.bias"])
            e.bind_grads(self.grads[prefix + "to_patch_embedding.0.weight"], self.grads[prefix + "to_patch_embedding.0.bias"])
            return e

        self.e_a = make_embed(f"{a}_mixer.", ca)
        self.e_b = make_embed(f"{b}_mixer.", cb)
        self._towers, self._embeds = [self.t_a, self.t_b, self.t_fus], [self.e_a, self.e_b]
        B, D, dev = self.B, self.D, self.device
        f = lambda *s: torch.zeros(*s, device=dev)
        # embedding outputs; a long-K embedding (audio) is computed as k-split partial sums that the tower launch adds
        grouped = can_group_embeds(self.e_a, self.e_b) and can_group(self.t_a, self.t_b, self.B)
        self.x0_splits = (self.e_a.fwd_splits(), self.e_b.fwd_splits()) if grouped and not self.t_a.wide else (1, 1)
        self._x0_a, self._x0_b = f(self.x0_splits[0], B * self.Na, D), f(self.x0_splits[1], B * self.Nb, D)
        self.x0_a, self.x0_b = self._x0_a[0], self._x0_b[0]
        self.fused, self.fus_out = f(B, self.Nf, D), f(B, self.Nf, D)
        self.pool_a, self.pool_b, self.pool_fus = f(B, D), f(B, D), f(B, D)
        self.dpool_a, self.dpool_b, self.dpool_fus = f(B, D), f(B, D), f(B, D)
        self.d_fused = f(B, self.Nf, D)
        self.dx0_a, self.dx0_b = f(B * self.Na, D), f(B * self.Nb, D)
        self._build_fusion()
        self.preds = torch.zeros(self._preds_shape(), dtype=torch.int32, device=dev)
        # M2M_EARLY_FUSION_WGRAD=1 (wide towers, small batch): the fusion tower's weight gradients on a side stream beside the
        # two modality towers' backward launches instead of inside the merged launch at the end.  Measured on MM-IMDb at its
        # cfg batch: 0.555 ms against 0.502 ms merged -- the extra fork / join of the replayed graph and a single-tower launch
        # without its slot (80 steps) cost more than the shorter tail returns.  Off.
        self._early_fus_wgrad = (self.concurrent and self.t_fus.wide and B * self.Nf <= 8192 and
                                 config.switch_on("M2M_EARLY_FUSION_WGRAD"))
        self._setup_wgrad([[self.t_fus], [self.t_a, self.t_b]] if self._early_fus_wgrad else [[self.t_fus, self.t_a, self.t_b]])
        self._fused_heads = self._heads_are_ce() and self.t_fus.backward_heads_ok(B, 3, self.K)
        # Wide towers (MM-IMDb): their forward cannot pool inside the chain launch (a workgroup does not own whole samples) and
        # appends a token-mean launch; the heads kernel pools the tower outputs itself instead (m2m_head.tokens): two launches less.
        self._heads_pool = (self.t_a.wide and self.t_b.wide and self.t_fus.wide and config.switch_on("M2M_HEADS_POOL"))
        # the fusion tower's backward is always followed by the weight-gradient launch (_backward): the reduction of its
        # small-gradient slots rides there instead of being a launch between the two backward launches (M2M_DEFER_SMALL=0: A/B)
        self.t_fus.set_wgrad_reduces_small(not self._fused_heads and config.switch_on("M2M_DEFER_SMALL"))
        # the heads' weight gradients: per-workgroup slots added in a fixed order by the weight-gradient launch instead of float
        # atomics -- with them a bf16 step is bit-reproducible (M2M_HEAD_SLOTS=0: atomics)
        self._head_part, self._wgrad_heads = None, None
        if (self._heads_write_slots() and not self._fused_heads and config.switch_on("M2M_HEAD_SLOTS")
                and self.K * D + self.K + 2 <= L.SPLIT_GPART):
            self._head_part = torch.zeros(3, int(L.lib().m2m_heads_part_tiles(B)), L.SPLIT_GPART, device=dev)
        # the two modality towers' backward launch: slots instead of 128-way contended float atomics for the small gradients,
        # their reduction in the weight-gradient launch as well (M2M_GROUP_SLOTS=0: atomics, A/B)
        if (config.switch_on("M2M_GROUP_SLOTS") and self.t_a.has_small_slots() and self.t_b.has_small_slots()
                and can_group(self.t_a, self.t_b, self.B)):
            for t in (self.t_a, self.t_b):
                t.set_wgrad_group_slots(True)
                t.set_wgrad_reduces_small(True)
        # the embeddings' weight gradients in their single-owner form: the tower backward leaves d_x0^T as packed blocks
        self._embed_towers = []
        if config.switch_on("M2M_EMBED_FAST") and self.t_a.enable_dx0_image(B) and self.t_b.enable_dx0_image(B):
            self._embed_towers = [self.t_a, self.t_b]
            # their weight gradients are then written ("="), and Adam leaves those ranges uncleared -- if the range table has room
            fast = bool(L.lib().m2m_embeds_wgrad_form(_embed_ptrs(self._embeds), _tower_ptrs(self._embed_towers), 2, B))
            if fast and config.switch_on("M2M_WGRAD_OVERWRITE"):
                self._keep_embed_ranges(self._embed_weight_grads())

        # Patch embeddings inside the two-tower forward launch (m2m_towers_forward_embeds: -1 launch at the head of the step).
        # The step head then splits: losses = 0 / Adam step += 1 ride in that launch, the dropout counter -- which that launch
        # READS -- holds "steps completed", every launch of a training step is given step = 1 and the merged weight-gradient
        # launch (the last reader is long done) advances it.  Observable counter values are those of the prologue form.
        # OFF by default (M2M_EMBED_FOLD=1 enables it).  Measured on M2-Mixer-B, batch 512, three interleaved repetitions in one
        # process: towers forward 103-105 us with the embeddings inside against 84-85 + 21-22 us as two launches, step
        # 0.5116-0.5163 against 0.5067-0.5121 ms -- the audio tower's 128 workgroups each stream the whole 800 KB embedding
        # weight + 200 KB of input alone (+19 us, not the 7.5 us the CU's 64 B/clk would allow) while the image tower's 128 CUs
        # wait; the launch of its own spreads that work over 256 + 128 workgroups (k-split).  Parity-green either way.
        self._embed_fold = (config.switch_on("M2M_EMBED_FOLD") and grouped and self.concurrent and not self._early_fus_wgrad
                            and self.x0_splits is not None and self.e_a.prec == self.t_a.prec and self.e_a.D == self.t_a.D
                            and towers_forward_embeds_ok([self.t_a, self.t_b], [self.e_a, self.e_b], B)
                            and self.t_a.wgrad_form(B) == 0 and self.t_fus.wgrad_form(B) == 0)
        self._pending_bump = False

    def _build_fusion(self):
        """Buffers of a fusion other than ConcatFusion: the towers' own outputs (B, N, D) and their input gradients; the gate's
        descriptor (weights from the fp32 masters, gradients into the flat buffer), saved activations and partial sums."""
        B, D, dev = self.B, self.D, self.device
        self.out_a = self.out_b = self.d_out_a = self.d_out_b = None
        self.gate = None
        if self.concat:
            return
        f = lambda *s: torch.zeros(*s, device=dev)
        self.out_a, self.out_b = f(B, self.Na, D), f(B, self.Nb, D)
        if self.fusion_name == "SumFusion":
            self.d_out_a = self.d_out_b = self.d_fused          # d(a + b) / da = d(a + b) / db = 1: both towers read d_fused
        else:
            self.d_out_a, self.d_out_b = f(B, self.Na, D), f(B, self.Nb, D)
        if self.fusion_name != "BiModalGatedUnit":
            return
        rows = B * self.Nf
        self._gate_bufs = dict(t1=f(rows, D), t2=f(rows, D), z=f(rows, D), dh=f(rows, 3 * D),
                               part=f(int(L.lib().m2m_gate_part_floats(rows, D))))
        g = L.Gate()
        g.D = D
        P, G = self.params, self.grads
        for fld, key in (("w1", "mod1_hidden.weight"), ("b1", "mod1_hidden.bias"), ("w2", "mod2_hidden.weight"),
                         ("b2", "mod2_hidden.bias"), ("wz", "z_hidden.weight"), ("bz", "z_hidden.bias")):
            setattr(g, fld, P["fusion_function." + key].data_ptr())
            setattr(g, "g_" + fld, G["fusion_function." + key].data_ptr())
        for fld, t in self._gate_bufs.items():
            setattr(g, fld, t.data_ptr())
        self.gate = g

    def _tower_outputs(self):
        """(out_a, out_b, sample stride): where the two towers write their tokens."""
        D = self.D
        if self.concat:
            return self.fused, self.fused.view(-1)[self.Na * D:], self.Nf * D
        return self.out_a, self.out_b, None

    def _fusion_forward(self, training: bool):
        rows = self.B * self.Nf
        if self.concat:
            return
        if self.gate is not None:
            L.check(L.lib().m2m_gate_forward(C.byref(self.gate), self.out_a.data_ptr(), self.out_b.data_ptr(), self.fused.data_ptr(),
                                             rows, int(training), L.stream_ptr()), "gate_forward")
        else:
            L.check(L.lib().m2m_fusion_forward(_ELEM_FUSION_MODE[self.fusion_name], self.out_a.data_ptr(), self.out_b.data_ptr(),
                                               self.fused.data_ptr(), rows * self.D, L.stream_ptr()), "fusion_forward")

    def _fusion_backward(self):
        """d_fused -> the towers' output gradients (and the gate's weight gradients, added into flat_g: Adam clears them)."""
        rows = self.B * self.Nf
        if self.concat or self.fusion_name == "SumFusion":
            return
        if self.gate is not None:
            L.check(L.lib().m2m_gate_backward(C.byref(self.gate), self.d_fused.data_ptr(), self.d_out_a.data_ptr(),
                                              self.d_out_b.data_ptr(), rows, L.stream_ptr()), "gate_backward")
            L.check(L.lib().m2m_gate_wgrad(C.byref(self.gate), self.out_a.data_ptr(), self.out_b.data_ptr(), rows, L.stream_ptr()),
                    "gate_wgrad")
        else:
            L.check(L.lib().m2m_fusion_backward(_ELEM_FUSION_MODE[self.fusion_name], self.out_a.data_ptr(), self.out_b.data_ptr(),
                                                self.d_fused.data_ptr(), self.d_out_a.data_ptr(), self.d_out_b.data_ptr(),
                                                rows * self.D, L.stream_ptr()), "fusion_backward")

    def _preds_shape(self):
        return (3, self.B)

    def _loss_heads(self, heads, labels, zero_losses):
        raise NotImplementedError

    def _heads_are_ce(self) -> bool:
        """True: three cross-entropy heads (the form m2m_tower_backward_heads computes)."""
        return False

    def _heads_write_slots(self) -> bool:
        """True: the heads launch can leave its weight gradients in per-workgroup slots (m2m_head.g_part) for the weight-gradient
        launch to add: the cross-entropy heads, and any engine whose own heads launch keeps that contract."""
        return self._heads_are_ce()

    # ---- one training step (enqueue only; no host synchronisation) ----------------------------------------
    def _forward(self, xa, xb, labels, training: bool, with_grad: bool, prologue: bool = False):
        B, D = self.B, self.D
        sd = self.drop_step if training else None
        fs = self.Nf * D
        out_a, b_part, ts = self._tower_outputs()
        sa_, sb_ = (ts, ts) if self.concat else (self.Na * D, self.Nb * D)      # sample strides of the two towers' outputs
        main, side, _ = self._streams()
        so = 0                                               # host step offset of this pass's launches (see _embed_fold)
        pa, pb, pf = (None, None, None) if self._heads_pool else (self.pool_a, self.pool_b, self.pool_fus)
        self._pending_bump = False
        self._step_weights = self._pass_weights(training)
        if self._embed_fold and training and prologue and not self._staged and not self._probing:      # (a stage: the plain head of the step)
            # both patch embeddings inside the two-tower launch; head of the step: losses = 0, Adam step += 1 in that launch,
            # the dropout counter advances in the weight-gradient launch of _backward (every launch in between gets step = 1)
            so, self._pending_bump = 1, True
            towers_forward([self.t_a, self.t_b],
                           [(self.x0_a, self.Na * D, out_a, sa_, pa), (self.x0_b, self.Nb * D, b_part, sb_, pb)],
                           B, training, self.seed, so, sd, embeds=[self.e_a, self.e_b], inputs=[xa, xb],
                           head=(self.adam_state, self.losses))
        elif self.concurrent and can_group(self.t_a, self.t_b, self.B):
            # one launch for both patch embeddings, one for both towers (blockIdx.y = tower), all on the main stream: no
            # cross-queue fork / join in the graph (a join costs ~6 us even when its event fired long ago)
            sa, sb = self.x0_splits
            if can_group_embeds(self.e_a, self.e_b):
                # the step prologue (counters, losses = 0) rides in this launch, the first one of the step
                head = (self._head_adam(), self.drop_step, self.losses) if prologue else None
                embeds_forward([self.e_a, self.e_b], [xa, xb], [self._x0_a, self._x0_b], B, [sa, sb], head)
            else:
                if prologue:
                    self._prologue()
                sa = sb = 1
                self.e_a.forward(xa, B, self.x0_a)
                self.e_b.forward(xb, B, self.x0_b)
            towers_forward([self.t_a, self.t_b],
                           [(self.x0_a, self.Na * D, out_a, sa_, pa, sa, B * self.Na * D),
                            (self.x0_b, self.Nb * D, b_part, sb_, pb, sb, B * self.Nb * D)],
                           B, training, self.seed, 0, sd)
        else:
            if prologue:
                self._prologue()
            side.wait_stream(main)
            with torch.cuda.stream(side):                   # second tower beside the first
                self.e_b.forward(xb, B, self.x0_b)
                self.t_b.forward(self.x0_b, self.Nb * D, B, b_part, sb_, pb, training, self.seed, 0, sd)
            self.e_a.forward(xa, B, self.x0_a)
            self.t_a.forward(self.x0_a, self.Na * D, B, out_a, sa_, pa, training, self.seed, 0, sd)
            main.wait_stream(side)
        modal = training and self._modal                    # the modalities-only stage: no fusion function, no fusion tower
        if not modal:
            self._fusion_forward(training and with_grad)
            self.t_fus.forward(self.fused, fs, B, self.fus_out, fs, pf, training, self.seed, so, sd)
        a, b = self.MODS
        hw = self.head_weights
        heads = [self._head(a, self.pool_a, self.dpool_a, hw[a], with_grad),
                 self._head(b, self.pool_b, self.dpool_b, hw[b], with_grad),
                 self._head("fusion", self.pool_fus, self.dpool_fus, hw["fusion"], with_grad)]
        if self._heads_pool:
            heads[0]["tokens"] = (out_a, self.Na, sa_)
            heads[1]["tokens"] = (b_part.data_ptr(), self.Nb, sb_)
            heads[2]["tokens"] = (self.fus_out, self.Nf, fs)
        self._wgrad_heads = None
        if modal:
            heads = heads[:2]                              # (their total lands in losses[2]: _stage_total)
        if training and with_grad and self._head_part is not None and not self._staged:
            # (a stage: its weight-gradient call adds no slots; the heads add with atomics)
            for i, h in enumerate(heads):
                h["g_part"] = self._head_part[i]
            self._wgrad_heads = heads                     # _backward's weight-gradient launch adds the slots to g_w / g_b
        self._heads = heads
        self._labels = labels
        if training and with_grad and self._fused_heads:
            return                                         # heads + losses ride in the fusion tower's backward launch (_backward)
        self._loss_heads(heads, labels, not training)      # a training step's _prologue already cleared the losses
        self._stage_total(training)

    def _backward(self, xa, xb, fused_update: bool = False):
        """Backward of the whole model.  fused_update: also apply Adam + re-pack (single-GPU path; with a gradient
        all-reduce the update is a separate phase)."""
        B, D = self.B, self.D
        fs = self.Nf * D
        sd = self.drop_step
        if self._frozen:
            # stage two: nothing behind the fusion function trains.  The fusion tower's backward, a non-concat fusion's own
            # backward (a gated unit's weight gradients are trainable), the fusion tower's weight gradients as a single-tower
            # call, Adam over the trainable ranges, the fusion tower's re-pack -- all on the main stream.
            self.t_fus.backward(B, None, 0, self.dpool_fus, self.d_fused, fs, self.seed, 0, sd)
            self._fusion_backward()
            self.t_fus.wgrad(B, self.seed, 0, sd)
            if fused_update:
                self._update(1.0)
            return
        a, b = self.MODS
        so = 1 if self._pending_bump else 0                 # (the forward of this step left the dropout counter un-advanced)
        modal = self._modal
        if modal:
            pass                                            # the modalities-only stage: nothing of the fusion tower runs
        elif self._fused_heads:
            # the three heads + multi-head CE in the prologue of this launch (m2m_tower_backward_heads): one launch less
            self.t_fus.backward_heads(B, self._heads, 2, self._labels, self.K, (self.logits, self.losses, self.preds),
                                      self.d_fused, fs, self.seed, so, sd)
        else:
            self.t_fus.backward(B, None, 0, self.dpool_fus, self.d_fused, fs, self.seed, so, sd)
        if modal:
            d_a_part, d_b_part, sa_, sb_ = None, None, 0, 0   # the towers' backward starts from their heads' d_pooled alone
        elif self.concat:
            d_a_part, d_b_part, sa_, sb_ = self.d_fused, self.d_fused.view(-1)[self.Na * D:], fs, fs
        else:
            self._fusion_backward()
            d_a_part, d_b_part, sa_, sb_ = self.d_out_a, self.d_out_b, self.Na * D, self.Nb * D
        main, s_a, s_f = self._streams()
        wg_towers = [self.t_a, self.t_b] if modal else [self.t_fus, self.t_a, self.t_b]
        if self._early_fus_wgrad and not modal:
            s_f.wait_stream(main)
            with torch.cuda.stream(s_f):
                self.t_fus.wgrad(B, self.seed, so, sd)
            wg_towers = [self.t_a, self.t_b]
        s_e = self.s_emb if self.concurrent else main
        # The two tower chains fill the chip (128 + 128 workgroups) side by side; then ONE launch computes the channel-mixing
        # weight gradients of all three towers (the hardware dispatcher balances their ~300 workgroups; three launches on
        # three queues of a replayed graph raced and sometimes serialised each other) AND the two patch-embedding
        # gradients, whose workgroups back-fill the CUs the tower workgroups leave idle: the whole step is one queue.
        # (Any side stream forks from and joins into `main` directly: a fork from a forked stream crashed hipGraph
        # capture on ROCm 7.2.)
        if self.concurrent and can_group(self.t_a, self.t_b, self.B):
            towers_backward([self.t_a, self.t_b],
                            [(d_a_part, sa_, self.dpool_a, self.dx0_a, self.Na * D), (d_b_part, sb_, self.dpool_b, self.dx0_b, self.Nb * D)],
                            B, self.seed, so, sd)
        else:
            s_a.wait_stream(main)
            with torch.cuda.stream(s_a):
                self.t_a.backward(B, d_a_part, sa_, self.dpool_a, self.dx0_a, self.Na * D, self.seed, so, sd)
            self.t_b.backward(B, d_b_part, sb_, self.dpool_b, self.dx0_b, self.Nb * D, self.seed, so, sd)
            main.wait_stream(s_a)
        bump = self.drop_step if self._pending_bump else None
        if can_group_embeds(self.e_a, self.e_b) and self.e_a.prec == self.t_a.prec and self.e_a.D == self.t_a.D:
            towers_wgrad(wg_towers, B, [self.e_a, self.e_b], [xa, xb], [self.dx0_a, self.dx0_b],
                         seed=self.seed, step=so, step_dev=sd, embed_towers=self._embed_towers, heads=self._wgrad_heads, K=self.K,
                         bump=bump)
        else:
            if bump is not None:
                raise RuntimeError("the embedding fold needs the merged weight-gradient launch (it advances the dropout counter)")
            s_e.wait_stream(main)
            with torch.cuda.stream(s_e):
                self.e_b.wgrad(xb, self.dx0_b, B)
                self.e_a.wgrad(xa, self.dx0_a, B)
            towers_wgrad(wg_towers, B, seed=self.seed, step=so, step_dev=sd, heads=self._wgrad_heads, K=self.K)
            main.wait_stream(s_e)
        self._pending_bump = False
        if self._early_fus_wgrad and not modal:
            main.wait_stream(s_f)
        if fused_update:
            self._update(1.0)

    def _embed_weight_grads(self) -> list:
        """[(patch embedding, its weight's gradient view)] of the two modalities."""
        return [(e, self.grads[f"{m}_mixer.to_patch_embedding.0.weight"]) for e, m in zip(self._embeds, self.MODS)]

    def _keep_embed_ranges(self, owners: list):
        """Enter the weight-gradient ranges of embeddings that can run in their single-owner form into _ranges_add (owners: of
        _embed_weight_grads): the gradients are then written ("="), and Adam leaves those ranges uncleared -- if the range table
        has room for all of them; else the embeddings add into cleared ranges like everything else."""
        fits = len(self._ranges_add) + len(owners) <= L.MAX_GRAD_RANGES
        for e, gw in owners:
            e.set_wgrad_overwrite(fits)
            if fits:
                self._ranges_add.append(((gw.data_ptr() - self.flat_g.data_ptr()) // 4, gw.numel(), None, 1))
        self._ranges_add.sort(key=lambda r: r[0])

    def _stage_options(self):
        """The options _build chose for the grouped weight-gradient launch (the fusion tower's slot, overwrite decided with the
        slot in hand, the embeddings' kept ranges) re-derived for the stage's own launch: the single-tower call of stage two, or
        the two modality towers and their embeddings without the fusion tower, whose slot and kept ranges leave the table."""
        towers = [self.t_fus] if self._frozen else [self.t_a, self.t_b]
        for t in dict.fromkeys(towers + [self.t_fus]):       # (a fusion tower that leaves the launch gives up its ranges too)
            t.set_wgrad_overwrite(False)
        self._setup_wgrad([towers])
        if not self._frozen:
            # the embeddings' gradients ride in their towers' launch: they keep their single-owner form and their uncleared
            # ranges where the table still has room
            self._keep_embed_ranges([(e, gw) for e, gw in self._embed_weight_grads() if e.desc.wgrad_flags & L.WGRAD_OVERWRITE])

    def _stage_packs(self) -> list:
        return [self.t_fus] if self._frozen else [self.t_a, self.e_a, self.t_b, self.e_b]

    def _update_chunks(self):
        """One chunk per parameter segment, in flat order: modality a (its patch embedding + tower), modality b, fusion tower
        + the three heads (heads have no packed copies)."""
        a, b = self.MODS
        mods = {a: [self.t_a, self.e_a], b: [self.t_b, self.e_b], "fusion": [self.t_fus]}
        segs = sorted(self.segments.items(), key=lambda kv: kv[1][0])
        return [(lo, hi, mods[name]) for name, (lo, hi) in segs]

    def _eval_outputs(self) -> dict:
        a, b = self.MODS
        return {"logits": self.logits[2], f"{a}_logits": self.logits[0], f"{b}_logits": self.logits[1],
                f"loss_{a}": self.losses[0], f"loss_{b}": self.losses[1], "loss_fusion": self.losses[2],
                "loss": self.losses[3], "preds": self.preds[2], f"preds_{a}": self.preds[0], f"preds_{b}": self.preds[1]}


class AVMnistEngine(_TwoTowerEngine):
    """cfg: {'dropout', 'num_classes', 'image': {...}, 'audio': {...}, 'multimodal': {...}} with the keys of
    cfg/avmnist/avmnist_m2-mixer_*.yml (model.modalities.*)."""

    MODS = ("image", "audio")

    def __init__(self, cfg: dict, batch_size: int, device="cuda:0", precision: Optional[str] = None,
                 lr: float = 1e-2, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 fusion_loss_weight: float = 1.0 / 3, seed: int = 42, init: bool = True, share=None, scores: bool = False,
                 rank_scores: bool = False, rank_capacity: int = 65536):
        w = fusion_loss_weight
        ow = (1 - w) / 2
        # loss = (w Lf + ow Li + ow La) * 3      (models/avmnist.py:289-290)
        self.head_weights = {"image": 3 * ow, "audio": 3 * ow, "fusion": 3 * w}
        self.fusion_loss_weight = w
        super().__init__(cfg, batch_size, device, precision, lr, betas, eps, weight_decay, seed, init, share, scores, rank_scores,
                         rank_capacity)

    HEAD_NAMES = ("image", "audio", "fusion")
    SCORES_TASK = "avmnist"

    def set_fusion_loss_weight(self, w: float):
        ow = (1 - w) / 2
        self.set_loss_weights(3 * ow, 3 * ow, 3 * w)          # loss = (w Lf + ow Li + ow La) * 3   (models/avmnist.py:289-290)
        self.fusion_loss_weight = w

    def _loss_heads(self, heads, labels, zero_losses):
        heads_ce(heads, labels, self.B, self.D, self.K, out=(self.logits, self.losses, self.preds), zero_losses=zero_losses,
                 weights=self._step_weights)

    def _heads_are_ce(self) -> bool:
        return True

    # names kept from the first engine revision (bench.py, tests)
    t_img = property(lambda self: self.t_a)
    t_aud = property(lambda self: self.t_b)
    e_img = property(lambda self: self.e_a)
    e_aud = property(lambda self: self.e_b)
    s_aud = property(lambda self: self.s_b)
    Ni = property(lambda self: self.Na)
    x0_img = property(lambda self: self.x0_a)


class AVMnistUQEngine(AVMnistEngine):
    """AVMnistEngine with the evidential heads of the reference's AVMnistMixerMultiLossUQ (models/avmnist.py:447-572): the three
    cross-entropy losses become EDLMSELoss squared-error Bayes risks (modules/losses.py:5-31, m2m_heads_edl), every sample gets a
    per-head uncertainty K / S, and the model's prediction is that of the least uncertain head.  Same parameters, same towers.

      * loss = loss_image + loss_audio + loss_fusion (avmnist.py:511): coefficients 1, 1, 1, no fusion_loss_weight
        (set_fusion_loss_weight is refused; set_loss_weights works, captured graphs follow it);
      * `preds` (3, B) rows are [image, audio, combined] -- the reference's preds_image, preds_audio, preds: score tables,
        data.run_epoch and evaluate() work unchanged and the plain score names mean the combined prediction (the fusion head's own
        argmax is not kept; it is argmax relu(logits[2]));
      * `uncertainty` (3, B) fp32 rows are [image, audio, fusion]; evaluate() returns them too.  A multi-step captured graph
        (capture(steps > 1)) writes every step's values there: afterwards it holds the last step's;
      * rank_scores=True is refused: the ranking buffers store a softmax, which is not this model's class probability.

    Three cfg keys choose the loss among the pieces of the reference's modules/losses.py (the reference hard-codes them; the keys
    are this build's extension).  The defaults are the reference's model, and with them nothing differs from an engine without
    the keys: m2m_heads_edl is called, no further buffer exists.
      * `edl_loss`: "mse" (default; EDLMSELoss, losses.py:24-31) or "ce" (EDLCELoss, :71-93): the Bayes risk of every head;
      * `kl_weight` (default 0.0) > 0 adds lambda x the Dirichlet KL regulariser (kl_divergence_loss, :52-68) to every head's loss,
        lambda = kl_weight x min(1, epoch / annealing_step) (:15-18);
      * `annealing_step` (default 10: the reference's EDLMSELoss(num_classes, 10)).
    With kl_weight > 0 the engine owns `kl_coef`, one device float holding lambda (shared with siblings like `loss_weights`; a
    clone gets a copy), and `kl` (3,): the heads' unscaled batch-mean KL of the last pass.  set_epoch(epoch) writes lambda in
    place: captured graphs and feed graphs follow from their next replay.  Evaluation uses the same lambda (the reference passes
    current_epoch in validation too).  A new engine is at epoch 0: lambda = 0, where the launch skips all KL arithmetic."""

    EDL_LOSSES = ("mse", "ce")

    def __init__(self, cfg: dict, batch_size: int, device="cuda:0", precision: Optional[str] = None,
                 lr: float = 1e-2, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 seed: int = 42, init: bool = True, share=None, scores: bool = False,
                 rank_scores: bool = False, rank_capacity: int = 65536):
        if rank_scores:
            raise RuntimeError("AVMnistUQEngine: rank_scores=True: the ranking buffers store the softmax of the logits, which is "
                               "not the evidential model's class probability (alpha / S)")
        self.edl_loss = cfg.get("edl_loss", "mse")
        self.kl_weight = float(cfg.get("kl_weight", 0.0))
        self.annealing_step = cfg.get("annealing_step", 10)
        if self.edl_loss not in self.EDL_LOSSES:
            raise ValueError(f"AVMnistUQEngine: edl_loss must be one of {', '.join(self.EDL_LOSSES)}, got {self.edl_loss!r}")
        if not self.kl_weight >= 0.0 or not self.annealing_step > 0:
            raise ValueError("AVMnistUQEngine: kl_weight >= 0 and annealing_step > 0")
        self.head_weights = {"image": 1.0, "audio": 1.0, "fusion": 1.0}
        # (past AVMnistEngine.__init__, which derives the coefficients from a fusion_loss_weight this model does not have)
        _TwoTowerEngine.__init__(self, cfg, batch_size, device, precision, lr, betas, eps, weight_decay, seed, init, share, scores,
                                 rank_scores, rank_capacity)
        self.uncertainty = torch.zeros(3, self.B, device=self.device)
        # the epoch the family is at (host side) and, with the KL term, lambda on the device: shared like loss_weights
        self._epoch_group = share._epoch_group if share is not None else {"epoch": 0}
        self.kl_coef = self.kl = None
        if self.kl_weight > 0.0:
            self.kl_coef = share.kl_coef if share is not None else torch.zeros(1, device=self.device)
            self.kl = torch.zeros(3, device=self.device)

    def set_fusion_loss_weight(self, w: float):
        raise NotImplementedError("AVMnistUQEngine: its loss has no fusion_loss_weight (models/avmnist.py:511)")

    @property
    def epoch(self) -> int:
        return self._epoch_group["epoch"]

    def kl_lambda(self, epoch: Optional[int] = None) -> float:
        """kl_weight x min(1, epoch / annealing_step) (modules/losses.py:15-18) at `epoch` (default: the engine's)."""
        e = self.epoch if epoch is None else epoch
        return self.kl_weight * min(1.0, e / self.annealing_step)

    def set_epoch(self, epoch: int):
        """The epoch the KL term's annealing coefficient follows: lambda is written in place into `kl_coef`, on the current stream
        (behind the steps already enqueued there) -- this engine, its siblings and every graph captured from them read the new
        value from their next launch on; no capture is dropped.  Without the KL term (kl_weight == 0) only the number is kept."""
        if epoch < 0:
            raise ValueError("set_epoch: epoch >= 0")
        self._epoch_group["epoch"] = epoch
        if self.kl_coef is not None:
            self.kl_coef.fill_(self.kl_lambda())

    def clone(self, batch_size: Optional[int] = None):
        new = super().clone(batch_size)
        new.set_epoch(self.epoch)                             # (its own table and epoch, at this engine's values)
        return new

    def _loss_heads(self, heads, labels, zero_losses):
        # (self.preds at call time: a multi-step capture points it at its per-step slots)
        out = (self.logits, self.losses, self.preds, self.uncertainty, self.preds[2])
        if self.edl_loss == "mse" and self.kl_coef is None:
            heads_edl(heads, labels, self.B, self.D, self.K, out=out, zero_losses=zero_losses, weights=self._step_weights)
            return
        if self.kl is not None and not zero_losses:
            self.kl.zero_()                                   # (a training step's prologue cleared the losses, not this)
        heads_edl(heads, labels, self.B, self.D, self.K, out=out, zero_losses=zero_losses, weights=self._step_weights,
                  risk=self.edl_loss, kl_coef=self.kl_coef, kl_out=self.kl)

    def _heads_are_ce(self) -> bool:
        return False                                          # no fused heads + fusion-backward launch: that one computes cross-entropy

    def _heads_write_slots(self) -> bool:
        return True                                           # m2m_heads_edl keeps m2m_heads_ce's g_part contract

    @torch.no_grad()
    def evaluate(self, *batch, scores: Optional[ScoreTable] = None, rank: Optional[RankBuffer] = None,
                 record: Optional[PredictionRecord] = None):
        """AVMnistEngine.evaluate; `preds` is the combined prediction, and the three uncertainties (B) are returned as well (a
        record of this engine holds them per sample)."""
        if rank is not None:
            raise RuntimeError("AVMnistUQEngine: ranking buffers are not built for the evidential model")
        return super().evaluate(*batch, scores=scores, record=record)

    def _eval_outputs(self) -> dict:
        out = super()._eval_outputs()
        out.update(uncertainty=self.uncertainty[2], uncertainty_image=self.uncertainty[0], uncertainty_audio=self.uncertainty[1])
        return out


class MMIMDBEngine(_TwoTowerEngine):
    """cfg: {'dropout', 'num_classes', 'pos_weight': [K], 'image': {...}, 'text': {...}, 'multimodal': {...}} with the
    keys of cfg/mmimdb/mmimdb_3loss.yml.  Loss = BCE_image + BCE_text + BCE_fusion (models/mmimdb.py:115-123),
    preds = sigmoid(logits) > 0.5 (:128-133); labels are (B, K) multi-hot floats."""

    MODS = ("image", "text")
    HEAD_NAMES = ("image", "text", "fusion")
    SCORES_TASK = "mmimdb"
    #: buffers of the three BCEWithLogitsLoss modules in the reference's state_dict (models/mmimdb.py:47-50)
    EXTRA_STATE_KEYS = ("image_criterion.pos_weight", "text_criterion.pos_weight", "fusion_criterion.pos_weight")

    def __init__(self, cfg: dict, batch_size: int, device="cuda:0", precision: Optional[str] = None,
                 lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 seed: int = 42, init: bool = True, share=None, scores: bool = False,
                 rank_scores: bool = False, rank_capacity: int = 65536):
        self.head_weights = {"image": 1.0, "text": 1.0, "fusion": 1.0}
        if rank_scores:
            raise RuntimeError("MMIMDBEngine: rank_scores=True: multilabel ranking is not built (the ranking buffers take one "
                               "label per sample: AVMnistEngine, MimicEngine)")
        super().__init__(cfg, batch_size, device, precision, lr, betas, eps, weight_decay, seed, init, share, scores, rank_scores,
                         rank_capacity)
        self.pos_weight = torch.tensor(cfg["pos_weight"], dtype=torch.float32, device=self.device)
        if self.pos_weight.numel() != self.K:
            raise RuntimeError("pos_weight needs one entry per class")

    def _consume_extra_state(self, key, value):
        v = value.to(self.device, torch.float32).reshape(-1)
        if v.numel() != self.K:
            raise RuntimeError(f"{key}: expected {self.K} entries")
        if key == self.EXTRA_STATE_KEYS[0]:
            self.pos_weight.copy_(v)                 # one pos_weight serves the three heads (the reference builds them equal)
        elif not torch.equal(v, self.pos_weight):
            raise RuntimeError(f"{key} differs from image_criterion.pos_weight: the fused heads kernel takes one pos_weight")

    def _extra_state(self):
        return OrderedDict((k, self.pos_weight.detach().clone()) for k in self.EXTRA_STATE_KEYS)

    def _copy_loaded_state(self, new):
        new.pos_weight.copy_(self.pos_weight)            # the LOADED criterion buffer, not cfg's

    def _preds_shape(self):
        return (3, self.B, self.K)

    def _loss_heads(self, heads, labels, zero_losses):
        heads_bce(heads, labels, self.pos_weight, self.B, self.D, self.K, out=(self.logits, self.losses, self.preds),
                  zero_losses=zero_losses, weights=self._step_weights)


class MimicEngine(_FlatEngine):
    """cfg: {'dropout', 'num_classes', 'time': {...}, 'static': {...}, 'multimodal': {...}} with the keys of
    cfg/mimic/mimic_m2-mixer_H.yml.  static (B, 5) -> MLP -> one token; time (B, 24, 12) -> Linear proj -> MixerBlocks;
    fused = cat(static token, time tokens) (models/mimic.py:98-103); loss = w Lf + ow Ls + ow Lt (:115-121, no x3)."""

    def __init__(self, cfg: dict, batch_size: int, device="cuda:0", precision: Optional[str] = None,
                 lr: float = 1e-2, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 fusion_loss_weight: float = 1.0 / 3, seed: int = 42, init: bool = True, share=None, scores: bool = False,
                 rank_scores: bool = False, rank_capacity: int = 65536):
        w = fusion_loss_weight
        ow = (1 - w) / 2
        self.head_weights = {"static": ow, "time": ow, "fusion": w}
        self.fusion_loss_weight = w
        super().__init__(cfg, batch_size, device, precision, lr, betas, eps, weight_decay, seed, init, share, scores, rank_scores,
                         rank_capacity)

    HEAD_NAMES = ("static", "time", "fusion")
    SCORES_TASK = "mimic"

    def set_fusion_loss_weight(self, w: float):
        ow = (1 - w) / 2
        self.set_loss_weights(ow, ow, w)                      # loss = w Lf + ow Ls + ow Lt   (models/mimic.py:115-121, no x3)
        self.fusion_loss_weight = w

    def _param_shapes(self, cfg):
        return mimic_param_shapes(cfg)

    def _segment_of(self, k: str) -> str:
        return "time" if k.startswith("time_mixer.") else ("static" if k.startswith("static_extractor.") else "fusion")

    def _build(self):
        cfg = self.cfg
        ct, cs, cm = cfg["time"], cfg["static"], cfg["multimodal"]
        self.D = ct["hidden_dim"]
        if not (ct["proj_dim"] == self.D == cm["hidden_dim"] == cs["output_dim"]):
            raise RuntimeError("time hidden_dim / proj_dim, static output_dim and fusion hidden_dim must agree")
        self.Nt = ct["num_patch"]
        self.Nf = 1 + self.Nt
        # Side streams (static MLP beside the time tower; the three parameter segments' weight gradients + Adam side by side):
        # every fork / join edge of the replayed graph costs ~5 us, the launches they hide are 5-30 us at the cfg batch:
        # measured 0.230 ms on one stream against 0.255 ms on three (fwd only 0.257, bwd only 0.25-0.27); at batch 8192 the
        # launches are long enough: 2.445 ms on three streams against 2.492 on one.  M2M_MIMIC_STREAMS=fwd|bwd|both|none (A/B).
        mode = config.switch("M2M_MIMIC_STREAMS", "none" if self.B <= 1024 else "both")
        self._merged_tail = config.switch_on("M2M_MIMIC_MERGED_TAIL")          # (A/B)
        # merged tail: the input projection's weight gradient in the towers' weight-gradient launch (one launch less)
        self._embed_wgrad_merged = config.switch_on("M2M_MIMIC_EMBED_WGRAD_MERGED")
        self._conc_fwd, self._conc_bwd = mode in ("fwd", "both"), mode in ("bwd", "both")
        # the heads pool the time and fusion towers' tokens themselves (m2m_head.tokens), on either path: a wide tower (MIMIC-H:
        # N = 24 / 25) would append a token-mean launch, a fused one (num_patch <= 8 / <= 7) is simply not asked to pool
        self._heads_pool = config.switch_on("M2M_HEADS_POOL")
        # the static MLP's two launches as extra workgroups of the time tower's token-mixing launches (MlpRuntime.forward_ride);
        # a fused time tower has no such launch and ride_flush launches the recorded call on its own
        self._mlp_ride = config.switch_on("M2M_MLP_RIDE") and self.B <= 2048
        self.t_time = self._make_tower("time_mixer.", ct, self.Nt, 0)
        self.t_fus = self._make_tower("fusion_mixer.", cm, self.Nf, 2048)
        # (B, N, K) rows == a (B, 1, N, K) image cut into (1, K) patches
        self.e_time = EmbedRuntime(1, self.Nt, ct["embedding_dim"], 1, ct["embedding_dim"], self.D, self.prec)
        self.e_time.bind_params(self.params["time_mixer.proj.weight"], self.params["time_mixer.proj.bias"])
        self.e_time.bind_grads(self.grads["time_mixer.proj.weight"], self.grads["time_mixer.proj.bias"])
        self._towers, self._embeds = [self.t_time, self.t_fus], [self.e_time]
        nb = cs["num_blocks"]
        keys = [f"static_extractor.module_list.{3 * i}." for i in range(nb)] + [f"static_extractor.module_list.{3 * nb}."]
        self.mlp = MlpRuntime([cs["input_dim"]] + [cs["hidden_dim"]] * nb + [cs["output_dim"]], True, self.p_drop, 4096)
        self.mlp.bind([(self.params[k + "weight"], self.params[k + "bias"]) for k in keys],
                      [(self.grads[k + "weight"], self.grads[k + "bias"]) for k in keys], self.B)
        B, D, dev = self.B, self.D, self.device
        f = lambda *s: torch.zeros(*s, device=dev)
        self.x0_time = f(B * self.Nt, D)
        self.fused, self.fus_out = f(B, self.Nf, D), f(B, self.Nf, D)
        self.pool_static, self.pool_time, self.pool_fus = f(B, D), f(B, D), f(B, D)
        self.dpool_static, self.dpool_time, self.dpool_fus = f(B, D), f(B, D), f(B, D)
        self.d_fused = f(B, self.Nf, D)
        self.dx0_time = f(B * self.Nt, D)
        self.preds = torch.zeros(3, B, dtype=torch.int32, device=dev)

    def _forward(self, static, time, labels, training: bool, with_grad: bool, prologue: bool = False):
        B, D = self.B, self.D
        sd = self.drop_step if training else None
        fs = self.Nf * D
        time_part = self.fused.view(-1)[D:]                 # tokens 1..Nt of every sample
        main, side, _ = self._streams(self._conc_fwd)
        head = None
        if prologue and side is main:
            # one stream: the step prologue rides in the input projection's launch, which then goes first (it reads none of the
            # counters; the static MLP draws its dropout masks from the bumped one)
            head = (self._head_adam(), self.drop_step, self.losses)
            self.e_time.forward(time, B, self.x0_time, step_head=head)
        elif prologue:
            self._prologue()
        ride = self._mlp_ride and side is main              # one stream: the MLP's workgroups ride in the time tower's token-mixing launch
        side.wait_stream(main)
        with torch.cuda.stream(side):                       # the static MLP beside the time tower: token 0 + its head's input
            (self.mlp.forward_ride if ride else self.mlp.forward)(static, B, self.fused, fs, self.pool_static, training, self.seed, 0, sd)
        if head is None:
            self.e_time.forward(time, B, self.x0_time)
        hp = self._heads_pool                               # the heads pool the two towers' outputs themselves (m2m_head.tokens)
        self.t_time.forward(self.x0_time, self.Nt * D, B, time_part, fs, None if hp else self.pool_time, training, self.seed, 0, sd)
        if ride:
            self.mlp.ride_flush()                           # (a launch of its own if no token launch took it)
        main.wait_stream(side)
        modal = training and self._modal                    # the modalities-only stage: no fusion tower
        if not modal:
            self.t_fus.forward(self.fused, fs, B, self.fus_out, fs, None if hp else self.pool_fus, training, self.seed, 0, sd)
        hw = self.head_weights
        heads = [self._head("static", self.pool_static, self.dpool_static, hw["static"], with_grad),
                 self._head("time", self.pool_time, self.dpool_time, hw["time"], with_grad),
                 self._head("fusion", self.pool_fus, self.dpool_fus, hw["fusion"], with_grad)]
        if hp:
            heads[1]["tokens"] = (time_part.data_ptr(), self.Nt, fs)
            heads[2]["tokens"] = (self.fus_out, self.Nf, fs)
        if modal:
            heads = heads[:2]                               # (their total lands in losses[2]: _stage_total)
        heads_ce(heads, labels, B, D, self.K, out=(self.logits, self.losses, self.preds), zero_losses=not training,
                 weights=self._pass_weights(training))
        self._stage_total(training)

    def _backward(self, static, time, fused_update: bool = False):
        B, D = self.B, self.D
        fs = self.Nf * D
        sd = self.drop_step
        if self._modal:
            # the modalities-only stage: the static MLP's and the time tower's backward from their heads' d_pooled alone (d_out
            # NULL), the time tower's and the projection's weight gradients as single calls -- on the main stream at any batch size
            self.mlp.backward(static, B, None, 0, self.dpool_static)
            self.t_time.backward(B, None, 0, self.dpool_time, self.dx0_time, self.Nt * D, self.seed, 0, sd)
            self.t_time.wgrad(B, self.seed, 0, sd)
            self.e_time.wgrad(time, self.dx0_time, B)
            if fused_update:
                self._update(1.0)
            return
        self.t_fus.backward(B, None, 0, self.dpool_fus, self.d_fused, fs, self.seed, 0, sd)
        if self._frozen:
            # stage two: the time tower's backward, the static MLP's (riding or not) and the projection's weight gradient are
            # skipped -- the existing single-tower forms cover what is left, on the main stream at any batch size
            self.t_fus.wgrad(B, self.seed, 0, sd)
            if fused_update:
                self._update(1.0)
            return
        d_time_part = self.d_fused.view(-1)[D:]
        if not (self._conc_bwd and self.concurrent) and self._merged_tail:
            # one stream (small batch): both towers' weight gradients in ONE launch, ONE Adam over the flat buffer, ONE re-pack
            # (seven launches less than the per-segment form the three-stream step needs)
            (self.mlp.backward_ride if self._mlp_ride else self.mlp.backward)(static, B, self.d_fused, fs, self.dpool_static)
            self.t_time.backward(B, d_time_part, fs, self.dpool_time, self.dx0_time, self.Nt * D, self.seed, 0, sd)
            if self._mlp_ride:
                self.mlp.ride_flush()
            if self._embed_wgrad_merged:
                towers_wgrad([self.t_fus, self.t_time], B, embeds=[self.e_time], inputs=[time], d_x0s=[self.dx0_time],
                             seed=self.seed, step=0, step_dev=sd)
            else:
                towers_wgrad([self.t_fus, self.t_time], B, seed=self.seed, step=0, step_dev=sd)
                self.e_time.wgrad(time, self.dx0_time, B)
            if fused_update:
                self._update(1.0)                       # one launch for small models (config_fused_update), else Adam + pack_all
            return
        main, s_b, s_f = self._streams(self._conc_bwd)
        s_b.wait_stream(main)
        s_f.wait_stream(main)
        with torch.cuda.stream(s_b):                        # static MLP: gradient of token 0 + of its own head
            self.mlp.backward(static, B, self.d_fused, fs, self.dpool_static)
            if fused_update:
                self._adam(*self.segments["static"], 1.0)
        with torch.cuda.stream(s_f):
            self.t_fus.wgrad(B, self.seed, 0, sd)
            if fused_update:
                self._adam(*self.segments["fusion"], 1.0)
                self.t_fus.pack(force=True)
        self.t_time.backward(B, d_time_part, fs, self.dpool_time, self.dx0_time, self.Nt * D, self.seed, 0, sd)
        self.t_time.wgrad(B, self.seed, 0, sd)
        self.e_time.wgrad(time, self.dx0_time, B)
        if fused_update:
            self._adam(*self.segments["time"], 1.0)
            self.t_time.pack(force=True)
            self.e_time.pack(force=True)
        main.wait_stream(s_b)
        main.wait_stream(s_f)

    def _stage_packs(self) -> list:
        # (the static MLP reads the fp32 masters: no packed copies)
        return [self.t_fus] if self._frozen else [self.t_time, self.e_time]

    def _eval_outputs(self) -> dict:
        return {"logits": self.logits[2], "logits_static": self.logits[0], "logits_time": self.logits[1],
                "loss_static": self.losses[0], "loss_time": self.losses[1], "loss_fusion": self.losses[2],
                "loss": self.losses[3], "preds": self.preds[2]}
