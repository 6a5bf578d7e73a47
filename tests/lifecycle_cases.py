"""The state between launches on the module path: one plain table of event sequences.

The module path (m2_mixer_amd.modules / m2_mixer_amd.models: `shared_step` -> `backward` -> `optimizer.step()`) keeps packed
MFMA-operand copies of every block's channel-mixing weights (`w1n`, `w2c`, `w2tn`, `w1tc`, `ch_b1p`) and of the embedding weight
(`wn`) beside the parameters.  Whatever changes the parameters -- an eager optimizer, torch's fused optimizer (which leaves the
version counters alone), a replayed hipGraph (which runs no Python), a `.data` edit, a load_state_dict -- the next forward, in
whichever mode, must compute with the weights as they are at that moment.

tests/test_gpu_module_lifecycle.py runs every case in the precisions it names: after the update events, each observation event
checks the packed copies bit for bit against a fresh pack, and in fp32 the logits of every head against the float64 oracle at
the module's current state_dict (tests/lifecycle_ref.py holds that float64 side).  tests/test_host_lifecycle.py (CPU) checks the
reach of the table, the premise about torch's optimizers that the `adam_fused` cases rest on, and on the oracle alone that stale
packed tensors would show at the table's learning rates.

Fields:
  name     test id
  model    key of MODELS
  precs    precisions the case runs in ("fp32": all three checks; "bf16": the bit-equality check only)
  events   update and observation events, in order
  lr       Adam's learning rate (and the size of a `data_edit`).  1e-2 unless the case's stale distance -- how far the logits
           move when the packed tensors alone are taken from the weights of before the last update -- would otherwise stay under
           ten times the logits bar (the GPU test asserts that condition and reports the distance)
  p        dropout (0 everywhere: the oracle comparison needs no masks)

Update events -- each is one training step on a fresh batch, or one edit of every parameter:
  adam_foreach     eager torch.optim.Adam, foreach form: advances the parameters' version counters (control)
  adam_fused       eager torch.optim.Adam(fused=True): does not advance them
  graph_fused      one replay of a GraphedStep(..., fused=True)
  graph_foreach    one replay of a GraphedStep(..., fused=False): a replay advances no counter whichever form was captured
  data_edit        p.data.add_(...) on every parameter, then the documented invalidate_packs() (control)
  load_state_dict  another seeded parameter set (control)

Observation events -- each must see the weights as they are at that moment:
  eval             net.eval(), no_grad, shared_step(mode="val")
  train_nograd     net.train() under no_grad (an MC-dropout pass; dropout is 0 here)
  eval_grad        net.eval() with gradients enabled, then backward: the backward launches read `w2tn` / `w1tc`

GraphedStep takes dict batches: the graph events run on `avmnist` and `mmimdb` only (MIMIC's batch is a tuple).  Within a case
every update kind that steps has an optimizer of its own (torch fixes an Adam's form, and where its step count lives, at the
first step), created at the kind's first event; a graph kind's GraphedStep is constructed there too.
"""
from collections import namedtuple

Case = namedtuple("Case", "name model precs events lr p")

UPDATES = ("adam_foreach", "adam_fused", "graph_fused", "graph_foreach", "data_edit", "load_state_dict")
GRAPH_UPDATES = ("graph_fused", "graph_foreach")
SILENT_UPDATES = ("adam_fused", "graph_fused", "graph_foreach")     # the parameters change, their version counters do not
OBSERVATIONS = ("eval", "train_nograd", "eval_grad")

# the three small task modules of tests/test_gpu_parity.py (_model_cfg: AV-MNIST-S, MIMIC-H, MM-IMDb) with that test's batch sizes
# and parameter seeds, and one bare tower deeper than one descriptor holds (test_towers_deeper_than_one_descriptor)
MODELS = {
    "avmnist": dict(B=8, seed=11, dict_batch=True),     # conv embeddings, fused towers, FusionMixer
    "mimic": dict(B=6, seed=31, dict_batch=False),      # Linear embedding, wide time tower, static MLP
    "mmimdb": dict(B=3, seed=51, dict_batch=True),      # wide towers, BCE heads
    "deep": dict(B=5, seed=95, dict_batch=False,        # FusionMixer, 11 blocks = descriptors of 8 + 3, driven by a hand-written
                 N=8, cfg=dict(hidden_dim=32, token_dim=16, channel_dim=64, num_mixers=11)),   # fused-Adam step on y.square().sum()
}
TASKS = ("avmnist", "mimic", "mmimdb")

BOTH = ("fp32", "bf16")

# state-dict keys of the tensors the runtimes keep packed copies of: every block's channel-mixing W1, b1 and W2, the weight of the
# patch embedding (MLPMixer) / of the input projection (MLPMixerNoPatching)
PACKED_SUFFIXES = ("channel_mix.1.net.0.weight", "channel_mix.1.net.0.bias", "channel_mix.1.net.3.weight",
                   "to_patch_embedding.0.weight", "proj.weight")


def is_packed(key: str) -> bool:
    return key.endswith(PACKED_SUFFIXES)


def applies(update: str, model: str) -> bool:
    return MODELS[model]["dict_batch"] or update not in GRAPH_UPDATES


def _c(name, model, events, lr=1e-2, precs=BOTH, p=0.0):
    return Case(name, model, tuple(precs), tuple(events), lr, p)


CASES = []
for _m in TASKS:
    for _u in UPDATES:
        if applies(_u, _m):
            CASES.append(_c(f"{_m}_{_u}_x2_eval", _m, [_u, _u, "eval"]))
    # the second evaluation: constructing a GraphedStep restores the parameters with copy_(), which advances the version
    # counters, so the FIRST evaluation after construction re-packs whatever the replays do
    for _u in SILENT_UPDATES:
        if applies(_u, _m):
            CASES.append(_c(f"{_m}_{_u}_two_evals", _m, [_u, _u, "eval", _u, _u, "eval"]))
    # (after graph replays the other observation kinds come second for the same reason: `U, U, observation` alone would pass
    # on the strength of the constructor's copy_())
    for _u in ("adam_fused", "graph_fused"):
        if applies(_u, _m):
            _head = [_u, _u, "eval"] if _u in GRAPH_UPDATES else []
            CASES.append(_c(f"{_m}_{_u}_x2_train_nograd", _m, _head + [_u, _u, "train_nograd"]))
            CASES.append(_c(f"{_m}_{_u}_x2_eval_grad", _m, _head + [_u, _u, "eval_grad"]))
CASES += [
    _c("avmnist_mixed", "avmnist", ["graph_fused", "graph_fused", "eval", "adam_foreach", "eval", "graph_fused", "eval"]),
    _c("deep_adam_fused", "deep", ["adam_fused", "adam_fused", "eval", "adam_fused", "train_nograd", "adam_fused", "eval_grad"]),
]
del _m, _u, _head
