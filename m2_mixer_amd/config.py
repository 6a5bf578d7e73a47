"""Process-wide knobs of the HIP path."""
from __future__ import annotations

import os

from . import _lib as L

_state = {
    # "bf16": bf16 MFMA operands, fp32 accumulate / residual / LayerNorm  (the training + bench mode)
    # "fp32": exact fp32 MFMA (parity mode: tracks the reference CPU path to ~1e-5)
    "precision": os.environ.get("M2M_PRECISION", "bf16"),
    "seed": None,
    # dropout step counters of the MODULE path on the device (a captured hipGraph must not bake the step in: graphs.GraphedStep)
    "device_step": False,
}


# ---- environment switches ---------------------------------------------------------------------------------------------------
# Every M2M_* variable the Python package reads: name -> (default, when it is read, meaning).  Diagnostics: the defaults are the
# measured optimum.  A default of "1" is a default-on switch (off only for "0"), "0" a default-off one (on only for "1"); None:
# the default depends on the model (see the meaning).  INTEGRATION.md lists them beside the library's own switches
# (tests/test_host_switches.py keeps that list complete).
SWITCHES = {
    "M2M_PRECISION": ("bf16", "import of config", "bf16 / fp32: the precision of engines and modules built without an explicit one"),
    "M2M_LIB_PATH": (None, "import of _lib", "load another build of libm2mixer.so (default: the one beside the package)"),
    "M2M_DIST_BACKEND": (None, "parallel.init_from_env", "torch.distributed backend (default nccl on GPUs; gloo: several ranks on one GPU)"),
    "M2M_FUSED_UPDATE": (None, "engine construction", "1 / 0 force Adam + operand re-pack as one launch / as two; unset: one launch"),
    "M2M_CONCURRENT": ("1", "engine construction", "0: every launch on the main stream, no grouped two-tower launches"),
    "M2M_WGRAD_OVERWRITE": ("1", "engine construction", "weight gradients with a single owner are written, Adam leaves them uncleared"),
    "M2M_WGRAD_SLOT": ("1", "engine construction", "second row group of a grouped weight-gradient launch into a slot that Adam adds"),
    "M2M_EARLY_FUSION_WGRAD": ("0", "engine construction", "wide towers: the fusion tower's weight gradients on a side stream"),
    "M2M_HEADS_POOL": ("1", "engine construction", "wide towers: the heads launch pools the tower outputs itself"),
    "M2M_DEFER_SMALL": ("1", "engine construction", "the fusion backward's small-gradient slots are reduced by the weight-gradient launch"),
    "M2M_HEAD_SLOTS": ("1", "engine construction", "the heads' weight gradients through slots (bit-reproducible) instead of float atomics"),
    "M2M_GROUP_SLOTS": ("1", "engine construction", "the two-tower backward's small gradients through per-workgroup slots"),
    "M2M_EMBED_FAST": ("1", "engine construction", "patch-embedding weight gradients in the single-owner form (d_x0^T image)"),
    "M2M_EMBED_FOLD": ("0", "engine construction", "patch embeddings inside the two-tower forward launch"),
    "M2M_MIMIC_STREAMS": (None, "engine construction", "none / fwd / bwd / both: side streams of the MIMIC step; unset: none up to batch 1024, else both"),
    "M2M_MIMIC_MERGED_TAIL": ("1", "engine construction", "MIMIC on one stream: one weight-gradient launch, one Adam, one re-pack"),
    "M2M_MIMIC_EMBED_WGRAD_MERGED": ("1", "engine construction", "MIMIC merged tail: the input projection's weight gradient inside the towers' launch"),
    "M2M_MLP_RIDE": ("1", "engine construction", "MIMIC: the static MLP's workgroups ride in the time tower's token-mixing launches"),
    "M2M_CAPTURE_SHARE_SLOTS": ("0", "engine.capture()", "multi-step capture: every step reads the same input slot (diagnostic)"),
}


def switch(name: str, default=None):
    """The environment's value of a switch in SWITCHES NOW (so a test's monkeypatch.setenv before construction counts), else
    `default`, else the table's default."""
    return os.environ.get(name, SWITCHES[name][0] if default is None else default)


def switch_on(name: str) -> bool:
    """Boolean form: a default-on switch is off only for "0", a default-off switch is on only for "1"."""
    return switch(name) != "0" if SWITCHES[name][0] == "1" else switch(name) == "1"


def set_precision(name: str) -> None:
    if name not in L.PREC_BY_NAME:
        raise ValueError(f"precision must be one of {sorted(L.PREC_BY_NAME)}")
    _state["precision"] = name


def get_precision() -> str:
    return _state["precision"]


def prec_id(name: str | None = None) -> int:
    return L.PREC_BY_NAME[name or _state["precision"]]


def set_dropout_seed(seed: int) -> None:
    _state["seed"] = int(seed) & 0xFFFFFFFF


def dropout_seed() -> int:
    if _state["seed"] is None:
        import torch
        _state["seed"] = int(torch.initial_seed()) & 0xFFFFFFFF
    return _state["seed"]


def set_device_dropout_step(on: bool) -> None:
    """Module path: keep every tower's / MLP's dropout step counter in device memory (advanced by a tiny launch in front of the
    forward, read by the kernels) instead of passing a host integer.  Needed when a training step is captured into a hipGraph
    (m2_mixer_amd.graphs.GraphedStep turns it on): a host integer would be baked into the graph and every replay would draw the
    SAME dropout masks.  The mask stream is the same in both modes (step 1, 2, 3, ...).  Not re-entrant: a backward must run
    before the next forward of the same module (always true for shared_step -> backward -> optimizer.step)."""
    _state["device_step"] = bool(on)


def device_dropout_step() -> bool:
    return _state["device_step"]
