#!/usr/bin/env python
"""Launch trace of the fused engines: every call into libm2mixer.so of one configuration, one line per call, then sha256 of the
buffers the steps leave behind.  The tool a change of the Python host layer (engine.py, runtime.py) is verified with: two trees
whose traces and hashes agree enqueue the same work with the same arguments.

    python scripts/launch_trace.py --model avmnist_B --precision bf16 --batch 512 [--fusion SumFusion] [--out trace.txt]
                                   [--dump buffers.pt]
    PYTHONPATH=<another tree> M2M_LIB_PATH=<this tree's libm2mixer.so> python scripts/launch_trace.py ...    (the other side)

The M2M_* switches under test come from the environment.  Every function of _lib.SIGNATURES is wrapped on the loaded CDLL.  A
line holds the symbol, every scalar passed by value, every scalar inside a struct (or array of structs, or array of scalars) the
call points to, and the status the call returned; array lengths are taken from the count argument include/m2mixer.h names.
Pointers are reduced to NULL / set, or to `flat_p+<element offset>` (flat_g, flat_m, flat_v) when they point into one of the
engine's four flat buffers.  Left out: the plan bytes of m2m_adam_pack_all (the layout is private to the library; the plan is
written by m2m_adam_pack_plan_ranges, whose arguments are traced in full, so it is a function of traced values and pointers).

One invocation: construct the engine (tests/golden/gen_util.py configs, seeded batch), load_state_dict(seeded make_params), two
fused_step, forward_backward + optimizer_step(1.0), train_step(grad_sync=lambda g: 1.0), train_step(grad_sync=
PipelinedGradSync()), evaluate, capture() + two replays, sibling(B - 3) + one train_step on it.  Only names that exist since the
engines have siblings and the pipelined exchange are used.
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):       # appended: a tree named in PYTHONPATH wins
    if p not in sys.path:
        sys.path.append(p)

import torch  # noqa: E402

import gen_util as G  # noqa: E402
from m2_mixer_amd import _lib as L  # noqa: E402
from m2_mixer_amd import engine as E  # noqa: E402
from m2_mixer_amd import parallel  # noqa: E402

# symbol -> {index of an array argument: index of the count argument the header names for it}
COUNTS = {
    "m2m_pack_all": {0: 1, 2: 3},
    "m2m_tower_backward_heads": {2: 3},
    "m2m_towers_forward": {0: 2, 1: 2},
    "m2m_towers_forward_embeds_ok": {0: 1, 2: 1},
    "m2m_towers_forward_embeds": {0: 2, 1: 2, 3: 2, 4: 2},
    "m2m_towers_backward": {0: 2, 1: 2},
    "m2m_towers_wgrad": {0: 2, 1: 2, 3: 7, 4: 7, 5: 7, 6: 7},
    "m2m_towers_wgrad_heads": {0: 2, 1: 2, 3: 7, 4: 7, 5: 7, 6: 7, 12: 13},
    "m2m_towers_wgrad_tail": {0: 2, 1: 2, 3: 7, 4: 7, 5: 7, 6: 7, 12: 13},
    "m2m_embeds_wgrad_form": {0: 2, 1: 2},
    "m2m_wgrad_slot_groups": {0: 1},
    "m2m_adam_step_ranges": {13: 14},
    "m2m_embeds_wgrad": {0: 3, 1: 3, 2: 3},
    "m2m_embeds_forward": {0: 5, 1: 5, 2: 5, 3: 5, 4: 5},
    "m2m_heads_ce": {0: 1}, "m2m_heads_bce": {0: 1}, "m2m_heads_ce_w": {0: 1}, "m2m_heads_bce_w": {0: 1},
    "m2m_adam_pack_plan": {0: 1, 2: 3},
    "m2m_adam_pack_plan_ranges": {0: 1, 2: 3, 16: 17},
    "m2m_adam_pack_all": {0: 1, 2: 3},
}
# (symbol, argument index): host memory whose bytes are not traced
OPAQUE = {("m2m_adam_pack_all", 5), ("m2m_adam_pack_plan", 16), ("m2m_adam_pack_plan_ranges", 18)}


class Ptr:
    """A pointer value as it reaches the library, rendered once the flat buffers are known."""

    def __init__(self, v):
        self.v = int(v or 0)


def _is_ptr_type(t):
    return isinstance(t, type) and issubclass(t, C._Pointer)


def enc_value(v, ctype):
    """A ctypes VALUE (struct, array, scalar field) -> nested lists of python scalars and Ptr."""
    if ctype is C.c_void_p:
        return Ptr(v)
    if issubclass(ctype, C.Structure):
        return [(n, enc_value(getattr(v, n), t)) for n, t in ctype._fields_]
    if issubclass(ctype, C.Array):
        return [enc_value(v[i], ctype._type_) for i in range(ctype._length_)]
    return v                                                     # int / float fields arrive as python scalars


def enc_pointee(arg, target, count):
    """What a POINTER(target) argument points to: `count` elements (None: one)."""
    if arg is None:
        return Ptr(0)
    if isinstance(arg, C.Array):
        n = len(arg) if count is None else count
        if n > len(arg):
            return f"<count {n} exceeds the array's {len(arg)} elements>"
        return [enc_elem(arg[i], target) for i in range(n)]
    obj = getattr(arg, "_obj", None)                            # byref(x)
    if obj is None and isinstance(arg, C._Pointer):
        obj = arg.contents if arg else None
    if obj is None:
        return Ptr(arg if isinstance(arg, int) else 1)
    return enc_elem(obj, target)


def enc_elem(x, target):
    if _is_ptr_type(target):                                     # an element of a pointer array: a pointer to a descriptor
        return enc_value(x.contents, target._type_) if x else Ptr(0)
    if target is C.c_void_p:
        return Ptr(x.value if isinstance(x, C.c_void_p) else x)
    if isinstance(x, (C.Structure, C.Array)):
        return enc_value(x, target)
    return x.value if hasattr(x, "value") else x


def enc_arg(name, i, arg, ctype, args):
    if (name, i) in OPAQUE:
        return "<host plan>"
    if ctype is C.c_void_p:
        return Ptr(arg)
    if _is_ptr_type(ctype):
        cnt = COUNTS.get(name, {}).get(i)
        return enc_pointee(arg, ctype._type_, None if cnt is None else int(args[cnt]))
    if ctype is C.c_char_p:
        return arg
    return ctype(arg).value                                      # by value: as the library receives it (float32, uint32, ...)


class Recorder:
    def __init__(self, out):
        self.out, self.flat, self.pending = out, None, []

    def install(self):
        lib = L.lib()
        for name, (_, argtypes) in L.SIGNATURES.items():
            setattr(lib, name, self._wrap(name, getattr(lib, name), argtypes))

    def _wrap(self, name, fn, argtypes):
        def call(*args):
            rec = [enc_arg(name, i, a, t, args) for i, (a, t) in enumerate(zip(args, argtypes))]
            rc = fn(*args)
            self.emit((name, rec, rc))
            return rc
        return call

    def emit(self, item):
        if self.flat is None:
            self.pending.append(item)                            # (calls of the constructor: the flat buffers are not known yet)
            return
        if isinstance(item, str):
            self.out.write(item + "\n")
        else:
            name, rec, rc = item
            self.out.write(f"{name}({', '.join(self.fmt(r) for r in rec)}) -> {rc!r}\n")
        self.out.flush()

    def set_flat(self, eng):
        self.flat = [(k, getattr(eng, k).data_ptr(), getattr(eng, k).numel() * 4) for k in ("flat_p", "flat_g", "flat_m", "flat_v")]
        pending, self.pending = self.pending, []
        for item in pending:
            self.emit(item)

    def fmt(self, r):
        if isinstance(r, Ptr):
            if not r.v:
                return "NULL"
            for k, base, nbytes in self.flat:
                if base <= r.v < base + nbytes:
                    q, rem = divmod(r.v - base, 4)
                    return f"{k}+{q}" + (f".{rem}" if rem else "")
            return "set"
        if isinstance(r, tuple):
            return f"{r[0]}={self.fmt(r[1])}"
        if isinstance(r, list):
            return "[" + " ".join(self.fmt(x) for x in r) + "]"
        return repr(r)


def build(args):
    name, dev = args.model, torch.device("cuda:0")
    if name.startswith("avmnist_"):
        cfg = dict(G.AVMNIST[name.split("_")[1]])
        cls, shapes_of, batch_of = E.AVMnistEngine, E.avmnist_param_shapes, G.avmnist_batch
    elif name == "mmimdb":
        cfg, cls, batch_of = dict(G.MMIMDB), E.MMIMDBEngine, G.mmimdb_batch
        shapes_of = lambda c: E.two_tower_param_shapes(c, E.MMIMDBEngine.MODS)
    elif name == "mimic":
        cfg, cls, shapes_of, batch_of = dict(G.MIMIC_H), E.MimicEngine, E.mimic_param_shapes, G.mimic_batch
    else:
        raise SystemExit(f"unknown model {name}")
    if args.dropout is not None:
        cfg["dropout"] = args.dropout
    if args.fusion:
        mm = dict(cfg["multimodal"], fusion_function=args.fusion)
        if args.fusion == "BiModalGatedUnit":
            mm.update(mod1_in=mm["hidden_dim"], mod2_in=mm["hidden_dim"], out_size=mm["hidden_dim"])
        cfg["multimodal"] = mm
    eng = cls(cfg, args.batch, device=dev, precision=args.precision, init=False)
    params = G.make_params(shapes_of(cfg), args.seed)
    batch = tuple(t.to(dev) for t in batch_of(args.batch, args.seed + 1, cfg))
    return eng, params, batch


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", required=True, help="avmnist_S | avmnist_M | avmnist_B | mmimdb | mimic")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, required=True)
    ap.add_argument("--fusion", default=None, help="multimodal.fusion_function of a two-tower model")
    ap.add_argument("--dropout", type=float, default=None)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=None, help="file for the trace (default: stdout)")
    ap.add_argument("--dump", default=None, help="also torch.save the hashed buffers here (for a max-abs-difference comparison)")
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else sys.stdout
    rec = Recorder(out)
    rec.install()
    phase = lambda s: rec.emit("# " + s)

    phase("construct")
    eng, params, batch = build(args)
    rec.set_flat(eng)
    phase("load_state_dict")
    eng.load_state_dict(params)
    for i in range(2):
        phase(f"fused_step {i}")
        eng.fused_step(*batch)
    phase("forward_backward + optimizer_step(1.0)")
    eng.forward_backward(*batch)
    eng.optimizer_step(1.0)
    phase("train_step(grad_sync=lambda g: 1.0)")
    eng.train_step(*batch, grad_sync=lambda g: 1.0)
    phase("train_step(grad_sync=PipelinedGradSync())")
    eng.train_step(*batch, grad_sync=parallel.PipelinedGradSync())
    phase("evaluate")
    eng.evaluate(*batch)
    phase("capture")
    replay = eng.capture(*batch)
    for i in range(2):
        phase(f"replay {i}")
        replay(*batch)
    torch.cuda.synchronize()
    eng.release_capture()                                        # (a training sibling may narrow the kept gradient ranges)
    phase(f"sibling({args.batch - 3})")
    nb = args.batch - 3
    sib = eng.sibling(nb)
    phase("sibling train_step")
    sib.train_step(*(t[:nb].contiguous() for t in batch))
    torch.cuda.synchronize()
    phase("sha256")
    bufs = {k: getattr(eng, k).detach().cpu() for k in ("flat_p", "flat_m", "flat_v", "flat_g", "losses", "logits", "preds")}
    for k, t in bufs.items():
        out.write(f"sha256 {k} {hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()}\n")
    out.flush()
    if args.dump:
        torch.save(bufs, args.dump)


if __name__ == "__main__":
    main()
