#!/usr/bin/env python
"""Launch trace of the fused engines: every call into libm2mixer.so of one configuration, one line per call, then sha256 of the
buffers the steps leave behind.  The tool a change of the Python host layer (engine.py, runtime.py) is verified with: two trees
whose traces and hashes agree enqueue the same work with the same arguments.

    python scripts/launch_trace.py --model avmnist_B --precision bf16 --batch 512 [--scenario base|stages|feed|epochs]
                                   [--fusion SumFusion] [--out trace.txt] [--dump buffers.pt]
    PYTHONPATH=<another tree> M2M_LIB_PATH=<this tree's libm2mixer.so> python scripts/launch_trace.py ...    (the other side)

The M2M_* switches under test come from the environment.  Every function of _lib.SIGNATURES is wrapped on the loaded CDLL.  A
line holds the symbol, every scalar passed by value, every scalar inside a struct (or array of structs, or array of scalars) the
call points to, and the status the call returned; array lengths are taken from the count argument include/m2mixer.h names.
Pointers are reduced to NULL / set, or to `flat_p+<element offset>` (flat_g, flat_m, flat_v) when they point into one of the
engine's four flat buffers.  Left out: the plan bytes of m2m_adam_pack_all (the layout is private to the library; the plan is
written by m2m_adam_pack_plan_ranges, whose arguments are traced in full, so it is a function of traced values and pointers).

One invocation runs one scenario (--scenario) on engines built from tests/golden/gen_util.py configs with seeded batches and
load_state_dict(seeded make_params):
  base    (the default; its output has not changed since the tool exists, old records stay comparable) two fused_step,
          forward_backward + optimizer_step(1.0), train_step(grad_sync=lambda g: 1.0), train_step(grad_sync=
          PipelinedGradSync()), evaluate, capture() + two replays, sibling(B - 3) + one train_step on it.  Only names that exist
          since the engines have siblings and the pipelined exchange are used.
  stages  two fused_step, capture() + one replay, sibling(B - 3), freeze_modalities(), two fused_step, forward_backward +
          optimizer_step(1.0), capture() + two replays, a sibling built after the freeze + one step on it, evaluate; then on a
          fresh engine one fused_step, train_modalities_only(), two fused_step, probe(), capture() + one replay, evaluate,
          clone() + one fused_step on the clone.
  feed    an engine with scores=True (rank_scores=True where the class builds ranking buffers): an EpochFeed over 2 * B + 5
          seeded rows, the tail's training sibling, capture_feed(steps=2), start(order), one replay, a fed step on the sibling,
          feed.read(), evaluate into the tables of "val"; then on a fresh engine freeze_modalities(), a feed with muting=True,
          start(order, muting=codes), capture_feed(steps=1), two replays.
  epochs  whole passes through the drivers above the engine, on 5 * B + 3 seeded rows and an engine with scores=True (and
          rank_scores=True): prepare_tail_engine, capture() + run_epoch(train=True, replay=), run_epoch(train=False) on "train" and
          "val" (these three on the models with class predictions), capture_feed(steps=2) + run_epoch_fed(train=True),
          capture_feed_eval(steps=2, scores=, rank=, record=) + run_epoch_fed(train=False, record=), run_epoch_fed(probe=True),
          GradBlend(epochs=1).get_weights(), then a task module (tests/test_gpu_engine_backed.make_net) bound with scores=True,
          test_record=True: training_step, validation_step and test_step at batch B and at batch 3.  The hash block adds the
          splits' tables, ranking and record state, the record's rows, the returned metrics and GradBlend's twelve sums.
A scenario's second engine (and a clone) has flat buffers of its own: from its construction on pointers are named after those
(the clone's as clone.flat_p+<offset>).  The sha256 block holds, per engine of the scenario, the seven buffers of the base
scenario (+ `uncertainty` on the evidential engine) and what the scenario adds: score tables, ranking state, the feed's state,
accumulators and muting state.  stages and feed use names that exist since GradBlend (probe, clone, train_modalities_only),
epochs names that exist since capture_feed_eval and the prediction record.
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
    "m2m_heads_edl": {0: 1}, "m2m_feed_gather": {0: 1}, "m2m_feed_gather_muted": {0: 1},
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
        self.out, self.flat, self.pending, self.held = out, None, [], []

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

    def hold(self):
        """Queue what follows until the next set_flat: an engine with flat buffers of its own is about to be built."""
        self.held, self.flat = self.flat, None

    def set_flat(self, eng, tag="", keep=False):
        """Name `eng`'s flat buffers (`tag` in front) and write out what was queued; keep: beside the ones named before hold()."""
        self.flat = (self.held if keep else []) + [(tag + k, getattr(eng, k).data_ptr(), getattr(eng, k).numel() * 4)
                                                   for k in ("flat_p", "flat_g", "flat_m", "flat_v")]
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


def build(args, **kw):
    name, dev = args.model, torch.device("cuda:0")
    if name == "avmnist_uq":
        cfg, cls, shapes_of, batch_of = dict(G.AVMNIST["S"]), E.AVMnistUQEngine, E.avmnist_param_shapes, G.avmnist_batch
    elif name.startswith("avmnist_"):
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
    eng = cls(cfg, args.batch, device=dev, precision=args.precision, init=False, **kw)
    params = G.make_params(shapes_of(cfg), args.seed)
    rows = lambda n, seed: tuple(t.to(dev) for t in batch_of(n, seed, cfg))       # n seeded samples, as the engine's batch
    return eng, params, rows(args.batch, args.seed + 1), rows


ENGINE_BUFFERS = ("flat_p", "flat_m", "flat_v", "flat_g", "losses", "logits", "preds")


def engine_buffers(eng, tag=""):
    """The buffers a scenario hashes for one engine, on the host: the seven of the base scenario, `uncertainty` where it exists."""
    keys = ENGINE_BUFFERS + (("uncertainty",) if hasattr(eng, "uncertainty") else ())
    return {tag + k: getattr(eng, k).detach().cpu() for k in keys}


def captured(rec, eng, batch, replays, what="capture"):
    """capture() + `replays` replays, then the graph is let go (a training sibling may narrow the kept gradient ranges)."""
    rec.emit("# " + what)
    replay = eng.capture(*batch)
    for i in range(replays):
        rec.emit(f"# replay {i}")
        replay(*batch)
    torch.cuda.synchronize()
    eng.release_capture()


def scenario_base(rec, args):
    phase = lambda s: rec.emit("# " + s)
    phase("construct")
    eng, params, batch, _ = build(args)
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
    captured(rec, eng, batch, 2)
    phase(f"sibling({args.batch - 3})")
    nb = args.batch - 3
    sib = eng.sibling(nb)
    phase("sibling train_step")
    sib.train_step(*(t[:nb].contiguous() for t in batch))
    torch.cuda.synchronize()
    return {k: getattr(eng, k).detach().cpu() for k in ENGINE_BUFFERS}


def scenario_stages(rec, args):
    """Both training stages, each on an engine of its own: the stage entered with a sibling alive and a graph captured, eager and
    captured staged steps, engines built after the stage was entered, evaluate, probe() and clone()."""
    phase = lambda s: rec.emit("# " + s)
    cut = lambda batch, n: tuple(t[:n].contiguous() for t in batch)
    phase("construct")
    eng, params, batch, _ = build(args)
    rec.set_flat(eng)
    phase("load_state_dict")
    eng.load_state_dict(params)
    for i in range(2):
        phase(f"fused_step {i}")
        eng.fused_step(*batch)
    captured(rec, eng, batch, 1)
    phase(f"sibling({args.batch - 3})")
    before = eng.sibling(args.batch - 3)                         # alive at the freeze: it re-enters the stage with the engine
    phase("freeze_modalities")
    eng.freeze_modalities()
    for i in range(2):
        phase(f"frozen fused_step {i}")
        eng.fused_step(*batch)
    phase("frozen forward_backward + optimizer_step(1.0)")
    eng.forward_backward(*batch)
    eng.optimizer_step(1.0)
    captured(rec, eng, batch, 2, "frozen capture")
    nb = args.batch - 5
    phase(f"frozen sibling({nb})")
    after = eng.sibling(nb)
    phase("frozen sibling fused_step")
    after.fused_step(*cut(batch, nb))
    phase("frozen evaluate")
    eng.pack()                                                   # (the sibling's step changed the weights)
    eng.evaluate(*batch)
    torch.cuda.synchronize()
    bufs = engine_buffers(eng)
    del eng, before, after

    rec.hold()
    phase("construct (modalities-only)")
    eng, params, batch, _ = build(args)
    rec.set_flat(eng)
    phase("load_state_dict")
    eng.load_state_dict(params)
    phase("fused_step")
    eng.fused_step(*batch)
    phase("train_modalities_only")
    eng.train_modalities_only()
    for i in range(2):
        phase(f"modal fused_step {i}")
        eng.fused_step(*batch)
    phase("probe")
    eng.probe(*batch)
    captured(rec, eng, batch, 1, "modal capture")
    phase("modal evaluate")
    eng.evaluate(*batch)
    rec.hold()
    phase("clone")
    twin = eng.clone()
    rec.set_flat(twin, "clone.", keep=True)
    phase("clone fused_step")
    twin.fused_step(*batch)
    torch.cuda.synchronize()
    bufs.update(engine_buffers(eng, "modal."))
    bufs.update(engine_buffers(twin, "clone."))
    return bufs


def feed_buffers(eng, feed, tag=""):
    """What a fed scenario adds to the hashed buffers: the training score table and ranking state, the feed's state, its
    accumulators (`_acc`, as its two views: float64 sums, int64 counts) and its muting state."""
    out = {}
    if eng.scores is not None:
        out[tag + "scores"] = eng.scores.table
    if eng.rank is not None:
        out[tag + "rank_state"] = eng.rank.state
    out.update({tag + "feed_state": feed.state, tag + "feed_sums": feed.sums, tag + "feed_counts": feed.counts})
    if feed.mute_state is not None:
        out[tag + "feed_mute_state"] = feed.mute_state
    return {k: t.detach().cpu() for k, t in out.items()}


def scenario_feed(rec, args):
    """Steps that feed themselves (EpochFeed, capture_feed) on an engine with count tables (and ranking buffers where the class
    builds them), the ragged tail's sibling, evaluation into a split's table; then a muted feed on a frozen engine.  The tail's
    training sibling is built before capture_feed, as sibling() demands, and takes its fed step after the replay."""
    phase = lambda s: rec.emit("# " + s)
    B, tail = args.batch, 5
    n = 2 * B + tail                                             # two full batches and the ragged tail
    ranks = args.model not in ("avmnist_uq", "mmimdb")           # (these two refuse rank_scores=True)
    order = torch.randperm(n, generator=torch.Generator().manual_seed(args.seed + 3))
    phase("construct")
    eng, params, batch, rows = build(args, scores=True, rank_scores=ranks)
    rec.set_flat(eng)
    phase("load_state_dict")
    eng.load_state_dict(params)
    sources = rows(n, args.seed + 2)
    phase("EpochFeed")
    feed = E.EpochFeed(sources, B, eng.device)
    phase(f"sibling({tail})")
    tail_eng = eng.sibling(tail)
    phase("capture_feed(steps=2)")
    replay = eng.capture_feed(feed, steps=2)
    phase("start(order)")
    feed.start(order)
    phase("replay")
    replay()
    phase("tail: fed step on the sibling")
    tslots = feed.new_slots(tail)
    tail_eng.pack()
    feed.gather_into(tslots)
    tail_eng.train_step(*tslots)
    eng.pack()
    feed.accumulate(tail_eng, tslots[-1])
    phase("feed.read")
    feed.read()
    feed.check()
    phase("evaluate into the tables of 'val'")
    extra = {"rank": eng.rank_buffer("val")} if ranks else {}
    eng.evaluate(*batch, scores=eng.score_table("val"), **extra)
    torch.cuda.synchronize()
    bufs = engine_buffers(eng)
    bufs.update(feed_buffers(eng, feed))
    bufs["scores_val"] = eng.score_table("val").table.cpu()
    if ranks:
        bufs["rank_val_state"] = eng.rank_buffer("val").state.cpu()
    del eng, tail_eng, feed, replay

    rec.hold()
    phase("construct (frozen, muted feed)")
    eng, params, batch, rows = build(args)
    rec.set_flat(eng)
    phase("load_state_dict")
    eng.load_state_dict(params)
    phase("freeze_modalities")
    eng.freeze_modalities()
    phase("EpochFeed(muting=True)")
    feed = E.EpochFeed(sources, B, eng.device, muting=True)
    phase("start(order, muting=codes)")
    feed.start(order, muting=torch.tensor([1, 0, 2]))            # one code per step of the epoch: ceil(n / B) = 3
    phase("capture_feed(steps=1)")
    replay = eng.capture_feed(feed, steps=1)
    for i in range(2):
        phase(f"replay {i}")
        replay()
    torch.cuda.synchronize()
    feed.check()
    bufs.update(engine_buffers(eng, "muted."))
    bufs.update(feed_buffers(eng, feed, "muted."))
    return bufs


def scenario_epochs(rec, args):
    """Whole passes over a split through every driver of the host layer (data.run_epoch / run_epoch_fed, gradblend.GradBlend, a
    bound task module's step hooks) on n = 5 * B + 3 seeded rows: feed_plan(n, B, 2) is 2 replays, 1 single step and a tail of 3."""
    from m2_mixer_amd import data as D
    from m2_mixer_amd.gradblend import GradBlend
    phase = lambda s: rec.emit("# " + s)
    B, tail = args.batch, 3
    n = 5 * B + tail
    task = args.model.split("_")[0]
    ranks = task != "mmimdb"                                     # (MM-IMDb refuses rank_scores=True ...
    classes = task != "mmimdb"                                   # ... and run_epoch's hit counts take class predictions)
    order = torch.randperm(n, generator=torch.Generator().manual_seed(args.seed + 3))
    phase("construct")
    eng, params, batch, rows = build(args, scores=True, rank_scores=ranks)
    rec.set_flat(eng)
    phase("load_state_dict")
    eng.load_state_dict(params)

    class Resident(D.ResidentTensors):                           # run_epoch iterates batches(); the tensors are any task's
        batches = D.ResidentAVMnist.batches

    data = Resident({"train": rows(n, args.seed + 2), "val": rows(n, args.seed + 4)})
    phase("prepare_tail_engine")
    D.prepare_tail_engine(eng, data, "train", B)
    out = {}
    if classes:
        phase("capture")
        replay = eng.capture(*batch)
        phase("run_epoch(train=True, replay)")
        out["run_epoch train"] = D.run_epoch(eng, data, "train", B, train=True, replay=replay)
        for split in ("train", "val"):
            phase(f"run_epoch(train=False) on {split!r}")
            out[f"run_epoch eval {split}"] = D.run_epoch(eng, data, split, B, train=False)
    phase("EpochFeed")
    feed = E.EpochFeed(data.splits["train"], B, eng.device)
    phase("capture_feed(steps=2)")
    fed = eng.capture_feed(feed, steps=2)
    phase("run_epoch_fed(train=True)")
    out["fed train"] = D.run_epoch_fed(eng, feed, fed, train=True, order=order)
    record = eng.prediction_record("val", n)
    accs = {"scores": eng.score_table("val"), "rank": eng.rank_buffer("val") if ranks else None, "record": record}
    phase("capture_feed_eval(steps=2, scores=, rank=, record=)")
    fed_eval = eng.capture_feed_eval(feed, steps=2, **accs)
    phase("run_epoch_fed(train=False, record=)")
    out["fed eval"] = D.run_epoch_fed(eng, feed, fed_eval, train=False, split="val", record=record)
    torch.cuda.synchronize()
    bufs = engine_buffers(eng)
    bufs.update(feed_buffers(eng, feed))
    for split in ("train_eval", "val") if classes else ("val",):
        bufs[f"scores_{split}"] = eng.score_table(split).table.cpu()
        if ranks:
            bufs[f"rank_{split}_state"] = eng.rank_buffer(split).state.cpu()
    bufs["record_val_state"] = record.state.cpu()
    bufs.update({"record_val_" + k: v for k, v in record.read().items()})
    phase("run_epoch_fed(train=False, probe=True)")
    out["fed probe"] = D.run_epoch_fed(eng, feed, None, train=False, probe=True, split="val")
    bufs.update(feed_buffers(eng, feed, "probe."))
    phase("GradBlend(epochs=1).get_weights")
    gb = GradBlend(eng, data, epochs=1, seed=args.seed + 5)
    gb.get_weights()
    bufs["gradblend_sums"] = torch.tensor([[gb.sums[h][k] for k in sorted(gb.sums[h])] for h in eng.HEAD_NAMES], dtype=torch.float64)
    for k, d in out.items():                                     # the returned metrics, as one float64 row per pass
        bufs["metrics " + k] = torch.tensor([float(d[key]) for key in sorted(d)], dtype=torch.float64)
        rec.emit(f"# keys {k}: {' '.join(sorted(d))}")

    sys.path.append(os.path.join(ROOT, "tests"))
    from test_gpu_engine_backed import make_net
    rec.hold()
    phase("module: make_net + bind_engine(scores=True, test_record=True)")
    net, _ = make_net(task, eng.cfg, args.seed + 6, eng.device)
    net.bind_engine(B, precision=args.precision, scores=True, rank_scores=ranks, test_record=True)
    rec.set_flat(net.engine, "net.", keep=True)
    names = {"avmnist": ("image", "audio", "label"), "mmimdb": ("image", "text", "label")}.get(task)
    for nb in (B, tail):
        mb = tuple(t[:nb].contiguous() for t in batch)
        mb = mb if names is None else dict(zip(names, mb))
        for hook in ("training_step", "validation_step", "test_step"):
            phase(f"module {hook} at batch {nb}")
            getattr(net, hook)(mb, 0)
    torch.cuda.synchronize()
    bufs.update(engine_buffers(net.engine, "net."))
    for split in ("train", "val", "test"):
        bufs[f"net.scores_{split}"] = net.engine.score_table(split).table.cpu()
        if ranks:
            bufs[f"net.rank_{split}_state"] = net.engine.rank_buffer(split).state.cpu()
    bufs["net.record_test_state"] = net.engine.prediction_record("test").state.cpu()
    return bufs


SCENARIOS = {"base": scenario_base, "stages": scenario_stages, "feed": scenario_feed, "epochs": scenario_epochs}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", required=True, help="avmnist_S | avmnist_M | avmnist_B | avmnist_uq | mmimdb | mimic")
    ap.add_argument("--scenario", default="base", choices=sorted(SCENARIOS), help="the sequence of engine calls to trace")
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
    bufs = SCENARIOS[args.scenario](rec, args)
    rec.emit("# sha256")
    for k, t in bufs.items():
        out.write(f"sha256 {k} {hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()}\n")
    out.flush()
    if args.dump:
        torch.save(bufs, args.dump)


if __name__ == "__main__":
    main()
