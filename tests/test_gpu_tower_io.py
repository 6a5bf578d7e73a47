"""The I/O contract of the tower entry points (-m gpu; include/m2mixer.h: m2m_tower_forward / _backward, m2m_towers_forward /
_backward, m2m_tower_wgrad), clause by clause, on every execution path: fused, wide and column-split, single towers and the
two-tower launches of each (tests/tower_io_cases.py; tests/test_host_tower_io.py shows on the CPU that the inputs make the
clauses sharp).

  1. sample strides: strided buffers whose padding holds the index-carrying NaN of nan_fill -- in the pair cases the
     ConcatFusion layout, both towers writing the halves of one (B, Na + Nb, D) buffer and reading d_out from one -- give
     results within the bars of float64, leave every pad word bit-identical, and out / pooled / d_x0 are BIT-EQUAL to the same
     call on dense buffers (no atomics touch these three on any path: only addresses differ between the runs);
  2. pooled: the float64 token mean with a buffer; with NULL the same bits in out and nothing written;
  3. upstream gradients: d_out, d_pooled, both, neither (zero d_x0, every gradient keeps its value);
  4. parameter gradients accumulate onto a pre-fill G0, d_x0 is written; M2M_WGRAD_OVERWRITE writes the channel-mixing three;
  5. inputs given as 2..4 parts; more (and any on a wide pair) refused with nothing written;
  6. training == 0 switches dropout off, whatever the step;
  7. what the calls refuse before launching anything: a tower of no blocks, NULL / unaligned buffers, short or odd strides.

(In the ConcatFusion layout `out` has no pad words of its own -- the other tower's half is the padding: there the fused buffer
must come back written in full, each half within the bars and bit-equal to the dense call; x0 and d_x0 keep their NaN pads.)

Inputs: tower_io_cases.draw at the tower's seed, the first whose float64 reference meets the conditions of
tests/test_host_tower_io.py.  One of them is the reference's own conditioning: at its base seed the one-token tower of
fused_pair_tiles missed the bf16 bar on token_mix.2.net.3.weight (5.98e-2 of the tensor's maximum with d_out alone, 3.0e-2
with both upstream gradients, against 4e-2; 1.9e-6 in fp32 on the same launch), and rounding the OPERANDS of the float64
oracle's products to bf16 moves that reference tensor by 2.6e-2 by itself: behind a LayerNorm the gradient of a token row sums
to zero over the hidden units, so most of what the token MLP's gradients add up cancels, and the rounding does not.

Reference: the oracle in float64 on the CPU.  Bars: the project's (tests/test_gpu_shape_envelope.py), relative to the reference
tensor's maximum.  Every error is recorded under "tower io <path> <prec> <tensor>" (conftest.observe).
"""
import ctypes as C

import pytest
import torch

import tower_io_cases as IO
from conftest import observe
from test_gpu_shape_envelope import BF16_GRAD_REL, BF16_REL, FP32_REL, dev, rel, tensor_class  # noqa: F401
from test_gpu_split_envelope import SEED, PairTower, nan_fill

pytestmark = pytest.mark.gpu

PAD = 8                                     # floats behind every sample of a strided buffer (a multiple of 4: float4 moves)
PADS = dict(x0=PAD, out=PAD, d_out=PAD, d_x0=PAD)
STEP = 3
ids = lambda pairs: [f"{n}-{p}" for n, p in pairs]


# ---- the driver -------------------------------------------------------------------------------------------------------------
def use_path(name, monkeypatch):
    """The switch the case's path needs (M2M_SPLIT=1 forces the column-split path; unset it is off at these batch sizes)."""
    monkeypatch.delenv("M2M_SPLIT_MIN_ROWS", raising=False)
    if IO.PATHS[name][0] == "split":
        monkeypatch.setenv("M2M_SPLIT", "1")
    else:
        monkeypatch.delenv("M2M_SPLIT", raising=False)


def build(name, prec, dev, pads=None, parts=(1, 1), pooled=True, up="both", p=0.0, concat=False):
    """The towers of a case on their inputs (tower_io_cases.draw).  concat: a pair's out and d_out are the halves of one
    (B, Na + Nb, D) buffer each (ConcatFusion): sample stride (Na + Nb) D, tower b's base pointer offset by Na D."""
    towers = []
    for i, (tow, ln) in enumerate(IO.towers_of(name)):
        inputs = IO.draw(tow, ln, IO.seed_of(name, i))
        towers.append(PairTower(tow._replace(p=p), 0, 1024 * i, dev, parts=parts[i], pooled=pooled, has_final_ln=ln, prec=prec,
                                pads=pads, inputs=inputs, up=up))
    if concat:
        a, b = towers
        B, D, Na, Nb = a.tow.B, a.tow.D, a.tow.N, b.tow.N
        out = torch.zeros(B, Na + Nb, D, device=dev)
        nan_fill(out)
        d_out = torch.cat([a.d_out, b.d_out], 1).to(dev)
        for t, sl in ((a, slice(0, Na)), (b, slice(Na, Na + Nb))):
            t.out, t.out_ss, t.d_out_dev, t.d_out_ss = out[:, sl], (Na + Nb) * D, d_out[:, sl], (Na + Nb) * D
            assert t.out.data_ptr() == out.data_ptr() + 4 * sl.start * D
        a.concat = b.concat = out
    assert_path(name, towers)
    return towers


def assert_path(name, towers, training=True):
    """No case silently takes another path: the library's own answers against the table."""
    from m2_mixer_amd.runtime import can_group
    path, kind = IO.PATHS[name]
    B = towers[0].tow.B
    rts = [t.rt for t in towers]
    assert len(rts) == (1 if kind == "single" else 2)
    assert all(rt.wide == (path == "wide") for rt in rts)
    form = rts[0].split_form(B, training, rts[1] if len(rts) == 2 else None)
    assert (form >= 2) == (path == "split") and form == (2 if path == "split" else 0), form
    if kind == "pair":
        assert can_group(*rts, B) and IO.can_group_wide(towers[0].tow, towers[1].tow, B) == (path == "wide")
        assert IO.can_group(towers[0].tow, towers[1].tow) == (path != "wide")


def forward(towers, step=STEP, training=True):
    from m2_mixer_amd.runtime import towers_forward
    B = towers[0].tow.B
    if len(towers) == 1:
        t = towers[0]
        t.rt.forward(t.xdev, t.x_ss, B, t.out, t.out_ss, t.pool if t.pooled else None, training, SEED, step)
    else:
        towers_forward([t.rt for t in towers], [t.fwd_io() for t in towers], B, training, SEED, step)
    torch.cuda.synchronize()


def backward(towers, step=STEP):
    """The backward of the forward just run, then each tower's weight-gradient launch."""
    from m2_mixer_amd.runtime import towers_backward
    B = towers[0].tow.B
    if len(towers) == 1:
        towers[0].rt.backward(B, *towers[0].bwd_io(), SEED, step)
    else:
        towers_backward([t.rt for t in towers], [t.bwd_io() for t in towers], B, SEED, step)
    for t in towers:
        t.rt.wgrad(B, SEED, step)
    torch.cuda.synchronize()


class Bars:
    """Measures against float64 with the project's bars, records every error, names every miss."""

    def __init__(self, name, prec):
        self.label, self.prec, self.bad = f"tower io {IO.PATHS[name][0]} {prec}", prec, []
        self.act = FP32_REL if prec == "fp32" else BF16_REL
        self.grad = FP32_REL if prec == "fp32" else BF16_GRAD_REL

    def want(self, tensor, got, ref, tol, what, floor=0.0):
        if not bool(torch.isfinite(got).all()):
            self.bad.append(f"{what}: not finite (a pad or an unwritten word was consumed)")
            return
        err = rel(got, ref, floor)
        print(f"{self.label} {what}: {err:.3e} (bar {tol:.0e})")
        observe(f"{self.label} {tensor}", err, tol)
        if not err < tol:
            self.bad.append(f"{what}: {err:.3e} > {tol:.0e} (reference max {float(ref.abs().max()):.3e})")

    def acts(self, what, got, ref):
        self.want(what.split()[-1].split("[")[0], got, ref, self.act, what)       # recorded per tensor: out, pooled, d_x0

    def grads(self, t, ref_grads, what, minus=None):
        """Every parameter gradient of tower t (minus: the pre-fill G0 per key, subtracted in float64)."""
        for k, v in zip(t.keys, t.views):
            got = v.detach().double().cpu()
            if minus is not None and k in minus and bool(torch.isfinite(got).all()):
                got = got - minus[k]
            self.want(tensor_class(k), got, ref_grads[k], self.grad, f"{what} {k}", IO.grad_floor(k, ref_grads))

    def tower(self, t, ref, what, minus=None, pooled=True):
        self.acts(f"{what} out", t.out, ref["out"])
        if pooled:
            self.acts(f"{what} pooled", t.pool, ref["pooled"])
        self.acts(f"{what} d_x0", t.dx, ref["dx"])
        self.grads(t, ref["grads"], what, minus)

    def done(self):
        assert not self.bad, f"[{self.label}]: " + "; ".join(self.bad)


def prefill(t, ref_grads, nan_keys=()):
    """Gradients = G0 (NaN where the launch must write, not accumulate); d_x0 = NaN: it is written.  Returns {key: G0}."""
    g0 = {}
    for k, v in zip(t.keys, t.views):
        g0[k] = IO.g0_of(k, ref_grads)
        v.copy_(g0[k].float().to(v.device))
        if any(k.endswith(s) for s in nan_keys):
            v.fill_(float("nan"))
            del g0[k]
    t.dx.fill_(float("nan"))
    return g0


# ---- 1. strided buffers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", IO.CASE_PRECS, ids=ids(IO.CASE_PRECS))
def test_strided_buffers_leave_their_padding_alone(name, prec, dev, monkeypatch):
    use_path(name, monkeypatch)
    pair = IO.PATHS[name][1] == "pair"
    towers = build(name, prec, dev, pads=dict(x0=PAD, d_x0=PAD) if pair else PADS, concat=pair)
    forward(towers)
    backward(towers)
    bars = Bars(name, prec)
    for i, t in enumerate(towers):
        bars.tower(t, IO.reference(name, i, 1, "both"), f"strided[{i}]")
        for buf in ("x0", "out", "d_out", "d_x0"):
            assert t.pads_untouched(buf), f"tower {i}: a pad word of {buf} was written"
    if pair:
        assert bool(torch.isfinite(towers[0].concat).all()), "a word of the fused output buffer was left unwritten"
    # ---- the same call on dense buffers: only addresses differ
    dense = build(name, prec, dev)
    forward(dense)
    backward(dense)
    for i, (t, d) in enumerate(zip(towers, dense)):
        bars.grads(d, IO.reference(name, i, 1, "both")["grads"], f"dense[{i}]")
        for what, a, b in (("out", t.out, d.out), ("pooled", t.pool, d.pool), ("d_x0", t.dx, d.dx)):
            assert torch.equal(a, b), f"tower {i}: {what} of the strided call differs from the dense call"
    bars.done()


# ---- 2. pooled ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", IO.CASE_PRECS, ids=ids(IO.CASE_PRECS))
def test_pooled_is_the_token_mean_and_optional(name, prec, dev, monkeypatch):
    use_path(name, monkeypatch)
    towers = build(name, prec, dev)
    forward(towers)
    bars = Bars(name, prec)
    for i, t in enumerate(towers):
        ref = IO.reference(name, i, 1, "both")
        bars.acts(f"pooled[{i}]", t.pool, ref["pooled"])
        bars.acts(f"out[{i}]", t.out, ref["out"])
    with_pool = [t.out.clone() for t in towers]
    before = []
    for t in towers:
        t.pooled = False
        t.out.fill_(0)
        before.append(nan_fill(t.pool))
    forward(towers)
    for i, t in enumerate(towers):
        assert torch.equal(t.out, with_pool[i]), f"tower {i}: out depends on whether pooled is given"
        assert torch.equal(t.pool.view(torch.int32), before[i]), f"tower {i}: a buffer that was not given was written"
    bars.done()


# ---- 3. upstream gradient forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", IO.CASE_PRECS, ids=ids(IO.CASE_PRECS))
def test_upstream_gradient_forms(name, prec, dev, monkeypatch):
    use_path(name, monkeypatch)
    towers = build(name, prec, dev)
    bars = Bars(name, prec)
    for form in IO.FORMS:
        g0 = []
        for i, t in enumerate(towers):
            t.up_form = form
            t.reset()
            if form == "none":
                g0.append(prefill(t, IO.reference(name, i, 1, "both")["grads"]))
        forward(towers)                          # each form behind its own training forward, same seed and step
        backward(towers)
        for i, t in enumerate(towers):
            if form != "none":
                bars.tower(t, IO.reference(name, i, 1, form), f"{form}[{i}]", pooled=False)
                continue
            # a zero upstream gradient: d_x0 exactly zero, every gradient bit-unchanged or changed by +0.0 (values, not sign bits)
            assert bool((t.dx == 0).all()), f"tower {i}: d_x0 is not zero without an upstream gradient"
            for k, v in zip(t.keys, t.views):
                assert torch.equal(v.double().cpu(), g0[i][k]), f"tower {i}: {k} changed without an upstream gradient"
    bars.done()


# ---- 4. accumulation -----------------------------------------------------------------------------------------------------------
ACC = [(n, p) for n, p in IO.CASE_PRECS if n in IO.ACCUMULATE]
CH3 = ("channel_mix.1.net.0.weight", "channel_mix.1.net.0.bias", "channel_mix.1.net.3.weight")


@pytest.mark.parametrize("name,prec", ACC, ids=ids(ACC))
def test_parameter_gradients_accumulate_and_d_x0_is_written(name, prec, dev, monkeypatch):
    use_path(name, monkeypatch)
    towers = build(name, prec, dev)
    g0 = [prefill(t, IO.reference(name, i, 1, "both")["grads"]) for i, t in enumerate(towers)]
    forward(towers)
    backward(towers)
    bars = Bars(name, prec)
    for i, t in enumerate(towers):
        bars.tower(t, IO.reference(name, i, 1, "both"), f"G0[{i}]", minus=g0[i])
    bars.done()


def test_wgrad_overwrite_writes_the_channel_gradients(dev, monkeypatch):
    name, prec = "fused_n3", "bf16"
    use_path(name, monkeypatch)
    (t,) = build(name, prec, dev)
    assert t.rt.wgrad_groups(t.tow.B) == 1      # one row group: "=" is a plain store of the whole sum
    t.rt.set_wgrad_overwrite(True)
    ref = IO.reference(name, 0, 1, "both")
    g0 = prefill(t, ref["grads"], nan_keys=CH3)
    assert len(g0) == len(t.keys) - 3 * t.tow.nb
    forward([t])
    backward([t])
    bars = Bars(name, prec)
    bars.tower(t, ref, "overwrite", minus=g0)    # the three come back NaN-free and right; the small gradients still accumulate
    bars.done()


# ---- 5. input parts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [2, 3, 4])
@pytest.mark.parametrize("name", IO.PARTS_CASES)
def test_input_given_as_parts(name, parts, dev, monkeypatch):
    """Tower 0 takes its input as `parts` buffers (strided, NaN between the samples), tower 1 a plain input."""
    prec = "bf16"
    use_path(name, monkeypatch)
    towers = build(name, prec, dev, pads=dict(x0=PAD), parts=(parts, 1))
    assert towers[0].fwd_io()[5:] == (parts, towers[0].tow.B * (towers[0].tow.N * towers[0].tow.D + PAD))
    forward(towers)
    backward(towers)
    bars = Bars(name, prec)
    for i, t in enumerate(towers):
        bars.tower(t, IO.reference(name, i, parts if i == 0 else 1, "both"), f"parts {parts}[{i}]")
    bars.done()


def unchanged(towers, value):
    torch.cuda.synchronize()
    return all(bool((x == value).all()) for t in towers for x in (t.out, t.pool, t.dx, t.flat))


@pytest.mark.parametrize("name,parts,message", [("fused_pair", 5, "at most 4 input parts"), ("split_pair", 5, "at most 4 input parts"),
                                                ("wide_pair", 2, "k-split inputs are not supported")])
def test_too_many_input_parts_are_refused(name, parts, message, dev, monkeypatch):
    from m2_mixer_amd.runtime import towers_forward
    use_path(name, monkeypatch)
    towers = build(name, "bf16", dev)
    a, b = towers
    B, N, D = a.tow.B, a.tow.N, a.tow.D
    x = torch.zeros(parts, B, N, D, device=dev)            # (every part is there: the refusal is not what keeps the call in bounds)
    for t in towers:
        t.reset(-7.25)
    with pytest.raises(RuntimeError, match=message):
        towers_forward([a.rt, b.rt], [(x, N * D, a.out, a.out_ss, a.pool, parts, B * N * D), b.fwd_io()], B, True, SEED, STEP)
    assert unchanged(towers, -7.25)


# ---- 6. evaluation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IO.EVAL_CASES)
def test_evaluation_switches_dropout_off(name, dev, monkeypatch):
    prec = "bf16"
    use_path(name, monkeypatch)
    (t,) = build(name, prec, dev, p=0.5)
    assert t.rt.desc.p_drop == 0.5
    assert_path(name, [t], training=False)
    forward([t], step=STEP, training=False)
    bars = Bars(name, prec)
    ref = IO.reference(name, 0, 1, "both")                 # the oracle without dropout
    bars.acts("eval out", t.out, ref["out"])
    bars.acts("eval pooled", t.pool, ref["pooled"])
    first = t.out.clone()
    t.out.fill_(0)
    forward([t], step=STEP + 1, training=False)
    assert torch.equal(t.out, first), "the evaluation output depends on the dropout step"
    bars.done()


# ---- 7. what the calls refuse before they launch anything ---------------------------------------------------------------------------
def raw_forward(towers, x0, x0_ss, out, out_ss, pooled, descs=None, parts=(1, 0)):
    """m2m_tower_forward (one tower) / m2m_towers_forward (two) with tower 0's buffers given as raw pointers."""
    from m2_mixer_amd import _lib as L
    from m2_mixer_amd.runtime import _drop_tail
    B = towers[0].tow.B
    descs = descs or [t.rt.desc for t in towers]
    if len(towers) == 1:
        L.check(L.lib().m2m_tower_forward(C.byref(descs[0]), x0, x0_ss, B, out, out_ss, pooled, 1, *_drop_tail(SEED, STEP)), "tower_forward")
        return
    io = (L.TowerIO * 2)()
    io[0].x0, io[0].x0_ss, io[0].out, io[0].out_ss, io[0].pooled = x0, x0_ss, out, out_ss, pooled
    io[0].x0_parts, io[0].x0_part_stride = parts
    b = towers[1]
    io[1].x0, io[1].x0_ss, io[1].out, io[1].out_ss, io[1].pooled = b.xdev.data_ptr(), b.x_ss, b.out.data_ptr(), b.out_ss, b.pool.data_ptr()
    io[1].x0_parts = 1
    ptrs = (C.POINTER(L.Tower) * 2)(*[C.pointer(d) for d in descs])
    L.check(L.lib().m2m_towers_forward(ptrs, io, 2, B, 1, *_drop_tail(SEED, STEP)), "towers_forward")


def raw_backward(towers, d_out, d_out_ss, d_pooled, d_x0, d_x0_ss, descs=None):
    from m2_mixer_amd import _lib as L
    from m2_mixer_amd.runtime import _drop_tail
    B = towers[0].tow.B
    descs = descs or [t.rt.desc for t in towers]
    if len(towers) == 1:
        L.check(L.lib().m2m_tower_backward(C.byref(descs[0]), B, d_out, d_out_ss, d_pooled, d_x0, d_x0_ss, *_drop_tail(SEED, STEP)), "tower_backward")
        return
    io = (L.TowerGIO * 2)()
    io[0].d_out, io[0].d_out_ss, io[0].d_pooled, io[0].d_x0, io[0].d_x0_ss = d_out, d_out_ss, d_pooled, d_x0, d_x0_ss
    b = towers[1]
    io[1].d_out, io[1].d_out_ss, io[1].d_pooled, io[1].d_x0, io[1].d_x0_ss = b.d_out_dev.data_ptr(), b.d_out_ss, b.d_pool_dev.data_ptr(), b.dx.data_ptr(), b.dx_ss
    ptrs = (C.POINTER(L.Tower) * 2)(*[C.pointer(d) for d in descs])
    L.check(L.lib().m2m_towers_backward(ptrs, io, 2, B, *_drop_tail(SEED, STEP)), "towers_backward")


@pytest.mark.parametrize("name", ["fused_n3", "fused_pair"])
def test_arguments_the_kernels_cannot_take_are_refused(name, dev, monkeypatch):
    """Through the single-tower call and through the pair call; every buffer has PAD floats of slack behind each sample, so no
    argument sent here could leave its buffer even unrefused.  Nothing is launched: every output keeps its pre-fill."""
    from m2_mixer_amd import _lib as L
    use_path(name, monkeypatch)
    towers = build(name, "bf16", dev, pads=PADS)
    a = towers[0]
    B, ND = a.tow.B, a.tow.N * a.tow.D
    for t in towers:
        t.reset(-7.25)
    F = dict(x0=a.xdev.data_ptr(), x0_ss=a.x_ss, out=a.out.data_ptr(), out_ss=a.out_ss, pooled=a.pool.data_ptr())
    G = dict(d_out=a.d_out_dev.data_ptr(), d_out_ss=a.d_out_ss, d_pooled=a.d_pool_dev.data_ptr(), d_x0=a.dx.data_ptr(), d_x0_ss=a.dx_ss)
    refusals = [(F, k, None, f"{k} is NULL") for k in ("x0", "out")] + [(G, "d_x0", None, "d_x0 is NULL")]
    for args in (F, G):
        for k in args:
            if k.endswith("_ss"):
                refusals.append((args, k, ND - 4, f"{k.replace('_ss', '_sample_stride')} is smaller than N \\* D"))
                refusals.append((args, k, ND + 2, f"{k.replace('_ss', '_sample_stride')} is not a multiple of 4 floats"))
            else:
                refusals.append((args, k, args[k] + 4, f"{k} is not 16-byte aligned"))       # the base pointer one float on
    assert len(refusals) == 3 + 4 * 2 + 6
    for args, k, value, message in refusals:
        call = dict(args, **{k: value})
        with pytest.raises(RuntimeError, match="unsupported shape/argument.*" + message):
            (raw_forward if args is F else raw_backward)(towers, **call)
        assert unchanged(towers, -7.25), message
    if len(towers) == 2:                                   # (the single-tower call takes one input buffer)
        with pytest.raises(RuntimeError, match="x0_part_stride is not a multiple of 4 floats"):
            raw_forward(towers, **F, parts=(2, B * ND + 1))
        assert unchanged(towers, -7.25)
    # ---- a tower of no blocks: the descriptor by hand, every pointer of the real one in place
    none = L.Tower.from_buffer_copy(bytes(a.rt.desc))
    none.nblocks = 0
    descs = [none] + [t.rt.desc for t in towers[1:]]
    calls = [lambda: raw_forward(towers, **F, descs=descs), lambda: raw_backward(towers, **G, descs=descs),
             lambda: L.check(L.lib().m2m_tower_wgrad(C.byref(none), B, SEED, STEP, None, L.stream_ptr()), "tower_wgrad"),
             lambda: L.check(L.lib().m2m_pack_tower(C.byref(none), L.stream_ptr()), "pack_tower")]
    for call in calls:
        with pytest.raises(RuntimeError, match="unsupported shape/argument.*a tower of no blocks is not supported"):
            call()
        assert unchanged(towers, -7.25)
    assert int(L.lib().m2m_split_form(C.byref(none), None, B, 1)) == 0          # (the query: "no split", nothing launched)
    # ---- and the calls as they stand are taken: the refusals above are the arguments', not the case's
    for t in towers:
        t.reset()
    forward(towers)
    backward(towers)
    bars = Bars(name, "bf16")
    for i, t in enumerate(towers):
        bars.tower(t, IO.reference(name, i, 1, "both"), f"after the refusals[{i}]")
    bars.done()
