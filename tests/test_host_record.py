"""Prediction record, host side (no GPU): the entry point exists in the header, the binding and the built library; the numpy
restatement (tests/record_ref.py) by hand; the argument refusals of m2m_record_append, which validates before it touches a
device; PredictionRecord's key names and dtypes for the four tasks (hand-filled buffers on the CPU: read() is host code);
feed_plan's arithmetic for an evaluation pass."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import record_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_library_carry_the_record_entry_point():
    from m2_mixer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "m2mixer.h")).read()
    assert re.search(r"\bint\s+m2m_record_append\s*\(", hdr), "m2m_record_append is not declared in include/m2mixer.h"
    assert "m2m_record_append" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "m2m_record_append"), "m2m_record_append is not exported by the built library"
    assert int(re.search(r"#define M2M_RECORD_STATE_WORDS (\d+)", hdr).group(1)) == _lib.RECORD_STATE_WORDS == 4
    assert int(re.search(r"#define M2M_RECORD_MAX_SOURCES (\d+)", hdr).group(1)) == _lib.RECORD_MAX_SOURCES == 16
    res, args = _lib.SIGNATURES["m2m_record_append"]
    assert res is C.c_int and len(args) == 6 and args[0] == C.POINTER(_lib.FeedSrc) and args[3] is C.c_int64
    assert C.sizeof(_lib.FeedSrc) == 24                                    # {const void*, void*, int64_t}: m2m_feed_src, shared
    assert "record.hip" in open(os.path.join(ROOT, "m2_mixer_amd", "csrc", "Makefile")).read()
    assert "models/avmnist.py:382-398" in hdr                              # the reference lines the entry point replaces
    assert _lib.lib().m2m_abi_version() == 18 == _lib.ABI_VERSION          # a new entry point only
    assert int(re.search(r"#define M2M_ABI_VERSION (\d+)", hdr).group(1)) == 18


def test_record_ref_by_hand():
    """Cursor, capacity and the dropped count: three appends of 3 rows into 7."""
    cap, B = 7, 3
    fill = lambda: [np.full((cap + 2, 8), 0xAB, dtype=np.uint8), np.full((cap + 2, 4), 0xAB, dtype=np.uint8)]
    step = lambda i: [np.full((B, 8), i, dtype=np.uint8) + np.arange(B, dtype=np.uint8)[:, None] * 16,
                      np.full((B, 4), 100 + i, dtype=np.uint8)]
    dsts, state = fill(), np.zeros(4, dtype=np.uint32)
    for i in range(2):
        dsts, state = RR.append(dsts, step(i), state, cap)
    assert state.tolist() == [6, 0, 0, 0]
    assert dsts[0][:6, 0].tolist() == [0, 16, 32, 1, 17, 33] and (dsts[0][6:] == 0xAB).all()
    dsts, state = RR.append(dsts, step(2), state, cap)                     # straddles the capacity: one row written, two dropped
    assert state.tolist() == [9, 0, 0, 2]
    assert dsts[0][6, 0] == 2 and dsts[1][6, 0] == 102 and (dsts[0][7:] == 0xAB).all() and (dsts[1][7:] == 0xAB).all()
    dsts, state = RR.append(dsts, step(3), state, cap)                     # a full record: everything dropped, the cursor counts on
    assert state.tolist() == [12, 0, 0, 5] and dsts[0][6, 0] == 2
    a = np.arange(6, dtype=np.float32).reshape(2, 3)
    assert RR.raw(a).shape == (2, 12) and RR.raw(a).view(np.float32).tolist() == a.tolist()


def _err(lib):
    return lib.m2m_last_error().decode("utf-8", "replace")


def test_append_refuses_bad_arguments_before_any_launch():
    """Every refusal returns -1 with a message; the pointers below are never dereferenced on a device (validation comes first)."""
    from m2_mixer_amd import _lib as L
    lib = L.lib()
    fake = 0x1000                                       # a non-NULL, 16-byte aligned address that is only ever compared

    def src(n=1, **kw):
        d = (L.FeedSrc * n)()
        for x in d:
            x.src, x.dst, x.row_bytes = fake, fake, 16
        for k, v in kw.items():
            setattr(d[0], k, v)
        return d

    f = lib.m2m_record_append
    cases = [("NULL srcs", lambda: f(None, 1, 4, 64, fake, 0), "srcs and state"),
             ("NULL state", lambda: f(src(), 1, 4, 64, 0, 0), "srcs and state"),
             ("nsrc 0", lambda: f(src(), 0, 4, 64, fake, 0), "nsrc"),
             ("nsrc 17", lambda: f(src(17), 17, 4, 64, fake, 0), "nsrc"),
             ("B 0", lambda: f(src(), 1, 0, 64, fake, 0), "B >= 1"),
             ("capacity 0", lambda: f(src(), 1, 4, 0, fake, 0), "capacity >= 1"),
             ("capacity -1", lambda: f(src(), 1, 4, -1, fake, 0), "capacity >= 1"),
             ("NULL src", lambda: f(src(src=0), 1, 4, 64, fake, 0), "src and dst"),
             ("NULL dst", lambda: f(src(dst=0), 1, 4, 64, fake, 0), "src and dst"),
             ("row_bytes 0", lambda: f(src(row_bytes=0), 1, 4, 64, fake, 0), "row_bytes"),
             ("row_bytes -4", lambda: f(src(row_bytes=-4), 1, 4, 64, fake, 0), "row_bytes"),
             ("row_bytes 6", lambda: f(src(row_bytes=6), 1, 4, 64, fake, 0), "row_bytes"),
             ("src at an odd address", lambda: f(src(src=fake + 2), 1, 4, 64, fake, 0), "4-byte aligned"),
             ("dst at an odd address", lambda: f(src(dst=fake + 1), 1, 4, 64, fake, 0), "4-byte aligned"),
             ("2^31 copy units", lambda: f(src(row_bytes=1 << 32), 1, 8, 64, fake, 0), "2\\^31"),
             ("exactly 2^31 copy units", lambda: f(src(row_bytes=1 << 30), 1, 8, 64, fake, 0), "2\\^31"),
             ("a product past 64 bits", lambda: f(src(row_bytes=1 << 62), 1, 1 << 30, 64, fake, 0), "2\\^31")]
    for what, call, msg in cases:
        assert call() == -1, what
        assert re.search(msg, _err(lib)), (what, _err(lib))


HEADS = {"avmnist": ("image", "audio", "fusion"), "mmimdb": ("image", "text", "fusion"), "mimic": ("static", "time", "fusion")}
# (task, uncertainty): the evidential engine is AV-MNIST with a fourth tensor per head
TASKS = [("avmnist", False), ("avmnist", True), ("mmimdb", False), ("mimic", False)]


@pytest.mark.parametrize("task, unc", TASKS, ids=["avmnist", "avmnist_uq", "mmimdb", "mimic"])
def test_prediction_record_names_dtypes_and_rows(task, unc):
    from m2_mixer_amd import models as M
    from m2_mixer_amd.accumulators import PredictionRecord, record_key_names
    K, cap, n = 5, 6, 4
    heads = HEADS[task]
    rec = PredictionRecord(task, heads, K, cap, "cpu", uncertainty=unc)
    ml = task == "mmimdb"
    assert tuple(rec.logits.shape) == (3, cap, K) and rec.logits.dtype == torch.float32
    assert tuple(rec.preds.shape) == ((3, cap, K) if ml else (3, cap)) and rec.preds.dtype == torch.int32
    assert tuple(rec.labels.shape) == ((cap, K) if ml else (cap,)) and rec.labels.dtype == (torch.float32 if ml else torch.int64)
    assert (rec.uncertainty is not None) == unc and tuple(rec.state.shape) == (4,)
    gen = torch.Generator().manual_seed(5)
    rec.logits.copy_(torch.randn(3, cap, K, generator=gen))
    rec.preds.copy_(torch.randint(0, 2 if ml else K, tuple(rec.preds.shape), generator=gen).int())
    rec.labels.copy_(torch.randint(0, 2 if ml else K, tuple(rec.labels.shape), generator=gen).to(rec.labels.dtype))
    if unc:
        rec.uncertainty.copy_(torch.rand(3, cap, generator=gen))
    rec.state[0] = n
    assert rec.rows() == n
    got = rec.read()
    a, b = heads[:2]
    names = record_key_names(task, heads)
    lg = (f"logits_{a}", f"logits_{b}", "logits") if task == "mimic" else (f"{a}_logits", f"{b}_logits", "logits")
    assert names["logits"] == lg and names["preds"] == (f"preds_{a}", f"preds_{b}", "preds")
    want = set(lg) | set(names["preds"]) | {"labels"} | (set(names["uncertainty"]) if unc else set())
    assert set(got) == want and not any(k.startswith("loss") for k in got)
    for h in range(3):
        assert torch.equal(got[lg[h]], rec.logits[h, :n]) and got[lg[h]].dtype == torch.float32
        p = got[names["preds"][h]]
        if task == "mimic":                                                # the module's `preds*`: softmax of the logits
            assert torch.equal(p, torch.softmax(rec.logits[h, :n], dim=1))
        else:
            assert p.dtype == torch.int64 and torch.equal(p, rec.preds[h, :n].long())
        if unc:
            assert torch.equal(got[names["uncertainty"][h]], rec.uncertainty[h, :n])
    assert torch.equal(got["labels"], rec.labels[:n]) and got["labels"].dtype == rec.labels.dtype
    # the dump's keys are the task module's, in its order
    module = {"avmnist": M.AVMnistMixerMultiLoss, "mmimdb": M.MMIMDBMixerMultiLoss, "mimic": M.MimicMixerMultiLoss}[task]
    if module.TEST_PRED_KEYS:
        assert rec.save_keys == module.TEST_PRED_KEYS
    assert set(rec.save_keys) <= set(got)
    # overflow names the capacity and the rows seen
    rec.state[0] = cap + 3
    rec.state[3] = 3
    with pytest.raises(RuntimeError, match=rf"capacity {cap} rows, {cap + 3} rows seen"):
        rec.read()
    rec.reset()
    assert rec.rows() == 0 and rec.state.tolist() == [0, 0, 0, 0]


def test_prediction_record_save_writes_the_dump_keys_in_order(tmp_path):
    from m2_mixer_amd.accumulators import PredictionRecord
    rec = PredictionRecord("avmnist", HEADS["avmnist"], 3, 5, "cpu")
    rec.logits.copy_(torch.arange(45, dtype=torch.float32).view(3, 5, 3))
    rec.state[0] = 2
    path = rec.save(str(tmp_path / "test_preds.pt"))
    got = torch.load(path)
    assert tuple(got) == rec.save_keys and torch.equal(got["logits"], rec.logits[2, :2]) and got["preds"].dtype == torch.int64
    assert os.path.getsize(path) < 4096                                    # the rows read, not the record's storage


def test_prediction_record_refuses_nonsense():
    from m2_mixer_amd.accumulators import PredictionRecord
    with pytest.raises(RuntimeError, match="capacity"):
        PredictionRecord("avmnist", HEADS["avmnist"], 10, 0, "cpu")
    with pytest.raises(RuntimeError, match="K = 0"):
        PredictionRecord("avmnist", HEADS["avmnist"], 0, 4, "cpu")
    with pytest.raises(RuntimeError, match="sources"):
        PredictionRecord("avmnist", ("a", "b", "c", "d", "e", "f"), 4, 4, "cpu", uncertainty=True)


@pytest.mark.parametrize("n, batch, steps, want", [
    (43, 8, 1, (5, 0, 3)),            # tests/test_gpu_eval_feed.py: five replays and the tail
    (43, 8, 2, (2, 1, 3)),            # two replays, one eager single, the tail
    (5000, 512, 1, (9, 0, 392)),      # AV-MNIST's validation split at batch 512 (scripts/eval_feed_overhead.py)
    (5000, 512, 3, (3, 0, 392)),
    (10000, 512, 3, (6, 1, 272)),
])
def test_feed_plan_of_an_evaluation_pass(n, batch, steps, want):
    from m2_mixer_amd.data import feed_plan
    got = feed_plan(n, batch, steps)
    assert got == want
    replays, singles, tail = got
    assert (replays * steps + singles) * batch + tail == n and singles < steps and tail < batch
