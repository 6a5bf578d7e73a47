"""Epoch feed, host side (no GPU): the entry points exist in the header, the binding and the built library; feed_plan's
arithmetic; the numpy restatement (tests/feed_ref.py) against a plain index_select; and the argument refusals of the two entry
points, which validate before they touch a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import feed_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_library_carry_the_feed_entry_points():
    from m2_mixer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "m2mixer.h")).read()
    for name in ("m2m_feed_gather", "m2m_epoch_accumulate"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/m2mixer.h"
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name), f"{name} is not exported by the built library"
    assert int(re.search(r"#define M2M_FEED_STATE_WORDS (\d+)", hdr).group(1)) == _lib.FEED_STATE_WORDS == 4
    assert int(re.search(r"#define M2M_FEED_MAX_SOURCES (\d+)", hdr).group(1)) == _lib.FEED_MAX_SOURCES == 4
    assert len(_lib.SIGNATURES["m2m_feed_gather"][1]) == 6 and len(_lib.SIGNATURES["m2m_epoch_accumulate"][1]) == 9
    assert C.sizeof(_lib.FeedSrc) == 24                                    # {const void*, void*, int64_t}
    assert "feed.hip" in open(os.path.join(ROOT, "m2_mixer_amd", "csrc", "Makefile")).read()
    assert _lib.lib().m2m_abi_version() == 18 == _lib.ABI_VERSION          # new entry points only
    assert int(re.search(r"#define M2M_ABI_VERSION (\d+)", hdr).group(1)) == 18


@pytest.mark.parametrize("n, batch, steps, drop_last, want", [
    (43, 8, 2, False, (2, 1, 3)),
    (16, 8, 1, False, (2, 0, 0)),
    (7, 8, 1, False, (0, 0, 7)),
    (43, 8, 2, True, (2, 1, 0)),
    (64, 8, 4, False, (2, 0, 0)),
])
def test_feed_plan(n, batch, steps, drop_last, want):
    from m2_mixer_amd.data import feed_plan
    got = feed_plan(n, batch, steps, drop_last)
    assert got == want
    replays, singles, tail = got
    assert (replays * steps + singles) * batch + tail == (n - n % batch if drop_last else n)      # every sample exactly once


def test_feed_plan_refuses_nonsense():
    from m2_mixer_amd.data import feed_plan
    for bad in ((-1, 8, 1), (8, 0, 1), (8, 8, 0)):
        with pytest.raises(ValueError):
            feed_plan(*bad)


def test_feed_ref_is_an_index_select_with_a_wrapping_cursor():
    rng = np.random.default_rng(3)
    n, B = 10, 4
    a = rng.standard_normal((n, 5)).astype(np.float32)
    y = rng.integers(0, 9, size=(n,), dtype=np.int64)
    perm = rng.permutation(n).astype(np.int32)
    state = np.array([0, 0, n, 0], dtype=np.uint32)
    ta, ty = torch.from_numpy(a), torch.from_numpy(y)
    for lo in (0, 4):
        slots, state = F.gather((a, y), perm, state, B)
        idx = torch.from_numpy(perm[lo:lo + B].astype(np.int64))
        assert np.array_equal(slots[0], F.raw(ta.index_select(0, idx).numpy()))
        assert np.array_equal(slots[1], F.raw(ty.index_select(0, idx).numpy()))
    assert state.tolist() == [8, 0, n, 0]
    # the hand-written wrap: the third batch is perm[8], perm[9], perm[0], perm[1]
    slots, state = F.gather((a, y), perm, state, B)
    hand = [int(perm[8]), int(perm[9]), int(perm[0]), int(perm[1])]
    assert np.array_equal(slots[0], F.raw(a[hand])) and np.array_equal(slots[1], F.raw(y[hand]))
    assert state.tolist() == [12, 0, n, 2]
    # no permutation: the rows themselves, from a cursor that is already past n
    slots, state = F.gather((a,), None, state, 3)
    assert np.array_equal(slots[0], F.raw(a[[2, 3, 4]])) and state.tolist() == [15, 0, n, 2 + 5]


def test_feed_ref_accumulate_by_hand():
    sums, counts = np.zeros(8), np.zeros(5, dtype=np.int64)
    preds = np.array([[1, 2, 3], [1, 0, 3], [0, 0, 0]], dtype=np.int32)
    labels = np.array([1, 2, 3], dtype=np.int64)
    sums, counts = F.accumulate(sums, counts, [0.5, 1.0, 2.0, 3.5], preds, labels, 3)
    assert sums.tolist() == [0.5, 1.0, 2.0, 3.5, 1.5, 3.0, 6.0, 10.5] and counts.tolist() == [3, 2, 0, 1, 3]
    s0, c0 = F.accumulate(np.zeros(8), np.zeros(2, dtype=np.int64), [1, 1, 1, 1], None, None, 5)
    assert c0.tolist() == [1, 5] and s0[4:].tolist() == [5.0] * 4


def _err(lib):
    return lib.m2m_last_error().decode("utf-8", "replace")


def test_gather_refuses_bad_arguments_before_any_launch():
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

    cases = [("NULL srcs", lambda: lib.m2m_feed_gather(None, 1, 0, 4, fake, 0), "srcs and state"),
             ("NULL state", lambda: lib.m2m_feed_gather(src(), 1, 0, 4, 0, 0), "srcs and state"),
             ("nsrc 0", lambda: lib.m2m_feed_gather(src(), 0, 0, 4, fake, 0), "nsrc"),
             ("nsrc 5", lambda: lib.m2m_feed_gather(src(5), 5, 0, 4, fake, 0), "nsrc"),
             ("B 0", lambda: lib.m2m_feed_gather(src(), 1, 0, 0, fake, 0), "B >= 1"),
             ("NULL src", lambda: lib.m2m_feed_gather(src(src=0), 1, 0, 4, fake, 0), "src and dst"),
             ("NULL dst", lambda: lib.m2m_feed_gather(src(dst=0), 1, 0, 4, fake, 0), "src and dst"),
             ("row_bytes 0", lambda: lib.m2m_feed_gather(src(row_bytes=0), 1, 0, 4, fake, 0), "row_bytes"),
             ("row_bytes -4", lambda: lib.m2m_feed_gather(src(row_bytes=-4), 1, 0, 4, fake, 0), "row_bytes"),
             ("row_bytes 6", lambda: lib.m2m_feed_gather(src(row_bytes=6), 1, 0, 4, fake, 0), "row_bytes"),
             ("src at an odd address", lambda: lib.m2m_feed_gather(src(src=fake + 2), 1, 0, 4, fake, 0), "4-byte aligned"),
             ("2^31 copy units", lambda: lib.m2m_feed_gather(src(row_bytes=1 << 32), 1, 0, 8, fake, 0), "2\\^31")]
    for what, call, msg in cases:
        assert call() == -1, what
        assert re.search(msg, _err(lib)), (what, _err(lib))


def test_accumulate_refuses_bad_arguments_before_any_launch():
    from m2_mixer_amd import _lib as L
    lib = L.lib()
    p = 0x1000
    cases = [("NULL losses", (0, 4, p, p, 3, 8, p, p, 0), "losses, sums and counts"),
             ("NULL sums", (p, 4, p, p, 3, 8, 0, p, 0), "losses, sums and counts"),
             ("NULL counts", (p, 4, p, p, 3, 8, p, 0, 0), "losses, sums and counts"),
             ("nloss 0", (p, 0, p, p, 3, 8, p, p, 0), "nloss >= 1"),
             ("nheads -1", (p, 4, p, p, -1, 8, p, p, 0), "nheads"),
             ("heads without preds", (p, 4, 0, p, 3, 8, p, p, 0), "needs preds and labels"),
             ("heads without labels", (p, 4, p, 0, 3, 8, p, p, 0), "needs preds and labels"),
             ("B 0", (p, 4, p, p, 3, 0, p, p, 0), "B >= 1")]
    for what, args, msg in cases:
        assert lib.m2m_epoch_accumulate(*args) == -1, what
        assert re.search(msg, _err(lib)), (what, _err(lib))


def test_resident_tensors_hold_any_tasks_splits():
    from m2_mixer_amd.data import ResidentTensors
    x, y = torch.zeros(43, 5), torch.zeros(43, dtype=torch.int64)
    data = ResidentTensors({"train": (x, y), "val": (x[:7], y[:7])})
    assert data.num_samples("train") == 43 and data.num_batches("train", 8) == 6 and data.num_batches("train", 8, drop_last=True) == 5
    assert data.num_samples("val") == 7 and data.world == 1
    with pytest.raises(ValueError):
        ResidentTensors({"train": (x, y[:5])})
