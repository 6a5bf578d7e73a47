"""Epoch feed kernels on the GPU (-m gpu), bit for bit against tests/feed_ref.py.

m2m_feed_gather is a pure copy, so every destination is compared as raw bytes; 64-byte guard cells on both sides of every
destination must stay untouched and the sources unchanged.  Row sizes: MIMIC's (20, 1152, 8) and AV-MNIST's (3136, 50176, 8)
source triples, one 16-byte unit, one dword, MM-IMDb's 92-byte target rows, 4100 bytes (1025 dwords: a row crosses the
1024-unit tile of a workgroup), and 16-divisible rows behind a source or a destination that sits 4 bytes off a 16-byte boundary
(the dword path).  B in {1, 3, 8, 64}, n in {B, B + 1, 5 B + 3}, cursor 0 and non-zero (past n for the small splits), with and
without a permutation.  m2m_epoch_accumulate: hits exact, sums to 1e-12 relative in float64."""
import numpy as np
import pytest
import torch

import feed_ref as F

pytestmark = pytest.mark.gpu

GUARD = 64
ROW_SETS = {"mimic": (20, 1152, 8), "avmnist": (3136, 50176, 8), "unit16": (16,), "dword": (4,), "mmimdb_targets": (92,),
            "tile_crossing": (4100,), "src_off4": (48,), "dst_off4": (48,)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def launch_gather(srcs, dsts, row_bytes, perm, B, state):
    from m2_mixer_amd import _lib as L
    desc = (L.FeedSrc * len(srcs))()
    for d, s, t, rb in zip(desc, srcs, dsts, row_bytes):
        d.src, d.dst, d.row_bytes = s.data_ptr(), t.data_ptr(), rb
    L.check(L.lib().m2m_feed_gather(desc, len(srcs), L.ptr(perm), B, state.data_ptr(), L.stream_ptr()), "feed_gather")


@pytest.mark.parametrize("B", [1, 3, 8, 64])
@pytest.mark.parametrize("rows", list(ROW_SETS), ids=list(ROW_SETS))
def test_gather_is_bit_exact_and_stays_inside_its_rows(rows, B, dev):
    row_bytes = ROW_SETS[rows]
    rng = np.random.default_rng(1000 * B + len(rows))
    src_off = 4 if rows == "src_off4" else 0
    dst_off = 4 if rows == "dst_off4" else 0
    for n in (B, B + 1, 5 * B + 3):
        host = [rng.integers(0, 256, size=(n, rb), dtype=np.uint8) for rb in row_bytes]
        hold = [torch.zeros(src_off + n * rb, dtype=torch.uint8, device=dev) for rb in row_bytes]
        srcs = [h[src_off:].view(n, rb) for h, rb in zip(hold, row_bytes)]
        for s, h in zip(srcs, host):
            s.copy_(torch.from_numpy(h))
        assert all(s.data_ptr() % 16 == src_off for s in srcs)
        for cursor in (0, 2 * B + 1):
            for with_perm in (True, False):
                perm_h = rng.permutation(n).astype(np.int32) if with_perm else None
                perm = torch.from_numpy(perm_h).to(dev) if with_perm else None
                before = np.array([cursor, 0, n, 0], dtype=np.uint32)
                state = torch.from_numpy(before.view(np.int32).copy()).to(dev)
                bufs = [torch.full((GUARD + dst_off + B * rb + GUARD,), 0xA5, dtype=torch.uint8, device=dev) for rb in row_bytes]
                dsts = [b[GUARD + dst_off:GUARD + dst_off + B * rb] for b, rb in zip(bufs, row_bytes)]
                for d in dsts:
                    d.fill_(0x5A)
                assert all(d.data_ptr() % 16 == dst_off for d in dsts)
                launch_gather(srcs, dsts, row_bytes, perm, B, state)
                torch.cuda.synchronize()
                want, after = F.gather(host, perm_h, before, B)
                tag = (rows, B, n, cursor, with_perm)
                for b, d, w, rb in zip(bufs, dsts, want, row_bytes):
                    assert np.array_equal(d.cpu().numpy().reshape(B, rb), w), tag
                    g = b.cpu().numpy()
                    assert (g[:GUARD + dst_off] == 0xA5).all() and (g[GUARD + dst_off + B * rb:] == 0xA5).all(), ("guard cells", tag)
                assert state.cpu().numpy().view(np.uint32).tolist() == after.tolist(), tag
        for s, h in zip(srcs, host):
            assert np.array_equal(s.cpu().numpy(), h), ("a source changed", rows, B, n)


def _feed(dev, n, B, seed=5):
    from m2_mixer_amd.engine import EpochFeed
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((n, 5)).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, 6, size=(n,), dtype=np.int64)).to(dev)
    return EpochFeed((x, y), B, dev), x, y


def test_three_launches_wrap_and_check_raises(dev):
    n, B = 10, 4
    feed, x, y = _feed(dev, n, B)
    order = torch.from_numpy(np.random.default_rng(8).permutation(n))
    feed.start(order)
    slots = feed.new_slots()
    seen = []
    for _ in range(3):
        feed.gather_into(slots)
        seen.append(tuple(t.clone() for t in slots))
    torch.cuda.synchronize()
    o = order.tolist()
    for k, idx in enumerate((o[0:4], o[4:8], [o[8], o[9], o[0], o[1]])):
        sel = torch.tensor(idx, device=dev)
        assert torch.equal(seen[k][0], x.index_select(0, sel)) and torch.equal(seen[k][1], y.index_select(0, sel)), k
    assert feed.state.cpu().numpy().view(np.uint32).tolist() == [12, 0, n, 2]
    assert feed.rows() == 12
    with pytest.raises(RuntimeError, match=r"12 rows .* split of 10"):
        feed.check()
    feed.start()                                       # identity order, cursor and wrapped count back to zero
    feed.gather_into(slots)
    torch.cuda.synchronize()
    assert torch.equal(slots[0], x[:4]) and torch.equal(slots[1], y[:4]) and feed.rows() == 4
    feed.check()


def test_start_refuses_an_order_outside_the_split(dev):
    feed, _, _ = _feed(dev, 10, 4)
    with pytest.raises(ValueError, match="span"):
        feed.start(torch.arange(1, 11))
    with pytest.raises(ValueError):
        feed.start(torch.arange(9))
    with pytest.raises(ValueError):
        feed.gather_into(feed.new_slots()[:1])


def test_captured_gather_walks_the_order_and_follows_a_new_one(dev):
    n, B = 43, 8
    feed, x, y = _feed(dev, n, B, seed=6)
    first = torch.from_numpy(np.random.default_rng(1).permutation(n)).to(dev)          # a device order
    second = torch.from_numpy(np.random.default_rng(2).permutation(n))                 # a host order
    slots = feed.new_slots()
    feed.start(first)
    perm_ptr, state_ptr = feed.perm.data_ptr(), feed.state.data_ptr()
    feed.gather_into(slots)                            # (lazy initialisation outside the capture)
    feed.start(first)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        feed.gather_into(slots)
    for order in (first, second):
        if order is second:
            feed.start(second)                         # written in place: the graph keeps reading the same memory
            assert (feed.perm.data_ptr(), feed.state.data_ptr()) == (perm_ptr, state_ptr)
        for k in range(3):
            g.replay()
            torch.cuda.synchronize()
            sel = order[k * B:(k + 1) * B].to(dev)
            assert torch.equal(slots[0], x.index_select(0, sel)) and torch.equal(slots[1], y.index_select(0, sel)), k
        assert feed.rows() == 3 * B
        feed.check()


class _Step:
    """What EpochFeed.accumulate reads off an engine."""

    def __init__(self, B, nheads, dev, multilabel=False):
        self.B = B
        self.losses = torch.zeros(4, device=dev)
        self.preds = torch.zeros((3, B, 7) if multilabel else (nheads, B), dtype=torch.int32, device=dev)


@pytest.mark.parametrize("B", [13, 70])
@pytest.mark.parametrize("multilabel", [False, True], ids=["three_heads", "no_heads"])
def test_epoch_accumulate_against_numpy(B, multilabel, dev):
    feed, _, _ = _feed(dev, 100, B)
    step = _Step(B, 3, dev, multilabel)
    feed.bind(step)
    assert feed.nheads == (0 if multilabel else 3) and feed.nloss == 4
    feed.start()
    rng = np.random.default_rng(B)
    sums, counts = np.zeros(8), np.zeros(feed.nheads + 2, dtype=np.int64)
    for _ in range(3):
        losses = rng.random(4).astype(np.float32) * 3
        labels = rng.integers(0, 4, size=(B,), dtype=np.int64)
        preds = None if multilabel else rng.integers(0, 4, size=(3, B)).astype(np.int32)
        step.losses.copy_(torch.from_numpy(losses))
        if not multilabel:
            step.preds.copy_(torch.from_numpy(preds))
        feed.accumulate(step, None if multilabel else torch.from_numpy(labels).to(dev))
        sums, counts = F.accumulate(sums, counts, losses, preds, labels, B)
    got_s, got_c = feed.read()
    assert got_c.tolist() == counts.tolist()                               # hits, steps, samples: exact
    assert got_c[feed.nheads] == 3 and got_c[feed.nheads + 1] == 3 * B
    rel = np.abs(got_s - sums) / np.abs(sums)
    print("sums, relative error:", rel.max())
    assert rel.max() < 1e-12
    feed.start()                                                           # a new epoch clears the accumulators in place
    got_s, got_c = feed.read()
    assert not got_s.any() and not got_c.any()
