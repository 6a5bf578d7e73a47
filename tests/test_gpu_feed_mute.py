"""The muted gather on the GPU (-m gpu), bit for bit against tests/mute_ref.py.

m2m_feed_gather_muted copies or zero-fills, so every destination is compared as raw bytes; 64-byte guard cells on both sides of
every destination must stay untouched and the sources unchanged.  Sources are triples in the engines' (input a, input b,
labels) order with rows of 8, 20, 92, 1152 and 3136 bytes (MIMIC's and AV-MNIST's rows, MM-IMDb's targets), plus a 48-byte-row
source view that starts 4 bytes off a 16-byte boundary (the dword path).  B in {1, 3, 8, 64}, n in {B, B + 1, 5 B + 3}; the codes
cycle through 0, 1, 2 over three consecutive gathers, a fourth gather runs past the schedule (it mutes nothing and is counted);
`mute_state` is checked after every gather."""
import numpy as np
import pytest
import torch

import feed_ref as F
import mute_ref as M

pytestmark = pytest.mark.gpu

GUARD = 64
ROW_SETS = {"mimic": (20, 1152, 8), "avmnist_image": (3136, 92, 8), "dwords": (8, 20, 8), "src_off4": (48, 92, 8)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def descs(srcs, dsts, row_bytes):
    from m2_mixer_amd import _lib as L
    desc = (L.FeedSrc * len(srcs))()
    for d, s, t, rb in zip(desc, srcs, dsts, row_bytes):
        d.src, d.dst, d.row_bytes = s.data_ptr(), t.data_ptr(), rb
    return desc


def launch_muted(srcs, dsts, row_bytes, perm, B, state, codes, mute_state):
    from m2_mixer_amd import _lib as L
    return L.lib().m2m_feed_gather_muted(descs(srcs, dsts, row_bytes), len(srcs), L.ptr(perm), B, state.data_ptr(), L.ptr(codes),
                                         0 if codes is None else int(codes.numel()), L.ptr(mute_state), L.stream_ptr())


def words(t):
    return t.cpu().numpy().view(np.uint32).tolist()


@pytest.mark.parametrize("B", [1, 3, 8, 64])
@pytest.mark.parametrize("rows", list(ROW_SETS), ids=list(ROW_SETS))
def test_muted_gather_is_bit_exact_and_stays_inside_its_rows(rows, B, dev):
    row_bytes = ROW_SETS[rows]
    rng = np.random.default_rng(2000 * B + len(rows))
    src_off = 4 if rows == "src_off4" else 0
    for n in (B, B + 1, 5 * B + 3):
        host = [rng.integers(1, 256, size=(n, rb), dtype=np.uint8) for rb in row_bytes]      # (no zero byte: a zeroed slot shows)
        hold = [torch.zeros(src_off + n * rb, dtype=torch.uint8, device=dev) for rb in row_bytes]
        srcs = [h[src_off:].view(n, rb) for h, rb in zip(hold, row_bytes)]
        for s, h in zip(srcs, host):
            s.copy_(torch.from_numpy(h))
        assert all(s.data_ptr() % 16 == src_off for s in srcs)
        perm_h = rng.permutation(n).astype(np.int32)
        perm = torch.from_numpy(perm_h).to(dev)
        codes_h = np.array([0, 1, 2], dtype=np.int32)
        codes = torch.from_numpy(codes_h).to(dev)
        state_h = np.array([1, 0, n, 0], dtype=np.uint32)                                     # a non-zero cursor
        state = torch.from_numpy(state_h.view(np.int32).copy()).to(dev)
        mstate_h = np.array([0, 0], dtype=np.uint32)
        mstate = torch.zeros(2, dtype=torch.int32, device=dev)
        for k in range(4):                                                                    # codes 0, 1, 2, then past the schedule
            bufs = [torch.full((GUARD + B * rb + GUARD,), 0xA5, dtype=torch.uint8, device=dev) for rb in row_bytes]
            dsts = [b[GUARD:GUARD + B * rb] for b, rb in zip(bufs, row_bytes)]
            for d in dsts:
                d.fill_(0x5A)
            assert launch_muted(srcs, dsts, row_bytes, perm, B, state, codes, mstate) == 0
            torch.cuda.synchronize()
            want, state_h, mstate_h = M.gather_muted(host, perm_h, state_h, B, codes_h, mstate_h)
            tag = (rows, B, n, k)
            for i, (b, d, w, rb) in enumerate(zip(bufs, dsts, want, row_bytes)):
                assert np.array_equal(d.cpu().numpy().reshape(B, rb), w), tag + (i,)
                assert bool(w.any()) == (k == 0 or k == 3 or i != k - 1), "the reference itself mutes source k - 1 only"
                g = b.cpu().numpy()
                assert (g[:GUARD] == 0xA5).all() and (g[GUARD + B * rb:] == 0xA5).all(), ("guard cells", tag)
            assert words(state) == state_h.tolist(), tag
            assert words(mstate) == mstate_h.tolist(), tag
        assert words(mstate) == [4, 1]
        for s, h in zip(srcs, host):
            assert np.array_equal(s.cpu().numpy(), h), ("a source changed", rows, B, n)


def test_code_zero_equals_the_plain_gather(dev):
    from m2_mixer_amd import _lib as L
    n, B, row_bytes = 29, 8, (3136, 1152, 8)
    rng = np.random.default_rng(12)
    host = [rng.integers(0, 256, size=(n, rb), dtype=np.uint8) for rb in row_bytes]
    srcs = [torch.from_numpy(h).to(dev) for h in host]
    perm = torch.from_numpy(rng.permutation(n).astype(np.int32)).to(dev)
    outs = []
    for muted in (False, True):
        state = torch.tensor([5, 0, n, 0], dtype=torch.int32, device=dev)
        dsts = [torch.full((B * rb,), 0x5A, dtype=torch.uint8, device=dev) for rb in row_bytes]
        if muted:
            assert launch_muted(srcs, dsts, row_bytes, perm, B, state, None, torch.zeros(2, dtype=torch.int32, device=dev)) == 0
        else:
            L.check(L.lib().m2m_feed_gather(descs(srcs, dsts, row_bytes), 3, perm.data_ptr(), B, state.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
        outs.append(([d.clone() for d in dsts], words(state)))
    assert all(torch.equal(a, b) for a, b in zip(outs[0][0], outs[1][0])) and outs[0][1] == outs[1][1]
    want, _ = F.gather(host, perm.cpu().numpy(), np.array([5, 0, n, 0], dtype=np.uint32), B)
    assert all(np.array_equal(d.cpu().numpy().reshape(B, -1), w) for d, w in zip(outs[1][0], want))


def _feed(dev, n, B, seed=5, **kw):
    from m2_mixer_amd.engine import EpochFeed
    rng = np.random.default_rng(seed)
    a = torch.from_numpy(rng.standard_normal((n, 5)).astype(np.float32) + 3.0).to(dev)
    b = torch.from_numpy(rng.standard_normal((n, 6, 4)).astype(np.float32) + 3.0).to(dev)
    y = torch.from_numpy(rng.integers(1, 6, size=(n,), dtype=np.int64)).to(dev)
    return EpochFeed((a, b, y), B, dev, **kw), (a, b, y)


def expect(srcs, order, lo, B, code):
    sel = order[lo:lo + B]
    out = [t.index_select(0, sel) for t in srcs]
    if code:
        out[code - 1] = torch.zeros_like(out[code - 1])
    return out


def test_feed_with_muting_walks_its_schedule_and_check_raises_past_it(dev):
    n, B = 20, 4
    feed, srcs = _feed(dev, n, B, muting=True)
    assert feed.mute_codes.dtype == torch.int32 and feed.mute_codes.numel() == 5 and feed.mute_state.numel() == 2
    order = torch.from_numpy(np.random.default_rng(8).permutation(n)).to(dev)
    codes = [2, 0, 1, 1, 0]
    feed.start(order, muting=codes)
    assert feed.mute_codes.tolist() == codes and words(feed.mute_state) == [0, 0]
    slots = feed.new_slots()
    for k in range(5):
        feed.gather_into(slots)
        torch.cuda.synchronize()
        for got, want in zip(slots, expect(srcs, order, k * B, B, codes[k])):
            assert torch.equal(got, want), k
        assert words(feed.mute_state) == [k + 1, 0]
    feed.check()
    feed.gather_into(slots)                                # a sixth gather: past the order AND past the schedule
    torch.cuda.synchronize()
    assert words(feed.mute_state) == [6, 1]
    for got, want in zip(slots, expect(srcs, order, 0, B, 0)):
        assert torch.equal(got, want), "a step past the schedule mutes nothing"
    with pytest.raises(RuntimeError):
        feed.check()
    feed.state.copy_(torch.tensor([0, 0, n, 0], dtype=torch.int32))          # only the muting overflow left
    with pytest.raises(RuntimeError, match="muting schedule"):
        feed.check()
    feed.start(order)                                      # None: all zeros; the step index and the overflow word reset
    assert feed.mute_codes.tolist() == [0] * 5 and words(feed.mute_state) == [0, 0]
    feed.start(order, muting=[1, 2])                       # a shorter schedule: the rest is zero
    assert feed.mute_codes.tolist() == [1, 2, 0, 0, 0]
    feed.check()


def test_start_refuses_codes_outside_the_inputs(dev):
    feed, _ = _feed(dev, 20, 4, muting=True)
    with pytest.raises(ValueError, match="labels"):
        feed.start(muting=[0, 3])                          # 3 would mute the last source, the labels
    with pytest.raises(ValueError):
        feed.start(muting=[-1])
    with pytest.raises(ValueError):
        feed.start(muting=[0] * 6)                         # more steps than the epoch has
    with pytest.raises(ValueError):
        feed.start(muting=[0.0, 1.0])
    plain, _ = _feed(dev, 20, 4)
    assert plain.mute_codes is None and plain.mute_state is None
    with pytest.raises(ValueError, match="muting=True"):
        plain.start(muting=[0])


def test_captured_muted_gather_follows_two_schedules(dev):
    n, B = 43, 8
    feed, srcs = _feed(dev, n, B, seed=6, muting=True)
    order = torch.from_numpy(np.random.default_rng(1).permutation(n)).to(dev)
    slots = feed.new_slots()
    feed.start(order)
    ptrs = (feed.mute_codes.data_ptr(), feed.mute_state.data_ptr(), feed.perm.data_ptr(), feed.state.data_ptr())
    feed.gather_into(slots)                                # (lazy initialisation outside the capture)
    feed.start(order)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        feed.gather_into(slots)
    for codes in ([1, 0, 2, 2], [0, 2, 1, 0]):
        feed.start(order, muting=codes)                    # written in place: the graph keeps reading the same memory
        assert ptrs == (feed.mute_codes.data_ptr(), feed.mute_state.data_ptr(), feed.perm.data_ptr(), feed.state.data_ptr())
        for k in range(4):
            g.replay()
            torch.cuda.synchronize()
            for got, want in zip(slots, expect(srcs, order, k * B, B, codes[k])):
                assert torch.equal(got, want), (codes, k)
        assert feed.rows() == 4 * B and words(feed.mute_state) == [4, 0]
        feed.check()


def test_every_refusal_returns_minus_one_and_leaves_the_slots(dev):
    from m2_mixer_amd import _lib as L
    n, B, row_bytes = 9, 4, (20, 16, 8)
    srcs = [torch.full((n, rb), 7, dtype=torch.uint8, device=dev) for rb in row_bytes]
    dsts = [torch.full((B * rb,), 0x5A, dtype=torch.uint8, device=dev) for rb in row_bytes]
    state = torch.tensor([0, 0, n, 0], dtype=torch.int32, device=dev)
    codes = torch.tensor([1, 2], dtype=torch.int32, device=dev)
    mstate = torch.zeros(2, dtype=torch.int32, device=dev)
    lib = L.lib()
    d = lambda **kw: descs(srcs, dsts, [kw.get("rb0", row_bytes[0])] + list(row_bytes[1:]))
    sp, cp, mp, st = state.data_ptr(), codes.data_ptr(), mstate.data_ptr(), L.stream_ptr()
    calls = {"NULL mute_state": lambda: lib.m2m_feed_gather_muted(d(), 3, 0, B, sp, cp, 2, 0, st),
             "NULL codes with ncodes > 0": lambda: lib.m2m_feed_gather_muted(d(), 3, 0, B, sp, 0, 2, mp, st),
             "ncodes < 0": lambda: lib.m2m_feed_gather_muted(d(), 3, 0, B, sp, cp, -1, mp, st),
             "NULL srcs": lambda: lib.m2m_feed_gather_muted(None, 3, 0, B, sp, cp, 2, mp, st),
             "NULL state": lambda: lib.m2m_feed_gather_muted(d(), 3, 0, B, 0, cp, 2, mp, st),
             "nsrc 0": lambda: lib.m2m_feed_gather_muted(d(), 0, 0, B, sp, cp, 2, mp, st),
             "nsrc 5": lambda: lib.m2m_feed_gather_muted(d(), 5, 0, B, sp, cp, 2, mp, st),
             "B 0": lambda: lib.m2m_feed_gather_muted(d(), 3, 0, 0, sp, cp, 2, mp, st),
             "row_bytes 6": lambda: lib.m2m_feed_gather_muted(d(rb0=6), 3, 0, B, sp, cp, 2, mp, st)}
    for what, call in calls.items():
        assert call() == -1, what
        assert lib.m2m_last_error(), what
    torch.cuda.synchronize()
    assert all(bool((t == 0x5A).all()) for t in dsts), "a refused call wrote a slot"
    assert words(state) == [0, 0, n, 0] and words(mstate) == [0, 0], "a refused call advanced a counter"
