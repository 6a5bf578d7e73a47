"""m2m_record_append through the C ABI (-m gpu) against its numpy restatement (tests/record_ref.py).  Copies are exact: every
comparison is byte for byte, no tolerance.

Every destination sits between guard cells filled with a pattern that must survive, and holds more rows than any capacity used,
so that rows at or past the capacity are there to be checked too.  row_bytes 4 and 8 take the 4-byte form, 16 and 256 the 16-byte
form, 40 and 92 are K = 10 and K = 23 float rows (no multiple of 16: the 4-byte form).  B = 70 at 256 bytes is 1120 16-byte units:
more than one 1024-unit workgroup tile; B = 70 at 92 bytes is 1610 4-byte units, the same for the 4-byte form.  A source or a
destination at an address that is a multiple of 4 but not of 16 must take the 4-byte form at row_bytes = 16 and 256 too."""
import numpy as np
import pytest
import torch

import record_ref as RR

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xAB, 256                                # guard bytes on either side (a multiple of 16: the alignment is the buffer's)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


class Bench:
    """nsrc sources of B rows and their destinations of `rows` rows between guards; src_off / dst_off: byte offsets (multiples of
    4) added to source / destination 0's address."""

    def __init__(self, dev, row_bytes, B, rows, src_off=0, dst_off=0):
        from m2_mixer_amd import _lib as L
        self.L, self.dev, self.rbs, self.B, self.rows = L, dev, list(row_bytes), B, rows
        self.offs = [(src_off, dst_off)] + [(0, 0)] * (len(self.rbs) - 1)
        self.src = [torch.zeros(B * rb + 32, dtype=torch.uint8, device=dev) for rb in self.rbs]
        self.dst = [torch.empty(2 * GUARD + rows * rb + 32, dtype=torch.uint8, device=dev) for rb in self.rbs]
        self.state = torch.zeros(L.RECORD_STATE_WORDS, dtype=torch.int32, device=dev)
        for t in self.src + self.dst:
            assert t.data_ptr() % 16 == 0
        self.desc = (L.FeedSrc * len(self.rbs))()
        for d, s, t, rb, (so, do) in zip(self.desc, self.src, self.dst, self.rbs, self.offs):
            d.src, d.dst, d.row_bytes = s.data_ptr() + so, t.data_ptr() + GUARD + do, rb
        self.clear()

    def clear(self):
        for t in self.dst:
            t.fill_(FILL)
        self.state.zero_()

    def load(self, data):
        """data: one (B, row_bytes) uint8 host array per source -> the static source buffers."""
        for s, a, rb, (so, _) in zip(self.src, data, self.rbs, self.offs):
            s[so:so + self.B * rb].copy_(torch.from_numpy(a.reshape(-1)).to(self.dev))

    def append(self, capacity):
        L = self.L
        L.check(L.lib().m2m_record_append(self.desc, len(self.rbs), self.B, capacity, self.state.data_ptr(), L.stream_ptr()),
                "record_append")

    def read(self):
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in self.dst], self.state.cpu().numpy().view(np.uint32)

    def expect(self, steps, capacity, restart=None):
        """The whole destination buffers (guards included) and the state after appending `steps` (a list of per-source arrays
        each) to an empty record -- and then, with `restart`, after clearing the state and appending that."""
        dsts = [np.full((self.rows, rb), FILL, dtype=np.uint8) for rb in self.rbs]
        state = np.zeros(4, dtype=np.uint32)
        for data in steps:
            dsts, state = RR.append(dsts, data, state, capacity)
        if restart is not None:
            dsts, state = RR.append(dsts, restart, np.zeros(4, dtype=np.uint32), capacity)
        whole = []
        for d, rb, (_, do) in zip(dsts, self.rbs, self.offs):
            buf = np.full(2 * GUARD + self.rows * rb + 32, FILL, dtype=np.uint8)
            buf[GUARD + do:GUARD + do + self.rows * rb] = d.reshape(-1)
            whole.append(buf)
        return whole, state


def steps_of(rbs, B, seed, count=3):
    rng = np.random.default_rng(seed)
    # (no byte equals the fill pattern: an unwritten cell cannot pass for a written one)
    draw = lambda rb: (rng.integers(0, 0xAB, size=(B, rb), dtype=np.uint8))
    return [[draw(rb) for rb in rbs] for _ in range(count)]


def check_bench(bench, seed):
    B = bench.B
    steps = steps_of(bench.rbs, B, seed)

    def same(got, want, what):
        (gd, gs), (wd, ws) = got, want
        assert gs.tolist() == ws.tolist(), (what, gs.tolist(), ws.tolist())
        for i, (g, w) in enumerate(zip(gd, wd)):
            assert np.array_equal(g, w), f"{what}: source {i} differs in {int((g != w).sum())} byte(s), first at {int(np.argmax(g != w))}"

    # three appends that fit: bit-equal to the restatement, state [3B, 0, 0, 0]
    fit = 3 * B + 1
    assert fit <= bench.rows
    for data in steps:
        bench.load(data)
        bench.append(fit)
    eager = bench.read()
    same(eager, bench.expect(steps, fit), "three appends")
    assert eager[1].tolist() == [3 * B, 0, 0, 0]
    # state cleared between epochs: restarts at row 0 (the rows behind the cursor keep what they held)
    bench.state.zero_()
    bench.load(steps[1])
    bench.append(fit)
    got = bench.read()
    same(got, bench.expect(steps, fit, restart=steps[1]), "restart at row 0")
    assert got[1].tolist() == [B, 0, 0, 0]
    # capacity 2B + 1: the third append writes exactly one row and drops B - 1; rows at or past the capacity keep their pattern
    bench.clear()
    tight = 2 * B + 1
    for data in steps:
        bench.load(data)
        bench.append(tight)
    got = bench.read()
    same(got, bench.expect(steps, tight), "capacity 2B + 1")
    assert got[1].tolist() == [3 * B, 0, 0, B - 1]
    for g, data, rb, (_, do) in zip(got[0], steps[2], bench.rbs, bench.offs):
        rows = g[GUARD + do:GUARD + do + bench.rows * rb].reshape(bench.rows, rb)
        assert np.array_equal(rows[2 * B], data[0]), "the one row below the capacity"
        assert (rows[tight:] == FILL).all(), "a row at or past the capacity was written"
    # captured in a graph and replayed three times: the same buffers and state as three eager calls
    bench.clear()
    bench.load(steps[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bench.append(fit)
    bench.clear()                                                          # (a capture runs nothing; clear for symmetry)
    for data in steps:
        bench.load(data)
        g.replay()
    same(bench.read(), eager, "graph replays against eager calls")


ROW_BYTES = (4, 8, 16, 40, 92, 256)
BATCHES = (1, 3, 8, 70)


@pytest.mark.parametrize("nsrc", [1, 7, 16])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("row_bytes", ROW_BYTES)
def test_append_is_the_restatement(row_bytes, B, nsrc, dev):
    check_bench(Bench(dev, [row_bytes] * nsrc, B, 3 * B + 3), seed=row_bytes * 1000 + B * 17 + nsrc)


@pytest.mark.parametrize("B", [3, 70])
@pytest.mark.parametrize("row_bytes, src_off, dst_off", [(16, 4, 0), (16, 0, 8), (256, 12, 0), (256, 4, 4)])
def test_an_address_that_is_no_multiple_of_16_takes_the_4_byte_form(row_bytes, src_off, dst_off, B, dev):
    """row_bytes is a multiple of 16, one address is not: 16-byte accesses there would be misaligned.  B = 70 at 256 bytes is 4480
    4-byte units: more than one workgroup tile in the 4-byte form.  The second source stays on the 16-byte form in the same
    launch."""
    check_bench(Bench(dev, [row_bytes, row_bytes], B, 3 * B + 3, src_off=src_off, dst_off=dst_off), seed=row_bytes + src_off + B)


@pytest.mark.parametrize("B", [3, 70])
def test_the_sources_of_an_engine_step_in_one_launch(B, dev):
    """Ten sources as PredictionRecord.add of the evidential engine hands them over: three heads' logits (K = 10: 40 bytes), preds
    and uncertainties (4 bytes each) and int64 labels (8 bytes) -- and MM-IMDb's K = 23 rows beside 16-byte-form rows."""
    check_bench(Bench(dev, [40, 40, 40, 4, 4, 4, 4, 4, 4, 8], B, 3 * B + 3), seed=77 + B)
    check_bench(Bench(dev, [92, 92, 92, 92, 92, 92, 92, 256, 16], B, 3 * B + 3), seed=78 + B)
