"""CPU tests of the dropout stream's host replica (tests/drop_ref.py; specification: DESIGN.md, "Dropout stream").

The replica is deterministic, so a bound it meets once holds for good.  What is checked is the STREAM's quality as specified --
keep rates, independence between sites / blocks / steps / seeds / towers, serial correlation, distinct keys, the threshold's
rounding -- on masks of n = 2^20 elements; tests/test_gpu_drop_stream.py then ties the library to the replica bit for bit.

Bounds: 5 standard deviations of the statistic under independent fair draws (binomial keep count; phi and serial correlations
are N(0, 1 / n) under independence), as set with the test's grid; observed maxima are in each test's docstring."""
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

import drop_ref as D

P_GRID = (0.1, 0.3, 0.5, 0.9)
SEEDS = (0, 123, 2 ** 32 - 1)
STEPS = (0, 1, 2, 2 ** 32 - 1)
SITES = (0, 1, 2, 3, 4, 1024, 2 ** 20)
# a tower geometry whose four sites all have 2^20 elements: (B D, T) = (B D, N) = (32768, 32), (B N, Cp) = (B N, D) = (8192, 128)
GEO = dict(B=256, N=32, D=128, T=32, Cp=128)
NEL = 1 << 20
SD = 5.0


def site_mask(p, seed, step, site):
    """The mask of absolute site number `site` (tower base 0: block site // 4, site site % 4) in the GEO tower."""
    return D.tower_mask(seed, step, 0, site // 4, site % 4, p, **GEO)


def keep_sd(m, p):
    q = D.drop_thr(p) / 65536
    return abs(float(m.mean()) - q) / math.sqrt(q * (1 - q) / m.size)


def corr_sd(a, b):
    """|phi correlation| x sqrt(n) of two 0 / 1 vectors."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    ma, mb = a.mean(), b.mean()
    phi = ((a * b).mean() - ma * mb) / math.sqrt(ma * (1 - ma) * mb * (1 - mb))
    return abs(phi) * math.sqrt(a.size)


def test_mix32_and_site_key_against_python_integers():
    """The uint32 array arithmetic against the same specification in Python's unbounded integers, reduced by hand."""
    M = 0xFFFFFFFF

    def mix(x):
        x ^= x >> 16
        x = x * 0x7FEB352D & M
        x ^= x >> 15
        x = x * 0x846CA68B & M
        return x ^ x >> 16

    xs = [0, 1, 2, 0x80000000, M, 0x12345678, 0xDEADBEEF]
    assert [int(v) for v in D.mix32(np.array(xs, dtype=np.uint32))] == [mix(x) for x in xs]
    assert int(D.mix32(0)[0]) == 0                     # the hash's fixed point: the key's additive constant keeps off it
    for seed, step, site in itertools.product(SEEDS, STEPS, SITES):
        want = mix(seed ^ mix((step * 0x9E3779B9 + site * 0x85EBCA77 + 0x1234567) & M))
        assert int(D.site_key(seed, step, site)[0]) == want
    # the step is a sum modulo 2^32, the site too
    assert D.add_steps(2 ** 32 - 1, 2) == 1 and D.add_steps(5, 0) == 5
    assert int(D.site_key(7, D.add_steps(2 ** 32 - 3, 5), 9)[0]) == int(D.site_key(7, 2, 9)[0])


def test_drop_thr_against_exact_rationals():
    """thr = (long)((1 - (double)p) 65536 + 0.5), p a float32, clamped to [1, 65536]: against fractions on a grid with the
    shipped rates, a tie (0.25 - 2^-17 is a float32 and (1 - p) 65536 = 49152.5 exactly: C's + 0.5-and-truncate rounds it UP,
    Python's round() to the even 49152), the smallest rates (thr 65536 with p > 0: nothing is dropped) and the largest."""
    tie = 0.25 - 2.0 ** -17
    assert float(np.float32(tie)) == tie and (1 - Fraction(tie)) * 65536 == Fraction(98305, 2)
    grid = [0.0, 0.5, 0.1, 0.3, float(np.float32(1) / np.float32(3)), tie, 0.75 - 2.0 ** -17, 0.5 - 2.0 ** -17, 0.5 + 2.0 ** -17,
            1e-6, 2.0 ** -17, float(np.nextafter(np.float32(2.0 ** -17), np.float32(1))), 0.99999, 1 - 2.0 ** -17, 1 - 2.0 ** -16,
            1.0, 0.2, 0.25, 0.7, 0.9]
    grid += [k / 997 for k in range(1, 997, 7)] + [float(np.float32(k * 2.0 ** -17)) for k in range(1, 2 ** 17, 1021)]
    for p in grid:
        assert D.drop_thr(p) == D.drop_thr_exact(p), p
        assert 1 <= D.drop_thr(p) <= 65536
    assert D.drop_thr(0.5) == 32768 and D.drop_thr(0.0) == 65536 and D.drop_thr(0.1) == 58982 and D.drop_thr(0.3) == 45875
    assert D.drop_thr(tie) == 49153 and round((1 - tie) * 65536) == 49152
    assert D.drop_thr(0.5 - 2.0 ** -17) == 32769 and D.drop_thr(0.5 + 2.0 ** -17) == 32768       # (both .5 ties go up)
    assert D.drop_thr(1e-6) == 65536 and D.drop_thr(0.99999) == 1 and D.drop_thr(1.0) == 1
    assert D.drop_scale(0.5) == 2.0 and D.p_effective(0.5) == 0.5
    assert D.p_effective(tie) == 1 - 49153 / 65536


def test_engine_ref_uses_the_library_threshold():
    """The oracle's drop_p of the engine tests is the rate the kernels realise, ties included."""
    import engine_ref as R
    tie = 0.25 - 2.0 ** -17
    for p in (0.1, 0.3, 0.5, tie):
        assert R.p_effective(p) == D.p_effective(p)


@pytest.mark.parametrize("p", P_GRID)
def test_keep_rate_and_serial_correlation(p):
    """Every mask of the grid (3 seeds x 4 steps x 7 sites; at p = 0.5 sites 0..2 modulo 4 are one-bit draws): keep rate within
    5 binomial sd of thr / 65536; serial correlation at lag 1 (the two halves of a word / neighbouring bits) and lag 32
    (neighbouring words) below 5 sd.  Observed maxima over the four rates: keep rate 2.44, lag 1 3.26, lag 32 3.33."""
    worst = dict(keep=0.0, lag1=0.0, lag32=0.0)
    for seed, step, site in itertools.product(SEEDS, STEPS, SITES):
        m = site_mask(p, seed, step, site)
        assert m.size == NEL and m.dtype == np.uint8 and int(m.max()) <= 1
        worst["keep"] = max(worst["keep"], keep_sd(m, p))
        for lag in (1, 32):
            worst[f"lag{lag}"] = max(worst[f"lag{lag}"], corr_sd(m[:-lag], m[lag:]))
    print(f"p = {p}: {worst}")
    assert worst["keep"] < SD and worst["lag1"] < SD and worst["lag32"] < SD, worst


def pair_set(p):
    """The masks whose pairwise independence is checked: name -> mask (all 2^20 elements)."""
    t = lambda seed, step, base, blk, site: D.tower_mask(seed, step, base, blk, site, p, **GEO)
    out = {}
    for blk, site in itertools.product((0, 1), range(4)):                 # the four sites of one block; block b against b + 1
        out[f"seed 123 step 1 base 0 block {blk} site {site}"] = t(123, 1, 0, blk, site)
    for site in range(4):                                                 # step s against s + 1
        out[f"seed 123 step 2 base 0 block 0 site {site}"] = t(123, 2, 0, 0, site)
    for step in (0, 2 ** 32 - 1):
        out[f"seed 123 step {step} base 0 block 0 site 3"] = t(123, step, 0, 0, 3)
    for seed in (0, 2 ** 32 - 1):
        out[f"seed {seed} step 1 base 0 block 0 site 3"] = t(seed, 1, 0, 0, 3)
    # two towers as the engines (bases 0 / 1024 / 2048: engine.py _build) and the modules (1024 k + 32 chunk: modules/mixer.py)
    # assign their bases; the MLP's layers under the MIMIC engine's base (4096) and a module's (2^20 | 16 k: modules/mlp.py)
    for base in (1024, 2048, 1024 + 32, 3 * 1024):
        for site in (0, 2):
            out[f"seed 123 step 1 base {base} block 0 site {site}"] = t(123, 1, base, 0, site)
    for base in (4096, 1 << 20, 1 << 20 | 16):
        for layer in (0, 1):
            out[f"seed 123 step 1 mlp base {base} layer {layer}"] = D.mlp_mask(123, 1, base, layer, p, 8192, 128).reshape(-1)
    return out


@pytest.mark.parametrize("p", P_GRID)
def test_masks_of_different_sites_blocks_steps_seeds_and_towers_are_independent(p):
    """|phi| sqrt(n) < 5 over every pair of pair_set(p) (30 masks, 435 pairs per p; equal masks would score 1024).  Observed
    maximum over the four rates: 3.57."""
    masks = pair_set(p)
    names = list(masks)
    f = {k: v.astype(np.float64) for k, v in masks.items()}
    mean = {k: v.mean() for k, v in f.items()}
    worst, at = 0.0, None
    for a, b in itertools.combinations(names, 2):
        phi = (np.dot(f[a], f[b]) / NEL - mean[a] * mean[b]) / math.sqrt(mean[a] * (1 - mean[a]) * mean[b] * (1 - mean[b]))
        v = abs(phi) * math.sqrt(NEL)
        if v > worst:
            worst, at = v, (a, b)
    print(f"p = {p}: {len(names)} masks, worst {worst:.2f} at {at}")
    assert worst < SD, (worst, at)


def assigned_sites():
    """Every dropout site number the package's code assigns, for a handful of module instances k."""
    from m2_mixer_amd import _lib as L
    ks = (0, 1, 2, 3, 7)
    sites = set()
    for base in (0, 1024, 2048):                                           # engine.py: _make_tower(..., 0 | 1024 | 2048) (two-tower
        sites |= {base + s for s in range(4 * L.MAX_BLOCKS)}               #   engines' _build; MimicEngine._build: 0 and 2048)
    sites |= {4096 + l for l in range(L.MLP_MAX_LAYERS)}                   # engine.py: MlpRuntime(..., self.p_drop, 4096)
    for k in ks:
        for chunk in (0, 1):                                               # modules/mixer.py: _site_base = 1024 * next(_site_counter);
            base = 1024 * k + 4 * L.MAX_BLOCKS * chunk                     #   _runtime: _site_base + 4 * L.MAX_BLOCKS * ci
            sites |= {base + s for s in range(4 * L.MAX_BLOCKS)}
        sites |= {(1 << 20 | 16 * k) + l for l in range(L.MLP_MAX_LAYERS)}   # modules/mlp.py: _site_base = 1 << 20 | (16 * next(..))
    return sorted(sites)


def test_no_two_step_site_pairs_share_a_key():
    """For one seed, the keys of every assigned site over steps 0 .. 19999 are all distinct (mix32 is a bijection, so this is a
    property of step * 0x9E3779B9 + site * 0x85EBCA77 modulo 2^32 on the sites in use): two sites, or a site at two steps, never
    draw the same stream."""
    sites = assigned_sites()
    assert len(sites) == 3 * 32 + 4 + (10 - 3) * 32 + 5 * 4   # (the modules' k = 0, 1, 2, chunk 0, are the engines' bases)
    steps = np.arange(20000, dtype=np.uint32)
    for seed in (123,):
        keys = D.site_key(seed, steps[:, None], np.array(sites, dtype=np.uint32)[None, :]).reshape(-1)
        assert keys.size == 20000 * len(sites)
        assert np.unique(keys).size == keys.size
