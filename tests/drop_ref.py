"""Host replica of the library's dropout stream, in numpy uint32, written from its specification ("Dropout stream";
the comments of csrc/common.h and csrc/tile.h) and never by calling the library: an independent reference for the masks the
kernels and the mask probe draw.

  mix32(x)      x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16            (all modulo 2^32)
  key           mix32(seed ^ mix32(step * 0x9E3779B9 + site * 0x85EBCA77 + 0x1234567)), step = host step + device counter
  thr           (long)((1 - (double)(float)p) * 65536 + 0.5) clamped to [1, 65536]; kept values are scaled by 65536 / thr
  generic draw  element idx keeps iff the 16-bit half (idx & 1: low, high) of mix32(key ^ (idx >> 1)) is < thr
  one-bit draw  (thr == 32768, the tower's token sites and channel-hidden site) element (row, col) of a site with `ncols` columns
                keeps iff bit col & 31 of mix32(key ^ (row * nw + (col >> 5))) is set, nw words per row

Sites: a tower's block b has site_base + 4 b + {0 token hidden (B, D, T), 1 token out (B, D, N), 2 channel hidden (B N, Cp),
3 channel out (B N, D)}; hidden layer l of the plain MLP has site_base + l, elements (sample, unit)."""
from fractions import Fraction

import numpy as np

U32 = np.uint32
_M1, _M2 = U32(0x7FEB352D), U32(0x846CA68B)
_STEP_MUL, _SITE_MUL, _KEY_ADD = U32(0x9E3779B9), U32(0x85EBCA77), U32(0x1234567)


def u32(x) -> np.ndarray:
    """x modulo 2^32 as a uint32 array (at least 1-d: numpy's arrays wrap silently, its scalars warn)."""
    a = np.asarray(x)
    if a.dtype != U32:
        a = (a.astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(U32)
    return np.atleast_1d(a)


def mix32(x) -> np.ndarray:
    x = u32(x).copy()
    x ^= x >> U32(16)
    x *= _M1
    x ^= x >> U32(15)
    x *= _M2
    x ^= x >> U32(16)
    return x


def site_key(seed, step, site) -> np.ndarray:
    """Key of one dropout site at one step; the arguments broadcast."""
    return mix32(u32(seed) ^ mix32(u32(step) * _STEP_MUL + u32(site) * _SITE_MUL + _KEY_ADD))


def add_steps(step_host: int, step_dev: int = 0) -> int:
    """The step a launch draws with: the host argument plus the device counter, modulo 2^32."""
    return (int(step_host) + int(step_dev)) & 0xFFFFFFFF


def drop_thr(p) -> int:
    """The 16-bit keep threshold of dropout rate p (which reaches the library as a float32)."""
    keep = 1.0 - float(np.float32(p))
    t = int(keep * 65536.0 + 0.5)              # C's conversion to long truncates toward zero
    return min(max(t, 1), 65536)


def drop_thr_exact(p) -> int:
    """The same threshold in exact rational arithmetic: the integer part of (1 - p) 65536 + 1/2, clamped."""
    v = (1 - Fraction(float(np.float32(p)))) * 65536 + Fraction(1, 2)
    t = int(v)                                 # (truncation; v > 0 for every p <= 1)
    return min(max(t, 1), 65536)


def drop_scale(p) -> float:
    return 65536.0 / drop_thr(p)


def p_effective(p) -> float:
    """The dropout rate the kernels realise: 1 - thr / 65536."""
    return 1.0 - drop_thr(p) / 65536.0


def generic_mask(key, thr: int, n: int) -> np.ndarray:
    """Keep-mask (uint8) of elements 0 .. n - 1 under the generic 16-bit draw."""
    idx = u32(np.arange(n, dtype=np.uint64))
    w = mix32(u32(key) ^ (idx >> U32(1)))
    r = np.where((idx & U32(1)) != 0, w >> U32(16), w & U32(0xFFFF))
    return (r < U32(thr)).astype(np.uint8)   # (thr == 65536 keeps everything: a draw is at most 65535)


def bit_mask(key, nrows: int, ncols: int, nw: int) -> np.ndarray:
    """Keep-mask (uint8, row-major (nrows, ncols)) under the one-bit draw with nw hash words per row."""
    i = np.arange(nrows * ncols, dtype=np.uint64)
    row, col = u32(i // ncols), u32(i % ncols)
    w = mix32(u32(key) ^ (row * U32(nw) + (col >> U32(5))))
    return ((w >> (col & U32(31))) & U32(1)).astype(np.uint8)


def tower_site_shape(site: int, B: int, N: int, D: int, T: int, Cp: int):
    return {0: (B * D, T), 1: (B * D, N), 2: (B * N, Cp), 3: (B * N, D)}[site]


def tower_mask(seed, step, site_base, blk: int, site: int, p, B: int, N: int, D: int, T: int, Cp: int) -> np.ndarray:
    """Keep-mask (flat uint8) of site `site` of block `blk` in the mask probe's element order."""
    key = site_key(seed, step, add_steps(site_base, 4 * blk + site))
    thr = drop_thr(p)
    rows, cols = tower_site_shape(site, B, N, D, T, Cp)
    if thr == 32768 and site in (0, 1):
        return bit_mask(key, rows, cols, (cols + 31) // 32)
    if thr == 32768 and site == 2:
        return bit_mask(key, rows, cols, Cp >> 5)
    return generic_mask(key, thr, rows * cols)


def mlp_mask(seed, step, site_base, layer: int, p, B: int, dout: int) -> np.ndarray:
    """Keep-mask (uint8, (B, dout)) of hidden layer `layer` of the plain MLP."""
    key = site_key(seed, step, add_steps(site_base, layer))
    return generic_mask(key, drop_thr(p), B * dout).reshape(B, dout)
