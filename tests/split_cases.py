"""The column-split tower path (csrc/split.h): one plain table of cases, and a Python restatement of the host rules that decide
whether a call takes the path, how many column splits it uses and how its rows and columns fall onto workgroups.

tests/test_host_split_cases.py classifies every case with these rules, checks that the table as a whole reaches each decision,
and shows on the CPU that the GPU test's bars see one lost 32-column unit; tests/test_gpu_split_envelope.py runs every case
against the float64 oracle and compares the restated rules with the library's own answer (m2m_split_form).

Restated from csrc/split_api.hip (split_count, m2m_split_eligible, m2m_split_can_group, the row space of chain_tower),
csrc/split_chain.hip (the unit range and chunk count of a split, the row tiles) and csrc/dispatch.h (m2m_fused_class).
All cases are bf16 and hidden_dim 128: the path takes nothing else.
"""
from collections import namedtuple

from shape_cases import Case

BM = 16                 # rows of a mix workgroup's tile (whole samples)
SP_ROWS = 128           # rows of a chain workgroup
SP_UNIT = 32            # hidden columns of one unit
SP_MAX_SPLITS = 8
SP_MAX_UNITS_PER_SPLIT = 64
MAX_BLOCKS = 8
NSPLIT = 8              # slabs TowerRuntime.ensure_split allocates


# ---- the host rules ---------------------------------------------------------------------------------------------------
def padC(C):
    return (C + 31) // 32 * 32


def nunits(C):
    return padC(C) // SP_UNIT


def split_count(C, nsplit=NSPLIT):
    """split_count: at most 8 splits, at least two 32-column units per split."""
    s = min(nsplit, SP_MAX_SPLITS)
    while s > 1 and nunits(C) // s < 2:
        s -= 1
    return s


def unit_ranges(C, S):
    """[(u0, u1)] of every split: split_chain.hip's u0 = s nunits / S, u1 = (s + 1) nunits / S."""
    n = nunits(C)
    return [(s * n // S, (s + 1) * n // S) for s in range(S)]


def chunks(u0, u1):
    """nch: two units per LDS chunk; an odd count ends in a half chunk."""
    return (u1 - u0 + 1) >> 1


def fused_class(N, T):
    """m2m_fused_class: (NMAX, TG) of the mix kernels."""
    if N <= 4:
        return (4, 8)
    return (8, 16) if T % 16 == 0 else (8, 8)


def spw(N):
    return BM // N


def mix_tiles(B, N):
    return (B + spw(N) - 1) // spw(N)


def image_rows(B, N):
    """Rows of the operand images and slabs: 16 per mix tile (= B N only where N divides 16 and 16 divides B N)."""
    return mix_tiles(B, N) * BM


def chain_row_tiles(B, N):
    return (image_rows(B, N) + SP_ROWS - 1) // SP_ROWS


def drop_mode(p):
    return "none" if p == 0 else ("half" if p == 0.5 else "gen")


def eligible(prec, D, N, C, nb, mode=1, B=1, min_rows=1 << 30):
    """m2m_split_eligible with the buffers of TowerRuntime.ensure_split; mode = M2M_SPLIT (-1: unset)."""
    if mode == 0 or prec != "bf16" or D != 128 or N > 8 or nb < 1:
        return False
    S = split_count(C)
    if S < 2 or (nunits(C) + S - 1) // S > SP_MAX_UNITS_PER_SPLIT:
        return False
    return True if mode == 1 else B * N >= min_rows


def can_group(a, b):
    """m2m_split_can_group of two (N, C, nb, p) towers."""
    return a.p == b.p and (a.N <= 4) == (b.N <= 4) and a.nb == b.nb and split_count(a.C) == split_count(b.C)


def split_form(a, b=None, prec="bf16", **kw):
    """m2m_split_form: the split count of the call, 0 for the fused / wide launch."""
    if not eligible(prec, a.D, a.N, a.C, a.nb, B=a.B, **kw):
        return 0
    if b is not None and (not eligible(prec, b.D, b.N, b.C, b.nb, B=b.B, **kw) or not can_group(a, b)):
        return 0
    return split_count(a.C)


# ---- single towers through the module path (MixerBlock: one block, no final LayerNorm; FusionMixer: final LayerNorm) ----------
def _c(name, kind, N, T, C, nb, B, p, D=128):
    return Case(name, kind, D, N, T, C, nb, B, p, None, None)


CASES = [
    # name              N  T   C   blocks B    p        units -> S: units per split; rows; what else the case forces
    _c("u4_s2", "block", 4, 32, 128, 1, 3, 0.0),        # 4 -> 2: 2,2 (nch 1 everywhere); 12 rows; NMAX 4
    _c("u5_s2_odd", "fusion", 3, 24, 130, 2, 7, 0.5),   # 5 -> 2: 2,3 (odd final split); 21 rows, 15 of 16 per tile; C % 32 != 0
    _c("u7_s3", "block", 5, 16, 200, 1, 26, 0.1),       # 7 -> 3: 2,2,3; 130 rows in 9 tiles of 15: a second chain row tile; NMAX 8 TG 16
    _c("u9_s4", "fusion", 7, 24, 288, 2, 19, 0.5),      # 9 -> 4: 2,2,2,3; 133 rows, 14 of 16; last mix tile one sample; NMAX 8 TG 8
    _c("u10_s5", "fusion", 4, 8, 320, 1, 5, 0.1),       # 10 -> 5: 2 each; token_dim 8 (zero-padded token MLP); final LayerNorm on one block
    _c("u13_s6", "block", 8, 32, 416, 1, 16, 0.0),      # 13 -> 6: 2,2,2,2,2,3; exactly 128 rows
    _c("u15_s7", "fusion", 2, 16, 480, 1, 9, 0.5),      # 15 -> 7: 2,2,2,2,2,2,3; 18 rows in 2 tiles
    _c("u16_s8", "block", 1, 8, 512, 1, 129, 0.1),      # 16 -> 8: 2 each (nch 1); 129 rows: 9 mix tiles, the last with one sample
    _c("u17_s8_x8", "fusion", 2, 16, 544, 8, 9, 0.5),   # 17 -> 8: ...,3; 8 blocks: the reduction's tables exactly full
    _c("u23_s8", "block", 6, 8, 736, 1, 11, 0.0),       # 23 -> 8: 2,3,3,3,3,3,3,3 (odd NON-final splits); 66 rows, 12 of 16
    _c("u512_s8_edge", "block", 4, 32, 16384, 1, 2, 0.5),   # 512 -> 8: 64 each = SP_MAX_UNITS_PER_SPLIT (the LDS bias stage full)
]
EXPECT_S = {"u4_s2": 2, "u5_s2_odd": 2, "u7_s3": 3, "u9_s4": 4, "u10_s5": 5, "u13_s6": 6, "u15_s7": 7, "u16_s8": 8,
            "u17_s8_x8": 8, "u23_s8": 8, "u512_s8_edge": 8}
# one unit of 512 cannot show at any bar: the case is there for the upper bound of the path, not for sharpness
INSENSITIVE = {"u512_s8_edge"}

# ---- shapes that must NOT take the path (m2m_split_form == 0 under M2M_SPLIT=1) ------------------------------------------------
# (name, precision, Case, the fused launch it falls back to refuses it)
REFUSED = [
    ("c64_two_units", "bf16", _c("c64", "block", 4, 16, 64, 1, 3, 0.0), False),           # S would be 1
    ("c96_three_units", "bf16", _c("c96", "block", 4, 16, 96, 1, 3, 0.0), False),         # S would be 1
    ("c16385_65_per_split", "bf16", _c("c16385", "block", 4, 16, 16385, 1, 2, 0.0), True),  # 513 units: 65 per split; fused: Cp > 4096
    ("fp32", "fp32", _c("fp32", "block", 4, 16, 128, 1, 3, 0.0), False),
    ("d64", "bf16", _c("d64", "block", 4, 16, 128, 1, 3, 0.0, D=64), False),
    ("n9_wide", "bf16", _c("n9", "block", 9, 16, 128, 1, 3, 0.0), False),
]

# ---- pairs through runtime.towers_forward / towers_backward ------------------------------------------------------------------
Tow = namedtuple("Tow", "D N T C nb B p")


def _t(N, T, C, nb, B, p):
    return Tow(128, N, T, C, nb, B, p)


# x0_parts: tower 0's input is given as two k-split parts; pooled: tower 1 is read out through pooled / d_pooled
PAIR_UNEQUAL = (_t(2, 16, 130, 2, 40, 0.5), _t(4, 32, 128, 2, 40, 0.5))     # 5 and 4 units, both S = 2; 80 and 160 rows: 1 and 2 row tiles
PAIR_NOT_GROUPABLE = {
    "token_class": (_t(4, 16, 128, 1, 6, 0.0), _t(8, 16, 128, 1, 6, 0.0)),      # NMAX 4 beside NMAX 8
    "split_count": (_t(4, 16, 128, 1, 6, 0.0), _t(4, 16, 512, 1, 6, 0.0)),      # S = 2 beside S = 8
    "depth": (_t(4, 16, 128, 1, 6, 0.0), _t(4, 16, 128, 2, 6, 0.0)),            # 1 block beside 2
}
PAIR_MIXED = (_t(4, 16, 128, 1, 6, 0.0), _t(4, 16, 96, 1, 6, 0.0))            # eligible beside C = 96 (S would be 1)


# ---- what the GPU test measures per 32-channel unit ------------------------------------------------------------------------
def unit_slices(key, t):
    """The 32-channel units of a channel-mixing gradient (W1 (C, D) rows, b1 (C), W2 (D, C) columns), else []: a unit lost at
    any split boundary is then a tail of its own, measured against the slice's maximum."""
    if key.endswith("channel_mix.1.net.0.weight") or key.endswith("channel_mix.1.net.0.bias"):
        return [t[u:u + SP_UNIT] for u in range(0, t.shape[0], SP_UNIT)]
    if key.endswith("channel_mix.1.net.3.weight"):
        return [t[:, u:u + SP_UNIT] for u in range(0, t.shape[1], SP_UNIT)]
    return []
